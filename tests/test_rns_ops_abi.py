"""CPU: hexl_rns_ntt_fwd / hexl_rns_ntt_inv / hexl_multiply_plain exist in the built library and in the ctypes table and refuse what
they cannot run on, and the plaintext multiply's scalar chains (f64_arith.hpp pt_mul / pt_mul_acc) agree with 128-bit integers on the
host (tests/cpp/pt_mul_selftest.cpp, compiled here)."""
import ctypes
import subprocess
from pathlib import Path

from ks_util import primes_below, primes_from

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
NEW = ("hexl_rns_ntt_fwd", "hexl_rns_ntt_inv", "hexl_multiply_plain")


def test_rns_entry_points_refuse_null_handles_and_pointers(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name in NEW:
        assert name in hx.C_ABI, f"{name} missing from the ctypes table"
        assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
        fn = getattr(lib, name)
        fn.argtypes = hx.C_ABI[name]
        fn.restype = ctypes.c_int
    buf = (ctypes.c_uint64 * 24)()
    a, b, c = (ctypes.addressof(buf) + 8 * 8 * k for k in range(3))
    for fn in (lib.hexl_rns_ntt_fwd, lib.hexl_rns_ntt_inv):
        assert fn(None, a, b, 1, 1) == HEXL_E_BADARG              # no plan
        assert fn(None, None, None, 0, 1) == HEXL_E_BADARG        # count == 0 does not excuse null pointers
        assert fn(None, a, a, 0, 1) == HEXL_E_BADARG
    assert lib.hexl_multiply_plain(None, a, b, c, 1, 2, 1, 1, 0) == HEXL_E_BADARG
    assert lib.hexl_multiply_plain(None, a, b, c, 1, 2, 1, 1, 1) == HEXL_E_BADARG
    assert lib.hexl_multiply_plain(None, None, None, None, 0, 2, 1, 1, 0) == HEXL_E_BADARG
    assert lib.hexl_multiply_plain(None, a, b, None, 0, 2, 1, 1, 0) == HEXL_E_BADARG


def selftest_moduli(orc):
    """the eleven moduli of f64_selftest.cpp's rescale replay: the largest primes = 1 mod 2^15 below 2^27, 2^30, 2^40, 2^49, 2^50, 2^51 and
    2^52, the bench's first 51-bit prime, the second-largest below 2^52, and both sides of the lazy / strict boundary 2^51 (1 + 2^-7)"""
    n = 16384
    below = lambda limit: primes_below(orc, 1, limit, n)[0]
    rs = [below(1 << b) for b in (27, 30, 40, 49, 50, 51, 52)]
    boundary = (1 << 51) + (1 << 44) + 1
    rs += [orc.primes(8, 51, n)[0], below(rs[6]), below(boundary), primes_from(orc, 1, boundary, n)[0]]
    assert len(set(rs)) == 11 and min(rs) < 1 << 27 and (1 << 52) - (1 << 20) < max(rs) < 1 << 52
    return rs


def test_pt_mul_host_replay(orc, tmp_path):
    exe = tmp_path / "pt_mul_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "pt_mul_selftest.cpp")], check=True)
    out = subprocess.run([str(exe), "4000"] + [str(q) for q in selftest_moduli(orc)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL PASSED" in out.stdout
