"""CPU: hexl_ks_set_keys_device / hexl_ks_gen_keys are exported, sit in the ctypes table with their wrappers, carry the same constants
in the header and in Python, and refuse a null plan or pointer whatever the other arguments are (the refusals come before anything
touches a device). The layout arithmetic the host and the kernels share (hexl-fpga_amd/csrc/key_layout.hpp) is replayed on the host
against Geom::idxB's definition -- tests/cpp/key_layout_selftest.cpp, compiled here; the program is stand-alone."""
import ctypes
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "hexl_mi355x.h").read_text()
BADARG = -1


def test_symbols_table_and_wrappers(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name, n_args in (("hexl_ks_set_keys_device", 2), ("hexl_ks_gen_keys", 8)):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in hx.C_ABI and len(hx.C_ABI[name]) == n_args
        assert re.search(rf"^int\s+{name}\s*\(", HEADER, flags=re.M), f"{name} is not declared in the header"
    for wrapper in ("set_keys_device", "gen_keys", "gen_relin_keys", "gen_galois_keys"):
        assert callable(getattr(hx.KeySwitchPlan, wrapper))


def test_constants_agree():
    for name, value in (("POLY", 0), ("SQUARE", 1), ("GALOIS", 2)):
        m = re.search(rf"^#define\s+HEXL_KEY_FROM_{name}\s+(\d+)", HEADER, flags=re.M)
        assert m and int(m.group(1)) == value, name
    import hexl_fpga_amd as hx
    assert (hx.KEY_FROM_POLY, hx.KEY_FROM_SQUARE, hx.KEY_FROM_GALOIS) == (0, 1, 2)


def test_the_header_points_to_the_new_calls():
    assert "is not offered" not in HEADER
    assert "hexl_ks_set_keys_device (below)" in HEADER
    warning = HEADER[HEADER.index("MUST NEVER BE USED TWICE"):HEADER.index("The streams (normative")]
    assert "hexl_ks_gen_keys" in warning, "the never-reuse warning names the call that consumes polynomials"


def test_null_refusals_need_no_device(hx):
    lib = hx.lib()
    buf = (ctypes.c_uint64 * 8)()
    seed = (ctypes.c_uint32 * 8)()
    p = ctypes.addressof(buf)
    assert lib.hexl_ks_set_keys_device(None, p) == BADARG
    assert lib.hexl_ks_set_keys_device(None, None) == BADARG
    for kind in (0, 1, 2, 3, -1):
        for g in (1, 5, 2, 1 << 40):
            for first in (0, 1 << 40, (1 << 64) - 1):
                assert lib.hexl_ks_gen_keys(None, p, kind, g, p, seed, 0, first) == BADARG
                assert lib.hexl_ks_gen_keys(None, None, kind, g, None, None, 0, first) == BADARG


def test_key_layout_host_replay(tmp_path):
    exe = tmp_path / "key_layout_selftest"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "key_layout_selftest.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.startswith("ok ")
