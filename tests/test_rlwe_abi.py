"""CPU: hexl_sample / hexl_rlwe_encrypt / hexl_rlwe_decrypt exist in the built library and in the ctypes table, and refuse null handles
and pointers whatever `count` is -- the part of the refusal matrix that needs no device (tests/test_gpu_rlwe.py has the rest)."""
import ctypes

import pytest

HEXL_E_BADARG = -1
NEW = ("hexl_sample", "hexl_rlwe_encrypt", "hexl_rlwe_decrypt")


@pytest.fixture(scope="module")
def lib(hx):
    hx.build()
    so = ctypes.CDLL(str(hx.LIB_PATH))
    for name in NEW:
        assert name in hx.C_ABI, f"{name} missing from the ctypes table"
        assert hasattr(so, name), f"{name} not exported by {hx.LIB_PATH.name}"
        fn = getattr(so, name)
        fn.argtypes = hx.C_ABI[name]
        fn.restype = ctypes.c_int
    return so


def test_rlwe_ctypes_table_and_wrappers(hx, lib):
    assert len(hx.C_ABI["hexl_sample"]) == 8 and hx.C_ABI["hexl_sample"][2] is ctypes.c_int
    assert len(hx.C_ABI["hexl_rlwe_encrypt"]) == 10 and len(hx.C_ABI["hexl_rlwe_decrypt"]) == 7
    for name in NEW:
        assert hasattr(hx.KeySwitchPlan, name[len("hexl_"):]), f"KeySwitchPlan.{name[len('hexl_'):]} missing"
    assert (hx.SAMPLE_UNIFORM, hx.SAMPLE_TERNARY, hx.SAMPLE_CBD21) == (1, 2, 3)
    header = (hx.ROOT / "include" / "hexl_mi355x.h").read_text()
    for name, v in (("UNIFORM", 1), ("TERNARY", 2), ("CBD21", 3)):
        assert f"#define HEXL_SAMPLE_{name}" in header and header.split(f"#define HEXL_SAMPLE_{name}")[1].split()[0] == str(v)
    assert "MUST NEVER BE USED TWICE WITH ONE SECRET" in header


def test_seed_words(hx):
    words, raw = hx.seed_words(bytes(range(32)))
    assert list(words) == [int.from_bytes(bytes(range(4 * k, 4 * k + 4)), "little") for k in range(8)] and raw == bytes(range(32))
    words, raw = hx.seed_words([1, 2, 3, 4, 5, 6, 7, 0xFFFFFFFF])
    assert list(words) == [1, 2, 3, 4, 5, 6, 7, 0xFFFFFFFF] and len(raw) == 32
    a, b = hx.seed_words()[1], hx.seed_words(None)[1]
    assert len(a) == 32 and a != b                                 # fresh bytes from the operating system each time
    for bad in (bytes(31), bytes(33), [1, 2, 3]):
        with pytest.raises(ValueError):
            hx.seed_words(bad)


def test_rlwe_entry_points_refuse_null_handles_and_pointers(lib):
    buf = (ctypes.c_uint64 * 64)()
    a, b, c = (ctypes.addressof(buf) + 8 * 16 * k for k in range(3))
    seed = (ctypes.c_uint32 * 8)(*range(8))
    for count in (1, 0):
        for kind in (1, 2, 3):
            assert lib.hexl_sample(None, a, kind, seed, 0, 0, count, 1) == HEXL_E_BADARG                # no plan
            assert lib.hexl_sample(None, None, kind, seed, 0, 0, count, 1) == HEXL_E_BADARG             # no output
            assert lib.hexl_sample(None, a, kind, None, 0, 0, count, 1) == HEXL_E_BADARG                # no seed
        assert lib.hexl_sample(None, a, 0, seed, 0, 0, count, 1) == HEXL_E_BADARG                       # unknown kinds
        assert lib.hexl_sample(None, a, 4, seed, 0, 0, count, 1) == HEXL_E_BADARG
        assert lib.hexl_sample(None, a, 1, seed, 0, 1 << 40, count + 1, 1) == HEXL_E_BADARG
        for pt, pt_batch in ((None, 1), (b, 1), (b, count), (b, 5)):
            assert lib.hexl_rlwe_encrypt(None, a, pt, pt_batch, c, seed, 0, 0, count, 1) == HEXL_E_BADARG
            assert lib.hexl_rlwe_encrypt(None, None, pt, pt_batch, c, seed, 0, 0, count, 1) == HEXL_E_BADARG
            assert lib.hexl_rlwe_encrypt(None, a, pt, pt_batch, None, seed, 0, 0, count, 1) == HEXL_E_BADARG   # no secret
            assert lib.hexl_rlwe_encrypt(None, a, pt, pt_batch, c, None, 0, 0, count, 1) == HEXL_E_BADARG      # no seed
        for ncomp in (2, 3, 1, 4, 0):
            assert lib.hexl_rlwe_decrypt(None, a, b, c, count, ncomp, 1) == HEXL_E_BADARG
            assert lib.hexl_rlwe_decrypt(None, None, b, c, count, ncomp, 1) == HEXL_E_BADARG
            assert lib.hexl_rlwe_decrypt(None, a, None, c, count, ncomp, 1) == HEXL_E_BADARG
            assert lib.hexl_rlwe_decrypt(None, a, b, None, count, ncomp, 1) == HEXL_E_BADARG
    assert lib.hexl_sample(None, None, 0, None, 0, 0, 0, 0) == HEXL_E_BADARG
    assert lib.hexl_rlwe_encrypt(None, None, None, 0, None, None, 0, 0, 0, 0) == HEXL_E_BADARG
    assert lib.hexl_rlwe_decrypt(None, None, None, None, 0, 0, 0) == HEXL_E_BADARG
