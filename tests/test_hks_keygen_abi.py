"""CPU: hexl_hks_keygen and hexl_hks_export_keys exist in the header, in the built library and in the ctypes table with their arities,
the Python wrappers are there with their signatures, every argument combination that can be refused without a device returns
HEXL_E_BADARG and writes nothing, and the header carries the extended WARNING and the normative sentence."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1
ARITY = {"hexl_hks_keygen": 9, "hexl_hks_export_keys": 2}


def test_entry_points_are_declared_exported_and_bound(hx):
    header = (ROOT / "include" / "hexl_mi355x.h").read_text()
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name, arity in ARITY.items():
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M)
        assert decl, f"{name} is not declared in include/hexl_mi355x.h"
        assert len(decl.group(1).split(",")) == arity, name
        assert name in hx.C_ABI and len(hx.C_ABI[name]) == arity, name
        assert hasattr(lib, name), f"{name} not exported by {hx.LIB_PATH.name}"
    assert re.search(r"^#define HEXL_HKS_KEYGEN_MAX_KEYS 64$", header, flags=re.M)
    # the knob tests/test_gpu_hks_keygen.py sets in its child process is the one the launcher reads
    assert 'hx_knob("HEXL_HKS_KEYGEN_CHUNK", 0)' in (ROOT / "hexl-fpga_amd" / "csrc" / "keygen.hip").read_text()


def test_the_header_states_the_contract():
    header = (ROOT / "include" / "hexl_mi355x.h").read_text()
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for text in ("hexl_hks_keygen (further below) is such a call as well: it consumes the UNIFORM and CBD21 polynomials first ... first + sum_r dnum_r - 1",
                 "afterwards object r is word for word what hexl_hks_set_keys_device leaves for the output of the Python wrapper",
                 "first_r = first + sum of dnum_r' over r' < r",
                 "a refused call leaves every object as it was",
                 "n_keys <= HEXL_HKS_KEYGEN_MAX_KEYS = 64",
                 "first + sum_r dnum_r > 2^40",
                 "gives X mod q exactly"):
        assert text in flat, text
    assert header.index("MUST NEVER BE USED TWICE") < header.index("hexl_hks_keygen (further below)") < header.index("The streams (normative")


def test_wrappers_exist(hx):
    gen = inspect.signature(hx.hks_keygen)
    assert list(gen.parameters) == ["hks_list", "secret", "from_kinds", "galois_elts", "from_polys", "seed", "stream", "first"]
    assert gen.parameters["galois_elts"].default is None and gen.parameters["from_polys"].default is None
    assert gen.parameters["seed"].default is None and gen.parameters["stream"].default == 0 and gen.parameters["first"].default == 0
    assert "WARNING" in hx.hks_keygen.__doc__
    cls = hx.HybridKeySwitch
    assert list(inspect.signature(cls.gen_keys).parameters) == ["self", "secret", "from_kind", "galois_elt", "from_poly", "seed", "stream", "first"]
    assert list(inspect.signature(cls.gen_relin_keys).parameters) == ["self", "secret", "seed", "stream", "first"]
    assert list(inspect.signature(cls.gen_galois_keys).parameters) == ["self", "secret", "g", "seed", "stream", "first"]
    assert list(inspect.signature(cls.export_keys).parameters) == ["self", "out"]
    assert "hks_keygen" in hx.__all__
    # the wrapper that defines the new call's words stays as it is, and stays a wrapper
    assert "hexl_gen_hybrid_key" not in hx.C_ABI and "hexl_hks_gen_keys" not in hx.C_ABI


def test_what_needs_no_device_is_refused_and_nothing_is_written(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    for name in ARITY:
        getattr(lib, name).argtypes = hx.C_ABI[name]
        getattr(lib, name).restype = ctypes.c_int
    buf = (ctypes.c_uint64 * 64)()
    secret = ctypes.addressof(buf)
    seed = (ctypes.c_uint32 * 8)(*range(1, 9))
    objs = (ctypes.c_void_p * 2)(None, None)                      # an array of null objects: refused at its first entry
    kinds = (ctypes.c_int * 2)(1, 1)
    elts = (ctypes.c_uint64 * 2)(5, 5)
    froms = (ctypes.c_void_p * 2)(None, None)
    for n_keys in (1, 2, 0, 65):
        assert lib.hexl_hks_keygen(None, n_keys, kinds, elts, froms, secret, seed, 0, 0) == HEXL_E_BADARG
        assert lib.hexl_hks_keygen(objs, n_keys, None, elts, froms, secret, seed, 0, 0) == HEXL_E_BADARG
        assert lib.hexl_hks_keygen(objs, n_keys, kinds, elts, froms, None, seed, 0, 0) == HEXL_E_BADARG
        assert lib.hexl_hks_keygen(objs, n_keys, kinds, elts, froms, secret, None, 0, 0) == HEXL_E_BADARG
        assert lib.hexl_hks_keygen(objs, n_keys, kinds, None, None, secret, seed, 0, 0) == HEXL_E_BADARG
    assert lib.hexl_hks_keygen(None, 0, None, None, None, None, None, 0, 0) == HEXL_E_BADARG
    assert lib.hexl_hks_export_keys(None, secret) == HEXL_E_BADARG
    assert lib.hexl_hks_export_keys(None, None) == HEXL_E_BADARG
    assert not any(buf), "a refused call wrote"
    assert list(seed) == list(range(1, 9)) and list(kinds) == [1, 1] and list(elts) == [5, 5]
