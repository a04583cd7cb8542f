"""CPU: hexl_pk_encrypt exists in the header, in the built library and in the ctypes table with its eleven arguments, the Python
wrappers are there, and the entry point refuses null handles and pointers (count == 0 does not excuse them) without a device."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG = -1


def test_pk_encrypt_is_declared_exported_and_bound(hx):
    header = (ROOT / "include" / "hexl_mi355x.h").read_text()
    decl = re.search(r"^int\s+hexl_pk_encrypt\s*\(([^;]*)\);", header, flags=re.M)
    assert decl, "hexl_pk_encrypt is not declared in include/hexl_mi355x.h"
    assert len(decl.group(1).split(",")) == 11
    assert "hexl_pk_encrypt" in hx.C_ABI and len(hx.C_ABI["hexl_pk_encrypt"]) == 11
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    assert hasattr(lib, "hexl_pk_encrypt"), f"hexl_pk_encrypt not exported by {hx.LIB_PATH.name}"
    # the WARNING paragraph names the indices the call consumes
    assert "2c + 1" in header and "hexl_pk_encrypt is another" in header


def test_wrappers_exist(hx):
    pk = inspect.signature(hx.KeySwitchPlan.pk_encrypt)
    assert list(pk.parameters) == ["self", "out", "pk", "count", "n_limbs", "pk_limbs", "pt", "pt_batch", "seed", "stream", "first"]
    assert pk.parameters["pk_limbs"].default is None and pk.parameters["pt"].default is None and pk.parameters["pt_batch"].default == 1
    assert pk.parameters["stream"].default == 0 and pk.parameters["first"].default == 0
    gen = inspect.signature(hx.KeySwitchPlan.gen_public_key)
    assert list(gen.parameters) == ["self", "out", "secret", "n_limbs", "seed", "stream", "first"]
    assert gen.parameters["n_limbs"].default is None
    assert "hexl_gen_public_key" not in hx.C_ABI                 # a wrapper over rlwe_encrypt, not a C entry point


def test_pk_encrypt_refuses_null_handles_and_pointers(hx):
    hx.build()
    lib = ctypes.CDLL(str(hx.LIB_PATH))
    fn = lib.hexl_pk_encrypt
    fn.argtypes = hx.C_ABI["hexl_pk_encrypt"]
    fn.restype = ctypes.c_int
    buf = (ctypes.c_uint64 * 64)()
    out, pk, pt = (ctypes.addressof(buf) + 8 * 16 * k for k in range(3))
    seed = (ctypes.c_uint32 * 8)(*range(8))
    assert fn(None, out, pt, 1, pk, 1, seed, 0, 0, 1, 1) == HEXL_E_BADARG             # no plan
    assert fn(None, out, None, 1, pk, 1, seed, 0, 0, 1, 1) == HEXL_E_BADARG
    assert fn(None, out, None, 1, pk, 1, seed, 0, 0, 0, 1) == HEXL_E_BADARG           # count == 0 does not excuse it
    assert fn(None, None, None, 1, None, 1, None, 0, 0, 0, 1) == HEXL_E_BADARG
    assert fn(None, None, None, 0, pk, 1, seed, 0, 0, 0, 1) == HEXL_E_BADARG          # no output
    assert fn(None, out, None, 0, None, 1, seed, 0, 0, 0, 1) == HEXL_E_BADARG         # no key
    assert fn(None, out, None, 0, pk, 1, None, 0, 0, 0, 1) == HEXL_E_BADARG           # no seed
    assert not any(buf), "a refused call wrote"
