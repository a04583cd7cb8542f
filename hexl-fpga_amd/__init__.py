"""hexl-fpga_amd -- MI355X-native FHE primitives behind the hexl-fpga interface.

Python side of the package: a thin ctypes binding over the C-ABI of
``include/hexl_mi355x.h`` (``lib/libhexl_mi355x.so``, hand-written HIP for gfx950) plus
``HexlFpga``, a host-side mirror of the reference's public API
(``host/inc/hexl-fpga.h:15-161``: ``set_worksize_X / X / XCompleted``) used by the parity
tests so they read like the reference's own gtests.

torch is plumbing only: device buffers, streams and ``torch.distributed``. All arithmetic
happens in the HIP kernels; there is NO CPU fallback -- if the extension is missing or no
gfx950 device is visible every entry point raises.

The directory name contains a hyphen (it mirrors the reference's project name), so import
it through the repo-root shim: ``import hexl_fpga_amd``.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
ROOT = _PKG.parent
# HEXL_MI355X_LIB: another build of the same library (tools/build_variant.sh: kernel experiments side by side on one box)
LIB_PATH = Path(os.environ["HEXL_MI355X_LIB"]) if os.environ.get("HEXL_MI355X_LIB") else _PKG / "lib" / "libhexl_mi355x.so"

_u64 = ctypes.c_uint64
_sz = ctypes.c_size_t
_vp = ctypes.c_void_p
_i = ctypes.c_int

# symbol -> argtypes; every function returns int status. Mirrors include/hexl_mi355x.h 1:1
# (tests/test_abi.py checks the header and this table against the built library).
C_ABI = {
    "hexl_device_count": [],
    "hexl_ctx_create": [_i, ctypes.POINTER(_vp)],
    "hexl_ctx_destroy": [_vp],
    "hexl_ctx_set_stream": [_vp, _vp],
    "hexl_ctx_use_own_stream": [_vp],
    "hexl_ctx_sync": [_vp],
    "hexl_ctx_describe": [_vp, ctypes.c_char_p, _sz],
    "hexl_ntt_fwd": [_vp, _vp, _sz, _vp, _vp, _u64, _u64],
    "hexl_ntt_inv": [_vp, _vp, _sz, _vp, _vp, _u64, _u64, _u64, _u64],
    "hexl_dyadic_multiply": [_vp, _vp, _vp, _vp, _sz, _u64, _vp, _u64],
    "hexl_ks_plan_create": [_vp, _u64, _u64, _u64, _u64, _u64, _vp, _vp, _vp, ctypes.POINTER(_vp)],
    "hexl_ks_plan_destroy": [_vp],
    "hexl_ks_set_keys": [_vp, ctypes.POINTER(_vp)],
    "hexl_keyswitch": [_vp, _vp, _vp, _sz],
    "hexl_ks_range_check": [_vp],
    "hexl_ks_plan_tiers": [_vp, ctypes.POINTER(_i)],
    "hexl_multiply_relinearize": [_vp, _vp, _vp, _vp, _sz],
    "hexl_apply_galois": [_vp, _vp, _vp, _sz, _u64, _u64],
    "hexl_rescale": [_vp, _vp, _vp, _sz, _u64, _u64],
    "hexl_rotate": [_vp, _vp, _vp, _sz, _u64],
    "hexl_rotate_hoisted": [ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz, ctypes.POINTER(_vp), _vp, _sz],
    "hexl_linear_transform": [ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_vp), _sz, _vp, _vp, _vp, _sz],
    "hexl_linear_transform_bsgs": [ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz, ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz,
                                   ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _sz],
    "hexl_lt_bsgs_scratch_bytes": [_vp, _sz, _sz],
    "hexl_rns_ntt_fwd": [_vp, _vp, _vp, _sz, _u64],
    "hexl_rns_ntt_inv": [_vp, _vp, _vp, _sz, _u64],
    "hexl_multiply_plain": [_vp, _vp, _vp, _vp, _sz, _u64, _u64, _sz, _i],
    "hexl_ct_lincomb": [_vp, _vp, ctypes.POINTER(_vp), _vp, _vp, _sz, _vp, _sz, _vp, _sz, _u64, _u64],
    "hexl_ct_tensor_sum": [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _sz, _sz, _u64],
    "hexl_relinearize": [_vp, _vp, _vp, _sz],
    "hexl_multiply_sum_relinearize": [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _sz, _sz],
    "hexl_rns_from_f64": [_vp, _vp, _vp, _sz, _u64],
    "hexl_rns_to_f64": [_vp, _vp, _vp, _sz, _u64],
    "hexl_ckks_encode": [_vp, _vp, _vp, _sz, _u64, ctypes.c_double],
    "hexl_ckks_decode": [_vp, _vp, _vp, _sz, _u64, ctypes.c_double],
    "hexl_sample": [_vp, _vp, _i, _vp, _u64, _u64, _sz, _u64],
    "hexl_rlwe_encrypt": [_vp, _vp, _vp, _sz, _vp, _vp, _u64, _u64, _sz, _u64],
    "hexl_pk_encrypt": [_vp, _vp, _vp, _sz, _vp, _u64, _vp, _u64, _u64, _sz, _u64],
    "hexl_rlwe_decrypt": [_vp, _vp, _vp, _vp, _sz, _u64, _u64],
    "hexl_ks_set_keys_device": [_vp, _vp],
    "hexl_ks_gen_keys": [_vp, _vp, _i, _u64, _vp, _vp, _u64, _u64],
    "hexl_ks_scratch_bytes": [_vp, _sz],
    "hexl_hks_create": [_vp, _u64, ctypes.POINTER(_vp)],
    "hexl_hks_destroy": [_vp],
    "hexl_hks_set_keys_device": [_vp, _vp],
    "hexl_hks_keyswitch": [_vp, _vp, _vp, _sz, _u64],
    "hexl_hks_relinearize": [_vp, _vp, _vp, _sz, _u64],
    "hexl_hks_rotate": [_vp, _vp, _vp, _sz, _u64, _u64],
    "hexl_hks_scratch_bytes": [_vp, _sz],
    "hexl_hks_keygen": [ctypes.POINTER(_vp), _sz, ctypes.POINTER(_i), ctypes.POINTER(_u64), ctypes.POINTER(_vp), _vp, _vp, _u64, _u64],
    "hexl_hks_export_keys": [_vp, _vp],
    "hexl_hks_rotate_hoisted": [ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz, ctypes.POINTER(_vp), _vp, _sz, _u64],
    "hexl_hks_linear_transform": [ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_vp), _sz, _vp, _vp, _vp, _sz, _u64],
    "hexl_hks_hoisted_scratch_bytes": [_vp, _sz],
    "hexl_hks_linear_transform_bsgs": [ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz, ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz,
                                       ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _sz, _u64],
    "hexl_hks_bsgs_scratch_bytes": [_vp, _sz, _sz],
    "hexl_hks_linear_transform_bsgs_ext": [ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz, ctypes.POINTER(_vp), ctypes.POINTER(_u64), _sz,
                                           ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _sz, _u64, _i],
    "hexl_hks_bsgs_ext_scratch_bytes": [_vp, _sz, _sz, _i],
    "hexl_hks_multiply_sum_relinearize": [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _sz, _sz, _u64],
    "hexl_hks_relinearize_rescale": [_vp, _vp, _vp, _sz, _u64],
    "hexl_hks_multiply_sum_rescale": [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _sz, _sz, _u64],
    "hexl_hks_mul_scratch_bytes": [_vp, _sz],
    "hexl_ntt_fwd_host": [_vp, ctypes.POINTER(_vp), _sz, _vp, _vp, _u64, _u64],
    "hexl_ntt_inv_host": [_vp, ctypes.POINTER(_vp), _sz, _vp, _vp, _u64, _u64, _u64, _u64],
    "hexl_dyadic_multiply_host": [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _sz, _u64,
                                  ctypes.POINTER(_vp), _u64],
    "hexl_keyswitch_host": [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _sz],
    "hexl_ks_time_stages": [_vp, _vp, _vp, _sz, _i, ctypes.POINTER(ctypes.c_float)],
}


class HexlError(RuntimeError):
    pass


def build(force: bool = False) -> Path:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not LIB_PATH.exists():
        subprocess.run(["make", "-C", str(_PKG / "csrc"), "-j4"] + (["-B"] if force else []), check=True)
    else:
        # cheap staleness check: make decides
        subprocess.run(["make", "-C", str(_PKG / "csrc"), "-j4", "-s"], check=True)
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    """Load libhexl_mi355x.so; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise HexlError(f"{LIB_PATH} missing: run __graft_entry__.build() / make -C hexl-fpga_amd/csrc "
                            "(there is no CPU fallback)")
        # torch must load its HIP runtime first so this library binds to the SAME libamdhip64 instance
        # (device pointers from torch tensors are only meaningful inside one runtime).
        import torch  # noqa: F401
        _lib = ctypes.CDLL(str(LIB_PATH))
        for name, args in C_ABI.items():
            fn = getattr(_lib, name)
            fn.argtypes = args
            fn.restype = _sz if name in ("hexl_ks_scratch_bytes", "hexl_lt_bsgs_scratch_bytes", "hexl_hks_scratch_bytes",
                                      "hexl_hks_hoisted_scratch_bytes", "hexl_hks_bsgs_scratch_bytes", "hexl_hks_bsgs_ext_scratch_bytes",
                                      "hexl_hks_mul_scratch_bytes") else _i
    return _lib


SAMPLE_UNIFORM, SAMPLE_TERNARY, SAMPLE_CBD21 = 1, 2, 3            # include/hexl_mi355x.h HEXL_SAMPLE_*
KEY_FROM_POLY, KEY_FROM_SQUARE, KEY_FROM_GALOIS = 0, 1, 2         # include/hexl_mi355x.h HEXL_KEY_FROM_*


def seed_words(seed=None):
    """the 32-byte seed of hexl_sample / hexl_rlwe_encrypt as (ctypes uint32[8], the bytes): `seed` is 32 bytes, eight u32 words, or
    None for 32 fresh bytes from os.urandom -- keep the returned bytes if the stream has to be expanded again"""
    if seed is None:
        seed = os.urandom(32)
    if not isinstance(seed, (bytes, bytearray)):
        seed = np.asarray(seed, dtype="<u4").tobytes()
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes (eight little-endian u32 words)")
    return (ctypes.c_uint32 * 8)(*np.frombuffer(bytes(seed), dtype="<u4").tolist()), bytes(seed)


def _check(rc: int, what: str):
    if rc != 0:
        raise HexlError(f"{what} failed with status {rc}")


def _check_warn(rc: int, what: str) -> int:
    """the status of an entry point for which 1 (HEXL_W_RANGE; hexl_ks_plan_tiers: the limbs differ) is an answer, not an error"""
    if rc != 1:
        _check(rc, what)
    return rc


def _handles(plans):
    """ctypes array of plan handles, None entries as NULL"""
    return (_vp * len(plans))(*[None if p is None else p.h.value for p in plans])


def _u64_array(values):
    return (_u64 * len(values))(*[int(v) for v in values])


def ptr_array(arrays):
    """ctypes array of pointers to numpy arrays (host) or torch tensors (device), kept alive by the caller"""
    return (_vp * len(arrays))(*[_ptr(a) for a in arrays])


def _ptr(t) -> int:
    """device pointer of a torch tensor / host pointer of a numpy array"""
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


def as_i64(a: np.ndarray):
    """numpy uint64 -> torch int64 view (bit pattern preserved)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64))


def to_u64(t) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint64)


class Context:
    """One GPU: stream + scratch (hexl_ctx). Device-pointer launchers take torch int64 CUDA tensors."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        import torch
        if not torch.cuda.is_available():
            raise HexlError("no ROCm device visible: the HIP path is the only path")
        self.device = device
        h = _vp()
        _check(lib().hexl_ctx_create(device, ctypes.byref(h)), "hexl_ctx_create")
        self.h = h
        if use_torch_stream:
            with torch.cuda.device(device):
                self.set_stream(torch.cuda.current_stream().cuda_stream)

    def set_stream(self, raw_stream: int):
        _check(lib().hexl_ctx_set_stream(self.h, _vp(raw_stream)), "hexl_ctx_set_stream")

    def use_own_stream(self):
        """back to the context's own non-blocking stream; like set_stream, ordered behind what the previous stream holds"""
        _check(lib().hexl_ctx_use_own_stream(self.h), "hexl_ctx_use_own_stream")

    def sync(self):
        _check(lib().hexl_ctx_sync(self.h), "hexl_ctx_sync")

    def describe(self) -> str:
        buf = ctypes.create_string_buffer(256)
        _check(lib().hexl_ctx_describe(self.h, buf, 256), "hexl_ctx_describe")
        return buf.value.decode()

    def close(self):
        if getattr(self, "h", None):
            lib().hexl_ctx_destroy(self.h)
            self.h = None

    # ---- K1 / K2 / K3 on device tensors (in place / out of place as the reference) ----
    def ntt_fwd(self, x, roots, precon, q: int, n: int):
        batch = x.numel() // n
        _check(lib().hexl_ntt_fwd(self.h, _ptr(x), batch, _ptr(roots), _ptr(precon), q, n), "hexl_ntt_fwd")

    def ntt_inv(self, x, inv_roots, inv_precon, q: int, inv_n: int, inv_n_w: int, n: int):
        batch = x.numel() // n
        _check(lib().hexl_ntt_inv(self.h, _ptr(x), batch, _ptr(inv_roots), _ptr(inv_precon), q, inv_n, inv_n_w, n),
               "hexl_ntt_inv")

    def dyadic_multiply(self, out, a, b, moduli, n: int, n_moduli: int):
        batch = a.numel() // (2 * n_moduli * n)
        _check(lib().hexl_dyadic_multiply(self.h, _ptr(out), _ptr(a), _ptr(b), batch, n, _ptr(moduli), n_moduli),
               "hexl_dyadic_multiply")

    def apply_galois(self, out, inp, count: int, n: int, g: int):
        """out[count][n] = X -> X^g of inp[count][n] in NTT form (a word permutation; out must not overlap inp)"""
        _check(lib().hexl_apply_galois(self.h, _ptr(out), _ptr(inp), count, n, g), "hexl_apply_galois")


class KeySwitchPlan:
    """Device state for one keyswitch parameter set (hexl_ks_plan): tables, constants, keys."""

    def __init__(self, ctx: Context, n: int, L: int, K: int, rns: int, kcc: int, moduli, modswitch,
                 twiddles=None):
        self.ctx, self.n, self.L, self.K = ctx, n, L, K
        mod = np.ascontiguousarray(moduli, dtype=np.uint64)
        self.moduli = [int(q) for q in mod[:K]]
        msf = np.ascontiguousarray(modswitch, dtype=np.uint64)
        tw = None if twiddles is None else np.ascontiguousarray(twiddles, dtype=np.uint64)
        h = _vp()
        _check(lib().hexl_ks_plan_create(ctx.h, n, L, K, rns, kcc, mod.ctypes.data, msf.ctypes.data,
                                         None if tw is None else tw.ctypes.data, ctypes.byref(h)),
               "hexl_ks_plan_create")
        self.h = h

    def set_keys(self, keys):
        """keys: list of L numpy uint64 arrays, keys[d][(k*K + i)*n + j]"""
        self._keys = [np.ascontiguousarray(k, dtype=np.uint64) for k in keys]
        arr = (_vp * len(self._keys))(*[k.ctypes.data for k in self._keys])
        _check(lib().hexl_ks_set_keys(self.h, arr), "hexl_ks_set_keys")

    def set_keys_device(self, keys):
        """keys: device tensor [L][2][K][n] in the layout of set_keys (what a key-shaped rlwe_encrypt writes); one kernel on the context's
        stream lays it into every copy the plan holds -- no host synchronisation, and a plan in use may be re-keyed"""
        _check(lib().hexl_ks_set_keys_device(self.h, _ptr(keys)), "hexl_ks_set_keys_device")

    def gen_keys(self, secret, from_kind: int, galois_elt: int = 1, from_poly=None, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """the switching key from s' to `secret` ([K][n], NTT form at all K limbs) generated into the plan: s' = from_poly [K][n]
        (KEY_FROM_POLY), secret^2 (KEY_FROM_SQUARE) or secret(X^galois_elt) (KEY_FROM_GALOIS). Word for word rlwe_encrypt(count = L,
        n_limbs = K, pt[d][i] = [i == d] (P mod q_i) s'_i) -> set_keys; consumes polynomials first ... first + L - 1 of (seed, stream).
        Returns the seed's bytes (None = os.urandom)."""
        words, raw = seed_words(seed)
        _check(lib().hexl_ks_gen_keys(self.h, _ptr(secret), from_kind, galois_elt, None if from_poly is None else _ptr(from_poly), words,
                                      stream, first), "hexl_ks_gen_keys")
        return raw

    def gen_relin_keys(self, secret, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """the relinearisation key of `secret` (multiply_relinearize)"""
        return self.gen_keys(secret, KEY_FROM_SQUARE, seed=seed, stream=stream, first=first)

    def gen_galois_keys(self, secret, g: int, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """the key rotate / the hoisted family need for the Galois element g"""
        return self.gen_keys(secret, KEY_FROM_GALOIS, galois_elt=g, seed=seed, stream=stream, first=first)

    def gen_hybrid_key(self, out, secret, digit_limbs: int, from_poly, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """out[dnum][2][K][n] = the hybrid switching key (HybridKeySwitch.set_keys_device) from s' = from_poly ([K][n], NTT form) to
        `secret` ([K][n]), dnum = ceil(L / digit_limbs): key d encrypts P [i in G_d] s' modulo q_i (0 modulo the special primes
        L ... K - 1, whose product is P), G_d = the limbs d digit_limbs ... min((d + 1) digit_limbs, L) - 1. A wrapper, not a C entry
        point: dnum calls of ct_lincomb on from_poly with per-limb weights, then ONE key-shaped rlwe_encrypt(count = dnum, n_limbs = K,
        pt_batch = dnum). WARNING (include/hexl_mi355x.h): it consumes the UNIFORM and CBD21 polynomials first ... first + dnum - 1 of
        (seed, stream) -- never give two keys of one secret the same triple. Returns the seed's bytes (None = os.urandom)."""
        import torch
        L, K, n = self.L, self.K, self.n
        if not 1 <= digit_limbs <= L or K <= L:
            raise ValueError("gen_hybrid_key: 1 <= digit_limbs <= L < K")
        dnum = -(-L // digit_limbs)
        P = 1
        for q in self.moduli[L:K]:
            P *= q
        pt = torch.empty((dnum, K, n), dtype=torch.int64, device=from_poly.device)
        for d in range(dnum):
            w = [P % self.moduli[i] if d * digit_limbs <= i < min((d + 1) * digit_limbs, L) else 0 for i in range(K)]
            self.ct_lincomb(pt[d], [from_poly], 1, 1, K, weights=[w])
        raw = self.rlwe_encrypt(out, secret, dnum, K, pt=pt, pt_batch=dnum, seed=seed, stream=stream, first=first)
        self._hybrid_pt = pt          # the launches are asynchronous on the context's stream: the plaintexts outlive this call
        return raw

    def keyswitch(self, result, t_target, batch: int):
        _check(lib().hexl_keyswitch(self.h, _ptr(result), _ptr(t_target), batch), "hexl_keyswitch")

    def range_check(self) -> bool:
        """True if every keyswitch since the last check saw in-range words (syncs the stream, clears the flag)"""
        return _check_warn(lib().hexl_ks_range_check(self.h), "hexl_ks_range_check") == 0

    def tiers(self):
        """(per-limb forward reduction periods [K] -- 0 = strict, -1 = integer kernels --, True when the limbs in use differ)"""
        out = (_i * self.K)()
        rc = _check_warn(lib().hexl_ks_plan_tiers(self.h, out), "hexl_ks_plan_tiers")
        return list(out), rc == 1

    def multiply_relinearize(self, out, a, b, batch: int):
        """out[batch][2][L][n] = (a0 b0, a0 b1 + a1 b0) + KeySwitch(a1 b1), one fused pass (N = 1024 ... 32768, moduli < 2^52)"""
        _check(lib().hexl_multiply_relinearize(self.h, _ptr(out), _ptr(a), _ptr(b), batch), "hexl_multiply_relinearize")

    def rescale(self, out, inp, batch: int, n_limbs: int, n_components: int):
        """out[batch][n_components][n_limbs - 1][n] = inp[batch][n_components][n_limbs][n] divided by q_(n_limbs - 1), rounded
        (SEAL's rescale_to_next); moduli < 2^52, 2 <= n_limbs <= K - 1, no keys needed"""
        _check(lib().hexl_rescale(self.h, _ptr(out), _ptr(inp), batch, n_limbs, n_components), "hexl_rescale")

    def rotate(self, out, ct, batch: int, g: int):
        """out[batch][2][L][n] = (sigma_g(c0), 0) + KeySwitch(sigma_g(c1)); the plan's keys switch from s(X^g) to s"""
        _check(lib().hexl_rotate(self.h, _ptr(out), _ptr(ct), batch, g), "hexl_rotate")

    def rns_ntt_fwd(self, out, inp, count: int, n_limbs: int):
        """out[count][n_limbs][n] = negacyclic NTT of inp, polynomial (c, i) modulo the plan's q_i (coefficients in natural order in,
        the transforms' bit-reversed order out); out may be inp; moduli < 2^52, 1 <= n_limbs <= K, no keys needed"""
        _check(lib().hexl_rns_ntt_fwd(self.h, _ptr(out), _ptr(inp), count, n_limbs), "hexl_rns_ntt_fwd")

    def rns_ntt_inv(self, out, inp, count: int, n_limbs: int):
        """the inverse of rns_ntt_fwd, n^-1 included"""
        _check(lib().hexl_rns_ntt_inv(self.h, _ptr(out), _ptr(inp), count, n_limbs), "hexl_rns_ntt_inv")

    def multiply_plain(self, out, ct, pt, batch: int, n_components: int, n_limbs: int, pt_batch: int, accumulate: bool = False):
        """out[batch][n_components][n_limbs][n] = (out +, if accumulate) ct * pt[pt_batch][n_limbs][n] mod q_i, word by word in NTT
        form; pt_batch = 1 or batch; out may be ct unless accumulating"""
        _check(lib().hexl_multiply_plain(self.h, _ptr(out), _ptr(ct), _ptr(pt), batch, n_components, n_limbs, pt_batch,
                                         1 if accumulate else 0), "hexl_multiply_plain")

    def ct_lincomb(self, out, cts, batch: int, n_components: int, n_limbs: int, weights=None, in_limbs=None, pt=None, pt_batch: int = 1,
                   const=None):
        """out[batch][n_components][n_limbs][n] = sum_t weights[t][i] * cts[t] + (component 0 only) pt[pt_batch][n_limbs][n] + const[i]
        mod q_i, word by word in NTT form. cts: 1 ... 8 device tensors, term t [batch][n_components][in_limbs[t]][n] read through its first
        n_limbs limbs (in_limbs None: all n_limbs); weights: host [n_terms][n_limbs] residues (None: all 1; q_i - 1 subtracts); const: host
        [n_limbs] residues or None; out may be a term whose in_limbs is n_limbs"""
        u64s = lambda a: None if a is None else np.ascontiguousarray(np.asarray([int(v) for v in np.asarray(a, dtype=object).reshape(-1)],
                                                                                dtype=np.uint64))
        w, il, c = u64s(weights), u64s(in_limbs), u64s(const)
        if (w is not None and w.size != len(cts) * n_limbs) or (il is not None and il.size != len(cts)) or (c is not None and c.size != n_limbs):
            raise ValueError("ct_lincomb: weights are [n_terms][n_limbs], in_limbs [n_terms], const [n_limbs]")
        hp = lambda a: None if a is None else a.ctypes.data
        _check(lib().hexl_ct_lincomb(self.h, _ptr(out), ptr_array(cts), hp(il), hp(w), len(cts), None if pt is None else _ptr(pt), pt_batch,
                                     hp(c), batch, n_components, n_limbs), "hexl_ct_lincomb")

    @staticmethod
    def _tensor_operands(what, a_s, b_s, in_limbs):
        """(pointer arrays of the two operand lists, the [n_terms][2] limb counts as a host array or None)"""
        if len(a_s) != len(b_s):
            raise ValueError(f"{what}: one b per a")
        il = None if in_limbs is None else np.ascontiguousarray(np.asarray([int(v) for v in np.asarray(in_limbs, dtype=object).reshape(-1)],
                                                                            dtype=np.uint64))
        if il is not None and il.size != 2 * len(a_s):
            raise ValueError(f"{what}: in_limbs is [n_terms][2]")
        return ptr_array(a_s), ptr_array(b_s), il

    def ct_tensor_sum(self, out, a_s, b_s, batch: int, n_limbs: int, in_limbs=None):
        """out[batch][3][n_limbs][n] = sum_t (a0 b0, a0 b1 + a1 b0, a1 b1) of the 1 ... 8 pairs (a_s[t], b_s[t]) mod q_i, word by word in
        NTT form -- the product before relinearisation, what ct_lincomb, rescale and rlwe_decrypt take with three components. a_s[t] is
        [batch][2][in_limbs[t][0]][n], b_s[t] [batch][2][in_limbs[t][1]][n], each read through its first n_limbs limbs (in_limbs None: all
        n_limbs); b_s[t] may be a_s[t]; out must not overlap an operand. No keys needed."""
        pa, pb, il = self._tensor_operands("ct_tensor_sum", a_s, b_s, in_limbs)
        _check(lib().hexl_ct_tensor_sum(self.h, _ptr(out), pa, pb, None if il is None else il.ctypes.data, len(a_s), batch, n_limbs),
               "hexl_ct_tensor_sum")

    def relinearize(self, out, ct3, batch: int):
        """out[batch][2][L][n] = (c0, c1) + KeySwitch(c2) of ct3[batch][3][L][n]; the plan's keys are the relinearisation key
        (gen_relin_keys). Every plan keyswitch accepts."""
        _check(lib().hexl_relinearize(self.h, _ptr(out), _ptr(ct3), batch), "hexl_relinearize")

    def multiply_sum_relinearize(self, out, a_s, b_s, batch: int, in_limbs=None):
        """out[batch][2][L][n] = relinearize(ct_tensor_sum(a_s, b_s, n_limbs = L)), word for word, with ONE key switch whatever the number
        of pairs and without the three-component sum ever existing in memory; in_limbs entries in L ... K"""
        pa, pb, il = self._tensor_operands("multiply_sum_relinearize", a_s, b_s, in_limbs)
        _check(lib().hexl_multiply_sum_relinearize(self.h, _ptr(out), pa, pb, None if il is None else il.ctypes.data, len(a_s), batch),
               "hexl_multiply_sum_relinearize")

    def rns_from_f64(self, out, coeffs, count: int, n_limbs: int):
        """out[count][n_limbs][n] = NTT_i(rint(coeffs[count][n]) mod q_i): real coefficients (float64, natural order) to NTT-form limbs,
        exact for |rint(c)| < 2^62; a coefficient outside that raises the range flag (range_check)"""
        _check(lib().hexl_rns_from_f64(self.h, _ptr(out), _ptr(coeffs), count, n_limbs), "hexl_rns_from_f64")

    def rns_to_f64(self, coeffs, inp, count: int, n_limbs: int):
        """coeffs[count][n] (float64) = the centred CRT value of every coefficient of inp[count][n_limbs][n] (NTT form): exact below 2^53,
        within 2^-50 relative above"""
        _check(lib().hexl_rns_to_f64(self.h, _ptr(coeffs), _ptr(inp), count, n_limbs), "hexl_rns_to_f64")

    def ckks_encode(self, out, slots, count: int, n_limbs: int, scale: float):
        """out[count][n_limbs][n] = the NTT-form plaintext of slots[count][n/2][2] (float64 re, im) at `scale`: slot k at the evaluation
        point zeta^(5^k), coefficients rounded to nearest"""
        _check(lib().hexl_ckks_encode(self.h, _ptr(out), _ptr(slots), count, n_limbs, scale), "hexl_ckks_encode")

    def ckks_decode(self, slots, inp, count: int, n_limbs: int, scale: float):
        """slots[count][n/2][2] = the slot values of the plaintext inp[count][n_limbs][n] divided by `scale`"""
        _check(lib().hexl_ckks_decode(self.h, _ptr(slots), _ptr(inp), count, n_limbs, scale), "hexl_ckks_decode")

    def sample(self, out, kind: int, count: int, n_limbs: int, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """out[count][n_limbs][n] = polynomials first ... first + count - 1 of the ChaCha20 stream (seed, stream, kind) modulo the plan's
        first n_limbs moduli, NTT form: SAMPLE_UNIFORM, SAMPLE_TERNARY (secrets) or SAMPLE_CBD21 (errors). seed: 32 bytes / eight u32,
        None = os.urandom(32); returns the seed's bytes. Never use (seed, stream, index) twice with one secret."""
        words, raw = seed_words(seed)
        _check(lib().hexl_sample(self.h, _ptr(out), kind, words, stream, first, count, n_limbs), "hexl_sample")
        return raw

    def rlwe_encrypt(self, out, secret, count: int, n_limbs: int, pt=None, pt_batch: int = 1, seed=None, stream: int = 0,
                     first: int = 0) -> bytes:
        """out[count][2][n_limbs][n] = (pt + e - a secret, a) with a = the UNIFORM and e = the CBD21 polynomial first + b of (seed,
        stream); pt None (an encryption of zero) or [pt_batch][n_limbs][n], pt_batch = 1 or count; secret [>= n_limbs][n] in NTT form.
        count = L, n_limbs = K, pt_batch = count: out is the h_keys layout of set_keys. Returns the seed's bytes (None = os.urandom)."""
        words, raw = seed_words(seed)
        _check(lib().hexl_rlwe_encrypt(self.h, _ptr(out), None if pt is None else _ptr(pt), pt_batch, _ptr(secret), words, stream, first,
                                       count, n_limbs), "hexl_rlwe_encrypt")
        return raw

    def gen_public_key(self, out, secret, n_limbs=None, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """out[2][n_limbs][n] = (pk0, pk1) = (e - a secret, a): rlwe_encrypt(pt=None, count=1), n_limbs None = K (such a key serves every
        level through pk_encrypt's pk_limbs). Consumes the UNIFORM and CBD21 polynomial `first` of (seed, stream). Returns the seed's
        bytes (None = os.urandom)."""
        return self.rlwe_encrypt(out, secret, 1, self.K if n_limbs is None else n_limbs, seed=seed, stream=stream, first=first)

    def pk_encrypt(self, out, pk, count: int, n_limbs: int, pk_limbs=None, pt=None, pt_batch: int = 1, seed=None, stream: int = 0,
                   first: int = 0) -> bytes:
        """out[count][2][n_limbs][n] = (pk0 u + e0 + pt, pk1 u + e1) under the public key pk[2][pk_limbs][n] (gen_public_key; pk_limbs
        None = n_limbs, only the first n_limbs limbs of each component are read): u = the TERNARY polynomial first + b, e0 / e1 = the
        CBD21 polynomials 2 (first + b) and 2 (first + b) + 1 of (seed, stream); pt None (an encryption of zero) or
        [pt_batch][n_limbs][n], pt_batch = 1 or count. Give the call a (seed, stream) of its own and advance `first` by `count`.
        Returns the seed's bytes (None = os.urandom)."""
        words, raw = seed_words(seed)
        _check(lib().hexl_pk_encrypt(self.h, _ptr(out), None if pt is None else _ptr(pt), pt_batch, _ptr(pk),
                                     n_limbs if pk_limbs is None else pk_limbs, words, stream, first, count, n_limbs), "hexl_pk_encrypt")
        return raw

    def rlwe_decrypt(self, out, ct, secret, count: int, n_components: int, n_limbs: int):
        """out[count][n_limbs][n] = c0 + c1 secret (+ c2 secret^2 when n_components = 3) of ct[count][n_components][n_limbs][n]"""
        _check(lib().hexl_rlwe_decrypt(self.h, _ptr(out), _ptr(ct), _ptr(secret), count, n_components, n_limbs), "hexl_rlwe_decrypt")

    def keyswitch_host(self, results, t_targets):
        n = len(results)
        r = (_vp * n)(*[_ptr(a) for a in results])
        t = (_vp * n)(*[_ptr(a) for a in t_targets])
        # (1 = HEXL_W_RANGE: computed, some object had an out-of-range word)
        return _check_warn(lib().hexl_keyswitch_host(self.h, r, t, n), "hexl_keyswitch_host") == 0

    def time_stages(self, result, t_target, batch: int, iters: int):
        out = (ctypes.c_float * 4)()
        _check(lib().hexl_ks_time_stages(self.h, _ptr(result), _ptr(t_target), batch, iters, out),
               "hexl_ks_time_stages")
        return list(out)

    def scratch_bytes(self, batch: int) -> int:
        return lib().hexl_ks_scratch_bytes(self.h, batch)

    def close(self):
        if getattr(self, "h", None):
            lib().hexl_ks_plan_destroy(self.h)
            self.h = None


class HybridKeySwitch:
    """The hybrid key switch (hexl_hks): digit_limbs = alpha data limbs per digit, the plan's limbs L ... K - 1 as special primes, one
    installed key for every level n_limbs = 1 ... L. Attached to an FP64 `plan` created with K > L, which it borrows: close() it
    before the plan. All launches are asynchronous on the context's stream."""

    def __init__(self, plan: KeySwitchPlan, digit_limbs: int):
        self.plan, self.alpha = plan, digit_limbs
        self.dnum = -(-plan.L // digit_limbs) if digit_limbs >= 1 else 0
        h = _vp()
        _check(lib().hexl_hks_create(plan.h, digit_limbs, ctypes.byref(h)), "hexl_hks_create")
        self.h = h

    def set_keys_device(self, keys):
        """keys: device tensor [dnum][2][K][n], key d at d*2*K*n, word (k*K + i)*n + j (KeySwitchPlan.gen_hybrid_key writes it); one
        kernel on the context's stream, no host synchronisation -- an object in use may be re-keyed"""
        _check(lib().hexl_hks_set_keys_device(self.h, _ptr(keys)), "hexl_hks_set_keys_device")

    def gen_keys(self, secret, from_kind: int, galois_elt: int = 1, from_poly=None, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """the hybrid switching key from s' to `secret` ([K][n], NTT form at all K limbs) generated into the object (hks_keygen with one
        key): s' = from_poly [K][n] (KEY_FROM_POLY), secret^2 (KEY_FROM_SQUARE) or secret(X^galois_elt) (KEY_FROM_GALOIS). Word for word
        plan.gen_hybrid_key -> set_keys_device; consumes polynomials first ... first + dnum - 1 of (seed, stream). Returns the seed's
        bytes (None = os.urandom)."""
        return hks_keygen([self], secret, [from_kind], galois_elts=[galois_elt], from_polys=[from_poly], seed=seed, stream=stream, first=first)

    def gen_relin_keys(self, secret, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """the relinearisation key of `secret` (relinearize and the hybrid multiply)"""
        return self.gen_keys(secret, KEY_FROM_SQUARE, seed=seed, stream=stream, first=first)

    def gen_galois_keys(self, secret, g: int, seed=None, stream: int = 0, first: int = 0) -> bytes:
        """the key rotate, the hoisted and the BSGS calls need for the Galois element g"""
        return self.gen_keys(secret, KEY_FROM_GALOIS, galois_elt=g, seed=seed, stream=stream, first=first)

    def export_keys(self, out):
        """out[dnum][2][K][n] = the installed key as canonical words in the set_keys_device layout (hexl_hks_export_keys); one kernel on
        the context's stream"""
        _check(lib().hexl_hks_export_keys(self.h, _ptr(out)), "hexl_hks_export_keys")

    def keyswitch(self, result, t_target, batch: int, n_limbs: int):
        """result[batch][2][n_limbs][n] += KeySwitch(t_target[batch][n_limbs][n]) mod q_i, as KeySwitchPlan.keyswitch"""
        _check(lib().hexl_hks_keyswitch(self.h, _ptr(result), _ptr(t_target), batch, n_limbs), "hexl_hks_keyswitch")

    def relinearize(self, out, ct3, batch: int, n_limbs: int):
        """out[batch][2][n_limbs][n] = (c0, c1) + KeySwitch(c2) of ct3[batch][3][n_limbs][n]"""
        _check(lib().hexl_hks_relinearize(self.h, _ptr(out), _ptr(ct3), batch, n_limbs), "hexl_hks_relinearize")

    def rotate(self, out, ct, batch: int, n_limbs: int, g: int):
        """out[batch][2][n_limbs][n] = (sigma_g(c0), 0) + KeySwitch(sigma_g(c1)); the keys switch from s(X^g) to s"""
        _check(lib().hexl_hks_rotate(self.h, _ptr(out), _ptr(ct), batch, n_limbs, g), "hexl_hks_rotate")

    def scratch_bytes(self, batch: int) -> int:
        return lib().hexl_hks_scratch_bytes(self.h, batch)

    def hoisted_scratch_bytes(self, batch: int) -> int:
        """scratch_bytes plus the buffer hks_rotate_hoisted / hks_linear_transform keep on their first object"""
        return lib().hexl_hks_hoisted_scratch_bytes(self.h, batch)

    def bsgs_scratch_bytes(self, n_baby: int, batch: int) -> int:
        """device bytes an hks_linear_transform_bsgs call with this object first holds on it: hoisted scratch, baby store and t_j"""
        return lib().hexl_hks_bsgs_scratch_bytes(self.h, n_baby, batch)

    def bsgs_ext_scratch_bytes(self, n_baby: int, batch: int, rescale: int) -> int:
        """device bytes an hks_linear_transform_bsgs_ext call with this object first holds on it: bsgs_scratch_bytes at the same chunk, the
        extended-basis accumulator A and, with rescale = 1, the key-free sums F"""
        return lib().hexl_hks_bsgs_ext_scratch_bytes(self.h, n_baby, batch, rescale)

    def multiply_sum_relinearize(self, out, a_s, b_s, batch: int, n_limbs: int, in_limbs=None):
        """out[batch][2][n_limbs][n] = relinearize(plan.ct_tensor_sum(a_s, b_s, n_limbs)) on the hybrid key, word for word, without the
        three-component sum ever existing in memory; operands as KeySwitchPlan.ct_tensor_sum, in_limbs entries in n_limbs ... K"""
        pa, pb, il = self.plan._tensor_operands("hks multiply_sum_relinearize", a_s, b_s, in_limbs)
        _check(lib().hexl_hks_multiply_sum_relinearize(self.h, _ptr(out), pa, pb, None if il is None else il.ctypes.data, len(a_s), batch,
                                                       n_limbs), "hexl_hks_multiply_sum_relinearize")

    def relinearize_rescale(self, out, ct3, batch: int, n_limbs: int):
        """out[batch][2][n_limbs - 1][n] = (P (d0, d1) + KSacc(d2)) / (P q_(n_limbs-1)) rounded, of ct3[batch][3][n_limbs][n]: the
        relinearisation and the rescale in ONE mod-down (n_limbs >= 2). Decrypts like relinearize -> plan.rescale, but is not
        word-identical to it (one rounding instead of two)."""
        _check(lib().hexl_hks_relinearize_rescale(self.h, _ptr(out), _ptr(ct3), batch, n_limbs), "hexl_hks_relinearize_rescale")

    def multiply_sum_rescale(self, out, a_s, b_s, batch: int, n_limbs: int, in_limbs=None):
        """out[batch][2][n_limbs - 1][n] = relinearize_rescale(plan.ct_tensor_sum(a_s, b_s, n_limbs)), word for word, with neither the
        three-component sum nor the un-rescaled ciphertext in memory (n_limbs >= 2); operands as KeySwitchPlan.ct_tensor_sum"""
        pa, pb, il = self.plan._tensor_operands("hks multiply_sum_rescale", a_s, b_s, in_limbs)
        _check(lib().hexl_hks_multiply_sum_rescale(self.h, _ptr(out), pa, pb, None if il is None else il.ctypes.data, len(a_s), batch,
                                                   n_limbs), "hexl_hks_multiply_sum_rescale")

    def mul_scratch_bytes(self, batch: int) -> int:
        """scratch_bytes plus the slice and (d0, d1) buffers the multiply calls keep on the object"""
        return lib().hexl_hks_mul_scratch_bytes(self.h, batch)

    def close(self):
        if getattr(self, "h", None):
            lib().hexl_hks_destroy(self.h)
            self.h = None


def rotate_hoisted(plans, galois_elts, outs, ct, batch: int):
    """outs[r][batch][2][L][n] = (sigma_g(c0), 0) + ModDown(sum_d sigma_g(u_d) . key_r[d]) for g = galois_elts[r] and the keys of
    plans[r], with the mod-up u of ct's component 1 computed once for all of them (hexl_rotate_hoisted). Decrypts like
    plans[r].rotate(outs[r], ct, batch, g) but is word-identical to it only for g = 1. The plans share one context, n, L, K and moduli
    (FP64 plans); the scratch is plans[0]'s."""
    if not (len(plans) == len(galois_elts) == len(outs)):
        raise ValueError("rotate_hoisted: one plan, one Galois element and one output per rotation")
    _check(lib().hexl_rotate_hoisted(_handles(plans), _u64_array(galois_elts), len(plans), ptr_array(outs), _ptr(ct), batch), "hexl_rotate_hoisted")


def linear_transform(plans, galois_elts, pts, out, ct, batch: int, pt_identity=None):
    """out[batch][2][L][n] = sum_r pts[r] . Rotate_g_r(ct) + pt_identity . ct for g_r = galois_elts[r] and the keys of plans[r], with
    the mod-up of ct's component 1 AND the mod-down shared by all rotations (hexl_linear_transform): the weighted sum is taken in the
    extended basis, so each pts[r] is [L + 1][n] -- the plaintext modulo q_0 ... q_(L-1) and modulo the special prime, in NTT form
    (plans[r].rns_ntt_fwd(..., 1, K) when K = L + 1); pt_identity is [L][n] or None. Decrypts like rotate_hoisted -> multiply_plain ->
    accumulate but is not word-identical to it (one rounding by the special prime instead of one per rotation). The plans share one
    context, n, L, K and moduli (FP64 plans); the scratch is plans[0]'s."""
    if not (len(plans) == len(galois_elts) == len(pts)):
        raise ValueError("linear_transform: one plan, one Galois element and one plaintext per rotation")
    _check(lib().hexl_linear_transform(_handles(plans), _u64_array(galois_elts), ptr_array(pts), len(plans), None if pt_identity is None else _ptr(pt_identity), _ptr(out),
                                       _ptr(ct), batch), "hexl_linear_transform")


def hks_keygen(hks_list, secret, from_kinds, galois_elts=None, from_polys=None, seed=None, stream: int = 0, first: int = 0) -> bytes:
    """one hybrid switching key per object of hks_list, generated into the objects by ONE call (hexl_hks_keygen): key r switches from s'_r
    to `secret` ([K][n], NTT form at all K limbs), s'_r = from_polys[r] (KEY_FROM_POLY), secret^2 (KEY_FROM_SQUARE) or
    secret(X^galois_elts[r]) (KEY_FROM_GALOIS) by from_kinds[r]. Word for word plan.gen_hybrid_key(..., first=first_r) -> set_keys_device
    per object with first_r = first + the dnum of the objects before r. The objects share one plan and may differ in alpha; at most 64.
    WARNING (include/hexl_mi355x.h): it consumes the UNIFORM and CBD21 polynomials first ... first + sum dnum - 1 of (seed, stream).
    galois_elts / from_polys: None, or one entry per key (entries of other kinds are ignored; from_polys entries may be None). Returns
    the seed's bytes (None = os.urandom)."""
    count = len(hks_list)
    if len(from_kinds) != count or any(x is not None and len(x) != count for x in (galois_elts, from_polys)):
        raise ValueError("hks_keygen: one kind (and one element / polynomial, where given) per object")
    words, raw = seed_words(seed)
    _check(lib().hexl_hks_keygen(_handles(hks_list), count, (_i * count)(*[int(k) for k in from_kinds]),
                                 None if galois_elts is None else _u64_array(galois_elts), None if from_polys is None else _opt_ptrs(from_polys),
                                 _ptr(secret), words, stream, first), "hexl_hks_keygen")
    return raw


def hks_rotate_hoisted(hks_list, galois_elts, outs, ct, batch: int, n_limbs: int):
    """outs[r][batch][2][n_limbs][n] = (sigma_g(c0), 0) + ModDown(sum_d sigma_g(ext_d) . key_r[d]) for g = galois_elts[r] and the hybrid
    key of hks_list[r], with the extended digits ext of ct's component 1 computed once for all of them (hexl_hks_rotate_hoisted).
    Decrypts like hks_list[r].rotate(outs[r], ct, batch, n_limbs, g) but is word-identical to it only for g = 1. The objects share one
    plan and one alpha; the scratch is hks_list[0]'s."""
    if not (len(hks_list) == len(galois_elts) == len(outs)):
        raise ValueError("hks_rotate_hoisted: one object, one Galois element and one output per rotation")
    _check(lib().hexl_hks_rotate_hoisted(_handles(hks_list), _u64_array(galois_elts), len(hks_list), ptr_array(outs), _ptr(ct), batch, n_limbs),
           "hexl_hks_rotate_hoisted")


def hks_linear_transform(hks_list, galois_elts, pts, pt_identity, out, ct, batch: int, n_limbs: int):
    """out[batch][2][n_limbs][n] = sum_r pts[r] . Rotate_g_r(ct) + pt_identity . ct on the hybrid keys of hks_list[r], with the mod-up of
    ct's component 1 AND the mod-down shared by all rotations (hexl_hks_linear_transform). Each pts[r] is [K][n]: the plaintext modulo
    all K plan limbs in NTT form (plan.rns_ntt_fwd / plan.ckks_encode at K limbs), one encoding for every level; pt_identity is
    [>= n_limbs][n] or None. The objects share one plan and one alpha; the scratch is hks_list[0]'s."""
    if not (len(hks_list) == len(galois_elts) == len(pts)):
        raise ValueError("hks_linear_transform: one object, one Galois element and one plaintext per rotation")
    _check(lib().hexl_hks_linear_transform(_handles(hks_list), _u64_array(galois_elts), ptr_array(pts), len(hks_list),
                                           None if pt_identity is None else _ptr(pt_identity), _ptr(out), _ptr(ct), batch, n_limbs),
           "hexl_hks_linear_transform")


def hks_linear_transform_bsgs(baby_hks, baby_elts, giant_hks, giant_elts, pts, pt_identity, out, ct, batch: int, n_limbs: int):
    """out[batch][2][n_limbs][n] = sum_j Rotate_G_j( sum_i pts[j][i] . Rotate_g_i(ct) + pt_identity[j] . ct ) on the hybrid keys of
    baby_hks[i] (g_i = baby_elts[i]) and giant_hks[j] (G_j = giant_elts[j]) (hexl_hks_linear_transform_bsgs): n_baby + n_giant keys and
    key passes instead of n_baby * n_giant. pts is a list of n_giant rows of n_baby entries, each None (an absent diagonal) or [K][n] as
    for hks_linear_transform, already rotated by G_j^-1; pt_identity is None or a list of n_giant entries, each None or [>= n_limbs][n].
    A baby object whose column is empty and a giant object with G_j = 1 may be None. Word for word hks_linear_transform per row ->
    hks_rotate_hoisted -> sum; the objects share one plan and one alpha, the scratch is the first object's."""
    n_baby, n_giant = len(baby_hks), len(giant_hks)
    if len(baby_elts) != n_baby or len(giant_elts) != n_giant or len(pts) != n_giant or any(len(row) != n_baby for row in pts):
        raise ValueError("hks_linear_transform_bsgs: one element per object and n_giant rows of n_baby plaintexts")
    if pt_identity is not None and len(pt_identity) != n_giant:
        raise ValueError("hks_linear_transform_bsgs: one identity plaintext (or None) per giant step")
    flat = [p for row in pts for p in row]
    _check(lib().hexl_hks_linear_transform_bsgs(_handles(baby_hks), _u64_array(baby_elts), n_baby, _handles(giant_hks), _u64_array(giant_elts),
                                                n_giant, _opt_ptrs(flat), None if pt_identity is None else _opt_ptrs(pt_identity), _ptr(out),
                                                _ptr(ct), batch, n_limbs), "hexl_hks_linear_transform_bsgs")


def hks_linear_transform_bsgs_ext(baby_hks, baby_elts, giant_hks, giant_elts, pts, pt_identity, out, ct, batch: int, n_limbs: int, rescale: int):
    """The sum of hks_linear_transform_bsgs with the giant steps kept in the extended basis and ONE division per call
    (hexl_hks_linear_transform_bsgs_ext): out[batch][2][n_limbs][n] for rescale = 0; rescale = 1 divides by P q_(l-1) in the same mod-down
    and writes out[batch][2][n_limbs - 1][n], the rescaled result. Arguments as hks_linear_transform_bsgs. Not word for word that call
    when some G_j != 1 (one rounding instead of one per row and per rotated giant step); both decrypt alike."""
    n_baby, n_giant = len(baby_hks), len(giant_hks)
    if len(baby_elts) != n_baby or len(giant_elts) != n_giant or len(pts) != n_giant or any(len(row) != n_baby for row in pts):
        raise ValueError("hks_linear_transform_bsgs_ext: one element per object and n_giant rows of n_baby plaintexts")
    if pt_identity is not None and len(pt_identity) != n_giant:
        raise ValueError("hks_linear_transform_bsgs_ext: one identity plaintext (or None) per giant step")
    flat = [p for row in pts for p in row]
    _check(lib().hexl_hks_linear_transform_bsgs_ext(_handles(baby_hks), _u64_array(baby_elts), n_baby, _handles(giant_hks),
                                                    _u64_array(giant_elts), n_giant, _opt_ptrs(flat),
                                                    None if pt_identity is None else _opt_ptrs(pt_identity), _ptr(out), _ptr(ct), batch,
                                                    n_limbs, rescale), "hexl_hks_linear_transform_bsgs_ext")


def _opt_ptrs(items):
    """ctypes array of pointers with None entries as NULL"""
    return (_vp * len(items))(*[None if a is None else _ptr(a) for a in items])


def linear_transform_bsgs(baby_plans, baby_elts, giant_plans, giant_elts, pts, out, ct, batch: int, pt_identity=None):
    """out[batch][2][L][n] = sum_j Rotate_G_j( sum_i pts[j][i] . Rotate_g_i(ct) + pt_identity[j] . ct ) with g_i = baby_elts[i] and the
    keys of baby_plans[i], G_j = giant_elts[j] and the keys of giant_plans[j] (hexl_linear_transform_bsgs): n_baby + n_giant key passes
    instead of n_baby * n_giant. pts is a list of n_giant rows of n_baby entries, each None (an absent diagonal) or [L + 1][n] as for
    linear_transform, already rotated by G_j^-1; pt_identity is None or a list of n_giant entries, each None or [L][n]. A baby plan whose
    column is empty and a giant plan with G_j = 1 may be None. Word for word linear_transform per row -> rotate_hoisted -> sum; the
    scratch, the buffers and the range flag are the first plan's."""
    n_baby, n_giant = len(baby_plans), len(giant_plans)
    if len(baby_elts) != n_baby or len(giant_elts) != n_giant or len(pts) != n_giant or any(len(row) != n_baby for row in pts):
        raise ValueError("linear_transform_bsgs: one element per plan and n_giant rows of n_baby plaintexts")
    if pt_identity is not None and len(pt_identity) != n_giant:
        raise ValueError("linear_transform_bsgs: one identity plaintext (or None) per giant step")
    flat = [p for row in pts for p in row]
    _check(lib().hexl_linear_transform_bsgs(_handles(baby_plans), _u64_array(baby_elts), n_baby, _handles(giant_plans), _u64_array(giant_elts), n_giant,
                                            _opt_ptrs(flat), None if pt_identity is None else _opt_ptrs(pt_identity), _ptr(out), _ptr(ct),
                                            batch), "hexl_linear_transform_bsgs")


def lt_bsgs_scratch_bytes(plan, n_baby: int, batch: int) -> int:
    """device bytes a linear_transform_bsgs call with `plan` first holds on it: baby store, inner result and keyswitch scratch"""
    return lib().hexl_lt_bsgs_scratch_bytes(plan.h, n_baby, batch)


from .host_api import HexlFpga  # noqa: E402  (mirror of host/inc/hexl-fpga.h)

__all__ = ["Context", "KeySwitchPlan", "HybridKeySwitch", "HexlFpga", "HexlError", "build", "lib", "as_i64", "to_u64", "rotate_hoisted", "linear_transform", "hks_keygen", "hks_rotate_hoisted", "hks_linear_transform", "hks_linear_transform_bsgs", "hks_linear_transform_bsgs_ext",
           "linear_transform_bsgs", "lt_bsgs_scratch_bytes", "C_ABI", "SAMPLE_UNIFORM", "SAMPLE_TERNARY", "SAMPLE_CBD21", "KEY_FROM_POLY", "KEY_FROM_SQUARE", "KEY_FROM_GALOIS", "seed_words",
           "LIB_PATH", "ROOT"]
