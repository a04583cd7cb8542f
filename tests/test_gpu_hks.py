"""GPU: the hybrid key switch (hexl_hks_*) bit-exact against tests/hks_model.py, every word of every instance: digit groups and several
special primes at n = 1024 (uniform and extreme operands, a ragged last digit at every level with ONE installed key, one digit, the
per-limb anchor against hexl_keyswitch on the same device key buffer, n_p != alpha, a mixed-tier chain), one case each at n = 16384 and
n = 32768, two scratch chunks (a child process with HEXL_KS_CHUNK) and a regrow followed by a smaller call, relinearize and rotate,
re-keying between launches without a synchronisation, a non-blocking caller stream, the borrowed plan's own key switch before and
after, every rejection, and end to end: gen_hybrid_key (square and Galois) -> switch -> hexl_rlwe_decrypt within the noise bound."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ckks_model import Limbs, apply_galois
from hks_model import Hks
from ks_util import KsCase, extreme_words, seal_chain
from rns_model import assert_instances

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("component", "limb", "coefficient")
HEXL_E_BADARG, HEXL_E_NOKEYS = -1, -2


def torch_():
    import torch
    return torch


def up(hx, dev, a):
    return hx.as_i64(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)).to(dev)


def minus_one(dev, words):
    return torch_().full((words,), -1, dtype=torch_().int64, device=dev)


class Setup:
    """a plan with K > L, its hybrid object and the model; keys: uniform or extreme words, [dnum][2][K][n]"""

    def __init__(self, hx, ctx, orc, n, L, K, alpha, moduli, family="uniform", seed=1):
        self.n, self.L, self.K, self.alpha = n, L, K, alpha
        self.case = KsCase(orc, n, L, K, seed=seed, moduli=moduli)
        self.qs = [int(q) for q in self.case.moduli]
        self.plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, self.case.moduli, self.case.modswitch)
        self.hks = hx.HybridKeySwitch(self.plan, alpha)
        self.model = Hks(orc, n, L, K, alpha, self.qs)
        self.orc, self.family = orc, family

    def keys(self, salt=0):
        rows = [extreme_words(self.n, self.qs[i], salt + d * 5 + k * 3 + i) if self.family == "extreme" else
                self.orc.splitmix(self.n, 9001 + salt * 7919 + d * 131 + k * 17 + i, self.qs[i])
                for d in range(self.model.dnum) for k in range(2) for i in range(self.K)]
        return np.concatenate(rows)

    def words(self, comps, l, b, salt):
        """instance b of a [comps][l][n] operand"""
        if self.family == "extreme":
            return np.concatenate([extreme_words(self.n, self.qs[i], salt + b * 5 + k * 3 + i) for k in range(comps) for i in range(l)])
        return np.concatenate([self.orc.splitmix(self.n, 5003 + salt * 1009 + b * 97 + k * 17 + i, self.qs[i])
                               for k in range(comps) for i in range(l)])

    def close(self):
        self.hks.close()
        self.plan.close()


def run_keyswitch(hx, ctx, dev, s, keys, l, batch, label, distinct=None):
    """hexl_hks_keyswitch of `batch` instances (cycling over `distinct` different ones) at level l against the model"""
    distinct = distinct or batch
    ts = [s.words(1, l, b, 1) for b in range(distinct)]
    rs = [s.words(2, l, b, 2) for b in range(distinct)]
    want = [s.model.keyswitch(keys, ts[b], rs[b], l) for b in range(distinct)]
    d_t = up(hx, dev, np.stack([ts[b % distinct] for b in range(batch)]))
    d_r = up(hx, dev, np.stack([rs[b % distinct] for b in range(batch)]))
    s.hks.keyswitch(d_r, d_t, batch, l)
    ctx.sync()
    assert_instances(hx.to_u64(d_r), want, batch, NAMES, (2, l, s.n), label)
    assert np.array_equal(hx.to_u64(d_t), np.stack([ts[b % distinct] for b in range(batch)]).reshape(-1)), "the input was written"


SHAPES = {
    # name: (L, alpha, K, moduli expression, family)
    "L4_a2_K6_uniform": (4, 2, 6, lambda orc, n: orc.primes(6, 51, n), "uniform"),
    "L4_a2_K6_extreme": (4, 2, 6, lambda orc, n: orc.primes(6, 51, n), "extreme"),
    "one_digit_a3": (3, 3, 6, lambda orc, n: orc.primes(6, 50, n), "uniform"),
    "np1_a2": (4, 2, 5, lambda orc, n: orc.primes(5, 51, n), "extreme"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_keyswitch_matches_the_model(hx, ctx, dev, orc, shape):
    L, alpha, K, mod, family = SHAPES[shape]
    s = Setup(hx, ctx, orc, 1024, L, K, alpha, mod(orc, 1024), family)
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    run_keyswitch(hx, ctx, dev, s, keys, L, 3, f"hexl_hks_keyswitch {shape}")
    assert s.hks.scratch_bytes(1) == (L + s.model.dnum * K + 2 * K) * 1024 * 8
    s.close()


def test_mixed_tier_chain(hx, ctx, dev, orc):
    """52, 30, 30, 40-bit data limbs and two 27-bit special primes: every transform on its own limb's tier"""
    s = Setup(hx, ctx, orc, 1024, 4, 6, 2, seal_chain(orc, 6, 1024), "extreme")
    tiers, mixed = s.plan.tiers()
    assert mixed and tiers[0] == 0 and all(t != 0 for t in tiers[1:]), tiers
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    for l in (4, 2):
        run_keyswitch(hx, ctx, dev, s, keys, l, 2, f"mixed tiers, level {l}")
    s.close()


def test_one_key_serves_every_level_with_a_ragged_last_digit(hx, ctx, dev, orc):
    """L = 5, alpha = 2, K = 7: digits {0,1} {2,3} {4}; levels 5 ... 1 on ONE installed key (levels 3 and 1 end in a partial digit)"""
    s = Setup(hx, ctx, orc, 1024, 5, 7, 2, orc.primes(7, 51, 1024))
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    for l in (5, 4, 3, 2, 1):
        run_keyswitch(hx, ctx, dev, s, keys, l, 2, f"ragged digits, level {l}")
    s.close()


@pytest.mark.parametrize("L", [2, 3])
def test_alpha_one_is_hexl_keyswitch_on_the_same_key_buffer(hx, ctx, dev, orc, L):
    """alpha = 1, K = L + 1: the per-limb gadget. Both objects install the SAME device buffer; the borrowed plan's own key switch gives
    the same words before the hybrid object exists, beside it and after it has run and gone"""
    torch = torch_()
    n, batch = 1024, 3
    case = KsCase(orc, n, L, L + 1, seed=5)
    plan = hx.KeySwitchPlan(ctx, n, L, L + 1, L + 1, 2, case.moduli, case.modswitch)
    d_keys = up(hx, dev, np.concatenate(case.keys))
    plan.set_keys_device(d_keys)
    ins = [case.inputs(orc, b) for b in range(batch)]
    t0 = up(hx, dev, np.stack([t for t, _ in ins]))
    r0 = up(hx, dev, np.stack([r for _, r in ins]))

    def plan_switch():
        r = r0.clone()
        plan.keyswitch(r, t0, batch)
        ctx.sync()
        return r

    before = plan_switch()
    assert_instances(hx.to_u64(before), [case.expected(orc, t, r) for t, r in ins], batch, NAMES, (2, L, n), "hexl_keyswitch")
    hks = hx.HybridKeySwitch(plan, 1)
    hks.set_keys_device(d_keys)
    r = r0.clone()
    hks.keyswitch(r, t0, batch, L)
    ctx.sync()
    assert torch.equal(r, before), "alpha = 1, K = L + 1 must be hexl_keyswitch word for word"
    assert torch.equal(plan_switch(), before), "the borrowed plan changed beside the hybrid object"
    hks.close()
    assert torch.equal(plan_switch(), before), "the borrowed plan changed after the hybrid object"
    plan.close()


@pytest.mark.parametrize("n", [16384, 32768])
def test_large_rings(hx, ctx, dev, orc, n):
    s = Setup(hx, ctx, orc, n, 3, 5, 2, orc.primes(5, 51, n))
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    run_keyswitch(hx, ctx, dev, s, keys, 3, 2, f"n = {n}")
    s.close()


def test_regrow_then_a_smaller_call(hx, ctx, dev, orc):
    """batch 2, then 5, then 3 on one object: the grow-only scratch and slice buffer at every size"""
    s = Setup(hx, ctx, orc, 1024, 3, 5, 2, orc.primes(5, 51, 1024))
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    for nb in (2, 5, 3):
        run_keyswitch(hx, ctx, dev, s, keys, 3, nb, f"batch {nb}", distinct=2)
    assert s.hks.scratch_bytes(5) == 5 * s.hks.scratch_bytes(1)
    s.close()


CHUNK_CASE = dict(n=1024, L=3, K=5, alpha=2, nb=5, distinct=3)


def chunk_calls(hx, ctx, dev, orc):
    """keyswitch, relinearize and rotate at batch 5 over three distinct instances -> {name: words}; the parent (one chunk) and the child
    (HEXL_KS_CHUNK=2: two chunks and a tail of one) run the same calls"""
    c = CHUNK_CASE
    s = Setup(hx, ctx, orc, c["n"], c["L"], c["K"], c["alpha"], orc.primes(c["K"], 51, c["n"]))
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    L, n, nb = c["L"], c["n"], c["nb"]
    ct3 = [s.words(3, L, b, 4) for b in range(c["distinct"])]
    tile = lambda parts, comps: np.stack([parts[b % c["distinct"]].reshape(-1)[:comps * L * n] for b in range(nb)])
    d_ct3 = up(hx, dev, tile(ct3, 3))
    d_ct = up(hx, dev, tile(ct3, 2))
    ks = up(hx, dev, tile(ct3, 2))
    s.hks.keyswitch(ks, up(hx, dev, np.stack([ct3[b % c["distinct"]].reshape(3, L, n)[2].reshape(-1) for b in range(nb)])), nb, L)
    relin, rot = minus_one(dev, nb * 2 * L * n), minus_one(dev, nb * 2 * L * n)
    s.hks.relinearize(relin, d_ct3, nb, L)
    s.hks.rotate(rot, d_ct, nb, L, 5)
    ctx.sync()
    res = {"ks": hx.to_u64(ks), "relin": hx.to_u64(relin), "rot": hx.to_u64(rot)}
    return s, keys, ct3, res


def test_two_scratch_chunks(hx, ctx, dev, orc, tmp_path):
    c = CHUNK_CASE
    s, keys, ct3, res = chunk_calls(hx, ctx, dev, orc)
    assert s.hks.scratch_bytes(2) < s.hks.scratch_bytes(5), "this process must run batch 5 in one chunk"
    L, n = c["L"], c["n"]
    want = [s.model.relinearize(keys, ct3[b], L) for b in range(c["distinct"])]
    assert_instances(res["relin"], want, c["nb"], NAMES, (2, L, n), "hexl_hks_relinearize, one chunk")
    assert np.array_equal(res["ks"], res["relin"]), "relinearize must be the key switch of component 2 added into components 0-1"
    want = [s.model.rotate(keys, ct3[b].reshape(-1)[:2 * L * n], L, 5) for b in range(c["distinct"])]
    assert_instances(res["rot"], want, c["nb"], NAMES, (2, L, n), "hexl_hks_rotate g = 5, one chunk")
    s.close()
    ref = tmp_path / "one_chunk.npz"
    np.savez(ref, **res)
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
from test_gpu_hks import chunk_calls
dev = torch.device("cuda:0")
ctx = hx.Context(0)
s, keys, ct3, res = chunk_calls(hx, ctx, dev, orc)
assert s.hks.scratch_bytes(2) == s.hks.scratch_bytes(100) > s.hks.scratch_bytes(1), "HEXL_KS_CHUNK=2 not in force"
want = np.load(%r)
for name in ("ks", "relin", "rot"):
    assert np.array_equal(res[name], want[name]), name + " differs from the one-chunk words"
s.close()
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"), str(ref))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="2"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_relinearize_and_rotate_at_two_levels(hx, ctx, dev, orc):
    n, L, K, alpha, batch = 1024, 4, 6, 2, 2
    s = Setup(hx, ctx, orc, n, L, K, alpha, orc.primes(K, 51, n))
    keys = s.keys()
    s.hks.set_keys_device(up(hx, dev, keys))
    for l in (4, 3):
        ct3 = [s.words(3, l, b, 6) for b in range(batch)]
        out = minus_one(dev, batch * 2 * l * n)
        s.hks.relinearize(out, up(hx, dev, np.stack(ct3)), batch, l)
        ctx.sync()
        assert_instances(hx.to_u64(out), [s.model.relinearize(keys, c, l) for c in ct3], batch, NAMES, (2, l, n), f"relinearize level {l}")
        cts = [c[:2 * l * n] for c in ct3]
        d_ct = up(hx, dev, np.stack(cts))
        for g in (5, 2 * n - 1, 1):
            out = minus_one(dev, batch * 2 * l * n)
            s.hks.rotate(out, d_ct, batch, l, g)
            ctx.sync()
            assert_instances(hx.to_u64(out), [s.model.rotate(keys, c, l, g) for c in cts], batch, NAMES, (2, l, n), f"rotate g = {g} level {l}")
        assert np.array_equal(hx.to_u64(d_ct), np.stack(cts).reshape(-1)), "the input was written"
    s.close()


def test_rekey_between_launches_without_a_synchronisation(hx, ctx, dev, orc):
    s = Setup(hx, ctx, orc, 1024, 3, 5, 2, orc.primes(5, 51, 1024))
    ka, kb = s.keys(0), s.keys(1)
    d_ka, d_kb = up(hx, dev, ka), up(hx, dev, kb)
    t, r = s.words(1, 3, 0, 1), s.words(2, 3, 0, 2)
    d_t, r1, r2 = up(hx, dev, t), up(hx, dev, r), up(hx, dev, r)
    s.hks.set_keys_device(d_ka)
    s.hks.keyswitch(r1, d_t, 1, 3)
    s.hks.set_keys_device(d_kb)
    s.hks.keyswitch(r2, d_t, 1, 3)
    ctx.sync()
    assert np.array_equal(hx.to_u64(r1), s.model.keyswitch(ka, t, r, 3)), "the first launch did not see the first key"
    assert np.array_equal(hx.to_u64(r2), s.model.keyswitch(kb, t, r, 3)), "the second launch did not see the second key"
    s.close()


def test_on_a_non_blocking_caller_stream(hx, dev, orc):
    torch = torch_()
    own = hx.Context(0, use_torch_stream=False)
    side = torch.cuda.Stream()
    own.set_stream(side.cuda_stream)
    s = Setup(hx, own, orc, 1024, 3, 5, 2, orc.primes(5, 51, 1024))
    keys = s.keys()
    d_keys = up(hx, dev, keys)
    ts, rs = [s.words(1, 3, b, 1) for b in range(2)], [s.words(2, 3, b, 2) for b in range(2)]
    d_t, d_r = up(hx, dev, np.stack(ts)), up(hx, dev, np.stack(rs))
    torch.cuda.synchronize()                                      # the uploads ran on torch's stream
    s.hks.set_keys_device(d_keys)
    s.hks.keyswitch(d_r, d_t, 2, 3)
    side.synchronize()
    assert_instances(hx.to_u64(d_r), [s.model.keyswitch(keys, ts[b], rs[b], 3) for b in range(2)], 2, NAMES, (2, 3, 1024), "side stream")
    own.use_own_stream()
    s.close()
    own.close()


def test_every_rejection(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K = 1024, 3, 5
    s = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))
    lib = hx.lib()
    out_h = ctypes.c_void_p()
    for alpha in (0, L + 1):
        assert lib.hexl_hks_create(s.plan.h, alpha, ctypes.byref(out_h)) == HEXL_E_BADARG and not out_h.value
    assert lib.hexl_hks_create(None, 1, ctypes.byref(out_h)) == HEXL_E_BADARG
    assert lib.hexl_hks_create(s.plan.h, 1, None) == HEXL_E_BADARG
    big = KsCase(orc, n, 2, 4, seed=3, bits=55)                   # a modulus >= 2^52: the plan runs the integer kernels
    iplan = hx.KeySwitchPlan(ctx, n, 2, 4, 4, 2, big.moduli, big.modswitch)
    assert lib.hexl_hks_create(iplan.h, 1, ctypes.byref(out_h)) == HEXL_E_BADARG
    iplan.close()
    t = torch.zeros(2 * L * n, dtype=torch.int64, device=dev)
    ct3 = torch.zeros(2 * 3 * L * n, dtype=torch.int64, device=dev)
    out = minus_one(dev, 2 * 2 * L * n)
    h, p = s.hks.h, lambda x: ctypes.c_void_p(x.data_ptr())
    for batch in (2, 0):
        # before an install: malformed arguments first, then HEXL_E_NOKEYS
        assert lib.hexl_hks_keyswitch(h, p(out), p(t), batch, L) == HEXL_E_NOKEYS
        assert lib.hexl_hks_relinearize(h, p(out), p(ct3), batch, L) == HEXL_E_NOKEYS
        assert lib.hexl_hks_rotate(h, p(out), p(ct3), batch, L, 5) == HEXL_E_NOKEYS
        assert lib.hexl_hks_keyswitch(None, p(out), p(t), batch, L) == HEXL_E_BADARG
        assert lib.hexl_hks_keyswitch(h, None, p(t), batch, L) == HEXL_E_BADARG
        assert lib.hexl_hks_keyswitch(h, p(out), None, batch, L) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize(h, None, p(ct3), batch, L) == HEXL_E_BADARG
        assert lib.hexl_hks_relinearize(h, p(out), None, batch, L) == HEXL_E_BADARG
        assert lib.hexl_hks_rotate(h, None, p(ct3), batch, L, 5) == HEXL_E_BADARG
        assert lib.hexl_hks_rotate(h, p(out), None, batch, L, 5) == HEXL_E_BADARG
        for l in (0, L + 1):
            assert lib.hexl_hks_keyswitch(h, p(out), p(t), batch, l) == HEXL_E_BADARG
            assert lib.hexl_hks_relinearize(h, p(out), p(ct3), batch, l) == HEXL_E_BADARG
            assert lib.hexl_hks_rotate(h, p(out), p(ct3), batch, l, 5) == HEXL_E_BADARG
        for g in (4, 2 * n, 2 * n + 1):
            assert lib.hexl_hks_rotate(h, p(out), p(ct3), batch, L, g) == HEXL_E_BADARG
        assert lib.hexl_hks_keyswitch(h, p(out), p(t), 1 << 62, L) == HEXL_E_BADARG            # a size that overflows
    assert lib.hexl_hks_keyswitch(h, p(ct3), p(ct3[n:]), 2, L) == HEXL_E_BADARG                # output overlapping input
    assert lib.hexl_hks_relinearize(h, p(ct3[n:]), p(ct3), 2, L) == HEXL_E_BADARG
    assert lib.hexl_hks_rotate(h, p(ct3), p(ct3), 2, L, 5) == HEXL_E_BADARG
    assert lib.hexl_hks_set_keys_device(h, None) == HEXL_E_BADARG and lib.hexl_hks_set_keys_device(None, p(t)) == HEXL_E_BADARG
    assert lib.hexl_hks_destroy(None) == HEXL_E_BADARG and lib.hexl_hks_scratch_bytes(None, 1) == 0
    ctx.sync()
    assert bool((out == -1).all()) and not bool(t.any()) and not bool(ct3.any()), "a refusal wrote something"
    s.hks.set_keys_device(up(hx, dev, s.keys()))
    assert lib.hexl_hks_keyswitch(h, p(out), p(t), 0, L) == 0 and lib.hexl_hks_rotate(h, p(out), p(ct3), 0, L, 5) == 0
    assert lib.hexl_hks_relinearize(h, p(out), p(ct3), 0, L) == 0
    ctx.sync()
    assert bool((out == -1).all()), "an empty batch wrote something"
    s.close()


@pytest.mark.parametrize("kind", ["square", "galois"])
def test_end_to_end_decrypts_within_the_noise_bound(hx, ctx, dev, orc, kind):
    """secret = hexl_sample(TERNARY) at K limbs; s' = s^2 (hexl_multiply_plain) or s(X^g) (hexl_apply_galois); gen_hybrid_key; then at
    every level l the switch of a uniform t -- relinearize of (0, 0, t), or rotate of (0, t) -- decrypts under s (hexl_rlwe_decrypt) to
    t s' (square) or sigma_g(t) s' (Galois) up to a noise whose centred CRT lift over the l limbs is within
    B = 21 n sum_d |G_d| D_d / P + (n_p + 1/2)(n + 1) (tests/hks_model.py noise_bound; CBD21 errors are at most 21, ||s||_1 <= n)."""
    torch = torch_()
    n, L, K, alpha, g = 1024, 4, 6, 2, 5
    s = Setup(hx, ctx, orc, n, L, K, alpha, orc.primes(K, 45, n))
    plan, qs = s.plan, s.qs
    seed = bytes((37 * k + 11) & 0xFF for k in range(32))
    sec = minus_one(dev, K * n)
    plan.sample(sec, hx.SAMPLE_TERNARY, 1, K, seed=seed, stream=1)
    s_from = minus_one(dev, K * n)
    if kind == "square":
        plan.multiply_plain(s_from, sec, sec, 1, 1, K, 1)
    else:
        ctx.apply_galois(s_from, sec, K, n, g)
    d_keys = minus_one(dev, s.model.dnum * 2 * K * n)
    plan.gen_hybrid_key(d_keys, sec, alpha, s_from, seed=seed, stream=2)
    s.hks.set_keys_device(d_keys)
    lm = Limbs(orc, n, qs)
    for l in range(L, 0, -1):
        t = np.stack([orc.splitmix(n, 31 + 7 * l + i, qs[i]) for i in range(l)])
        out = minus_one(dev, 2 * l * n)
        if kind == "square":
            ct3 = np.concatenate([np.zeros((2, l, n), dtype=np.uint64), t[None]])
            s.hks.relinearize(out, up(hx, dev, ct3), 1, l)
            moved = t
        else:
            s.hks.rotate(out, up(hx, dev, np.concatenate([np.zeros((1, l, n), dtype=np.uint64), t[None]])), 1, l, g)
            moved = apply_galois(t, n, g)
        dec, exp = minus_one(dev, l * n), minus_one(dev, l * n)
        plan.rlwe_decrypt(dec, out, sec, 1, 2, l)
        plan.multiply_plain(exp, up(hx, dev, moved), s_from, 1, 1, l, 1)
        ctx.sync()
        got, want = hx.to_u64(dec).reshape(l, n), hx.to_u64(exp).reshape(l, n)
        Q = 1
        for q in qs[:l]:
            Q *= q
        acc = np.zeros(n, dtype=object)
        for i in range(l):
            q = qs[i]
            c = lm.intt(np.array((got[i].astype(object) - want[i].astype(object)) % q, dtype=np.uint64), i).astype(object)
            acc = acc + c * ((Q // q) * pow(Q // q, -1, q))
        worst = max(min(int(v), Q - int(v)) for v in acc % Q)
        B = s.model.noise_bound(l)
        print(f"[hks] {kind} level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"{kind} level {l}: {worst} > {B}"
    s.close()
