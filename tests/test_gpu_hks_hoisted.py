"""GPU: hexl_hks_rotate_hoisted and hexl_hks_linear_transform bit-exact against tests/hks_hoisted_model.py, every word of every instance,
every output pre-filled with -1 (WRITTEN, and nothing written on a refusal): n = 1024 with L = 4, alpha = 2, K = 6 at l = 4 and l = 3 (a
ragged last digit) on uniform and extreme words, keys and plaintexts, g = 5, 2n - 1, 1 and a repeated g through a repeated object, the
identity term, the word identities of the header (g = 1 against hexl_hks_rotate, one all-ones plaintext against the hoisted call, alpha = 1
against hexl_rotate_hoisted / hexl_linear_transform on per-limb plans keyed from the same device buffers), a mixed-tier chain, n = 16384
and n = 32768, two scratch chunks (a child process with HEXL_KS_CHUNK), a regrow followed by a smaller call, a plain hexl_hks_rotate
between two hoisted calls, a non-blocking caller stream, every rejection, and end to end: gen_hybrid_key (Galois) for two elements ->
hexl_hks_linear_transform -> hexl_rlwe_decrypt within B_lt (hks_hoisted_model.lt_noise_bound)."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hks_hoisted_model as model
from ckks_model import Limbs, apply_galois
from ks_util import KsCase, extreme_words, seal_chain
from rns_model import assert_instances
from test_gpu_hks import NAMES, Setup, minus_one, torch_, up

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG, HEXL_E_NOKEYS = -1, -2


class Rig:
    """R hybrid objects on ONE plan (the first is Setup's), each with keys of its own installed"""

    def __init__(self, hx, ctx, dev, orc, n, L, K, alpha, moduli, R, family="uniform"):
        self.s = Setup(hx, ctx, orc, n, L, K, alpha, moduli, family)
        self.objs = [self.s.hks] + [hx.HybridKeySwitch(self.s.plan, alpha) for _ in range(R - 1)]
        self.keys = [self.s.keys(r) for r in range(R)]
        for o, k in zip(self.objs, self.keys):
            o.set_keys_device(up(hx, dev, k))
        self.n, self.L, self.K, self.model, self.family, self.orc = n, L, K, self.s.model, family, orc

    def plaintext(self, salt, rows=None):
        rows = self.K if rows is None else rows
        if self.family == "extreme":
            return np.stack([extreme_words(self.n, self.s.qs[i], salt + 2 * i) for i in range(rows)])
        return np.stack([self.orc.splitmix(self.n, 7000 + salt * 131 + i, self.s.qs[i]) for i in range(rows)])

    def cts(self, l, distinct, salt):
        return [self.s.words(2, l, b, salt) for b in range(distinct)]

    def close(self):
        for o in reversed(self.objs[1:]):
            o.close()
        self.s.close()


def tiled(hx, dev, cts, nb):
    return up(hx, dev, np.stack([cts[b % len(cts)] for b in range(nb)]))


def run_hoisted(hx, ctx, dev, rig, picks, gs, l, nb, cts, label, want=None):
    """the hoisted call with object rig.objs[picks[r]] for rotation r against the model; returns (outputs, expected words)"""
    m, n = rig.model, rig.n
    if want is None:
        exts = [m.mod_up(ct.reshape(2, l, n)[1], l) for ct in cts]
        want = [[model.rotate_hoisted(m, rig.keys[p], ct, l, g, e) for ct, e in zip(cts, exts)] for p, g in zip(picks, gs)]
    d_ct = tiled(hx, dev, cts, nb)
    outs = [minus_one(dev, nb * 2 * l * n) for _ in gs]
    hx.hks_rotate_hoisted([rig.objs[p] for p in picks], gs, outs, d_ct, nb, l)
    ctx.sync()
    for r, out in enumerate(outs):
        assert_instances(hx.to_u64(out), want[r], nb, NAMES, (2, l, n), f"{label}, rotation {r} (g = {gs[r]})")
    assert np.array_equal(hx.to_u64(d_ct), np.stack([cts[b % len(cts)] for b in range(nb)]).reshape(-1)), "the input was written"
    return outs, want, d_ct


def run_transform(hx, ctx, dev, rig, picks, gs, pts, pt_id, l, nb, cts, label, want=None):
    m, n = rig.model, rig.n
    if want is None:
        want = [model.linear_transform(m, [rig.keys[p] for p in picks], gs, pts, pt_id, ct, l) for ct in cts]
    d_ct = tiled(hx, dev, cts, nb)
    out = minus_one(dev, nb * 2 * l * n)
    d_pts = [up(hx, dev, p) for p in pts]
    d_id = None if pt_id is None else up(hx, dev, pt_id)
    hx.hks_linear_transform([rig.objs[p] for p in picks], gs, d_pts, d_id, out, d_ct, nb, l)
    ctx.sync()
    assert_instances(hx.to_u64(out), want, nb, NAMES, (2, l, n), label)
    return out, want, d_ct


@pytest.mark.parametrize("l", [4, 3])
@pytest.mark.parametrize("family", ["uniform", "extreme"])
def test_hoisted_smallest_ring(hx, ctx, dev, orc, family, l):
    """g = 5, 2n - 1, 1, and g = 5 once more through the first object again; the g = 1 output is hexl_hks_rotate's word for word"""
    n, nb = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 4, 6, 2, orc.primes(6, 51, n), 3, family)
    outs, _, d_ct = run_hoisted(hx, ctx, dev, rig, [0, 1, 2, 0], [5, 2 * n - 1, 1, 5], l, nb, rig.cts(l, nb, 3), f"hoisted {family} level {l}")
    plain = minus_one(dev, nb * 2 * l * n)
    rig.objs[2].rotate(plain, d_ct, nb, l, 1)
    ctx.sync()
    assert torch_().equal(plain, outs[2]), "g = 1: the hoisted rotation must be hexl_hks_rotate word for word"
    assert torch_().equal(outs[0], outs[3]), "a repeated object with a repeated g must repeat its words"
    assert rig.objs[0].hoisted_scratch_bytes(1) == rig.objs[0].scratch_bytes(1) + 4 * n * 8
    rig.close()


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("family", ["uniform", "extreme"])
def test_transform_smallest_ring(hx, ctx, dev, orc, family, identity):
    n, nb = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 4, 6, 2, orc.primes(6, 51, n), 3, family)
    gs = [5, 2 * n - 1, 1]
    pts = [rig.plaintext(1 + r) for r in range(3)]
    for l in (4, 3):
        pt_id = rig.plaintext(9, rows=l) if identity else None
        run_transform(hx, ctx, dev, rig, [0, 1, 2], gs, pts, pt_id, l, nb, rig.cts(l, 2, 5), f"transform {family} identity {identity} level {l}")
    rig.close()


@pytest.mark.parametrize("l", [4, 3])
def test_one_all_ones_plaintext_is_the_hoisted_call(hx, ctx, dev, orc, l):
    n, nb = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 4, 6, 2, orc.primes(6, 51, n), 1)
    d_ct = tiled(hx, dev, rig.cts(l, nb, 7), nb)
    ones = up(hx, dev, model.ones_plaintext(rig.model))
    for g in (5, 1):
        a, b = minus_one(dev, nb * 2 * l * n), minus_one(dev, nb * 2 * l * n)
        hx.hks_rotate_hoisted(rig.objs, [g], [a], d_ct, nb, l)
        hx.hks_linear_transform(rig.objs, [g], [ones], None, b, d_ct, nb, l)
        ctx.sync()
        assert torch_().equal(a, b), f"g = {g}: one rotation weighted by ones must be hexl_hks_rotate_hoisted's words"
    rig.close()


def test_mixed_tier_chain(hx, ctx, dev, orc):
    """52, 30, 30, 40, 27-bit data limbs and two 27-bit special primes: every transform on its own limb's tier"""
    n, L, K, l = 1024, 5, 7, 5
    rig = Rig(hx, ctx, dev, orc, n, L, K, 2, seal_chain(orc, K, n), 2, "extreme")
    tiers, mixed = rig.s.plan.tiers()
    assert mixed and tiers[0] == 0 and all(t != 0 for t in tiers[1:]), tiers
    gs = [5, 2 * n - 1]
    cts = rig.cts(l, 2, 11)
    run_hoisted(hx, ctx, dev, rig, [0, 1], gs, l, 2, cts, "hoisted, mixed tiers")
    run_transform(hx, ctx, dev, rig, [0, 1], gs, [rig.plaintext(3), rig.plaintext(4)], rig.plaintext(6, rows=l), l, 2, cts, "transform, mixed tiers")
    rig.close()


@pytest.mark.parametrize("L", [2, 3])
def test_alpha_one_is_the_per_limb_calls_on_the_same_key_buffers(hx, ctx, dev, orc, L):
    """alpha = 1, K = L + 1, n_limbs = L: hexl_rotate_hoisted / hexl_linear_transform on per-limb plans that install the SAME device key
    buffers give the same words; [K][n] plaintexts are [L + 1][n]"""
    torch = torch_()
    n, nb, K = 1024, 3, L + 1
    gs = [5, 2 * n - 1]
    cases = [KsCase(orc, n, L, K, seed=5 + r) for r in range(2)]
    plans = [hx.KeySwitchPlan(ctx, n, L, K, K, 2, c.moduli, c.modswitch) for c in cases]
    objs = [hx.HybridKeySwitch(plans[0], 1) for _ in cases]
    d_keys = [up(hx, dev, np.concatenate(c.keys)) for c in cases]
    for p, o, k in zip(plans, objs, d_keys):
        p.set_keys_device(k)
        o.set_keys_device(k)
    qs = [int(q) for q in cases[0].moduli]
    d_ct = up(hx, dev, np.stack([np.concatenate([orc.splitmix(n, 300 + b * 31 + k * 7 + i, qs[i]) for k in range(2) for i in range(L)])
                                 for b in range(nb)]))
    d_pts = [up(hx, dev, np.stack([orc.splitmix(n, 500 + r * 13 + i, qs[i]) for i in range(K)])) for r in range(2)]
    d_id = up(hx, dev, np.stack([orc.splitmix(n, 700 + i, qs[i]) for i in range(L)]))
    fresh = lambda: minus_one(dev, nb * 2 * L * n)
    a, b = [fresh(), fresh()], [fresh(), fresh()]
    hx.rotate_hoisted(plans, gs, a, d_ct, nb)
    hx.hks_rotate_hoisted(objs, gs, b, d_ct, nb, L)
    ctx.sync()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "alpha = 1, K = L + 1 must be hexl_rotate_hoisted word for word"
    for pid in (None, d_id):
        x, y = fresh(), fresh()
        hx.linear_transform(plans, gs, d_pts, x, d_ct, nb, pid)
        hx.hks_linear_transform(objs, gs, d_pts, pid, y, d_ct, nb, L)
        ctx.sync()
        assert torch.equal(x, y), f"alpha = 1, K = L + 1 must be hexl_linear_transform word for word (identity {pid is not None})"
    for o in reversed(objs):
        o.close()
    for p in reversed(plans):
        p.close()


@pytest.mark.parametrize("n", [16384, 32768])
def test_large_rings(hx, ctx, dev, orc, n):
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 2)
    gs = [pow(5, 3, 2 * n), 2 * n - 1]
    cts = rig.cts(3, 2, 13)
    run_hoisted(hx, ctx, dev, rig, [0, 1], gs, 3, 2, cts, f"hoisted n = {n}")
    run_transform(hx, ctx, dev, rig, [0, 1], gs, [rig.plaintext(1), rig.plaintext(2)], rig.plaintext(3, rows=3), 3, 2, cts, f"transform n = {n}")
    rig.close()


CHUNK_CASE = dict(n=1024, L=3, K=5, alpha=2, nb=5, distinct=3, gs=[5, 2047])


def chunk_calls(hx, ctx, dev, orc):
    """both calls at batch 5 over three distinct instances -> (rig, inputs, {name: words}); the parent (one chunk) and the child
    (HEXL_KS_CHUNK=2: two chunks and a tail of one) run the same calls"""
    c = CHUNK_CASE
    rig = Rig(hx, ctx, dev, orc, c["n"], c["L"], c["K"], c["alpha"], orc.primes(c["K"], 51, c["n"]), 2)
    L, n, nb = c["L"], c["n"], c["nb"]
    cts = rig.cts(L, c["distinct"], 4)
    pts = [rig.plaintext(1), rig.plaintext(2)]
    pt_id = rig.plaintext(3, rows=L)
    d_ct = tiled(hx, dev, cts, nb)
    outs = [minus_one(dev, nb * 2 * L * n) for _ in range(3)]
    hx.hks_rotate_hoisted(rig.objs, c["gs"], outs[:2], d_ct, nb, L)
    hx.hks_linear_transform(rig.objs, c["gs"], [up(hx, dev, p) for p in pts], up(hx, dev, pt_id), outs[2], d_ct, nb, L)
    ctx.sync()
    return rig, (cts, pts, pt_id), {"rot0": hx.to_u64(outs[0]), "rot1": hx.to_u64(outs[1]), "lt": hx.to_u64(outs[2])}


def test_two_scratch_chunks(hx, ctx, dev, orc, tmp_path):
    """the extended digits of chunk 1 are chunk 1's, not left over from chunk 0"""
    c = CHUNK_CASE
    rig, (cts, pts, pt_id), res = chunk_calls(hx, ctx, dev, orc)
    assert rig.objs[0].scratch_bytes(2) < rig.objs[0].scratch_bytes(5), "this process must run batch 5 in one chunk"
    L, n, m = c["L"], c["n"], rig.model
    for r, g in enumerate(c["gs"]):
        want = [model.rotate_hoisted(m, rig.keys[r], ct, L, g) for ct in cts]
        assert_instances(res[f"rot{r}"], want, c["nb"], NAMES, (2, L, n), f"hoisted g = {g}, one chunk")
    want = [model.linear_transform(m, rig.keys, c["gs"], pts, pt_id, ct, L) for ct in cts]
    assert_instances(res["lt"], want, c["nb"], NAMES, (2, L, n), "transform, one chunk")
    rig.close()
    ref = tmp_path / "one_chunk.npz"
    np.savez(ref, **res)
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
from test_gpu_hks_hoisted import chunk_calls
dev = torch.device("cuda:0")
ctx = hx.Context(0)
rig, _, res = chunk_calls(hx, ctx, dev, orc)
h = rig.objs[0]
assert h.hoisted_scratch_bytes(2) == h.hoisted_scratch_bytes(100) > h.hoisted_scratch_bytes(1), "HEXL_KS_CHUNK=2 not in force"
want = np.load(%r)
for name in ("rot0", "rot1", "lt"):
    assert np.array_equal(res[name], want[name]), name + " differs from the one-chunk words"
rig.close()
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"), str(ref))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="2"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_regrow_then_a_smaller_call(hx, ctx, dev, orc):
    """batch 2, then 5, then 3 on one set of objects: the grow-only scratch and the w buffer at every size"""
    n, l = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 2)
    gs = [5, 2 * n - 1]
    cts = rig.cts(l, 2, 8)
    pts = [rig.plaintext(1), rig.plaintext(2)]
    want_rot = want_lt = None
    for nb in (2, 5, 3):
        _, want_rot, _ = run_hoisted(hx, ctx, dev, rig, [0, 1], gs, l, nb, cts, f"hoisted batch {nb}", want_rot)
        _, want_lt, _ = run_transform(hx, ctx, dev, rig, [0, 1], gs, pts, None, l, nb, cts, f"transform batch {nb}", want_lt)
    assert rig.objs[0].hoisted_scratch_bytes(5) == 5 * rig.objs[0].hoisted_scratch_bytes(1)
    rig.close()


def test_a_plain_rotate_between_two_hoisted_calls(hx, ctx, dev, orc):
    """hexl_hks_rotate puts w of component 1 into the extended block, the hoisted call into a buffer of its own: neither disturbs the other"""
    n, l, nb = 1024, 3, 2
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 2)
    gs = [5, 2 * n - 1]
    cts = rig.cts(l, nb, 9)
    d_ct = tiled(hx, dev, cts, nb)
    first = [minus_one(dev, nb * 2 * l * n) for _ in gs]
    again = [minus_one(dev, nb * 2 * l * n) for _ in gs]
    plain = minus_one(dev, nb * 2 * l * n)
    hx.hks_rotate_hoisted(rig.objs, gs, first, d_ct, nb, l)
    rig.objs[0].rotate(plain, d_ct, nb, l, 5)
    hx.hks_rotate_hoisted(rig.objs, gs, again, d_ct, nb, l)
    ctx.sync()
    m = rig.model
    for r, g in enumerate(gs):
        want = [model.rotate_hoisted(m, rig.keys[r], ct, l, g) for ct in cts]
        assert_instances(hx.to_u64(first[r]), want, nb, NAMES, (2, l, n), f"first hoisted call, g = {g}")
        assert_instances(hx.to_u64(again[r]), want, nb, NAMES, (2, l, n), f"hoisted call after a plain rotate, g = {g}")
    assert_instances(hx.to_u64(plain), [m.rotate(rig.keys[0], ct, l, 5) for ct in cts], nb, NAMES, (2, l, n), "hexl_hks_rotate between them")
    rig.close()


def test_on_a_non_blocking_caller_stream(hx, dev, orc):
    torch = torch_()
    n, l, nb = 1024, 3, 2
    own = hx.Context(0, use_torch_stream=False)
    side = torch.cuda.Stream()
    own.set_stream(side.cuda_stream)
    s = Setup(hx, own, orc, n, 3, 5, 2, orc.primes(5, 51, n))
    second = hx.HybridKeySwitch(s.plan, 2)
    keys = [s.keys(0), s.keys(1)]
    d_keys = [up(hx, dev, k) for k in keys]
    gs = [5, 2 * n - 1]
    cts = [s.words(2, l, b, 2) for b in range(nb)]
    pts = [np.stack([orc.splitmix(n, 800 + r * 11 + i, s.qs[i]) for i in range(5)]) for r in range(2)]
    d_ct, d_pts = up(hx, dev, np.stack(cts)), [up(hx, dev, p) for p in pts]
    outs = [minus_one(dev, nb * 2 * l * n) for _ in range(3)]
    torch.cuda.synchronize()                                      # the uploads ran on torch's stream
    s.hks.set_keys_device(d_keys[0])
    second.set_keys_device(d_keys[1])
    hx.hks_rotate_hoisted([s.hks, second], gs, outs[:2], d_ct, nb, l)
    hx.hks_linear_transform([s.hks, second], gs, d_pts, None, outs[2], d_ct, nb, l)
    side.synchronize()
    for r, g in enumerate(gs):
        assert_instances(hx.to_u64(outs[r]), [model.rotate_hoisted(s.model, keys[r], ct, l, g) for ct in cts], nb, NAMES, (2, l, n),
                         f"side stream, hoisted g = {g}")
    assert_instances(hx.to_u64(outs[2]), [model.linear_transform(s.model, keys, gs, pts, None, ct, l) for ct in cts], nb, NAMES, (2, l, n),
                     "side stream, transform")
    own.use_own_stream()
    second.close()
    s.close()
    own.close()


def test_every_rejection(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K, nb = 1024, 3, 5, 2
    s = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))
    second = hx.HybridKeySwitch(s.plan, 2)                        # no keys yet
    other_alpha = hx.HybridKeySwitch(s.plan, 1)
    t = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))      # the same shape on ANOTHER plan
    for o in (s.hks, other_alpha, t.hks):
        o.set_keys_device(up(hx, dev, s.keys()))
    lib = hx.lib()
    words = nb * 2 * L * n
    ct = torch.zeros(words, dtype=torch.int64, device=dev)
    pts = [torch.zeros(K * n, dtype=torch.int64, device=dev) for _ in range(2)]
    pt_id = torch.zeros(L * n, dtype=torch.int64, device=dev)
    outs = [minus_one(dev, words) for _ in range(2)]
    big = minus_one(dev, 2 * words)
    H = lambda *objs: hx._handles(list(objs))
    G = lambda *gs: hx._u64_array(list(gs))
    P = lambda *ts: (ctypes.c_void_p * len(ts))(*[None if x is None else x.data_ptr() for x in ts])
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rot, lt = lib.hexl_hks_rotate_hoisted, lib.hexl_hks_linear_transform
    ok_h, ok_g = H(s.hks, second), G(5, 3)
    for batch in (nb, 0):
        # everything well-formed but the second object's keys: malformed arguments first, then HEXL_E_NOKEYS
        assert rot(ok_h, ok_g, 2, P(*outs), p(ct), batch, L) == HEXL_E_NOKEYS
        assert lt(ok_h, ok_g, P(*pts), 2, p(pt_id), p(outs[0]), p(ct), batch, L) == HEXL_E_NOKEYS
        # null arguments and entries
        assert rot(None, ok_g, 2, P(*outs), p(ct), batch, L) == HEXL_E_BADARG
        assert rot(ok_h, None, 2, P(*outs), p(ct), batch, L) == HEXL_E_BADARG
        assert rot(ok_h, ok_g, 2, None, p(ct), batch, L) == HEXL_E_BADARG
        assert rot(ok_h, ok_g, 2, P(*outs), None, batch, L) == HEXL_E_BADARG
        assert rot(H(s.hks, None), ok_g, 2, P(*outs), p(ct), batch, L) == HEXL_E_BADARG
        assert rot(ok_h, ok_g, 2, P(outs[0], None), p(ct), batch, L) == HEXL_E_BADARG
        assert lt(None, ok_g, P(*pts), 2, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG
        assert lt(ok_h, None, P(*pts), 2, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG
        assert lt(ok_h, ok_g, None, 2, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG
        assert lt(ok_h, ok_g, P(*pts), 2, None, None, p(ct), batch, L) == HEXL_E_BADARG
        assert lt(ok_h, ok_g, P(*pts), 2, None, p(outs[0]), None, batch, L) == HEXL_E_BADARG
        assert lt(H(None, second), ok_g, P(*pts), 2, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG
        assert lt(ok_h, ok_g, P(pts[0], None), 2, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG
        assert lt(ok_h, ok_g, P(*pts), 0, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG      # no rotation at all
        # objects that do not share hks[0]'s plan and alpha
        for stranger in (t.hks, other_alpha):
            assert rot(H(s.hks, stranger), ok_g, 2, P(*outs), p(ct), batch, L) == HEXL_E_BADARG
            assert lt(H(s.hks, stranger), ok_g, P(*pts), 2, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG
        for l in (0, L + 1):
            assert rot(ok_h, ok_g, 2, P(*outs), p(ct), batch, l) == HEXL_E_BADARG
            assert lt(ok_h, ok_g, P(*pts), 2, None, p(outs[0]), p(ct), batch, l) == HEXL_E_BADARG
        for g in (4, 2 * n, 2 * n + 1):
            assert rot(ok_h, G(5, g), 2, P(*outs), p(ct), batch, L) == HEXL_E_BADARG
            assert lt(ok_h, G(g, 5), P(*pts), 2, None, p(outs[0]), p(ct), batch, L) == HEXL_E_BADARG
        assert rot(ok_h, ok_g, 2, P(*outs), p(ct), 1 << 62, L) == HEXL_E_BADARG                     # a size that overflows
        assert lt(ok_h, ok_g, P(*pts), 2, None, p(outs[0]), p(ct), 1 << 62, L) == HEXL_E_BADARG
    # overlaps (at the real batch): an output with d_ct, with another output, with a plaintext, with the identity plaintext
    assert rot(ok_h, ok_g, 2, P(outs[0], big[n:]), p(big), nb, L) == HEXL_E_BADARG
    assert rot(ok_h, ok_g, 2, P(big, big[n:]), p(ct), nb, L) == HEXL_E_BADARG
    assert lt(ok_h, ok_g, P(*pts), 2, None, p(big[n:]), p(big), nb, L) == HEXL_E_BADARG
    assert lt(ok_h, ok_g, P(pts[0], big[words - n:]), 2, None, p(big), p(ct), nb, L) == HEXL_E_BADARG
    assert lt(ok_h, ok_g, P(*pts), 2, p(big[words - n:]), p(big), p(ct), nb, L) == HEXL_E_BADARG
    assert lib.hexl_hks_hoisted_scratch_bytes(None, 1) == 0
    ctx.sync()
    clean = lambda: all(bool((o == -1).all()) for o in outs + [big]) and not bool(ct.any()) and not any(bool(x.any()) for x in pts + [pt_id])
    assert clean(), "a refusal wrote something"
    second.set_keys_device(up(hx, dev, s.keys(1)))
    assert rot(ok_h, ok_g, 2, P(*outs), p(ct), 0, L) == 0 and lt(ok_h, ok_g, P(*pts), 2, p(pt_id), p(outs[0]), p(ct), 0, L) == 0
    assert rot(ok_h, ok_g, 0, P(*outs), p(ct), nb, L) == 0                                          # no rotation: nothing to do
    ctx.sync()
    assert clean(), "an empty batch or an empty list of rotations wrote something"
    for o in (other_alpha, second):
        o.close()
    t.close()
    s.close()


def test_end_to_end_decrypts_within_the_noise_bound(hx, ctx, dev, orc):
    """secret = hexl_sample(TERNARY) at K limbs; for g in {5, 2n - 1} s_g = s(X^g) (hexl_apply_galois) and gen_hybrid_key from s_g to s on an
    object of its own; a uniform ciphertext (c0, c1) at l = L and l = L - 1; dense plaintexts with |coefficient| <= 8 encoded modulo all
    K limbs, and an identity term. hexl_rlwe_decrypt of the transform's output equals sum_r pt_r sigma_r(c0 + c1 s) + pt_id (c0 + c1 s)
    up to a noise whose centred CRT lift over the l limbs is within B_lt (hks_hoisted_model.lt_noise_bound: CBD21 errors, ||s||_1 <= n)."""
    n, L, K, alpha = 1024, 4, 6, 2
    gs = [5, 2 * n - 1]
    s = Setup(hx, ctx, orc, n, L, K, alpha, orc.primes(K, 45, n))
    objs = [s.hks, hx.HybridKeySwitch(s.plan, alpha)]
    plan, qs, m = s.plan, s.qs, s.model
    seed = bytes((41 * k + 5) & 0xFF for k in range(32))
    sec = minus_one(dev, K * n)
    plan.sample(sec, hx.SAMPLE_TERNARY, 1, K, seed=seed, stream=1)
    for r, g in enumerate(gs):
        s_from = minus_one(dev, K * n)
        ctx.apply_galois(s_from, sec, K, n, g)
        d_keys = minus_one(dev, m.dnum * 2 * K * n)
        plan.gen_hybrid_key(d_keys, sec, alpha, s_from, seed=seed, stream=2 + r)
        objs[r].set_keys_device(d_keys)
    rng = np.random.default_rng(5)
    polys = [rng.integers(-8, 9, n) for _ in gs]
    pts = [model.encode_small(m, poly) for poly in polys]
    pt_id = model.encode_small(m, rng.integers(-8, 9, n))
    d_pts, d_id = [up(hx, dev, x) for x in pts], up(hx, dev, pt_id)
    lm = Limbs(orc, n, qs)
    for l in (L, L - 1):
        ct = s.words(2, l, 0, 20 + l)
        d_ct, out = up(hx, dev, ct), minus_one(dev, 2 * l * n)
        hx.hks_linear_transform(objs, gs, d_pts, d_id, out, d_ct, 1, l)
        dec, dec_in = minus_one(dev, l * n), minus_one(dev, l * n)
        plan.rlwe_decrypt(dec, out, sec, 1, 2, l)
        plan.rlwe_decrypt(dec_in, d_ct, sec, 1, 2, l)
        ctx.sync()
        got, msg = hx.to_u64(dec).reshape(l, n), hx.to_u64(dec_in).reshape(l, n)
        Q = 1
        for q in qs[:l]:
            Q *= q
        acc = np.zeros(n, dtype=object)
        for i in range(l):
            q = qs[i]
            want = pt_id[i].astype(object) * msg[i].astype(object)
            for g, pt in zip(gs, pts):
                want = want + pt[i].astype(object) * apply_galois(msg[i], n, g).astype(object)
            c = lm.intt(np.array((got[i].astype(object) - want) % q, dtype=np.uint64), i).astype(object)
            acc = acc + c * ((Q // q) * pow(Q // q, -1, q))
        worst = max(min(int(v), Q - int(v)) for v in acc % Q)
        B = model.lt_noise_bound(m, l, [int(np.abs(poly).sum()) for poly in polys])
        print(f"[hks hoisted] linear transform level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"level {l}: {worst} > {B}"
    objs[1].close()
    s.close()
