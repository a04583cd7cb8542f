"""GPU: hexl_hks_linear_transform_bsgs bit for bit, every word of every instance, every output pre-filled with -1 behind a guard row:
against the exact model (tests/hks_bsgs_model.py, pinned in test_hks_bsgs_model.py) and against the DEVICE composition the header fixes the
output by -- hexl_hks_linear_transform per row, hexl_hks_rotate_hoisted with one rotation, a modular add on the host -- which does not
involve the model. n = 1024 with L = 4, alpha = 2, K = 6 at l = 4 and l = 3 on uniform and extreme words, keys and plaintexts (three grids:
G = 1 first, second and in the middle; G in {1, 3, 2n - 1}; NULL entries, an unused column, identity-only rows, a repeated object), a
mixed-tier chain at l = 5 and l = 2, one digit, one special prime, alpha = 1 against hexl_linear_transform_bsgs on per-limb plans keyed from
the same device buffers, n = 2048, 16384 and 32768, two scratch chunks with a ragged tail (a child process with HEXL_KS_CHUNK) followed by a
smaller call and the three sibling calls, batches 2, 5, 3 on one set of objects, a non-blocking caller stream, every rejection, the
reported scratch size, and end to end: gen_hybrid_key (Galois) -> this call -> hexl_rlwe_decrypt within B_bsgs. No tolerance anywhere but
in that last case."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hks_bsgs_model as model
import hks_hoisted_model as hoisted
from ckks_model import Limbs, apply_galois
from ks_util import KsCase, seal_chain
from rns_model import assert_instances
from test_gpu_hks import NAMES, Setup, minus_one, torch_, up
from test_gpu_hks_hoisted import Rig, tiled

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG, HEXL_E_NOKEYS = -1, -2


def grid_of(rig, name):
    """(baby picks, baby elements, giant picks, giant elements, pts, pt_ids); a pick is an index into rig.objs / rig.keys or None.
    2x2: G = 1 FIRST (t_0 computed in place in d_out), 125 as a giant step.
    3x2: the shape of test_hks_bsgs_model.GRIDS["3x2"]: a NULL entry, a column no row uses (no object), a row of identity only,
         G = 1 NOT first, 25 as a baby and as a giant step (different keys).
    2x3: ONE object for both baby steps (a repeated object), G = 3, 1, 2n - 1 with one object for both rotated giant steps, G = 1 in
         the middle with a full row, a NULL entry in a used column, an identity term on a row that has plaintexts."""
    n, pt = rig.n, rig.plaintext
    if name == "2x2":
        return [0, 1], [5, 25], [None, 2], [1, 125], [[pt(0), pt(1)], [pt(2), pt(3)]], None
    if name == "3x2":
        return [0, None, 1], [25, 5, 2 * n - 1], [2, None], [25, 1], [[pt(0), None, pt(1)], [None, None, None]], [pt(5, rows=rig.L), pt(6, rows=rig.L)]
    return [0, 0], [5, 7], [1, None, 1], [3, 1, 2 * n - 1], [[pt(0), pt(1)], [pt(2), pt(3)], [None, pt(4)]], [None, pt(5, rows=rig.L), None]


def expected(rig, g, l, cts):
    bp, bgs, gp, ggs, pts, ids = g
    keys = lambda picks: [None if p is None else rig.keys[p] for p in picks]
    return [model.linear_transform_bsgs(rig.model, keys(bp), bgs, keys(gp), ggs, pts, ids, ct, l) for ct in cts]


def device_grid(hx, dev, rig, g):
    """the objects and the uploaded plaintexts of a grid: (baby objects, giant objects, d_pts, d_ids)"""
    bp, _, gp, _, pts, ids = g
    obj = lambda picks: [None if p is None else rig.objs[p] for p in picks]
    d = lambda x: None if x is None else up(hx, dev, x)
    return obj(bp), obj(gp), [[d(x) for x in row] for row in pts], None if ids is None else [d(x) for x in ids]


def guarded(dev, words, n):
    """an output of `words` words and a guard row of n behind it, all -1"""
    buf = minus_one(dev, words + n)
    return buf, buf[:words]


def call(hx, ctx, dev, rig, g, dg, l, nb, d_ct):
    n = rig.n
    buf, out = guarded(dev, nb * 2 * l * n, n)
    hx.hks_linear_transform_bsgs(dg[0], g[1], dg[1], g[3], dg[2], dg[3], out, d_ct, nb, l)
    ctx.sync()
    assert bool((buf[nb * 2 * l * n:] == -1).all()), "the guard row behind the output was written"
    assert not bool((out == -1).any()), "a word of the output was not written"
    return out


def run_bsgs(hx, ctx, dev, rig, g, l, nb, cts, label, want=None, compose=False, dg=None):
    """the call against the model (want: its words per distinct ciphertext; False: no model) and, when asked, the device composition"""
    n = rig.n
    dg = dg or device_grid(hx, dev, rig, g)
    d_ct = tiled(hx, dev, cts, nb)
    out = call(hx, ctx, dev, rig, g, dg, l, nb, d_ct)
    if want is None:
        want = expected(rig, g, l, cts)
    if want is not False:
        assert_instances(hx.to_u64(out), want, nb, NAMES, (2, l, n), label)
    if compose:
        comp = device_composition(hx, ctx, dev, rig, g, dg, d_ct, nb, l)
        assert_instances(hx.to_u64(out), list(comp), nb, NAMES, (2, l, n), label + ", against the device composition")
    assert np.array_equal(hx.to_u64(d_ct), np.stack([cts[b % len(cts)] for b in range(nb)]).reshape(-1)), "the input was written"
    return out, want


def device_composition(hx, ctx, dev, rig, g, dg, d_ct, nb, l):
    """the header's definition on the device: hexl_hks_linear_transform per row (an identity-only row: the word product on the host),
    hexl_hks_rotate_hoisted with one rotation, the modular sum on the host. Returns uint64 [nb][2 l n]."""
    _, bgs, _, ggs, _, _ = g
    bobjs, gobjs, d_pts, d_ids = dg
    n = rig.n
    q = np.array(rig.s.qs[:l], dtype=np.uint64).reshape(1, 1, l, 1)
    total = np.zeros((nb, 2, l, n), dtype=np.uint64)
    for j, G in enumerate(ggs):
        used = [i for i, p in enumerate(d_pts[j]) if p is not None]
        d_id = None if d_ids is None else d_ids[j]
        if used:
            t = minus_one(dev, nb * 2 * l * n)
            hx.hks_linear_transform([bobjs[i] for i in used], [bgs[i] for i in used], [d_pts[j][i] for i in used], d_id, t, d_ct, nb, l)
        else:
            c = hx.to_u64(d_ct).reshape(nb, 2, l, n).astype(object)
            p = hx.to_u64(d_id).reshape(-1, n)[:l].reshape(1, 1, l, n).astype(object)
            t = up(hx, dev, np.array(c * p % q.astype(object), dtype=np.uint64))
        r = t
        if G != 1:
            r = minus_one(dev, nb * 2 * l * n)
            hx.hks_rotate_hoisted([gobjs[j]], [G], [r], t, nb, l)
        ctx.sync()
        total = (total + hx.to_u64(r).reshape(nb, 2, l, n)) % q        # words below 2^52: no overflow
    return total.reshape(nb, -1)


@pytest.mark.parametrize("l", [4, 3])
@pytest.mark.parametrize("family", ["uniform", "extreme"])
def test_grids_smallest_ring(hx, ctx, dev, orc, family, l):
    n, nb = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 4, 6, 2, orc.primes(6, 51, n), 3, family)
    cts = rig.cts(l, 2, 3)
    for name in ("2x2", "3x2", "2x3"):
        run_bsgs(hx, ctx, dev, rig, grid_of(rig, name), l, nb, cts, f"{name} {family} level {l}", compose=True)
    rig.close()


@pytest.mark.parametrize("l", [5, 2])
def test_mixed_tier_chain(hx, ctx, dev, orc, l):
    """52, 30, 30, 40, 27-bit data limbs and two 27-bit special primes; l = 2 is a single partial digit whose basis T_l = {0, 1, 5, 6} is
    not a prefix of the plan's limbs: the plaintext is read at the physical limb, the stored sums at the row of T_l"""
    n, L, K = 1024, 5, 7
    rig = Rig(hx, ctx, dev, orc, n, L, K, 2, seal_chain(orc, K, n), 3, "extreme")
    tiers, mixed = rig.s.plan.tiers()
    assert mixed and tiers[0] == 0 and all(t != 0 for t in tiers[1:]), tiers
    assert [q.bit_length() for q in rig.s.qs] == [52, 30, 30, 40, 27, 27, 27]
    run_bsgs(hx, ctx, dev, rig, grid_of(rig, "2x2"), l, 2, rig.cts(l, 2, 11), f"mixed tiers level {l}", compose=True)
    rig.close()


@pytest.mark.parametrize("shape", ["one_digit", "one_special_prime"])
def test_one_digit_and_one_special_prime(hx, ctx, dev, orc, shape):
    n = 1024
    L, alpha, K, bits = (3, 3, 6, 50) if shape == "one_digit" else (4, 2, 5, 51)
    rig = Rig(hx, ctx, dev, orc, n, L, K, alpha, orc.primes(K, bits, n), 3)
    assert rig.model.dnum == (1 if shape == "one_digit" else 2) and K - L == (3 if shape == "one_digit" else 1)
    run_bsgs(hx, ctx, dev, rig, grid_of(rig, "2x3"), L, 2, rig.cts(L, 2, 6), shape)
    rig.close()


@pytest.mark.parametrize("L", [2, 3])
def test_alpha_one_is_the_per_limb_call_on_the_same_key_buffers(hx, ctx, dev, orc, L):
    """alpha = 1, K = L + 1, n_limbs = L: hexl_linear_transform_bsgs on per-limb plans that install the SAME device key buffers gives the
    same words; [K][n] plaintexts are [L + 1][n]"""
    torch = torch_()
    n, nb, K = 1024, 3, L + 1
    cases = [KsCase(orc, n, L, K, seed=5 + r) for r in range(3)]
    plans = [hx.KeySwitchPlan(ctx, n, L, K, K, 2, c.moduli, c.modswitch) for c in cases]
    objs = [hx.HybridKeySwitch(plans[0], 1) for _ in cases]
    d_keys = [up(hx, dev, np.concatenate(c.keys)) for c in cases]
    for p, o, k in zip(plans, objs, d_keys):
        p.set_keys_device(k)
        o.set_keys_device(k)
    qs = [int(q) for q in cases[0].moduli]
    d_ct = up(hx, dev, np.stack([np.concatenate([orc.splitmix(n, 300 + b * 31 + k * 7 + i, qs[i]) for k in range(2) for i in range(L)])
                                 for b in range(nb)]))
    pt = lambda s: up(hx, dev, np.stack([orc.splitmix(n, 500 + s * 13 + i, qs[i]) for i in range(K)]))
    pid = lambda s: up(hx, dev, np.stack([orc.splitmix(n, 700 + s * 13 + i, qs[i]) for i in range(L)]))
    bgs, ggs = [5, 2 * n - 1], [3, 1]
    d_pts, d_ids = [[pt(0), None], [pt(1), pt(2)]], [pid(0), None]
    x, (buf, y) = minus_one(dev, nb * 2 * L * n), guarded(dev, nb * 2 * L * n, n)
    hx.linear_transform_bsgs(plans[:2], bgs, [plans[2], None], ggs, d_pts, x, d_ct, nb, d_ids)
    hx.hks_linear_transform_bsgs(objs[:2], bgs, [objs[2], None], ggs, d_pts, d_ids, y, d_ct, nb, L)
    ctx.sync()
    assert torch.equal(x, y), "alpha = 1, K = L + 1 must be hexl_linear_transform_bsgs word for word"
    assert bool((buf[nb * 2 * L * n:] == -1).all())
    for o in reversed(objs):
        o.close()
    for p in reversed(plans):
        p.close()


@pytest.mark.parametrize("n", [2048, 16384, 32768])
def test_larger_rings_against_the_device_composition(hx, ctx, dev, orc, n):
    """two and more 512-word pieces per polynomial; L = 3, alpha = 2, K = 5, batch 2"""
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 3)
    g = ([0, 1], [pow(5, 3, 2 * n), 2 * n - 1], [2, None], [5, 1],
         [[rig.plaintext(0), rig.plaintext(1)], [rig.plaintext(2), rig.plaintext(3)]], None)
    run_bsgs(hx, ctx, dev, rig, g, 3, 2, rig.cts(3, 2, 13), f"n = {n}", want=False, compose=True)
    rig.close()


CHUNK_CASE = dict(n=1024, L=3, K=5, alpha=2, nb=5, distinct=3)


def chunk_calls(hx, ctx, dev, orc):
    """the 2x3 grid at batch 5 over three distinct instances -> (rig, grid, cts, words); the parent (one chunk) and the child
    (HEXL_KS_CHUNK=2: two chunks and a tail of one) run the same call"""
    c = CHUNK_CASE
    rig = Rig(hx, ctx, dev, orc, c["n"], c["L"], c["K"], c["alpha"], orc.primes(c["K"], 51, c["n"]), 3)
    g = grid_of(rig, "2x3")
    cts = rig.cts(c["L"], c["distinct"], 4)
    out = call(hx, ctx, dev, rig, g, device_grid(hx, dev, rig, g), c["L"], c["nb"], tiled(hx, dev, cts, c["nb"]))
    return rig, g, cts, hx.to_u64(out)


def test_chunks_with_a_ragged_tail_then_fewer_babies_then_the_siblings(hx, ctx, dev, orc, tmp_path):
    """HEXL_KS_CHUNK=2 (read once per process, so a child process): batch 5 runs two full chunks and a tail of one through the baby store,
    the t buffer and the extended digits, and must give the one-chunk words; a second call with ONE baby step runs in the grown buffers
    with another slice stride; then hexl_hks_rotate, hexl_hks_rotate_hoisted and hexl_hks_linear_transform on the same objects still
    give their models' words."""
    c = CHUNK_CASE
    rig, g, cts, words = chunk_calls(hx, ctx, dev, orc)
    assert rig.objs[0].bsgs_scratch_bytes(2, 2) < rig.objs[0].bsgs_scratch_bytes(2, 5), "this process must run batch 5 in one chunk"
    assert_instances(words, expected(rig, g, c["L"], cts), c["nb"], NAMES, (2, c["L"], c["n"]), "one chunk")
    rig.close()
    ref = tmp_path / "one_chunk.npy"
    np.save(ref, words)
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
import hks_hoisted_model as hoisted
from rns_model import assert_instances
from test_gpu_hks import NAMES, minus_one
from test_gpu_hks_hoisted import tiled
from test_gpu_hks_bsgs import chunk_calls, run_bsgs, CHUNK_CASE as c
dev = torch.device("cuda:0")
ctx = hx.Context(0)
rig, g, cts, words = chunk_calls(hx, ctx, dev, orc)
h = rig.objs[0]
assert h.bsgs_scratch_bytes(2, 2) == h.bsgs_scratch_bytes(2, 100) > h.bsgs_scratch_bytes(2, 1), "HEXL_KS_CHUNK=2 not in force"
assert np.array_equal(words, np.load(%r)), "two chunks and a tail differ from the one-chunk words"
n, l = c["n"], c["L"]
one = ([0], [5], [1, None], [3, 1], [[rig.plaintext(0)], [rig.plaintext(2)]], None)
run_bsgs(hx, ctx, dev, rig, one, l, 3, cts, "one baby step in the grown buffers")
m, nb, gs = rig.model, 3, [5, 2 * n - 1]
d_ct = tiled(hx, dev, cts, nb)
plain, lt = minus_one(dev, nb * 2 * l * n), minus_one(dev, nb * 2 * l * n)
rots = [minus_one(dev, nb * 2 * l * n) for _ in gs]
pts = [rig.plaintext(1), rig.plaintext(2)]
rig.objs[0].rotate(plain, d_ct, nb, l, 5)
hx.hks_rotate_hoisted(rig.objs[:2], gs, rots, d_ct, nb, l)
hx.hks_linear_transform(rig.objs[:2], gs, [hx.as_i64(p.reshape(-1)).to(dev) for p in pts], None, lt, d_ct, nb, l)
ctx.sync()
shape = (2, l, n)
assert_instances(hx.to_u64(plain), [m.rotate(rig.keys[0], ct, l, 5) for ct in cts], nb, NAMES, shape, "hexl_hks_rotate afterwards")
for r, gg in enumerate(gs):
    assert_instances(hx.to_u64(rots[r]), [hoisted.rotate_hoisted(m, rig.keys[r], ct, l, gg) for ct in cts], nb, NAMES, shape, "hoisted afterwards")
assert_instances(hx.to_u64(lt), [hoisted.linear_transform(m, rig.keys[:2], gs, pts, None, ct, l) for ct in cts], nb, NAMES, shape, "transform afterwards")
rig.close()
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"), str(ref))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="2"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_batches_two_five_three_on_one_set_of_objects(hx, ctx, dev, orc):
    """the grow-only baby store, t buffer and scratch at every size, with the slice stride of each"""
    n, l = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 3)
    g = grid_of(rig, "3x2")
    dg = device_grid(hx, dev, rig, g)
    cts = rig.cts(l, 2, 8)
    want = None
    for nb in (2, 5, 3):
        _, want = run_bsgs(hx, ctx, dev, rig, g, l, nb, cts, f"batch {nb}", want, dg=dg)
    assert rig.objs[0].bsgs_scratch_bytes(3, 5) == 5 * rig.objs[0].bsgs_scratch_bytes(3, 1)
    rig.close()


def test_on_a_non_blocking_caller_stream(hx, dev, orc):
    torch = torch_()
    n, l, nb = 1024, 3, 2
    own = hx.Context(0, use_torch_stream=False)
    side = torch.cuda.Stream()
    own.set_stream(side.cuda_stream)
    rig = Rig(hx, own, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 3)
    g = grid_of(rig, "2x3")
    dg = device_grid(hx, dev, rig, g)
    cts = rig.cts(l, nb, 2)
    d_ct = tiled(hx, dev, cts, nb)
    buf, out = guarded(dev, nb * 2 * l * n, n)
    d_keys = [up(hx, dev, k) for k in rig.keys]                   # kept until the end: the installs read them on the side stream
    torch.cuda.synchronize()                                      # the uploads ran on torch's stream
    for o, k in zip(rig.objs, d_keys):
        o.set_keys_device(k)
    hx.hks_linear_transform_bsgs(dg[0], g[1], dg[1], g[3], dg[2], dg[3], out, d_ct, nb, l)
    side.synchronize()                                            # the only wait
    assert_instances(hx.to_u64(out), expected(rig, g, l, cts), nb, NAMES, (2, l, n), "side stream")
    assert bool((buf[nb * 2 * l * n:] == -1).all())
    own.use_own_stream()
    rig.close()
    own.close()


def test_every_rejection(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K, nb = 1024, 3, 5, 2
    s = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))
    second, third = hx.HybridKeySwitch(s.plan, 2), hx.HybridKeySwitch(s.plan, 2)
    nokeys = hx.HybridKeySwitch(s.plan, 2)                        # never keyed
    other_alpha = hx.HybridKeySwitch(s.plan, 1)
    t = Setup(hx, ctx, orc, n, L, K, 2, orc.primes(K, 51, n))      # the same shape on ANOTHER plan
    for r, o in enumerate((s.hks, second, third, other_alpha, t.hks)):
        o.set_keys_device(up(hx, dev, s.keys(r)))
    lib = hx.lib()
    words = nb * 2 * L * n
    ct = torch.zeros(words, dtype=torch.int64, device=dev)
    pa, pb, pc = (torch.zeros(K * n, dtype=torch.int64, device=dev) for _ in range(3))
    pid = torch.zeros(L * n, dtype=torch.int64, device=dev)
    out, big = minus_one(dev, words), minus_one(dev, 2 * words)
    H = lambda *objs: hx._handles(list(objs))
    G = lambda *gs: hx._u64_array(list(gs))
    P = lambda *ts: (ctypes.c_void_p * len(ts))(*[None if x is None else x.data_ptr() for x in ts])
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    fn = lib.hexl_hks_linear_transform_bsgs
    bh, bg, gh, gg, grid = H(s.hks, second), G(3, 5), H(None, third), G(1, 7), P(pa, pb, pc, None)

    def status(batch=nb, l=L, bh_=bh, bg_=bg, nbaby=2, gh_=gh, gg_=gg, ngiant=2, pts_=grid, ids_=None, out_=None, ct_=None):
        return fn(bh_, bg_, nbaby, gh_, gg_, ngiant, pts_, ids_, p(out) if out_ is None else out_, p(ct) if ct_ is None else ct_, batch, l)

    for batch in (nb, 0):
        # everything well-formed but a used object's keys: malformed arguments first, then HEXL_E_NOKEYS
        assert status(batch, bh_=H(s.hks, nokeys)) == HEXL_E_NOKEYS                        # a baby object that is used
        assert status(batch, gh_=H(None, nokeys)) == HEXL_E_NOKEYS                         # a giant object that is used
        assert status(batch, bh_=H(s.hks, nokeys), l=0) == HEXL_E_BADARG                   # ... but malformed arguments come first
        # null arguments
        for kw in (dict(bh_=None), dict(bg_=None), dict(gh_=None), dict(gg_=None), dict(pts_=None), dict(out_=ctypes.c_void_p(None)),
                   dict(ct_=ctypes.c_void_p(None))):
            assert status(batch, **kw) == HEXL_E_BADARG, kw
        assert status(batch, ngiant=0) == HEXL_E_BADARG
        assert status(batch, bh_=H(None, None), gh_=H(None, None), gg_=G(1, 1), pts_=P(None, None, None, None), ids_=P(pid, pid)) == HEXL_E_BADARG   # no object
        assert status(batch, pts_=P(pa, pb, None, None)) == HEXL_E_BADARG                  # a giant row with no term at all
        assert status(batch, pts_=P(pa, pb, None, None), ids_=P(pid, None)) == HEXL_E_BADARG
        for stranger in (t.hks, other_alpha):                                              # objects that do not share the first one's plan and alpha
            assert status(batch, bh_=H(s.hks, stranger)) == HEXL_E_BADARG
            assert status(batch, gh_=H(stranger, third)) == HEXL_E_BADARG                  # ... an unused one (G = 1) included
        assert status(batch, bh_=H(s.hks, None)) == HEXL_E_BADARG                          # a NULL baby object whose column has a plaintext
        assert status(batch, gh_=H(None, None)) == HEXL_E_BADARG                           # a NULL giant object with G != 1
        for l in (0, L + 1):
            assert status(batch, l=l) == HEXL_E_BADARG
        for g in (4, 2 * n, 2 * n + 1):
            assert status(batch, bg_=G(3, g)) == HEXL_E_BADARG
            assert status(batch, gg_=G(g, 7)) == HEXL_E_BADARG                             # on the row whose object is NULL
            assert status(batch, bg_=G(3, g), pts_=P(pa, None, pc, None)) == HEXL_E_BADARG   # an element that is not used
        assert status(1 << 62) == HEXL_E_BADARG                                            # a size that overflows
        assert status(batch, nbaby=1 << 40, ngiant=1 << 40) == HEXL_E_BADARG               # a table whose size overflows
    # an n_baby for which not one instance fits the baby store (2 GiB / (2 K n 8) = 26214 slices), everything else well-formed
    many = (2 << 30) // (2 * K * n * 8) + 1
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    wide_h, wide_g, wide_p = (vp * many)(*([s.hks.h.value] * many)), (u64 * many)(*([5] * many)), (vp * many)(*([pa.data_ptr()] * many))
    assert fn(wide_h, wide_g, many, H(None), G(1), 1, wide_p, None, p(out), p(ct), nb, L) == HEXL_E_BADARG
    # overlaps (at the real batch): d_out with d_ct, with a plaintext, with an identity plaintext
    assert status(out_=p(big[n:]), ct_=p(big)) == HEXL_E_BADARG
    assert status(out_=p(ct)) == HEXL_E_BADARG
    assert status(out_=p(big), pts_=P(pa, big[words - n:], pc, None)) == HEXL_E_BADARG
    assert status(out_=p(big), ids_=P(None, big[words - n:])) == HEXL_E_BADARG
    assert lib.hexl_hks_bsgs_scratch_bytes(None, 2, 1) == 0
    assert status(0) == 0                                                                  # an empty batch: 0, nothing written
    ctx.sync()
    clean = lambda: bool((out == -1).all()) and bool((big == -1).all()) and not bool(ct.any()) and not any(bool(x.any()) for x in (pa, pb, pc, pid))
    assert clean(), "a refusal or an empty batch wrote something"
    # an unused object without keys is fine: column 1 holds no plaintext, row 0 has G = 1
    assert status(bh_=H(s.hks, nokeys), gh_=H(nokeys, third), pts_=P(pa, None, pc, None)) == 0
    ctx.sync()
    assert not bool((out == -1).any()) and bool((big == -1).all())
    out.fill_(-1)
    # n_baby == 0: every row needs its identity term
    none = P()
    assert status(bh_=H(), bg_=G(), nbaby=0, pts_=none, ids_=P(pid, None)) == HEXL_E_BADARG
    assert status(bh_=H(), bg_=G(), nbaby=0, pts_=none, ids_=P(pid, pid)) == 0
    ctx.sync()
    # row 0 (G = 1) is pt_id . 0 = 0; row 1 is hexl_hks_rotate_hoisted of the zero ciphertext, whose mod-down leaves its overshoot
    rot = minus_one(dev, words)
    hx.hks_rotate_hoisted([third], [7], [rot], ct, nb, L)
    ctx.sync()
    assert torch.equal(out, rot), "identity-only rows: the composition's words"
    for o in (other_alpha, nokeys, third, second):
        o.close()
    t.close()
    s.close()


def test_scratch_bytes_cover_what_a_first_call_allocates(hx, dev, orc):
    """hexl_hks_bsgs_scratch_bytes against the device memory a call takes on objects that have held nothing so far. A first call with
    other objects on the same context loads the kernels and sizes the context's table; the measured call then allocates the owner's
    six buffers only (coef, ext, acc, w1, baby store and t). The allocator hands out whole 2 MiB pages, one rounding
    per buffer."""
    torch = torch_()
    n, L, K, alpha, nb, l = 16384, 3, 5, 2, 8, 3
    own = hx.Context(0)
    grew = []
    for _ in range(2):
        rig = Rig(hx, own, dev, orc, n, L, K, alpha, orc.primes(K, 51, n), 2)
        d_ct = tiled(hx, dev, rig.cts(l, 1, 1), nb)
        d_pt = up(hx, dev, rig.plaintext(0))
        out = minus_one(dev, nb * 2 * l * n)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        hx.hks_linear_transform_bsgs(rig.objs[:1], [3], rig.objs[1:], [5], [[d_pt]], None, out, d_ct, nb, l)
        torch.cuda.synchronize()
        grew.append(before - torch.cuda.mem_get_info()[0])
        said = rig.objs[0].bsgs_scratch_bytes(1, nb)
        assert said == rig.objs[0].hoisted_scratch_bytes(nb) + nb * (2 * K * n * 8 + 2 * L * n * 8)
        assert rig.objs[0].hoisted_scratch_bytes(nb) == rig.objs[0].scratch_bytes(nb) + nb * L * n * 8, "the parents' figures are unchanged"
        rig.close()
    print(f"reported {said} bytes, the call took {grew[1]} (the first call on the context {grew[0]})")
    # two-sided: the six buffers are new (nothing of them was held before), each rounded UP to whole pages, and nothing else is allocated
    assert said <= grew[1] <= said + 6 * (2 << 20)
    own.close()


def test_end_to_end_decrypts_within_the_noise_bound(hx, ctx, dev, orc):
    """secret = hexl_sample(TERNARY) at K limbs; for g in {5, 25} (baby steps) and G = 125 (the giant step that rotates; the other is G = 1)
    s_g = s(X^g) (hexl_apply_galois) and gen_hybrid_key from s_g to s on an object of its own; a uniform ciphertext at l = L and
    l = L - 1; dense plaintexts with |coefficient| <= 8 encoded modulo all K limbs, and identity terms. hexl_rlwe_decrypt of the output
    equals sum_j sigma_{G_j}(sum_i pt_{j,i} sigma_{g_i}(m) + pt_id_j m), m = c0 + c1 s, up to a noise whose centred CRT lift over the l
    limbs is within B_bsgs (hks_bsgs_model.bsgs_noise_bound: CBD21 errors, ||s||_1 <= n)."""
    n, L, K, alpha = 1024, 4, 6, 2
    bgs, ggs = [5, 25], [125, 1]                                  # two baby and two giant elements; G = 1 second, no key for it
    s = Setup(hx, ctx, orc, n, L, K, alpha, orc.primes(K, 45, n))
    objs = [s.hks] + [hx.HybridKeySwitch(s.plan, alpha) for _ in range(2)]
    plan, qs, m = s.plan, s.qs, s.model
    seed = bytes((37 * k + 11) & 0xFF for k in range(32))
    sec = minus_one(dev, K * n)
    plan.sample(sec, hx.SAMPLE_TERNARY, 1, K, seed=seed, stream=1)
    for r, g in enumerate(bgs + [ggs[0]]):
        s_from = minus_one(dev, K * n)
        ctx.apply_galois(s_from, sec, K, n, g)
        d_keys = minus_one(dev, m.dnum * 2 * K * n)
        plan.gen_hybrid_key(d_keys, sec, alpha, s_from, seed=seed, stream=2 + r)
        objs[r].set_keys_device(d_keys)
    rng = np.random.default_rng(7)
    polys = [[rng.integers(-8, 9, n), rng.integers(-8, 9, n)], [rng.integers(-8, 9, n), None]]
    pts = [[None if x is None else hoisted.encode_small(m, x) for x in row] for row in polys]
    ids = [None, hoisted.encode_small(m, rng.integers(-8, 9, n))]
    norms = [[int(np.abs(x).sum()) for x in row if x is not None] for row in polys]
    d_pts = [[None if x is None else up(hx, dev, x) for x in row] for row in pts]
    d_ids = [None if x is None else up(hx, dev, x) for x in ids]
    lm = Limbs(orc, n, qs)
    for l in (L, L - 1):
        ct = s.words(2, l, 0, 30 + l)
        d_ct, out = up(hx, dev, ct), minus_one(dev, 2 * l * n)
        hx.hks_linear_transform_bsgs(objs[:2], bgs, [objs[2], None], ggs, d_pts, d_ids, out, d_ct, 1, l)
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
            want = np.zeros(n, dtype=object)
            for j, G in enumerate(ggs):
                inner = np.zeros(n, dtype=object)
                for b, pt in enumerate(pts[j]):
                    if pt is not None:
                        inner = inner + pt[i].astype(object) * apply_galois(msg[i], n, bgs[b]).astype(object)
                if ids[j] is not None:
                    inner = inner + ids[j][i].astype(object) * msg[i].astype(object)
                want = want + apply_galois(np.array(inner % q, dtype=np.uint64), n, G).astype(object)
            c = lm.intt(np.array((got[i].astype(object) - want) % q, dtype=np.uint64), i).astype(object)
            acc = acc + c * ((Q // q) * pow(Q // q, -1, q))
        worst = max(min(int(v), Q - int(v)) for v in acc % Q)
        B = model.bsgs_noise_bound(m, l, norms, ggs)
        print(f"[hks bsgs] level {l}: |noise| = {worst}, bound {B:.4g}")
        assert worst <= B, f"level {l}: {worst} > {B}"
    for o in reversed(objs[1:]):
        o.close()
    s.close()
