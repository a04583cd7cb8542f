"""GPU: hexl_hks_linear_transform_bsgs_ext bit for bit, every word of every instance, every output pre-filled with -1 behind a guard row,
against the exact model (tests/hks_bsgs_ext_model.py, pinned in test_hks_bsgs_ext_model.py) and -- the two word identities of the
header -- against hexl_hks_linear_transform on the DEVICE. n = 1024 with L = 4, alpha = 2, K = 6 at l = 4 and l = 3, rescale 0 and 1, on
the uniform and extreme words, keys and plaintexts and the three grids of test_gpu_hks_bsgs.py (G in {3, 1, 2n - 1}, a repeated object,
NULL diagonals, an unused column without an object, identity-only rows); the mixed-tier chain at l = 5 and l = 2; alpha = L; n_p = 1;
l = 2 with rescale = 1 (a one-limb output); the identities at n = 1024, 2048, 16384, 32768; a rotated grid at n = 16384 against the
model; two scratch chunks with a ragged tail (a child process with HEXL_KS_CHUNK) followed by the older callers on the grown buffers;
batches 2, 5, 3 alternating rescale; a non-blocking caller stream; every rejection; the reported scratch; and end to end: gen_hybrid_key
(Galois) -> this call -> hexl_rlwe_decrypt within the bound DESIGN.md 4.6.14 proves. No tolerance anywhere but in that last case."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hks_bsgs_ext_model as model
import hks_hoisted_model as hoisted
from ckks_model import Limbs, apply_galois
from ks_util import seal_chain
from rns_model import assert_instances
from test_gpu_hks import NAMES, Setup, minus_one, torch_, up
from test_gpu_hks_bsgs import device_grid, grid_of, guarded
from test_gpu_hks_hoisted import Rig, tiled

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HEXL_E_BADARG, HEXL_E_NOKEYS = -1, -2


def expected(rig, g, l, cts, rescale):
    bp, bgs, gp, ggs, pts, ids = g
    keys = lambda picks: [None if p is None else rig.keys[p] for p in picks]
    return [model.linear_transform_bsgs_ext(rig.model, keys(bp), bgs, keys(gp), ggs, pts, ids, ct, l, rescale) for ct in cts]


def call(hx, ctx, dev, rig, g, dg, l, nb, d_ct, rescale):
    n = rig.n
    words = nb * 2 * (l - rescale) * n
    buf, out = guarded(dev, words, n)
    hx.hks_linear_transform_bsgs_ext(dg[0], g[1], dg[1], g[3], dg[2], dg[3], out, d_ct, nb, l, rescale)
    ctx.sync()
    assert bool((buf[words:] == -1).all()), "the guard row behind the output was written"
    assert not bool((out == -1).any()), "a word of the output was not written"
    return out


def run_ext(hx, ctx, dev, rig, g, l, nb, cts, rescale, label, want=None, dg=None):
    n = rig.n
    dg = dg or device_grid(hx, dev, rig, g)
    d_ct = tiled(hx, dev, cts, nb)
    out = call(hx, ctx, dev, rig, g, dg, l, nb, d_ct, rescale)
    if want is None:
        want = expected(rig, g, l, cts, rescale)
    assert_instances(hx.to_u64(out), want, nb, NAMES, (2, l - rescale, n), f"{label}, rescale {rescale}")
    assert np.array_equal(hx.to_u64(d_ct), np.stack([cts[b % len(cts)] for b in range(nb)]).reshape(-1)), "the input was written"
    return out, want


@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("l", [4, 3])
@pytest.mark.parametrize("family", ["uniform", "extreme"])
def test_grids_smallest_ring(hx, ctx, dev, orc, family, l, rescale):
    n, nb = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 4, 6, 2, orc.primes(6, 51, n), 3, family)
    cts = rig.cts(l, 2, 3)
    for name in ("2x2", "3x2", "2x3"):
        run_ext(hx, ctx, dev, rig, grid_of(rig, name), l, nb, cts, rescale, f"{name} {family} level {l}")
    rig.close()


@pytest.mark.parametrize("l", [5, 2])
def test_mixed_tier_chain(hx, ctx, dev, orc, l):
    """52, 30, 30, 40, 27-bit data limbs and two 27-bit special primes; l = 2 is a single partial digit, and with rescale = 1 its output
    has ONE limb"""
    n, L, K = 1024, 5, 7
    rig = Rig(hx, ctx, dev, orc, n, L, K, 2, seal_chain(orc, K, n), 3, "extreme")
    tiers, mixed = rig.s.plan.tiers()
    assert mixed and tiers[0] == 0 and all(t != 0 for t in tiers[1:]), tiers
    for rescale in (0, 1):
        run_ext(hx, ctx, dev, rig, grid_of(rig, "2x3"), l, 2, rig.cts(l, 2, 11), rescale, f"mixed tiers level {l}")
    rig.close()


@pytest.mark.parametrize("shape", ["one_digit", "one_special_prime", "two_limbs"])
def test_one_digit_one_special_prime_and_a_one_limb_output(hx, ctx, dev, orc, shape):
    """alpha = L (one digit, three special primes); n_p = 1; l = 2 of L = 4 with rescale = 1: the output is [2][1][n]"""
    n = 1024
    L, alpha, K, bits, l = {"one_digit": (3, 3, 6, 50, 3), "one_special_prime": (4, 2, 5, 51, 4), "two_limbs": (4, 2, 6, 51, 2)}[shape]
    rig = Rig(hx, ctx, dev, orc, n, L, K, alpha, orc.primes(K, bits, n), 3)
    for rescale in ((1,) if shape == "two_limbs" else (0, 1)):
        run_ext(hx, ctx, dev, rig, grid_of(rig, "2x3"), l, 2, rig.cts(l, 2, 6), rescale, shape)
    rig.close()


@pytest.mark.parametrize("n", [1024, 2048, 16384, 32768])
def test_the_two_word_identities_on_the_device(hx, ctx, dev, orc, n):
    """n_giant = 1, G = 1 is hexl_hks_linear_transform on row 0; three rows with G = 1 each are the flat hexl_hks_linear_transform over
    the concatenated non-NULL terms. L = 3, alpha = 2, K = 5, batch 2, rescale = 0. No model: both sides run on the device."""
    torch = torch_()
    l, nb = 3, 2
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 2)
    gs = [pow(5, 3, 2 * n), 2 * n - 1]
    d_ct = tiled(hx, dev, rig.cts(l, 2, 13), nb)
    pt = [up(hx, dev, rig.plaintext(r)) for r in range(4)]
    pid = up(hx, dev, rig.plaintext(7, rows=l))
    words = nb * 2 * l * n
    for label, ggs, grid, ids in (("one row", [1], [[pt[0], pt[1]]], [pid]),
                                  ("three rows", [1, 1, 1], [[pt[0], pt[1]], [None, pt[2]], [pt[3], None]], [None, pid, None])):
        buf, out = guarded(dev, words, n)
        hx.hks_linear_transform_bsgs_ext(rig.objs, gs, [None] * len(ggs), ggs, grid, ids, out, d_ct, nb, l, 0)
        flat = [(rig.objs[i], gs[i], row[i]) for row in grid for i in range(2) if row[i] is not None]
        want = minus_one(dev, words)
        hx.hks_linear_transform([f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat], pid, want, d_ct, nb, l)
        ctx.sync()
        assert torch.equal(out, want), f"n = {n}, {label}: not hexl_hks_linear_transform word for word"
        assert bool((buf[words:] == -1).all())
    rig.close()


def test_a_rotated_grid_at_n_16384_against_the_model(hx, ctx, dev, orc):
    """32 pieces of 512 words per polynomial through the half mod-down, the permuted add and the accumulate mode"""
    n, l = 16384, 3
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 2)
    g = ([0], [pow(5, 3, 2 * n)], [1], [2 * n - 1], [[rig.plaintext(0)]], [rig.plaintext(1, rows=3)])
    run_ext(hx, ctx, dev, rig, g, l, 1, rig.cts(l, 1, 13), 1, "n = 16384")
    rig.close()


CHUNK_CASE = dict(n=1024, L=3, K=5, alpha=2, nb=5, distinct=3)


def chunk_calls(hx, ctx, dev, orc):
    """the 2x3 grid at batch 5 over three distinct instances, rescale 0 and 1 -> (rig, grid, cts, [words, words]); the parent (one chunk)
    and the child (HEXL_KS_CHUNK=2: two chunks and a tail of one) run the same calls"""
    c = CHUNK_CASE
    rig = Rig(hx, ctx, dev, orc, c["n"], c["L"], c["K"], c["alpha"], orc.primes(c["K"], 51, c["n"]), 3)
    g = grid_of(rig, "2x3")
    cts = rig.cts(c["L"], c["distinct"], 4)
    dg = device_grid(hx, dev, rig, g)
    outs = [hx.to_u64(call(hx, ctx, dev, rig, g, dg, c["L"], c["nb"], tiled(hx, dev, cts, c["nb"]), rescale)) for rescale in (0, 1)]
    return rig, g, cts, outs


def test_chunks_with_a_ragged_tail_then_the_older_callers(hx, ctx, dev, orc, tmp_path):
    """HEXL_KS_CHUNK=2 (read once per process, so a child process): batch 5 runs two full chunks and a tail of one through A, F, the baby
    store and t, and must give the one-chunk words; then hexl_hks_linear_transform_bsgs, hexl_hks_linear_transform and
    hexl_hks_relinearize_rescale run on the grown buffers of the same objects and still give their models' words."""
    c = CHUNK_CASE
    rig, g, cts, outs = chunk_calls(hx, ctx, dev, orc)
    assert rig.objs[0].bsgs_ext_scratch_bytes(2, 2, 1) < rig.objs[0].bsgs_ext_scratch_bytes(2, 5, 1), "this process must run batch 5 in one chunk"
    for rescale in (0, 1):
        assert_instances(outs[rescale], expected(rig, g, c["L"], cts, rescale), c["nb"], NAMES, (2, c["L"] - rescale, c["n"]), "one chunk")
    rig.close()
    refs = [tmp_path / f"one_chunk_{r}.npy" for r in (0, 1)]
    for ref, words in zip(refs, outs):
        np.save(ref, words)
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
import hks_hoisted_model as hoisted
from hks_mul_model import HksMul
from rns_model import assert_instances
from test_gpu_hks import NAMES, minus_one, up
from test_gpu_hks_hoisted import tiled
from test_gpu_hks_bsgs import run_bsgs
from test_gpu_hks_bsgs_ext import chunk_calls, CHUNK_CASE as c
dev = torch.device("cuda:0")
ctx = hx.Context(0)
rig, g, cts, outs = chunk_calls(hx, ctx, dev, orc)
h = rig.objs[0]
assert h.bsgs_ext_scratch_bytes(2, 2, 1) == h.bsgs_ext_scratch_bytes(2, 100, 1) > h.bsgs_ext_scratch_bytes(2, 1, 1), "HEXL_KS_CHUNK=2 not in force"
for r, ref in enumerate(%r):
    assert np.array_equal(outs[r], np.load(ref)), "two chunks and a tail differ from the one-chunk words, rescale %%d" %% r
n, l = c["n"], c["L"]
run_bsgs(hx, ctx, dev, rig, g, l, 3, cts, "hexl_hks_linear_transform_bsgs afterwards")
m, nb, gs = rig.model, 3, [5, 2 * n - 1]
d_ct = tiled(hx, dev, cts, nb)
lt = minus_one(dev, nb * 2 * l * n)
pts = [rig.plaintext(1), rig.plaintext(2)]
hx.hks_linear_transform(rig.objs[:2], gs, [hx.as_i64(p.reshape(-1)).to(dev) for p in pts], None, lt, d_ct, nb, l)
ct3 = [np.concatenate([ct, ct[: l * n]]) for ct in cts]
rr = minus_one(dev, nb * 2 * (l - 1) * n)
rig.objs[0].relinearize_rescale(rr, tiled(hx, dev, ct3, nb), nb, l)
ctx.sync()
assert_instances(hx.to_u64(lt), [hoisted.linear_transform(m, rig.keys[:2], gs, pts, None, ct, l) for ct in cts], nb, NAMES, (2, l, n), "transform afterwards")
mm = HksMul(orc, n, c["L"], c["K"], c["alpha"], m.qs, lm=m.lm)
assert_instances(hx.to_u64(rr), [mm.relinearize_rescale(rig.keys[0], x, l) for x in ct3], nb, NAMES, (2, l - 1, n), "relinearize_rescale afterwards")
rig.close()
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"), [str(r) for r in refs])
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="2"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_batches_two_five_three_alternating_rescale(hx, ctx, dev, orc):
    """the grow-only A, F, baby store, t buffer and scratch at every size, the final mod-down switching between P and R"""
    n, l = 1024, 3
    rig = Rig(hx, ctx, dev, orc, n, 3, 5, 2, orc.primes(5, 51, n), 3)
    g = grid_of(rig, "3x2")
    dg = device_grid(hx, dev, rig, g)
    cts = rig.cts(l, 2, 8)
    want = {0: None, 1: None}
    for nb, rescale in ((2, 0), (5, 1), (3, 0), (2, 1)):
        _, want[rescale] = run_ext(hx, ctx, dev, rig, g, l, nb, cts, rescale, f"batch {nb}", want[rescale], dg=dg)
    for rescale in (0, 1):
        assert rig.objs[0].bsgs_ext_scratch_bytes(3, 5, rescale) == 5 * rig.objs[0].bsgs_ext_scratch_bytes(3, 1, rescale)
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
    words = nb * 2 * (l - 1) * n
    buf, out = guarded(dev, words, n)
    d_keys = [up(hx, dev, k) for k in rig.keys]                   # kept until the end: the installs read them on the side stream
    torch.cuda.synchronize()                                      # the uploads ran on torch's stream
    for o, k in zip(rig.objs, d_keys):
        o.set_keys_device(k)
    hx.hks_linear_transform_bsgs_ext(dg[0], g[1], dg[1], g[3], dg[2], dg[3], out, d_ct, nb, l, 1)
    side.synchronize()                                            # the only wait
    assert_instances(hx.to_u64(out), expected(rig, g, l, cts, 1), nb, NAMES, (2, l - 1, n), "side stream")
    assert bool((buf[words:] == -1).all())
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
    fn = lib.hexl_hks_linear_transform_bsgs_ext
    bh, bg, gh, gg, grid = H(s.hks, second), G(3, 5), H(None, third), G(1, 7), P(pa, pb, pc, None)

    def status(batch=nb, l=L, bh_=bh, bg_=bg, nbaby=2, gh_=gh, gg_=gg, ngiant=2, pts_=grid, ids_=None, out_=None, ct_=None, rescale=0):
        return fn(bh_, bg_, nbaby, gh_, gg_, ngiant, pts_, ids_, p(out) if out_ is None else out_, p(ct) if ct_ is None else ct_, batch, l, rescale)

    for batch in (nb, 0):
        for rescale in (0, 1):
            # everything well-formed but a used object's keys: malformed arguments first, then HEXL_E_NOKEYS
            assert status(batch, bh_=H(s.hks, nokeys), rescale=rescale) == HEXL_E_NOKEYS       # a baby object that is used
            assert status(batch, gh_=H(None, nokeys), rescale=rescale) == HEXL_E_NOKEYS        # a giant object that is used
            assert status(batch, bh_=H(s.hks, nokeys), l=0, rescale=rescale) == HEXL_E_BADARG  # ... but malformed arguments come first
            for kw in (dict(bh_=None), dict(bg_=None), dict(gh_=None), dict(gg_=None), dict(pts_=None), dict(out_=ctypes.c_void_p(None)),
                       dict(ct_=ctypes.c_void_p(None))):
                assert status(batch, rescale=rescale, **kw) == HEXL_E_BADARG, kw
            assert status(batch, ngiant=0, rescale=rescale) == HEXL_E_BADARG
            assert status(batch, pts_=P(pa, pb, None, None), rescale=rescale) == HEXL_E_BADARG  # a giant row with no term at all
            for stranger in (t.hks, other_alpha):                                              # another plan, another alpha
                assert status(batch, bh_=H(s.hks, stranger), rescale=rescale) == HEXL_E_BADARG
                assert status(batch, gh_=H(stranger, third), rescale=rescale) == HEXL_E_BADARG
            assert status(batch, bh_=H(s.hks, None), rescale=rescale) == HEXL_E_BADARG         # a NULL baby object whose column has a plaintext
            assert status(batch, gh_=H(None, None), rescale=rescale) == HEXL_E_BADARG          # a NULL giant object with G != 1
            for l in (0, L + 1):
                assert status(batch, l=l, rescale=rescale) == HEXL_E_BADARG
            for g in (4, 2 * n, 2 * n + 1):
                assert status(batch, bg_=G(3, g), rescale=rescale) == HEXL_E_BADARG
                assert status(batch, gg_=G(g, 7), rescale=rescale) == HEXL_E_BADARG
            assert status(1 << 62, rescale=rescale) == HEXL_E_BADARG                           # a size that overflows
        assert status(batch, bh_=H(None, None), gh_=H(None, None), gg_=G(1, 1), pts_=P(None, None, None, None), ids_=P(pid, pid)) == HEXL_E_BADARG
        for rescale in (2, -1, 1 << 16):
            assert status(batch, rescale=rescale) == HEXL_E_BADARG
        assert status(batch, l=1, rescale=1) == HEXL_E_BADARG                                  # nothing to rescale into
        assert status(batch, l=1, rescale=1, bh_=H(s.hks, nokeys)) == HEXL_E_BADARG            # ... in front of HEXL_E_NOKEYS
    # overlaps (at the real batch), with the output's REAL size: [nb][2][L - 1][n] words for rescale = 1
    short = nb * 2 * (L - 1) * n
    assert status(out_=p(big[n:]), ct_=p(big)) == HEXL_E_BADARG
    assert status(out_=p(ct)) == HEXL_E_BADARG
    assert status(out_=p(big), pts_=P(pa, big[words - n:], pc, None)) == HEXL_E_BADARG
    assert status(out_=p(big), ids_=P(None, big[words - n:])) == HEXL_E_BADARG
    assert status(out_=p(big), ct_=p(big[short - n:]), rescale=1) == HEXL_E_BADARG             # the last row of the short output
    assert status(out_=p(big), pts_=P(pa, big[short - n:], pc, None), rescale=1) == HEXL_E_BADARG
    assert lib.hexl_hks_bsgs_ext_scratch_bytes(None, 2, 1, 1) == 0
    for rescale in (0, 1):
        assert status(0, rescale=rescale) == 0                                                 # an empty batch: 0, nothing written
    ctx.sync()
    clean = lambda: bool((out == -1).all()) and bool((big == -1).all()) and not bool(ct.any()) and not any(bool(x.any()) for x in (pa, pb, pc, pid))
    assert clean(), "a refusal or an empty batch wrote something"
    # rescale = 1 writes exactly the short output: a plaintext right behind it is no overlap, and the words behind it keep their fill
    assert status(out_=p(big), ct_=p(big[short:]), rescale=1, batch=0) == 0
    assert status(rescale=1) == 0
    ctx.sync()
    assert not bool((out[:short] == -1).any()) and bool((out[short:] == -1).all()) and bool((big == -1).all())
    out.fill_(-1)
    # an unused object without keys is fine: column 1 holds no plaintext, row 0 has G = 1
    assert status(bh_=H(s.hks, nokeys), gh_=H(nokeys, third), pts_=P(pa, None, pc, None)) == 0
    ctx.sync()
    assert not bool((out == -1).any()) and bool((big == -1).all())
    for o in (other_alpha, nokeys, third, second):
        o.close()
    t.close()
    s.close()


def test_scratch_bytes_cover_what_a_first_call_allocates(hx, dev, orc):
    """hexl_hks_bsgs_ext_scratch_bytes against the device memory a call takes on objects that have held nothing so far. A first call with
    other objects on the same context loads the kernels and sizes the context's table; the measured call then allocates the owner's eight
    buffers only (coef, ext, acc, w1, baby store, t, A and F). The allocator hands out whole 2 MiB pages, one rounding per buffer."""
    torch = torch_()
    n, L, K, alpha, nb, l = 16384, 3, 5, 2, 8, 3
    own = hx.Context(0)
    grew = []
    for _ in range(2):
        rig = Rig(hx, own, dev, orc, n, L, K, alpha, orc.primes(K, 51, n), 2)
        d_ct = tiled(hx, dev, rig.cts(l, 1, 1), nb)
        d_pt = up(hx, dev, rig.plaintext(0))
        out = minus_one(dev, nb * 2 * (l - 1) * n)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        hx.hks_linear_transform_bsgs_ext(rig.objs[:1], [3], rig.objs[1:], [5], [[d_pt]], None, out, d_ct, nb, l, 1)
        torch.cuda.synchronize()
        grew.append(before - torch.cuda.mem_get_info()[0])
        h = rig.objs[0]
        said = h.bsgs_ext_scratch_bytes(1, nb, 1)
        assert said == h.bsgs_scratch_bytes(1, nb) + nb * (2 * K * n * 8 + 2 * L * n * 8)
        assert h.bsgs_ext_scratch_bytes(1, nb, 0) == h.bsgs_scratch_bytes(1, nb) + nb * 2 * K * n * 8
        assert h.bsgs_scratch_bytes(1, nb) == h.hoisted_scratch_bytes(nb) + nb * (2 * K * n * 8 + 2 * L * n * 8), "the older figures are unchanged"
        assert h.hoisted_scratch_bytes(nb) == h.scratch_bytes(nb) + nb * L * n * 8
        assert h.mul_scratch_bytes(nb) == h.scratch_bytes(nb) + nb * 3 * L * n * 8
        rig.close()
    print(f"reported {said} bytes, the call took {grew[1]} (the first call on the context {grew[0]})")
    assert said <= grew[1] <= said + 8 * (2 << 20)
    own.close()


def test_end_to_end_decrypts_within_the_noise_bound(hx, ctx, dev, orc):
    """test_gpu_hks_bsgs's end-to-end case on this call: secret = hexl_sample(TERNARY), gen_hybrid_key from s(X^g) to s for g in {5, 25}
    and G = 125 (the other giant step is G = 1), a uniform ciphertext at l = L and L - 1, dense plaintexts with |coefficient| <= 8.
    rescale = 0: hexl_rlwe_decrypt(out) - M is within B. rescale = 1: q_(l-1) hexl_rlwe_decrypt(out) - M modulo Q_l is within q_(l-1) B,
    i.e. out decrypts to M / q_(l-1) within B. M = sum_j sigma_{G_j}(sum_i pt_{j,i} sigma_{g_i}(m) + pt_id_j m), m = c0 + c1 s, and B is
    hks_bsgs_ext_model.bsgs_ext_noise_bound (CBD21 errors, ||s||_1 <= n)."""
    n, L, K, alpha = 1024, 4, 6, 2
    bgs, ggs = [5, 25], [125, 1]
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
        d_ct = up(hx, dev, ct)
        dec_in = minus_one(dev, l * n)
        plan.rlwe_decrypt(dec_in, d_ct, sec, 1, 2, l)
        ctx.sync()
        msg = hx.to_u64(dec_in).reshape(l, n)
        Q = 1
        for q in qs[:l]:
            Q *= q
        want = []
        for i in range(l):
            total = np.zeros(n, dtype=object)
            for j, G in enumerate(ggs):
                inner = np.zeros(n, dtype=object)
                for b, pt in enumerate(pts[j]):
                    if pt is not None:
                        inner = inner + pt[i].astype(object) * apply_galois(msg[i], n, bgs[b]).astype(object)
                if ids[j] is not None:
                    inner = inner + ids[j][i].astype(object) * msg[i].astype(object)
                total = total + apply_galois(np.array(inner % qs[i], dtype=np.uint64), n, G).astype(object)
            want.append(total)
        for rescale in (0, 1):
            lo = l - rescale
            out, dec = minus_one(dev, 2 * lo * n), minus_one(dev, lo * n)
            hx.hks_linear_transform_bsgs_ext(objs[:2], bgs, [objs[2], None], ggs, d_pts, d_ids, out, d_ct, 1, l, rescale)
            plan.rlwe_decrypt(dec, out, sec, 1, 2, lo)
            ctx.sync()
            got = hx.to_u64(dec).reshape(lo, n).astype(object)
            scale = qs[l - 1] if rescale else 1
            acc = np.zeros(n, dtype=object)
            for i in range(l):
                q = qs[i]
                have = got[i] * scale if i < lo else 0               # q_(l-1) dec(out) modulo Q_l: limb l - 1 is zero
                c = lm.intt(np.array((have - want[i]) % q, dtype=np.uint64), i).astype(object)
                acc = acc + c * ((Q // q) * pow(Q // q, -1, q))
            worst = max(min(int(v), Q - int(v)) for v in acc % Q)
            B = model.bsgs_ext_noise_bound(m, l, norms, ggs, rescale) * scale
            print(f"[hks bsgs ext] level {l} rescale {rescale}: |noise| = {worst}, bound {float(B):.4g}")
            assert worst <= B, f"level {l} rescale {rescale}: {worst} > {float(B)}"
    for o in reversed(objs[1:]):
        o.close()
    s.close()
