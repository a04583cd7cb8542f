"""GPU: hexl_linear_transform_bsgs, bit for bit, every instance of every launch: against the exact model (tests/bsgs_model.py, pinned in
test_bsgs_model.py) and, at n = 1024 and n = 4096, also against the DEVICE composition the header fixes the output by --
hexl_linear_transform per row, hexl_rotate_hoisted with one rotation, a modular add on the host -- which does not involve the model.
Every output buffer starts as -1: the call writes it. Helpers of the two parents' test files are reused by import."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from bsgs_model import check_decrypts_bsgs, linear_transform_bsgs, reference_case
from hoist_model import limbs_of, mod_up, rotate_hoisted
from ks_util import KsCase, RlweCase, extreme_ciphertext, seal_chain
from lt_model import linear_transform, ones_plaintext, uniform_plaintext
from test_bsgs_model import BSGS_GRIDS, bsgs_plaintexts, bsgs_rlwe
from test_gpu_linear_transform import assert_output, extreme_plaintext
from test_gpu_rotate_hoisted import cases_for, made, plans_for, torch_, uniform_ct  # noqa: F401  (made: a fixture)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def expected(orc, bcases, bgs, gcases, ggs, pts, pt_ids, cts):
    """want[c]: the model's words for distinct ciphertext c"""
    ref = reference_case(bcases, gcases)
    lm = limbs_of(orc, ref)
    return [linear_transform_bsgs(orc, bcases, bgs, gcases, ggs, pts, pt_ids, ct, lm, mod_up(lm, ref, ct)) for ct in cts]


def device_inputs(hx, dev, cts, nb, pts, pt_ids):
    torch = torch_()
    up = lambda p: None if p is None else hx.as_i64(p).to(dev)
    base = hx.as_i64(np.stack(cts)).to(dev)
    d_ct = base[torch.arange(nb, device=dev) % len(cts)].reshape(-1).contiguous()
    return d_ct, torch.full_like(d_ct, -1), [[up(p) for p in row] for row in pts], None if pt_ids is None else [up(p) for p in pt_ids]


def run_and_check(hx, ctx, dev, want, ref, bplans, bgs, gplans, ggs, pts, pt_ids, cts, nb, label=""):
    d_ct, out, d_pts, d_ids = device_inputs(hx, dev, cts, nb, pts, pt_ids)
    hx.linear_transform_bsgs(bplans, bgs, gplans, ggs, d_pts, out, d_ct, nb, d_ids)
    ctx.sync()
    assert_output(hx, want, out, nb, ref, label)
    return d_ct, out, d_pts, d_ids


def device_composition(hx, ctx, ref, bplans, bgs, gplans, ggs, d_pts, d_ids, d_ct, nb):
    """the header's definition on the device: hexl_linear_transform per row (an identity-only row: the word product on the host),
    hexl_rotate_hoisted with one rotation, the modular sum on the host. Returns [nb][2 L n] uint64."""
    torch = torch_()
    n, L = ref.n, ref.L
    q = np.array(ref.moduli[:L], dtype=np.uint64).reshape(1, 1, L, 1)
    total = np.zeros((nb, 2, L, n), dtype=np.uint64)
    for j, G in enumerate(ggs):
        used = [i for i, p in enumerate(d_pts[j]) if p is not None]
        d_id = None if d_ids is None else d_ids[j]
        t = torch.full_like(d_ct, -1)
        if used:
            hx.linear_transform([bplans[i] for i in used], [bgs[i] for i in used], [d_pts[j][i] for i in used], t, d_ct, nb, d_id)
        else:
            c = hx.to_u64(d_ct).reshape(nb, 2, L, n).astype(object)
            p = hx.to_u64(d_id).reshape(1, 1, L, n).astype(object)
            t = hx.as_i64(np.array(c * p % q.astype(object), dtype=np.uint64).reshape(-1)).to(d_ct.device)
        r = t
        if G != 1:
            r = torch.full_like(d_ct, -1)
            hx.rotate_hoisted([gplans[j]], [G], [r], t, nb)
        ctx.sync()
        total = (total + hx.to_u64(r).reshape(nb, 2, L, n)) % q        # words below 2^52: no overflow
    return total.reshape(nb, -1)


def grid_of(orc, n, L, K, name, ext, made_, hx, ctx, moduli=None):
    """the two small grids of the issue at ring dimension n: cases, plans, elements, plaintexts.
    2x2: G = 1 FIRST, g = 3 as a baby and as a giant step (different keys), g = 2n - 1.
    3x2: three baby steps (g = 1 WITH a key, an unused column without a plan, g = 3), two giant steps (G = 2n - 1, then G = 1 NOT
         first): a NULL entry, identity terms, a row of identity only."""
    cases = cases_for(orc, n, L, K, 3, moduli=moduli, extreme_keys=ext)
    plans = plans_for(hx, ctx, cases, made_)
    pt = lambda s: extreme_plaintext(cases[0], 1 + s) if ext else uniform_plaintext(orc, cases[0], s)
    pid = lambda s: extreme_plaintext(cases[0], 5 + s, rows=L) if ext else uniform_plaintext(orc, cases[0], 9 + s, rows=L)
    if name == "2x2":
        b, g = [0, 1], [None, 2]
        bgs, ggs = [3, 2 * n - 1], [1, 3]
        pts, ids = [[pt(0), pt(1)], [pt(2), pt(3)]], None
    else:
        b, g = [0, None, 1], [2, None]
        bgs, ggs = [1, 5, 3], [2 * n - 1, 1]
        pts, ids = [[pt(0), None, pt(1)], [None, None, None]], [pid(0), pid(1)]
    pick = lambda idx, xs: [None if k is None else xs[k] for k in idx]
    return pick(b, cases), pick(g, cases), pick(b, plans), pick(g, plans), bgs, ggs, pts, ids


def test_one_giant_step_without_rotation_is_linear_transform(hx, ctx, dev, orc, made):
    n, L, K, nb = 1024, 2, 3, 5
    gs = [1, 3, 2 * n - 1]
    cases = cases_for(orc, n, L, K, 3)
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], 0), extreme_ciphertext(cases[0], 1, 2)]
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(3)]
    pt_id = uniform_plaintext(orc, cases[0], 9, rows=L)
    lm = limbs_of(orc, cases[0])
    want = [linear_transform(orc, cases, gs, pts, pt_id, ct, lm) for ct in cts]
    d_ct, out, d_pts, d_ids = run_and_check(hx, ctx, dev, want, cases[0], plans, gs, [None], [1], [pts], [pt_id], cts, nb)
    d_lt = torch_().full_like(d_ct, -1)
    hx.linear_transform(plans, gs, d_pts[0], d_lt, d_ct, nb, d_ids[0])
    ctx.sync()
    assert torch_().equal(d_lt, out), "one giant step with G = 1 must be hexl_linear_transform's words"
    assert plans[0].range_check()


def test_all_ones_baby_and_one_giant_is_two_chained_hoisted_rotations(hx, ctx, dev, orc, made):
    n, L, K, nb = 1024, 3, 4, 5
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], 0), extreme_ciphertext(cases[0], 1, 2)]
    lm = limbs_of(orc, cases[0])
    want = [rotate_hoisted(orc, cases[1], rotate_hoisted(orc, cases[0], ct, 3, lm), 2 * n - 1, lm) for ct in cts]
    d_ct, out, _, _ = run_and_check(hx, ctx, dev, want, cases[0], plans[:1], [3], plans[1:], [2 * n - 1], [[ones_plaintext(cases[0])]], None,
                                    cts, nb)
    a, b = torch_().full_like(d_ct, -1), torch_().full_like(d_ct, -1)
    hx.rotate_hoisted(plans[:1], [3], [a], d_ct, nb)
    hx.rotate_hoisted(plans[1:], [2 * n - 1], [b], a, nb)
    ctx.sync()
    assert torch_().equal(b, out)


@pytest.mark.parametrize("family", ["uniform", "extreme"])
@pytest.mark.parametrize("name", ["2x2", "3x2"])
def test_grids_smallest_ring(hx, ctx, dev, orc, made, name, family):
    n, L, K, nb = 1024, 2, 3, 5
    ext = family == "extreme"
    bcases, gcases, bplans, gplans, bgs, ggs, pts, ids = grid_of(orc, n, L, K, name, ext, made, hx, ctx)
    ref = bcases[0]
    cts = [extreme_ciphertext(ref, b, 2) if ext else uniform_ct(orc, ref, b) for b in range(2)]
    want = expected(orc, bcases, bgs, gcases, ggs, pts, ids, cts)
    d_ct, out, d_pts, d_ids = run_and_check(hx, ctx, dev, want, ref, bplans, bgs, gplans, ggs, pts, ids, cts, nb)
    comp = device_composition(hx, ctx, ref, bplans, bgs, gplans, ggs, d_pts, d_ids, d_ct, nb)
    assert np.array_equal(hx.to_u64(out).reshape(nb, -1), comp), "not the device composition's words"
    assert all(p.range_check() for p in bplans + gplans if p is not None), "in-range words must not raise a range flag"


def test_seal_chain_four_babies_three_giants(hx, ctx, dev, orc, made):
    """bridge-seal's chain (mixed tiers): g = 5^0 ... 5^3 as baby steps (5^0 with a key of its own), G = 5^0, 5^4, 5^8, batch 5"""
    n, L, K, nb = 4096, 5, 6, 5
    bgs = [pow(5, k, 2 * n) for k in range(4)]
    ggs = [1, pow(5, 4, 2 * n), pow(5, 8, 2 * n)]
    cases = cases_for(orc, n, L, K, 6, moduli=seal_chain(orc, K, n))
    plans = plans_for(hx, ctx, cases, made)
    assert plans[0].tiers()[1], "the seal chain mixes tiers"
    bcases, bplans, gcases, gplans = cases[:4], plans[:4], [None] + cases[4:], [None] + plans[4:]
    pts = [[uniform_plaintext(orc, cases[0], 4 * j + i) for i in range(4)] for j in range(3)]
    ids = [None, uniform_plaintext(orc, cases[0], 40, rows=L), None]
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    want = expected(orc, bcases, bgs, gcases, ggs, pts, ids, cts)
    d_ct, out, d_pts, d_ids = run_and_check(hx, ctx, dev, want, cases[0], bplans, bgs, gplans, ggs, pts, ids, cts, nb)
    comp = device_composition(hx, ctx, cases[0], bplans, bgs, gplans, ggs, d_pts, d_ids, d_ct, nb)
    assert np.array_equal(hx.to_u64(out).reshape(nb, -1), comp), "not the device composition's words"


@pytest.fixture(scope="module")
def headline(orc):
    """n = 16384 on the headline chain (L = 7, K = 8, 51-bit primes), two baby and two giant steps (G = 1 second) of two distinct
    ciphertexts: the model's words, computed once for every batch and tier below"""
    n, L, K = 16384, 7, 8
    bgs, ggs = [pow(5, 3, 2 * n), 2 * n - 1], [5, 1]
    cases = cases_for(orc, n, L, K, 3)
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    pts = [[uniform_plaintext(orc, cases[0], 2 * j + i) for i in range(2)] for j in range(2)]
    gcases = [cases[2], None]
    return cases, gcases, bgs, ggs, pts, cts, expected(orc, cases[:2], bgs, gcases, ggs, pts, None, cts)


@pytest.mark.parametrize("route", ["split_intt_ntt_up", "fused_up"])
def test_both_mod_up_routes_and_two_tiers(hx, ctx, dev, orc, made, headline, route):
    """batch 2 runs k_ksf_intt + k_ksf_ntt_up, the smallest batch with nb * L >= 2 * CUs runs k_ksf_up, for the ciphertext's mod-up and
    for every giant step's. baby_plans[0] in the strict tier (the others lazy) and in a lazy tier (the second baby plan strict) in turn"""
    cases, gcases, bgs, ggs, pts, cts, want = headline
    L = cases[0].L
    cus = torch_().cuda.get_device_properties(0).multi_processor_count
    nb = 2 if route == "split_intt_ntt_up" else -(-2 * cus // L)
    assert (nb * L >= 2 * cus) == (route == "fused_up") and nb <= 256, "one scratch chunk, on the route the name says"
    strict = 0 if route == "fused_up" else 1
    plans = plans_for(hx, ctx, cases, made, env={strict: {"HEXL_KS_NOLAZY": "1"}})
    tiers = [p.tiers()[0] for p in plans]
    assert all(t == 0 for t in tiers[strict][:cases[0].K]) and all(t > 0 for t in tiers[1 - strict][:cases[0].K])
    run_and_check(hx, ctx, dev, want, cases[0], plans[:2], bgs, [plans[2], None], ggs, pts, None, cts, nb)


def test_largest_ring(hx, ctx, dev, orc, made):
    """n = 32768: half-size exchanges in the transforms, 512 threads per workgroup in the gathering multiply-accumulate, k_galois
    without LDS for the first giant step's key-free part"""
    n, L, K, nb = 32768, 2, 3, 2
    bgs, ggs = [pow(5, 5, 2 * n), 3], [pow(5, 2, 2 * n), 2 * n - 1]
    cases = cases_for(orc, n, L, K, 4)
    plans = plans_for(hx, ctx, cases, made)
    pts = [[uniform_plaintext(orc, cases[0], 0), None], [uniform_plaintext(orc, cases[0], 1), uniform_plaintext(orc, cases[0], 2)]]
    cts = [uniform_ct(orc, cases[0], b) for b in range(nb)]
    want = expected(orc, cases[:2], bgs, cases[2:], ggs, pts, None, cts)
    run_and_check(hx, ctx, dev, want, cases[0], plans[:2], bgs, plans[2:], ggs, pts, None, cts, nb)


def test_more_than_eight_digits(hx, ctx, dev, orc, made):
    """L = 9: the multiply-accumulates built for up to 16 digits"""
    n, L, K, nb = 1024, 9, 10, 3
    bgs, ggs = [pow(5, 2, 2 * n), 1], [2 * n - 1, 1]
    cases = cases_for(orc, n, L, K, 3)
    plans = plans_for(hx, ctx, cases, made)
    pts = [[uniform_plaintext(orc, cases[0], 2 * j + i) for i in range(2)] for j in range(2)]
    ids = [uniform_plaintext(orc, cases[0], 7, rows=L), None]
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    gcases = [cases[2], None]
    want = expected(orc, cases[:2], bgs, gcases, ggs, pts, ids, cts)
    run_and_check(hx, ctx, dev, want, cases[0], plans[:2], bgs, [plans[2], None], ggs, pts, ids, cts, nb)


def test_chunks_with_a_ragged_tail_then_fewer_babies_then_the_parents():
    """HEXL_KS_CHUNK=3 (read once per process, so a child process): batch 8 runs two full chunks and a tail of two through the baby
    store, the t buffer and u; a second call with ONE baby step and batch 4 runs in the grown buffers with another slice stride; then
    hexl_keyswitch, hexl_linear_transform and hexl_rotate_hoisted on the same plans still give their models' words."""
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
from test_gpu_rotate_hoisted import cases_for, uniform_ct
from test_gpu_linear_transform import assert_output
from test_gpu_linear_transform_bsgs import expected, device_inputs
from hoist_model import limbs_of, rotate_hoisted
from lt_model import linear_transform, uniform_plaintext
dev = torch.device("cuda:0")
ctx = hx.Context(0)
n, L, K = 1024, 2, 3
bgs, ggs = [pow(5, 3, 2 * n), 2 * n - 1, 1], [3, 1, 5]
cases = cases_for(orc, n, L, K, 5)
plans = []
for case in cases:
    plans.append(hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch))
    plans[-1].set_keys(case.keys)
assert plans[0].scratch_bytes(3) == plans[0].scratch_bytes(100) > plans[0].scratch_bytes(2), "HEXL_KS_CHUNK=3 not in force"
assert hx.lt_bsgs_scratch_bytes(plans[0], 3, 100) == hx.lt_bsgs_scratch_bytes(plans[0], 3, 3) > hx.lt_bsgs_scratch_bytes(plans[0], 3, 2)
bcases, bplans = cases[:3], plans[:3]
gcases, gplans = [cases[3], None, cases[4]], [plans[3], None, plans[4]]
cts = [uniform_ct(orc, cases[0], b) for b in range(3)]
pt = lambda s: uniform_plaintext(orc, cases[0], s)
pts = [[pt(0), pt(1), None], [None, pt(2), pt(3)], [pt(4), None, None]]
ids = [None, uniform_plaintext(orc, cases[0], 9, rows=L), None]
for nb, nbaby in ((8, 3), (4, 1)):
    p_ = [row[:nbaby] for row in pts]
    i_ = ids if nbaby == 3 else [ids[1]] * 3                      # (one baby step: row 1 would be empty without an identity term)
    want = expected(orc, bcases[:nbaby], bgs[:nbaby], gcases, ggs, p_, i_, cts)
    d_ct, out, d_pts, d_ids = device_inputs(hx, dev, cts, nb, p_, i_)
    hx.linear_transform_bsgs(bplans[:nbaby], bgs[:nbaby], gplans, ggs, d_pts, out, d_ct, nb, d_ids)
    ctx.sync()
    assert_output(hx, want, out, nb, cases[0], "batch %%d: " %% nb)
lm = limbs_of(orc, cases[0])
tt, rr = cases[0].inputs(orc, 0)
d_r = hx.as_i64(rr).to(dev)
plans[0].keyswitch(d_r, hx.as_i64(tt).to(dev), 1)
lt_pts = [pt(0), pt(1)]
d_lt = torch.full_like(d_ct, -1)
hx.linear_transform(plans[:2], bgs[:2], [hx.as_i64(p).to(dev) for p in lt_pts], d_lt, d_ct, 4)
d_rot = torch.full_like(d_ct, -1)
hx.rotate_hoisted(plans[:1], bgs[:1], [d_rot], d_ct, 4)
ctx.sync()
assert np.array_equal(hx.to_u64(d_r), cases[0].expected(orc, tt, rr))
assert_output(hx, [linear_transform(orc, cases[:2], bgs[:2], lt_pts, None, ct, lm) for ct in cts], d_lt, 4, cases[0], "linear_transform: ")
assert_output(hx, [rotate_hoisted(orc, cases[0], ct, bgs[0], lm) for ct in cts], d_rot, 4, cases[0], "rotate_hoisted: ")
assert all(p.range_check() for p in plans)
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="3"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_on_a_caller_side_stream(hx, dev, orc, made):
    """a context of its own on a non-blocking side stream, the stream the only ordering: the input is poison (zeros, in range) until a
    copy queued on that stream behind a filler replaces it, the output is cloned on that stream, and only the stream is waited for"""
    torch = torch_()
    n, L, K, nb = 4096, 2, 3, 6
    ctx2 = hx.Context(0)
    made.append(ctx2)
    s = torch.cuda.Stream()
    ctx2.set_stream(s.cuda_stream)
    bcases, gcases, bplans, gplans, bgs, ggs, pts, ids = grid_of(orc, n, L, K, "3x2", False, made, hx, ctx2)
    cts = [uniform_ct(orc, bcases[0], b) for b in range(2)]
    want = expected(orc, bcases, bgs, gcases, ggs, pts, ids, cts)
    real, out, d_pts, d_ids = device_inputs(hx, dev, cts, nb, pts, ids)
    d_ct = torch.zeros_like(real)
    filler = torch.zeros(1 << 27, dtype=torch.int64, device=dev)
    for _ in range(2):                                                 # the second pass runs in warm buffers, with every kernel loaded
        d_ct.zero_()
        out.fill_(-1)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(4):
                filler.add_(1)
            d_ct.copy_(real, non_blocking=True)
            hx.linear_transform_bsgs(bplans, bgs, gplans, ggs, d_pts, out, d_ct, nb, d_ids)
            clone = out.clone()
        s.synchronize()                                                # the only wait
        assert_output(hx, want, clone, nb, bcases[0], "side stream: ")


@pytest.mark.parametrize("component", [0, 1])
def test_range_flag_is_raised_on_the_first_baby_plan(hx, ctx, dev, orc, made, component):
    n, L, K, nb = 1024, 2, 3, 2
    bcases, gcases, bplans, gplans, bgs, ggs, pts, ids = grid_of(orc, n, L, K, "2x2", False, made, hx, ctx)
    cts = [uniform_ct(orc, bcases[0], b) for b in range(nb)]
    others = [p for p in bplans[1:] + gplans if p is not None]
    d_ct, out, d_pts, d_ids = device_inputs(hx, dev, cts, nb, pts, ids)
    hx.linear_transform_bsgs(bplans, bgs, gplans, ggs, d_pts, out, d_ct, nb, d_ids)
    assert bplans[0].range_check() and all(p.range_check() for p in others), "in-range words: the flags stay clear"
    cts[1][(component * L + 1) * n + 17] = bcases[0].moduli[1]          # limb 1 of c0 / c1: a word equal to its modulus
    d_ct, out, d_pts, d_ids = device_inputs(hx, dev, cts, nb, pts, ids)
    hx.linear_transform_bsgs(bplans, bgs, gplans, ggs, d_pts, out, d_ct, nb, d_ids)
    assert not bplans[0].range_check(), "HEXL_W_RANGE expected on baby_plans[0]"
    assert all(p.range_check() for p in others)
    assert bplans[0].range_check(), "the check clears the flag"


def test_rejections(hx, ctx, dev, orc, made):
    torch = torch_()
    n, L, K = 1024, 2, 3
    cases = cases_for(orc, n, L, K, 4)
    plans = plans_for(hx, ctx, cases, made)
    per, ptw = 2 * L * n, (L + 1) * n
    buf = torch.full((3 * per + 4 * ptw,), -1, dtype=torch.int64, device=dev)
    ct, out, spare = buf[:per], buf[per:2 * per], buf[2 * per:3 * per]
    ct.zero_()
    pa, pb, pc, pid = (buf[3 * per + k * ptw:3 * per + (k + 1) * ptw] for k in range(4))
    for t in (pa, pb, pc, pid):
        t.fill_(1)
    bp, gp, bgs, ggs = plans[:2], [None, plans[2]], [3, 5], [1, 7]
    grid = [[pa, pb], [pc, None]]

    def refused(status, bp_=bp, bgs_=bgs, gp_=gp, ggs_=ggs, pts_=grid, out_=out, ct_=ct, ids_=None):
        with pytest.raises(hx.HexlError, match=f"status {status}$"):
            hx.linear_transform_bsgs(bp_, bgs_, gp_, ggs_, pts_, out_, ct_, 1, ids_)

    other_l = plans_for(hx, ctx, [KsCase(orc, n, 1, K, seed=3)], made)
    refused(-1, bp_=[plans[0], other_l[0]])                            # a baby plan with another L
    refused(-1, gp_=[other_l[0], plans[2]])                            # an unused giant plan (G = 1) that does not match
    other_q = plans_for(hx, ctx, [KsCase(orc, n, L, K, seed=3, bits=50)], made)
    refused(-1, gp_=[None, other_q[0]])                                # different moduli
    ctx2 = hx.Context(0)
    made.append(ctx2)
    refused(-1, bp_=[plans[0]] + plans_for(hx, ctx2, cases[1:2], made))  # a plan on another context
    ints = plans_for(hx, ctx, cases_for(orc, n, L, K, 3, bits=55), made)
    assert ints[0].tiers()[0][0] == -1
    refused(-1, bp_=ints[:2], gp_=[None, ints[2]])                     # integer kernels
    nokeys = hx.KeySwitchPlan(ctx, n, L, K, K, 2, cases[1].moduli, cases[1].modswitch)
    made.append(nokeys)
    refused(-2, bp_=[plans[0], nokeys])                                # HEXL_E_NOKEYS: a baby plan that is used
    refused(-2, gp_=[None, nokeys])                                    # ... a giant plan that is used
    hx.linear_transform_bsgs([plans[0], nokeys], bgs, [nokeys, plans[2]], ggs, [[pa, None], [pc, None]], spare, ct, 1)   # unused ones may lack keys
    ctx.sync()
    assert not bool((spare == -1).any())
    spare.fill_(-1)
    refused(-1, bp_=[plans[0], None])                                  # a NULL baby plan whose column has a plaintext
    refused(-1, gp_=[None, None])                                      # a NULL giant plan with G != 1
    refused(-1, pts_=[[pa, pb], [None, None]])                         # a giant row with no term at all
    refused(-1, bgs_=[3, 4])                                           # g even
    refused(-1, bgs_=[2 * n, 5])                                       # g = 2n
    refused(-1, ggs_=[1, 2 * n + 1])
    refused(-1, ggs_=[2, 7])                                           # G even, on the row whose plan is NULL
    refused(-1, out_=buf[per // 2:per // 2 + per])                     # d_out overlaps d_ct
    refused(-1, out_=ct)
    refused(-1, pts_=[[pa, out[per - 8:]], [pc, None]])                # d_out's last words inside a plaintext's range
    refused(-1, pts_=[[pa, pb], [out[:ptw], None]])                    # a plaintext inside d_out
    refused(-1, ids_=[None, out[L * n:]])                              # an identity plaintext inside d_out
    refused(-1, ids_=[spare[:L * n], None], out_=buf[per + L * n:2 * per + L * n])   # d_out's tail reaches an identity plaintext
    # raw calls: a size that overflows, batch == 0
    fn = hx.lib().hexl_linear_transform_bsgs
    vp = ctypes.c_void_p
    bh, gh = (vp * 2)(plans[0].h.value, plans[1].h.value), (vp * 2)(None, plans[2].h.value)
    ba, ga = (ctypes.c_uint64 * 2)(*bgs), (ctypes.c_uint64 * 2)(*ggs)
    ptrs = (vp * 4)(pa.data_ptr(), pb.data_ptr(), pc.data_ptr(), None)
    assert fn(bh, ba, 2, gh, ga, 2, ptrs, None, out.data_ptr(), ct.data_ptr(), (1 << 64) // (per * 8) + 1) == -1
    assert fn(bh, ba, 2, gh, ga, 2, ptrs, None, out.data_ptr(), ct.data_ptr(), 0) == 0                 # batch == 0: 0, nothing written
    assert fn(bh, ba, 2, gh, ga, 2, ptrs, None, None, ct.data_ptr(), 0) == -1                          # ... after the checks
    assert fn(bh, ba, 1 << 40, gh, ga, 1 << 40, ptrs, None, out.data_ptr(), ct.data_ptr(), 1) == -1    # a grid whose size overflows
    ctx.sync()
    assert bool((buf[per:3 * per] == -1).all()), "a refused or empty call wrote to an output"
    # n_baby == 0: every row has its identity term; without one it is refused
    ids = [pid[:L * n], pid[:L * n]]
    refused(-1, bp_=[], bgs_=[], pts_=[[], []], ids_=[pid[:L * n], None])
    hx.linear_transform_bsgs([], [], gp, ggs, [[], []], out, ct, 1, ids)
    ctx.sync()
    assert not bool((out == -1).any()) and bool((spare == -1).all())
    out.fill_(-1)
    hx.linear_transform_bsgs(bp, bgs, gp, ggs, grid, out, ct, 1, [pid[:L * n], None])   # adjacent buffers: accepted
    ctx.sync()
    assert bool((spare == -1).all()) and not bool((out == -1).any())
    assert bool((buf[3 * per:3 * per + 4 * ptw] == 1).all()), "the plaintexts are read, never written"


def test_end_to_end_decryption(hx, ctx, dev, orc, made):
    """real Galois keys over one secret: the device's words are the model's, and they decrypt under s to the baby-step/giant-step sum
    within the bound derived in bsgs_model.check_decrypts_bsgs"""
    rc = RlweCase(orc, 1024, 2, 3, 50, seed=4)
    baby, giant = bsgs_rlwe(orc, rc, "3x2")
    bgs, ggs, coeffs, id_coeffs = BSGS_GRIDS["3x2"]
    pts, ids = bsgs_plaintexts(rc, "3x2")
    used = [g for g in baby + giant if g is not None]
    plans = dict(zip(map(id, used), plans_for(hx, ctx, used, made)))
    pick = lambda xs: [None if g is None else plans[id(g)] for g in xs]
    want = expected(orc, baby, bgs, giant, ggs, pts, ids, [baby[0].ct])
    _, out, _, _ = run_and_check(hx, ctx, dev, want, baby[0], pick(baby), bgs, pick(giant), ggs, pts, ids, [baby[0].ct], 3)
    noise, bound = check_decrypts_bsgs(baby, giant, ggs, coeffs, id_coeffs, hx.to_u64(out).reshape(3, -1)[2])
    print(f"largest noise coefficient {noise}, bound {bound}")


def test_scratch_bytes_cover_what_a_first_call_allocates(hx, dev, orc, made):
    """hexl_lt_bsgs_scratch_bytes against the device memory a call takes on plans that have held nothing so far. A first call with
    other plans on the same context loads the kernels and sizes the context's table; the measured call then allocates the three
    buffers only. The allocator hands out whole 2 MiB pages, one rounding per buffer."""
    torch = torch_()
    n, L, K, nb = 16384, 3, 4, 8
    ctx2 = hx.Context(0)
    made.append(ctx2)
    cases = cases_for(orc, n, L, K, 2)
    bgs, ggs = [3], [5]
    pts = [[uniform_plaintext(orc, cases[0], 0)]]
    d_ct, out, d_pts, _ = device_inputs(hx, dev, [uniform_ct(orc, cases[0], 0)], nb, pts, None)
    grew = []
    for _ in range(2):
        plans = plans_for(hx, ctx2, cases, made)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        hx.linear_transform_bsgs(plans[:1], bgs, plans[1:], ggs, d_pts, out, d_ct, nb)
        torch.cuda.synchronize()
        grew.append(before - torch.cuda.mem_get_info()[0])
    said = hx.lt_bsgs_scratch_bytes(plans[0], 1, nb)
    assert said == nb * (2 * (L + 1) * n * 8 + 2 * L * n * 8) + plans[0].scratch_bytes(nb)
    print(f"reported {said} bytes, the call took {grew[1]} (the first call on the context {grew[0]})")
    assert 0 < grew[1] <= said + 3 * (2 << 20)
