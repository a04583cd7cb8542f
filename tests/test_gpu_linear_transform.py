"""GPU: hexl_linear_transform against the exact model (tests/lt_model.py, pinned in test_lt_model.py), bit for bit, every instance,
compared on the device. The model's mod-up is computed once per distinct ciphertext (two per case) and shared by the rotations, as the
launcher shares it. Every output buffer starts as -1: the call writes it. Rejections are host-side argument checks that return before
any launch. Helpers of test_gpu_rotate_hoisted.py are reused by import."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ckks_model import first_mismatch
from hoist_model import limbs_of, mod_up, rotate_hoisted
from ks_util import KsCase, RlweCase, extreme_ciphertext, extreme_words, seal_chain
from lt_model import check_decrypts, linear_transform, ones_plaintext, sparse_plaintext, uniform_plaintext
from test_gpu_rotate_hoisted import cases_for, chunk_of, made, plans_for, torch_, uniform_ct  # noqa: F401  (made: a fixture)
from test_lt_model import LT_COEFFS, LT_GS, LT_ID_COEFFS, rlwe_rotations

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def extreme_plaintext(case, salt, rows=None):
    """[rows][n] words from ks_util.extreme_words (q - 1, beside q / 2, 0, 1), row L of L + 1 below the special prime"""
    limbs = (list(range(case.L)) + [case.K - 1])[:case.L + 1 if rows is None else rows]
    return np.concatenate([extreme_words(case.n, int(case.moduli[i]), salt + 2 * s) for s, i in enumerate(limbs)])


def expected(orc, cases, gs, pts, pt_id, cts):
    """want[c]: the model's words for distinct ciphertext c"""
    lm = limbs_of(orc, cases[0])
    return [linear_transform(orc, cases, gs, pts, pt_id, ct, lm, mod_up(lm, cases[0], ct)) for ct in cts]


def device_inputs(hx, dev, cts, nb, pts, pt_id):
    torch = torch_()
    base = hx.as_i64(np.stack(cts)).to(dev)
    d_ct = base[torch.arange(nb, device=dev) % len(cts)].reshape(-1).contiguous()
    return d_ct, torch.full_like(d_ct, -1), [hx.as_i64(p).to(dev) for p in pts], None if pt_id is None else hx.as_i64(pt_id).to(dev)


def assert_output(hx, want, out, nb, case, label=""):
    """instance b against want[b % distinct], compared on the device; names the first wrong word"""
    torch = torch_()
    w = hx.as_i64(np.stack(want)).to(out.device)
    bad = (out.view(nb, -1) != w[torch.arange(nb, device=out.device) % len(want)]).any(dim=1)
    if bool(bad.any()):
        b = int(torch.nonzero(bad)[0])
        where = first_mismatch(hx.to_u64(out.view(nb, -1)[b]), want[b % len(want)], ("component", "limb", "coefficient"), (2, case.L, case.n))
        raise AssertionError(f"{label}{int(bad.sum())} of {nb} instances wrong, the first is instance {b}, {where}")


def run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, pt_id, cts, nb, want=None, label=""):
    d_ct, out, d_pts, d_id = device_inputs(hx, dev, cts, nb, pts, pt_id)
    hx.linear_transform(plans, gs, d_pts, out, d_ct, nb, d_id)
    ctx.sync()
    assert_output(hx, want or expected(orc, cases, gs, pts, pt_id, cts), out, nb, cases[0], label)
    return d_ct, out, d_pts, d_id


@pytest.mark.parametrize("g", ["1", "3", "2n-1"])
def test_one_rotation_all_ones_is_rotate_hoisted(hx, ctx, dev, orc, made, g):
    n, L, K, nb = 1024, 2, 3, 5
    g = {"1": 1, "3": 3, "2n-1": 2 * n - 1}[g]
    cases = cases_for(orc, n, L, K, 1)
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], 0), extreme_ciphertext(cases[0], 1, 2)]
    d_ct, out, _, _ = run_and_check(hx, ctx, dev, orc, cases, plans, [g], [ones_plaintext(cases[0])], None, cts, nb)
    d_rot = torch_().full_like(d_ct, -1)
    hx.rotate_hoisted(plans, [g], [d_rot], d_ct, nb)
    ctx.sync()
    assert torch_().equal(d_rot, out), "one rotation weighted by ones must be hexl_rotate_hoisted's words"


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("family", ["uniform", "extreme"])
def test_three_rotations_smallest_ring(hx, ctx, dev, orc, made, family, identity):
    n, L, K, nb = 1024, 2, 3, 5
    gs = [1, 3, 2 * n - 1]
    ext = family == "extreme"
    cases = cases_for(orc, n, L, K, 3, extreme_keys=ext)
    plans = plans_for(hx, ctx, cases, made)
    cts = [extreme_ciphertext(cases[0], b, 2) if ext else uniform_ct(orc, cases[0], b) for b in range(2)]
    pts = [extreme_plaintext(cases[0], 1 + r) if ext else uniform_plaintext(orc, cases[0], r) for r in range(3)]
    pt_id = None if not identity else extreme_plaintext(cases[0], 5, rows=L) if ext else uniform_plaintext(orc, cases[0], 9, rows=L)
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, pt_id, cts, nb)
    assert plans[0].range_check(), "in-range words must not raise the range flag"


def test_seal_chain_powers_of_five_and_a_repeated_element(hx, ctx, dev, orc, made):
    """g = 5^k, k = 1 ... 8, on a chain of mixed tiers, 5^3 once more with other keys and another plaintext, the identity term, and a
    batch that is no multiple of anything"""
    n, L, K, nb = 4096, 5, 6, 70
    gs = [pow(5, k, 2 * n) for k in range(1, 9)] + [pow(5, 3, 2 * n)]
    cases = cases_for(orc, n, L, K, len(gs), moduli=seal_chain(orc, K, n))
    assert not np.array_equal(cases[2].keys[0], cases[8].keys[0])
    plans = plans_for(hx, ctx, cases, made)
    assert plans[0].tiers()[1], "the seal chain mixes tiers"
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(len(gs))]
    assert not np.array_equal(pts[2], pts[8])
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, uniform_plaintext(orc, cases[0], 40, rows=L), cts, nb)


@pytest.fixture(scope="module")
def headline(orc):
    """n = 16384 on the headline chain (L = 7, K = 8, 51-bit primes), two rotations of two distinct ciphertexts: the model's words,
    computed once for every batch and tier below"""
    n, L, K = 16384, 7, 8
    gs = [pow(5, 3, 2 * n), 2 * n - 1]
    cases = cases_for(orc, n, L, K, 2)
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(2)]
    return cases, gs, pts, cts, expected(orc, cases, gs, pts, None, cts)


@pytest.mark.parametrize("route", ["split_intt_ntt_up", "fused_up"])
def test_both_mod_up_routes_and_two_tiers(hx, ctx, dev, orc, made, headline, route):
    """batch 5 runs k_ksf_intt + k_ksf_ntt_up; the smallest batch with nb * L >= 2 * CUs runs k_ksf_up. One plan in the strict tier and
    one in a lazy tier (the same moduli: HEXL_KS_NOLAZY at the plan's creation), in either order: everything but the keys is plans[0]'s"""
    cases, gs, pts, cts, want = headline
    L = cases[0].L
    cus = int(ctx.describe().split(" CUs")[0].split()[-1])
    assert cus == torch_().cuda.get_device_properties(0).multi_processor_count
    nb = 5 if route == "split_intt_ntt_up" else -(-2 * cus // L)
    assert (nb * L >= 2 * cus) == (route == "fused_up") and nb <= 256, "one scratch chunk, on the route the name says"
    strict_first = route == "fused_up"
    plans = plans_for(hx, ctx, cases, made, env={0 if strict_first else 1: {"HEXL_KS_NOLAZY": "1"}})
    tiers = [p.tiers()[0] for p in plans]
    assert all(t == 0 for t in tiers[0 if strict_first else 1][:cases[0].K]) and all(t > 0 for t in tiers[1 if strict_first else 0][:cases[0].K])
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, None, cts, nb, want=want)


def test_largest_ring(hx, ctx, dev, orc, made):
    """n = 32768: half-size exchanges in the transforms, 512 threads per workgroup in the gathering multiply-accumulate"""
    n, L, K, nb = 32768, 3, 4, 2
    gs = [pow(5, 5, 2 * n), 3]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(2)]
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, None, [uniform_ct(orc, cases[0], b) for b in range(nb)], nb)


def test_more_than_eight_digits(hx, ctx, dev, orc, made):
    """L = 9: the multiply-accumulate built for up to 16 digits (up to 8 is the other instantiation)"""
    n, L, K, nb = 1024, 9, 10, 3
    gs = [pow(5, 2, 2 * n), 2 * n - 1]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(2)]
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, uniform_plaintext(orc, cases[0], 7, rows=L),
                  [uniform_ct(orc, cases[0], b) for b in range(2)], nb)


def test_chunks_with_a_ragged_tail_then_the_grown_scratch():
    """HEXL_KS_CHUNK=3 (read once per process, so a child process): batch 1 sizes the scratch for one instance; batch 8 grows it and runs
    two full chunks and a tail of two, the accumulator rewritten by each chunk's first rotation; batch 4 then runs in the grown scratch.
    Three distinct ciphertexts: row r of one chunk differs from row r of the next."""
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
from test_gpu_rotate_hoisted import cases_for, uniform_ct
from test_gpu_linear_transform import expected, device_inputs, assert_output
from lt_model import uniform_plaintext
dev = torch.device("cuda:0")
ctx = hx.Context(0)
n, L, K = 1024, 2, 3
gs = [pow(5, 3, 2 * n), 2 * n - 1, 1]
cases = cases_for(orc, n, L, K, 3)
plans = []
for case in cases:
    plans.append(hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch))
    plans[-1].set_keys(case.keys)
assert plans[0].scratch_bytes(3) == plans[0].scratch_bytes(100) > plans[0].scratch_bytes(2), "HEXL_KS_CHUNK=3 not in force"
cts = [uniform_ct(orc, cases[0], b) for b in range(3)]
pts = [uniform_plaintext(orc, cases[0], r) for r in range(3)]
pt_id = uniform_plaintext(orc, cases[0], 9, rows=L)
want = expected(orc, cases, gs, pts, pt_id, cts)
for nb in (1, 8, 4):
    d_ct, out, d_pts, d_id = device_inputs(hx, dev, cts, nb, pts, pt_id)
    hx.linear_transform(plans, gs, d_pts, out, d_ct, nb, d_id)
    ctx.sync()
    assert_output(hx, want, out, nb, cases[0], "batch %%d: " %% nb)
assert all(p.range_check() for p in plans)
print("CHUNKS OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="3"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout


def test_plans_serve_keyswitch_and_rotate_hoisted_afterwards(hx, ctx, dev, orc, made):
    """the scratch and the flags a linear transform leaves are sane: plans[0].keyswitch and hexl_rotate_hoisted on the same plans still
    give their models' words"""
    torch = torch_()
    n, L, K, nb = 1024, 2, 3, 4
    gs = [3, 5]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(2)]
    d_ct, _, _, _ = run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, None, cts, nb)
    tt, rr = cases[0].inputs(orc, 0)
    d_r = hx.as_i64(rr).to(dev)
    plans[0].keyswitch(d_r, hx.as_i64(tt).to(dev), 1)
    outs = [torch.full_like(d_ct, -1) for _ in gs]
    hx.rotate_hoisted(plans, gs, outs, d_ct, nb)
    ctx.sync()
    assert np.array_equal(hx.to_u64(d_r), cases[0].expected(orc, tt, rr))
    lm = limbs_of(orc, cases[0])
    for r, (case, g) in enumerate(zip(cases, gs)):
        assert_output(hx, [rotate_hoisted(orc, case, ct, g, lm) for ct in cts], outs[r], nb, case, f"rotate_hoisted {r}: ")
    assert plans[0].range_check() and plans[1].range_check()


def test_on_a_caller_side_stream(hx, dev, orc, made):
    """a context of its own on a non-blocking side stream, the stream the only ordering: the input is poison (zeros, in range) until a
    copy queued on that stream behind a filler replaces it, the output is cloned on that stream, and only the stream is waited for"""
    torch = torch_()
    n, L, K, nb = 4096, 2, 3, 6
    gs = [pow(5, 3, 2 * n), 1]
    ctx2 = hx.Context(0)
    made.append(ctx2)
    s = torch.cuda.Stream()
    ctx2.set_stream(s.cuda_stream)
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx2, cases, made)
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(2)]
    pt_id = uniform_plaintext(orc, cases[0], 9, rows=L)
    want = expected(orc, cases, gs, pts, pt_id, cts)
    real, out, d_pts, d_id = device_inputs(hx, dev, cts, nb, pts, pt_id)
    d_ct = torch.zeros_like(real)
    filler = torch.zeros(1 << 27, dtype=torch.int64, device=dev)
    for _ in range(2):                                                 # the second pass runs in warm scratch, with every kernel loaded
        d_ct.zero_()
        out.fill_(-1)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(4):
                filler.add_(1)
            d_ct.copy_(real, non_blocking=True)
            hx.linear_transform(plans, gs, d_pts, out, d_ct, nb, d_id)
            clone = out.clone()
        s.synchronize()                                                # the only wait
        assert_output(hx, want, clone, nb, cases[0], "side stream: ")


def test_output_is_written_not_accumulated_into(hx, ctx, dev, orc, made):
    """the same call into a buffer of -1 and into the buffer a different call left: the same words"""
    n, L, K, nb = 2048, 2, 3, 3
    gs = [5, 2 * n - 1]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(2)]
    want = expected(orc, cases, gs, pts, None, cts)
    d_ct, out, d_pts, _ = run_and_check(hx, ctx, dev, orc, cases, plans, gs, pts, None, cts, nb, want=want)
    assert not bool((out == -1).any())
    first = out.clone()
    hx.linear_transform(plans[::-1], gs, d_pts, out, d_ct, nb)          # other keys per element: other words
    ctx.sync()
    assert not torch_().equal(out, first)
    hx.linear_transform(plans, gs, d_pts, out, d_ct, nb)
    ctx.sync()
    assert torch_().equal(out, first)


@pytest.mark.parametrize("component", [0, 1])
def test_range_flag_is_raised_on_the_first_plan(hx, ctx, dev, orc, made, component):
    n, L, K, nb = 1024, 2, 3, 2
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], b) for b in range(nb)]
    pts = [uniform_plaintext(orc, cases[0], r) for r in range(2)]
    d_ct, out, d_pts, _ = device_inputs(hx, dev, cts, nb, pts, None)
    hx.linear_transform(plans, [3, 5], d_pts, out, d_ct, nb)
    assert plans[0].range_check() and plans[1].range_check(), "in-range words: the flag stays clear"
    cts[1][(component * L + 1) * n + 17] = cases[0].moduli[1]           # limb 1 of c0 / c1: a word equal to its modulus
    d_ct, out, d_pts, _ = device_inputs(hx, dev, cts, nb, pts, None)
    hx.linear_transform(plans, [3, 5], d_pts, out, d_ct, nb)
    assert not plans[0].range_check(), "HEXL_W_RANGE expected on plans[0]"
    assert plans[1].range_check()
    assert plans[0].range_check(), "the check clears the flag"


def test_rejections(hx, ctx, dev, orc, made):
    torch = torch_()
    n, L, K = 1024, 2, 3
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    per, ptw = 2 * L * n, (L + 1) * n
    buf = torch.full((3 * per + 4 * ptw,), -1, dtype=torch.int64, device=dev)
    ct, out, spare = buf[:per], buf[per:2 * per], buf[2 * per:3 * per]
    ct.zero_()
    pa, pb, pid = (buf[3 * per + k * ptw:3 * per + (k + 1) * ptw] for k in range(3))
    for t in (pa, pb, pid):
        t.fill_(1)
    gs = [3, 5]

    def refused(status, plans_, gs_, pts_, out_=out, ct_=ct, pid_=None):
        with pytest.raises(hx.HexlError, match=f"status {status}$"):
            hx.linear_transform(plans_, gs_, pts_, out_, ct_, 1, pid_)

    other_l = plans_for(hx, ctx, [KsCase(orc, n, 1, K, seed=3)], made)
    refused(-1, [plans[0], other_l[0]], gs, [pa, pb])                  # different L
    other_q = plans_for(hx, ctx, [KsCase(orc, n, L, K, seed=3, bits=50)], made)
    refused(-1, [plans[0], other_q[0]], gs, [pa, pb])                  # different moduli
    ctx2 = hx.Context(0)
    made.append(ctx2)
    refused(-1, [plans[0]] + plans_for(hx, ctx2, cases[1:], made), gs, [pa, pb])   # a plan on another context
    ints = plans_for(hx, ctx, cases_for(orc, n, L, K, 2, bits=55), made)
    assert ints[0].tiers()[0][0] == -1
    refused(-1, ints, gs, [pa, pb])                                    # integer kernels
    nokeys = hx.KeySwitchPlan(ctx, n, L, K, K, 2, cases[1].moduli, cases[1].modswitch)
    made.append(nokeys)
    refused(-2, [plans[0], nokeys], gs, [pa, pb])                      # HEXL_E_NOKEYS
    refused(-1, plans, [3, 4], [pa, pb])                               # g even
    refused(-1, plans, [2 * n, 3], [pa, pb])                           # g = 2n
    refused(-1, plans, [2 * n + 1, 3], [pa, pb])
    refused(-1, plans, gs, [pa, pb], out_=buf[per // 2:per // 2 + per])  # d_out overlaps d_ct
    refused(-1, plans, gs, [pa, pb], out_=ct)
    refused(-1, plans, gs, [pa, out[per - 8:]])                        # d_out's last words inside d_pts[1]'s range
    refused(-1, plans, gs, [out[:ptw], pb])                            # d_pts[0] inside d_out
    refused(-1, plans, gs, [pa, pb], pid_=out[L * n:])                 # d_pt_identity inside d_out
    refused(-1, plans, gs, [pa, pb], pid_=spare[:L * n], out_=buf[per + L * n:2 * per + L * n])   # d_out's tail reaches d_pt_identity
    # raw calls: null entries, n_rot == 0, batch == 0
    fn = hx.lib().hexl_linear_transform
    hs = (ctypes.c_void_p * 2)(*[p.h.value for p in plans])
    g_arr = (ctypes.c_uint64 * 2)(*gs)
    ptrs = hx.ptr_array([pa, pb])
    assert fn(hs, g_arr, ptrs, 0, None, out.data_ptr(), ct.data_ptr(), 1) == -1                        # n_rot == 0
    assert fn((ctypes.c_void_p * 2)(plans[0].h.value, None), g_arr, ptrs, 2, None, out.data_ptr(), ct.data_ptr(), 1) == -1
    assert fn(hs, g_arr, (ctypes.c_void_p * 2)(pa.data_ptr(), None), 2, None, out.data_ptr(), ct.data_ptr(), 1) == -1
    assert fn(hs, g_arr, ptrs, 2, None, out.data_ptr(), ct.data_ptr(), (1 << 64) // (per * 8) + 1) == -1  # a size that overflows
    assert fn(hs, g_arr, ptrs, 2, None, out.data_ptr(), ct.data_ptr(), 0) == 0                         # batch == 0: 0, nothing written
    assert fn(hs, g_arr, ptrs, 2, None, None, ct.data_ptr(), 0) == -1                                  # ... after the checks
    with pytest.raises(ValueError):
        hx.linear_transform(plans, [3], [pa, pb], out, ct, 1)
    ctx.sync()
    assert bool((buf[per:3 * per] == -1).all()), "a refused or empty call wrote to an output"
    hx.linear_transform(plans, gs, [pa, pb], out, ct, 1, pid[:L * n])  # adjacent buffers: accepted
    ctx.sync()
    assert bool((spare == -1).all()) and not bool((out == -1).any())
    assert bool((buf[3 * per:3 * per + 3 * ptw] == 1).all()), "the plaintexts are read, never written"


def test_end_to_end_decryption(hx, ctx, dev, orc, made):
    """real Galois keys over one secret: the device's words are the model's, and they decrypt under s to
    sum_r pt_r . sigma_{g_r}(m) + pt_id . m within (sum of the plaintexts' 1-norms) . 2^24"""
    rc = RlweCase(orc, 1024, 2, 3, 50, seed=4)
    grs = rlwe_rotations(orc, rc)
    plans = plans_for(hx, ctx, grs, made)
    pts = [sparse_plaintext(rc, c) for c in LT_COEFFS]
    pt_id = sparse_plaintext(rc, LT_ID_COEFFS, rows=rc.L)
    _, out, _, _ = run_and_check(hx, ctx, dev, orc, grs, plans, LT_GS(rc.n), pts, pt_id, [grs[0].ct], 3)
    got = hx.to_u64(out).reshape(3, -1)
    noise, bound = check_decrypts(grs, LT_COEFFS, LT_ID_COEFFS, got[2])
    print(f"largest noise coefficient {noise}, bound {bound}")
