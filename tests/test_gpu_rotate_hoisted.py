"""GPU: hexl_rotate_hoisted against the exact model (tests/hoist_model.py, pinned to the oracle in test_hoist_model.py), bit for bit,
every instance of every output. The model's mod-up is computed once per distinct ciphertext and shared by the rotations, as the
launcher shares it. Rejections are host-side argument checks that return before any launch."""
import ctypes
import os

import numpy as np
import pytest

from ckks_model import first_mismatch, rotate
from hoist_model import limbs_of, mod_up, rotate_hoisted
from ks_util import KsCase, extreme_ciphertext, seal_chain

pytestmark = pytest.mark.gpu


def torch_():
    import torch
    return torch


def cases_for(orc, n, L, K, R, moduli=None, extreme_keys=False, bits=51):
    """R parameter sets with the same moduli and different keys (KsCase's keys follow the seed; extreme keys are the same for all)"""
    return [KsCase(orc, n, L, K, seed=90 + r, moduli=moduli, extreme_keys=extreme_keys, bits=bits) for r in range(R)]


def plans_for(hx, ctx, cases, made, env=None):
    """one plan per case; env[r]: environment of plan r's creation (HEXL_KS_NOLAZY is read by hexl_ks_plan_create)"""
    plans = []
    for r, case in enumerate(cases):
        extra = (env or {}).get(r, {})
        old = {k: os.environ.get(k) for k in extra}
        os.environ.update(extra)
        try:
            plan = hx.KeySwitchPlan(ctx, case.n, case.L, case.K, case.K, 2, case.moduli, case.modswitch)
        finally:
            for k, v in old.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        made.append(plan)
        plan.set_keys(case.keys)
        plans.append(plan)
    return plans


@pytest.fixture
def made():
    """plans and contexts of one test, closed in reverse order once everything queued has finished"""
    objs = []
    try:
        yield objs
    finally:
        torch_().cuda.synchronize()
        for o in reversed(objs):
            o.close()


def uniform_ct(orc, case, b):
    n, L = case.n, case.L
    return np.concatenate([orc.splitmix(n, 4000 + b * 977 + k * 17 + i, int(case.moduli[i])) for k in range(2) for i in range(L)])


def expected(orc, cases, gs, cts):
    """want[r][c]: the model's words for rotation r of distinct ciphertext c"""
    lm = limbs_of(orc, cases[0])
    ups = [mod_up(lm, cases[0], ct) for ct in cts]
    return [[rotate_hoisted(orc, case, ct, g, lm, u) for ct, u in zip(cts, ups)] for case, g in zip(cases, gs)]


def buffers(hx, dev, cts, nb, R):
    """device input of nb instances cycling over the distinct ones, and R outputs filled with -1 (written, not accumulated into)"""
    torch = torch_()
    base = hx.as_i64(np.stack(cts)).to(dev)
    d_ct = base[torch.arange(nb, device=dev) % len(cts)].reshape(-1).contiguous()
    return d_ct, [torch.full_like(d_ct, -1) for _ in range(R)]


def assert_outputs(hx, want, outs, nb, case, label=""):
    """instance b of output r against want[r][b % distinct], compared on the device; names the first wrong word"""
    torch = torch_()
    for r, out in enumerate(outs):
        w = hx.as_i64(np.stack(want[r])).to(out.device)
        idx = torch.arange(nb, device=out.device) % len(want[r])
        bad = (out.view(nb, -1) != w[idx]).any(dim=1)
        if bool(bad.any()):
            b = int(torch.nonzero(bad)[0])
            where = first_mismatch(hx.to_u64(out.view(nb, -1)[b]), want[r][b % len(want[r])], ("component", "limb", "coefficient"),
                                   (2, case.L, case.n))
            raise AssertionError(f"{label}rotation {r}: {int(bad.sum())} of {nb} instances wrong, the first is instance {b}, {where}")


def run_and_check(hx, ctx, dev, orc, cases, plans, gs, cts, nb, want=None, label=""):
    d_ct, outs = buffers(hx, dev, cts, nb, len(gs))
    hx.rotate_hoisted(plans, gs, outs, d_ct, nb)
    ctx.sync()
    assert_outputs(hx, want or expected(orc, cases, gs, cts), outs, nb, cases[0], label)
    return d_ct, outs


def chunk_of(plan):
    """instances per scratch chunk of the keyswitch, read off hexl_ks_scratch_bytes as test_gpu_galois.py does"""
    chunk = plan.scratch_bytes(1 << 24) // plan.scratch_bytes(1)
    assert chunk >= 2 and plan.scratch_bytes(chunk) == plan.scratch_bytes(chunk + 1) > plan.scratch_bytes(chunk - 1)
    return chunk


@pytest.mark.parametrize("family", ["uniform", "extreme"])
def test_three_rotations_smallest_ring(hx, ctx, dev, orc, made, family):
    n, L, K, nb = 1024, 2, 3, 5
    gs = [1, 3, 2 * n - 1]
    cases = cases_for(orc, n, L, K, 3, extreme_keys=family == "extreme")
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], b) if family == "uniform" else extreme_ciphertext(cases[0], b, 2) for b in range(nb)]
    d_ct, outs = run_and_check(hx, ctx, dev, orc, cases, plans, gs, cts, nb)
    # g = 1: word for word hexl_rotate's output and the oracle's keyswitch
    d_rot = torch_().full_like(d_ct, -1)
    plans[0].rotate(d_rot, d_ct, nb, 1)
    ctx.sync()
    assert torch_().equal(d_rot, outs[0])
    assert np.array_equal(hx.to_u64(outs[0]).reshape(nb, -1)[nb - 1], rotate(orc, cases[0], cts[nb - 1], 1))


def test_seal_chain_powers_of_five_and_a_repeated_element(hx, ctx, dev, orc, made):
    """g = 5^k, k = 1 ... 8, on a chain of mixed tiers, and 5^3 once more on a ninth plan with other keys"""
    n, L, K, nb = 4096, 5, 6, 3
    gs = [pow(5, k, 2 * n) for k in range(1, 9)] + [pow(5, 3, 2 * n)]
    cases = cases_for(orc, n, L, K, len(gs), moduli=seal_chain(orc, K, n))
    assert not np.array_equal(cases[2].keys[0], cases[8].keys[0])
    plans = plans_for(hx, ctx, cases, made)
    assert plans[0].tiers()[1], "the seal chain mixes tiers"
    cts = [uniform_ct(orc, cases[0], b) for b in range(nb)]
    _, outs = run_and_check(hx, ctx, dev, orc, cases, plans, gs, cts, nb)
    assert not torch_().equal(outs[2], outs[8]), "the same g with different keys gives different words"


@pytest.fixture(scope="module")
def big_ring(orc):
    """n = 16384, L = 3, K = 4, two rotations of two distinct ciphertexts: the model's words, computed once for both batches"""
    n, L, K = 16384, 3, 4
    gs = [pow(5, 3, 2 * n), 2 * n - 1]
    cases = cases_for(orc, n, L, K, 2)
    cts = [uniform_ct(orc, cases[0], b) for b in range(2)]
    return cases, gs, cts, expected(orc, cases, gs, cts)


@pytest.mark.parametrize("route", ["split_intt_ntt_up", "fused_up"])
def test_both_mod_up_routes_and_two_tiers(hx, ctx, dev, orc, made, big_ring, route):
    """batch 2 runs k_ksf_intt + k_ksf_ntt_up; a batch with nb * L >= 2 * CUs runs k_ksf_up. One plan in the strict tier and one in a
    lazy tier (the same moduli: HEXL_KS_NOLAZY at the plan's creation), in either order: the shared mod-up runs on plans[0]'s tier"""
    cases, gs, cts, want = big_ring
    L = cases[0].L
    cus = torch_().cuda.get_device_properties(0).multi_processor_count
    nb = 2 if route == "split_intt_ntt_up" else -(-2 * cus // L)
    assert nb <= 256, "one scratch chunk"
    strict_first = route == "fused_up"
    plans = plans_for(hx, ctx, cases, made, env={0 if strict_first else 1: {"HEXL_KS_NOLAZY": "1"}})
    tiers = [p.tiers()[0] for p in plans]
    assert all(t == 0 for t in tiers[0 if strict_first else 1][:cases[0].K]) and all(t > 0 for t in tiers[1 if strict_first else 0][:cases[0].K])
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, cts, nb, want=want)


def test_largest_ring_gathers_from_global_memory(hx, ctx, dev, orc, made):
    """n = 32768: half-size exchanges in the transforms, k_galois without LDS, 512 threads per workgroup in the gathering MAC"""
    n, L, K, nb = 32768, 2, 3, 2
    gs = [pow(5, 5, 2 * n), 3]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, [uniform_ct(orc, cases[0], b) for b in range(nb)], nb)


def test_more_than_eight_digits(hx, ctx, dev, orc, made):
    """L = 9: the gathering MAC built for up to 16 digits (up to 8 is the other instantiation)"""
    n, L, K, nb = 1024, 9, 10, 2
    gs = [pow(5, 2, 2 * n), 2 * n - 1]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, [uniform_ct(orc, cases[0], b) for b in range(nb)], nb)


def test_two_chunks_then_a_smaller_batch(hx, ctx, dev, orc, made):
    """one scratch chunk plus 3: the second chunk's mod-up overwrites u behind the last rotation of the first. Three distinct inputs do
    not divide the chunk, so the last instances of chunk 1 and the first of chunk 2 differ, and row r of chunk 2 differs from row r of
    chunk 1. Then a smaller batch on the same plans, in the scratch the first call left."""
    n, L, K = 1024, 2, 3
    gs = [pow(5, 3, 2 * n), 2 * n - 1]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    chunk = chunk_of(plans[0])
    assert chunk % 3
    cts = [uniform_ct(orc, cases[0], b) for b in range(3)]
    want = expected(orc, cases, gs, cts)
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, cts, chunk + 3, want=want, label="two chunks: ")
    run_and_check(hx, ctx, dev, orc, cases, plans, gs, cts[::-1], 7, want=[w[::-1] for w in want], label="second call: ")


def test_keyswitch_and_rotate_unchanged_afterwards(hx, ctx, dev, orc, made):
    """the scratch and the flags a hoisted call leaves are sane: plans[0].keyswitch and plans[1].rotate still give the oracle's words"""
    torch = torch_()
    n, L, K, nb = 1024, 2, 3, 4
    gs = [3, 5]
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    cts = [uniform_ct(orc, cases[0], b) for b in range(nb)]
    d_ct, _ = run_and_check(hx, ctx, dev, orc, cases, plans, gs, cts, nb)
    tt, rr = cases[0].inputs(orc, 0)
    d_r = hx.as_i64(rr).to(dev)
    plans[0].keyswitch(d_r, hx.as_i64(tt).to(dev), 1)
    d_rot = torch.full_like(d_ct, -1)
    plans[1].rotate(d_rot, d_ct, nb, 5)
    ctx.sync()
    assert np.array_equal(hx.to_u64(d_r), cases[0].expected(orc, tt, rr))
    got = hx.to_u64(d_rot).reshape(nb, -1)
    for b in range(nb):
        assert np.array_equal(got[b], rotate(orc, cases[1], cts[b], 5)), f"instance {b}"
    assert plans[0].range_check() and plans[1].range_check()


def test_range_flag_is_raised_on_the_first_plan(hx, ctx, dev, orc, made):
    n, L, K, nb = 1024, 2, 3, 2
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    assert plans[0].range_check() and plans[1].range_check()
    cts = [uniform_ct(orc, cases[0], b) for b in range(nb)]
    cts[1][(L + 1) * n + 17] = cases[0].moduli[1]                       # c1, limb 1: a word equal to its modulus
    d_ct, outs = buffers(hx, dev, cts, nb, 2)
    hx.rotate_hoisted(plans, [3, 5], outs, d_ct, nb)
    assert not plans[0].range_check(), "HEXL_W_RANGE expected on plans[0]"
    assert plans[1].range_check()
    assert plans[0].range_check(), "the check clears the flag"


def test_on_a_caller_side_stream(hx, dev, orc, made):
    """a context of its own on a non-blocking side stream, the stream the only ordering: the input is poison (zeros, in range) until a
    copy queued on that stream behind a filler replaces it, the outputs are cloned on that stream, and only the stream is waited for"""
    torch = torch_()
    n, L, K, nb = 4096, 2, 3, 6
    gs = [pow(5, 3, 2 * n), 1]
    ctx2 = hx.Context(0)
    made.append(ctx2)
    s = torch.cuda.Stream()
    ctx2.set_stream(s.cuda_stream)
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx2, cases, made)
    cts = [uniform_ct(orc, cases[0], b) for b in range(3)]
    want = expected(orc, cases, gs, cts)
    real, outs = buffers(hx, dev, cts, nb, 2)
    d_ct = torch.zeros_like(real)
    filler = torch.zeros(1 << 27, dtype=torch.int64, device=dev)
    for _ in range(2):                                                 # the second pass runs in warm scratch, with every kernel loaded
        d_ct.zero_()
        for o in outs:
            o.fill_(-1)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(4):
                filler.add_(1)
            d_ct.copy_(real, non_blocking=True)
            hx.rotate_hoisted(plans, gs, outs, d_ct, nb)
            clones = [o.clone() for o in outs]
        s.synchronize()                                                # the only wait
        assert_outputs(hx, want, clones, nb, cases[0], "side stream: ")


def test_rejections(hx, ctx, dev, orc, made):
    torch = torch_()
    n, L, K = 1024, 2, 3
    cases = cases_for(orc, n, L, K, 2)
    plans = plans_for(hx, ctx, cases, made)
    per = 2 * L * n
    buf = torch.full((4 * per,), -1, dtype=torch.int64, device=dev)
    ct, a, b = buf[:per], buf[per:2 * per], buf[2 * per:3 * per]
    ct.zero_()
    gs = [3, 5]

    def refused(status, plans_, gs_, outs_, ct_=ct):
        with pytest.raises(hx.HexlError, match=f"status {status}$"):
            hx.rotate_hoisted(plans_, gs_, outs_, ct_, 1)

    other_l = plans_for(hx, ctx, [KsCase(orc, n, 1, K, seed=3)], made)
    refused(-1, [plans[0], other_l[0]], gs, [a, b])                    # different L
    other_q = plans_for(hx, ctx, [KsCase(orc, n, L, K, seed=3, bits=50)], made)
    refused(-1, [plans[0], other_q[0]], gs, [a, b])                    # different moduli
    ctx2 = hx.Context(0)
    made.append(ctx2)
    refused(-1, [plans[0]] + plans_for(hx, ctx2, cases[1:], made), gs, [a, b])     # a plan on another context
    ints = plans_for(hx, ctx, cases_for(orc, n, L, K, 2, bits=55), made)
    assert ints[0].tiers()[0][0] == -1
    refused(-1, ints, gs, [a, b])                                      # integer kernels
    nokeys = hx.KeySwitchPlan(ctx, n, L, K, K, 2, cases[1].moduli, cases[1].modswitch)
    made.append(nokeys)
    refused(-2, [plans[0], nokeys], gs, [a, b])                        # HEXL_E_NOKEYS
    refused(-1, plans, [3, 4], [a, b])                                 # g even
    refused(-1, plans, [2 * n, 3], [a, b])                             # g = 2n
    refused(-1, plans, [2 * n + 1, 3], [a, b])
    refused(-1, plans, gs, [buf[per // 2:per // 2 + per], b])          # d_outs[0] overlaps d_ct
    refused(-1, plans, gs, [ct, b])
    refused(-1, plans, gs, [a, buf[per + per // 2:2 * per + per // 2]])    # d_outs[1] overlaps d_outs[0]
    refused(-1, plans, gs, [a, a])
    with pytest.raises(ValueError):
        hx.rotate_hoisted(plans, [3], [a, b], ct, 1)
    # n_rot = 0 with valid arguments: 0, and nothing is written
    hs = (ctypes.c_void_p * 2)(*[p.h.value for p in plans])
    g_arr = (ctypes.c_uint64 * 2)(*gs)
    assert hx.lib().hexl_rotate_hoisted(hs, g_arr, 0, hx.ptr_array([a, b]), ct.data_ptr(), 1) == 0
    assert hx.lib().hexl_rotate_hoisted(hs, g_arr, 2, hx.ptr_array([a, b]), ct.data_ptr(), 0) == 0      # batch == 0 likewise
    ctx.sync()
    assert bool((buf[per:] == -1).all()), "a refused or empty call wrote to an output"
    hx.rotate_hoisted(plans, gs, [a, b], ct, 1)                        # adjacent buffers: accepted
    ctx.sync()
    assert bool((buf[3 * per:] == -1).all()) and not bool((a == -1).any())
