"""GPU: hexl_rns_ntt_fwd / hexl_rns_ntt_inv bit-exact against the oracle's keyswitch transforms limb by limb (tests/rns_model.py rns_ntt
= ckks_model.Limbs.ntt / .intt), every polynomial of every launch; the first wrong word is named."""
import numpy as np
import pytest

from ckks_model import Limbs, rescale, rescale_input
from ks_util import KsCase
from rns_model import TIER_OF, assert_instances, chain, ntt_input, rns_ntt

pytestmark = pytest.mark.gpu

FAMILIES = ("uniform", "extreme", "zero")


def make_plan(hx, ctx, orc, n, qs):
    K = len(qs)
    case = KsCase(orc, n, 1, K, moduli=qs)
    return hx.KeySwitchPlan(ctx, n, 1, K, K, 2, case.moduli, case.modswitch)       # no keys: the transforms do not need them


def launch(hx, plan, dev, x, count, n_limbs, inverse, in_place=False):
    """one launch on x[count][n_limbs][n]; the output starts as all-ones words; returns (output words, input words after the launch)"""
    import torch
    d_in = hx.as_i64(np.ascontiguousarray(x).reshape(-1)).to(dev)
    d_out = d_in if in_place else torch.full_like(d_in, -1)
    (plan.rns_ntt_inv if inverse else plan.rns_ntt_fwd)(d_out, d_in, count, n_limbs)
    plan.ctx.sync()
    return hx.to_u64(d_out), hx.to_u64(d_in)


def check_transforms(hx, ctx, dev, plan, lm, n_limbs, count, label, families=FAMILIES, seed=1, in_place=False):
    """forward and inverse, `count` polynomial sets cycling over the families (the inverse adds `edge`), against the model"""
    n = lm.n
    for inverse in (False, True):
        fams = tuple(families) + (("edge",) if inverse else ())
        distinct = [ntt_input(lm, n_limbs, fams[c % len(fams)], c, seed, inverse) for c in range(min(count, max(3, len(fams))))]
        x = np.stack([distinct[c % len(distinct)] for c in range(count)])
        got, after = launch(hx, plan, dev, x, count, n_limbs, inverse, in_place)
        want = [rns_ntt(lm, d, n_limbs, inverse) for d in distinct]
        which = f"{label}: {'inverse' if inverse else 'forward'}{' in place' if in_place else ''}, n={n} n_limbs={n_limbs} count={count}"
        assert_instances(got, want, count, ("limb", "coefficient"), (n_limbs, n), which)
        if not in_place:
            assert np.array_equal(after, x.reshape(-1)), f"{which}: the input was written"
        for i in range(n_limbs):
            assert int(got.reshape(count, n_limbs, n)[:, i].max()) < lm.qs[i], f"{which}: limb {i} holds a word that is not canonical"


@pytest.mark.parametrize("n", [1024, 2048, 4096, 8192, 16384, 32768])
def test_rns_ntt_every_ring_dimension(hx, ctx, dev, orc, n):
    K = 4
    qs = chain(orc, "gen", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    check_transforms(hx, ctx, dev, plan, Limbs(orc, n, qs), K, 6, "gen")
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "period3_top", "strict_bottom", "period6", "period12"])
def test_rns_ntt_every_tier_at_16384(hx, ctx, dev, orc, kind):
    """plans uniformly in one tier: the only way into the <14, 4, 0 / 3 / 6 / 12> kernels; plan.tiers() pins the selection"""
    n, K = 16384, 4
    qs = chain(orc, kind, K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    assert plan.tiers() == ([TIER_OF[kind]] * K, False), f"{kind}: the plan no longer selects the kernels this case is for"
    check_transforms(hx, ctx, dev, plan, Limbs(orc, n, qs), K, 6, kind)
    plan.close()


@pytest.mark.parametrize("kind,n", [("seal", 16384), ("seal", 4096), ("ladder", 16384)])
def test_rns_ntt_mixed_tiers(hx, ctx, dev, orc, kind, n):
    """limbs of different tiers (LAZY = -1, the schedule looked up per limb), all seven limbs, the special prime among them"""
    K = 7
    qs = chain(orc, kind, K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    tiers, mixed = plan.tiers()
    assert len(set(tiers)) > 1, f"{kind}: the limbs no longer differ in tier"
    check_transforms(hx, ctx, dev, plan, Limbs(orc, n, qs), K, 6, kind)
    plan.close()


def test_rns_ntt_every_limb_count_on_one_plan(hx, ctx, dev, orc):
    """n_limbs = 1 ... K with three polynomial sets: odd numbers of transforms, the limb-major split at every n_limbs"""
    n, K = 2048, 5
    qs = chain(orc, "gen", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    lm = Limbs(orc, n, qs)
    for n_limbs in range(1, K + 1):
        check_transforms(hx, ctx, dev, plan, lm, n_limbs, 3, "gen", families=("uniform", "extreme"), seed=n_limbs)
    plan.close()


def test_rns_ntt_more_workgroups_than_compute_units(hx, ctx, dev, orc):
    """560 transforms in one launch; the polynomial sets cycle over three distinct inputs"""
    n, K = 1024, 4
    qs = chain(orc, "gen", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    check_transforms(hx, ctx, dev, plan, Limbs(orc, n, qs), K, 140, "gen", families=("uniform", "extreme"))
    plan.close()


@pytest.mark.parametrize("kind,n,K", [("gen", 16384, 4), ("seal", 2048, 7), ("strict", 32768, 3)])
def test_rns_ntt_in_place_matches_out_of_place(hx, ctx, dev, orc, kind, n, K):
    qs = chain(orc, kind, K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    check_transforms(hx, ctx, dev, plan, Limbs(orc, n, qs), K, 4, kind, in_place=True)
    plan.close()


def test_rns_ntt_rejections(hx, ctx, dev, orc):
    import torch
    n, K, count = 4096, 4, 2
    case = KsCase(orc, n, 2, K, seed=1)
    plan = hx.KeySwitchPlan(ctx, n, 2, K, K, 2, case.moduli, case.modswitch)
    buf = torch.zeros((2 * count * K + 1) * n, dtype=torch.int64, device=dev)
    a, b = buf[:count * K * n], buf[count * K * n:2 * count * K * n]
    for fn in (plan.rns_ntt_fwd, plan.rns_ntt_inv):
        with pytest.raises(hx.HexlError):
            fn(buf[n:n + count * K * n], a, count, K)              # offset by one polynomial: neither in place nor apart
        with pytest.raises(hx.HexlError):
            fn(a, buf[n:n + count * K * n], count, K)
        for n_limbs in (0, K + 1):
            with pytest.raises(hx.HexlError):
                fn(b, a, count, n_limbs)
        fn(b, a, count, K)                                         # adjacent: accepted
        fn(a, a, count, K)                                         # in place: accepted
        fn(b, a, 0, K)                                             # nothing to do
    ctx.sync()
    plan.close()
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)                   # a plan on the integer kernels (moduli >= 2^52): out of scope
    plan = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    for fn in (plan.rns_ntt_fwd, plan.rns_ntt_inv):
        with pytest.raises(hx.HexlError):
            fn(b, a, 1, 2)
    plan.close()


@pytest.mark.parametrize("kind,n", [("gen", 4096), ("seal", 16384)])
def test_rns_ntt_round_trip_and_plan_state(hx, ctx, dev, orc, kind, n):
    """forward in place, inverse in place: the input again. Then a rescale on the same plan and a forward transform at n_limbs - 1, all in
    stream order: the transforms neither depend on nor disturb what the plan keeps for its other entry points"""
    import torch
    K, count = 6, 4
    n_limbs = K - 1
    qs = chain(orc, kind, K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    lm = Limbs(orc, n, qs)
    x = np.stack([ntt_input(lm, n_limbs, ("uniform", "extreme")[c % 2], c, seed=7) for c in range(count)])
    d = hx.as_i64(x.reshape(-1)).to(dev)
    plan.rns_ntt_fwd(d, d, count, n_limbs)
    ctx.sync()
    fwd = hx.to_u64(d).copy()
    assert_instances(fwd, [rns_ntt(lm, x[c], n_limbs) for c in range(count)], count, ("limb", "coefficient"), (n_limbs, n), f"{kind}: forward")
    plan.rns_ntt_inv(d, d, count, n_limbs)
    ctx.sync()
    assert_instances(hx.to_u64(d), list(x), count, ("limb", "coefficient"), (n_limbs, n), f"{kind}: inverse of forward")
    # rescale (fills the plan's per-level constants and scratch), then the transforms again with one limb fewer
    ct = np.stack([rescale_input(lm, n_limbs, 2, "uniform", b, seed=3) for b in range(2)])             # [2][2][n_limbs][n]
    d_ct = hx.as_i64(ct.reshape(-1)).to(dev)
    d_rs = torch.full((2 * 2 * (n_limbs - 1) * n,), -1, dtype=torch.int64, device=dev)
    d_co = torch.full_like(d_rs, -1)
    y = x[:, :n_limbs - 1]
    d_y = hx.as_i64(np.ascontiguousarray(y).reshape(-1)).to(dev)
    d_fy = torch.full_like(d_y, -1)
    plan.rescale(d_rs, d_ct, 2, n_limbs, 2)
    plan.rns_ntt_inv(d_co, d_rs, 2 * 2, n_limbs - 1)               # the rescaled ciphertext to coefficient form
    plan.rns_ntt_fwd(d_fy, d_y, count, n_limbs - 1)
    ctx.sync()
    rs = rescale(lm, ct, 2, n_limbs, 2)                            # [2][2][n_limbs - 1][n]
    assert_instances(hx.to_u64(d_rs), list(rs.reshape(4, -1)), 4, ("limb", "coefficient"), (n_limbs - 1, n), f"{kind}: rescale between transforms")
    assert_instances(hx.to_u64(d_co), [rns_ntt(lm, c, n_limbs - 1, True) for c in rs.reshape(4, n_limbs - 1, n)], 4, ("limb", "coefficient"),
                     (n_limbs - 1, n), f"{kind}: inverse of the rescale's output")
    assert_instances(hx.to_u64(d_fy), [fwd.reshape(count, n_limbs, n)[c, :n_limbs - 1] for c in range(count)], count, ("limb", "coefficient"),
                     (n_limbs - 1, n), f"{kind}: forward at n_limbs - 1 after the rescale")
    plan.close()


def test_rns_ntt_agrees_with_the_standalone_transforms(hx, ctx, dev, orc):
    """limb by limb, hexl_ntt_fwd / hexl_ntt_inv with HEXL tables for MinimalPrimitiveRoot(2n, q_i) give the same words"""
    n, K, count = 4096, 4, 3
    qs = chain(orc, "gen", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    lm = Limbs(orc, n, qs)
    x = np.stack([ntt_input(lm, K, ("uniform", "extreme", "uniform")[c], c, seed=5) for c in range(count)])     # [count][K][n]
    fwd, _ = launch(hx, plan, dev, x, count, K, False)
    inv, _ = launch(hx, plan, dev, fwd, count, K, True)
    fwd, inv = fwd.reshape(count, K, n), inv.reshape(count, K, n)
    assert np.array_equal(inv, x), "inverse of forward is not the input"
    for i, q in enumerate(qs):
        t = orc.HexlTables(n, q)
        tabs = [hx.as_i64(a).to(dev) for a in (t.roots, t.precon, t.inv_roots, t.inv_precon)]
        d = hx.as_i64(np.ascontiguousarray(x[:, i])).to(dev)
        ctx.ntt_fwd(d, tabs[0], tabs[1], q, n)
        ctx.sync()
        alone = hx.to_u64(d).reshape(count, n).copy()
        assert_instances(fwd[:, i], list(alone), count, ("coefficient",), (n,), f"limb {i}: forward against hexl_ntt_fwd")
        ctx.ntt_inv(d, tabs[2], tabs[3], q, t.inv_n, t.inv_n_w, n)
        ctx.sync()
        assert_instances(inv[:, i], list(hx.to_u64(d).reshape(count, n)), count, ("coefficient",), (n,), f"limb {i}: inverse against hexl_ntt_inv")
    plan.close()
