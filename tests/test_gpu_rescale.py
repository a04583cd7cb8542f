"""GPU: hexl_rescale bit-exact against the model (tests/ckks_model.py rescale, which test_ckks_ops_model.py checks against big-integer
CRT rounding), every instance of every launch."""
import numpy as np
import pytest

from ckks_model import Limbs, first_mismatch, rescale, rescale_input
from ks_util import KsCase, big_dropped, primes_below, primes_from, seal_chain, small_dropped, tier_ladder

pytestmark = pytest.mark.gpu

BOUNDARY = (1 << 51) + (1 << 44)                                  # f64_arith.hpp LAZY_MAX_MODULUS: period 3 at and below, strict above


def chain(orc, kind, K, n):
    if kind == "strict":
        return primes_below(orc, K, 1 << 52, n)
    if kind == "seal":
        return seal_chain(orc, K, n)
    if kind == "ladder":
        return tier_ladder(orc, K, n)
    if kind == "period6":
        return primes_below(orc, K, 1 << 50, n)
    if kind == "period12":
        return primes_below(orc, K, 1 << 49, n)
    if kind == "period3_top":
        return primes_below(orc, K, BOUNDARY, n)
    if kind == "strict_bottom":
        return primes_from(orc, K, BOUNDARY, n)
    if kind in ("big_dropped", "small_dropped"):
        assert K == 4
        return (big_dropped if kind == "big_dropped" else small_dropped)(orc, n)
    return orc.primes(K, 51, n)


def assert_rescaled(out, want, nb, ncomp, l, n, distinct, label):
    """every instance of a launch against the expectation of its distinct input; the first wrong word is named"""
    out = out.reshape(nb, -1)
    for b in range(nb):
        if not np.array_equal(out[b], want[b % distinct]):
            where = first_mismatch(out[b], want[b % distinct], ("component", "limb", "coefficient"), (ncomp, l, n))
            raise AssertionError(f"{label}: instance {b}, {where}")


def run_case(hx, ctx, dev, orc, n, K, kind, n_limbs, ncomp, nb, seed=1, families=("uniform",), tiers=None):
    """one plan, one launch of nb instances; instance b is drawn from families[b % len(families)] (ckks_model.rescale_input)"""
    import torch
    qs = chain(orc, kind, K, n)
    case = KsCase(orc, n, 1, K, moduli=qs)
    plan = hx.KeySwitchPlan(ctx, n, 1, K, K, 2, case.moduli, case.modswitch)      # no keys: rescale does not need them
    if tiers is not None:
        assert plan.tiers() == tiers, f"{kind}: the plan no longer selects the kernels this case is for"
    lm = Limbs(orc, n, qs)
    distinct = min(nb, max(3, len(families)))
    inst = [rescale_input(lm, n_limbs, ncomp, families[b % len(families)], b, seed).reshape(-1) for b in range(distinct)]
    d_in = hx.as_i64(np.concatenate([inst[b % distinct] for b in range(nb)])).to(dev)
    d_out = torch.full((nb * ncomp * (n_limbs - 1) * n,), -1, dtype=torch.int64, device=dev)
    plan.rescale(d_out, d_in, nb, n_limbs, ncomp)
    ctx.sync()
    want = [rescale(lm, inst[b], 1, n_limbs, ncomp).reshape(-1) for b in range(distinct)]
    assert_rescaled(hx.to_u64(d_out), want, nb, ncomp, n_limbs - 1, n, distinct, f"{kind} n={n} n_limbs={n_limbs} families={families}")
    plan.close()


@pytest.mark.parametrize("n", [1024, 2048, 4096, 8192, 16384, 32768])
def test_rescale_every_ring_dimension(hx, ctx, dev, orc, n):
    run_case(hx, ctx, dev, orc, n, 4, "gen", 3, 2, 3)


@pytest.mark.parametrize("n_limbs", [2, 3, 4, 5, 6, 7])
def test_rescale_every_level(hx, ctx, dev, orc, n_limbs):
    run_case(hx, ctx, dev, orc, 16384, 8, "gen", n_limbs, 2, 2, seed=n_limbs)


@pytest.mark.parametrize("n,K,kind,n_limbs,ncomp,nb", [(16384, 7, "seal", 6, 2, 4), (16384, 7, "seal", 3, 3, 2),
                                                       (16384, 8, "ladder", 7, 1, 2), (4096, 5, "ladder", 4, 3, 3),
                                                       (16384, 4, "strict", 3, 2, 3), (32768, 4, "seal", 3, 2, 2),
                                                       (32768, 3, "strict", 2, 1, 2)])
def test_rescale_mixed_tiers_and_components(hx, ctx, dev, orc, n, K, kind, n_limbs, ncomp, nb):
    run_case(hx, ctx, dev, orc, n, K, kind, n_limbs, ncomp, nb)


ALL = ("uniform", "edge", "extreme")


@pytest.mark.parametrize("n", [16384, 4096])
@pytest.mark.parametrize("kind,period", [("period6", 6), ("period12", 12)])
def test_rescale_plans_uniformly_in_the_period6_and_period12_tiers(hx, ctx, dev, orc, kind, period, n):
    """every limb just below 2^50 / 2^49: at N = 16384 the only plans that reach run_rescale<14, 4, 6> / <14, 4, 12> (dispatch_rescale;
    every other ring dimension maps them to period 3). plan.tiers() pins the selection: uniform, rounding-edge and extreme instances"""
    K = 4
    run_case(hx, ctx, dev, orc, n, K, kind, 3, 2, 6, families=ALL, tiers=([period] * K, False) if n == 16384 else None)
    run_case(hx, ctx, dev, orc, n, K, kind, 2, 3, 3, seed=2, families=ALL)


@pytest.mark.parametrize("n", [16384, 1024])
@pytest.mark.parametrize("kind,period", [("period3_top", 3), ("strict_bottom", 0)])
def test_rescale_on_both_sides_of_the_lazy_strict_boundary(hx, ctx, dev, orc, kind, period, n):
    """the largest moduli of the period-3 tier and the smallest strict ones (2^51 (1 + 2^-7)), rounding-edge and extreme instances"""
    K = 4
    run_case(hx, ctx, dev, orc, n, K, kind, 3, 2, 4, families=("edge", "extreme"), tiers=([period] * K, False))


@pytest.mark.parametrize("n", [16384, 2048, 32768])
@pytest.mark.parametrize("kind,K,levels", [("gen", 5, ((4, 2), (2, 3))), ("strict", 4, ((3, 1), (2, 2))),
                                           ("seal", 7, ((6, 2), (3, 3))), ("ladder", 8, ((7, 1), (4, 2)))])
def test_rescale_rounding_edges_and_extreme_words_in_every_family(hx, ctx, dev, orc, kind, K, levels, n):
    """the inputs where round(X / q_l) changes (dropped limb's INTT at 0, 1, half - 1 ... half + 2, q_l - 2, q_l - 1) and the largest
    magnitudes of the kept limbs, per modulus family, two levels each, 1 to 3 components; N = 32768 is the branch that loads c_i
    behind the transform (G::HALF_ONLY)"""
    for n_limbs, ncomp in levels:
        run_case(hx, ctx, dev, orc, n, K, kind, n_limbs, ncomp, 4, seed=n_limbs, families=("edge", "extreme"))


@pytest.mark.parametrize("n", [16384, 4096])
@pytest.mark.parametrize("kind", ["big_dropped", "small_dropped"])
def test_rescale_large_prime_beside_small_ones(hx, ctx, dev, orc, kind, n):
    """big_dropped: the largest prime below 2^52 dropped beside 30-bit limbs -- reduce(s + fix_i) takes a 22-bit quotient out of one
    rounded multiply; small_dropped: a 27-bit prime dropped beside 52- and 51-bit limbs"""
    run_case(hx, ctx, dev, orc, n, 4, kind, 3, 2, 6, families=ALL)
    run_case(hx, ctx, dev, orc, n, 4, kind, 3, 3, 3, seed=5, families=("edge",))


@pytest.mark.parametrize("n,K,kind", [(16384, 8, "ladder"), (2048, 5, "seal"), (2048, 5, "gen")])
def test_rescale_one_plan_walked_down_the_chain(hx, ctx, dev, orc, n, K, kind):
    """One plan used as a CKKS computation uses it: n_limbs = K - 1 down to 2, every output the next call's input, nothing but stream
    order between the calls; every intermediate against the model. Then, still without a sync between the calls: two levels already
    visited (the cached per-level constants read again, with every other level's row filled since), a call with more
    (instance, component) pairs than any before (the grow-only scratch is replaced while earlier launches are queued) and a smaller
    one after it."""
    import torch
    qs = chain(orc, kind, K, n)
    case = KsCase(orc, n, 1, K, moduli=qs)
    plan = hx.KeySwitchPlan(ctx, n, 1, K, K, 2, case.moduli, case.modswitch)
    lm = Limbs(orc, n, qs)
    nb, ncomp, top = 3, 2, K - 1
    x = np.stack([rescale_input(lm, top, ncomp, ALL[b % 3], b, seed=9) for b in range(nb)])          # [nb][ncomp][top][n]
    d = {top: hx.as_i64(x.reshape(-1)).to(dev)}
    for nl in range(top, 1, -1):
        d[nl - 1] = torch.full((nb * ncomp * (nl - 1) * n,), -1, dtype=torch.int64, device=dev)
        plan.rescale(d[nl - 1], d[nl], nb, nl, ncomp)
    ctx.sync()
    want = {top: x}
    for nl in range(top, 1, -1):
        want[nl - 1] = rescale(lm, want[nl], nb, nl, ncomp)
        assert_rescaled(hx.to_u64(d[nl - 1]), want[nl - 1].reshape(nb, -1), nb, ncomp, nl - 1, n, nb, f"{kind} n={n}: walk, n_limbs={nl}")
    # second group, same plan: repeated levels, regrowth, a smaller call
    mid = max(2, top // 2)
    big_nb, big_comp = 7, 3
    y = np.stack([rescale_input(lm, mid, big_comp, ALL[b % 3], b, seed=11) for b in range(big_nb)])
    d_y = hx.as_i64(y.reshape(-1)).to(dev)
    outs = [torch.full((nb * ncomp * (top - 1) * n,), -1, dtype=torch.int64, device=dev),
            torch.full((nb * ncomp * (mid - 1) * n,), -1, dtype=torch.int64, device=dev),
            torch.full((big_nb * big_comp * (mid - 1) * n,), -1, dtype=torch.int64, device=dev),
            torch.full((1 * 1 * (top - 1) * n,), -1, dtype=torch.int64, device=dev)]
    plan.rescale(outs[0], d[top], nb, top, ncomp)                 # level top again
    plan.rescale(outs[1], d[mid], nb, mid, ncomp)                 # a level in the middle again, fed by the walk's own output
    plan.rescale(outs[2], d_y, big_nb, mid, big_comp)             # 21 (instance, component) pairs after 6: the scratch regrows
    plan.rescale(outs[3], d[top][:top * n], 1, top, 1)            # ... and one pair: instance 0, component 0 of the first input
    ctx.sync()
    assert_rescaled(hx.to_u64(outs[0]), want[top - 1].reshape(nb, -1), nb, ncomp, top - 1, n, nb, f"{kind} n={n}: level {top} repeated")
    assert_rescaled(hx.to_u64(outs[1]), want[mid - 1].reshape(nb, -1), nb, ncomp, mid - 1, n, nb, f"{kind} n={n}: level {mid} repeated")
    assert_rescaled(hx.to_u64(outs[2]), rescale(lm, y, big_nb, mid, big_comp).reshape(big_nb, -1), big_nb, big_comp, mid - 1, n, big_nb,
                    f"{kind} n={n}: larger batch x components")
    assert_rescaled(hx.to_u64(outs[3]), want[top - 1][0, 0].reshape(1, -1), 1, 1, top - 1, n, 1, f"{kind} n={n}: smaller call")
    plan.close()


@pytest.mark.parametrize("n,nb,ncomp", [(16384, 258, 1), (1024, 4097, 1), (32768, 130, 1)])
def test_rescale_across_chunks(hx, ctx, dev, orc, n, nb, ncomp):
    run_case(hx, ctx, dev, orc, n, 3, "gen", 2, ncomp, nb)


def test_rescale_rejections(hx, ctx, dev, orc):
    import torch
    n = 4096
    buf = torch.zeros(4 * 2 * 3 * n, dtype=torch.int64, device=dev)
    a, b = buf[:2 * 3 * n], buf[2 * 3 * n:]
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)                   # integer-path plan: out of scope
    plan = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    with pytest.raises(hx.HexlError):
        plan.rescale(b, a, 1, 2, 2)
    plan.close()
    case = KsCase(orc, n, 2, 4, seed=1)
    plan = hx.KeySwitchPlan(ctx, n, 2, 4, 4, 2, case.moduli, case.modswitch)
    for n_limbs, ncomp in ((1, 2), (4, 2), (0, 2), (3, 0), (3, 4)):          # 2 <= n_limbs <= K - 1, 1 <= components <= 3
        with pytest.raises(hx.HexlError):
            plan.rescale(b, a, 1, n_limbs, ncomp)
    with pytest.raises(hx.HexlError):
        plan.rescale(buf[3 * n:], a, 1, 3, 2)                      # overlap
    plan.rescale(b, a, 1, 3, 2)                                    # adjacent, before any keys: accepted
    ctx.sync()
    plan.close()


def test_rescale_rejects_ring_dimensions_the_plan_does_not_take(hx, ctx, orc):
    """n is the plan's: a plan outside 1024 ... 32768 cannot be created in the first place"""
    case = KsCase(orc, 1024, 1, 3, seed=1)
    with pytest.raises(hx.HexlError):
        hx.KeySwitchPlan(ctx, 512, 1, 3, 3, 2, case.moduli, case.modswitch)
