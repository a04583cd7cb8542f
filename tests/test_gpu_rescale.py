"""GPU: hexl_rescale bit-exact against the model (tests/ckks_model.py rescale, which test_ckks_ops_model.py checks against big-integer
CRT rounding), every instance of every launch."""
import numpy as np
import pytest

from ckks_model import Limbs, rescale
from ks_util import KsCase, primes_below, seal_chain, tier_ladder

pytestmark = pytest.mark.gpu


def chain(orc, kind, K, n):
    if kind == "strict":
        return primes_below(orc, K, 1 << 52, n)
    if kind == "seal":
        return seal_chain(orc, K, n)
    if kind == "ladder":
        return tier_ladder(orc, K, n)
    return orc.primes(K, 51, n)


def run_case(hx, ctx, dev, orc, n, K, kind, n_limbs, ncomp, nb, seed=1):
    import torch
    qs = chain(orc, kind, K, n)
    case = KsCase(orc, n, 1, K, moduli=qs)
    plan = hx.KeySwitchPlan(ctx, n, 1, K, K, 2, case.moduli, case.modswitch)      # no keys: rescale does not need them
    lm = Limbs(orc, n, qs)
    distinct = min(nb, 3)
    inst = [np.concatenate([orc.splitmix(n, seed * 1009 + b * 101 + k * 13 + i, qs[i]) for k in range(ncomp) for i in range(n_limbs)])
            for b in range(distinct)]
    d_in = hx.as_i64(np.concatenate([inst[b % distinct] for b in range(nb)])).to(dev)
    d_out = torch.full((nb * ncomp * (n_limbs - 1) * n,), -1, dtype=torch.int64, device=dev)
    plan.rescale(d_out, d_in, nb, n_limbs, ncomp)
    ctx.sync()
    out = hx.to_u64(d_out).reshape(nb, -1)
    want = [rescale(lm, inst[b], 1, n_limbs, ncomp).reshape(-1) for b in range(distinct)]
    for b in range(nb):
        assert np.array_equal(out[b], want[b % distinct]), f"instance {b}"
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
