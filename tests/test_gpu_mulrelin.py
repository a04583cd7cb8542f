"""GPU parity: hexl_multiply_relinearize (ciphertext multiply + relinearize in one pass, SURVEY 8f.4 -- the use-case of
the reference's combined image, device/dyadic_multiply_keyswitch.cpp:4-5) against the COMPOSITION of the two oracle
calls the reference's flow makes: DyadicMultiply (tests/test_dyadic_multiply.cpp:59-82 semantics), then KeySwitch with
result = product components 0..1 and t_target = component 2 (tests/test_dyadic_multiply_keyswitch.cpp:295-313 runs the
two primitives of that image back to back)."""
import numpy as np
import pytest

from ckks_model import first_mismatch
from ks_util import EXTREME_TIERS, TIERS, KsCase, extreme_ciphertext, primes_below, seal_chain, tier_ladder, tier_moduli

pytestmark = pytest.mark.gpu


def operands(orc, case, b, which):
    n, L = case.n, case.L
    return np.concatenate([orc.splitmix(n, case.seed * 7 + b * 131 + which * 17 + p * 5 + i, int(case.moduli[i]))
                           for p in range(2) for i in range(L)])


def composed(orc, case, a, b):
    n, L = case.n, case.L
    prod = orc.dyadic(a, b, n, case.moduli[:L], exact=True)              # [3][L][n]
    out = prod[:2 * L * n].copy()
    orc.keyswitch(out, prod[2 * L * n:].copy(), n, L, case.K, L + 1, case.moduli, case.keys, case.modswitch)
    return out


@pytest.mark.parametrize("n,L,K,nb,strict", [(16384, 6, 7, 2, False), (16384, 7, 8, 96, False), (16384, 3, 4, 5, True),
                                             (8192, 3, 4, 70, False), (1024, 2, 3, 300, False), (8192, 2, 3, 3, True),
                                             (2048, 2, 3, 150, False), (4096, 3, 4, 120, False), (4096, 2, 3, 4, True),
                                             # round 5: limbs of different tiers (one launch per tier group, keyswitch_x.hip run_chunk_x)
                                             (16384, 6, 7, 40, "seal"), (16384, 3, 4, 5, "ladder"), (4096, 3, 4, 60, "seal"),
                                             # ... and N = 32768: every transform as two 16384-point halves (k_ksh_*<..., FUSED>)
                                             (32768, 3, 4, 5, False), (32768, 2, 3, 130, False), (32768, 3, 4, 4, True), (32768, 3, 4, 4, "seal")])
def test_vs_composition_of_the_oracles(hx, ctx, dev, orc, n, L, K, nb, strict):
    moduli = primes_below(orc, K, 1 << 52, n) if strict is True else None      # just below 2^52: the strict FP64 kernels
    if strict == "seal":
        moduli = seal_chain(orc, K, n)
    elif strict == "ladder":
        moduli = tier_ladder(orc, K, n)
    run_fused(hx, ctx, dev, orc, n, L, K, nb, moduli)


def run_fused(hx, ctx, dev, orc, n, L, K, nb, moduli, extreme=False):
    """nb instances (three distinct ones repeated) through hexl_multiply_relinearize, every one against the composition of the oracles;
    extreme: keys and both operands from ks_util.extreme_words, the two operands on different patterns"""
    import torch
    case = KsCase(orc, n, L, K, seed=40 + L, moduli=moduli, extreme_keys=extreme)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    distinct = min(nb, 3)
    if extreme:
        A = [extreme_ciphertext(case, b, 2) for b in range(distinct)]
        B = [extreme_ciphertext(case, b, 2, salt=4) for b in range(distinct)]
        assert not any(np.array_equal(a, b) for a, b in zip(A, B))
    else:
        A = [operands(orc, case, b, 0) for b in range(distinct)]
        B = [operands(orc, case, b, 1) for b in range(distinct)]
    d_a = hx.as_i64(np.concatenate([A[b % distinct] for b in range(nb)])).to(dev)
    d_b = hx.as_i64(np.concatenate([B[b % distinct] for b in range(nb)])).to(dev)
    d_out = torch.full((nb * 2 * L * n,), -1, dtype=torch.int64, device=dev)   # written, not accumulated into
    plan.multiply_relinearize(d_out, d_a, d_b, nb)
    ctx.sync()
    out = hx.to_u64(d_out).reshape(nb, -1)
    want = [composed(orc, case, A[b], B[b]) for b in range(distinct)]
    for b in range(nb):
        assert np.array_equal(out[b], want[b % distinct]), \
            f"instance {b}, {first_mismatch(out[b], want[b % distinct], ('component', 'limb', 'coefficient'), (2, L, n))}"
    plan.close()


# the tiers of ks_util.TIERS that change nothing but the moduli (no environment knob): these run in this process
THREE = ("period3_tier_top_2^51_plus_2^44", "strict_just_below_2^52", "mixed_seal_chain_strict_and_period12")


@pytest.mark.parametrize("tier,n,nb", [(t, n, nb) for t in EXTREME_TIERS for n, nb in ((16384, 40), (8192, 5))] +
                         [(t, n, nb) for t in THREE for n, nb in ((32768, 3), (2048, 5))])
def test_extreme_operands_and_keys_in_every_tier(hx, ctx, dev, orc, tier, n, nb):
    """The fused pass starts its bound chains from the operands: mul_mod(a, b) into the transforms, reduce(mul_mod + mul_mod) as the
    old result of the mod-down epilogue. Every word of both operands and of the keys at q - 1, beside q / 2, 0 or 1 (extreme_words), in
    every tier the keyswitch runs such inputs in. N = 8192 is the geometry whose epilogue goes through LDS (G::KL > 2); N = 32768 (the
    half-transform kernels k_ksh_*<..., FUSED>) and N = 2048 in three tiers."""
    assert TIERS[tier][0] == {}, "a tier that needs an environment variable belongs in a child process"
    run_fused(hx, ctx, dev, orc, n, 3, 4, nb, tier_moduli(orc, tier, n, 4), extreme=True)


@pytest.mark.parametrize("tier,n,nb", [(t, 16384, 5) for t in ("skip_period6_just_below_2^50", "skip_period12_just_below_2^49",
                                                               "period3_tier_top_2^51_plus_2^44", "strict_just_above_2^51_plus_2^44",
                                                               "skip_period3_ratio_1p24", "noskip_period3_mixed_51_and_30bit")] +
                         [("skip_period3_ratio_1p24", 32768, 3), ("noskip_period3_mixed_51_and_30bit", 32768, 3)])
def test_uniform_operands_in_the_tiers_the_fused_pass_had_not_seen(hx, ctx, dev, orc, tier, n, nb):
    """period 6, period 12, both sides of the lazy / strict boundary, and the two plans that select the SKIP (moduli within a factor
    1.25) and the non-SKIP (51-bit beside 30-bit) instantiation of the fused main kernel"""
    assert TIERS[tier][0] == {}
    run_fused(hx, ctx, dev, orc, n, 3, 4, nb, tier_moduli(orc, tier, n, 4))


def test_rejects_what_it_does_not_cover(hx, ctx, dev, orc):
    n = 4096                                                     # moduli >= 2^52: the integer kernels have no fused pass
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)
    plan = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    import torch
    z = torch.zeros(2 * 2 * n, dtype=torch.int64, device=dev)
    z2 = torch.zeros(2 * 2 * n, dtype=torch.int64, device=dev)
    z3 = torch.zeros(2 * 2 * n, dtype=torch.int64, device=dev)
    with pytest.raises(hx.HexlError):
        plan.multiply_relinearize(z, z2, z3, 1)
    plan.close()


def test_rejects_output_aliasing_an_operand(hx, ctx, dev, orc):
    """d_out is written while the operands are still being read (component 0 is stored before component 1's operands are
    loaded): overlap with d_a or d_b is refused instead of silently producing a wrong ciphertext"""
    n, L, K = 16384, 2, 3
    case = KsCase(orc, n, L, K, seed=3)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    import torch
    a = torch.zeros(2 * 2 * L * n, dtype=torch.int64, device=dev)
    b = torch.zeros(2 * L * n, dtype=torch.int64, device=dev)
    for out, x, y in ((a[:2 * L * n], a[:2 * L * n], b), (a[:2 * L * n], b, a[:2 * L * n]), (a[n:n + 2 * L * n], a[:2 * L * n], b)):
        with pytest.raises(hx.HexlError):
            plan.multiply_relinearize(out, x, y, 1)
    plan.multiply_relinearize(a[2 * L * n:], a[:2 * L * n], b, 1)       # adjacent, not overlapping: accepted
    ctx.sync()
    plan.close()
