"""GPU: one CKKS level on the device at bridge-seal's chain (52, 30, 30, 40, 27, 27, 27) -- multiply_relinearize -> rescale ->
rotate -- bit-exact against the same composition of oracle calls (orc.dyadic + orc.keyswitch, the rescale model, the Galois
permutation + orc.keyswitch)."""
import numpy as np
import pytest

from ckks_model import Limbs, rescale, rotate
from ks_util import KsCase, extreme_ciphertext, seal_chain

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,nb", [(16384, 5), (4096, 70)])
def test_multiply_rescale_rotate(hx, ctx, dev, orc, n, nb):
    run_level(hx, ctx, dev, orc, n, nb, extreme=False)


def test_multiply_rescale_rotate_extreme_operands(hx, ctx, dev, orc):
    """the same level with every word of both operands and of both key sets at q - 1, beside q / 2, 0 or 1 (ks_util.extreme_words): the
    rescale then takes what the fused multiply made of them, the rotate what the rescale did"""
    run_level(hx, ctx, dev, orc, 4096, 5, extreme=True)


def run_level(hx, ctx, dev, orc, n, nb, extreme):
    import torch
    K = 7
    L = K - 1
    qs = seal_chain(orc, K, n)
    # level L: data limbs q_0 ... q_5, special q_6; after the rescale: q_0 ... q_4, special q_6
    relin = KsCase(orc, n, L, K, seed=21, moduli=qs, extreme_keys=extreme)
    galois = KsCase(orc, n, L - 1, K - 1, seed=22, moduli=qs[:L - 1] + qs[K - 1:], extreme_keys=extreme)
    p1 = hx.KeySwitchPlan(ctx, n, L, K, K, 2, relin.moduli, relin.modswitch)
    p1.set_keys(relin.keys)
    p2 = hx.KeySwitchPlan(ctx, n, L - 1, K - 1, K - 1, 2, galois.moduli, galois.modswitch)
    p2.set_keys(galois.keys)
    lm = Limbs(orc, n, qs)
    g = pow(5, 11, 2 * n)

    def operand(b, which):
        if extreme:
            return extreme_ciphertext(relin, b, 2, salt=4 * which)
        return np.concatenate([orc.splitmix(n, 500 + b * 131 + which * 17 + k * 5 + i, qs[i]) for k in range(2) for i in range(L)])

    distinct = 2
    A = [operand(b, 0) for b in range(distinct)]
    B = [operand(b, 1) for b in range(distinct)]
    d_a = hx.as_i64(np.concatenate([A[b % distinct] for b in range(nb)])).to(dev)
    d_b = hx.as_i64(np.concatenate([B[b % distinct] for b in range(nb)])).to(dev)
    d_m = torch.empty(nb * 2 * L * n, dtype=torch.int64, device=dev)
    d_r = torch.empty(nb * 2 * (L - 1) * n, dtype=torch.int64, device=dev)
    d_o = torch.full((nb * 2 * (L - 1) * n,), -1, dtype=torch.int64, device=dev)
    p1.multiply_relinearize(d_m, d_a, d_b, nb)
    p1.rescale(d_r, d_m, nb, L, 2)
    p2.rotate(d_o, d_r, nb, g)
    ctx.sync()
    out = hx.to_u64(d_o).reshape(nb, -1)
    for b in range(distinct):
        prod = orc.dyadic(A[b], B[b], n, relin.moduli[:L], exact=True)
        m = prod[:2 * L * n].copy()
        orc.keyswitch(m, prod[2 * L * n:].copy(), n, L, K, L + 1, relin.moduli, relin.keys, relin.modswitch)
        r = rescale(lm, m, 1, L, 2).reshape(-1)
        want = rotate(orc, galois, r, g)
        for c in range(b, nb, distinct):
            assert np.array_equal(out[c], want), f"instance {c}"
    p1.close()
    p2.close()
