"""GPU: hexl_multiply_plain bit-exact against Python-integer products (tests/rns_model.py multiply_plain), every instance of every
launch; the first wrong word is named. The products of each (chain, n, operand family) are computed once for three components and all
K limbs; a launch with fewer components or limbs compares against the slice it covers."""
import numpy as np
import pytest

from ks_util import KsCase, extreme_words
from rns_model import assert_instances, chain, multiply_plain, negacyclic_product

pytestmark = pytest.mark.gpu

DISTINCT = 3                                                       # distinct instances; a larger batch cycles over them
KS = {"seal": 7, "strict": 4, "gen": 3}


def make_plan(hx, ctx, orc, n, qs):
    K = len(qs)
    case = KsCase(orc, n, 1, K, moduli=qs)
    return hx.KeySwitchPlan(ctx, n, 1, K, K, 2, case.moduli, case.modswitch)       # no keys: the multiply does not need them


def words(orc, family, n, q, salt, operand):
    return orc.splitmix(n, 7919 + 1000 * operand + salt, q) if family == "uniform" else extreme_words(n, q, salt)


_cache = {}


def operands(orc, kind, n, family):
    """(qs, ct[DISTINCT][3][K][n], pt[DISTINCT][K][n], prev[DISTINCT][3][K][n], shared[b] = ct[b] * pt[0], own[b] = ct[b] * pt[b]) -- the
    two operands of a call draw different patterns of the family (salts that differ by a non-multiple of the pattern count)"""
    key = (kind, n, family)
    if key not in _cache:
        K = KS[kind]
        qs = chain(orc, kind, K, n)
        ct = np.array([[[words(orc, family, n, qs[i], b * 5 + k * 3 + i, 0) for i in range(K)] for k in range(3)] for b in range(DISTINCT)])
        pt = np.array([[words(orc, family, n, qs[i], 4 + b * 7 + i, 1) for i in range(K)] for b in range(DISTINCT)])
        prev = np.array([[[orc.splitmix(n, 104729 + b * 64 + k * 16 + i, qs[i]) for i in range(K)] for k in range(3)] for b in range(DISTINCT)])
        shared = np.stack([multiply_plain(qs, n, ct[b], pt[0], 3, K) for b in range(DISTINCT)])
        own = np.stack([multiply_plain(qs, n, ct[b], pt[b], 3, K) for b in range(DISTINCT)])
        _cache[key] = (qs, ct, pt, prev, shared, own)
    return _cache[key]


def run(hx, ctx, dev, plan, ops, n, batch, ncomp, n_limbs, per_instance, mode, label):
    """mode: write | in_place | acc_uniform (out pre-filled with uniform words) | acc_top (with q_i - 1)"""
    import torch
    qs, ct, pt, prev, shared, own = ops
    qv = np.array(qs[:n_limbs], dtype=np.uint64).reshape(1, n_limbs, 1)
    inst = lambda a, b: np.ascontiguousarray(a[b % DISTINCT][:ncomp, :n_limbs])
    d_ct = hx.as_i64(np.stack([inst(ct, b) for b in range(batch)]).reshape(-1)).to(dev)
    pts = np.stack([pt[b % DISTINCT][:n_limbs] for b in range(batch if per_instance else 1)])
    d_pt = hx.as_i64(pts.reshape(-1)).to(dev)
    want = [inst(own if per_instance else shared, b) for b in range(DISTINCT)]
    if mode.startswith("acc"):
        before = [inst(prev, b) if mode == "acc_uniform" else np.broadcast_to(qv - np.uint64(1), (ncomp, n_limbs, n)) for b in range(DISTINCT)]
        d_out = hx.as_i64(np.stack([before[b % DISTINCT] for b in range(batch)]).reshape(-1)).to(dev)
        want = [(w + p) % qv for w, p in zip(want, before)]        # both below q_i < 2^52: the sum is exact in 64 bits
    else:
        d_out = d_ct if mode == "in_place" else torch.full_like(d_ct, -1)
    plan.multiply_plain(d_out, d_ct, d_pt, batch, ncomp, n_limbs, batch if per_instance else 1, accumulate=mode.startswith("acc"))
    ctx.sync()
    which = f"{label}: n={n} batch={batch} components={ncomp} n_limbs={n_limbs} pt_batch={'batch' if per_instance else 1} {mode}"
    assert_instances(hx.to_u64(d_out), want, batch, ("component", "limb", "coefficient"), (ncomp, n_limbs, n), which)
    assert np.array_equal(hx.to_u64(d_pt), pts.reshape(-1)), f"{which}: the plaintext was written"


MODES = ("write", "in_place", "acc_uniform", "acc_top")


@pytest.mark.parametrize("family", ["uniform", "extreme"])
@pytest.mark.parametrize("kind", ["seal", "strict"])
@pytest.mark.parametrize("n", [1024, 16384])
def test_multiply_plain_components_limbs_plaintexts_and_accumulate(hx, ctx, dev, orc, n, kind, family):
    ops = operands(orc, kind, n, family)
    K = KS[kind]
    plan = make_plan(hx, ctx, orc, n, ops[0])
    for ncomp in (1, 2, 3):
        for n_limbs in (1, K):
            for per_instance in (False, True):
                for mode in MODES:
                    run(hx, ctx, dev, plan, ops, n, 3, ncomp, n_limbs, per_instance, mode, f"{kind} {family}")
    plan.close()


@pytest.mark.parametrize("per_instance", [False, True])
def test_multiply_plain_batch_of_70(hx, ctx, dev, orc, per_instance):
    n, kind = 1024, "seal"
    for family in ("uniform", "extreme"):
        ops = operands(orc, kind, n, family)
        plan = make_plan(hx, ctx, orc, n, ops[0])
        for ncomp, n_limbs, mode in ((2, KS[kind], "write"), (3, KS[kind] - 1, "acc_uniform"), (2, 1, "in_place"), (1, KS[kind], "acc_top")):
            run(hx, ctx, dev, plan, ops, n, 70, ncomp, n_limbs, per_instance, mode, f"{kind} {family}")
        plan.close()


def test_multiply_plain_at_32768(hx, ctx, dev, orc):
    n, kind = 32768, "gen"
    ops = operands(orc, kind, n, "uniform")
    plan = make_plan(hx, ctx, orc, n, ops[0])
    for per_instance, mode in ((False, "write"), (True, "acc_uniform"), (True, "in_place"), (False, "acc_top")):
        run(hx, ctx, dev, plan, ops, n, 3, 2, KS[kind], per_instance, mode, kind)
    plan.close()


def test_multiply_plain_rejections(hx, ctx, dev, orc):
    import torch
    n, K, batch, ncomp = 4096, 4, 3, 2
    case = KsCase(orc, n, 2, K, seed=1)
    plan = hx.KeySwitchPlan(ctx, n, 2, K, K, 2, case.moduli, case.modswitch)
    per = ncomp * K * n
    buf = torch.zeros((2 * batch * per + batch * K * n + n,), dtype=torch.int64, device=dev)
    out, ct, pt = buf[:batch * per], buf[batch * per:2 * batch * per], buf[2 * batch * per:2 * batch * per + batch * K * n]
    for args, kw in (((out, ct, pt, batch, 0, K, 1), {}), ((out, ct, pt, batch, 4, K, 1), {}),            # 1 <= components <= 3
                     ((out, ct, pt, batch, ncomp, 0, 1), {}), ((out, ct, pt, batch, ncomp, K + 1, 1), {}),  # 1 <= n_limbs <= K
                     ((out, ct, pt, batch, ncomp, K, 2), {}), ((out, ct, pt, batch, ncomp, K, 0), {}),      # pt_batch is 1 or batch
                     ((ct, ct, pt, batch, ncomp, K, 1), {"accumulate": True}),                             # in place while accumulating
                     ((buf[n:n + batch * per], out, pt, batch, ncomp, K, 1), {}),                          # out partly over ct
                     ((out, buf[n:n + batch * per], pt, batch, ncomp, K, 1), {"accumulate": True}),
                     ((out, ct, out[:batch * K * n], batch, ncomp, K, batch), {}),                         # out over pt
                     ((out, ct, out[per - n:per - n + K * n], batch, ncomp, K, 1), {})):
        with pytest.raises(hx.HexlError):
            plan.multiply_plain(*args, **kw)
    plan.multiply_plain(out, ct, pt, batch, ncomp, K, batch)                                              # adjacent buffers: accepted
    plan.multiply_plain(ct, ct, pt, batch, ncomp, K, 1)                                                   # in place, written
    plan.multiply_plain(out, ct, ct[:K * n], batch, ncomp, K, 1, accumulate=True)                         # pt may lie inside ct
    plan.multiply_plain(out, ct, pt, 0, ncomp, K, 1)                                                      # nothing to do
    ctx.sync()
    plan.close()
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)                   # a plan on the integer kernels (moduli >= 2^52): out of scope
    plan = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    with pytest.raises(hx.HexlError):
        plan.multiply_plain(out, ct, pt, 1, 2, 2, 1)
    plan.close()


def test_multiply_plain_then_inverse_is_the_negacyclic_product(hx, ctx, dev, orc):
    """forward transforms of two coefficient polynomials, multiply_plain, inverse transform = a(X) b(X) mod (X^n + 1, q), the product
    computed by the schoolbook method in Python integers: ties the transforms' output order to the order multiply_plain pairs words in"""
    import torch
    n, K = 1024, 3
    qs = chain(orc, "gen", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    a, b = orc.splitmix(n, 11, qs[0]), orc.splitmix(n, 12, qs[0])
    a[:4], b[:4] = (qs[0] - 1, 0, 1, qs[0] - 1), (qs[0] - 1, qs[0] - 1, 0, 1)
    d = hx.as_i64(np.concatenate([a, b])).to(dev)                  # [2][1][n]
    d_out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    plan.rns_ntt_fwd(d, d, 2, 1)
    plan.multiply_plain(d_out, d[:n], d[n:], 1, 1, 1, 1)
    plan.rns_ntt_inv(d_out, d_out, 1, 1)
    ctx.sync()
    assert_instances(hx.to_u64(d_out), [negacyclic_product(a, b, qs[0])], 1, ("coefficient",), (n,), "multiply_plain -> rns_ntt_inv")
    plan.close()
