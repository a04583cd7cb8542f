"""GPU: hexl_ct_tensor_sum bit-exact against the Python-integer model (tests/tensor_model.py), every instance of every launch; the first
wrong word is named. Ring sizes 1024 (one piece per polynomial), 2048 (two) and one case at 16384; batch 3 of three distinct instances;
the chains strict / period3_top / period12 / seal at K = 5; 1, 2, 3 and 8 terms (both parities of the kernel's two register slots and the
full argument table). The words of the operands of each (chain, n, family) are made once for eight terms and K limbs; a launch takes the
slice it covers. Limbs an operand carries beyond the output's (in_limbs > n_limbs) hold a sentinel that is no residue; the output is
pre-filled with -1; the operands are compared with their host copies after the call. At the end the algebraic identity
(a0 + a1 s)(b0 + b1 s) = d0 + d1 s + d2 s^2 is checked on the device, word for word, through hexl_rlwe_decrypt."""
import itertools

import numpy as np
import pytest

from ks_util import KsCase, extreme_words
from rns_model import assert_instances, chain
from tensor_model import ct_tensor_sum
from test_gpu_streams import Op, assert_every, closing, dev_pair, fill, first_then_warm, side_context  # noqa: F401  (closing, fill: fixtures)

pytestmark = pytest.mark.gpu

K, BATCH, MAX_TERMS = 5, 3, 8
SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)
KINDS = ["strict", "period3_top", "period12", "seal"]
NAMES = ("component", "limb", "coefficient")


def make_plan(hx, ctx, orc, n, qs):
    k = len(qs)
    case = KsCase(orc, n, 1, k, moduli=qs)
    return hx.KeySwitchPlan(ctx, n, 1, k, k, 2, case.moduli, case.modswitch)       # no keys: the tensor sum does not need them


_pool = {}


def pool(orc, kind, n, family):
    """(qs, a[8][BATCH][2][K][n], b[8][BATCH][2][K][n]): operands that meet in one call draw different patterns of the family"""
    key = (kind, n, family)
    if key not in _pool:
        qs = chain(orc, kind, K, n)
        if family == "uniform":
            word = lambda salt, i: orc.splitmix(n, 7001 + salt, qs[i])
        else:
            word = lambda salt, i: extreme_words(n, qs[i], salt)
        make = lambda side: np.array([[[[word(side * 5000 + t * 131 + b * 37 + k * 11 + i, i) for i in range(K)] for k in range(2)]
                                       for b in range(BATCH)] for t in range(MAX_TERMS)])
        _pool[key] = (qs, make(0), make(1))
    return _pool[key]


def mixed_limbs(n_terms, n_limbs):
    """[n_terms][2]: n_limbs + 1, K and n_limbs in one call (capped at K), a_t and b_t of one term at different counts"""
    cycle = [min(n_limbs + 1, K), K, n_limbs]
    return [[cycle[t % 3], cycle[(t + 1) % 3]] for t in range(n_terms)]


def operand_words(side, t, n_limbs, lt):
    """operand t of every instance as the call takes it: [BATCH][2][lt][n], the limbs beyond n_limbs hold the sentinel"""
    w = np.ascontiguousarray(side[t][:, :, :lt]).copy()
    w[:, :, n_limbs:] = SENTINEL
    return w


def run(hx, ctx, dev, plan, ops, n, n_limbs, n_terms, in_limbs=None, squares=(), label=""):
    """one call and its checks; squares: the terms whose b is the very buffer of a"""
    import torch
    qs, A, B = ops
    il = [[n_limbs, n_limbs]] * n_terms if in_limbs is None else [list(p) for p in in_limbs]
    for t in squares:
        il[t][1] = il[t][0]
    host_a = [operand_words(A, t, n_limbs, il[t][0]) for t in range(n_terms)]
    host_b = [host_a[t] if t in squares else operand_words(B, t, n_limbs, il[t][1]) for t in range(n_terms)]
    d_a = [hx.as_i64(h.reshape(-1)).to(dev) for h in host_a]
    d_b = [d_a[t] if t in squares else hx.as_i64(host_b[t].reshape(-1)).to(dev) for t in range(n_terms)]
    want = [ct_tensor_sum(qs, n, [h[b] for h in host_a], [h[b] for h in host_b], n_limbs, il) for b in range(BATCH)]
    which = f"{label}: n={n} n_limbs={n_limbs} terms={n_terms} in_limbs={None if in_limbs is None else il} squares={list(squares)}"
    d_out = torch.full((BATCH * 3 * n_limbs * n,), -1, dtype=torch.int64, device=dev)
    plan.ct_tensor_sum(d_out, d_a, d_b, BATCH, n_limbs, in_limbs=None if in_limbs is None else il)
    ctx.sync()
    assert_instances(hx.to_u64(d_out), want, BATCH, NAMES, (3, n_limbs, n), which)
    for t in range(n_terms):
        assert np.array_equal(hx.to_u64(d_a[t]), host_a[t].reshape(-1)), f"{which}: a_{t} was written"
        assert np.array_equal(hx.to_u64(d_b[t]), host_b[t].reshape(-1)), f"{which}: b_{t} was written"
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_ct_tensor_sum_limbs_terms_families_and_levels(hx, ctx, dev, orc, kind):
    """n = 1024: every (n_limbs, n_terms) of {1, 3, K} x {1, 2, 3, 8}. The operand family, the mix of levels and a square term walk along
    the 12 shapes, shifted by one per chain: across the four chains every value of each meets every number of limbs and of terms
    (mixed levels need n_limbs < K)"""
    n = 1024
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    shift = KINDS.index(kind)
    for c, (n_limbs, n_terms) in enumerate(itertools.product((1, 3, K), (1, 2, 3, 8))):
        c += shift
        family = ("uniform", "extreme")[c % 2]
        mixed = n_limbs < K and (c // 2) % 2 == 0
        squares = (n_terms - 1,) if c % 4 == 3 else ()
        run(hx, ctx, dev, plan, pool(orc, kind, n, family), n, n_limbs, n_terms, in_limbs=mixed_limbs(n_terms, n_limbs) if mixed else None,
            squares=squares, label=f"{kind} {family}")
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_ct_tensor_sum_two_pieces_per_polynomial(hx, ctx, dev, orc, kind):
    """n = 2048: the piece index inside a polynomial"""
    n = 2048
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    for c, (n_limbs, n_terms, mixed) in enumerate([(K, 2, False), (3, 8, True), (1, 3, True), (3, 1, True)]):
        family = ("uniform", "extreme")[c % 2]
        run(hx, ctx, dev, plan, pool(orc, kind, n, family), n, n_limbs, n_terms, in_limbs=mixed_limbs(n_terms, n_limbs) if mixed else None,
            label=f"{kind} {family}")
    plan.close()


def test_ct_tensor_sum_at_16384(hx, ctx, dev, orc):
    """sixteen pieces per polynomial, mixed levels: the piece and stride arithmetic at the ring size of the headline shape"""
    n, kind = 16384, "seal"
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    run(hx, ctx, dev, plan, pool(orc, kind, n, "uniform"), n, 3, 3, in_limbs=[[4, K], [K, 3], [3, 4]], label=kind)
    plan.close()


def test_ct_tensor_sum_four_to_seven_terms(hx, ctx, dev, orc):
    """the kernel is built once per term count: the four counts the matrix above leaves out"""
    n, kind = 1024, "period3_top"
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    for n_terms in (4, 5, 6, 7):
        family = ("uniform", "extreme")[n_terms % 2]
        run(hx, ctx, dev, plan, pool(orc, kind, n, family), n, 3, n_terms, in_limbs=mixed_limbs(n_terms, 3) if n_terms & 2 else None,
            label=f"{kind} {family}")
    plan.close()


def test_ct_tensor_sum_squares(hx, ctx, dev, orc):
    """d_as[t] == d_bs[t]: every term a square, and one square among products"""
    n, kind = 1024, "seal"
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    run(hx, ctx, dev, plan, pool(orc, kind, n, "extreme"), n, K, 2, squares=(0, 1), label="all squares")
    run(hx, ctx, dev, plan, pool(orc, kind, n, "uniform"), n, 3, 3, in_limbs=mixed_limbs(3, 3), squares=(1,), label="one square")
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_ct_tensor_sum_eight_terms_all_extreme_one_sign(hx, ctx, dev, orc, kind):
    """the worst case the host replay runs (tests/cpp/tensor_selftest.cpp): all eight terms hold the same extreme words everywhere, so the
    products of a component have one sign and every partial sum sits at its bound"""
    import torch
    n = 1024
    qs = chain(orc, kind, K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    edges = lambda q: {"top": q - 1, "lo": (q - 1) // 2, "hi": (q + 1) // 2, "one": 1}
    const = lambda e0, e1: np.array([[np.full(n, edges(qs[i])[e], dtype=np.uint64) for i in range(K)] for e in (e0, e1)])   # [2][K][n]
    for ea, eb in ((("top", "top"), ("top", "top")), (("top", "lo"), ("hi", "top")), (("hi", "hi"), ("hi", "hi")), (("lo", "lo"), ("hi", "hi")),
                   (("top", "one"), ("lo", "top"))):
        a, b = const(*ea), const(*eb)
        d_a = [hx.as_i64(np.stack([a] * BATCH).reshape(-1)).to(dev) for _ in range(MAX_TERMS)]
        d_b = [hx.as_i64(np.stack([b] * BATCH).reshape(-1)).to(dev) for _ in range(MAX_TERMS)]
        want = ct_tensor_sum(qs, n, [a] * MAX_TERMS, [b] * MAX_TERMS, K)
        d_out = torch.full((BATCH * 3 * K * n,), -1, dtype=torch.int64, device=dev)
        plan.ct_tensor_sum(d_out, d_a, d_b, BATCH, K)
        ctx.sync()
        assert_instances(hx.to_u64(d_out), [want], BATCH, NAMES, (3, K, n), f"{kind}: a = {ea}, b = {eb}")
    plan.close()


def test_ct_tensor_sum_refusals_write_nothing(hx, ctx, dev, orc):
    import torch
    n, n_limbs = 1024, 3
    qs = chain(orc, "seal", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    per = 3 * n_limbs * n                                          # words of one output instance
    big = 2 * K * n
    buf = torch.full((BATCH * per + n,), -1, dtype=torch.int64, device=dev)
    out = buf[:BATCH * per]
    a = torch.zeros(BATCH * big + n, dtype=torch.int64, device=dev)    # large enough for every in_limbs
    b = torch.zeros(BATCH * big, dtype=torch.int64, device=dev)
    call = lambda *args, **kw: plan.ct_tensor_sum(*args, **kw)
    bad = [
        lambda: call(buf[n:n + BATCH * per], [out[:BATCH * 2 * n_limbs * n], a], [b, b], BATCH, n_limbs),     # out partly over an a
        lambda: call(a[n:n + BATCH * per], [b, b], [b, a], BATCH, n_limbs),                                   # ... over a b
        lambda: call(a[:BATCH * per], [a], [b], BATCH, n_limbs),                                              # no in-place form
        lambda: call(a[:BATCH * per], [b], [a], BATCH, n_limbs, in_limbs=[[n_limbs, K]]),
        lambda: call(out, [], [], BATCH, n_limbs),                                                            # 1 <= n_terms <= 8
        lambda: call(out, [a] * 9, [b] * 9, BATCH, n_limbs),
        lambda: call(out, [a, b], [b, a], BATCH, n_limbs, in_limbs=[[n_limbs - 1, n_limbs], [n_limbs, n_limbs]]),   # n_limbs <= in_limbs <= K
        lambda: call(out, [a, b], [b, a], BATCH, n_limbs, in_limbs=[[n_limbs, n_limbs], [n_limbs, K + 1]]),
        lambda: call(out, [a], [b], BATCH, 0),                                                                # 1 <= n_limbs <= K
        lambda: call(out, [a], [b], BATCH, K + 1),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(hx.HexlError, match="status -1"):
            f()
        ctx.sync()
        assert bool((buf == -1).all()), f"refusal {k} wrote to the output"
        assert not bool(a.any()) and not bool(b.any()), f"refusal {k} wrote to an operand"
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)                   # a plan on the integer kernels (moduli >= 2^52): out of scope
    integer = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    assert integer.tiers()[0][0] == -1
    with pytest.raises(hx.HexlError, match="status -1"):
        integer.ct_tensor_sum(out, [a], [b], BATCH, 2)
    ctx.sync()
    assert bool((buf == -1).all())
    integer.close()
    # accepted: adjacent buffers, operands that overlap each other, an operand twice, nothing to do
    plan.ct_tensor_sum(out, [a, a[n:]], [b, a], BATCH, n_limbs, in_limbs=[[K, K], [n_limbs, K]])
    plan.ct_tensor_sum(out, [a], [b], 0, n_limbs)
    ctx.sync()
    assert not bool(out.any()) and bool((buf[BATCH * per:] == -1).all())                                   # sums of zeros; nothing behind them
    plan.close()


def test_ct_tensor_sum_is_ordered_on_a_caller_stream(hx, dev, orc, fill, closing):
    """behind a filler on a side stream set by hexl_ctx_set_stream: the operands are poison until copies queued on that stream replace
    them, the output is cloned on that stream, and the stream is the only thing waited for (test_gpu_streams.py, part A)"""
    import torch
    n, kind, n_limbs, n_terms = 1024, "seal", 3, 3
    side, s = side_context(hx, closing)
    qs, A, B = pool(orc, kind, n, "uniform")
    plan = make_plan(hx, side, orc, n, qs)
    closing.append(plan)
    il = [[n_limbs, K], [K, n_limbs], [n_limbs, n_limbs]]
    host_a = [np.ascontiguousarray(A[t][:, :, :il[t][0]]) for t in range(n_terms)]
    host_b = [np.ascontiguousarray(B[t][:, :, :il[t][1]]) for t in range(n_terms)]
    pa = [dev_pair(hx, dev, list(h), BATCH) for h in host_a]
    pb = [dev_pair(hx, dev, list(h), BATCH) for h in host_b]
    out = torch.empty(BATCH * 3 * n_limbs * n, dtype=torch.int64, device=dev)
    want = [ct_tensor_sum(qs, n, [h[b] for h in host_a], [h[b] for h in host_b], n_limbs, il) for b in range(BATCH)]
    label = "hexl_ct_tensor_sum on a side stream"
    op = Op(label, pa + pb, [out], [out],
            lambda: plan.ct_tensor_sum(out, [p[0] for p in pa], [p[0] for p in pb], BATCH, n_limbs, in_limbs=il),
            lambda c: assert_every(hx, c[0], want, BATCH, NAMES, (3, n_limbs, n), label))
    first_then_warm(op, s, fill)


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_tensor_sum_decrypts_to_the_sum_of_the_products_of_the_decryptions(hx, ctx, dev, orc, kind):
    """no tolerance: (a0 + a1 s)(b0 + b1 s) = d0 + d1 s + d2 s^2 exactly, for arbitrary operand words, so with a TERNARY secret from
    hexl_sample hexl_rlwe_decrypt(tensor_sum(a, b), n_components = 3) equals sum_t hexl_multiply_plain(dec(a_t), dec(b_t)) modulo q_i,
    word for word. Everything stays on the device."""
    import torch
    n, n_limbs = 1024, 3
    for family, n_terms in (("uniform", 4), ("extreme", 8)):
        qs, A, B = pool(orc, kind, n, family)
        plan = make_plan(hx, ctx, orc, n, qs)
        s = torch.full((K * n,), -1, dtype=torch.int64, device=dev)
        plan.sample(s, hx.SAMPLE_TERNARY, 1, K, seed=bytes(range(32)), stream=5)
        il = mixed_limbs(n_terms, n_limbs)
        d_a = [hx.as_i64(operand_words(A, t, n_limbs, il[t][0]).reshape(-1)).to(dev) for t in range(n_terms)]
        d_b = [hx.as_i64(operand_words(B, t, n_limbs, il[t][1]).reshape(-1)).to(dev) for t in range(n_terms)]
        ct3 = torch.full((BATCH * 3 * n_limbs * n,), -1, dtype=torch.int64, device=dev)
        plan.ct_tensor_sum(ct3, d_a, d_b, BATCH, n_limbs, in_limbs=il)
        lhs = torch.full((BATCH * n_limbs * n,), -1, dtype=torch.int64, device=dev)
        plan.rlwe_decrypt(lhs, ct3, s, BATCH, 3, n_limbs)
        rhs = torch.full_like(lhs, -1)
        da, db, level = torch.empty_like(lhs), torch.empty_like(lhs), torch.empty(BATCH * 2 * n_limbs * n, dtype=torch.int64, device=dev)
        for t in range(n_terms):
            for src, lt, dst in ((d_a[t], il[t][0], da), (d_b[t], il[t][1], db)):
                plan.ct_lincomb(level, [src], BATCH, 2, n_limbs, in_limbs=[lt])                             # the level drop
                plan.rlwe_decrypt(dst, level, s, BATCH, 2, n_limbs)
            plan.multiply_plain(rhs, da, db, BATCH, 1, n_limbs, BATCH, accumulate=t > 0)
        ctx.sync()
        assert torch.equal(lhs, rhs), f"{kind} {family}: the decrypted tensor sum is not the sum of the products of the decryptions"
        assert bool((lhs.view(BATCH, n_limbs, n) < torch.tensor(qs[:n_limbs], device=dev).view(1, n_limbs, 1)).all()) and bool((lhs >= 0).all())
        plan.close()
