"""GPU: hexl_ct_lincomb bit-exact against the Python-integer model (tests/lincomb_model.py), every instance of every launch; the first
wrong word is named. Ring sizes 1024 (one chunk per polynomial), 2048 (two) and one case at 16384; batch 3 of three distinct instances;
the chains strict / period3_top / period12 / seal at K = 5. The words of the terms and the plaintexts of each
(chain, n, family) are made once for eight terms, three components and K limbs; a launch takes the slice it covers. Limbs a term carries
beyond the output's (in_limbs > n_limbs) hold a sentinel that is no residue; an output buffer that is not a term is pre-filled with -1.
At the end one polynomial, x^2 - 3x + 0.5, is evaluated across a level without the host touching a limb."""
import itertools
import math

import numpy as np
import pytest

from ks_util import KsCase, extreme_words
from lincomb_model import ct_lincomb
from rns_model import assert_instances, chain, multiply_plain
from test_gpu_streams import Op, assert_every, closing, dev_pair, fill, first_then_warm, side_context  # noqa: F401  (closing, fill: fixtures)

pytestmark = pytest.mark.gpu

K, BATCH, MAX_TERMS = 5, 3, 8
SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)
KINDS = ["strict", "period3_top", "period12", "seal"]


def make_plan(hx, ctx, orc, n, qs):
    k = len(qs)
    case = KsCase(orc, n, 1, k, moduli=qs)
    return hx.KeySwitchPlan(ctx, n, 1, k, k, 2, case.moduli, case.modswitch)       # no keys: the linear combination does not need them


_pool = {}


def pool(orc, kind, n, family):
    """(qs, terms[8][BATCH][3][K][n], pts[BATCH][K][n]): operands that meet in one call draw different patterns of the family"""
    key = (kind, n, family)
    if key not in _pool:
        qs = chain(orc, kind, K, n)
        if family == "uniform":
            word = lambda salt, i: orc.splitmix(n, 3001 + salt, qs[i])
        else:
            word = lambda salt, i: extreme_words(n, qs[i], salt)
        terms = np.array([[[[word(t * 131 + b * 37 + k * 11 + i, i) for i in range(K)] for k in range(3)] for b in range(BATCH)]
                          for t in range(MAX_TERMS)])
        pts = np.array([[word(5000 + b * 7 + i, i) for i in range(K)] for b in range(BATCH)])
        _pool[key] = (qs, terms, pts)
    return _pool[key]


def make_weights(orc, qs, kind, n_terms, n_limbs):
    """[n_terms][n_limbs] residues, or None for the NULL argument (every weight 1)"""
    if kind == "null":
        return None
    if kind == "uniform":
        return [[int(orc.splitmix(1, 9001 + 17 * t + i, qs[i])[0]) for i in range(n_limbs)] for t in range(n_terms)]
    if kind == "top":
        return [[qs[i] - 1 for i in range(n_limbs)] for t in range(n_terms)]
    if kind == "half":                                             # beside q / 2, both sides
        return [[(qs[i] - 1) // 2 + ((t + i) & 1) for i in range(n_limbs)] for t in range(n_terms)]
    assert kind == "mixed", kind                                   # 1 among others: the path without the multiply next to the other
    return [[1 if (t + i) % 2 == 0 else qs[i] - 1 - t for i in range(n_limbs)] for t in range(n_terms)]


def mixed_limbs(n_terms, n_limbs):
    """n_limbs + 1, K and n_limbs in one call (capped at K); the last of several terms is at n_limbs, so that it can be the output"""
    cycle = [min(n_limbs + 1, K), K, n_limbs]
    il = [cycle[t % 3] for t in range(n_terms)]
    if n_terms > 1:
        il[-1] = n_limbs
    return il


def term_words(terms, t, ncomp, n_limbs, lt):
    """term t of every instance as the call takes it: [BATCH][ncomp][lt][n], the limbs beyond n_limbs hold the sentinel"""
    w = np.ascontiguousarray(terms[t][:, :ncomp, :lt]).copy()
    w[:, :, n_limbs:] = SENTINEL
    return w


def run(hx, ctx, dev, orc, plan, ops, n, ncomp, n_limbs, n_terms, wkind, in_limbs=None, addend="none", place="fresh", label=""):
    """one call and its checks. addend: none | pt1 | ptb | const | pt1+const | ptb+const; place: fresh | first | last (d_out is that term)"""
    import torch
    qs, terms, pts = ops
    il = [n_limbs] * n_terms if in_limbs is None else in_limbs
    weights = make_weights(orc, qs, wkind, n_terms, n_limbs)
    host = [term_words(terms, t, ncomp, n_limbs, il[t]) for t in range(n_terms)]
    d_terms = [hx.as_i64(h.reshape(-1)).to(dev) for h in host]
    per_instance = addend.startswith("ptb")
    pt = np.ascontiguousarray(pts[:BATCH if per_instance else 1, :n_limbs]) if addend.startswith("pt") else None
    d_pt = None if pt is None else hx.as_i64(pt.reshape(-1)).to(dev)
    const = [qs[i] - 1 - 3 * i for i in range(n_limbs)] if addend.endswith("const") else None
    want = [ct_lincomb(qs, n, [h[b] for h in host], ncomp, n_limbs, weights=weights, in_limbs=il,
                       pt=None if pt is None else pt[b if per_instance else 0], const=const) for b in range(BATCH)]
    which = (f"{label}: n={n} components={ncomp} n_limbs={n_limbs} terms={n_terms} weights={wkind} in_limbs={in_limbs} addend={addend} "
             f"out={place}")
    if place == "fresh":
        d_out = torch.full((BATCH * ncomp * n_limbs * n,), -1, dtype=torch.int64, device=dev)
    else:
        at = 0 if place == "first" else n_terms - 1
        assert il[at] == n_limbs, which
        d_out = d_terms[at]
    plan.ct_lincomb(d_out, d_terms, BATCH, ncomp, n_limbs, weights=weights, in_limbs=in_limbs, pt=d_pt,
                    pt_batch=BATCH if per_instance else 1, const=const)
    ctx.sync()
    assert_instances(hx.to_u64(d_out), want, BATCH, ("component", "limb", "coefficient"), (ncomp, n_limbs, n), which)
    for t in range(n_terms):
        if d_terms[t] is not d_out:
            assert np.array_equal(hx.to_u64(d_terms[t]), host[t].reshape(-1)), f"{which}: term {t} was written"
    if pt is not None:
        assert np.array_equal(hx.to_u64(d_pt), pt.reshape(-1)), f"{which}: the plaintext was written"
    return want


WEIGHTS = ["uniform", "null", "top", "half", "mixed"]
ADDENDS = ["none", "pt1", "ptb", "const", "pt1+const", "ptb+const"]


@pytest.mark.parametrize("kind", KINDS)
def test_ct_lincomb_components_limbs_terms_weights_and_addends(hx, ctx, dev, orc, kind):
    """n = 1024: every (components, n_limbs, n_terms) of {1, 2, 3} x {1, 3, K} x {1, 2, 3, 8}. The operand family, the weights, the addends,
    the mix of levels and the place of the output walk through their lists along the 36 shapes, shifted by one per chain: across the four
    chains every value of each meets every number of components, of limbs and of terms (mixed levels need n_limbs < K; a lone term or a
    term with more limbs cannot be the output)"""
    n = 1024
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    shift = KINDS.index(kind)
    for c, (ncomp, n_limbs, n_terms) in enumerate(itertools.product((1, 2, 3), (1, 3, K), (1, 2, 3, 8))):
        c += shift
        family = ("uniform", "extreme")[c % 2]
        mixed = n_limbs < K and (c // 3) % 2 == 0
        place = ("fresh", "first", "last")[c % 3]
        if mixed and place != "fresh":                             # the first term of a mixed call carries more limbs, a lone term too
            place = "fresh" if n_terms == 1 else "last"
        run(hx, ctx, dev, orc, plan, pool(orc, kind, n, family), n, ncomp, n_limbs, n_terms, WEIGHTS[c % 5],
            in_limbs=mixed_limbs(n_terms, n_limbs) if mixed else None, addend=ADDENDS[c % 6], place=place, label=f"{kind} {family}")
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_ct_lincomb_two_chunks_per_polynomial(hx, ctx, dev, orc, kind):
    """n = 2048: the chunk index inside a polynomial"""
    n = 2048
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    cases = [(2, K, 2, "uniform", None, "ptb+const", "fresh"), (3, 3, 8, "half", "mixed", "pt1", "last"), (1, 1, 3, "top", "mixed", "const", "fresh"),
             (2, 3, 1, "null", "mixed", "none", "fresh"), (2, K, 3, "mixed", None, "ptb", "first")]
    for c, (ncomp, n_limbs, n_terms, wkind, il, addend, place) in enumerate(cases):
        family = ("uniform", "extreme")[c % 2]
        run(hx, ctx, dev, orc, plan, pool(orc, kind, n, family), n, ncomp, n_limbs, n_terms, wkind,
            in_limbs=mixed_limbs(n_terms, n_limbs) if il else None, addend=addend, place=place, label=f"{kind} {family}")
    plan.close()


def test_ct_lincomb_at_16384(hx, ctx, dev, orc):
    """sixteen chunks per polynomial, mixed levels: the chunk and stride arithmetic at the ring size of the headline shape"""
    n, kind = 16384, "seal"
    plan = make_plan(hx, ctx, orc, n, pool(orc, kind, n, "uniform")[0])
    run(hx, ctx, dev, orc, plan, pool(orc, kind, n, "uniform"), n, 2, 3, 3, "uniform", in_limbs=[4, K, 3], addend="ptb+const", place="fresh", label=kind)
    plan.close()


@pytest.mark.parametrize("kind", ["strict", "seal"])
def test_ct_lincomb_eight_terms_all_extreme_one_sign(hx, ctx, dev, orc, kind):
    """the worst case the host replay runs (tests/cpp/lincomb_selftest.cpp): all eight terms hold the same extreme word everywhere and
    carry the same extreme weight, so all terms have one sign and every partial sum sits at its bound"""
    import torch
    n = 1024
    qs = chain(orc, kind, K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    edges = lambda q: {"top": q - 1, "lo": (q - 1) // 2, "hi": (q + 1) // 2, "one": 1}
    for xe, we in (("top", "top"), ("top", "lo"), ("top", "hi"), ("lo", "hi"), ("hi", "hi"), ("hi", "top"), ("top", "one")):
        one = np.array([[np.full(n, edges(qs[i])[xe], dtype=np.uint64) for i in range(K)]] * 2)          # [2][K][n]
        d_terms = [hx.as_i64(np.stack([one] * BATCH).reshape(-1)).to(dev) for _ in range(MAX_TERMS)]
        weights = [[edges(qs[i])[we] for i in range(K)]] * MAX_TERMS
        pt = np.array([np.full(n, qs[i] - 1, dtype=np.uint64) for i in range(K)])
        const = [qs[i] - 1 for i in range(K)]
        want = ct_lincomb(qs, n, [one] * MAX_TERMS, 2, K, weights=weights, pt=pt, const=const)
        d_out = torch.full((BATCH * 2 * K * n,), -1, dtype=torch.int64, device=dev)
        plan.ct_lincomb(d_out, d_terms, BATCH, 2, K, weights=weights, pt=hx.as_i64(pt.reshape(-1)).to(dev), pt_batch=1, const=const)
        ctx.sync()
        assert_instances(hx.to_u64(d_out), [want], BATCH, ("component", "limb", "coefficient"), (2, K, n), f"{kind}: words {xe}, weights {we}")
    plan.close()


def test_ct_lincomb_addends_leave_component_one_alone(hx, ctx, dev, orc):
    n, kind = 1024, "seal"
    ops = pool(orc, kind, n, "uniform")
    plan = make_plan(hx, ctx, orc, n, ops[0])
    bare = run(hx, ctx, dev, orc, plan, ops, n, 2, K, 2, "uniform", label="without addends")
    full = run(hx, ctx, dev, orc, plan, ops, n, 2, K, 2, "uniform", addend="ptb+const", label="with addends")
    for b in range(BATCH):                                         # `run` compared the device words with these
        assert np.array_equal(bare[b][1], full[b][1]) and not np.array_equal(bare[b][0], full[b][0])
    plan.close()


def test_ct_lincomb_accumulates_over_two_calls(hx, ctx, dev, orc):
    """out = a0 + w1 a1 (written), then out = out + w2 a2 - a3 with d_out as the first term, then as the last"""
    import torch
    n, kind, ncomp = 1024, "period3_top", 2
    qs, terms, _ = pool(orc, kind, n, "uniform")
    plan = make_plan(hx, ctx, orc, n, qs)
    a = [np.ascontiguousarray(terms[t][:, :ncomp]) for t in range(4)]
    d = [hx.as_i64(x.reshape(-1)).to(dev) for x in a]
    w = make_weights(orc, qs, "uniform", 2, K)
    minus = [q - 1 for q in qs]
    for order in ("first", "last"):
        d_out = torch.full((BATCH * ncomp * K * n,), -1, dtype=torch.int64, device=dev)
        plan.ct_lincomb(d_out, [d[0], d[1]], BATCH, ncomp, K, weights=[[1] * K, w[0]])
        if order == "first":
            plan.ct_lincomb(d_out, [d_out, d[2], d[3]], BATCH, ncomp, K, weights=[[1] * K, w[1], minus])
        else:
            plan.ct_lincomb(d_out, [d[2], d[3], d_out], BATCH, ncomp, K, weights=[w[1], minus, [1] * K])
        ctx.sync()
        want = [ct_lincomb(qs, n, [x[b] for x in a], ncomp, K, weights=[[1] * K, w[0], w[1], minus]) for b in range(BATCH)]
        assert_instances(hx.to_u64(d_out), want, BATCH, ("component", "limb", "coefficient"), (ncomp, K, n), f"accumulate, d_out {order}")
    plan.close()


def test_ct_lincomb_refusals_write_nothing(hx, ctx, dev, orc):
    import torch
    n, ncomp, n_limbs = 1024, 2, 3
    qs = chain(orc, "seal", K, n)
    plan = make_plan(hx, ctx, orc, n, qs)
    per = ncomp * n_limbs * n                                      # words of one output instance
    big = ncomp * K * n
    buf = torch.full((BATCH * per + n,), -1, dtype=torch.int64, device=dev)
    out = buf[:BATCH * per]
    a = torch.zeros(BATCH * big, dtype=torch.int64, device=dev)    # large enough for every in_limbs
    b = torch.zeros(BATCH * big, dtype=torch.int64, device=dev)
    pt = torch.zeros(BATCH * n_limbs * n, dtype=torch.int64, device=dev)
    ones = [[1] * n_limbs] * 2
    call = lambda *args, **kw: plan.ct_lincomb(*args, **kw)
    bad = [
        lambda: call(buf[n:n + BATCH * per], [out, a], BATCH, ncomp, n_limbs),                                # out partly over a term
        lambda: call(a[n:n + BATCH * per], [a, b], BATCH, ncomp, n_limbs),
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, pt=buf[n:n + n_limbs * n]),                          # out over the plaintext
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, pt=out[:BATCH * n_limbs * n], pt_batch=BATCH),
        lambda: call(a, [a, b], BATCH, ncomp, n_limbs, in_limbs=[n_limbs + 1, n_limbs]),                      # out == a term of another layout
        lambda: call(a, [b, a], BATCH, ncomp, n_limbs, in_limbs=[n_limbs, K]),
        lambda: call(out, [], BATCH, ncomp, n_limbs),                                                         # 1 <= n_terms <= 8
        lambda: call(out, [a] * 9, BATCH, ncomp, n_limbs),
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, in_limbs=[n_limbs - 1, n_limbs]),                    # n_limbs <= in_limbs[t] <= K
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, in_limbs=[n_limbs, K + 1]),
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, weights=[[1, qs[1], 1], [1] * n_limbs]),             # a weight equal to q_i
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, weights=ones, const=[0, 0, qs[2]]),                  # a constant equal to q_i
        lambda: call(out, [a, b], BATCH, 0, n_limbs),                                                         # 1 <= n_components <= 3
        lambda: call(out, [a, b], BATCH, 4, n_limbs),
        lambda: call(out, [a, b], BATCH, ncomp, 0),                                                           # 1 <= n_limbs <= K
        lambda: call(out, [a, b], BATCH, ncomp, K + 1),
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, pt=pt, pt_batch=2),                                  # pt_batch is 1 or batch
        lambda: call(out, [a, b], BATCH, ncomp, n_limbs, pt=pt, pt_batch=0),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(hx.HexlError, match="status -1"):
            f()
        ctx.sync()
        assert bool((buf == -1).all()), f"refusal {k} wrote to the output"
        assert not bool(a.any()) and not bool(b.any()), f"refusal {k} wrote to a term"
    case = KsCase(orc, n, 2, 3, seed=1, bits=55)                   # a plan on the integer kernels (moduli >= 2^52): out of scope
    integer = hx.KeySwitchPlan(ctx, n, 2, 3, 3, 2, case.moduli, case.modswitch)
    assert integer.tiers()[0][0] == -1
    with pytest.raises(hx.HexlError, match="status -1"):
        integer.ct_lincomb(out, [a, b], BATCH, ncomp, 2)
    ctx.sync()
    assert bool((buf == -1).all())
    integer.close()
    # accepted: adjacent buffers, a plaintext inside a term, a term twice, pt_batch ignored without a plaintext, nothing to do
    plan.ct_lincomb(out, [a, b], BATCH, ncomp, n_limbs, pt=a[:n_limbs * n])
    plan.ct_lincomb(out, [a, a], BATCH, ncomp, n_limbs, in_limbs=[K, n_limbs])
    plan.ct_lincomb(out, [a, b], BATCH, ncomp, n_limbs, pt_batch=7)
    plan.ct_lincomb(out, [a, b], 0, ncomp, n_limbs)
    ctx.sync()
    assert not bool(out.any()) and bool((buf[BATCH * per:] == -1).all())                                   # sums of zeros; nothing behind them
    plan.close()


def test_ct_lincomb_is_multiply_plain_by_a_constant_word_plaintext(hx, ctx, dev, orc):
    """the route that existed before: a plaintext whose words are all w_i through hexl_multiply_plain, the second term accumulated"""
    import torch
    n, kind, ncomp = 1024, "seal", 2
    qs, terms, _ = pool(orc, kind, n, "extreme")
    plan = make_plan(hx, ctx, orc, n, qs)
    w = make_weights(orc, qs, "uniform", 2, K)
    a = [hx.as_i64(np.ascontiguousarray(terms[t][:, :ncomp]).reshape(-1)).to(dev) for t in range(2)]
    d_pts = [hx.as_i64(np.array([np.full(n, w[t][i], dtype=np.uint64) for i in range(K)]).reshape(-1)).to(dev) for t in range(2)]
    via_pt = torch.full_like(a[0], -1)
    plan.multiply_plain(via_pt, a[0], d_pts[0], BATCH, ncomp, K, 1)
    one = torch.full_like(a[0], -1)
    plan.ct_lincomb(one, [a[0]], BATCH, ncomp, K, weights=[w[0]])
    ctx.sync()
    assert torch.equal(via_pt, one), "T = 1"
    assert np.array_equal(hx.to_u64(one).reshape(BATCH, ncomp, K, n)[1], multiply_plain(qs, n, terms[0][1][:ncomp], hx.to_u64(d_pts[0]), ncomp, K))
    plan.multiply_plain(via_pt, a[1], d_pts[1], BATCH, ncomp, K, 1, accumulate=True)
    plan.ct_lincomb(one, a, BATCH, ncomp, K, weights=w)
    ctx.sync()
    assert torch.equal(via_pt, one), "T = 2 against write + accumulate"
    plan.close()



def test_ct_lincomb_is_ordered_on_a_caller_stream(hx, dev, orc, fill, closing):
    """behind a filler on a side stream set by hexl_ctx_set_stream: the terms and the plaintext are poison until copies queued on that
    stream replace them, the output is cloned on that stream, and the stream is the only thing waited for (test_gpu_streams.py, part A)"""
    n, kind, ncomp, n_limbs = 1024, "seal", 2, 3
    side, s = side_context(hx, closing)
    qs, terms, pts = pool(orc, kind, n, "uniform")
    plan = make_plan(hx, side, orc, n, qs)
    closing.append(plan)
    il = [n_limbs, K, n_limbs]
    weights = make_weights(orc, qs, "mixed", 3, n_limbs)
    const = [q - 2 for q in qs[:n_limbs]]
    host = [np.ascontiguousarray(terms[t][:, :ncomp, :il[t]]) for t in range(3)]
    pairs = [dev_pair(hx, dev, list(h), BATCH) for h in host]
    pt = np.ascontiguousarray(pts[:, :n_limbs])
    d_pt, real_pt = dev_pair(hx, dev, list(pt), BATCH)
    import torch
    out = torch.empty(BATCH * ncomp * n_limbs * n, dtype=torch.int64, device=dev)
    want = [ct_lincomb(qs, n, [h[b] for h in host], ncomp, n_limbs, weights=weights, in_limbs=il, pt=pt[b], const=const) for b in range(BATCH)]
    label = "hexl_ct_lincomb on a side stream"
    op = Op(label, pairs + [(d_pt, real_pt)], [out], [out],
            lambda: plan.ct_lincomb(out, [p[0] for p in pairs], BATCH, ncomp, n_limbs, weights=weights, in_limbs=il, pt=d_pt, pt_batch=BATCH,
                                    const=const),
            lambda c: assert_every(hx, c[0], want, BATCH, ("component", "limb", "coefficient"), (ncomp, n_limbs, n), label))
    first_then_warm(op, s, fill)


def test_polynomial_across_a_level_on_the_device(hx, ctx, dev, orc):
    """x^2 - 3x + 0.5 on slots |x| <= 1, n = 1024, four 40-bit primes (L = 3 and the special prime), scale D = q_2, all on the device:
    encode x at three limbs -> the trivial ciphertext (pt, 0) -> multiply_relinearize with itself -> rescale to two limbs (scale D^2 / q_2
    = D again) -> ONE ct_lincomb of (x^2 at two limbs, x at in_limbs = 3) with weights (1, q_i - 3) and the constant rint(0.5 D) -> decode
    component 0 at two limbs.

    The tolerance, derived before any run. Units: one integer step of a coefficient; a coefficient error e_j reaches a slot as
    sum_j e_j zeta^(j 5^k), so errors of at most h per coefficient reach a slot with at most n h. F = 16 log2(n) 2^-53 is the FFT bound
    of DESIGN.md 4.6.4 (2-norm of the error over 2-norm of the data).
      encode      the real coefficients c of D x have ||c||_2 = ||slots||_2 / sqrt(n) <= D; the device's are off by at most F ||c||_2 in the
                  2-norm, so by at most sqrt(n) F D in a slot, and are then rounded, 1/2 each: the plaintext's slots are D x + eps with
                  |eps| <= E = n/2 + sqrt(n) F D
      square      (D x + eps)^2 = D^2 x^2 + 2 D x eps + eps^2: after the division by q_2 = D the error is 2 |x| |eps| + eps^2 / D
                  <= 2 E + E^2 / D -- the squaring doubles the encode error for |x| <= 1
      keyswitch   of the zero component: its rounding, at most 1/2 per coefficient -> n/2 (generous: it precedes the division by q_2)
      rescale     its rounding, 1/2 per coefficient -> n/2
      -3 x        three times the encode error: 3 E
      constant    rint(0.5 D) is off by at most 1/2, in coefficient 0 alone -> 1/2
    Sum: 5 E + E^2 / D + n + 1/2 steps, divided by the scale D. Decode converts exactly (every coefficient is far below 2^53) and its
    FFT adds at most F ||result||_2 to any slot; the numpy reference itself is good to a few ulp of 4.5 (2^-50 allowed).
    With n = 1024 and D ~ 2^40 that is (3585 + 5 * 0.62 + ...) / D + 1.8e-12 ~ 3.3e-9."""
    import torch
    n, Kc, L, count = 1024, 4, 3, 2
    qs = [int(q) for q in orc.primes(Kc, 40, n)]
    case = KsCase(orc, n, L, Kc, seed=5, moduli=qs)
    plan = hx.KeySwitchPlan(ctx, n, L, Kc, Kc, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    D = float(qs[2])
    assert int(D) == qs[2]
    rng = np.random.default_rng(11)
    x = np.sqrt(rng.random((count, n // 2))) * np.exp(2j * np.pi * rng.random((count, n // 2)))         # uniform in the unit disc
    x[:, 0], x[:, 1], x[:, 2] = 1.0, -1.0, 1j
    assert np.abs(x).max() <= 1.0 + 1e-15
    d_x = torch.from_numpy(np.ascontiguousarray(np.stack([x.real, x.imag], axis=-1))).to(dev)               # [count][n/2][2]
    ct = torch.zeros(count, 2, L, n, dtype=torch.int64, device=dev)                                         # (pt, 0)
    enc = torch.empty(count, L, n, dtype=torch.int64, device=dev)
    plan.ckks_encode(enc, d_x, count, L, D)
    ct[:, 0] = enc
    sq = torch.full((count * 2 * L * n,), -1, dtype=torch.int64, device=dev)
    plan.multiply_relinearize(sq, ct, ct, count)
    sq2 = torch.full((count * 2 * 2 * n,), -1, dtype=torch.int64, device=dev)
    plan.rescale(sq2, sq, count, L, 2)
    res = torch.full((count, 2, 2, n), -1, dtype=torch.int64, device=dev)
    half = int(np.rint(0.5 * D))
    plan.ct_lincomb(res, [sq2, ct], count, 2, 2, weights=[[1, 1], [qs[0] - 3, qs[1] - 3]], in_limbs=[2, L], const=[half % qs[0], half % qs[1]])
    d_z = torch.full((count, n // 2, 2), float("nan"), dtype=torch.float64, device=dev)
    for b in range(count):
        plan.ckks_decode(d_z[b], res[b, 0], 1, 2, D)
    ctx.sync()
    assert plan.range_check()
    z = d_z.cpu().numpy()
    got = z[..., 0] + 1j * z[..., 1]
    want = x * x - 3 * x + 0.5
    F = 16 * math.log2(n) * 2.0 ** -53
    E = n / 2 + math.sqrt(n) * F * D
    for b in range(count):
        tol = (5 * E + E * E / D + n + 0.5) / D + F * float(np.linalg.norm(want[b])) + 2.0 ** -50
        err = float(np.abs(got[b] - want[b]).max())
        print(f"[ct_lincomb] x^2 - 3x + 0.5 across a level, instance {b}: max |error| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, f"instance {b}: {err:.3e} > {tol:.3e}"
    plan.close()
