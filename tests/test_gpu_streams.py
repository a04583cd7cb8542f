"""GPU: the device-pointer entry points on caller streams, bit-exact against the oracle.

Every other GPU test runs on the legacy default stream, which every blocking stream serialises against: a launch, memset or copy that
escaped to the wrong stream would still give right answers there. Here a context is bound to a NON-BLOCKING stream (a torch side
stream, or the context's own) and the only ordering is the stream's:

A  every entry point behind a filler on a side stream: the input is poison until a copy queued on that stream replaces it, the output
   is cloned on that stream, and the stream is the only thing waited for. A kernel on another stream reads poison; one that finishes
   after the clone leaves stale words in the clone. The warm call must return while the filler is still pending.
B  the context's own stream (Context(0, use_torch_stream=False)), ctx.sync() as the only wait, then the round trip
   set_stream(side) -> use_own_stream().
C  a stream switch with work in flight: the context and its plans keep ONE set of scratch buffers (derived NTT tables, keyswitch /
   rescale / rotate scratch), so the second stream has to run behind the first (include/hexl_mi355x.h, hexl_ctx_set_stream).
D  the legacy default stream as an explicit case, null handles, two contexts on two streams.

Expected values come from the oracle (orc, KsCase, rns_model, ckks_model) or from composing oracle results, as in the per-op tests."""
import time

import numpy as np
import pytest

from ckks_model import Limbs, apply_galois, first_mismatch, rescale, rescale_input, rotate
from ks_util import KsCase, primes_below
from rns_model import chain, multiply_plain, ntt_input, rns_ntt

pytestmark = pytest.mark.gpu

# The filler of part A: FILL_REPS in-place adds on a tensor of FILL_WORDS 64-bit words, queued in front of the input copy.
# Measured on an MI355X (a shared host, all of this file in one process, two runs): the filler takes 6.1-6.3 ms on the device. From the
# filler's first launch to the return of the warm entry point the host took 69-138 us (slowest: the integer two-lane keyswitch, 138-140
# us; rotate over two slices 116-205 us), and 204-211 us in the first test of the process: the filler is 30 times the slowest.
FILL_WORDS = 1 << 29
FILL_REPS = 4
# C1: polynomials of the first launch (n = 4096). Measured: the launch takes 0.96-1.04 ms on the device, the second call (set_stream +
# hexl_ntt_fwd / _inv of 8 polynomials) is enqueued in 15-16 us. At the 6000 polynomials of the per-op tests it would take 0.1 ms.
C1_BATCH = 60000


def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def fill():
    """the filler: plain adds on a large tensor, nothing that can fault"""
    torch = torch_()
    buf = torch.zeros(FILL_WORDS, dtype=torch.int64, device="cuda:0")

    def run():
        for _ in range(FILL_REPS):
            buf.add_(1)
    yield run
    del buf
    torch.cuda.empty_cache()


@pytest.fixture
def closing():
    """contexts and plans of one test, closed in reverse order whatever happens (after everything queued has finished)"""
    made = []
    try:
        yield made
    finally:
        torch_().cuda.synchronize()
        for obj in reversed(made):
            obj.close()


def side_context(hx, closing, stream=None):
    """a context of this test's own, bound to a new torch side stream (non-blocking)"""
    ctx = hx.Context(0)
    closing.append(ctx)
    s = stream or torch_().cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    return ctx, s


def make_plan(hx, ctx, closing, case, keys=True):
    plan = hx.KeySwitchPlan(ctx, case.n, case.L, case.K, case.K, 2, case.moduli, case.modswitch)
    closing.append(plan)
    if keys:
        plan.set_keys(case.keys)
    return plan


def chunk_of(plan):
    """instances per scratch chunk of the keyswitch = per slice of the rotate, read off hexl_ks_scratch_bytes"""
    chunk = plan.scratch_bytes(1 << 24) // plan.scratch_bytes(1)
    assert chunk >= 2 and plan.scratch_bytes(chunk) == plan.scratch_bytes(chunk + 1) > plan.scratch_bytes(chunk - 1)
    return chunk


def assert_every(hx, got, want, count, names, shape, label):
    """got: device tensor of `count` instances, instance c against want[c % len(want)] (numpy words), compared on the device; the first
    wrong instance and its first wrong word are named"""
    torch = torch_()
    w = hx.as_i64(np.stack([np.asarray(v, dtype=np.uint64).reshape(-1) for v in want])).to(got.device)
    bad = (got.view(count, -1) != w[torch.arange(count, device=got.device) % len(want)]).any(dim=1)
    if bool(bad.any()):
        c = int(torch.nonzero(bad)[0])
        where = first_mismatch(hx.to_u64(got.view(count, -1)[c]), np.asarray(want[c % len(want)]).reshape(-1), names, shape)
        raise AssertionError(f"{label}: {int(bad.sum())} of {count} instances wrong, the first is instance {c}, {where}")


class Op:
    """one entry-point call on fixed device buffers.
    inputs  [(buffer the call reads, device tensor holding the real words)]: poisoned with zeros (in range for every modulus) until
            the real words are copied in on the stream under test -- a read-modify-write output is listed here too
    fresh   output buffers the call only writes: filled with all-ones words before every pass
    outs    buffers to clone and hand to check(clones)"""

    def __init__(self, label, inputs, fresh, outs, call, check):
        self.label, self.inputs, self.fresh, self.outs, self.call, self.check = label, inputs, fresh, outs, call, check

    def poison(self):
        for buf, _ in self.inputs:
            buf.zero_()
        for o in self.fresh:
            o.fill_(-1)


def pass_on_side_stream(op, s, fill, warm):
    """part A's sequence, once. warm: the call must return while the filler is pending"""
    torch = torch_()
    op.poison()
    torch.cuda.synchronize()                                       # poison and real words are in place; no device-wide wait from here on
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        t0 = time.perf_counter()
        e0.record()
        fill()
        e1.record()
        for buf, real in op.inputs:
            buf.copy_(real, non_blocking=True)
        op.call()
        idle = s.query()
        host_us = (time.perf_counter() - t0) * 1e6
        clones = [o.clone() for o in op.outs]
    s.synchronize()                                                # the only wait
    print(f"[streams A] {op.label} ({'warm' if warm else 'first'}): returned {host_us:.0f} us after the filler's first launch, "
          f"filler {e0.elapsed_time(e1):.2f} ms on the device, stream {'idle' if idle else 'pending'} at return")
    op.check(clones)
    if warm:
        assert not idle, f"{op.label}: the stream was idle when the warm call returned -- the filler did not cover the call ({host_us:.0f} us)"


def first_then_warm(op, s, fill):
    pass_on_side_stream(op, s, fill, warm=False)
    pass_on_side_stream(op, s, fill, warm=True)


def pass_on_own_stream(op, ctx):
    """part B: inputs made visible device-wide first, ctx.sync() the only wait behind the call"""
    op.poison()
    for buf, real in op.inputs:
        buf.copy_(real)
    torch_().cuda.synchronize()
    op.call()
    ctx.sync()
    op.check(op.outs)


# ---------------------------------------------------------------------------------------------------------------- the operations
def dev_pair(hx, dev, distinct, count=None):
    """(zeroed device buffer, device tensor with the real words): `count` instances cycling over the distinct ones, laid out on the device"""
    torch = torch_()
    base = hx.as_i64(np.stack([np.asarray(d, dtype=np.uint64).reshape(-1) for d in distinct])).to(dev)
    count = len(distinct) if count is None else count
    real = base[torch.arange(count, device=dev) % len(distinct)].reshape(-1).contiguous()
    return torch.zeros_like(real), real


def ntt_op(hx, ctx, dev, orc, n, q, batch, inverse, seed=300, distinct=3):
    t = orc.HexlTables(n, q)
    base = np.stack([orc.splitmix(n, seed + b, q) for b in range(distinct)])
    buf, real = dev_pair(hx, dev, base, batch)
    tabs = [hx.as_i64(a).to(dev) for a in (t.roots, t.precon, t.inv_roots, t.inv_precon)]
    want = (orc.ntt_inv if inverse else orc.ntt_fwd)(base, t)
    if inverse:
        call = lambda: ctx.ntt_inv(buf, tabs[2], tabs[3], q, t.inv_n, t.inv_n_w, n)
    else:
        call = lambda: ctx.ntt_fwd(buf, tabs[0], tabs[1], q, n)
    label = f"hexl_ntt_{'inv' if inverse else 'fwd'} n={n} batch={batch} q<2^{q.bit_length()}"
    return Op(label, [(buf, real)], [], [buf], call, lambda c: assert_every(hx, c[0], want, batch, ("coefficient",), (n,), label))


def dyadic_op(hx, ctx, dev, orc, n=1024, nm=2, batch=16):
    mod1 = np.array(orc.primes(nm, 52, n), dtype=np.uint64)
    A = [np.concatenate([orc.splitmix(n, 900 + b * 16 + k * 4 + i, int(mod1[i])) for k in range(2) for i in range(nm)]) for b in range(3)]
    B = [np.concatenate([orc.splitmix(n, 950 + b * 16 + k * 4 + i, int(mod1[i])) for k in range(2) for i in range(nm)]) for b in range(3)]
    a, ra = dev_pair(hx, dev, A, batch)
    b, rb = dev_pair(hx, dev, B, batch)
    mod = hx.as_i64(np.tile(mod1, batch)).to(dev)
    out = torch_().empty(batch * 3 * nm * n, dtype=torch_().int64, device=dev)
    want = [orc.dyadic(x, y, n, mod1, exact=True) for x, y in zip(A, B)]
    label = f"hexl_dyadic_multiply n={n} moduli={nm} batch={batch}"
    return Op(label, [(a, ra), (b, rb)], [out], [out], lambda: ctx.dyadic_multiply(out, a, b, mod, n, nm),
              lambda c: assert_every(hx, c[0], want, batch, ("component", "limb", "coefficient"), (3, nm, n), label))


def galois_op(hx, ctx, dev, orc, n=1024, count=32):
    g = pow(5, 3, 2 * n)
    x = orc.splitmix(count * n, 77).reshape(count, n)              # arbitrary 64-bit words: moved, never interpreted
    x[x == 0] = 1                                                   # (no word equal to the poison)
    buf, real = dev_pair(hx, dev, [x])
    out = torch_().empty_like(buf)
    want = list(apply_galois(x, n, g))
    label = f"hexl_apply_galois n={n} count={count}"
    return Op(label, [(buf, real)], [out], [out], lambda: ctx.apply_galois(out, buf, count, n, g),
              lambda c: assert_every(hx, c[0], want, count, ("coefficient",), (n,), label))


def keyswitch_op(hx, dev, orc, plan, case, nb, first=0, what="hexl_keyswitch"):
    """nb instances over min(nb, 3) distinct ones, KsCase.inputs(first ...); result is read-modify-write: poisoned and copied like t"""
    ins = [case.inputs(orc, first + b) for b in range(min(nb, 3))]
    t, rt = dev_pair(hx, dev, [i[0] for i in ins], nb)
    r, rr = dev_pair(hx, dev, [i[1] for i in ins], nb)
    want = [case.expected(orc, *i) for i in ins]
    label = f"{what} n={case.n} L={case.L} K={case.K} batch={nb} q<2^{int(case.moduli[0]).bit_length()}"
    return Op(label, [(t, rt), (r, rr)], [], [r], lambda: plan.keyswitch(r, t, nb),
              lambda c: assert_every(hx, c[0], want, nb, ("component", "limb", "coefficient"), (2, case.L, case.n), label))


def ciphertexts(orc, case, first, count, salt):
    n, L = case.n, case.L
    return [np.concatenate([orc.splitmix(n, case.seed * 31 + (first + b) * 977 + salt + k * 17 + i, int(case.moduli[i]))
                            for k in range(2) for i in range(L)]) for b in range(count)]


def mulrelin_op(hx, dev, orc, plan, case, nb):
    n, L = case.n, case.L
    A, B = ciphertexts(orc, case, 0, 3, 0), ciphertexts(orc, case, 0, 3, 5000)
    a, ra = dev_pair(hx, dev, A, nb)
    b, rb = dev_pair(hx, dev, B, nb)
    out = torch_().empty_like(a)
    want = []
    for x, y in zip(A, B):                                         # DyadicMultiply, then KeySwitch(result = components 0..1, t = component 2)
        prod = orc.dyadic(x, y, n, case.moduli[:L], exact=True)
        w = prod[:2 * L * n].copy()
        orc.keyswitch(w, prod[2 * L * n:].copy(), n, L, case.K, L + 1, case.moduli, case.keys, case.modswitch)
        want.append(w)
    label = f"hexl_multiply_relinearize n={n} L={L} K={case.K} batch={nb}"
    return Op(label, [(a, ra), (b, rb)], [out], [out], lambda: plan.multiply_relinearize(out, a, b, nb),
              lambda c: assert_every(hx, c[0], want, nb, ("component", "limb", "coefficient"), (2, L, n), label))


def rescale_op(hx, dev, orc, plan, qs, n, n_limbs, ncomp, nb, seed=1):
    lm = Limbs(orc, n, qs)
    inst = [rescale_input(lm, n_limbs, ncomp, "uniform", b, seed).reshape(-1) for b in range(min(nb, 3))]
    buf, real = dev_pair(hx, dev, inst, nb)
    out = torch_().empty(nb * ncomp * (n_limbs - 1) * n, dtype=torch_().int64, device=dev)
    want = [rescale(lm, x, 1, n_limbs, ncomp).reshape(-1) for x in inst]
    label = f"hexl_rescale n={n} n_limbs={n_limbs} components={ncomp} batch={nb}"
    return Op(label, [(buf, real)], [out], [out], lambda: plan.rescale(out, buf, nb, n_limbs, ncomp),
              lambda c: assert_every(hx, c[0], want, nb, ("component", "limb", "coefficient"), (ncomp, n_limbs - 1, n), label))


def rotate_op(hx, dev, orc, plan, case, nb, first=0):
    g = pow(5, 3, 2 * case.n)
    cts = ciphertexts(orc, case, first, 3, 0)
    buf, real = dev_pair(hx, dev, cts, nb)
    out = torch_().empty_like(buf)
    want = [rotate(orc, case, ct, g) for ct in cts]
    label = f"hexl_rotate n={case.n} L={case.L} K={case.K} batch={nb}"
    return Op(label, [(buf, real)], [out], [out], lambda: plan.rotate(out, buf, nb, g),
              lambda c: assert_every(hx, c[0], want, nb, ("component", "limb", "coefficient"), (2, case.L, case.n), label))


def rns_ntt_op(hx, dev, orc, plan, qs, n, count, inverse, in_place):
    K = len(qs)
    lm = Limbs(orc, n, qs)
    x = [ntt_input(lm, K, ("uniform", "extreme")[c % 2], c, 3, inverse) for c in range(3)]
    buf, real = dev_pair(hx, dev, x, count)
    out = buf if in_place else torch_().empty_like(buf)
    want = [rns_ntt(lm, v, K, inverse) for v in x]
    fn = plan.rns_ntt_inv if inverse else plan.rns_ntt_fwd
    label = f"hexl_rns_ntt_{'inv' if inverse else 'fwd'}{' in place' if in_place else ''} n={n} K={K} count={count}"
    return Op(label, [(buf, real)], [] if in_place else [out], [out], lambda: fn(out, buf, count, K),
              lambda c: assert_every(hx, c[0], want, count, ("limb", "coefficient"), (K, n), label))


def multiply_plain_op(hx, dev, orc, plan, qs, n, batch, ncomp, accumulate):
    K = len(qs)
    word = lambda seed, i: orc.splitmix(n, seed, int(qs[i]))
    cts = [np.stack([[word(7000 + b * 64 + k * 16 + i, i) for i in range(K)] for k in range(ncomp)]) for b in range(3)]
    prev = [np.stack([[word(8000 + b * 64 + k * 16 + i, i) for i in range(K)] for k in range(ncomp)]) for b in range(3)]
    pt = np.stack([word(9000 + i, i) for i in range(K)])
    ct, rct = dev_pair(hx, dev, cts, batch)
    d_pt, rpt = dev_pair(hx, dev, [pt])
    want = [multiply_plain(qs, n, cts[b], pt, ncomp, K, prev[b] if accumulate else None) for b in range(3)]
    if accumulate:
        out, rout = dev_pair(hx, dev, prev, batch)
        inputs, fresh = [(ct, rct), (d_pt, rpt), (out, rout)], []
    else:
        out = torch_().empty_like(ct)
        inputs, fresh = [(ct, rct), (d_pt, rpt)], [out]
    label = f"hexl_multiply_plain{' accumulate' if accumulate else ''} n={n} K={K} batch={batch} components={ncomp}"
    return Op(label, inputs, fresh, [out], lambda: plan.multiply_plain(out, ct, d_pt, batch, ncomp, K, 1, accumulate=accumulate),
              lambda c: assert_every(hx, c[0], want, batch, ("component", "limb", "coefficient"), (ncomp, K, n), label))


def integer_two_lane_op(hx, ctx, closing, dev, orc):
    """n = 1024, L = 2, K = 3, 55-bit primes, batch 96: the integer kernels; a batch >= 64 is split over the plan's two non-blocking
    auxiliary lanes, which must start behind the caller's stream and join back into it"""
    case = KsCase(orc, 1024, 2, 3, seed=81, bits=55)
    plan = make_plan(hx, ctx, closing, case)
    assert plan.tiers()[0][0] == -1
    return keyswitch_op(hx, dev, orc, plan, case, 96, what="hexl_keyswitch (integer kernels, two lanes)")


def rns_plan(hx, ctx, closing, orc, n=1024, K=4):
    qs = chain(orc, "gen", K, n)
    return make_plan(hx, ctx, closing, KsCase(orc, n, 1, K, moduli=qs), keys=False), qs


# ---------------------------------------------------------------------------------------------------------------- A
def build_a(which, hx, ctx, closing, dev, orc):
    if which.startswith("ntt_"):
        n, bits = 2048, int(which[-2:])
        q = orc.primes(2, bits, n)[1]
        return ntt_op(hx, ctx, dev, orc, n, q, 64, which.startswith("ntt_inv"))
    if which == "dyadic":
        return dyadic_op(hx, ctx, dev, orc)
    if which == "galois":
        return galois_op(hx, ctx, dev, orc)
    if which == "keyswitch_f64_one_lane":
        case = KsCase(orc, 2048, 3, 4, seed=82)
        return keyswitch_op(hx, dev, orc, make_plan(hx, ctx, closing, case), case, 40)
    if which == "keyswitch_f64_lone_instance":
        case = KsCase(orc, 16384, 3, 4, seed=83)
        return keyswitch_op(hx, dev, orc, make_plan(hx, ctx, closing, case), case, 1)
    if which == "keyswitch_f64_chunk_plus_one":
        case = KsCase(orc, 1024, 1, 2, seed=84)
        plan = make_plan(hx, ctx, closing, case)
        return keyswitch_op(hx, dev, orc, plan, case, chunk_of(plan) + 1)
    if which == "keyswitch_integer_two_lanes":
        return integer_two_lane_op(hx, ctx, closing, dev, orc)
    if which == "multiply_relinearize":
        case = KsCase(orc, 2048, 3, 4, seed=85)
        return mulrelin_op(hx, dev, orc, make_plan(hx, ctx, closing, case), case, 8)
    if which == "rescale":
        plan, qs = rns_plan(hx, ctx, closing, orc)
        return rescale_op(hx, dev, orc, plan, qs, 1024, 3, 2, 4)
    if which == "rotate_two_slices":
        case = KsCase(orc, 1024, 1, 2, seed=86)
        plan = make_plan(hx, ctx, closing, case)
        return rotate_op(hx, dev, orc, plan, case, chunk_of(plan) + 1)
    if which.startswith("rns_ntt_"):
        plan, qs = rns_plan(hx, ctx, closing, orc)
        return rns_ntt_op(hx, dev, orc, plan, qs, 1024, 6, "inv" in which, which.endswith("in_place"))
    assert which.startswith("multiply_plain"), which
    plan, qs = rns_plan(hx, ctx, closing, orc)
    return multiply_plain_op(hx, dev, orc, plan, qs, 1024, 3, 2, which.endswith("accumulate"))


A_OPS = ["ntt_fwd_51", "ntt_inv_51", "ntt_fwd_55", "ntt_inv_55", "dyadic", "galois", "keyswitch_f64_one_lane", "keyswitch_f64_lone_instance",
         "keyswitch_f64_chunk_plus_one", "keyswitch_integer_two_lanes", "multiply_relinearize", "rescale", "rotate_two_slices",
         "rns_ntt_fwd", "rns_ntt_fwd_in_place", "rns_ntt_inv", "rns_ntt_inv_in_place", "multiply_plain", "multiply_plain_accumulate"]


@pytest.mark.parametrize("which", A_OPS)
def test_entry_point_is_ordered_on_a_side_stream(hx, dev, orc, fill, closing, which):
    """the first call on a fresh context / plan (it may allocate; the rescale uploads its level's constants inside it) and the warm call,
    both against the oracle; the warm one returned while the filler was pending"""
    ctx, s = side_context(hx, closing)
    first_then_warm(build_a(which, hx, ctx, closing, dev, orc), s, fill)


def test_range_check_behind_a_keyswitch_on_a_side_stream(hx, dev, orc, fill, closing):
    """hexl_ks_range_check waits for the context's stream (so nothing is pending when it returns): in range, and the result is right"""
    ctx, s = side_context(hx, closing)
    case = KsCase(orc, 2048, 3, 4, seed=87)
    plan = make_plan(hx, ctx, closing, case)
    op = keyswitch_op(hx, dev, orc, plan, case, 40)
    keyswitch, seen = op.call, []
    op.call = lambda: (keyswitch(), seen.append(plan.range_check()))
    pass_on_side_stream(op, s, fill, warm=False)
    pass_on_side_stream(op, s, fill, warm=False)
    assert seen == [True, True], "an in-range keyswitch on the side stream was flagged (or the flag was read on another stream)"


# ---------------------------------------------------------------------------------------------------------------- B
def test_the_contexts_own_stream_and_the_round_trip(hx, dev, orc, fill, closing):
    """Context(0, use_torch_stream=False): the non-blocking stream of hexl_ctx_create, ctx.sync() the only wait behind each call. Then
    the round trip of the header: set_stream(side stream), checked as in part A, and use_own_stream(), checked through ctx.sync()"""
    ctx = hx.Context(0, use_torch_stream=False)
    closing.append(ctx)
    n = 2048
    fwd = ntt_op(hx, ctx, dev, orc, n, orc.primes(2, 51, n)[1], 64, False)
    plan, qs = rns_plan(hx, ctx, closing, orc)
    ops = [fwd, integer_two_lane_op(hx, ctx, closing, dev, orc), rescale_op(hx, dev, orc, plan, qs, 1024, 3, 2, 4),
           rns_ntt_op(hx, dev, orc, plan, qs, 1024, 6, False, False)]
    for op in ops:
        pass_on_own_stream(op, ctx)
    s = torch_().cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    pass_on_side_stream(fwd, s, fill, warm=True)
    ctx.use_own_stream()
    pass_on_own_stream(ops[1], ctx)
    pass_on_own_stream(fwd, ctx)


# ---------------------------------------------------------------------------------------------------------------- C
def switch_with_work_in_flight(ctx, a, b, first, second, label):
    """first() on stream a, then -- no wait -- the context moves to stream b and second() is called; both streams are waited for at the
    end. Returns whether the first launch was still in flight when the second call returned (the condition of part C)."""
    torch = torch_()
    torch.cuda.synchronize()
    ctx.set_stream(a.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(a)
    first()
    e1.record(a)
    t0 = time.perf_counter()
    ctx.set_stream(b.cuda_stream)
    second()
    in_flight = not e1.query()
    host_us = (time.perf_counter() - t0) * 1e6
    a.synchronize()
    b.synchronize()
    print(f"[streams C] {label}: first launch {e0.elapsed_time(e1):.3f} ms on the device, second call (switch + launch) enqueued in "
          f"{host_us:.0f} us, first launch {'in flight' if in_flight else 'FINISHED'} when it returned")
    return in_flight


def run_switch(ctx, op_a, op_b, label):
    """op_a on one side stream, op_b on another with op_a in flight; every instance of both against the oracle. The sequence runs twice:
    a rehearsal that is waited for and not looked at (first calls allocate scratch, load kernels, create the switch event and the streams'
    hardware queues, all on the host's time), then the pass that counts, on inputs and outputs set up afresh"""
    torch = torch_()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for counts in (False, True):
        for op in (op_a, op_b):
            op.poison()
            for buf, real in op.inputs:
                buf.copy_(real)
        in_flight = switch_with_work_in_flight(ctx, a, b, op_a.call, op_b.call, label + ("" if counts else " (rehearsal)"))
    op_a.check(op_a.outs)
    op_b.check(op_b.outs)
    assert in_flight, f"{label}: the first launch had finished when the second call returned -- nothing was in flight at the switch"


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_switching_streams_with_a_transform_in_flight(hx, dev, orc, closing, inverse):
    """C1. One derived-table buffer per context ([64 counters | w | w/p], rewritten by the preparation kernel in front of every launch):
    a large launch under a 51-bit prime on stream A, then, with no wait, set_stream(B) and 8 polynomials under the largest prime below
    2^52 (the strict tier, which also writes w/p). Without the ordering of hexl_ctx_set_stream the second preparation overwrites the
    tables the first transform is still reading (observed on an MI355X with that ordering taken out: every polynomial of the large
    forward launch and 59989 of 60000 of the inverse one came back wrong). Every polynomial of both launches. Timings: see C1_BATCH."""
    n = 4096
    ctx = hx.Context(0)
    closing.append(ctx)
    q1, q2 = orc.primes(2, 51, n)[1], primes_below(orc, 1, 1 << 52, n)[0]
    big = ntt_op(hx, ctx, dev, orc, n, q1, C1_BATCH, inverse, seed=500, distinct=7)
    small = ntt_op(hx, ctx, dev, orc, n, q2, 8, inverse, seed=600, distinct=8)
    run_switch(ctx, big, small, f"hexl_ntt_{'inv' if inverse else 'fwd'} n={n}, {C1_BATCH} polynomials then 8")


@pytest.mark.parametrize("what", ["keyswitch", "rescale", "rotate"])
def test_switching_streams_with_plan_scratch_in_flight(hx, dev, orc, closing, what):
    """C2. One FP64 plan, n = 1024, L = 3, K = 4: one full chunk on stream A, then, with no wait, set_stream(B) and one full chunk of
    different inputs -- both calls work in the plan's one keyswitch scratch / rescale scratch (d_rs_s) / rotate buffer (d_rot_t).
    Measured on an MI355X, device time of the first launch / host time to enqueue the second call (switch included): keyswitch
    0.311 ms / 19 us, rotate 0.410 ms / 21 us. One chunk of the rescale (three components, the most it takes) measured 0.161 ms / 18 us,
    9 times: its first call is therefore TWO full chunks (two launches back to back through the same d_rs_s), the second call one."""
    n, L, K = 1024, 3, 4
    ctx = hx.Context(0)
    closing.append(ctx)
    case = KsCase(orc, n, L, K, seed=88)
    plan = make_plan(hx, ctx, closing, case)
    assert plan.tiers()[0][0] >= 0, "not an FP64 plan"
    nb = chunk_of(plan)
    if what == "keyswitch":
        ops = [keyswitch_op(hx, dev, orc, plan, case, nb, first=f) for f in (0, 3)]
    elif what == "rescale":
        ops = [rescale_op(hx, dev, orc, plan, [int(q) for q in case.moduli], n, 3, 3, count, seed=sd) for count, sd in ((2 * nb, 1), (nb, 2))]
    else:
        ops = [rotate_op(hx, dev, orc, plan, case, nb, first=f) for f in (0, 3)]
    run_switch(ctx, ops[0], ops[1], f"{what}, chunks of {nb}")


# ---------------------------------------------------------------------------------------------------------------- D
def test_the_legacy_default_stream_set_explicitly(hx, dev, orc, closing):
    ctx = hx.Context(0, use_torch_stream=False)
    closing.append(ctx)
    ctx.set_stream(0)
    n = 2048
    pass_on_own_stream(ntt_op(hx, ctx, dev, orc, n, orc.primes(2, 51, n)[1], 64, False), ctx)
    case = KsCase(orc, n, 3, 4, seed=82)
    pass_on_own_stream(keyswitch_op(hx, dev, orc, make_plan(hx, ctx, closing, case), case, 40), ctx)


def test_null_context_handles_are_refused(hx):
    assert hx.lib().hexl_ctx_set_stream(None, None) == -1          # HEXL_E_BADARG
    assert hx.lib().hexl_ctx_use_own_stream(None) == -1


def test_two_contexts_on_two_streams_interleaved(hx, dev, orc, closing):
    """two contexts on one device, each on its own side stream with its own plan: they share no scratch, so nothing orders them against
    each other. Calls queued alternately, both streams waited for once at the end."""
    torch = torch_()
    n = 2048
    sides = [side_context(hx, closing) for _ in range(2)]
    qs = orc.primes(3, 51, n)[1:]
    ops = []
    for (ctx, _), q, seed, first in zip(sides, qs, (91, 92), (0, 3)):
        case = KsCase(orc, n, 3, 4, seed=seed)
        ops.append([ntt_op(hx, ctx, dev, orc, n, q, 64, False, seed=700 + seed),
                    keyswitch_op(hx, dev, orc, make_plan(hx, ctx, closing, case), case, 40, first=first)])
    for pair in ops:
        for op in pair:
            op.poison()
            for buf, real in op.inputs:
                buf.copy_(real)
    torch.cuda.synchronize()
    for k in range(2):
        for pair in ops:
            pair[k].call()
    for _, s in sides:
        s.synchronize()
    for pair in ops:
        for op in pair:
            op.check(op.outs)
