"""GPU: hexl_relinearize and hexl_multiply_sum_relinearize, bit-exact against the oracle's key switch on the split components
(tests/tensor_model.py), every instance; the fused call also against its normative composition on the device (hexl_ct_tensor_sum then
hexl_relinearize) and, for one term, against hexl_multiply_relinearize. K = L + 1. Every output buffer starts as -1: the calls write it.
Slices: a child process with HEXL_KS_CHUNK=3 and batch 8 against the unchunked words of this process. At the end a slot-wise dot product
of four encrypted pairs with ONE key switch, nothing downloaded but the slots."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ks_util import KsCase, extreme_ciphertext
from rns_model import assert_instances
from tensor_model import ct_tensor_sum, multiply_sum_relinearize, relinearize

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BATCH = 3
NAMES = ("component", "limb", "coefficient")
HEXL_E_BADARG, HEXL_E_NOKEYS = -1, -2


def torch_():
    import torch
    return torch


def minus_one(dev, words):
    return torch_().full((words,), -1, dtype=torch_().int64, device=dev)


def up(hx, dev, a):
    return hx.as_i64(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)).to(dev)


def keyed_plan(hx, ctx, case):
    plan = hx.KeySwitchPlan(ctx, case.n, case.L, case.K, case.K, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    return plan


def words(orc, case, family, components, limbs, b, salt):
    """instance b of a [components][limbs][n] operand: uniform residues or ks_util.extreme_words"""
    if family == "extreme":
        return extreme_ciphertext(case, b, components, limbs=limbs, salt=salt)
    return np.concatenate([orc.splitmix(case.n, 4001 + salt * 1009 + b * 97 + k * 17 + i, int(case.moduli[i]))
                           for k in range(components) for i in range(limbs)])


def operands(orc, case, family, n_terms, count, in_limbs=None):
    """(a[t][b], b[t][b]): `count` distinct instances of every operand, flat [2][limbs][n]; salts differ by non-multiples of nine"""
    il = [[case.L, case.L]] * n_terms if in_limbs is None else in_limbs
    a = [[words(orc, case, family, 2, il[t][0], b, 2 * t) for b in range(count)] for t in range(n_terms)]
    bb = [[words(orc, case, family, 2, il[t][1], b, 2 * t + 1) for b in range(count)] for t in range(n_terms)]
    return a, bb


def mixed(case, n_terms):
    """in_limbs entries in L ... K, a_t and b_t of a term at different counts"""
    return [[case.K if t % 2 == 0 else case.L, case.L if t % 3 == 0 else case.K] for t in range(n_terms)]


def tile(hx, dev, distinct, nb):
    """nb instances cycling over the distinct ones, on the device"""
    torch = torch_()
    base = up(hx, dev, np.stack(distinct)).view(len(distinct), -1)
    return base[torch.arange(nb, device=dev) % len(distinct)].reshape(-1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ hexl_relinearize
@pytest.mark.parametrize("family", ["uniform", "extreme"])
@pytest.mark.parametrize("n,L", [(1024, 2), (1024, 3), (2048, 2), (2048, 3)])
def test_relinearize_is_the_keyswitch_on_the_split_components(hx, ctx, dev, orc, n, L, family):
    case = KsCase(orc, n, L, L + 1, seed=7, extreme_keys=family == "extreme")
    plan = keyed_plan(hx, ctx, case)
    cts = [words(orc, case, family, 3, L, b, 4) for b in range(BATCH)]
    want = [relinearize(orc, case, ct) for ct in cts]
    d_ct3 = up(hx, dev, np.stack(cts))
    out = minus_one(dev, BATCH * 2 * L * n)
    plan.relinearize(out, d_ct3, BATCH)
    ctx.sync()
    assert_instances(hx.to_u64(out), want, BATCH, NAMES, (2, L, n), f"hexl_relinearize n={n} L={L} {family}")
    assert np.array_equal(hx.to_u64(d_ct3), np.stack(cts).reshape(-1)), "the input was written"
    assert plan.range_check()
    plan.close()


def test_relinearize_on_an_integer_kernel_plan(hx, ctx, dev, orc):
    """a modulus >= 2^52: the plan runs the integer kernels, and the call -- word moves and the key switch -- serves it"""
    n, L = 1024, 2
    case = KsCase(orc, n, L, L + 1, seed=9, bits=55)
    plan = keyed_plan(hx, ctx, case)
    assert plan.tiers()[0][0] == -1
    cts = [words(orc, case, "uniform", 3, L, b, 4) for b in range(BATCH)]
    want = [relinearize(orc, case, ct) for ct in cts]
    out = minus_one(dev, BATCH * 2 * L * n)
    plan.relinearize(out, up(hx, dev, np.stack(cts)), BATCH)
    ctx.sync()
    assert_instances(hx.to_u64(out), want, BATCH, NAMES, (2, L, n), "hexl_relinearize on the integer kernels")
    a, b = operands(orc, case, "uniform", 1, BATCH)
    with pytest.raises(hx.HexlError, match="status -1"):          # the tensor kernel is FP64 arithmetic
        plan.multiply_sum_relinearize(out, [up(hx, dev, np.stack(a[0]))], [up(hx, dev, np.stack(b[0]))], BATCH)
    plan.close()


# ------------------------------------------------------------------------------------------------------- hexl_multiply_sum_relinearize
def fused_and_composition(hx, ctx, dev, plan, case, d_a, d_b, nb, il):
    """(the fused call's output, ct_tensor_sum then relinearize, the three-component sum), all on the device"""
    n, L = case.n, case.L
    fused = minus_one(dev, nb * 2 * L * n)
    plan.multiply_sum_relinearize(fused, d_a, d_b, nb, in_limbs=il)
    ct3 = minus_one(dev, nb * 3 * L * n)
    plan.ct_tensor_sum(ct3, d_a, d_b, nb, L, in_limbs=il)
    composed = minus_one(dev, nb * 2 * L * n)
    plan.relinearize(composed, ct3, nb)
    ctx.sync()
    return fused, composed, ct3


@pytest.mark.parametrize("family", ["uniform", "extreme"])
@pytest.mark.parametrize("n,L", [(1024, 2), (2048, 3)])
def test_multiply_sum_relinearize_model_composition_and_one_term(hx, ctx, dev, orc, n, L, family):
    torch = torch_()
    case = KsCase(orc, n, L, L + 1, seed=11, extreme_keys=family == "extreme")
    plan = keyed_plan(hx, ctx, case)
    for n_terms in (1, 2, 8):
        il = mixed(case, n_terms) if n_terms != 2 else None
        a, b = operands(orc, case, family, n_terms, BATCH, il)
        want = [multiply_sum_relinearize(orc, case, [x[i] for x in a], [y[i] for y in b], il) for i in range(BATCH)]
        d_a = [up(hx, dev, np.stack(x)) for x in a]
        d_b = [up(hx, dev, np.stack(y)) for y in b]
        fused, composed, _ = fused_and_composition(hx, ctx, dev, plan, case, d_a, d_b, BATCH, il)
        label = f"n={n} L={L} {family} terms={n_terms} in_limbs={il}"
        assert_instances(hx.to_u64(fused), want, BATCH, NAMES, (2, L, n), f"hexl_multiply_sum_relinearize {label}")
        assert torch.equal(fused, composed), f"{label}: not ct_tensor_sum followed by relinearize"
        for t in range(n_terms):
            assert np.array_equal(hx.to_u64(d_a[t]), np.stack(a[t]).reshape(-1)) and np.array_equal(hx.to_u64(d_b[t]), np.stack(b[t]).reshape(-1))
    # one pair at L limbs: hexl_multiply_relinearize's words
    a, b = operands(orc, case, family, 1, BATCH)
    d_a, d_b = up(hx, dev, np.stack(a[0])), up(hx, dev, np.stack(b[0]))
    one, pair = minus_one(dev, BATCH * 2 * L * n), minus_one(dev, BATCH * 2 * L * n)
    plan.multiply_sum_relinearize(one, [d_a], [d_b], BATCH)
    plan.multiply_relinearize(pair, d_a, d_b, BATCH)
    ctx.sync()
    assert torch.equal(one, pair), "one term must be hexl_multiply_relinearize word for word"
    assert plan.range_check()
    plan.close()


def test_errors_in_the_house_order(hx, ctx, dev, orc):
    """HEXL_E_BADARG for anything malformed, then HEXL_E_NOKEYS, then nothing to do for an empty batch"""
    n, L = 1024, 2
    case = KsCase(orc, n, L, L + 1, seed=13)
    plan = hx.KeySwitchPlan(ctx, n, L, L + 1, L + 1, 2, case.moduli, case.modswitch)          # no keys yet
    ct3 = torch_().zeros(BATCH * 3 * L * n, dtype=torch_().int64, device=dev)
    a = torch_().zeros(BATCH * 2 * (L + 1) * n, dtype=torch_().int64, device=dev)
    out = minus_one(dev, BATCH * 2 * L * n)
    for batch in (BATCH, 0):
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_NOKEYS}$"):
            plan.relinearize(out, ct3, batch)
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_NOKEYS}$"):
            plan.multiply_sum_relinearize(out, [a], [a], batch)
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_BADARG}$"):      # overlap is found before the missing keys
            plan.relinearize(ct3[:BATCH * 2 * L * n], ct3, batch or 1)
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_BADARG}$"):
            plan.multiply_sum_relinearize(a[n:n + BATCH * 2 * L * n], [a], [a], batch or 1)
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_BADARG}$"):
            plan.multiply_sum_relinearize(out, [], [], batch)
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_BADARG}$"):
            plan.multiply_sum_relinearize(out, [a] * 9, [a] * 9, batch)
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_BADARG}$"):
            plan.multiply_sum_relinearize(out, [a], [a], batch, in_limbs=[[L - 1, L]])
        with pytest.raises(hx.HexlError, match=f"status {HEXL_E_BADARG}$"):
            plan.multiply_sum_relinearize(out, [a], [a], batch, in_limbs=[[L, L + 2]])
    ctx.sync()
    assert bool((out == -1).all()) and not bool(ct3.any()) and not bool(a.any()), "a refusal wrote something"
    plan.set_keys(case.keys)
    plan.relinearize(out, ct3, 0)
    plan.multiply_sum_relinearize(out, [a], [a], 0)
    ctx.sync()
    assert bool((out == -1).all()), "an empty batch wrote something"
    plan.close()


def test_a_plan_grows_its_slice_buffer(hx, ctx, dev, orc):
    """batch 2, then 5, then 3 on one plan: the grow-only slice buffer, shared with hexl_rotate, at every size"""
    n, L = 1024, 2
    case = KsCase(orc, n, L, L + 1, seed=17)
    plan = keyed_plan(hx, ctx, case)
    a, b = operands(orc, case, "uniform", 2, 3)
    want = [multiply_sum_relinearize(orc, case, [x[i] for x in a], [y[i] for y in b]) for i in range(3)]
    for nb in (2, 5, 3):
        d_a, d_b = [tile(hx, dev, x, nb) for x in a], [tile(hx, dev, y, nb) for y in b]
        fused, composed, _ = fused_and_composition(hx, ctx, dev, plan, case, d_a, d_b, nb, None)
        assert_instances(hx.to_u64(fused), want, nb, NAMES, (2, L, n), f"batch {nb}, fused")
        assert_instances(hx.to_u64(composed), want, nb, NAMES, (2, L, n), f"batch {nb}, composed")
    rot = minus_one(dev, 4 * 2 * L * n)                           # the other user of the buffer still runs
    plan.rotate(rot, tile(hx, dev, a[0], 4), 4, 1)
    ctx.sync()
    assert not bool((rot == -1).all())
    plan.close()


SLICE_CASE = dict(n=1024, L=2, seed=19, n_terms=3, distinct=3, nb=8)


def slice_calls(hx, ctx, dev, orc):
    """the three calls at batch 8 over three distinct instances -> {name: words}; shared by the parent (unchunked) and the child"""
    c = SLICE_CASE
    case = KsCase(orc, c["n"], c["L"], c["L"] + 1, seed=c["seed"])
    plan = keyed_plan(hx, ctx, case)
    il = mixed(case, c["n_terms"])
    a, b = operands(orc, case, "uniform", c["n_terms"], c["distinct"], il)
    d_a, d_b = [tile(hx, dev, x, c["nb"]) for x in a], [tile(hx, dev, y, c["nb"]) for y in b]
    fused, composed, ct3 = fused_and_composition(hx, ctx, dev, plan, case, d_a, d_b, c["nb"], il)
    assert plan.range_check()
    res = {"fused": hx.to_u64(fused), "composed": hx.to_u64(composed), "ct3": hx.to_u64(ct3)}
    return plan, res


def test_slices_with_a_ragged_tail(hx, ctx, dev, orc, tmp_path):
    """HEXL_KS_CHUNK=3 (read once per process, so a child process) and batch 8: two full slices and a tail of two, the slice buffer
    rewritten by each slice. Three distinct instances: row r of one slice differs from row r of the next. The child's words are
    compared with this process's unchunked ones."""
    plan, res = slice_calls(hx, ctx, dev, orc)
    assert plan.scratch_bytes(3) < plan.scratch_bytes(8), "this process must run batch 8 in one slice"
    plan.close()
    assert np.array_equal(res["fused"], res["composed"])
    ref = tmp_path / "unchunked.npz"
    np.savez(ref, **res)
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch, hexl_fpga_amd as hx, orc
from test_gpu_relinearize import slice_calls
dev = torch.device("cuda:0")
ctx = hx.Context(0)
plan, res = slice_calls(hx, ctx, dev, orc)
assert plan.scratch_bytes(3) == plan.scratch_bytes(100) > plan.scratch_bytes(2), "HEXL_KS_CHUNK=3 not in force"
want = np.load(%r)
for name in ("ct3", "composed", "fused"):
    assert np.array_equal(res[name], want[name]), name + " differs from the unchunked words"
print("SLICES OK")
''' % (str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests"), str(ref))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HEXL_KS_CHUNK="3"))
    print(out.stdout[-1000:], out.stderr[-1500:])
    assert out.returncode == 0 and "SLICES OK" in out.stdout


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_dot_product_end_to_end_one_key_switch(hx, ctx, dev, orc):
    """sum_t x_t y_t, slot-wise, for T = 4 encrypted pairs with |x|, |y| <= 1: n = 1024, L = 3, K = 4, four 40-bit primes, scale D = q_2;
    secret = hexl_sample(TERNARY) at K limbs; gen_relin_keys; hexl_ckks_encode -> hexl_rlwe_encrypt (2 T ciphertexts) -> ONE
    hexl_multiply_sum_relinearize -> hexl_rescale -> hexl_rlwe_decrypt -> hexl_ckks_decode.

    The bound, derived before any run, from the terms of test_gpu_keygen.py::test_square_end_to_end_nothing_downloaded_but_the_slots
    (whose docstring, with test_gpu_rlwe.py's, derives them; units: one integer step of a coefficient; an error of at most h in every
    coefficient reaches a slot with at most n h; ||s||_1 <= n; F = 16 log2(n) 2^-53):
      encode      slots D z + eps, |eps| <= E = n/2 + sqrt(n) F D
      fresh noise |e_j| <= 21 -> at most 21 n in a slot: a ciphertext decrypts to D z + d, |d| <= N1 = E + 21 n
      product     (D x + d)(D y + d') = D^2 x y + D x d' + D y d + d d', exactly, under (1, s, s^2): error at most 2 D N1 + N1^2 per
                  product for |x|, |y| <= 1 -- the square's term -- and T of them in the sum: T (2 D N1 + N1^2)
      key switch  ONCE, on the summed c2: its digits are below q_d whatever T is, so the term is the square's, not T times it:
                  KS = n (L n 21 max(q_d) / P + (n + 1) / 2)
      rescale     once: n (n + 1) / 2 in a slot, after the division by q_2 = D
    Slot error of the result at scale D: (T (2 D N1 + N1^2) + KS) / D + n (n + 1) / 2; divided by D by decode, whose FFT adds at most
    F ||result||_2; the numpy reference is good to 2^-50 per product (T 2^-50). With n = 1024, D ~ 2^40, T = 4: 2 T N1 / D ~ 1.6e-7,
    n (n + 1) / (2 D) ~ 4.8e-7: about 6.4e-7 in all."""
    torch = torch_()
    n, Kc, L, count, T = 1024, 4, 3, 2, 4
    qs = [int(q) for q in orc.primes(Kc, 40, n)]
    P = qs[Kc - 1]
    case = KsCase(orc, n, L, Kc, seed=5, moduli=qs)
    plan = hx.KeySwitchPlan(ctx, n, L, Kc, Kc, 2, case.moduli, case.modswitch)
    seed = bytes((29 * k + 3) & 0xFF for k in range(32))
    s = minus_one(dev, Kc * n)
    plan.sample(s, hx.SAMPLE_TERNARY, 1, Kc, seed=seed, stream=1)
    plan.gen_relin_keys(s, seed=seed, stream=2)
    D = float(qs[2])
    assert int(D) == qs[2]
    rng = np.random.default_rng(31)

    def unit_disc():
        z = np.sqrt(rng.random((count, n // 2))) * np.exp(2j * np.pi * rng.random((count, n // 2)))
        z[:, 0], z[:, 1], z[:, 2] = 1.0, -1.0, 1j
        assert np.abs(z).max() <= 1.0 + 1e-15
        return z

    def encrypted(z, index):
        enc = minus_one(dev, count * L * n)
        plan.ckks_encode(enc, torch.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))).to(dev), count, L, D)
        ct = minus_one(dev, count * 2 * L * n)
        plan.rlwe_encrypt(ct, s, count, L, pt=enc, pt_batch=count, seed=seed, stream=3, first=index * count)
        return ct

    xs, ys = [unit_disc() for _ in range(T)], [unit_disc() for _ in range(T)]
    d_x = [encrypted(z, t) for t, z in enumerate(xs)]
    d_y = [encrypted(z, T + t) for t, z in enumerate(ys)]
    dot = minus_one(dev, count * 2 * L * n)
    plan.multiply_sum_relinearize(dot, d_x, d_y, count)
    dot2 = minus_one(dev, count * 2 * 2 * n)
    plan.rescale(dot2, dot, count, L, 2)
    dec = minus_one(dev, count * 2 * n)
    plan.rlwe_decrypt(dec, dot2, s, count, 2, 2)
    d_out = torch.full((count, n // 2, 2), float("nan"), dtype=torch.float64, device=dev)
    plan.ckks_decode(d_out, dec, count, 2, D)
    ctx.sync()
    assert plan.range_check()
    o = d_out.cpu().numpy()
    got, want = o[..., 0] + 1j * o[..., 1], sum(x * y for x, y in zip(xs, ys))
    F = 16 * math.log2(n) * 2.0 ** -53
    E = n / 2 + math.sqrt(n) * F * D
    N1 = E + 21 * n
    KS = n * (L * n * 21 * max(qs[:L]) / P + (n + 1) / 2)
    for b in range(count):
        tol = ((T * (2 * D * N1 + N1 * N1) + KS) / D + n * (n + 1) / 2) / D + F * float(np.linalg.norm(want[b])) + T * 2.0 ** -50
        err = float(np.abs(got[b] - want[b]).max())
        print(f"[relinearize] dot product of {T} pairs with one key switch, instance {b}: max |error| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, f"instance {b}: {err:.3e} > {tol:.3e}"
    plan.close()
