"""GPU: hexl_ks_set_keys_device and hexl_ks_gen_keys against the host route they replace.

A plan's key copies are not readable from outside, so each copy is checked through the pipeline that reads it, with two plans of the
same parameters: plan A keyed by hexl_ks_set_keys (the route every other test pins to the oracle), plan B keyed on the device. Inputs
are uniform residues in t_target and result, so every key word meets a random digit and one wrong word changes the output; all
comparisons are on the device, every word, no tolerance.

Which copy a batch reads (hx_launch_keyswitch, keyswitch.hip; `path_of` below restates the rules and every case asserts the path it
means to pin, with the CU count read from the context):
  int   integer plans (a modulus >= 2^52): d_keys, words beside Shoup factors; two lanes from 64 instances
  x     FP64, 4 nb L n >= 7 CUs 16384 (hx_ks_x_applies): d_keys_x, slot-major order; two halves at n = 32768
  lat   FP64, n = 16384, nb <= 8 and nb L (L + 1) <= 128 (hx_ks_lat_applies): d_keys_nat, natural order
  f64   every other FP64 batch: d_keys_f64, the (b, d)-major order
No environment knob is needed: the default rules reach every copy with batches of a few to a few thousand instances."""
import math
import re

import numpy as np
import pytest

import sample_model as sm
from ks_util import KsCase, extreme_words
from test_gpu_streams import Op, closing, dev_pair, fill, first_then_warm, side_context  # noqa: F401  (closing, fill: fixtures)

pytestmark = pytest.mark.gpu

SEED = bytes((37 * k + 11) & 0xFF for k in range(32))
DISTINCT = 5


def torch_():
    import torch
    return torch


def num_cu(ctx):
    return int(re.search(r"(\d+) CUs", ctx.describe()).group(1))


def path_of(ctx, case, nb, integer=False):
    """the copy of the keys a batch of nb (one chunk) reads under the default knobs"""
    n, L = case.n, case.L
    logn = n.bit_length() - 1
    chunk = 256 >> (logn - 14) if logn >= 14 else 256 << (14 - logn)
    assert nb <= chunk, "one scratch chunk per case: a batch beyond it is split and each piece routed on its own"
    if integer:
        return "int"
    if 4 * nb * L * n >= 7 * num_cu(ctx) * 16384:
        return "x"
    if n == 16384 and nb <= 8 and nb * L * (L + 1) <= 128:
        return "lat"
    return "f64"


def x_batch(ctx, case):
    """the smallest batch the slot-major pipeline takes"""
    return -(-7 * num_cu(ctx) * 16384 // (4 * case.L * case.n))


def key_words(case, salt):
    """L key slices of 2 K n words: full-range 64-bit words (most of them >= q) with limbs of extreme_words and of 2^64 - 1 between"""
    rng = np.random.default_rng(1000 + salt)
    n, K = case.n, case.K
    keys = []
    for d in range(case.L):
        k = rng.integers(0, 1 << 64, size=2 * K * n, dtype=np.uint64)
        for row in range(2 * K):
            i = row % K
            if (row + d + salt) % 3 == 0:
                k[row * n:(row + 1) * n] = extreme_words(n, int(case.moduli[i]), row + 2 * d + salt)
            elif (row + d + salt) % 7 == 1:
                k[row * n:(row + 1) * n] = np.uint64(0xFFFFFFFFFFFFFFFF)
        keys.append(k)
    return keys


def uniform_inputs(hx, dev, case, nb, salt=0):
    """(t_target [nb][L][n], result [nb][2][L][n]) on the device: DISTINCT instances of uniform residues, cycled"""
    rng = np.random.default_rng(77 + salt)
    qs = [int(q) for q in case.moduli[:case.L]]
    t = [np.concatenate([rng.integers(0, q, size=case.n, dtype=np.uint64) for q in qs]) for _ in range(DISTINCT)]
    r = [np.concatenate([rng.integers(0, q, size=case.n, dtype=np.uint64) for _ in range(2) for q in qs]) for _ in range(DISTINCT)]
    return dev_pair(hx, dev, t, nb)[1], dev_pair(hx, dev, r, nb)[1]


def make_plans(hx, ctx, case, count=2):
    return [hx.KeySwitchPlan(ctx, case.n, case.L, case.K, case.K, 2, case.moduli, case.modswitch) for _ in range(count)]


def up(hx, dev, a):
    return hx.as_i64(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)).to(dev)


def same_keyswitch(hx, ctx, dev, case, plan_a, plan_b, nb, label, salt=0):
    """plan_a and plan_b leave the same words for a batch of nb, and the keyswitch changed the result"""
    torch = torch_()
    t, r = uniform_inputs(hx, dev, case, nb, salt)
    ra, rb = r.clone(), r.clone()
    plan_a.keyswitch(ra, t, nb)
    plan_b.keyswitch(rb, t, nb)
    ctx.sync()
    assert not torch.equal(ra, r), f"{label}: the keyswitch left the result as it was"
    bad = int((ra != rb).sum())
    assert bad == 0, f"{label}: {bad} of {ra.numel()} words differ, the first at {int(torch.nonzero(ra != rb)[0])}"
    return ra


# (n, L, K, bits, [(batch or "x" = the slot-major threshold, the path it pins)])
INSTALL = [
    (1024, 3, 4, 51, [(3, "f64"), ("x", "x")]),
    (1024, 2, 4, 51, [(3, "f64"), ("x", "x")]),                   # K > L + 1: the special prime is not limb L, limb 2 is never read
    (1024, 1, 2, 51, [(1, "f64"), (5, "f64")]),                   # L = 1 (the slot-major threshold lies beyond one chunk here)
    (1024, 15, 16, 40, [(2, "f64"), ("x", "x")]),
    (4096, 3, 4, 51, [(3, "f64"), ("x", "x")]),
    (16384, 2, 3, 51, [(1, "lat"), (9, "f64"), ("x", "x")]),      # the three paths of n = 16384, each with a copy of its own
    (32768, 3, 4, 51, [(2, "f64"), ("x", "x")]),                  # slot-major: the two-halves order
    (1024, 3, 4, 55, [(3, "int"), (70, "int")]),                  # integer kernels, 16 coefficients per thread; 70: two lanes
    (2048, 2, 3, 55, [(3, "int")]),                               # ... 32 per thread, a one-bit partial pass
]


@pytest.mark.parametrize("n,L,K,bits,batches", INSTALL, ids=[f"n{c[0]}_L{c[1]}_K{c[2]}_{c[3]}bit" for c in INSTALL])
def test_install_is_set_keys(hx, ctx, dev, orc, n, L, K, bits, batches):
    case = KsCase(orc, n, L, K, seed=3, bits=bits)
    a, b = make_plans(hx, ctx, case)
    integer = bits > 52
    assert (a.tiers()[0][0] == -1) == integer
    keys = key_words(case, n + L)
    a.set_keys(keys)
    d_keys = up(hx, dev, np.concatenate(keys))
    b.set_keys_device(d_keys)
    for nb, path in batches:
        nb = x_batch(ctx, case) if nb == "x" else nb
        assert path_of(ctx, case, nb, integer) == path
        same_keyswitch(hx, ctx, dev, case, a, b, nb, f"install n={n} L={L} K={K} batch={nb} ({path})")
    # the caller's buffer was only read
    assert np.array_equal(hx.to_u64(d_keys), np.concatenate(keys))
    a.close()
    b.close()


def test_install_serves_rotate_and_multiply_relinearize(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K, nb = 1024, 3, 4, 3
    case = KsCase(orc, n, L, K, seed=4)
    a, b = make_plans(hx, ctx, case)
    keys = key_words(case, 5)
    a.set_keys(keys)
    b.set_keys_device(up(hx, dev, np.concatenate(keys)))
    _, ct = uniform_inputs(hx, dev, case, nb, 1)
    _, ct2 = uniform_inputs(hx, dev, case, nb, 2)
    outs = []
    for plan in (a, b):
        rot, mul = torch.full_like(ct, -1), torch.full_like(ct, -1)
        plan.rotate(rot, ct, nb, 5)
        plan.multiply_relinearize(mul, ct, ct2, nb)
        outs.append((rot, mul))
    ctx.sync()
    assert torch.equal(outs[0][0], outs[1][0]), "hexl_rotate"
    assert torch.equal(outs[0][1], outs[1][1]), "hexl_multiply_relinearize"
    a.close()
    b.close()


@pytest.mark.parametrize("bits,nb", [(51, 3), (55, 70)], ids=["fp64", "integer_two_lanes"])
def test_rekeying_in_stream_order(hx, ctx, dev, orc, bits, nb):
    """install key 1, launch, install key 2, launch -- nothing waits in between: the second install is behind the first launch's lanes
    and in front of the second's. Both outputs are plan A's, which was keyed and synchronised the old way."""
    torch = torch_()
    n, L, K = 1024, 3, 4
    case = KsCase(orc, n, L, K, seed=6, bits=bits)
    a, b = make_plans(hx, ctx, case)
    k1, k2 = key_words(case, 1), key_words(case, 2)
    t, r = uniform_inputs(hx, dev, case, nb)
    want = []
    for keys in (k1, k2):
        a.set_keys(keys)
        ra = r.clone()
        a.keyswitch(ra, t, nb)
        ctx.sync()
        want.append(ra)
    assert not torch.equal(want[0], want[1])
    d1, d2 = up(hx, dev, np.concatenate(k1)), up(hx, dev, np.concatenate(k2))
    r1, r2 = r.clone(), r.clone()
    ctx.sync()
    b.set_keys_device(d1)
    b.keyswitch(r1, t, nb)
    b.set_keys_device(d2)
    b.keyswitch(r2, t, nb)
    ctx.sync()
    assert torch.equal(r1, want[0]), "the first launch saw something else than key 1"
    assert torch.equal(r2, want[1]), "the second launch saw something else than key 2"
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------- generate
def minus_one(dev, words):
    torch = torch_()
    return torch.full((words,), -1, dtype=torch.int64, device=dev)


def compose_keys(hx, ctx, plan, dev, case, s, kind, g, d_from, seed, stream, first):
    """today's route: s' by hexl_multiply_plain / hexl_apply_galois, the L plaintexts by hexl_ct_lincomb, one key-shaped
    hexl_rlwe_encrypt, one download, hexl_ks_set_keys (the recipe of test_gpu_rlwe.py::test_square_end_to_end_on_the_device)"""
    n, L, K = case.n, case.L, case.K
    qs = [int(q) for q in case.moduli]
    P = qs[K - 1]
    if kind == hx.KEY_FROM_POLY:
        sp = d_from
    else:
        sp = minus_one(dev, K * n)
        if kind == hx.KEY_FROM_SQUARE:
            plan.multiply_plain(sp, s, s, 1, 1, K, 1)
        else:
            ctx.apply_galois(sp, s, K, n, g)
    pts = minus_one(dev, L * K * n)
    for d in range(L):
        plan.ct_lincomb(pts[d * K * n:(d + 1) * K * n], [sp], 1, 1, K, weights=[[P % qs[i] if i == d else 0 for i in range(K)]])
    key = minus_one(dev, L * 2 * K * n)
    plan.rlwe_encrypt(key, s, L, K, pt=pts, pt_batch=L, seed=seed, stream=stream, first=first)
    ctx.sync()
    plan.set_keys(list(hx.to_u64(key).reshape(L, 2 * K * n)))


def secret_and_from(plan, dev, case):
    s, f = minus_one(dev, case.K * case.n), minus_one(dev, case.K * case.n)
    plan.sample(s, sm.TERNARY, 1, case.K, seed=SEED, stream=1)
    plan.sample(f, sm.UNIFORM, 1, case.K, seed=SEED, stream=9)
    return s, f


# (n, L, K, [(batch or "x", path)]): n = 16384 at small L on the lone path and on the slot-major one
GENERATE = [(1024, 3, 4, [(3, "f64"), ("x", "x")]), (1024, 2, 4, [(3, "f64"), ("x", "x")]), (16384, 2, 3, [(1, "lat"), ("x", "x")])]


@pytest.mark.parametrize("n,L,K,batches", GENERATE, ids=[f"n{c[0]}_L{c[1]}_K{c[2]}" for c in GENERATE])
def test_generate_is_the_composition(hx, ctx, dev, orc, n, L, K, batches):
    """every from_kind; Galois elements 5, 2n - 1 and 1; a nonzero `first` and a large stream number among the triples"""
    case = KsCase(orc, n, L, K, seed=8)
    a, b = make_plans(hx, ctx, case)
    s, f = secret_and_from(a, dev, case)
    s_before = s.clone()
    kinds = [(hx.KEY_FROM_POLY, 1, 2, 0), (hx.KEY_FROM_SQUARE, 1, 3, 5), (hx.KEY_FROM_GALOIS, 5, 0xFEDCBA9876543210, 0),
             (hx.KEY_FROM_GALOIS, 2 * n - 1, 4, (1 << 40) - L), (hx.KEY_FROM_GALOIS, 1, 5, 7)]
    for c, (kind, g, stream, first) in enumerate(kinds):
        compose_keys(hx, ctx, a, dev, case, s, kind, g, f, SEED, stream, first)
        # what the kind does not use is ignored: an even element and no d_from for the square, a stray d_from for the Galois key
        b.gen_keys(s, kind, galois_elt=g if kind == hx.KEY_FROM_GALOIS else 4, from_poly=f if kind != hx.KEY_FROM_SQUARE else None,
                   seed=SEED, stream=stream, first=first)
        for nb, path in batches:
            nb = x_batch(ctx, case) if nb == "x" else nb
            assert path_of(ctx, case, nb) == path
            same_keyswitch(hx, ctx, dev, case, a, b, nb, f"generate kind={kind} g={g} n={n} L={L} K={K} batch={nb} ({path})", salt=c)
    assert torch_().equal(s, s_before), "the secret was written"
    a.close()
    b.close()


def test_generate_depends_on_the_triple_and_only_on_it(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K, nb = 1024, 3, 4, 3
    case = KsCase(orc, n, L, K, seed=9)
    (plan,) = make_plans(hx, ctx, case, 1)
    s, _ = secret_and_from(plan, dev, case)
    t, r = uniform_inputs(hx, dev, case, nb)

    def out(seed, stream, first):
        plan.gen_relin_keys(s, seed=seed, stream=stream, first=first)
        rr = r.clone()
        plan.keyswitch(rr, t, nb)
        return rr

    base, again = out(SEED, 0, 0), out(SEED, 0, 0)
    moved, other_stream, other_seed = out(SEED, 0, 1), out(SEED, 1, 0), out(bytes(32), 0, 0)
    ctx.sync()
    assert torch.equal(base, again), "the same (seed, stream, first) gave another key"
    for what, o in (("first", moved), ("stream", other_stream), ("seed", other_seed)):
        assert not torch.equal(base, o), f"another {what} left the key as it was"
    plan.close()


# ------------------------------------------------------------------------------------------------------------------ end to end
def unit_disc(rng, count, n):
    z = np.sqrt(rng.random((count, n // 2))) * np.exp(2j * np.pi * rng.random((count, n // 2)))
    z[:, 0], z[:, 1], z[:, 2] = 1.0, -1.0, 1j
    assert np.abs(z).max() <= 1.0 + 1e-15
    return z


def slots_to_dev(dev, z):
    return torch_().from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))).to(dev)


def test_square_end_to_end_nothing_downloaded_but_the_slots(hx, ctx, dev, orc):
    """test_gpu_rlwe.py::test_square_end_to_end_on_the_device with the relinearisation key from gen_relin_keys: n = 1024, L = 3, K = 4,
    four 40-bit primes, scale D = q_2; secret = hexl_sample(TERNARY) at K limbs; hexl_ckks_encode -> hexl_rlwe_encrypt ->
    hexl_multiply_relinearize -> hexl_rescale -> hexl_rlwe_decrypt -> hexl_ckks_decode. The key is word for word that test's (the
    normative definition of hexl_ks_gen_keys), so the bound is that test's, term by term (its docstring derives it):
      E = n/2 + sqrt(n) F D, F = 16 log2(n) 2^-53;  N1 = E + 21 n;  KS = n (L n 21 max(q_d) / P + (n + 1) / 2)
      slot error <= ((2 D N1 + N1^2 + KS) / D + n (n + 1) / 2) / D + F ||z^2||_2 + 2^-50     (about 5.2e-7)"""
    torch = torch_()
    n, Kc, L, count = 1024, 4, 3, 2
    qs = [int(q) for q in orc.primes(Kc, 40, n)]
    P = qs[Kc - 1]
    case = KsCase(orc, n, L, Kc, seed=5, moduli=qs)
    (plan,) = make_plans(hx, ctx, case, 1)
    s = minus_one(dev, Kc * n)
    plan.sample(s, sm.TERNARY, 1, Kc, seed=SEED, stream=1)
    plan.gen_relin_keys(s, seed=SEED, stream=2)
    D = float(qs[2])
    assert int(D) == qs[2]
    z = unit_disc(np.random.default_rng(23), count, n)
    enc = minus_one(dev, count * L * n)
    plan.ckks_encode(enc, slots_to_dev(dev, z), count, L, D)
    ct = minus_one(dev, count * 2 * L * n)
    plan.rlwe_encrypt(ct, s, count, L, pt=enc, pt_batch=count, seed=SEED, stream=3)
    sq = minus_one(dev, count * 2 * L * n)
    plan.multiply_relinearize(sq, ct, ct, count)
    sq2 = minus_one(dev, count * 2 * 2 * n)
    plan.rescale(sq2, sq, count, L, 2)
    dec = minus_one(dev, count * 2 * n)
    plan.rlwe_decrypt(dec, sq2, s, count, 2, 2)
    d_out = torch.full((count, n // 2, 2), float("nan"), dtype=torch.float64, device=dev)
    plan.ckks_decode(d_out, dec, count, 2, D)
    ctx.sync()
    assert plan.range_check()
    o = d_out.cpu().numpy()
    got, want = o[..., 0] + 1j * o[..., 1], z * z
    F = 16 * math.log2(n) * 2.0 ** -53
    E = n / 2 + math.sqrt(n) * F * D
    N1 = E + 21 * n
    KS = n * (L * n * 21 * max(qs[:L]) / P + (n + 1) / 2)
    for b in range(count):
        tol = ((2 * D * N1 + N1 * N1 + KS) / D + n * (n + 1) / 2) / D + F * float(np.linalg.norm(want[b])) + 2.0 ** -50
        err = float(np.abs(got[b] - want[b]).max())
        print(f"[keygen] z^2 with a generated relinearisation key, instance {b}: max |error| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, f"instance {b}: {err:.3e} > {tol:.3e}"
    plan.close()


def test_rotation_end_to_end_nothing_downloaded_but_the_slots(hx, ctx, dev, orc):
    """z -> its rotation by one slot (g = 5: np.roll(z, -1)) and its conjugate (g = 2n - 1) with Galois keys from gen_galois_keys on two
    plans; n = 1024, L = 3, K = 4, four 40-bit primes, scale D = q_2: hexl_ckks_encode -> hexl_rlwe_encrypt -> hexl_rotate ->
    hexl_rlwe_decrypt -> hexl_ckks_decode at L limbs.

    The bound, derived before any run from the terms of the square test (units: one integer step of a coefficient; an error of at most
    h in every coefficient reaches a slot with at most n h; ||s||_1 <= n; F = 16 log2(n) 2^-53):
      encode      slots D z + eps, |eps| <= E = n/2 + sqrt(n) F D
      fresh noise |e_j| <= 21 -> at most 21 n in a slot: the ciphertext decrypts to D z + d, |d| <= N1 = E + 21 n
      rotation    sigma_g permutes the slots and maps a coefficient to a coefficient up to its sign: (sigma_g(c0), sigma_g(c1)) decrypts
                  under (1, sigma_g(s)) to sigma_g(D z + d), the rotated slots with the same |d|
      key switch  sigma_g(c1) sigma_g(s) is replaced by (sum_d [sigma_g(c1)]_(q_d) key_d) / P rounded: the key's errors (|.| <= 21) meet
                  digits below q_d, at most L n 21 max(q_d) / P per coefficient; the rounding is 1/2 in component 0 and 1/2 in
                  component 1, which meets s: (n + 1) / 2. Times n in a slot: KS = n (L n 21 max(q_d) / P + (n + 1) / 2)
    No product and no rescale: the slot error at scale D is N1 + KS; decode divides by D and its FFT adds at most F ||result||_2; numpy
    is good to 2^-50:
      slot error <= (N1 + KS) / D + F ||want||_2 + 2^-50.   With n = 1024, D ~ P ~ 2^40: N1 ~ 2.2e4, KS ~ 6.7e7, bound ~ 6.1e-5."""
    torch = torch_()
    n, Kc, L, count = 1024, 4, 3, 2
    qs = [int(q) for q in orc.primes(Kc, 40, n)]
    P = qs[Kc - 1]
    case = KsCase(orc, n, L, Kc, seed=5, moduli=qs)
    rot, conj = make_plans(hx, ctx, case)
    s = minus_one(dev, Kc * n)
    rot.sample(s, sm.TERNARY, 1, Kc, seed=SEED, stream=1)
    rot.gen_galois_keys(s, 5, seed=SEED, stream=2, first=0)
    conj.gen_galois_keys(s, 2 * n - 1, seed=SEED, stream=2, first=L)           # the same stream: `first` advanced by L
    D = float(qs[2])
    z = unit_disc(np.random.default_rng(29), count, n)
    enc = minus_one(dev, count * L * n)
    rot.ckks_encode(enc, slots_to_dev(dev, z), count, L, D)
    ct = minus_one(dev, count * 2 * L * n)
    rot.rlwe_encrypt(ct, s, count, L, pt=enc, pt_batch=count, seed=SEED, stream=3)
    F = 16 * math.log2(n) * 2.0 ** -53
    N1 = n / 2 + math.sqrt(n) * F * D + 21 * n
    KS = n * (L * n * 21 * max(qs[:L]) / P + (n + 1) / 2)
    for plan, g, want, what in ((rot, 5, np.roll(z, -1, axis=1), "rotate by one slot"), (conj, 2 * n - 1, np.conj(z), "conjugate")):
        out = minus_one(dev, count * 2 * L * n)
        plan.rotate(out, ct, count, g)
        dec = minus_one(dev, count * L * n)
        plan.rlwe_decrypt(dec, out, s, count, 2, L)
        d_out = torch.full((count, n // 2, 2), float("nan"), dtype=torch.float64, device=dev)
        plan.ckks_decode(d_out, dec, count, L, D)
        ctx.sync()
        assert plan.range_check()
        o = d_out.cpu().numpy()
        got = o[..., 0] + 1j * o[..., 1]
        for b in range(count):
            tol = (N1 + KS) / D + F * float(np.linalg.norm(want[b])) + 2.0 ** -50
            err = float(np.abs(got[b] - want[b]).max())
            print(f"[keygen] {what} with a generated Galois key, instance {b}: max |error| = {err:.3e}, bound {tol:.3e}")
            assert err <= tol, f"{what}, instance {b}: {err:.3e} > {tol:.3e}"
    rot.close()
    conj.close()


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_plan_as_it_was(hx, ctx, dev, orc):
    torch = torch_()
    n, L, K, nb = 1024, 3, 4, 3
    case = KsCase(orc, n, L, K, seed=10)
    plan, keyed = make_plans(hx, ctx, case)
    s, f = secret_and_from(plan, dev, case)
    t, r = uniform_inputs(hx, dev, case, nb)
    lib = hx.lib()
    seed_ok, _ = hx.seed_words(SEED)
    H, S, Fp = plan.h, s.data_ptr(), f.data_ptr()

    def bad_calls(h):
        return [
            lambda: lib.hexl_ks_set_keys_device(h, None),
            lambda: lib.hexl_ks_gen_keys(h, None, hx.KEY_FROM_SQUARE, 1, None, seed_ok, 0, 0),            # no secret
            lambda: lib.hexl_ks_gen_keys(h, S, hx.KEY_FROM_SQUARE, 1, None, None, 0, 0),                  # no seed
            lambda: lib.hexl_ks_gen_keys(h, S, hx.KEY_FROM_POLY, 1, None, seed_ok, 0, 0),                 # FROM_POLY without d_from
            lambda: lib.hexl_ks_gen_keys(h, S, 3, 1, Fp, seed_ok, 0, 0),                                  # unknown kinds
            lambda: lib.hexl_ks_gen_keys(h, S, -1, 1, Fp, seed_ok, 0, 0),
            lambda: lib.hexl_ks_gen_keys(h, S, hx.KEY_FROM_GALOIS, 4, None, seed_ok, 0, 0),               # even
            lambda: lib.hexl_ks_gen_keys(h, S, hx.KEY_FROM_GALOIS, 0, None, seed_ok, 0, 0),
            lambda: lib.hexl_ks_gen_keys(h, S, hx.KEY_FROM_GALOIS, 2 * n + 1, None, seed_ok, 0, 0),       # >= 2n
            lambda: lib.hexl_ks_gen_keys(h, S, hx.KEY_FROM_SQUARE, 1, None, seed_ok, 0, (1 << 40) - L + 1),   # first + L > 2^40
            lambda: lib.hexl_ks_gen_keys(h, S, hx.KEY_FROM_SQUARE, 1, None, seed_ok, 0, (1 << 64) - 1),
        ]

    # a plan that was only ever refused has no keys
    for k, call in enumerate(bad_calls(H)):
        assert call() == -1, f"refusal {k}"
    with pytest.raises(hx.HexlError, match="status -2"):
        plan.keyswitch(r.clone(), t, nb)
    # a keyed plan keeps its keys
    keyed.gen_relin_keys(s, seed=SEED, stream=3)
    before = r.clone()
    keyed.keyswitch(before, t, nb)
    for k, call in enumerate(bad_calls(keyed.h)):
        assert call() == -1, f"refusal {k} on a keyed plan"
    after = r.clone()
    keyed.keyswitch(after, t, nb)
    ctx.sync()
    assert torch.equal(before, after), "a refused call changed the keys"
    # accepted: first + L == 2^40
    plan.gen_relin_keys(s, seed=SEED, stream=3, first=(1 << 40) - L)
    ctx.sync()
    # a plan on the integer kernels: hexl_ks_gen_keys is out of scope, and leaves it keyless
    icase = KsCase(orc, n, 2, 3, seed=1, bits=55)
    (integer,) = make_plans(hx, ctx, icase, 1)
    assert integer.tiers()[0][0] == -1
    with pytest.raises(hx.HexlError, match="status -1"):
        integer.gen_relin_keys(s, seed=SEED)
    ti, ri = uniform_inputs(hx, dev, icase, nb)
    with pytest.raises(hx.HexlError, match="status -2"):
        integer.keyswitch(ri, ti, nb)
    for p in (plan, keyed, integer):
        p.close()


# ---------------------------------------------------------------------------------------------------------------- caller stream
def test_install_and_generate_are_ordered_on_a_caller_stream(hx, ctx, dev, orc, fill, closing):
    """behind a filler on a side stream set by hexl_ctx_set_stream (test_gpu_streams.py, part A): the key buffer / the secret and the
    keyswitch's operands are poison until copies queued on that stream replace them, the output is cloned on that stream, and the
    stream is the only thing waited for. Expected words: the oracle for the installed key; for the generated one a plan keyed by the
    composition on the session's context."""
    n, L, K, nb = 1024, 3, 4, 3
    side, s = side_context(hx, closing)
    case = KsCase(orc, n, L, K, seed=11)
    ins = [case.inputs(orc, b) for b in range(nb)]
    t, real_t = dev_pair(hx, dev, [i[0] for i in ins], nb)
    r, real_r = dev_pair(hx, dev, [i[1] for i in ins], nb)
    want = [case.expected(orc, *i) for i in ins]
    want_dev = hx.as_i64(np.concatenate(want)).to(dev)

    def check_against(w, label):
        def check(c):
            bad = int((c[0] != w).sum())
            assert bad == 0, f"{label}: {bad} words differ"
        return check

    # install
    plan = hx.KeySwitchPlan(side, n, L, K, K, 2, case.moduli, case.modswitch)
    closing.append(plan)
    d_keys, real_keys = dev_pair(hx, dev, [np.concatenate(case.keys)])

    def install():
        plan.set_keys_device(d_keys)
        plan.keyswitch(r, t, nb)

    label = "hexl_ks_set_keys_device -> hexl_keyswitch on a side stream"
    first_then_warm(Op(label, [(d_keys, real_keys), (t, real_t), (r, real_r)], [], [r], install, check_against(want_dev, label)), s, fill)

    # generate: the reference on the session's context (its own stream), synchronised before the side stream starts
    ref = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    closing.append(ref)
    sec, _ = secret_and_from(ref, dev, case)
    compose_keys(hx, ctx, ref, dev, case, sec, hx.KEY_FROM_SQUARE, 1, None, SEED, 6, 2)
    rr = real_r.clone()
    ref.keyswitch(rr, real_t, nb)
    ctx.sync()
    torch_().cuda.synchronize()
    d_s, real_s = torch_().zeros_like(sec), sec

    def generate():
        plan.gen_relin_keys(d_s, seed=SEED, stream=6, first=2)
        plan.keyswitch(r, t, nb)

    label = "hexl_ks_gen_keys -> hexl_keyswitch on a side stream"
    first_then_warm(Op(label, [(d_s, real_s), (t, real_t), (r, real_r)], [], [r], generate, check_against(rr, label)), s, fill)
