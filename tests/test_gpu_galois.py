"""GPU: hexl_apply_galois against the permutation model (tests/ckks_model.py, checked against the oracle's transforms in
test_ckks_ops_model.py) and hexl_rotate against (perm(c0), 0) + orc.keyswitch(perm(c1)), every instance of every launch."""
import numpy as np
import pytest

from ckks_model import apply_galois, automorphism_coeff, first_mismatch, rotate
from ks_util import KsCase, RlweCase, primes_below, seal_chain, tier_ladder

pytestmark = pytest.mark.gpu


def galois_elts(n):
    return [1, 3, 5, pow(5, 7, 2 * n), 2 * n - 1]


@pytest.mark.parametrize("n", [1024, 2048, 4096, 8192, 16384, 32768])
def test_apply_galois_matches_the_permutation(hx, ctx, dev, orc, n):
    import torch
    count = 5
    x = orc.splitmix(count * n, 7 + n)                                 # arbitrary 64-bit words: moved, never interpreted
    d_in = hx.as_i64(x).to(dev)
    d_out = torch.full((count * n,), -1, dtype=torch.int64, device=dev)
    for g in galois_elts(n):
        ctx.apply_galois(d_out, d_in, count, n, g)
        ctx.sync()
        assert np.array_equal(hx.to_u64(d_out), apply_galois(x, n, g)), f"g = {g}"


def test_apply_galois_many_polynomials(hx, ctx, dev, orc):
    """more polynomials than the launch has workgroups: the grid-stride loop"""
    n, count = 1024, 70000
    x = np.tile(orc.splitmix(3 * n, 99), count // 3 + 1)[:count * n]
    import torch
    d_out = torch.zeros(count * n, dtype=torch.int64, device=dev)
    ctx.apply_galois(d_out, hx.as_i64(x).to(dev), count, n, 5)
    ctx.sync()
    assert np.array_equal(hx.to_u64(d_out), apply_galois(x, n, 5))


def test_apply_galois_rejections(hx, ctx, dev):
    import torch
    n = 4096
    buf = torch.zeros(4 * n, dtype=torch.int64, device=dev)
    a, b = buf[:2 * n], buf[2 * n:]
    for nn, g in ((n, 2), (n, 2 * n + 1), (n, 4 * n - 1), (512, 3), (3000, 3), (65536, 3)):
        with pytest.raises(hx.HexlError):
            ctx.apply_galois(b, a, 1, nn, g)
    with pytest.raises(hx.HexlError):
        ctx.apply_galois(buf[n:3 * n], a, 2, n, 3)                     # overlap
    with pytest.raises(hx.HexlError):
        ctx.apply_galois(a, a, 2, n, 3)                                # in place
    ctx.apply_galois(b, a, 2, n, 3)                                    # adjacent: accepted
    ctx.sync()


def ct_of(orc, case, b):
    n, L = case.n, case.L
    return np.concatenate([orc.splitmix(n, case.seed * 31 + b * 977 + k * 17 + i, int(case.moduli[i]))
                           for k in range(2) for i in range(L)])


@pytest.mark.parametrize("n,L,K,nb,kind", [(16384, 6, 7, 2, "gen"), (16384, 6, 7, 40, "seal"), (16384, 3, 4, 260, "gen"),
                                           (8192, 3, 4, 5, "strict"), (4096, 3, 4, 4, "ladder"), (1024, 2, 3, 4100, "gen"),
                                           (32768, 2, 3, 130, "gen"), (4096, 2, 3, 3, "int")])
def test_rotate_vs_oracle(hx, ctx, dev, orc, n, L, K, nb, kind):
    moduli = {"strict": lambda: primes_below(orc, K, 1 << 52, n), "seal": lambda: seal_chain(orc, K, n),
              "ladder": lambda: tier_ladder(orc, K, n)}.get(kind, lambda: None)()
    case = KsCase(orc, n, L, K, seed=60 + L, moduli=moduli, bits=55 if kind == "int" else 51)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    if kind == "int":
        assert plan.tiers()[0][0] == -1
    plan.set_keys(case.keys)
    g = pow(5, 3, 2 * n)
    check_rotate(hx, ctx, dev, orc, case, plan, nb, g, min(nb, 3))
    plan.close()


def rotate_buffers(hx, dev, cts, nb):
    """device input of nb instances (the distinct ones in `cts`, repeated) and an output filled with -1 (written, not accumulated into)"""
    import torch
    d_ct = hx.as_i64(np.concatenate([cts[b % len(cts)] for b in range(nb)])).to(dev)
    return torch.full((nb * len(cts[0]),), -1, dtype=torch.int64, device=dev), d_ct


def assert_rotated(hx, orc, case, d_out, cts, nb, g, label=""):
    out = hx.to_u64(d_out).reshape(nb, -1)
    want = [rotate(orc, case, ct, g) for ct in cts]
    for b in range(nb):
        if not np.array_equal(out[b], want[b % len(cts)]):
            where = first_mismatch(out[b], want[b % len(cts)], ("component", "limb", "coefficient"), (2, case.L, case.n))
            raise AssertionError(f"{label}instance {b} of {nb}, {where}")


def check_rotate(hx, ctx, dev, orc, case, plan, nb, g, distinct):
    cts = [ct_of(orc, case, b) for b in range(distinct)]
    d_out, d_ct = rotate_buffers(hx, dev, cts, nb)
    plan.rotate(d_out, d_ct, nb, g)
    ctx.sync()
    assert_rotated(hx, orc, case, d_out, cts, nb, g)


def slice_of(plan):
    """instances per slice of hexl_rotate = per scratch chunk of the keyswitch, read off hexl_ks_scratch_bytes (bytes grow with the batch
    up to one chunk, DESIGN section 3: 256 at N = 16384, the same number of coefficients at the other ring dimensions)"""
    chunk = plan.scratch_bytes(1 << 24) // plan.scratch_bytes(1)
    assert chunk >= 2 and plan.scratch_bytes(chunk) == plan.scratch_bytes(chunk + 1) > plan.scratch_bytes(chunk - 1)
    return chunk


@pytest.mark.parametrize("which", ["identity", "conjugation", "5^3"])
@pytest.mark.parametrize("n", [4096, 32768])
def test_rotate_at_the_ends_of_the_galois_group(hx, ctx, dev, orc, n, which):
    """g = 1 and g = 2n - 1 through the rotate's own branch of k_galois (component 1 gathered into the plan's t buffer, zeros into the
    output), on the LDS gather (n <= 16384) and on the global one (n = 32768)"""
    g = {"identity": 1, "conjugation": 2 * n - 1, "5^3": pow(5, 3, 2 * n)}[which]
    L, K = 2, 3
    case = KsCase(orc, n, L, K, seed=71)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    check_rotate(hx, ctx, dev, orc, case, plan, 3, g, 3)
    plan.close()


@pytest.mark.parametrize("kernels", ["fp64", "integer"])
def test_rotate_two_full_slices(hx, ctx, dev, orc, kernels):
    """2 x slice + 1 instances: the second slice's gather overwrites EVERY row of the t buffer the first slice's keyswitch reads. The
    distinct instances do not divide the slice, so row r of the second slice differs from row r of the first: a gather that ran before
    the keyswitch had read t would change the first slice's result. An FP64 plan runs a slice on the caller's stream alone; a plan on
    the integer kernels (moduli above 2^52) splits it over two lanes, and hx_launch_rotate then relies on hx_launch_keyswitch having
    joined them back into the stream."""
    n, L, K = 4096, 2, 3
    case = KsCase(orc, n, L, K, seed=72, bits=55 if kernels == "integer" else 51)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    assert (plan.tiers()[0][0] == -1) == (kernels == "integer")
    plan.set_keys(case.keys)
    chunk = slice_of(plan)
    distinct = 3 if chunk % 3 else 5
    assert chunk % distinct
    check_rotate(hx, ctx, dev, orc, case, plan, 2 * chunk + 1, pow(5, 3, 2 * n), distinct)
    plan.close()


def test_rotate_one_plan_growing_batch(hx, ctx, dev, orc):
    """one instance, then more than a slice, then three, on one plan and with nothing but stream order between the calls: the plan's t
    buffer is replaced (grow-only) while the first call is queued, and the third call runs in the larger one"""
    n, L, K = 4096, 1, 2
    case = KsCase(orc, n, L, K, seed=73)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    plan.set_keys(case.keys)
    chunk = slice_of(plan)
    cts = [ct_of(orc, case, b) for b in range(3)]
    g = pow(5, 5, 2 * n)
    calls = [(1, cts[2:]), (chunk + 2, cts), (3, cts[::-1])]
    bufs = [rotate_buffers(hx, dev, c, nb) for nb, c in calls]    # every upload first: a copy from host memory waits for the stream
    ctx.sync()
    for (nb, _), (d_out, d_ct) in zip(calls, bufs):
        plan.rotate(d_out, d_ct, nb, g)
    ctx.sync()
    for (nb, c), (d_out, _) in zip(calls, bufs):
        assert_rotated(hx, orc, case, d_out, c, nb, g, label=f"call with {nb}: ")
    plan.close()


def test_rotate_rejections(hx, ctx, dev, orc):
    import torch
    n, L, K = 4096, 2, 3
    case = KsCase(orc, n, L, K, seed=5)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, case.moduli, case.modswitch)
    buf = torch.zeros(3 * 2 * L * n, dtype=torch.int64, device=dev)
    a, b = buf[:2 * L * n], buf[2 * L * n:4 * L * n]
    with pytest.raises(hx.HexlError, match="status -2"):               # HEXL_E_NOKEYS
        plan.rotate(b, a, 1, 3)
    plan.set_keys(case.keys)
    for g in (4, 2 * n + 1):
        with pytest.raises(hx.HexlError, match="status -1"):
            plan.rotate(b, a, 1, g)
    with pytest.raises(hx.HexlError, match="status -1"):
        plan.rotate(buf[L * n:3 * L * n], a, 1, 3)                      # overlap
    plan.rotate(b, a, 1, 3)
    ctx.sync()
    plan.close()


def test_rotate_rlwe_decrypts_to_the_rotated_message(hx, ctx, dev, orc):
    """a real Galois key (RlweCase's construction with s_new = sigma_g(s), s_old = s): encrypt m under s, rotate, decrypt with
    s -> sigma_g(m) up to small noise, the same noise polynomial in every limb"""
    n, L, K, g = 4096, 3, 4, 5
    rc = RlweCase(orc, n, L, K, 50, seed=4)
    qs, P = rc.qs, rc.qs[K - 1]
    rng = np.random.default_rng(9)
    s = rc.s_old
    s_rot = np.zeros(n, dtype=object)
    e_idx = (np.arange(n) * g) % (2 * n)
    for k in range(n):
        s_rot[e_idx[k] % n] = -int(s[k]) if e_idx[k] >= n else int(s[k])
    keys = []
    for d in range(L):
        e = rng.integers(-3, 4, n)
        key = np.zeros(2 * K * n, dtype=np.uint64)
        for i in range(K):
            a = rc.ntt(rng.integers(0, 2**62, n).astype(object) % qs[i], i)
            b = (-a * rc.ntt(s, i) + rc.ntt(e, i) + (P % qs[i] if i == d else 0) * rc.ntt(s_rot, i)) % qs[i]
            key[i * n:(i + 1) * n] = np.array(b, dtype=np.uint64)
            key[(K + i) * n:(K + i + 1) * n] = np.array(a, dtype=np.uint64)
        keys.append(key)
    m = rng.integers(-2**30, 2**30, n)
    e = rng.integers(-3, 4, n)
    a_int = rng.integers(0, 2**62, n).astype(object)
    c0, c1 = [], []
    for i in range(L):
        a = rc.ntt(a_int % qs[i], i)
        c1.append(np.array(a, dtype=np.uint64))
        c0.append(np.array((-a * rc.ntt(s, i) + rc.ntt(e, i) + rc.ntt(m, i)) % qs[i], dtype=np.uint64))
    ct = np.concatenate(c0 + c1)
    plan = hx.KeySwitchPlan(ctx, n, L, K, K, 2, rc.moduli, rc.modswitch)
    plan.set_keys(keys)
    import torch
    d_out = torch.zeros(2 * L * n, dtype=torch.int64, device=dev)
    plan.rotate(d_out, hx.as_i64(ct).to(dev), 1, g)
    ctx.sync()
    out = hx.to_u64(d_out)
    m_rot = [int(v) for v in automorphism_coeff(np.array([v % (1 << 62) for v in m], dtype=np.uint64), n, g, 1 << 62)]
    m_rot = np.array([v - (1 << 62) if v >= 1 << 61 else v for v in m_rot], dtype=object)
    noises = []
    for i in range(L):
        r0 = out[i * n:(i + 1) * n].astype(object)
        r1 = out[(L + i) * n:(L + i + 1) * n].astype(object)
        dec = rc.intt((r0 + r1 * rc.ntt(s, i)) % qs[i], i)
        centred = np.array([int(v) if v <= qs[i] // 2 else int(v) - qs[i] for v in dec], dtype=object)
        noise = centred - m_rot
        assert max(abs(int(v)) for v in noise) < 1 << 24, f"limb {i}: decryption is not sigma_g(m)"
        noises.append(noise)
    for i in range(1, L):
        assert (noises[i] == noises[0]).all(), "limbs disagree on the noise polynomial"
    plan.close()
