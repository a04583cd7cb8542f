"""GPU: hexl_apply_galois against the permutation model (tests/ckks_model.py, checked against the oracle's transforms in
test_ckks_ops_model.py) and hexl_rotate against (perm(c0), 0) + orc.keyswitch(perm(c1)), every instance of every launch."""
import numpy as np
import pytest

from ckks_model import apply_galois, automorphism_coeff, rotate
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
    distinct = min(nb, 3)
    cts = [ct_of(orc, case, b) for b in range(distinct)]
    d_ct = hx.as_i64(np.concatenate([cts[b % distinct] for b in range(nb)])).to(dev)
    import torch
    d_out = torch.full((nb * 2 * L * n,), -1, dtype=torch.int64, device=dev)   # written, not accumulated into
    g = pow(5, 3, 2 * n)
    plan.rotate(d_out, d_ct, nb, g)
    ctx.sync()
    out = hx.to_u64(d_out).reshape(nb, -1)
    want = [rotate(orc, case, cts[b], g) for b in range(distinct)]
    for b in range(nb):
        assert np.array_equal(out[b], want[b % distinct]), f"instance {b}"
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
