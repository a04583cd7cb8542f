"""Synthetic keyswitch workloads: moduli = GeneratePrimes(K, 51, n) (< 2^52 as
host/src/keyswitch.cpp:32 requires), special prime = moduli[K-1],
modswitch_factors[i] = q_sp^-1 mod q_i, everything else uniform mod its limb (splitmix seeds)."""
import numpy as np


class KsCase:
    def __init__(self, orc, n, L, K, seed=1, bits=51, with_twiddles=False, moduli=None, extreme_keys=False):
        self.n, self.L, self.K, self.rns = n, L, K, L + 1
        self.moduli = np.array(orc.primes(K, bits, n) if moduli is None else moduli, dtype=np.uint64)
        q_sp = int(self.moduli[K - 1])
        self.modswitch = np.array([orc.orc().orc_invmod(q_sp % int(q), int(q)) if i < K - 1 else 1
                                   for i, q in enumerate(self.moduli)], dtype=np.uint64)
        self.keys = []
        for d in range(L):
            k = np.empty(2 * K * n, dtype=np.uint64)
            for kk in range(2):
                for i in range(K):
                    k[(kk * K + i) * n:(kk * K + i + 1) * n] = (
                        extreme_words(n, int(self.moduli[i]), d + kk + i) if extreme_keys else
                        orc.splitmix(n, seed * 7919 + d * 131 + kk * 17 + i, int(self.moduli[i])))
            self.keys.append(k)
        self.twiddles = None
        if with_twiddles:
            tw = np.zeros(K * 4 * n, dtype=np.uint64)
            for i in range(K):
                q = int(self.moduli[i])
                orc.orc().orc_tables_keyswitch(n, q, orc.orc().orc_minimal_primitive_root(2 * n, q),
                                               orc.p(tw[i * 4 * n:(i + 1) * 4 * n]))
            self.twiddles = tw
        self.seed = seed

    def inputs(self, orc, b):
        n, L = self.n, self.L
        t = np.concatenate([orc.splitmix(n, self.seed * 104729 + b * 64 + d, int(self.moduli[d])) for d in range(L)])
        r = np.concatenate([orc.splitmix(n, self.seed * 15485863 + b * 64 + k * 32 + i, int(self.moduli[i]))
                            for k in range(2) for i in range(L)])
        return t, r

    def extreme_inputs(self, orc, b):
        """instance b of a worst-case family: every word at an end of the residue range or beside its middle (the largest
        magnitudes of the centred representation the FP64 kernels compute in), in runs and alternations that line signs up"""
        n, L = self.n, self.L
        t = np.concatenate([extreme_words(n, int(self.moduli[d]), b * 5 + d) for d in range(L)])
        r = np.concatenate([extreme_words(n, int(self.moduli[i]), b * 7 + k * 3 + i + 1) for k in range(2) for i in range(L)])
        return t, r

    def expected(self, orc, t, r):
        out = r.copy()
        orc.keyswitch(out, t, self.n, self.L, self.K, self.rns, self.moduli, self.keys, self.modswitch, self.twiddles)
        return out


def extreme_words(n, q, which):
    """n words below q from {q - 1, (q - 1) / 2, (q + 1) / 2, 0, 1} -- constant, alternating, in halves or in runs of 16"""
    lo, hi, top = (q - 1) // 2, (q + 1) // 2, q - 1
    j = np.arange(n)
    pats = [np.full(n, top), np.full(n, lo), np.full(n, hi), np.where(j & 1, hi, lo), np.where(j < n // 2, lo, hi),
            np.where(j & 1, top, 1), np.where((j >> 4) & 1, hi, top), np.where(j & 2, lo, top), np.where(j & 1, 0, hi)]
    return pats[which % len(pats)].astype(np.uint64)


def primes_below(orc, count, limit, n):
    """the `count` largest primes p < limit with p = 1 (mod 2n), descending"""
    out, v = [], (limit - 2) // (2 * n) * (2 * n) + 1
    while len(out) < count:
        if v < limit and orc.orc().orc_is_prime(v):
            out.append(v)
        v -= 2 * n
    return out


def primes_from(orc, count, start, n):
    """the `count` smallest primes p >= start with p = 1 (mod 2n), ascending"""
    out, v = [], (start + 2 * n - 2) // (2 * n) * (2 * n) + 1
    while len(out) < count:
        if orc.orc().orc_is_prime(v):
            out.append(v)
        v += 2 * n
    return out


def seal_chain(orc, K, n):
    """K key moduli shaped like bridge-seal's run (experimental/bridge-seal/tests/seal_test.sh:20: CoeffModulus::Create(16384,
    {52, 30, 30, 40, 27, 27, 27}), SEAL picks the LARGEST primes = 1 mod 2n below each 2^bits): a 52-bit first limb (strict FP64 tier)
    followed by 30 / 30 / 40 / 27 / 27 / 27-bit ones (reduction period 12), the last one being the special prime"""
    bits = [52, 30, 30, 40, 27, 27, 27]
    bits = (bits + bits[1:] * 3)[:K]
    out = []
    for b in bits:
        k = 1 + sum(1 for v in out if v < (1 << b) and v > (1 << (b - 1)))          # the next-largest prime of that size not used yet
        out.append(primes_below(orc, k, 1 << b, n)[k - 1])
    return out


def tier_ladder(orc, K, n):
    """K distinct key moduli that walk through all four FP64 tiers (strict, period 3, 6, 12): the largest unused primes below
    2^52, 2^51, 2^50, 2^49, 2^44, 2^50, ...; the special prime (last) is a 49-bit one"""
    out = []
    for b in ([52, 51, 50, 49, 44, 50, 51, 52] * 2)[:K - 1] + [49]:
        k = 1
        while primes_below(orc, k, 1 << b, n)[k - 1] in out:
            k += 1
        out.append(primes_below(orc, k, 1 << b, n)[k - 1])
    return out


def big_dropped(orc, n):
    """K = 4, used with n_limbs = 3: the rescale drops the largest prime below 2^52 beside two 30-bit limbs (the quotient inside
    reduce(s + fix_i) has 22 bits); the special prime is a 27-bit one"""
    return primes_below(orc, 2, 1 << 30, n) + primes_below(orc, 1, 1 << 52, n) + primes_below(orc, 1, 1 << 27, n)


def small_dropped(orc, n):
    """the reverse, K = 4 with n_limbs = 3: a 27-bit prime dropped beside the largest primes below 2^52 and 2^51; special prime 27-bit"""
    small = primes_below(orc, 2, 1 << 27, n)
    return primes_below(orc, 1, 1 << 52, n) + primes_below(orc, 1, 1 << 51, n) + small


def rounding_edge_coeffs(n, q, which):
    """n COEFFICIENT-domain words from {0, 1, half - 1, half, half + 1, half + 2, q - 2, q - 1}, half = q >> 1: as the INTT of a
    rescale's dropped limb they put s = (x + half) mod q on every point where round(X / q) changes or wraps. Constant, alternating,
    in runs of 8, or a walk through all eight values whose stride depends on `which`."""
    half = q >> 1
    vals = np.array([0, 1, half - 1, half, half + 1, half + 2, q - 2, q - 1], dtype=np.uint64)
    j = np.arange(n)
    kind, v = which % 4, which // 4
    idx = [np.full(n, v), np.where(j & 1, v + 3, v), (j >> 3) + v, j * (2 * v + 1) + (j >> 5) * 3 + v][kind] % 8
    return vals[idx]


def extreme_ciphertext(case, b, components, limbs=None, salt=0):
    """instance b of the [k][i][n] layout hexl_rescale and hexl_multiply_relinearize take, every word from extreme_words with the
    pattern varied per (b, k, i); operands that meet in one call take salts that differ by a non-multiple of 9 (the pattern count)"""
    limbs = case.L if limbs is None else limbs
    return np.concatenate([extreme_words(case.n, int(case.moduli[i]), salt + b * 5 + k * 3 + i)
                           for k in range(components) for i in range(limbs)])


# The arithmetic tiers of the FP64 kernels as (environment of the child process, expression for the key moduli; "None" = the bench's
# 51-bit primes): shared by test_gpu_keyswitch.py (every pipeline) and test_gpu_mulrelin.py (the fused multiply).
TIERS = {
    "skip_period3_51bit": ({}, "None"),
    "noskip_forced_period3_51bit": ({"HEXL_KSX_SKIP": "0"}, "None"),
    "skip_period3_ratio_1p24": ({}, "[orc.primes(1, 51, n)[0]] + primes_below(orc, K - 1, int(0.81 * 2**51), n)"),
    "skip_period3_special_prime_smallest": ({}, "orc.primes(K - 1, 51, n) + primes_below(orc, 1, int(0.81 * 2**51), n)"),
    "skip_period6_just_below_2^50": ({}, "primes_below(orc, K, 1 << 50, n)"),
    "skip_period12_just_below_2^49": ({}, "primes_below(orc, K, 1 << 49, n)"),
    "noskip_period6_mixed_50_to_40bit": ({}, "primes_below(orc, 2, 1 << 50, n) + orc.primes(K - 3, 40, n) + orc.primes(1, 45, n)"),
    "noskip_period3_mixed_51_and_30bit": ({}, "orc.primes(2, 51, n)[:1] + orc.primes(K - 2, 30, n) + orc.primes(2, 51, n)[1:]"),
    "strict_just_below_2^52": ({}, "primes_below(orc, K, 1 << 52, n)"),
    # round 6: both sides of the lazy / strict boundary 2^51 (1 + 2^-7) (f64_arith.hpp LAZY_MAX_MODULUS)
    "period3_tier_top_2^51_plus_2^44": ({}, "primes_below(orc, K, (1 << 51) + (1 << 44), n)"),
    "strict_just_above_2^51_plus_2^44": ({}, "primes_from(orc, K, (1 << 51) + (1 << 44), n)"),
    "strict_forced_51bit": ({"HEXL_KS_NOLAZY": "1"}, "None"),
    # round 5: plans whose limbs differ in tier -- every transform takes the tier of ITS modulus (hexl_ks_plan::tier; the reference's NTT
    # engines each run on their own modulus, device/keyswitch/ntt_core.hpp:285-291)
    "mixed_seal_chain_strict_and_period12": ({}, "seal_chain(orc, K, n)"),
    "mixed_seal_chain_plan_wide_tier": ({"HEXL_KS_PER_LIMB": "0"}, "seal_chain(orc, K, n)"),
    "mixed_special_prime_strict_rest_period12": ({}, "orc.primes(K - 1, 47, n) + primes_below(orc, 1, 1 << 52, n)"),
    "mixed_skip_period6_and_period3_around_2^50": ({}, "(primes_below(orc, K, 1 << 50, n) + orc.primes(K, 50, n))[K // 2:K // 2 + K]"),
    "mixed_all_four_tiers": ({}, "tier_ladder(orc, K, n)"),
}
# the tiers the worst-case operand families (extreme_words) run in
EXTREME_TIERS = ["skip_period3_51bit", "period3_tier_top_2^51_plus_2^44", "strict_just_above_2^51_plus_2^44", "skip_period6_just_below_2^50",
                 "skip_period12_just_below_2^49", "strict_just_below_2^52", "mixed_seal_chain_strict_and_period12", "mixed_all_four_tiers"]


def tier_moduli(orc, tier, n, K):
    """the key moduli of TIERS[tier] in this process (None: KsCase's default primes)"""
    return eval(TIERS[tier][1], {"orc": orc, "n": n, "K": K, "primes_below": primes_below, "primes_from": primes_from,
                                 "seal_chain": seal_chain, "tier_ladder": tier_ladder})


class RlweCase:
    """Real RLWE switching keys with special prime P = moduli[K-1]: key d, limb i holds (b, a) with
    b = -a*s_old + e + (i == d ? P : 0) * s_new in the NTT domain. check(res) asserts that
    res0 + res1*s_old == t*s_new + small noise in every limb and that the limbs agree on the noise polynomial -- what
    the reference's SEAL test asserts end to end (experimental/bridge-seal/tests/keyswitch-example.cpp:119-206)."""

    def __init__(self, orc, n, L, K, bits, seed=2):
        self.orc, self.n, self.L, self.K = orc, n, L, K
        self.qs = [int(v) for v in orc.primes(K, bits, n)]
        qs, P = self.qs, self.qs[K - 1]
        rng = np.random.default_rng(seed)
        self.s_old = rng.integers(-1, 2, n)
        self.s_new = rng.integers(-1, 2, n)
        self.blks = []
        for q in qs:
            b = np.zeros(4 * n, dtype=np.uint64)
            orc.orc().orc_tables_keyswitch(n, q, orc.orc().orc_minimal_primitive_root(2 * n, q), orc.p(b))
            self.blks.append(b)
        self.keys = []
        for d in range(L):
            e = rng.integers(-3, 4, n)
            key = np.zeros(2 * K * n, dtype=np.uint64)
            for i in range(K):
                a = self.ntt(rng.integers(0, 2**62, n).astype(object) % qs[i], i)
                b = (-a * self.ntt(self.s_old, i) + self.ntt(e, i) + (P % qs[i] if i == d else 0) * self.ntt(self.s_new, i)) % qs[i]
                key[(0 * K + i) * n:(0 * K + i + 1) * n] = np.array(b, dtype=np.uint64)
                key[(1 * K + i) * n:(1 * K + i + 1) * n] = np.array(a, dtype=np.uint64)
            self.keys.append(key)
        self.moduli = np.array(qs, dtype=np.uint64)
        self.modswitch = np.array([pow(P, -1, q) if q != P else 1 for q in qs], dtype=np.uint64)
        # the polynomial being switched, given in NTT form per limb (a consistent RNS element)
        t_int = rng.integers(0, 2**62, n).astype(object)
        self.t = np.concatenate([np.array(self.ntt(t_int % qs[d], d), dtype=np.uint64) for d in range(L)])

    def ntt(self, poly, i):
        n, q = self.n, self.qs[i]
        x = np.array([int(v) % q for v in poly], dtype=np.uint64)
        self.orc.orc().orc_ks_ntt(self.orc.p(x), n, q, self.orc.p(self.blks[i][2 * n:3 * n]))
        return x.astype(object)

    def intt(self, x, i):
        n, q = self.n, self.qs[i]
        y = np.array([int(v) % q for v in x], dtype=np.uint64)
        self.orc.orc().orc_ks_intt(self.orc.p(y), n, q, self.orc.p(self.blks[i][0:n]))
        return y.astype(object)

    def check(self, res, noise_bits=24):
        n, L, qs = self.n, self.L, self.qs
        noises = []
        for i in range(L):
            r0 = res[(0 * L + i) * n:(0 * L + i + 1) * n].astype(object)
            r1 = res[(1 * L + i) * n:(1 * L + i + 1) * n].astype(object)
            lhs = (r0 + r1 * self.ntt(self.s_old, i) - self.t[i * n:(i + 1) * n].astype(object) * self.ntt(self.s_new, i)) % qs[i]
            diff = self.intt(lhs, i)
            centered = np.array([int(v) if v <= qs[i] // 2 else int(v) - qs[i] for v in diff], dtype=object)
            noises.append(centered)
            assert max(abs(int(v)) for v in centered) < 1 << noise_bits, "keyswitch noise too large in limb %d" % i
        for i in range(1, L):
            assert (noises[i] == noises[0]).all(), "limbs disagree on the noise polynomial"
