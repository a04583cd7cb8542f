"""Host model of hexl_linear_transform in exact integers on hoist_model.mod_up / ckks_model.Limbs' transforms:

    u[d][slot]   = the keyswitch's mod-up of c1 (hoist_model.mod_up), slot = the L data limbs and the special prime
    acc[k][slot] = sum_r pt_r[slot] . ( sum_d sigma_{g_r}(u[d][slot]) . key_r[d][k][slot] )            mod q_slot
    s'_k         = (INTT_sp(acc[k][sp]) + floor(q_sp / 2)) mod q_sp
    out[0][i]    = sum_r pt_r[i] . sigma_{g_r}(c0[i]) + pt_id[i] . c0[i] + (acc[0][i] - NTT_i((s'_0 + fix_i) mod q_i)) . msf_i
    out[1][i]    =                                      pt_id[i] . c1[i] + (acc[1][i] - NTT_i((s'_1 + fix_i) mod q_i)) . msf_i

pt_r is [L + 1][n]: rows 0 ... L - 1 modulo the data limbs, row L modulo the special prime. With one rotation and an all-ones plaintext
this is hoist_model.rotate_hoisted word for word; in general it is NOT the composition rotate_hoisted -> multiply -> add
(`composition` below), which rounds by q_sp once per rotation (include/hexl_mi355x.h)."""
import numpy as np

from ckks_model import apply_galois
from hoist_model import limbs_of, mod_up, rotate_hoisted


def linear_transform(orc, cases, gs, pts, pt_id, ct, lm=None, u=None):
    """ct[2][L][n] -> out[2][L][n] (flat uint64), the words hexl_linear_transform writes for the keys of cases[r], Galois elements gs[r]
    and plaintexts pts[r] ([L + 1][n] uint64); pt_id: [L][n] or None. `lm` and `u` (mod_up of the same ct) may be shared."""
    case = cases[0]
    n, L, K = case.n, case.L, case.K
    lm = lm or limbs_of(orc, case)
    u = u or mod_up(lm, case, ct)
    c = np.asarray(ct, dtype=np.uint64).reshape(2, L, n)
    pts = [np.asarray(p, dtype=np.uint64).reshape(L + 1, n).astype(object) for p in pts]
    pid = None if pt_id is None else np.asarray(pt_id, dtype=np.uint64).reshape(L, n).astype(object)
    slots = list(range(L)) + [K - 1]
    q_sp, half = lm.qs[K - 1], lm.qs[K - 1] >> 1
    rot_u = [[[apply_galois(u[d][si], n, g) for si in range(L + 1)] for d in range(L)] for g in gs]
    out = np.empty((2, L, n), dtype=np.uint64)
    for k in range(2):
        acc = []
        for si, i in enumerate(slots):
            q = lm.qs[i]
            total = np.zeros(n, dtype=object)
            for r, kc in enumerate(cases):
                inner = np.zeros(n, dtype=object)
                for d in range(L):
                    inner = inner + rot_u[r][d][si] * kc.keys[d][(k * K + i) * n:(k * K + i + 1) * n].astype(object)
                total = total + pts[r][si] * (inner % q)
            acc.append(total % q)
        s = (lm.intt(np.array(acc[L], dtype=np.uint64), K - 1).astype(object) + half) % q_sp
        for i in range(L):
            qi = lm.qs[i]
            fix = qi - half % qi
            w = lm.ntt(np.array((s + fix) % qi, dtype=np.uint64), i).astype(object)
            first = np.zeros(n, dtype=object)
            if k == 0:
                for r, g in enumerate(gs):
                    first = first + pts[r][i] * apply_galois(c[0, i], n, g).astype(object)
            if pid is not None:
                first = first + pid[i] * c[k, i].astype(object)
            out[k, i] = np.array((first + (acc[i] - w) * int(case.modswitch[i])) % qi, dtype=np.uint64)
    return out.reshape(-1)


def composition(orc, cases, gs, pts, pt_id, ct, lm=None, u=None):
    """the three-call route in the same exact integers: rotate_hoisted per rotation, times the plaintext's data-limb rows, summed"""
    case = cases[0]
    n, L = case.n, case.L
    lm = lm or limbs_of(orc, case)
    u = u or mod_up(lm, case, ct)
    total = np.zeros((2, L, n), dtype=object)
    for kc, g, pt in zip(cases, gs, pts):
        rot = rotate_hoisted(orc, kc, ct, g, lm, u).reshape(2, L, n).astype(object)
        total = total + rot * np.asarray(pt, dtype=np.uint64).reshape(L + 1, n)[:L].astype(object)[None]
    if pt_id is not None:
        total = total + np.asarray(ct, dtype=np.uint64).reshape(2, L, n).astype(object) * np.asarray(pt_id, dtype=np.uint64).reshape(L, n).astype(object)[None]
    q = np.array([lm.qs[i] for i in range(L)], dtype=object).reshape(1, L, 1)
    return np.array(total % q, dtype=np.uint64).reshape(-1)


def ones_plaintext(case):
    return np.ones((case.L + 1) * case.n, dtype=np.uint64)


def uniform_plaintext(orc, case, seed, rows=None):
    """[rows][n] uniform words, row i below q_i and row L (of L + 1) below the special prime"""
    n, L, K = case.n, case.L, case.K
    limbs = (list(range(L)) + [K - 1])[:L + 1 if rows is None else rows]
    return np.concatenate([orc.splitmix(n, 7000 + seed * 131 + i, int(case.moduli[i])) for i in limbs])


def sparse_plaintext(rc, coeffs, rows=None):
    """a signed polynomial given as {exponent: coefficient}, in NTT form: [L + 1][n] (or the first `rows` rows) on the transforms of an
    RlweCase, row L modulo the special prime"""
    poly = np.zeros(rc.n, dtype=object)
    for e, v in coeffs.items():
        poly[e] = v
    limbs = (list(range(rc.L)) + [rc.K - 1])[:rc.L + 1 if rows is None else rows]
    return np.concatenate([np.array(rc.ntt(poly, i), dtype=np.uint64) for i in limbs])


def negacyclic_sparse(coeffs, poly, n):
    """(sum_e coeffs[e] X^e) . poly mod X^n + 1 over the integers; poly a signed object array"""
    out = np.zeros(n, dtype=object)
    for e, v in coeffs.items():
        out = out + v * np.concatenate([-poly[n - e:], poly[:n - e]])
    return out


def check_decrypts(gr_list, coeffs_list, id_coeffs, out, noise_bits=24):
    """out[2][L][n] decrypts under s to sum_r pt_r . sigma_{g_r}(m) + pt_id . m + noise with |noise| < (sum ||pt||_1) 2^noise_bits --
    GaloisRlwe.check's bound for one rotation, carried through a negacyclic product (factor ||pt_r||_1) and the sum -- and every limb
    sees the same noise polynomial. gr_list: GaloisRlwe objects over one RlweCase with one message; the first one's message is used."""
    gr0 = gr_list[0]
    rc, n, L = gr0.rc, gr0.n, gr0.L
    out = np.asarray(out, dtype=np.uint64).reshape(2, L, n)
    want = np.zeros(n, dtype=object)
    l1 = 0
    for gr, coeffs in zip(gr_list, coeffs_list):
        want = want + negacyclic_sparse(coeffs, gr.sigma_signed(gr0.m), n)
        l1 += sum(abs(v) for v in coeffs.values())
    if id_coeffs is not None:
        want = want + negacyclic_sparse(id_coeffs, np.array([int(v) for v in gr0.m], dtype=object), n)
        l1 += sum(abs(v) for v in id_coeffs.values())
    assert l1 << 30 < min(rc.qs[:L]) // 4, "the plaintexts leave no room for the message below q / 4"
    bound = l1 << noise_bits
    noises = []
    for i in range(L):
        q = rc.qs[i]
        dec = rc.intt((out[0, i].astype(object) + out[1, i].astype(object) * gr0.s_ntt[i]) % q, i)
        centred = np.array([int(v) if v <= q // 2 else int(v) - q for v in dec], dtype=object)
        noise = centred - want
        assert max(abs(int(v)) for v in noise) < bound, f"limb {i}: does not decrypt to the weighted sum of rotations"
        noises.append(noise)
    for i in range(1, L):
        assert (noises[i] == noises[0]).all(), "limbs disagree on the noise polynomial"
    return max(abs(int(v)) for v in noises[0]), bound
