"""Host models of hexl_ct_tensor_sum, hexl_relinearize and hexl_multiply_sum_relinearize in Python integers, one instance each:
    out[0][i] = sum_t a_t[0][i] b_t[0][i],  out[1][i] = sum_t (a_t[0][i] b_t[1][i] + a_t[1][i] b_t[0][i]),  out[2][i] = sum_t a_t[1][i] b_t[1][i]
modulo q_i, with operand t laid out [2][in_limbs[t][.]][n] and read through its first n_limbs limbs; the key switch is the oracle's
(orc.keyswitch). Layouts are the library's."""
import numpy as np


def ct_tensor_sum(qs, n, a_s, b_s, n_limbs, in_limbs=None):
    """a_s, b_s: one instance of every operand, flat or [2][limbs][n]; in_limbs [n_terms][2] or None (all n_limbs) -> [3][n_limbs][n] uint64"""
    n_terms = len(a_s)
    assert n_terms >= 1 and len(b_s) == n_terms
    il = [[n_limbs, n_limbs]] * n_terms if in_limbs is None else [[int(v) for v in pair] for pair in in_limbs]
    assert all(la >= n_limbs and lb >= n_limbs for la, lb in il)
    A = [np.asarray(a, dtype=np.uint64).reshape(2, il[t][0], n).astype(object) for t, a in enumerate(a_s)]
    B = [np.asarray(b, dtype=np.uint64).reshape(2, il[t][1], n).astype(object) for t, b in enumerate(b_s)]
    out = np.empty((3, n_limbs, n), dtype=np.uint64)
    for i in range(n_limbs):
        q = int(qs[i])
        d = [np.zeros(n, dtype=object) for _ in range(3)]
        for a, b in zip(A, B):
            d[0] = d[0] + a[0, i] * b[0, i]
            d[1] = d[1] + a[0, i] * b[1, i] + a[1, i] * b[0, i]
            d[2] = d[2] + a[1, i] * b[1, i]
        for k in range(3):
            out[k, i] = np.array(d[k] % q, dtype=np.uint64)
    return out


def relinearize(orc, case, ct3):
    """ct3 [3][L][n] (flat or shaped) -> flat [2][L][n]: (c0, c1) + KeySwitch(c2) with case's keys"""
    n, L = case.n, case.L
    ct3 = np.ascontiguousarray(np.asarray(ct3, dtype=np.uint64).reshape(-1))
    out = ct3[:2 * L * n].copy()
    orc.keyswitch(out, ct3[2 * L * n:].copy(), n, L, case.K, case.rns, case.moduli, case.keys, case.modswitch, case.twiddles)
    return out


def multiply_sum_relinearize(orc, case, a_s, b_s, in_limbs=None):
    """the normative composition: ct_tensor_sum at n_limbs = L, then relinearize"""
    qs = [int(q) for q in case.moduli]
    return relinearize(orc, case, ct_tensor_sum(qs, case.n, a_s, b_s, case.L, in_limbs))
