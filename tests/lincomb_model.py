"""Host model of hexl_ct_lincomb in Python integers: one instance of
    out[k][i][j] = ( sum_t w[t][i] ct_t[k][i][j] + [k == 0] (pt[i][j] + const[i]) ) mod q_i
with term t laid out [n_components][in_limbs[t]][n] and read through its first n_limbs limbs. Layouts are the library's."""
import numpy as np


def ct_lincomb(qs, n, cts, n_components, n_limbs, weights=None, in_limbs=None, pt=None, const=None):
    """cts: one instance of every term, term t flat or [n_components][in_limbs[t]][n]; weights [n_terms][n_limbs] residues or None (all 1);
    in_limbs [n_terms] or None (all n_limbs); pt [n_limbs][n] or None; const [n_limbs] or None -> [n_components][n_limbs][n] uint64"""
    n_terms = len(cts)
    il = [n_limbs] * n_terms if in_limbs is None else [int(v) for v in in_limbs]
    assert n_terms >= 1 and all(v >= n_limbs for v in il)
    terms = [np.asarray(c, dtype=np.uint64).reshape(n_components, il[t], n).astype(object) for t, c in enumerate(cts)]
    out = np.empty((n_components, n_limbs, n), dtype=np.uint64)
    for k in range(n_components):
        for i in range(n_limbs):
            q = int(qs[i])
            v = np.zeros(n, dtype=object)
            for t in range(n_terms):
                w = 1 if weights is None else int(weights[t][i])
                assert 0 <= w < q
                v = v + w * terms[t][k, i]
            if k == 0 and pt is not None:
                v = v + np.asarray(pt, dtype=np.uint64).reshape(n_limbs, n)[i].astype(object)
            if k == 0 and const is not None:
                assert 0 <= int(const[i]) < q
                v = v + int(const[i])
            out[k, i] = np.array(v % q, dtype=np.uint64)
    return out
