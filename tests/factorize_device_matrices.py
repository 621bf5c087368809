"""Unsymmetric matrices for the tests of the factorization from device values (tests/test_factorize_device_api.py without a
GPU, tests/factorize_device_cases.py with one), and the product A*A' restated in numpy from a product map.  No torch here."""
import math
import os

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53


def afiro():
    """tests/golden/demo/lp_afiro.tri: 27 x 51, 102 entries"""
    from matrix_files import read_file
    m = read_file(os.path.join(HERE, "golden", "demo", "lp_afiro.tri"))
    assert m["kind"] == "sparse" and m["stype"] == 0
    M = sp.csc_matrix((np.asarray(m["Ax"], dtype=np.float64), np.asarray(m["Ai"]), np.asarray(m["Ap"])), shape=(m["nrow"], m["ncol"]))
    M.sort_indices()
    return M


def engineered():
    """70 rows, 133 columns, every list length class of the product kernel:
      column 0          dense: every pair of rows shares it (lists of 1 .. 3 pairs for most of A*A');
      columns 1 .. 40   rows {0, 1}: entries (1,0) and (1,1) of A*A' have lists of 41 pairs;
      columns 41 .. 130 rows {0, 2 + (k - 41) % 68}: with the above, 130 two-entry columns, and row 0 lies in 131
                        columns: entry (0,0) has a list of 131 pairs;
      column 131        a single entry (row 5); column 132 empty.
    The values are of mixed sign, 0.5 <= |a| < 2: A*A' is then positive definite with a condition number below 1000
    (833), so that a last-bit difference in its entries (the device sums them in another order than the host)
    amplified by that stays below the 1e-12 the factors are compared at."""
    m = 70
    rows, cols = list(range(m)), [0] * m
    for k in range(1, 41):
        rows += [0, 1]
        cols += [k, k]
    for k in range(41, 131):
        rows += [0, 2 + (k - 41) % 68]
        cols += [k, k]
    rows.append(5)
    cols.append(131)
    rng = np.random.default_rng(70)
    vals = rng.uniform(0.5, 2.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    M = sp.csc_matrix((vals, (rows, cols)), shape=(m, 133))
    M.sort_indices()
    assert M.nnz == len(rows)
    return M


def one_by_one():
    return sp.csc_matrix(np.array([[2.5]]))


def symbolic_tril_aat(M):
    """(Cp, Ci) of tril (A*A') as a pattern: every position two rows of A share a column at, columns sorted"""
    B = sp.csc_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    Cs = sp.tril(B @ B.T, format="csc")
    Cs.sort_indices()
    return Cs.indptr.astype(np.int64), Cs.indices.astype(np.int64)


def exact_products(M, Cp, Ci):
    """per entry of tril (A*A'), from the dense A: (the sum of the exactly formed products, rounded once -- what math.fsum
    gives over exact terms; the products of two doubles are exact as fractions --, the sum of their absolute values, the
    number of terms)"""
    from fractions import Fraction
    D = M.toarray()
    ref, mag, cnt = np.zeros(len(Ci)), np.zeros(len(Ci)), np.zeros(len(Ci), dtype=np.int64)
    for j in range(M.shape[0]):
        for c in range(Cp[j], Cp[j + 1]):
            i = Ci[c]
            ks = np.nonzero((D[i] != 0) & (D[j] != 0))[0]
            terms = [Fraction(float(D[i, k])) * Fraction(float(D[j, k])) for k in ks]
            ref[c] = float(sum(terms, Fraction(0)))
            mag[c] = math.fsum(abs(float(D[i, k])) * abs(float(D[j, k])) for k in ks)
            cnt[c] = len(ks)
    return ref, mag, cnt
