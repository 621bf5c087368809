"""Unsymmetric matrices for the tests of the gradients through A*A' + beta*I (tests/test_aat_grad_api.py without a GPU,
tests/aat_grad_cases.py with one): afiro, engineered and the 1 x 1 of tests/factorize_device_matrices.py, and classes160,
the smallest matrix at which every length class and class edge of k_product_grad is hit.  No torch here."""
import numpy as np
import scipy.sparse as sp

from factorize_device_matrices import afiro, engineered, one_by_one  # noqa: F401  (re-used as they are)

PM_LEN1, PM_LEN16 = 8, 128          # the class edges of the product kernels (csrc/hip/descriptors.hip.h)


def classes160():
    """160 rows, 171 columns, 606 entries.  The list of a value in the transposed product map is one half-pair per entry
    of its column plus one (the value meets itself twice), so a column of c entries gives lists of c + 1:
      columns 0 .. 5     160, 128, 127, 9, 8, 7 entries: lists of 161 and 129 (a wave), 128 (the last of 16 lanes),
                         10 and 9 (16 lanes), 8 (the last of one lane);
      columns 6 .. 8     2 entries each (lists of 3);    column 9: 1 entry (a list of 2);    column 10: empty;
      columns 11 .. 170  a single entry 8 in row k - 11: they make A*A' positive definite (64 I plus six terms of rank
                         one and three of rank two; (min L_jj / max L_jj)^2 is about 0.7, the condition number 21).
    The other values are integers 1 .. 4 of mixed sign; the rows of a column are drawn at random."""
    m = 160
    rng = np.random.default_rng(160)
    rows, cols, vals = [], [], []
    for k, c in enumerate((160, 128, 127, 9, 8, 7, 2, 2, 2, 1)):
        r = np.sort(rng.choice(m, size=c, replace=False))
        rows += r.tolist()
        cols += [k] * c
        vals += (rng.integers(1, 5, size=c) * rng.choice([-1.0, 1.0], size=c)).tolist()
    rows += list(range(m))
    cols += list(range(11, 11 + m))
    vals += [8.0] * m
    M = sp.csc_matrix((np.array(vals), (rows, cols)), shape=(m, 11 + m))
    M.sort_indices()
    assert M.nnz == len(rows) == 606 and np.diff(M.indptr)[10] == 0
    lens = np.repeat(np.diff(M.indptr), np.diff(M.indptr)) + 1
    for edge in (PM_LEN1, PM_LEN1 + 1, PM_LEN16, PM_LEN16 + 1):
        assert (lens == edge).any(), edge
    return M


MATRICES = {"afiro": afiro, "engineered": engineered, "classes160": classes160, "one_by_one": one_by_one}


def integer_values(name, M):
    """the values of the exact cases: small integers, the pattern kept (a zero is a value like any other)
      afiro: its own values rounded;  engineered: integers 1 .. 4 of the sign of its own values;  others: as they are"""
    if name == "afiro":
        return np.round(M.data)
    if name == "engineered":
        return np.sign(M.data) * (1.0 + np.arange(M.nnz) % 4)
    return np.round(M.data)


def shift_of(name, M):
    """the nonzero beta of the end-to-end cases: 0.375; afiro: 1e-3 max |A*A'|, as tests/factorize_device_cases.py takes it"""
    if name == "afiro":
        return 1e-3 * float(np.abs((M @ M.T).toarray()).max())
    return 0.375
