"""Test-side reference of the Schur complement on the factor (tests/test_schur_api.py, tests/schur_cases.py): a numpy
restatement of what the device kernels are specified to read -- the supernodes that hold trailing columns, of each the
contributing columns and the rows from the first of them down, the strictly upper triangle of every diagonal block masked
--, the dense references it and the device are checked against, and the list of m both test files walk.  No torch, no GPU.

With t = n - m, I = the first t positions of the factor's ordering and S = the last m:
    L = [L11 0 ; L21 L22],   Sc = M_SS - M_SI inv (M_II) M_IS = L22 L22'   for M = P (A + beta I) P'."""
import numpy as np
import scipy.linalg as sla

from selinv_reference import CASES, dense_symmetric, factor_rcond, factorized, tolerance  # noqa: F401  (re-exported)

BETAS = (0.0, 0.375)


def _panels(sup, pi, px, s, Lx, n, m):
    """per contributing supernode: (rows - t, columns - t, the panel restricted and masked as the kernel reads it)"""
    t0 = n - m
    if m == 0:
        return
    s0 = int(np.searchsorted(sup, t0, side="right")) - 1
    for k in range(s0, len(sup) - 1):
        rows = np.asarray(s[pi[k]:pi[k + 1]])
        nscol, nsrow = int(sup[k + 1] - sup[k]), len(rows)
        P = np.asarray(Lx[px[k]:px[k] + nsrow * nscol]).reshape(nscol, nsrow).T
        c0 = max(0, t0 - int(sup[k]))                   # the boundary may fall inside the first supernode
        w = nscol - c0
        Pc = P[c0:, c0:].copy()                         # the rows from the first contributing column down
        Pc[:w] = np.tril(Pc[:w])                        # the dead upper triangle counts as zero whatever it holds
        assert np.all(rows[c0:] >= t0)
        yield rows[c0:] - t0, np.arange(int(sup[k]) + c0, int(sup[k + 1])) - t0, Pc


def trailing_factor(sup, pi, px, s, Lx, n, m):
    """the dense L22 = L [n-m:, n-m:] (m x m), zeros outside the pattern and above the diagonal"""
    F = np.zeros((m, m))
    for r, c, Pc in _panels(sup, pi, px, s, Lx, n, m):
        F[np.ix_(r, c)] = Pc
    return F


def schur_restated(sup, pi, px, s, Lx, n, m):
    """Sc = sum over the contributing supernodes of panel panel', scattered by the row lists"""
    Sc = np.zeros((m, m))
    for r, _, Pc in _panels(sup, pi, px, s, Lx, n, m):
        Sc[np.ix_(r, r)] += Pc @ Pc.T
    return Sc


def permuted_dense(case, perm, beta=0.0):
    """M = P (A + beta I) P', dense"""
    Ad = dense_symmetric(case["n"], case["Lp"], case["Li"], case["Lx"], beta)
    p = np.asarray(perm)
    return Ad[np.ix_(p, p)]


def dense_schur(M, m):
    """M_SS - M_SI inv (M_II) M_IS for the last m variables of the dense symmetric positive definite M"""
    n = M.shape[0]
    t0 = n - m
    if m == 0:
        return np.zeros((0, 0))
    if t0 == 0:
        return M.copy()
    return M[t0:, t0:] - M[t0:, :t0] @ sla.solve(M[:t0, :t0], M[:t0, t0:], assume_a="pos")


def dense_reduce(M, m, Bp):
    """the condensed right-hand side B_S - M_SI inv (M_II) B_I; Bp (n x nrhs) in the factor's ordering"""
    t0 = M.shape[0] - m
    if t0 == 0:
        return Bp.copy()
    return Bp[t0:] - M[t0:, :t0] @ sla.solve(M[:t0, :t0], Bp[:t0], assume_a="pos")


def reduce_restated(Lfull, F, perm, B):
    """(G, Y) as cholmod_l_hip_schur_reduce_device forms them: Y = inv (L) P B, G = L22 Y_S; B (n x nrhs), A's ordering"""
    n, m = Lfull.shape[0], F.shape[0]
    Y = sla.solve_triangular(Lfull, B[np.asarray(perm)], lower=True)
    return F @ Y[n - m:], Y


def expand_restated(Lfull, F, perm, Y, XS):
    """X = P' inv (L') [Y_I ; L22' XS], in A's ordering"""
    n, m = Lfull.shape[0], F.shape[0]
    W = Y.copy()
    W[n - m:] = F.T @ XS
    X = np.empty_like(W)
    X[np.asarray(perm)] = sla.solve_triangular(Lfull, W, lower=True, trans="T")
    return X


def m_first_column(fv):
    """an m for which n - m is the first column of a supernode (the middle one; a single supernode: m = n)"""
    return int(fv.n - fv.super[fv.nsuper // 2])


def m_inside(fv):
    """an m for which n - m lies strictly inside the LAST supernode of at least 3 columns (its second column); None: the
    factor has no such supernode"""
    w = np.diff(np.asarray(fv.super))
    wide = np.flatnonzero(w >= 3)
    return int(fv.n - fv.super[wide[-1]] - 1) if len(wide) else None


def m_list(fv):
    n = int(fv.n)
    ms = {m for m in (0, 1, 2, 15, 16, 17, 63, 64, 65, n // 2, n - 1, n) if 0 <= m <= n}
    ms.add(m_first_column(fv))
    if m_inside(fv) is not None:
        ms.add(m_inside(fv))
    return sorted(ms)
