"""Test-side reference of the factor gradient (tests/test_factor_grad_api.py, tests/factor_grad_cases.py): reverse-mode
Cholesky.  Given Lbar = df/dL on the pattern of L it returns Gbar = df/dS on the pattern of L, S = L L' LOWER-STORED: an
off-diagonal entry of S stands for two entries of the symmetric matrix, Gbar (i, j), i >= j, is the derivative with respect
to that stored entry.  A numpy restatement of the supernodal recurrence on a factor's own maps, and the dense formula it
is checked against.  No torch, no GPU.

For a supernode with columns J and below-rows I, a column block b of J and R = the rows of the front after b, with
W = Gbar [R, R] known (lower-stored; the below-rows looked up in the panels of the ancestors):
    M = W + W'                                   (full square, the diagonal doubled)
    Gbar [R, b] = (Lbar [R, b] - M L [R, b]) inv (L_bb)
    Lbb  = tril (Lbar [b, b]) - tril (Gbar [R, b]' L [R, b])
    P    = inv (L_bb)' Phi (L_bb' Lbb) inv (L_bb),    Phi = the lower triangle with the diagonal halved
    Gbar [b, b] = tril (P + P') - diag (P)
blocks from the last to the first, supernodes from the last to the first.  Whatever stands in the dead strictly-upper
triangles of the diagonal blocks of Lbar is ignored."""
import numpy as np

from selinv_reference import trapezoid_of  # noqa: F401  (samples a dense result on the stored lower trapezoids)


def phi(X):
    """the lower triangle of X with the diagonal halved"""
    return np.tril(X) - 0.5 * np.diag(np.diag(X))


def lower_stored(P):
    """the derivative with respect to the stored lower triangle from P, the one with respect to every entry"""
    return np.tril(P + P.T) - np.diag(np.diag(P))


def dense_factor_grad(L, Lbar):
    """the dense formula on the whole matrix: L lower triangular, Lbar = df/dL (its strictly upper triangle is ignored);
    returns the lower triangular Gbar = df/d (lower-stored L L')"""
    n = L.shape[0]
    Li = np.linalg.solve(L, np.eye(n))
    return lower_stored(Li.T @ phi(L.T @ np.tril(Lbar)) @ Li)


def factor_grad_reference(sup, pi, px, s, Lx, Lbar_x, nb=64):
    """Gx in the layout of Lx from the supernodal factor (super, pi, px, s, Lx) and Lbar_x in the same layout"""
    Gx = np.zeros(len(Lx))
    for k in range(len(sup) - 2, -1, -1):
        rows = s[pi[k]:pi[k + 1]]
        nscol, nsrow = int(sup[k + 1] - sup[k]), len(rows)
        L = Lx[px[k]:px[k] + nsrow * nscol].reshape(nscol, nsrow).T
        Lb = Lbar_x[px[k]:px[k] + nsrow * nscol].reshape(nscol, nsrow).T
        M = np.zeros((nsrow, nsrow))                # W + W' on the rows of the front
        I = rows[nscol:]
        for j, c in enumerate(I):                   # column c of Gbar [I, I]: in the panel of the supernode that owns c
            t = int(np.searchsorted(sup, c, side="right")) - 1
            trows = s[pi[t]:pi[t + 1]]
            q = np.searchsorted(trows, I[j:])
            assert np.array_equal(trows[q], I[j:])
            col = Gx[px[t] + (c - sup[t]) * len(trows) + q].copy()
            col[0] *= 2.0
            M[nscol + j:, nscol + j] = col
            M[nscol + j, nscol + j:] = col
        for b0 in range(((nscol - 1) // nb) * nb, -1, -nb):
            b1 = min(b0 + nb, nscol)
            Lbb = L[b0:b1, b0:b1]
            Li = np.linalg.inv(Lbb)
            GR = (Lb[b1:, b0:b1] - M[b1:, b1:] @ L[b1:, b0:b1]) @ Li
            M[b1:, b0:b1], M[b0:b1, b1:] = GR, GR.T
            Q = np.tril(Lb[b0:b1, b0:b1]) - np.tril(GR.T @ L[b1:, b0:b1])
            P = Li.T @ phi(Lbb.T @ Q) @ Li
            M[b0:b1, b0:b1] = P + P.T
        Gp = M[:, :nscol].copy()
        Gp[:nscol] = np.tril(Gp[:nscol])
        Gp[np.arange(nscol), np.arange(nscol)] *= 0.5
        Gx[px[k]:px[k] + nsrow * nscol] = Gp.T.ravel()
    return Gx


def dense_of_layout(fv, Xx):
    """the dense lower triangular matrix of an array in the layout of Lx (fv: the FactorView), the dead triangles left out"""
    Xx = np.asarray(Xx)
    D = np.zeros((fv.n, fv.n))
    for k in range(fv.nsuper):
        rows = fv.s[fv.pi[k]:fv.pi[k + 1]]
        nscol, nsrow = int(fv.super[k + 1] - fv.super[k]), len(rows)
        P = Xx[fv.px[k]:fv.px[k] + nsrow * nscol].reshape(nscol, nsrow).T.copy()
        P[:nscol] = np.tril(P[:nscol])
        D[np.ix_(rows, rows[:nscol])] = P
    return D


def dense_factor(fv):
    """the dense lower triangular L of a numeric supernodal factor (FactorView), in the factor's ordering"""
    return dense_of_layout(fv, fv.x)


def random_lbar(fv, seed, dead=0.0):
    """a seeded standard-normal Lbar on the stored lower trapezoids, `dead` in the dead triangles -> (Lbar_x, mask)"""
    _, mask = trapezoid_of(np.zeros((fv.n, fv.n)), fv.super, fv.pi, fv.px, fv.s, fv.xsize)
    Lbar_x = np.where(mask, np.random.default_rng(seed).standard_normal(fv.xsize), dead)
    return Lbar_x, mask
