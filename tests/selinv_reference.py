"""Test-side reference of the selected inverse (tests/test_selinv_api.py, tests/selinv_cases.py): a numpy restatement of
the supernodal Takahashi recurrence on a factor's own maps, the dense inverse it is checked against, and the matrices of
both test files.  No torch, no GPU.

For a supernode with columns J and below-rows I, a column block b of J and R = the rows of the front after b:
    G = L[R,b] inv(L[b,b]),   Z[R,b] = -Z[R,R] G,   Z[b,b] = inv(L[b,b])' inv(L[b,b]) - G' Z[R,b]
blocks from the last to the first, supernodes from the last to the first, Z[I,I] looked up in the panels of the ancestors."""
import os

import numpy as np
import scipy.sparse as sp

from suitesparse_amd import generators as G

EPS = np.finfo(float).eps
HERE = os.path.dirname(os.path.abspath(__file__))


def selinv_reference(sup, pi, px, s, Lx, nb=64):
    """Zx in the layout of Lx from the supernodal factor (super, pi, px, s, Lx)"""
    Zx = np.zeros(len(Lx))
    for k in range(len(sup) - 2, -1, -1):
        rows = s[pi[k]:pi[k + 1]]
        nscol, nsrow = int(sup[k + 1] - sup[k]), len(rows)
        L = Lx[px[k]:px[k] + nsrow * nscol].reshape(nscol, nsrow).T
        Z = np.zeros((nsrow, nsrow))
        I = rows[nscol:]
        for j, c in enumerate(I):                   # column c of Z[I,I]: in the panel of the supernode that owns c
            t = int(np.searchsorted(sup, c, side="right")) - 1
            trows = s[pi[t]:pi[t + 1]]
            q = np.searchsorted(trows, I[j:])
            assert np.array_equal(trows[q], I[j:])
            col = Zx[px[t] + (c - sup[t]) * len(trows) + q]
            Z[nscol + j:, nscol + j] = col
            Z[nscol + j, nscol + j:] = col
        for b0 in range(((nscol - 1) // nb) * nb, -1, -nb):
            b1 = min(b0 + nb, nscol)
            Li = np.linalg.inv(L[b0:b1, b0:b1])
            Gm = L[b1:, b0:b1] @ Li
            W = -Z[b1:, b1:] @ Gm
            Z[b1:, b0:b1], Z[b0:b1, b1:] = W, W.T
            D = Li.T @ Li - Gm.T @ W
            Z[b0:b1, b0:b1] = 0.5 * (D + D.T)
        P = Z[:, :nscol].copy()
        P[:nscol] = np.tril(P[:nscol])
        Zx[px[k]:px[k] + nsrow * nscol] = P.T.ravel()
    return Zx


def dense_symmetric(n, Lp, Li, Lx, beta=0.0):
    """the symmetric matrix given by its lower triangle (CSC), plus beta I, dense"""
    Lo = sp.csc_matrix((Lx, Li, Lp), shape=(n, n)).toarray()
    return np.tril(Lo) + np.tril(Lo, -1).T + beta * np.eye(n)


def trapezoid_of(Zd, sup, pi, px, s, xsize):
    """(the entries of the dense Zd on the stored lower trapezoids, in the layout of Lx; the mask of those entries)"""
    out, mask = np.zeros(xsize), np.zeros(xsize, dtype=bool)
    for k in range(len(sup) - 1):
        rows = s[pi[k]:pi[k + 1]]
        nscol, nsrow = int(sup[k + 1] - sup[k]), len(rows)
        P = Zd[np.ix_(rows, rows[:nscol])]
        live = np.ones((nsrow, nscol), dtype=bool)
        live[:nscol] = np.tril(live[:nscol])
        out[px[k]:px[k] + nsrow * nscol] = np.where(live, P, 0.0).T.ravel()
        mask[px[k]:px[k] + nsrow * nscol] = live.T.ravel()
    return out, mask


def factor_rcond(fv):
    """(min L_jj / max L_jj)^2 of a numeric supernodal factor (FactorView)"""
    d = []
    for k in range(fv.nsuper):
        nsrow, nscol = int(fv.pi[k + 1] - fv.pi[k]), int(fv.super[k + 1] - fv.super[k])
        d.append(fv.x[int(fv.px[k]) + (nsrow + 1) * np.arange(nscol)])
    d = np.concatenate(d)
    return float((d.min() / d.max()) ** 2)


def tolerance(rcond):
    """the project's parity bar with the scaling of tests/test_tcov_matrices.py, relative to max |Z_ref|"""
    return max(1e-12, 20 * EPS / rcond)


def compare(fv, Zx, n, Lp, Li, Lx, beta=0.0):
    """-> (max |Z - Z_ref| / max |Z_ref| over the stored lower trapezoids, tol, entries != 0 in the dead upper triangles)
    for Zx against the dense inverse of P (A + beta I) P', P = fv.Perm"""
    Ad = dense_symmetric(n, Lp, Li, Lx, beta)
    p = np.asarray(fv.Perm)
    Zd = np.linalg.inv(Ad[np.ix_(p, p)])
    ref, mask = trapezoid_of(Zd, fv.super, fv.pi, fv.px, fv.s, fv.xsize)
    with np.errstate(invalid="ignore"):
        diff = np.abs(np.asarray(Zx)[mask] - ref[mask])
    err = float(np.where(np.isfinite(diff), diff, np.inf).max() / np.abs(ref[mask]).max())
    dead = int(np.count_nonzero(np.asarray(Zx)[~mask] != 0.0))
    return err, tolerance(factor_rcond(fv)), dead


# ---- the matrices: name -> dict (n, Lp, Li, Lx: lower CSC; perm or None; postorder; norelax) ----------------------------------

def _lower_csc(Ad):
    M = sp.csc_matrix(sp.tril(sp.csc_matrix(Ad)))
    M.sort_indices()
    return Ad.shape[0], M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)


def dense200():
    B = np.random.default_rng(1).standard_normal((200, 200))
    return _lower_csc(B @ B.T / 200 + np.eye(200))


def arrow300():
    n = 300
    A = np.zeros((n, n))
    rng = np.random.default_rng(2)
    for i in range(230, n):
        A[i, :i] = rng.uniform(-.5, .5, i)
    A = A + A.T
    A[np.arange(n), np.arange(n)] = 1.0 + np.abs(A).sum(axis=1)
    return _lower_csc(A)


def forest148():
    blocks = []
    for n, Ap, Ai, Ax in (G.poisson2d(9), G.poisson3d(4)):
        blocks.append(sp.csc_matrix((Ax, Ai, Ap), shape=(n, n)))
    blocks += [sp.csc_matrix(np.array([[v]])) for v in (2.0, 0.5, 3.0)]
    M = sp.csc_matrix(sp.block_diag(blocks))
    M.sort_indices()
    return M.shape[0], M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)


def _golden(f):
    from matrix_files import read_file, to_lower
    m = read_file(os.path.join(HERE, "golden", "demo", f))
    _, Lp, Li, Lx = to_lower(m)
    return m["nrow"], np.asarray(Lp, dtype=np.int64), np.asarray(Li, dtype=np.int64), np.asarray(Lx, dtype=np.float64)


def _case(mat, perm=None, postorder=True, norelax=False):
    n, Lp, Li, Lx = mat
    return dict(n=n, Lp=Lp, Li=Li, Lx=Lx, perm=perm, postorder=postorder, norelax=norelax)


CASES = {
    "p3d_12_nd": lambda: _case(G.poisson3d(12), G.geometric_nd(12, 12, 12, 4)),
    "p2d_60_nd": lambda: _case(G.poisson2d(60), G.geometric_nd(60, 60, 1, 4)),
    "box9r2_nd": lambda: _case(G.box_stencil3d(9, 2), G.geometric_nd(9, 9, 9, 3)),
    "p3d_10x7x5_nd": lambda: _case(G.poisson3d(10, 7, 5), G.geometric_nd(10, 7, 5, 3)),
    "p3d_9_natural_norelax": lambda: _case(G.poisson3d(9), norelax=True),
    "p3d_9_random_nopost": lambda: _case(G.poisson3d(9), np.random.default_rng(3).permutation(729).astype(np.int64), postorder=False),
    "dense200": lambda: _case(dense200()),
    "arrow300": lambda: _case(arrow300()),
    "arrow300_norelax": lambda: _case(arrow300(), norelax=True),
    "forest148": lambda: _case(forest148()),
    "forest148_norelax": lambda: _case(forest148(), norelax=True),
    "bcsstk01": lambda: _case(_golden("bcsstk01.tri")),
    "bcsstk02": lambda: _case(_golden("bcsstk02.tri")),
}


def factorized(case, use_gpu, beta=0.0, hip_flags=0):
    """-> (Session, A, Lf) with Lf the numeric supernodal factor of the case (lower-stored A)"""
    from suitesparse_amd import cholmod as ch
    S = ch.Session(use_gpu=use_gpu, postorder=case["postorder"], hip_flags=hip_flags)
    if case["norelax"]:
        for k in range(3):
            S.cm.nrelax[k] = 0
            S.cm.zrelax[k] = 0.0
    A = S.sparse(case["n"], case["Lp"], case["Li"], case["Lx"], -1)
    Lf = S.analyze(A, case["perm"])
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK, S.cm.status
    return S, A, Lf
