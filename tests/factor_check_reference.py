"""A plain numpy restatement of the invariants cholmod_hip_factor_checks and cholmod_hip_diag_minmax report, and the
small matrices tests/test_gpu_factor_checks.py plants defects into.

The reference knows the supernodal layout only through `super`, `pi` and `px` (ch.FactorView): supernode k holds the
columns super[k] .. super[k+1]-1 as a column-major panel of nsrow = pi[k+1] - pi[k] rows at x[px[k]], its first nscol
rows being the diagonal block.  Nothing here looks at the engine's own descriptors (fronts, check tasks)."""
import math

import numpy as np

from suitesparse_amd import generators as G

EPS = 2.0 ** -52


class FactorShape:
    """The three index sets of a packed supernodal Lx: `lower` (the trapezoids, i >= j), `dead` (the strictly upper
    triangles of the diagonal blocks, i < j < nscol, which no factorization writes) and `diag` (in column order)."""

    def __init__(self, super_, pi, px, xsize):
        super_, pi, px = (np.asarray(a, dtype=np.int64) for a in (super_, pi, px))
        self.nsuper = len(super_) - 1
        self.n = int(super_[-1])
        self.xsize = int(xsize)
        self.nscol = np.diff(super_)
        self.nsrow = np.diff(pi)
        self.px = px[:-1].copy()
        self.col0 = super_[:-1].copy()
        lower, dead, diag = [], [], []
        for k in range(self.nsuper):
            nscol, nsrow, p = int(self.nscol[k]), int(self.nsrow[k]), int(self.px[k])
            assert 1 <= nscol <= nsrow and p + nscol * nsrow <= self.xsize
            i = np.arange(nsrow, dtype=np.int64)[None, :]
            j = np.arange(nscol, dtype=np.int64)[:, None]
            idx = p + j * nsrow + i                     # [column, row]
            lower.append(idx[i >= j])
            dead.append(idx[i < j])
            diag.append(p + np.arange(nscol, dtype=np.int64) * (nsrow + 1))
        self.lower = np.concatenate(lower)
        self.dead = np.concatenate(dead)
        self.diag = np.concatenate(diag)
        # every entry of a panel is in exactly one of the two sets
        both = np.concatenate([self.lower, self.dead])
        assert len(np.unique(both)) == len(both) == int((self.nscol * self.nsrow).sum())

    def at(self, k, i, j):
        """index of the entry in local row i, local column j of supernode k"""
        assert 0 <= i < self.nsrow[k] and 0 <= j < self.nscol[k]
        return int(self.px[k] + j * self.nsrow[k] + i)


def factor_checks(shape, x):
    """The five values of cholmod_hip_factor_checks for the packed factor x, in high precision."""
    x = np.asarray(x, dtype=np.float64)
    d = x[shape.diag]
    pos = d[d > 0]                                       # (a NaN is not > 0)
    lo = x[shape.lower]
    fin = lo[np.isfinite(lo)].astype(np.longdouble)
    return dict(
        half_logdet=math.fsum(np.log(pos.astype(np.longdouble))),
        upper_nonzeros=int(np.count_nonzero(x[shape.dead] != 0)),       # NaN != 0 is true, -0.0 != 0 is false
        nonfinite=int(len(lo) - len(fin)),
        fro2=math.fsum(fin * fin),
        nonpositive_diag=int(len(d) - len(pos)))


def sum_abs_log_diag(shape, x):
    d = np.asarray(x, dtype=np.float64)[shape.diag]
    return math.fsum(np.abs(np.log(d[d > 0].astype(np.longdouble))))


def diag_minmax(shape, x):
    """(min, max, count) of cholmod_hip_diag_minmax: the extremes over the diagonal entries >= 0 (+inf and 0 if there
    are none), a zero of either sign being +0.0; count = the NaN and negative ones."""
    d = np.asarray(x, dtype=np.float64)[shape.diag]
    ok = d[d >= 0] + 0.0                                 # (-0.0 + 0.0 = +0.0)
    return (float(ok.min()) if len(ok) else math.inf, float(ok.max()) if len(ok) else 0.0, int(len(d) - len(ok)))


def twin_of_complex(super_, pi, px, xsize, z):
    """The real embedding of a complex supernodal factor (suitesparse_amd/csrc/host/complex.c): every supernode doubled,
    twin(2i, 2j) = Re, twin(2i+1, 2j) = Im, twin(2i, 2j+1) = -Im, twin(2i+1, 2j+1) = Re.  z: the xsize interleaved
    complex entries.  Returns (FactorShape of the twin, its packed values)."""
    super_, pi, px = (np.asarray(a, dtype=np.int64) for a in (super_, pi, px))
    z = np.asarray(z, dtype=np.complex128)
    shape = FactorShape(2 * super_, 2 * pi, 4 * px, 4 * int(xsize))
    t = np.zeros(4 * int(xsize))
    for k in range(len(super_) - 1):
        nscol, nsrow, p = int(super_[k + 1] - super_[k]), int(pi[k + 1] - pi[k]), int(px[k])
        Z = z[p:p + nscol * nsrow].reshape(nscol, nsrow)            # [column, row]
        T = np.zeros((2 * nscol, 2 * nsrow))
        T[0::2, 0::2] = Z.real
        T[0::2, 1::2] = Z.imag
        T[1::2, 0::2] = -Z.imag
        T[1::2, 1::2] = Z.real
        t[4 * p:4 * p + 4 * nscol * nsrow] = T.reshape(-1)
    return shape, t


# ---- the matrices -------------------------------------------------------------------------------------------------

def two_dense_blocks(n1, n2, skip, seed=7):
    """A dense n1-column block and a dense n2-column root; the first block is coupled to the root's rows from `skip`
    on only.  Diagonally dominant: M M' + 4 I on the pattern, plus the largest absolute row sum on the diagonal.
    Lower-stored CSC (n, Ap, Ai, Ax); natural ordering gives the two supernodes n1 x (n1 + n2 - skip) and n2 x n2."""
    n = n1 + n2
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n)) * 0.05
    Ad = M @ M.T + np.eye(n) * 4.0
    mask = np.zeros((n, n), dtype=bool)
    mask[:n1, :n1] = True
    mask[n1:, n1:] = True
    mask[n1 + skip:, :n1] = True
    mask[:n1, n1 + skip:] = True
    Ad = np.where(mask, Ad, 0.0)
    Ad += np.eye(n) * (np.abs(Ad).sum(axis=1).max())
    ii, jj = np.nonzero(np.tril(mask))
    order = np.lexsort((ii, jj))
    Ai, cols = ii[order].astype(np.int64), jj[order]
    Ax = Ad[Ai, cols]
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    return n, Ap, Ai, Ax


def matrix(name):
    """(n, Ap, Ai, Ax, perm) of a named case; lower-stored, stype -1."""
    if name == "blocks70_135":
        return two_dense_blocks(70, 135, 74) + (np.arange(205, dtype=np.int64),)
    if name == "p2d_24_nd":
        return G.poisson2d(24) + (G.geometric_nd(24, 24, 1, 4),)
    if name == "p3d_12_nd":
        return G.poisson3d(12) + (G.geometric_nd(12, 12, 12, 4),)
    if name == "one":
        return 1, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int64), np.array([4.0]), np.zeros(1, dtype=np.int64)
    if name == "blocks1400_200":
        return two_dense_blocks(1400, 200, 100) + (np.arange(1600, dtype=np.int64),)
    raise KeyError(name)


REAL_CASES = ["blocks70_135", "p2d_24_nd", "p3d_12_nd", "one"]


def assert_front_shapes(name, shape):
    """The front shapes the tests rely on (where the strides and task boundaries of the kernels fall): asserted from
    the factor's own super / pi, not assumed."""
    nscol, nsrow = shape.nscol, shape.nsrow
    fronts = list(zip(nscol.tolist(), nsrow.tolist()))
    if name == "blocks70_135":
        # 70 = 64 + 6 columns (two check tasks, 70 = 2 mod 4) by 131 = 3 mod 64 rows; 135 = 2 * 64 + 7 = 3 mod 4 columns
        assert shape.n == 205 and fronts == [(70, 131), (135, 135)]
    elif name == "p2d_24_nd":
        # 576 = 2 * 256 + 64 diagonal entries: three blocks of the diagonal scan, the last partial
        assert shape.n == 576 and shape.nsuper == 49
        assert nscol.max() <= 35 and nsrow.max() <= 41 and int((nscol == 1).sum()) == 3
    elif name == "p3d_12_nd":
        assert shape.n == 1728 and shape.nsuper == 107
        # the widest front is the root, 214 = 3 * 64 + 22 columns (four check tasks) and square; the tallest has
        # 219 = 3 * 64 + 27 rows under 75 = 64 + 11 columns
        assert fronts[int(np.argmax(nscol))] == (214, 214) and fronts[int(np.argmax(nsrow))] == (75, 219)
        assert int((nsrow > 64).sum()) == 31 and int((nscol == 1).sum()) == 5
    elif name == "one":
        assert shape.n == 1 and fronts == [(1, 1)]
    elif name == "blocks1400_200":
        # wider than SOLVE_BIG_COLS = 256 columns (csrc/hip/descriptors.hip.h, used in plan_build.hip): the solve walks such
        # a supernode in 64-column blocks with cached inverses of the diagonal blocks -- what the upload must void
        assert shape.n == 1600 and nscol.max() >= 1400 - 64 and nscol.max() > 256
    else:
        raise KeyError(name)
