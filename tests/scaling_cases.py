"""Diagonal scalings by powers of two, shared by tests/test_scaling_reference.py (CPU) and tests/test_gpu_pivot_range.py.

For D = diag(2^e_i), chol(D M D) = D chol(M): every operation of a Cholesky factorization (multiply, fused multiply-add,
divide, square root) is homogeneous, and a power of two changes no significand, so the identity holds bit for bit in IEEE
arithmetic while nothing overflows and nothing that matters goes subnormal.  The reference for a scaled problem is
therefore the factor of the UNSCALED matrix (the oracle's, LAPACK's), the result under test is descaled by exact powers of
two, and the suite's existing tolerances apply unchanged.  Code that adds quantities of different homogeneity -- a
literal 1.0 leaking out of padding, an absolute threshold, a rescale undone by the wrong power -- breaks the identity
grossly.

Nothing here touches a GPU.  Every case asserts its preconditions on the CPU (check_* below): a case that fails one is an
error of the test, never a skip."""
import functools
import zlib

import numpy as np

from oracle.oracle import OracleFactor
from suitesparse_amd import generators as G

HI, LO = 1e290, 1e-290                  # the rescale thresholds of sqrt_rsqrt (csrc/hip/kernels.hip.h)
DBL_MIN = np.finfo(np.float64).tiny     # 2^-1022
DBL_MAX = np.finfo(np.float64).max
PROFILES = ["up", "down", "graded", "mixed"]


# ---- scaling and descaling ---------------------------------------------------------------------------------------------

def _ldexp(v, k):
    """v * 2^k, exact; complex values part by part"""
    v = np.asarray(v)
    k = np.asarray(k, dtype=np.int64)
    if np.iscomplexobj(v):
        return np.ldexp(v.real, k) + 1j * np.ldexp(v.imag, k)
    return np.ldexp(v, k)


def scale_csc(n, Ap, Ai, Ax, e):
    """the values of D A D for the CSC matrix (Ap, Ai, Ax), D = diag(2^e)"""
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    return _ldexp(Ax, e[np.asarray(Ai)] + e[cols])


def scale_dense(F, e):
    return np.ldexp(F, e[:, None] + e[None, :])


def descale_front(F, nscol, e):
    """[L11; L21] and the Schur block of a dense front factored from D F D, back in the units of F: rows of L by D_i, the
    Schur block by D_i D_j.  (The strictly upper part of the first nscol columns is scaled input: by D_i D_j as well.)"""
    out = np.empty_like(F)
    out[:, :nscol] = np.ldexp(F[:, :nscol], -e[:, None])
    iu = np.triu_indices(nscol, 1)
    out[:nscol, :nscol][iu] = np.ldexp(F[:nscol, :nscol][iu], -(e[iu[0]] + e[iu[1]]))
    out[:, nscol:] = np.ldexp(F[:, nscol:], -(e[:, None] + e[None, nscol:]))
    return out


def descale_factor(x, ref, e):
    """a supernodal factor of D A D (packed x, the structure of ref), row by row back to that of A: entry (i, j) of L by
    D of the ORIGINAL index of permuted row i"""
    return _ldexp(x, -e[ref.rowidx])


# ---- sparse matrices and their reference -----------------------------------------------------------------------------------

def _big_supernode():
    """the matrix of test_big_supernode_block_walk_solves_multi_rhs (solve_device_cases._big_supernode_matrix (1.0), written
    out here because that module imports torch, which stays out of the pytest process): a 1400-column supernode with 100
    rows below it, followed by a dense 200-column root"""
    n1, n2 = 1400, 200
    n = n1 + n2
    rng = np.random.default_rng(7)
    M = rng.standard_normal((n, n)) * 0.05
    Ad = M @ M.T + np.eye(n) * 4.0
    mask = np.zeros((n, n), dtype=bool)
    mask[:n1, :n1] = True
    mask[n1:, n1:] = True
    mask[n1 + 100:, :n1] = True
    mask[:n1, n1 + 100:] = True
    Ad = np.where(mask, Ad, 0.0)
    Ad += np.eye(n) * (np.abs(Ad).sum(axis=1).max())
    ii, jj = np.nonzero(np.tril(mask))
    order = np.lexsort((ii, jj))
    Ai, cols = ii[order].astype(np.int64), jj[order]
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    return n, Ap, Ai, Ad[Ai, cols], np.arange(n, dtype=np.int64)


def _complex_p3d9():
    from test_complex import hermitian_from
    n, Ap, Ai, Ax = G.poisson3d(9)
    return (n,) + hermitian_from(n, Ap, Ai, Ax) + (G.geometric_nd(9, 9, 9, 3),)


MATRICES = {
    "p2d_48_nd": lambda: G.poisson2d(48) + (G.geometric_nd(48, 48, 1, 4),),           # thin fronts
    "p3d_12_nd": lambda: G.poisson3d(12) + (G.geometric_nd(12, 12, 12, 4),),
    "box9r2_nd": lambda: G.box_stencil3d(9, 2) + (G.geometric_nd(9, 9, 9, 3),),
    "big_supernode": _big_supernode,
    "cx_p3d_9_nd": _complex_p3d9,                                                    # complex Hermitian
}
SPARSE_NAMES = ["p2d_48_nd", "p3d_12_nd", "box9r2_nd"]


class Ref:
    """A matrix, the oracle's factor of it (computed once, never changed) and what the scalings need of both."""

    def __init__(self, name):
        self.name = name
        self.n, self.Ap, self.Ai, self.Ax, self.perm = MATRICES[name]()
        self.Ap, self.Ai = np.asarray(self.Ap, dtype=np.int64), np.asarray(self.Ai, dtype=np.int64)
        self.cx = np.iscomplexobj(self.Ax)
        self.O = self.factor(self.Ax)
        O = self.O
        self.x = (O.xc if self.cx else O.x).copy()
        self.struct = {k: getattr(O, k).copy() for k in ("Perm", "super", "pi", "px", "s")}
        self.mask = O.lower_mask()
        sup, pi, px, s, Perm = (self.struct[k] for k in ("super", "pi", "px", "s", "Perm"))
        self.rowidx = np.zeros(O.xsize, dtype=np.int64)
        self.pivot = np.zeros(self.n)                   # L_ref(j,j)^2 at the ORIGINAL index of permuted column j
        for k in range(O.nsuper):
            nscol, nsrow = int(sup[k + 1] - sup[k]), int(pi[k + 1] - pi[k])
            self.rowidx[px[k]:px[k] + nsrow * nscol] = np.tile(Perm[s[pi[k]:pi[k + 1]]], nscol)
            d = self.x[px[k] + np.arange(nscol) * (nsrow + 1)]
            self.pivot[Perm[sup[k]:sup[k + 1]]] = np.real(d) ** 2
        assert np.all(self.pivot > 0)

    def factor(self, Ax):
        """a fresh oracle factorization of other values on the same pattern"""
        O = OracleFactor(self.n, self.Ap, self.Ai, -1, perm=self.perm, postorder=True)
        assert (O.factorize_complex(Ax) if self.cx else O.factorize(Ax)) == 0
        return O


@functools.lru_cache(maxsize=None)
def reference(name):
    return Ref(name)


# ---- exponent profiles -------------------------------------------------------------------------------------------------

def _e_up(amax):
    """the largest E with 2^(2E) amax < 2^1020: amax = m 2^k, 1/2 <= m < 1, holds iff 1020 - 2E >= k"""
    k = int(np.frexp(amax)[1])
    return (1020 - k) // 2


def _e_down(pmax):
    """the largest E with 2^(2E) pmax < 1e-290 (the most room above the subnormals)"""
    E = -400
    while np.ldexp(pmax, 2 * (E + 1)) < LO:
        E += 1
    while not np.ldexp(pmax, 2 * E) < LO:
        E -= 1
    return E


def exponents(profile, n, amax, pmax, seed):
    """e_i of the profile, for a matrix with largest entry amax and largest reference pivot pmax"""
    Eup, Edn = _e_up(amax), _e_down(pmax)
    rng = np.random.default_rng(seed)
    if profile == "up":
        return np.full(n, Eup, dtype=np.int64)
    if profile == "down":
        return np.full(n, Edn, dtype=np.int64)
    if profile == "graded":
        return rng.integers(-240, 241, n).astype(np.int64)
    if profile == "mixed":
        e = rng.choice(np.array([Edn, 0, Eup], dtype=np.int64), n)
        e[rng.permutation(n)[:3]] = [Edn, 0, Eup]           # (every class occurs, whatever the draw)
        return e
    raise KeyError(profile)


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def check_pivots(profile, e, pivot):
    """the scaled pivots 2^(2 e_i) p_i lie on the side of sqrt_rsqrt's thresholds the profile is about"""
    sp = np.ldexp(pivot, 2 * e)
    assert np.all(np.isfinite(sp)) and np.all(sp >= DBL_MIN)
    if profile == "up":
        assert np.all(sp > HI), sp.min()
    elif profile == "down":
        assert np.all(sp < LO), sp.max()
    elif profile == "graded":
        assert np.all((sp > LO) & (sp < HI))
        assert sp.max() / sp.min() > 2.0 ** 600                 # magnitudes really are mixed
    else:
        hi, lo = e == e.max(), e == e.min()
        assert hi.any() and lo.any() and (~hi & ~lo).any()
        assert np.all(sp[hi] > HI) and np.all(sp[lo] < LO) and np.all((sp[~hi & ~lo] > LO) & (sp[~hi & ~lo] < HI))


def check_values(v):
    """finite, and no nonzero subnormal"""
    a = np.abs(np.asarray(v)).reshape(-1)
    if np.iscomplexobj(v):
        a = np.concatenate([np.abs(np.real(v)).reshape(-1), np.abs(np.imag(v)).reshape(-1)])
    assert np.all(np.isfinite(a))
    assert np.all((a == 0) | (a >= DBL_MIN)), a[(a != 0) & (a < DBL_MIN)][:4]


def sparse_case(name, profile):
    """(ref, e, scaled values of A), preconditions asserted"""
    ref = reference(name)
    amax, amin = np.abs(ref.Ax).max(), np.abs(ref.Ax[ref.Ax != 0]).min()
    assert ref.pivot.max() / amin < 2.0 ** 58                   # (an E_down exists)
    e = exponents(profile, ref.n, amax, ref.pivot.max(), _seed(name, profile))
    Axs = scale_csc(ref.n, ref.Ap, ref.Ai, ref.Ax, e)
    check_values(Axs)
    check_values(descale_factor(ref.x, ref, -e)[ref.mask])     # D L_ref
    check_pivots(profile, e, ref.pivot)
    return ref, e, Axs


# ---- dense fronts ------------------------------------------------------------------------------------------------------

DENSE_SHAPES = [(65, 64), (200, 100), (333, 129), (700, 530)]


@functools.lru_cache(maxsize=None)
def dense_reference(nsrow, nscol):
    """M M' + n I (as test_dense_partial_factorization draws it) and LAPACK's L11, L21 and Schur block of it"""
    import scipy.linalg as sl
    rng = np.random.default_rng(nsrow * 1000 + nscol)
    M = rng.standard_normal((nsrow, nsrow))
    Fm = M @ M.T + nsrow * np.eye(nsrow)
    Fm = np.tril(Fm) + np.tril(Fm, -1).T                        # exactly symmetric
    L11 = np.linalg.cholesky(Fm[:nscol, :nscol])
    L21 = sl.solve_triangular(L11, Fm[nscol:, :nscol].T, lower=True).T
    Sc = np.tril(Fm[nscol:, nscol:] - L21 @ L21.T)
    for a in (Fm, L11, L21, Sc):
        a.setflags(write=False)
    return Fm, L11, L21, Sc


def dense_case(nsrow, nscol, profile):
    """(Fm, L11, L21, Sc, e, D Fm D), preconditions asserted"""
    Fm, L11, L21, Sc = dense_reference(nsrow, nscol)
    piv = np.diag(L11) ** 2
    assert piv.max() / np.abs(Fm).min() < 2.0 ** 58
    e = exponents(profile, nsrow, np.abs(Fm).max(), piv.max(), _seed(nsrow, nscol, profile))
    Fs = scale_dense(Fm, e)
    check_values(Fs)
    check_values(np.ldexp(L11, e[:nscol, None]))
    check_values(np.ldexp(L21, e[nscol:, None]))
    check_values(np.ldexp(Sc, e[nscol:, None] + e[None, nscol:]))
    check_pivots(profile, e[:nscol], piv)
    return Fm, L11, L21, Sc, e, Fs
