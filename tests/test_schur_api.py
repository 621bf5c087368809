"""The Schur complement on the device-resident factor (cholmod_l_hip_schur_device / _reduce_device / _expand_device and the
engine's cholmod_hip_schur_device / cholmod_hip_trailing_multiply_device): what can be checked without a GPU -- the exported
symbols, the argument checks, which come before the engine or a device is touched (integers stand in for device pointers:
nothing here may dereference them), the numpy restatement of what the kernels read (tests/schur_reference.py) against the
dense Schur complement, and Session.schur_perm, a pure host helper."""
import ctypes as C

import numpy as np
import pytest

import schur_reference as R
from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FS, FF, FB, FY, FG, FX = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
NEW = ("cholmod_hip_schur_device", "cholmod_hip_trailing_multiply_device", "cholmod_l_hip_schur_device",
       "cholmod_l_hip_schur_reduce_device", "cholmod_l_hip_schur_expand_device")


def test_library_exports_the_schur_complement():
    for L in (ch.lib(), ch.lib(hooks=True)):
        for name in NEW:
            assert hasattr(L, name), name
            assert name in ch.API_SYMBOLS + ch.HIP_SYMBOLS
    for name in ("schur_index", "schur_device", "schur_reduce_device", "schur_expand_device", "schur_perm"):
        assert callable(getattr(ch.Session, name))


def _cpu_factor(numeric=True):
    case = R.CASES["p3d_12_nd"]()
    S = ch.Session(use_gpu=0)
    A = S.sparse(case["n"], case["Lp"], case["Li"], case["Lx"], -1)
    Lf = S.analyze(A, case["perm"])
    if numeric:
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    S.cm.error_handler = ch.ERRFUNC(0)
    return S, A, Lf


def _schur(S, Lf, m=5, Sd=FS, lds=None, Fd=FF, ldf=None):
    S.cm.status = ch.OK
    lds, ldf = m if lds is None else lds, m if ldf is None else ldf
    return S.L.cholmod_l_hip_schur_device(Lf, m, Sd, lds, Fd, ldf, None, C.byref(S.cm)), S.cm.status


def _reduce(S, Lf, m=5, B=FB, ldb=None, Y=FY, ldy=None, Gd=FG, ldg=None, nrhs=3):
    S.cm.status = ch.OK
    n = int(Lf.contents.n) if Lf else 0
    ldb, ldy, ldg = n if ldb is None else ldb, n if ldy is None else ldy, m if ldg is None else ldg
    return S.L.cholmod_l_hip_schur_reduce_device(Lf, m, B, ldb, Y, ldy, Gd, ldg, nrhs, None, C.byref(S.cm)), S.cm.status


def _expand(S, Lf, m=5, Y=FY, ldy=None, XS=FG, ldxs=None, X=FX, ldx=None, nrhs=3):
    S.cm.status = ch.OK
    n = int(Lf.contents.n) if Lf else 0
    ldy, ldx, ldxs = n if ldy is None else ldy, n if ldx is None else ldx, m if ldxs is None else ldxs
    return S.L.cholmod_l_hip_schur_expand_device(Lf, m, Y, ldy, XS, ldxs, X, ldx, nrhs, None, C.byref(S.cm)), S.cm.status


def _all_three(S, Lf, want):
    assert _schur(S, Lf) == want and _reduce(S, Lf) == want and _expand(S, Lf) == want


def test_argument_checks_come_before_any_device():
    S, A, Lf = _cpu_factor()
    n = int(Lf.contents.n)
    bad = (0, ch.INVALID)
    # the GPU is off: no host fallback, with or without hip_cpu_fallback
    for fb in (0, 1):
        S.cm.hip_cpu_fallback = fb
        _all_three(S, Lf, bad)
        assert _schur(S, Lf, m=0) == bad and _reduce(S, Lf, nrhs=0) == bad
    S.cm.hip_cpu_fallback = 0
    for gpu in (0, 1):          # ... the rest also with the GPU asked for: no check needs a device
        S.cm.useGPU = gpu
        # NULL pointers, both outputs NULL
        _all_three(S, None, bad)
        assert _schur(S, Lf, Sd=None, Fd=None) == bad
        assert _reduce(S, Lf, B=None) == bad and _reduce(S, Lf, Y=None) == bad and _reduce(S, Lf, Gd=None) == bad
        assert _expand(S, Lf, Y=None) == bad and _expand(S, Lf, XS=None) == bad and _expand(S, Lf, X=None) == bad
        # m > n, leading dimensions
        assert _schur(S, Lf, m=n + 1) == bad and _reduce(S, Lf, m=n + 1) == bad and _expand(S, Lf, m=n + 1) == bad
        assert _schur(S, Lf, lds=4) == bad and _schur(S, Lf, ldf=4) == bad
        assert _schur(S, Lf, Sd=None, lds=0, ldf=4) == bad and _schur(S, Lf, Fd=None, ldf=0, lds=4) == bad
        assert _reduce(S, Lf, ldb=n - 1) == bad and _reduce(S, Lf, ldy=n - 1) == bad and _reduce(S, Lf, ldg=4) == bad
        assert _expand(S, Lf, ldy=n - 1) == bad and _expand(S, Lf, ldx=n - 1) == bad and _expand(S, Lf, ldxs=4) == bad
        assert _expand(S, Lf, X=FY) == bad
        # a CPU-path factor was not factorized on the device (also for what would touch nothing)
        _all_three(S, Lf, bad)
        assert _schur(S, Lf, m=0) == bad and _reduce(S, Lf, m=0) == bad and _expand(S, Lf, m=0) == bad
        # L->minor < n
        Lf.contents.minor = n - 1
        _all_three(S, Lf, bad)
        Lf.contents.minor = n
        # several ranks
        S.cm.hip_world = 2
        _all_three(S, Lf, bad)
        S.cm.hip_world = 1
        # a simplicial L
        Lf.contents.is_super = 0
        _all_three(S, Lf, bad)
        Lf.contents.is_super = 1
        # complex / zomplex L
        for xt in (ch.COMPLEX, ch.ZOMPLEX):
            Lf.contents.xtype = xt
            _all_three(S, Lf, (0, ch.NOT_INSTALLED))
            Lf.contents.xtype = ch.REAL
    S.cm.useGPU = 0
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_symbolic_factor_is_refused():
    S, A, Lf = _cpu_factor(numeric=False)
    assert Lf.contents.xtype == ch.PATTERN
    for gpu in (0, 1):
        S.cm.useGPU = gpu
        _all_three(S, Lf, (0, ch.INVALID))
    S.cm.useGPU = 0
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_engine_refuses_a_host_only_plan():
    lib = ch.lib()
    n, Ap, Ai, Ax = G.poisson3d(5)
    O = OracleFactor(n, Ap, Ai, -1, perm=None, postorder=True)
    keep = [np.ascontiguousarray(getattr(O, k), dtype=np.int64) for k in ("super", "pi", "px", "s")]
    st = C.c_int(0)
    P = lib.cholmod_hip_plan_create(n, len(keep[0]) - 1, *(a.ctypes.data_as(C.c_void_p) for a in keep),
                                    ch.HIP_PLAN_HOST_ONLY, C.byref(st))
    assert P and st.value == 0
    for plan in (P, None):
        assert lib.cholmod_hip_schur_device(plan, 5, FS, 5, FF, 5, None) == ch.HIP_INVALID
        assert lib.cholmod_hip_schur_device(plan, 0, FS, 5, FF, 5, None) == ch.HIP_INVALID
        for trans in (0, 1):
            assert lib.cholmod_hip_trailing_multiply_device(plan, 5, trans, FB, 5, FG, 5, 2, None) == ch.HIP_INVALID
    lib.cholmod_hip_plan_destroy(P)


@pytest.mark.parametrize("beta", R.BETAS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_against_the_dense_schur_complement(name, beta):
    """the numpy restatement -- the supernodes from supermap [n - m] on, their contributing columns, the rows from the first
    of them down, the masked upper triangles, a straddled first supernode -- on the CPU path's factor, against the dense
    M_SS - M_SI inv (M_II) M_IS of M = P (A + beta I) P', for every m of the list: at least 4 x inside the bar
    max (1e-12, 20 eps / rcond) max |ref| the device is held to.  L22 L22' of the restated dense L22 is the same matrix."""
    case = R.CASES[name]()
    S, A, Lf = R.factorized(case, use_gpu=0, beta=beta)
    fv = ch.FactorView(Lf)
    n = case["n"]
    tol = R.tolerance(R.factor_rcond(fv))
    M = R.permuted_dense(case, fv.Perm, beta)
    ms = R.m_list(fv)
    mi, mf = R.m_inside(fv), R.m_first_column(fv)
    # every case of the table has a supernode of at least 3 columns
    assert mi is not None and mi in ms and mf in ms
    k = int(np.searchsorted(fv.super, n - mi, side="right")) - 1
    assert fv.super[k] < n - mi < fv.super[k + 1] and (n - mf) in set(fv.super[:-1].tolist())
    worst = 0.0
    for m in ms:
        fac = (fv.super, fv.pi, fv.px, fv.s, fv.x, n, m)
        Sc, F = R.schur_restated(*fac), R.trailing_factor(*fac)
        ref = R.dense_schur(M, m)
        assert Sc.shape == ref.shape == (m, m)
        if m == 0:
            continue
        scale = np.abs(ref).max()
        err = max(np.abs(Sc - ref).max(), np.abs(F @ F.T - ref).max()) / scale
        worst = max(worst, err / tol)
        assert err <= tol / 4, (name, beta, m, err, tol)
        assert np.array_equal(F, np.tril(F))
    print(f"{name} beta={beta}: n={n} nsuper={fv.nsuper} m in {ms}: worst err / tol = {worst:.3f}")
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


@pytest.mark.parametrize("name", ["p3d_12_nd", "forest148", "bcsstk01"])
def test_restated_reduce_and_expand_against_dense_algebra(name):
    """G = L22 (inv (L) P B)_S is the condensed right-hand side; with x_S = inv (Sc) G the expansion
    P' inv (L') [Y_I ; L22' x_S] is inv (A) B; and with x_S perturbed by what a caller's coupling K adds, it solves
    the bordered system (A + E_S K E_S') x = B"""
    case = R.CASES[name]()
    S, A, Lf = R.factorized(case, use_gpu=0)
    fv = ch.FactorView(Lf)
    n = case["n"]
    tol = R.tolerance(R.factor_rcond(fv))
    M = R.permuted_dense(case, fv.Perm)
    Ad = R.dense_symmetric(n, case["Lp"], case["Li"], case["Lx"])
    fac = (fv.super, fv.pi, fv.px, fv.s, fv.x)
    Lfull = R.trailing_factor(*fac, n, n)
    B = np.random.default_rng(11).standard_normal((n, 5))
    Xref = np.linalg.solve(Ad, B)
    for m in (1, min(65, n - 1), n // 2, R.m_inside(fv), n):
        F = R.trailing_factor(*fac, n, m)
        Gv, Y = R.reduce_restated(Lfull, F, fv.Perm, B)
        Gref = R.dense_reduce(M, m, B[fv.Perm])
        assert np.abs(Gv - Gref).max() <= tol * np.abs(Gref).max(), (name, m)
        Sc = F @ F.T
        X = R.expand_restated(Lfull, F, fv.Perm, Y, np.linalg.solve(Sc, Gv))
        assert np.abs(X - Xref).max() <= tol * np.abs(Xref).max(), (name, m)
        K = np.diag(1.0 + np.arange(m) % 3)
        X = R.expand_restated(Lfull, F, fv.Perm, Y, np.linalg.solve(Sc + K, Gv))
        Ak = Ad.copy()
        sidx = fv.Perm[n - m:]
        Ak[np.ix_(sidx, sidx)] += K
        Xk = np.linalg.solve(Ak, B)
        assert np.abs(X - Xk).max() <= tol * np.abs(Xk).max(), (name, m)
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def _perm_case():
    n, Ap, Ai, Ax = G.poisson3d(9)
    return n, Ap, Ai, Ax, np.random.default_rng(5).permutation(n)[:40].astype(np.int64)


@pytest.mark.parametrize("stype", [-1, 0])
def test_schur_perm_orders_the_subset_last(stype):
    n, Ap, Ai, Ax, sub = _perm_case()
    S = ch.Session(use_gpu=0, postorder=False)
    if stype == 0:              # an unsymmetric A whose A A' is factorized: both triangles of the Poisson matrix
        import scipy.sparse as sp
        Lo = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
        Mf = sp.csc_matrix(Lo + sp.tril(Lo, -1).T)
        Mf.sort_indices()
        Ap, Ai, Ax = Mf.indptr.astype(np.int64), Mf.indices.astype(np.int64), Mf.data
    A = S.sparse(n, Ap, Ai, Ax, stype)
    p = ch.Session.schur_perm(A, sub)
    m = len(sub)
    assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(n))          # a permutation
    assert np.array_equal(p[n - m:], sub)                                              # its tail: subset in order
    assert set(p[:n - m].tolist()) == set(range(n)) - set(sub.tolist())                # its head orders the complement
    assert not np.array_equal(p[:n - m], np.sort(p[:n - m]))                           # ... by a fill-reducing ordering
    Lf = S.analyze(A, p)
    fv = ch.FactorView(Lf)
    assert set(fv.Perm[n - m:].tolist()) == set(sub.tolist())
    assert np.array_equal(ch.Session.schur_index(Lf, m), fv.Perm[n - m:])
    S.free_factor(Lf)
    # the whole matrix and the empty subset
    assert np.array_equal(ch.Session.schur_perm(A, np.arange(n)[::-1]), np.arange(n)[::-1])
    assert np.array_equal(np.sort(ch.Session.schur_perm(A, [])), np.arange(n))
    # a repeated or out-of-range entry
    for badsub in ([3, 4, 3], [0, n], [-1, 2]):
        with pytest.raises(ValueError):
            ch.Session.schur_perm(A, badsub)
    S.free_sparse(A)
    assert S.cm.malloc_count == 0
    S.finish()
