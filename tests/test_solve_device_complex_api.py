"""The device-resident solve, residual and refinement for complex factors (cholmod_l_hip_solve_device_complex,
cholmod_l_hip_residual_device_complex, cholmod_l_hip_refine_device_complex): what can be checked without a GPU -- the
exported symbols and the refusals, all of which come before the engine or a device is touched.  Integers stand in for
device pointers: nothing here may dereference them."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FAKE_X, FAKE_B, FAKE_R, FAKE_N = 0x1000, 0x2000, 0x3000, 0x4000
NEW = ("cholmod_l_hip_solve_device_complex", "cholmod_l_hip_residual_device_complex",
       "cholmod_l_hip_refine_device_complex")
HIP_CX_STORAGE = 32768      # CHOLMOD_HIP_CX_STORAGE (include/cholmod_hip.h)


def test_library_exports_the_complex_device_entry_points():
    L = ch.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in ch.API_SYMBOLS
        assert getattr(L, name).argtypes is not None, name          # ... and has a signature


def hermitian_from(n, Ap, Ai, Ax, seed=0, scale=0.9):
    """(a copy of the helper of tests/test_complex.py) a Hermitian positive definite matrix on the pattern of a real SPD
    one: every off-diagonal entry is turned by a random phase and shrunk.  Lower-stored CSC, sorted."""
    rng = np.random.default_rng(seed)
    Al = sp.tril(sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))).tocsc()
    Al.sort_indices()
    vals = Al.data.astype(np.complex128)
    off = Al.indices != np.repeat(np.arange(n), np.diff(Al.indptr))
    vals[off] *= scale * np.exp(1j * rng.uniform(0, 2 * np.pi, int(off.sum())))
    return Al.indptr.astype(np.int64), Al.indices.astype(np.int64), vals


def _cpu_factor(kind="complex", numeric=True):
    """p3d_9_nd on the CPU path: a complex factor (its twin has no plan and nothing on a device), or a real one"""
    n, Ap, Ai, Ax = G.poisson3d(9)
    perm = G.geometric_nd(9, 9, 9, 3)
    if kind == "complex":
        Ap, Ai, Ax = hermitian_from(n, Ap, Ai, Ax)
    S = ch.Session(use_gpu=0)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    if numeric:
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        assert Lf.contents.xtype == (ch.COMPLEX if kind == "complex" else ch.REAL)
    return S, A, Lf, n


def _solve(S, Lf, n, sys=ch.SYS_A, B=FAKE_B, ldb=None, X=FAKE_X, ldx=None, nrhs=3):
    S.cm.status = ch.OK
    ok = S.L.cholmod_l_hip_solve_device_complex(sys, Lf, B, n if ldb is None else ldb, X, n if ldx is None else ldx, nrhs,
                                                None, C.byref(S.cm))
    return ok, S.cm.status


def _residual(S, Lf, n, X=FAKE_X, ldx=None, B=FAKE_B, ldb=None, R=FAKE_R, ldr=None, nrhs=3):
    S.cm.status = ch.OK
    ok = S.L.cholmod_l_hip_residual_device_complex(Lf, X, n if ldx is None else ldx, B, n if ldb is None else ldb, R,
                                                   n if ldr is None else ldr, nrhs, FAKE_N, None, C.byref(S.cm))
    return ok, S.cm.status


def _refine(S, Lf, n, B=FAKE_B, ldb=None, X=FAKE_X, ldx=None, nrhs=3, steps=1):
    S.cm.status = ch.OK
    ok = S.L.cholmod_l_hip_refine_device_complex(Lf, B, n if ldb is None else ldb, X, n if ldx is None else ldx, nrhs,
                                                 steps, FAKE_N, None, C.byref(S.cm))
    return ok, S.cm.status


def _all_three(S, Lf, n, **kw):
    return {_solve(S, Lf, n, **kw), _residual(S, Lf, n, **kw), _refine(S, Lf, n, **kw)}


def _done(S, A, Lf):
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_argument_checks_come_before_any_device():
    S, A, Lf, n = _cpu_factor()
    bad = (0, ch.INVALID)
    # NULL pointers
    assert _all_three(S, None, n) == {bad}
    for k in ("X", "B"):
        assert _solve(S, Lf, n, **{k: None}) == bad, k
        assert _refine(S, Lf, n, **{k: None}) == bad, k
    for k in ("X", "B", "R"):
        assert _residual(S, Lf, n, **{k: None}) == bad, k
    # sys out of range
    for sys in (-1, 9):
        assert _solve(S, Lf, n, sys=sys) == bad
    # ld < n (in complex elements)
    for k in ("ldx", "ldb"):
        assert _all_three(S, Lf, n, **{k: n - 1}) == {bad}, k
    assert _residual(S, Lf, n, ldr=n - 1) == bad
    # steps < 0, R == X
    assert _refine(S, Lf, n, steps=-1) == bad
    assert _residual(S, Lf, n, R=FAKE_X) == bad
    # the GPU is off: never a host fallback for device pointers, with or without hip_cpu_fallback, whatever nrhs is
    for fb in (0, 1):
        S.cm.hip_cpu_fallback = fb
        for sys in range(9):
            assert _solve(S, Lf, n, sys=sys) == bad
        for nrhs in (3, 0, 20):
            assert _all_three(S, Lf, n, nrhs=nrhs) == {bad}
            assert _refine(S, Lf, n, nrhs=nrhs, steps=0) == bad
    S.cm.hip_cpu_fallback = 0
    # zomplex L
    Lf.contents.xtype = ch.ZOMPLEX
    assert _all_three(S, Lf, n) == {(0, ch.NOT_INSTALLED)}
    Lf.contents.xtype = ch.COMPLEX
    # a simplicial L
    Lf.contents.is_super = 0
    assert _all_three(S, Lf, n) == {bad}
    Lf.contents.is_super = 1
    _done(S, A, Lf)


def test_cpu_path_complex_factor_has_no_twin_on_the_device():
    """useGPU switched on AFTER a CPU-path factorization: the complex L has values and a twin, but the twin has no plan
    and nothing in HBM; several ranks are refused as well.  The refusals need no device."""
    S, A, Lf, n = _cpu_factor()
    S.cm.useGPU = 1
    assert Lf.contents.cx_twin
    T = C.cast(Lf.contents.cx_twin, C.POINTER(ch.Factor))
    assert not T.contents.hip_plan
    assert _all_three(S, Lf, n) == {(0, ch.INVALID)}
    assert _all_three(S, Lf, n, nrhs=0) == {(0, ch.INVALID)}
    S.cm.hip_world = 2
    assert _all_three(S, Lf, n) == {(0, ch.INVALID)}
    S.cm.hip_world = 1
    S.cm.useGPU = 0
    _done(S, A, Lf)


def test_real_factor_is_refused():
    """a real L has the real entry points"""
    S, A, Lf, n = _cpu_factor(kind="real")
    for gpu in (0, 1):
        S.cm.useGPU = gpu
        assert _all_three(S, Lf, n) == {(0, ch.INVALID)}
    S.cm.useGPU = 0
    _done(S, A, Lf)


def test_symbolic_factor_is_refused():
    for kind in ("complex", "real"):
        S, A, Lf, n = _cpu_factor(kind=kind, numeric=False)
        assert Lf.contents.xtype == ch.PATTERN
        for gpu in (0, 1):          # ... also with the GPU asked for: the check needs no device
            S.cm.useGPU = gpu
            assert _all_three(S, Lf, n) == {(0, ch.INVALID)}
        S.cm.useGPU = 0
        _done(S, A, Lf)


def _host_only_twin_plan(lib, flags):
    """a host-only plan on the doubled structure of a twin (4 x px: the full twin; 2 x px: complex storage)"""
    n, Ap, Ai, Ax = G.poisson3d(5)
    O = OracleFactor(n, Ap, Ai, -1, perm=None, postorder=True)
    sup, pi, px, s = (np.ascontiguousarray(getattr(O, k), dtype=np.int64) for k in ("super", "pi", "px", "s"))
    s2 = np.empty(2 * len(s), dtype=np.int64)
    s2[0::2] = 2 * s
    s2[1::2] = 2 * s + 1
    keep = [2 * sup, 2 * pi, (2 if flags & HIP_CX_STORAGE else 4) * px, s2]
    st = C.c_int(0)
    P = lib.cholmod_hip_plan_create(2 * n, len(sup) - 1, *(a.ctypes.data_as(C.c_void_p) for a in keep),
                                    ch.HIP_PLAN_HOST_ONLY | flags, C.byref(st))
    assert P and st.value == 0, st.value
    return P, 2 * n


def test_complex_storage_plan_with_an_odd_bound_is_refused_at_plan_time():
    """the solve kernels in complex storage read row r ^ 1 of a row r and rely on even bounds: a structure that is not a
    twin's (odd supernode widths and row counts) never becomes a plan"""
    lib = ch.lib()
    n, Ap, Ai, Ax = G.poisson3d(5)
    O = OracleFactor(n, Ap, Ai, -1, perm=None, postorder=True)
    keep = [np.ascontiguousarray(getattr(O, k), dtype=np.int64) for k in ("super", "pi", "px", "s")]
    assert (np.diff(keep[0]) % 2).any()
    st = C.c_int(0)
    P = lib.cholmod_hip_plan_create(n, len(keep[0]) - 1, *(a.ctypes.data_as(C.c_void_p) for a in keep),
                                    ch.HIP_PLAN_HOST_ONLY | HIP_CX_STORAGE, C.byref(st))
    assert not P and st.value == ch.HIP_INVALID


def test_engine_still_refuses_a_host_only_plan():
    """the engine entry points now serve the plans of complex factors, but not one without a device"""
    lib = ch.lib()
    for flags in (ch.HIP_PHI_TWIN, HIP_CX_STORAGE):
        P, n = _host_only_twin_plan(lib, flags)
        for nrhs in (0, 2, 16):
            for which in range(4):
                assert lib.cholmod_hip_solve_device(P, which, 0, 0, FAKE_B, n, FAKE_X, n, nrhs, None) == ch.HIP_INVALID
            for perm in (0, 1):
                assert lib.cholmod_hip_residual_device(P, perm, FAKE_X, n, FAKE_B, n, FAKE_R, n, nrhs, FAKE_N, None) == ch.HIP_INVALID
                for steps in (0, 1):
                    assert lib.cholmod_hip_refine_device(P, perm, FAKE_B, n, FAKE_X, n, nrhs, steps, FAKE_N, None) == ch.HIP_INVALID
        lib.cholmod_hip_plan_destroy(P)
