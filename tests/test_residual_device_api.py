"""The device-resident residual and refinement (cholmod_l_hip_residual_device / cholmod_l_hip_refine_device and the engine's
cholmod_hip_residual_device / cholmod_hip_refine_device): what can be checked without a GPU -- the exported symbols and the
argument checks, which come before the engine or a device is touched.  Integers stand in for device pointers: nothing here
may dereference them."""
import ctypes as C

import numpy as np

from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FAKE_X, FAKE_B, FAKE_R, FAKE_N = 0x1000, 0x2000, 0x3000, 0x4000
NEW = ("cholmod_l_hip_residual_device", "cholmod_l_hip_refine_device", "cholmod_hip_residual_device",
       "cholmod_hip_refine_device")


def test_library_exports_the_device_residual():
    L = ch.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in ch.API_SYMBOLS + ch.HIP_SYMBOLS
    assert callable(ch.Session.residual_device) and callable(ch.Session.refine_device)


def _cpu_factor(numeric=True):
    # golden case p3d_12_nd on the CPU path
    n, Ap, Ai, Ax = G.poisson3d(12)
    perm = G.geometric_nd(12, 12, 12, 4)
    S = ch.Session(use_gpu=0)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    if numeric:
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    return S, A, Lf, n


def _residual(S, Lf, n, X=FAKE_X, ldx=None, B=FAKE_B, ldb=None, R=FAKE_R, ldr=None, nrhs=3):
    S.cm.status = ch.OK
    ok = S.L.cholmod_l_hip_residual_device(Lf, X, n if ldx is None else ldx, B, n if ldb is None else ldb, R,
                                           n if ldr is None else ldr, nrhs, FAKE_N, None, C.byref(S.cm))
    return ok, S.cm.status


def _refine(S, Lf, n, B=FAKE_B, ldb=None, X=FAKE_X, ldx=None, nrhs=3, steps=1):
    S.cm.status = ch.OK
    ok = S.L.cholmod_l_hip_refine_device(Lf, B, n if ldb is None else ldb, X, n if ldx is None else ldx, nrhs, steps,
                                         FAKE_N, None, C.byref(S.cm))
    return ok, S.cm.status


def test_argument_checks_come_before_any_device():
    S, A, Lf, n = _cpu_factor()
    bad = (0, ch.INVALID)
    # NULL pointers
    assert _residual(S, None, n) == bad and _refine(S, None, n) == bad
    for k in ("X", "B", "R"):
        assert _residual(S, Lf, n, **{k: None}) == bad, k
    for k in ("X", "B"):
        assert _refine(S, Lf, n, **{k: None}) == bad, k
    # ld < n
    for k in ("ldx", "ldb", "ldr"):
        assert _residual(S, Lf, n, **{k: n - 1}) == bad, k
    for k in ("ldx", "ldb"):
        assert _refine(S, Lf, n, **{k: n - 1}) == bad, k
    # steps < 0, R == X
    assert _refine(S, Lf, n, steps=-1) == bad
    assert _residual(S, Lf, n, R=FAKE_X) == bad
    # the GPU is off: no host fallback for device pointers, with or without hip_cpu_fallback, whatever nrhs is
    for fb in (0, 1):
        S.cm.hip_cpu_fallback = fb
        for nrhs in (3, 0, 20):
            assert _residual(S, Lf, n, nrhs=nrhs) == bad
            assert _refine(S, Lf, n, nrhs=nrhs) == bad
            assert _refine(S, Lf, n, nrhs=nrhs, steps=0) == bad
    S.cm.hip_cpu_fallback = 0
    # complex / zomplex L
    for xt in (ch.COMPLEX, ch.ZOMPLEX):
        Lf.contents.xtype = xt
        assert _residual(S, Lf, n) == (0, ch.NOT_INSTALLED)
        assert _refine(S, Lf, n) == (0, ch.NOT_INSTALLED)
    Lf.contents.xtype = ch.REAL
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_cpu_path_factor_has_no_resident_matrix():
    """useGPU switched on AFTER a CPU-path factorization: L has values but nothing was factorized on the device, and the
    refusal needs no device"""
    S, A, Lf, n = _cpu_factor()
    S.cm.useGPU = 1
    assert _residual(S, Lf, n) == (0, ch.INVALID)
    assert _refine(S, Lf, n) == (0, ch.INVALID)
    S.cm.useGPU = 0
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_symbolic_factor_is_refused():
    S, A, Lf, n = _cpu_factor(numeric=False)
    assert Lf.contents.xtype == ch.PATTERN
    for gpu in (0, 1):          # ... also with the GPU asked for: the check needs no device
        S.cm.useGPU = gpu
        assert _residual(S, Lf, n) == (0, ch.INVALID)
        assert _refine(S, Lf, n) == (0, ch.INVALID)
    S.cm.useGPU = 0
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def _host_only_plan(lib):
    n, Ap, Ai, Ax = G.poisson3d(5)
    O = OracleFactor(n, Ap, Ai, -1, perm=None, postorder=True)
    keep = [np.ascontiguousarray(getattr(O, k), dtype=np.int64) for k in ("super", "pi", "px", "s")]
    st = C.c_int(0)
    P = lib.cholmod_hip_plan_create(n, len(keep[0]) - 1, *(a.ctypes.data_as(C.c_void_p) for a in keep),
                                    ch.HIP_PLAN_HOST_ONLY, C.byref(st))
    assert P and st.value == 0
    return P, n


def test_engine_refuses_a_host_only_plan_and_bad_arguments():
    lib = ch.lib()
    P, n = _host_only_plan(lib)
    for perm in (0, 1):
        for nrhs in (0, 2, 16):
            assert lib.cholmod_hip_residual_device(P, perm, FAKE_X, n, FAKE_B, n, FAKE_R, n, nrhs, FAKE_N, None) == ch.HIP_INVALID
            assert lib.cholmod_hip_residual_device(P, perm, FAKE_X, n, FAKE_B, n, FAKE_R, n, nrhs, None, None) == ch.HIP_INVALID
            for steps in (0, 1, -1):
                assert lib.cholmod_hip_refine_device(P, perm, FAKE_B, n, FAKE_X, n, nrhs, steps, FAKE_N, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_residual_device(None, 0, FAKE_X, n, FAKE_B, n, FAKE_R, n, 1, None, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_refine_device(None, 0, FAKE_B, n, FAKE_X, n, 1, 1, None, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_residual_device(P, 0, None, n, FAKE_B, n, FAKE_R, n, 1, None, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_residual_device(P, 0, FAKE_X, n, FAKE_B, n, FAKE_X, n, 1, None, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_residual_device(P, 0, FAKE_X, n, FAKE_B, n, FAKE_R, n, -1, None, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_residual_device(P, 0, FAKE_X, n - 1, FAKE_B, n, FAKE_R, n, 1, None, None) == ch.HIP_INVALID
    lib.cholmod_hip_plan_destroy(P)
