"""The device-resident solve (cholmod_l_hip_solve_device / cholmod_hip_solve_device / cholmod_hip_set_perm): what can
be checked without a GPU -- the exported symbols and the argument checks, which come before the engine or a device is
touched.  Integers stand in for device pointers: nothing here may dereference them."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FAKE_B, FAKE_X = 0x1000, 0x2000


def test_library_exports_the_device_solve():
    L = ch.lib()
    for name in ("cholmod_l_hip_solve_device", "cholmod_hip_solve_device", "cholmod_hip_set_perm"):
        assert hasattr(L, name), name
        assert name in ch.API_SYMBOLS + ch.HIP_SYMBOLS


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


def _call(S, Lf, sys=ch.SYS_A, B=FAKE_B, ldb=None, X=FAKE_X, ldx=None, nrhs=3, n=0):
    S.cm.status = ch.OK
    ok = S.L.cholmod_l_hip_solve_device(sys, Lf, B, n if ldb is None else ldb, X, n if ldx is None else ldx, nrhs, None,
                                        C.byref(S.cm))
    return ok, S.cm.status


def test_argument_checks_come_before_any_device():
    S, A, Lf, n = _cpu_factor()
    # NULL pointers
    assert _call(S, None, n=n) == (0, ch.INVALID)
    assert _call(S, Lf, B=None, n=n) == (0, ch.INVALID)
    assert _call(S, Lf, X=None, n=n) == (0, ch.INVALID)
    # sys out of range
    assert _call(S, Lf, sys=-1, n=n) == (0, ch.INVALID)
    assert _call(S, Lf, sys=9, n=n) == (0, ch.INVALID)
    # ld < n
    assert _call(S, Lf, ldb=n - 1, n=n) == (0, ch.INVALID)
    assert _call(S, Lf, ldx=n - 1, n=n) == (0, ch.INVALID)
    # the GPU is off: no silent host fallback for device pointers, with or without hip_cpu_fallback
    for sys in range(9):
        assert _call(S, Lf, sys=sys, n=n) == (0, ch.INVALID)
    S.cm.hip_cpu_fallback = 1
    assert _call(S, Lf, n=n) == (0, ch.INVALID)
    assert _call(S, Lf, nrhs=0, n=n) == (0, ch.INVALID)
    S.cm.hip_cpu_fallback = 0
    # complex / zomplex L
    for xt in (ch.COMPLEX, ch.ZOMPLEX):
        Lf.contents.xtype = xt
        assert _call(S, Lf, n=n) == (0, ch.NOT_INSTALLED)
    Lf.contents.xtype = ch.REAL
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_symbolic_factor_is_refused():
    S, A, Lf, n = _cpu_factor(numeric=False)
    assert Lf.contents.xtype == ch.PATTERN
    assert _call(S, Lf, n=n) == (0, ch.INVALID)
    # ... also with the GPU asked for: the check needs no device
    S.cm.useGPU = 1
    assert _call(S, Lf, n=n) == (0, ch.INVALID)
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
    for which in range(4):
        assert lib.cholmod_hip_solve_device(P, which, 0, 0, FAKE_B, n, FAKE_X, n, 2, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_solve_device(P, 0, 1, 1, FAKE_B, n, FAKE_X, n, 0, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_solve_device(None, 0, 0, 0, FAKE_B, n, FAKE_X, n, 1, None) == ch.HIP_INVALID
    lib.cholmod_hip_plan_destroy(P)


def test_set_perm_rejects_what_is_not_a_permutation():
    lib = ch.lib()
    P, n = _host_only_plan(lib)
    ok = np.arange(n, dtype=np.int64)[::-1].copy()
    for bad in (n, -1, 1 << 40):
        p = ok.copy()
        p[3] = bad                              # out of range
        assert lib.cholmod_hip_set_perm(P, p.ctypes.data) == ch.HIP_INVALID
    p = ok.copy()
    p[7] = p[2]                                 # duplicate (and so one index missing)
    assert lib.cholmod_hip_set_perm(P, p.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_set_perm(P, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_set_perm(None, ok.ctypes.data) == ch.HIP_INVALID
    # a permutation passes the validation; a host-only plan then has no device to store it on
    assert lib.cholmod_hip_set_perm(P, ok.ctypes.data) == ch.HIP_NO_DEVICE
    lib.cholmod_hip_plan_destroy(P)
