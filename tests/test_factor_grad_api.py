"""The gradient through the factor (cholmod_l_hip_factor_grad_device / _outer_grad_device / _to_host and the engine's
cholmod_hip_factor_grad_*): what can be checked without a GPU -- the exported symbols, the argument checks, which come
before the engine or a device is touched (integers stand in for device pointers: nothing here may dereference them), and
the numpy restatement of the recurrence (tests/factor_grad_reference.py), which must hold the bar of the GPU test against
the dense formula of reverse-mode Cholesky itself."""
import ctypes as C

import numpy as np
import pytest

import factor_grad_reference as F
import selinv_reference as R
from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FAKE_L, FAKE_G, FAKE_T = 0x1000, 0x2000, 0x3000
NEW_HIP = ("cholmod_hip_factor_grad_device", "cholmod_hip_factor_outer_grad_device", "cholmod_hip_factor_grad_gather_device",
           "cholmod_hip_factor_grad_download", "cholmod_hip_factor_grad_release", "cholmod_hip_factor_grad_info")
NEW_API = ("cholmod_l_hip_factor_grad_device", "cholmod_l_hip_factor_outer_grad_device", "cholmod_l_hip_factor_grad_to_host")


def test_library_exports_the_factor_gradient():
    for L in (ch.lib(), ch.lib(hooks=True)):
        for name in NEW_HIP + NEW_API:
            assert hasattr(L, name), name
    assert all(name in ch.HIP_SYMBOLS for name in NEW_HIP) and all(name in ch.API_SYMBOLS for name in NEW_API)
    for name in ("factor_grad_device", "factor_outer_grad_device", "factor_grad_host"):
        assert callable(getattr(ch.Session, name))
    from suitesparse_amd.autograd import DeviceCholesky
    assert callable(DeviceCholesky.solve_Lt) and callable(DeviceCholesky.solve_L)


def _cpu_factor(numeric=True):
    case = R.CASES["p3d_12_nd"]()
    S = ch.Session(use_gpu=0)
    A = S.sparse(case["n"], case["Lp"], case["Li"], case["Lx"], -1)
    Lf = S.analyze(A, case["perm"])
    if numeric:
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    return S, A, Lf


def _grad(S, A, Lf, Lbar=FAKE_L, Gd=FAKE_G, T=FAKE_T):
    S.cm.status = ch.OK
    return S.L.cholmod_l_hip_factor_grad_device(A, Lf, Lbar, Gd, T, None, C.byref(S.cm)), S.cm.status


def _outer(S, A, Lf, P=FAKE_L, Q=FAKE_L, ld=None, Gd=FAKE_G, T=FAKE_T):
    S.cm.status = ch.OK
    ld = int(Lf.contents.n) if ld is None and Lf else (ld or 0)
    return S.L.cholmod_l_hip_factor_outer_grad_device(A, Lf, -1.0, P, ld, Q, ld, 3, Gd, T, None, C.byref(S.cm)), S.cm.status


def _host(S, Lf, out):
    S.cm.status = ch.OK
    return S.L.cholmod_l_hip_factor_grad_to_host(Lf, out, C.byref(S.cm)), S.cm.status


def test_argument_checks_come_before_any_device():
    S, A, Lf = _cpu_factor()
    S.cm.error_handler = ch.ERRFUNC(0)
    out = np.zeros(int(Lf.contents.xsize))
    bad = (0, ch.INVALID)
    # NULL pointers; G_dev without A; a leading dimension smaller than n
    assert _grad(S, A, None) == bad and _grad(S, A, Lf, Lbar=None) == bad and _grad(S, None, Lf) == bad
    assert _outer(S, A, None) == bad and _outer(S, A, Lf, P=None) == bad and _outer(S, A, Lf, Q=None) == bad
    assert _outer(S, None, Lf) == bad and _outer(S, A, Lf, ld=int(Lf.contents.n) - 1) == bad
    assert _host(S, None, out.ctypes.data) == bad and _host(S, Lf, None) == bad
    # the GPU is off: no host fallback, with or without hip_cpu_fallback, with and without A
    for fb in (0, 1):
        S.cm.hip_cpu_fallback = fb
        assert _grad(S, A, Lf) == bad and _grad(S, None, Lf, Gd=None) == bad and _outer(S, A, Lf) == bad
        assert _host(S, Lf, out.ctypes.data) == bad
    S.cm.hip_cpu_fallback = 0
    for gpu in (0, 1):          # ... the rest also with the GPU asked for: no check needs a device
        S.cm.useGPU = gpu
        # a CPU-path factor was not factorized on the device
        assert _grad(S, A, Lf) == bad and _outer(S, A, Lf) == bad and _host(S, Lf, out.ctypes.data) == bad
        # L->minor < n
        n = Lf.contents.minor
        Lf.contents.minor = n - 1
        assert _grad(S, None, Lf, Gd=None) == bad and _outer(S, A, Lf) == bad and _host(S, Lf, out.ctypes.data) == bad
        Lf.contents.minor = n
        # complex / zomplex L or A
        for xt in (ch.COMPLEX, ch.ZOMPLEX):
            ni = (0, ch.NOT_INSTALLED)
            Lf.contents.xtype = xt
            assert _grad(S, A, Lf) == ni and _outer(S, A, Lf) == ni and _host(S, Lf, out.ctypes.data) == ni
            Lf.contents.xtype = ch.REAL
            A.contents.xtype = xt
            assert _grad(S, A, Lf) == ni and _outer(S, A, Lf) == ni
            A.contents.xtype = ch.REAL
        # G_dev with an unsymmetric, an unpacked A
        A.contents.stype = 0
        assert _grad(S, A, Lf) == bad and _outer(S, A, Lf) == bad
        A.contents.stype = -1
        A.contents.packed = 0
        assert _grad(S, A, Lf) == bad and _outer(S, A, Lf) == bad
        A.contents.packed = 1
    S.cm.useGPU = 0
    assert np.all(out == 0)
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_symbolic_factor_is_refused():
    S, A, Lf = _cpu_factor(numeric=False)
    S.cm.error_handler = ch.ERRFUNC(0)
    assert Lf.contents.xtype == ch.PATTERN
    out = np.zeros(max(int(Lf.contents.xsize), 1))
    for gpu in (0, 1):
        S.cm.useGPU = gpu
        assert _grad(S, A, Lf) == (0, ch.INVALID) and _outer(S, A, Lf) == (0, ch.INVALID)
        assert _host(S, Lf, out.ctypes.data) == (0, ch.INVALID)
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
    out8 = np.full(8, 7.0)
    for plan in (P, None):
        assert lib.cholmod_hip_factor_grad_device(plan, FAKE_L, None) == ch.HIP_INVALID
        assert lib.cholmod_hip_factor_outer_grad_device(plan, -1.0, FAKE_L, n, FAKE_L, n, 1, None) == ch.HIP_INVALID
        assert lib.cholmod_hip_factor_grad_gather_device(plan, FAKE_G, 10, FAKE_T, None) == ch.HIP_INVALID
        assert lib.cholmod_hip_factor_grad_download(plan, FAKE_G) == ch.HIP_INVALID
        assert lib.cholmod_hip_factor_grad_release(plan) == ch.HIP_INVALID
        assert lib.cholmod_hip_factor_grad_info(plan, out8.ctypes.data) == ch.HIP_INVALID
    assert np.all(out8 == 7.0)
    lib.cholmod_hip_plan_destroy(P)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_against_the_dense_formula(name):
    """the numpy restatement on the CPU path's factor, for a seeded random Lbar, holds the bar the device is held to:
    max |G - G_ref| over the stored lower trapezoids within max (1e-12, 20 eps / rcond) max |G_ref| of the dense formula, the
    dead upper triangles exact zeros whatever stands there in Lbar"""
    case = R.CASES[name]()
    S, A, Lf = R.factorized(case, use_gpu=0)
    fv = ch.FactorView(Lf)
    Lbar_x, mask = F.random_lbar(fv, 7, dead=1e30)
    Gx = F.factor_grad_reference(fv.super, fv.pi, fv.px, fv.s, fv.x, Lbar_x)
    Gd = F.dense_factor_grad(F.dense_factor(fv), F.dense_of_layout(fv, Lbar_x))
    ref, mask2 = F.trapezoid_of(Gd, fv.super, fv.pi, fv.px, fv.s, fv.xsize)
    assert np.array_equal(mask, mask2)
    err = float(np.abs(Gx[mask] - ref[mask]).max() / np.abs(ref[mask]).max())
    tol = R.tolerance(R.factor_rcond(fv))
    print(f"{name}: n={case['n']} nsuper={fv.nsuper} err={err:.2e} tol={tol:.2e}")
    assert err <= tol and np.count_nonzero(Gx[~mask]) == 0, (err, tol)
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_selected_inverse_is_the_special_case():
    """Lbar = diag (2 / L_jj) gives Z on the diagonal and 2 Z off it: the two restatements agree"""
    case = R.CASES["p3d_9_random_nopost"]()
    S, A, Lf = R.factorized(case, use_gpu=0)
    fv = ch.FactorView(Lf)
    Lbar_x = np.zeros(fv.xsize)
    for k in range(fv.nsuper):
        nsrow, nscol = int(fv.pi[k + 1] - fv.pi[k]), int(fv.super[k + 1] - fv.super[k])
        d = int(fv.px[k]) + (nsrow + 1) * np.arange(nscol)
        Lbar_x[d] = 2.0 / fv.x[d]
    Gx = F.factor_grad_reference(fv.super, fv.pi, fv.px, fv.s, fv.x, Lbar_x)
    Zx = R.selinv_reference(fv.super, fv.pi, fv.px, fv.s, fv.x)
    m = np.full(fv.xsize, 2.0)
    m[np.nonzero(Lbar_x)[0]] = 1.0
    err = float(np.abs(Gx - m * Zx).max() / np.abs(Zx).max())
    assert err <= R.tolerance(R.factor_rcond(fv)), err
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()
