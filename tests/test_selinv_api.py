"""The selected inverse (cholmod_l_hip_selinv_device / cholmod_l_hip_selinv_to_host and the engine's cholmod_hip_selinv_*):
what can be checked without a GPU -- the exported symbols, the argument checks, which come before the engine or a device is
touched (integers stand in for device pointers: nothing here may dereference them), and the numpy restatement of the
recurrence (tests/selinv_reference.py), which must hold the bar of the GPU test against the dense inverse itself."""
import ctypes as C

import numpy as np
import pytest

import selinv_reference as R
from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FAKE_Z, FAKE_D = 0x1000, 0x2000
NEW = ("cholmod_hip_selinv_device", "cholmod_hip_selinv_gather_device", "cholmod_hip_selinv_download",
       "cholmod_hip_selinv_release", "cholmod_hip_selinv_info", "cholmod_l_hip_selinv_device", "cholmod_l_hip_selinv_to_host")


def test_library_exports_the_selected_inverse():
    for L in (ch.lib(), ch.lib(hooks=True)):
        for name in NEW:
            assert hasattr(L, name), name
            assert name in ch.API_SYMBOLS + ch.HIP_SYMBOLS
    assert callable(ch.Session.selinv_device) and callable(ch.Session.selinv_host)


def _cpu_factor(numeric=True):
    case = R.CASES["p3d_12_nd"]()
    S = ch.Session(use_gpu=0)
    A = S.sparse(case["n"], case["Lp"], case["Li"], case["Lx"], -1)
    Lf = S.analyze(A, case["perm"])
    if numeric:
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    return S, A, Lf


def _device(S, A, Lf, Z=FAKE_Z, D=FAKE_D):
    S.cm.status = ch.OK
    return S.L.cholmod_l_hip_selinv_device(A, Lf, Z, D, None, C.byref(S.cm)), S.cm.status


def _host(S, Lf, out):
    S.cm.status = ch.OK
    return S.L.cholmod_l_hip_selinv_to_host(Lf, out, C.byref(S.cm)), S.cm.status


def test_argument_checks_come_before_any_device():
    S, A, Lf = _cpu_factor()
    S.cm.error_handler = ch.ERRFUNC(0)
    out = np.zeros(int(Lf.contents.xsize))
    bad = (0, ch.INVALID)
    # NULL pointers, both outputs NULL, Z_dev without A
    assert _device(S, A, None) == bad and _host(S, None, out.ctypes.data) == bad and _host(S, Lf, None) == bad
    assert _device(S, A, Lf, Z=None, D=None) == bad
    assert _device(S, None, Lf) == bad
    # the GPU is off: no host fallback, with or without hip_cpu_fallback, with and without A
    for fb in (0, 1):
        S.cm.hip_cpu_fallback = fb
        assert _device(S, A, Lf) == bad and _device(S, None, Lf, Z=None) == bad and _device(S, A, Lf, D=None) == bad
        assert _host(S, Lf, out.ctypes.data) == bad
    S.cm.hip_cpu_fallback = 0
    for gpu in (0, 1):          # ... the rest also with the GPU asked for: no check needs a device
        S.cm.useGPU = gpu
        # a CPU-path factor was not factorized on the device
        assert _device(S, A, Lf) == bad and _host(S, Lf, out.ctypes.data) == bad
        # L->minor < n
        n = Lf.contents.minor
        Lf.contents.minor = n - 1
        assert _device(S, None, Lf, Z=None) == bad and _host(S, Lf, out.ctypes.data) == bad
        Lf.contents.minor = n
        # complex / zomplex L or A
        for xt in (ch.COMPLEX, ch.ZOMPLEX):
            Lf.contents.xtype = xt
            assert _device(S, A, Lf) == (0, ch.NOT_INSTALLED) and _host(S, Lf, out.ctypes.data) == (0, ch.NOT_INSTALLED)
            Lf.contents.xtype = ch.REAL
            A.contents.xtype = xt
            assert _device(S, A, Lf) == (0, ch.NOT_INSTALLED)
            A.contents.xtype = ch.REAL
        # Z_dev with an unsymmetric, an unpacked, a mismatched A
        A.contents.stype = 0
        assert _device(S, A, Lf) == bad
        A.contents.stype = -1
        A.contents.packed = 0
        assert _device(S, A, Lf) == bad
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
        assert _device(S, A, Lf) == (0, ch.INVALID)
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
        assert lib.cholmod_hip_selinv_device(plan, None) == ch.HIP_INVALID
        assert lib.cholmod_hip_selinv_gather_device(plan, FAKE_Z, 10, FAKE_D, 0, None) == ch.HIP_INVALID
        assert lib.cholmod_hip_selinv_download(plan, FAKE_Z) == ch.HIP_INVALID
        assert lib.cholmod_hip_selinv_release(plan) == ch.HIP_INVALID
        assert lib.cholmod_hip_selinv_info(plan, out8.ctypes.data) == ch.HIP_INVALID
    assert np.all(out8 == 7.0)
    lib.cholmod_hip_plan_destroy(P)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_against_the_dense_inverse(name):
    """the numpy restatement on the CPU path's factor holds the bar the device is held to: max |Z - Z_ref| over the stored
    lower trapezoids within max (1e-12, 20 eps / rcond) max |Z_ref|, the dead upper triangles exact zeros"""
    case = R.CASES[name]()
    S, A, Lf = R.factorized(case, use_gpu=0)
    fv = ch.FactorView(Lf)
    Zx = R.selinv_reference(fv.super, fv.pi, fv.px, fv.s, fv.x)
    err, tol, dead = R.compare(fv, Zx, case["n"], case["Lp"], case["Li"], case["Lx"])
    print(f"{name}: n={case['n']} nsuper={fv.nsuper} err={err:.2e} tol={tol:.2e}")
    assert err <= tol and dead == 0, (err, tol, dead)
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()
