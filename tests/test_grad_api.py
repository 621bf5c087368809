"""Gradients through the device path (cholmod_l_hip_values_grad_device / cholmod_l_hip_logdet_device and the engine's
cholmod_hip_values_grad_device / cholmod_hip_logdet_device): what can be checked without a GPU -- the exported symbols,
the argument checks, which come before the engine or a device is touched (integers stand in for device pointers: nothing
here may dereference them), and the numpy formulas of tests/grad_reference.py, which must hold the bars of the GPU test
against dense torch autograd themselves."""
import ctypes as C

import numpy as np
import pytest

import grad_reference as GR
import selinv_reference as R
from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FAKE_U, FAKE_V, FAKE_G = 0x1000, 0x2000, 0x3000
NEW = ("cholmod_hip_values_grad_device", "cholmod_hip_logdet_device", "cholmod_l_hip_values_grad_device",
       "cholmod_l_hip_logdet_device")


def test_library_exports_the_gradient_entry_points():
    for L in (ch.lib(), ch.lib(hooks=True)):
        for name in NEW:
            assert hasattr(L, name), name
            assert name in ch.API_SYMBOLS + ch.HIP_SYMBOLS
    assert callable(ch.Session.values_grad_device) and callable(ch.Session.logdet_device)


def _cpu_factor(numeric=True):
    case = R.CASES["p3d_12_nd"]()
    S = ch.Session(use_gpu=0)
    A = S.sparse(case["n"], case["Lp"], case["Li"], case["Lx"], -1)
    Lf = S.analyze(A, case["perm"])
    if numeric:
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    return S, A, Lf


def _grad(S, A, Lf, U=FAKE_U, V=FAKE_V, Gp=FAKE_G, ld=None, nrhs=3):
    S.cm.status = ch.OK
    n = int(Lf.contents.n) if Lf else 0
    ld = n if ld is None else ld
    return S.L.cholmod_l_hip_values_grad_device(A, Lf, -1.0, U, ld, V, ld, nrhs, Gp, None, C.byref(S.cm)), S.cm.status


def _logdet(S, Lf, out=FAKE_G):
    S.cm.status = ch.OK
    return S.L.cholmod_l_hip_logdet_device(Lf, out, None, C.byref(S.cm)), S.cm.status


def test_argument_checks_come_before_any_device():
    S, A, Lf = _cpu_factor()
    S.cm.error_handler = ch.ERRFUNC(0)
    bad = (0, ch.INVALID)
    n = int(Lf.contents.n)
    # NULL pointers
    assert _grad(S, None, Lf) == bad and _grad(S, A, None) == bad
    assert _grad(S, A, Lf, U=None) == bad and _grad(S, A, Lf, V=None) == bad and _grad(S, A, Lf, Gp=None) == bad
    assert _logdet(S, None) == bad and _logdet(S, Lf, out=None) == bad
    # the GPU is off: no host fallback, with or without hip_cpu_fallback
    for fb in (0, 1):
        S.cm.hip_cpu_fallback = fb
        assert _grad(S, A, Lf) == bad and _logdet(S, Lf) == bad
    S.cm.hip_cpu_fallback = 0
    for gpu in (0, 1):          # ... the rest also with the GPU asked for: no check needs a device
        S.cm.useGPU = gpu
        # a CPU-path factor was not factorized on the device
        assert _grad(S, A, Lf) == bad and _logdet(S, Lf) == bad
        # a leading dimension smaller than n
        assert _grad(S, A, Lf, ld=n - 1) == bad
        # L->minor < n: the log-determinant
        Lf.contents.minor = n - 1
        assert _logdet(S, Lf) == bad
        Lf.contents.minor = n
        # complex / zomplex L or A
        for xt in (ch.COMPLEX, ch.ZOMPLEX):
            Lf.contents.xtype = xt
            assert _grad(S, A, Lf) == (0, ch.NOT_INSTALLED) and _logdet(S, Lf) == (0, ch.NOT_INSTALLED)
            Lf.contents.xtype = ch.REAL
            A.contents.xtype = xt
            assert _grad(S, A, Lf) == (0, ch.NOT_INSTALLED)
            A.contents.xtype = ch.REAL
        # an unsymmetric, an unpacked, a mismatched A
        A.contents.stype = 0
        assert _grad(S, A, Lf) == bad
        A.contents.stype = -1
        A.contents.packed = 0
        assert _grad(S, A, Lf) == bad
        A.contents.packed = 1
        A.contents.nrow -= 1
        assert _grad(S, A, Lf) == bad
        A.contents.nrow += 1
        # several ranks
        S.cm.hip_world = 2
        assert _grad(S, A, Lf) == bad and _logdet(S, Lf) == bad
        S.cm.hip_world = 1
    S.cm.useGPU = 0
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def test_symbolic_factor_is_refused():
    S, A, Lf = _cpu_factor(numeric=False)
    S.cm.error_handler = ch.ERRFUNC(0)
    assert Lf.contents.xtype == ch.PATTERN
    for gpu in (0, 1):
        S.cm.useGPU = gpu
        assert _grad(S, A, Lf) == (0, ch.INVALID)
        assert _logdet(S, Lf) == (0, ch.INVALID)
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
        for perm in (0, 1):
            assert lib.cholmod_hip_values_grad_device(plan, perm, -1.0, FAKE_U, n, FAKE_V, n, 3, FAKE_G, len(Ai), None) == ch.HIP_INVALID
        assert lib.cholmod_hip_logdet_device(plan, FAKE_G, None) == ch.HIP_INVALID
    lib.cholmod_hip_plan_destroy(P)


def test_formulas_on_a_hand_example():
    """3 x 3, lower-stored with one entry in the ignored triangle: the sampled product by hand, +0.0 where A is not read"""
    Ap, Ai = np.array([0, 2, 4, 5]), np.array([0, 2, 0, 1, 2])          # (0,0) (2,0) | (0,1): ignored, (1,1) | (2,2)
    U, V = np.array([[1.0, 2.0, 3.0], [0.0, -1.0, 2.0]]), np.array([[4.0, 5.0, 6.0], [1.0, 1.0, -2.0]])
    Gv = GR.values_grad(Ap, Ai, -1, U, V, -1.0)
    want = -np.array([1 * 4 + 0 * 1, (3 * 4 + 1 * 6) + (2 * 1 + 0 * -2), 0.0, 2 * 5 + -1 * 1, 3 * 6 + 2 * -2])
    assert np.array_equal(Gv, want) and not np.signbit(Gv[2])
    assert np.array_equal(GR.logdet_multiplier(Ap, Ai, -1), [1, 2, 0, 1, 1])
    assert np.array_equal(GR.values_grad_magnitude(Ap, Ai, U, V)[1], (3 * 4 + 1 * 6) + (2 * 1 + 0 * 2))


@pytest.mark.parametrize("nrhs", [1, 19])
@pytest.mark.parametrize("beta", [0.0, 0.375])
@pytest.mark.parametrize("name", ["p3d_12_nd", "arrow300", "forest148", "bcsstk02", "dense200"])
def test_formulas_against_dense_torch_autograd(name, beta, nrhs):
    """the numpy restatement of the backward pass holds the bars the device is held to, against dense torch autograd"""
    case = R.CASES[name]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    B, W = GR.inputs(n, nrhs, 7)
    ref = GR.torch_reference(n, Ap, Ai, Ax, -1, beta, B, W)
    gv, gb = GR.loss_gradients(n, Ap, Ai, Ax, -1, beta, B, W)
    S, A, Lf = R.factorized(case, use_gpu=0, beta=beta)
    tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
    bar_v, bar_b = GR.bars(ref, tol, nrhs)
    ev, eb = np.abs(gv - ref["grad_values"]).max(), np.abs(gb - ref["grad_B"]).max()
    print(f"{name} beta={beta} nrhs={nrhs}: grad_values {ev:.2e} (bar {bar_v:.2e}), grad_B {eb:.2e} (bar {bar_b:.2e})")
    assert ev <= bar_v and eb <= bar_b, (ev, bar_v, eb, bar_b)
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()
