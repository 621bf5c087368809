"""Gradients through A*A' + beta*I and with respect to beta (cholmod_l_hip_aat_values_grad_device /
cholmod_l_hip_aat_logdet_grad_device, the engine's cholmod_hip_product_values_grad_device /
cholmod_hip_product_logdet_grad_device, DeviceCholesky with an unsymmetric A or a tensor beta): what can be checked without
a GPU -- the exported symbols, the argument checks, which come before the engine or a device is touched (integers stand in
for device pointers: nothing here may dereference them), and the numpy formulas of tests/aat_grad_reference.py, which must
hold the bars of the GPU test against dense torch autograd themselves."""
import ctypes as C

import numpy as np
import pytest

import aat_grad_matrices as AM
import aat_grad_reference as AR
import grad_reference as GR
import selinv_reference as R
from oracle.oracle import OracleFactor
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

FAKE_U, FAKE_V, FAKE_A, FAKE_G = 0x1000, 0x2000, 0x3000, 0x4000
NEW_API = ("cholmod_l_hip_aat_values_grad_device", "cholmod_l_hip_aat_logdet_grad_device")
NEW_HIP = ("cholmod_hip_product_values_grad_device", "cholmod_hip_product_logdet_grad_device")


def test_library_exports_the_entry_points():
    for L in (ch.lib(), ch.lib(hooks=True)):
        for name in NEW_API + NEW_HIP:
            assert hasattr(L, name), name
    assert all(name in ch.API_SYMBOLS for name in NEW_API) and all(name in ch.HIP_SYMBOLS for name in NEW_HIP)
    assert callable(ch.Session.aat_values_grad_device) and callable(ch.Session.aat_logdet_grad_device)


def _rect(S, M, x=None):
    m, n = M.shape
    A = S.L.cholmod_l_allocate_sparse(m, n, max(M.nnz, 1), 1, 1, 0, ch.REAL, C.byref(S.cm))
    assert A
    a = A.contents
    ch._view(a.p, n + 1, C.c_int64, np.int64)[:] = M.indptr
    ch._view(a.i, M.nnz, C.c_int64, np.int64)[:] = M.indices
    ch._view(a.x, M.nnz, C.c_double, np.float64)[:] = M.data if x is None else x
    return A


def _cpu_factor(M, beta=0.0, x=None):
    """-> (Session, A, Lf): the factor of A*A' + beta*I on the CPU path"""
    S = ch.Session(use_gpu=0, ordering="default")
    A = _rect(S, M, x)
    Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
    assert Lf and S.cm.status == ch.OK and Lf.contents.n == M.shape[0]
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK
    return S, A, Lf


def _free(S, A, Lf):
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def _grad(S, A, Lf, U=FAKE_U, V=FAKE_V, Av=FAKE_A, Gp=FAKE_G, ld=None, nrhs=3):
    S.cm.status = ch.OK
    n = int(Lf.contents.n) if Lf else 0
    ld = n if ld is None else ld
    return S.L.cholmod_l_hip_aat_values_grad_device(A, Lf, -1.0, U, ld, V, ld, nrhs, Av, Gp, None, C.byref(S.cm)), S.cm.status


def _logdet(S, A, Lf, Av=FAKE_A, Gp=FAKE_G):
    S.cm.status = ch.OK
    return S.L.cholmod_l_hip_aat_logdet_grad_device(A, Lf, Av, Gp, None, C.byref(S.cm)), S.cm.status


def test_argument_checks_come_before_any_device():
    S, A, Lf = _cpu_factor(AM.engineered())
    S.cm.error_handler = ch.ERRFUNC(0)
    bad = (0, ch.INVALID)
    n = int(Lf.contents.n)
    # NULL pointers
    assert _grad(S, None, Lf) == bad and _grad(S, A, None) == bad
    for k in ("U", "V", "Av", "Gp"):
        assert _grad(S, A, Lf, **{k: None}) == bad, k
    assert _logdet(S, None, Lf) == bad and _logdet(S, A, None) == bad
    assert _logdet(S, A, Lf, Av=None) == bad and _logdet(S, A, Lf, Gp=None) == bad
    # the GPU is off: no host fallback, with or without hip_cpu_fallback
    for fb in (0, 1):
        S.cm.hip_cpu_fallback = fb
        assert _grad(S, A, Lf) == bad and _logdet(S, A, Lf) == bad
    S.cm.hip_cpu_fallback = 0
    for gpu in (0, 1):          # ... the rest also with the GPU asked for: no check needs a device
        S.cm.useGPU = gpu
        # a CPU-path factor was not factorized on the device
        assert _grad(S, A, Lf) == bad and _logdet(S, A, Lf) == bad
        # a leading dimension smaller than n
        assert _grad(S, A, Lf, ld=n - 1) == bad
        # L->minor < n: the log-determinant
        Lf.contents.minor = n - 1
        assert _logdet(S, A, Lf) == bad
        Lf.contents.minor = n
        # complex / zomplex L or A
        for xt in (ch.COMPLEX, ch.ZOMPLEX):
            Lf.contents.xtype = xt
            assert _grad(S, A, Lf) == (0, ch.NOT_INSTALLED) and _logdet(S, A, Lf) == (0, ch.NOT_INSTALLED)
            Lf.contents.xtype = ch.REAL
            A.contents.xtype = xt
            assert _grad(S, A, Lf) == (0, ch.NOT_INSTALLED) and _logdet(S, A, Lf) == (0, ch.NOT_INSTALLED)
            A.contents.xtype = ch.REAL
        # a SYMMETRIC A (its entry point is cholmod_l_hip_values_grad_device), an unpacked, a mismatched A
        for stype in (-1, 1):
            A.contents.stype = stype
            assert _grad(S, A, Lf) == bad and _logdet(S, A, Lf) == bad
        A.contents.stype = 0
        A.contents.packed = 0
        assert _grad(S, A, Lf) == bad and _logdet(S, A, Lf) == bad
        A.contents.packed = 1
        A.contents.nrow -= 1
        assert _grad(S, A, Lf) == bad and _logdet(S, A, Lf) == bad
        A.contents.nrow += 1
        # several ranks
        S.cm.hip_world = 2
        assert _grad(S, A, Lf) == bad and _logdet(S, A, Lf) == bad
        S.cm.hip_world = 1
    S.cm.useGPU = 0
    _free(S, A, Lf)


def test_engine_refuses_null_and_host_only_plans():
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
            assert lib.cholmod_hip_product_values_grad_device(plan, perm, -1.0, FAKE_U, n, FAKE_V, n, 3, FAKE_A, FAKE_G, len(Ai),
                                                              None) == ch.HIP_INVALID
        assert lib.cholmod_hip_product_logdet_grad_device(plan, FAKE_A, FAKE_G, len(Ai), None) == ch.HIP_INVALID
    lib.cholmod_hip_plan_destroy(P)


def test_formulas_on_a_hand_example():
    """A = [[a0, 0], [a1, a2], [0, a3]]: tril (A A') has the entries (0,0) a0^2, (1,0) a1 a0, (1,1) a1^2 + a2^2, (2,1) a3 a2,
    (2,2) a3^2; the lists, their transpose and the chain rule by hand"""
    import scipy.sparse as sp
    a = np.array([1.0, 2.0, 3.0, 4.0])
    M = sp.csc_matrix((a, [0, 1, 1, 2], [0, 2, 4]), shape=(3, 2))
    Cp, Ci, cp, ia, ib = AR.product_map(M)
    assert Cp.tolist() == [0, 2, 4, 5] and Ci.tolist() == [0, 1, 1, 2, 2]
    assert cp.tolist() == [0, 1, 2, 4, 5, 6] and ia.tolist() == [0, 1, 1, 2, 3, 3] and ib.tolist() == [0, 0, 1, 2, 2, 3]
    assert AR.product_values(cp, ia, ib, a).tolist() == [1.0, 2.0, 13.0, 12.0, 16.0]
    tp, tc, tpart = AR.transpose_map(cp, ia, ib, 4)
    assert tp.tolist() == [0, 3, 6, 9, 12]
    assert tc.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4] and tpart.tolist() == [0, 0, 1, 0, 1, 1, 2, 2, 3, 2, 3, 3]
    Gv = np.array([10.0, 20.0, 30.0, 40.0, 50.0])
    # d (sum Gv vals) / d a0 = 2 * 10 a0 + 20 a1, / d a1 = 20 a0 + 2 * 30 a1, / d a2 = 2 * 30 a2 + 40 a3, / d a3 = 40 a2 + 2 * 50 a3
    want = [60.0, 140.0, 340.0, 520.0]
    assert AR.product_grad(tp, tc, tpart, Gv, a).tolist() == want
    assert AR.product_grad_in_kernel_order(tp, tc, tpart, Gv, a).tolist() == want
    assert AR.product_grad_magnitude(tp, tc, tpart, -Gv, a).tolist() == want
    # a value in no pair does not exist (every value meets itself), but an EMPTY list gives +0.0
    g = AR.product_grad(np.array([0, 0]), tc[:0], tpart[:0], Gv, a)
    assert g.tolist() == [0.0] and not np.signbit(g[0])


@pytest.mark.parametrize("name", ["afiro", "engineered", "classes160", "one_by_one"])
def test_product_map_restated_in_numpy_is_the_library_s(name):
    """the numpy product map equals cholmod_l_hip_aat_product_map, list by list; the lists of the transposed map have the
    length of the value's column + 1; classes160 has both sides of both class edges"""
    M = AM.MATRICES[name]()
    Cp, Ci, cp, ia, ib = AR.product_map(M)
    S = ch.Session(use_gpu=0)
    A = _rect(S, M)
    f = S.L.cholmod_l_hip_aat_product_map
    npairs = f(A, None, None, None, C.byref(S.cm))
    assert npairs == len(ia)
    cp2, ia2, ib2 = np.zeros(len(Ci) + 1, dtype=np.int64), np.zeros(max(npairs, 1), dtype=np.int64), np.zeros(max(npairs, 1), dtype=np.int64)
    assert f(A, cp2.ctypes.data, ia2.ctypes.data, ib2.ctypes.data, C.byref(S.cm)) == npairs
    assert np.array_equal(cp, cp2) and np.array_equal(ia, ia2[:npairs]) and np.array_equal(ib, ib2[:npairs])
    S.free_sparse(A)
    S.finish()
    tp, tc, tpart = AR.transpose_map(cp, ia, ib, M.nnz)
    ck = np.diff(M.indptr)
    assert np.array_equal(np.diff(tp), np.repeat(ck, ck) + 1)
    if name == "classes160":
        assert {8, 9, 128, 129, 161} <= set(np.diff(tp).tolist())


CASES = [(name, k, nrhs) for name in ("afiro", "engineered", "classes160") for k in (0, 1) for nrhs in (1, 19)]


@pytest.mark.parametrize("name,k,nrhs", CASES)
def test_formulas_against_dense_torch_autograd(name, k, nrhs):
    """the numpy restatement of the backward pass holds the bars the device is held to, against dense torch autograd:
    beta 0 and 0.375 (afiro: 1e-3 max |A A'|), nrhs 1 and 19"""
    M = AM.MATRICES[name]()
    a, m = M.data.copy(), M.shape[0]
    beta = AM.shift_of(name, M) if k else 0.0
    B, W = GR.inputs(m, nrhs, 7)
    ref = AR.torch_reference(M, a, beta, B, W)
    gv, gb, gbeta = AR.loss_gradients(M, a, beta, B, W)
    S, A, Lf = _cpu_factor(M, beta)
    tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
    _free(S, A, Lf)
    bar_v, bar_b, bar_beta = AR.bars(M, a, ref, tol, nrhs)
    ev, eb, ebeta = np.abs(gv - ref["grad_values"]).max(), np.abs(gb - ref["grad_B"]).max(), abs(gbeta - ref["grad_beta"])
    print(f"{name} beta={beta:.3e} nrhs={nrhs}: grad_values {ev:.2e} (bar {bar_v:.2e}), grad_B {eb:.2e} (bar {bar_b:.2e}), "
          f"grad_beta {ebeta:.2e} (bar {bar_beta:.2e})")
    assert ev <= bar_v and eb <= bar_b and ebeta <= bar_beta, (ev, bar_v, eb, bar_b, ebeta, bar_beta)


@pytest.mark.parametrize("nrhs", [1, 19])
@pytest.mark.parametrize("beta", [0.0, 0.375])
def test_symmetric_beta_gradient_against_dense_torch_autograd(beta, nrhs):
    """p3d_12_nd, M = A + beta I: -(Lambda . X).sum () + 0.3 trace Z against torch's gradient with respect to beta"""
    case = R.CASES["p3d_12_nd"]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    B, W = GR.inputs(n, nrhs, 7)
    ref = AR.torch_reference_symmetric(n, Ap, Ai, Ax, -1, beta, B, W)
    got = AR.symmetric_beta_gradient(n, Ap, Ai, Ax, -1, beta, B, W)
    S, A, Lf = R.factorized(case, use_gpu=0, beta=beta)
    tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
    _free(S, A, Lf)
    bar = tol * n * (2 * nrhs * ref["lam_max"] * ref["x_max"] + 0.3 * ref["z_max"])
    print(f"p3d_12_nd beta={beta} nrhs={nrhs}: grad_beta {abs(got - ref['grad_beta']):.2e} (bar {bar:.2e})")
    assert abs(got - ref["grad_beta"]) <= bar
    # (the values and B of the symmetric reference are those of tests/grad_reference.py)
    old = GR.torch_reference(n, Ap, Ai, Ax, -1, beta, B, W)
    assert np.array_equal(old["grad_values"], ref["grad_values"]) and np.array_equal(old["grad_B"], ref["grad_B"])


def test_device_cholesky_takes_a_tensor_beta_and_an_unsymmetric_pattern():
    """what DeviceCholesky decides before it touches a device: stype == 0 means A A' + beta I; beta is a float or a 0-dim
    float64 tensor, read once per version and passed to the autograd functions only when it is a tensor"""
    import torch
    from suitesparse_amd.autograd import DeviceCholesky
    S, A, Lf = _cpu_factor(AM.engineered())
    chol = DeviceCholesky(S, A, Lf, beta=0.25)
    assert chol.aat and chol.beta == 0.25 and chol._beta_value() == 0.25 and chol._beta_input() is None
    b = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
    chol.beta = b
    assert chol._beta_input() is b and chol._beta_value() == 0.5
    with torch.no_grad():
        b.mul_(3.0)
    assert chol._beta_value() == 1.5
    for wrong in (torch.tensor([0.5], dtype=torch.float64), torch.tensor(0.5, dtype=torch.float32)):
        with pytest.raises(TypeError):
            DeviceCholesky(S, A, Lf, beta=wrong)
    _free(S, A, Lf)
    case = R.CASES["p3d_12_nd"]()
    S, A, Lf = R.factorized(case, use_gpu=0)
    assert not DeviceCholesky(S, A, Lf, beta=b).aat
    _free(S, A, Lf)
