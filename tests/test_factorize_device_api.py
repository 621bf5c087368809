"""The factorization from device values (cholmod_l_hip_factorize_values_device, cholmod_hip_factorize_values_device,
cholmod_hip_set_product_map, cholmod_hip_download_matrix_values, cholmod_l_hip_aat_product_map, Session.factorize_device):
what can be checked without a GPU -- the exported symbols, the argument checks, which come before the engine or a device
is touched (integers stand in for device pointers: nothing here may dereference them), and the product map of A*A', which
is integer work on the host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import factorize_device_matrices as FM  # noqa: E402
from oracle.oracle import OracleFactor  # noqa: E402
from suitesparse_amd import cholmod as ch  # noqa: E402
from suitesparse_amd import generators as G  # noqa: E402

FAKE_V = 0x3000
NEW_API = ("cholmod_l_hip_factorize_values_device", "cholmod_l_hip_aat_product_map")
NEW_HIP = ("cholmod_hip_factorize_values_device", "cholmod_hip_set_product_map", "cholmod_hip_download_matrix_values")


def test_library_exports_the_factorization_from_device_values():
    L = ch.lib()
    for name in NEW_API:
        assert hasattr(L, name), name
        assert name in ch.API_SYMBOLS
    for name in NEW_HIP:
        assert hasattr(L, name), name
        assert name in ch.HIP_SYMBOLS
    assert callable(getattr(ch.Session, "factorize_device", None))
    for hdr, names in (("cholmod.h", NEW_API), ("cholmod_hip.h", NEW_HIP)):
        text = open(os.path.join(os.path.dirname(HERE), "include", hdr)).read()
        for name in names:
            assert name + " (" in text, (hdr, name)


def _cpu_factor(numeric=True):
    n, Ap, Ai, Ax = G.poisson3d(6)
    perm = G.geometric_nd(6, 6, 6, 3)
    S = ch.Session(use_gpu=0)
    S.cm.error_handler = ch.ERRFUNC(0)
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    if numeric:
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    return S, A, Lf, n


def _call(S, A, Lf, V=FAKE_V, beta=0.0):
    S.cm.status = ch.OK
    b = (C.c_double * 2)(beta, 0.0)
    ok = S.L.cholmod_l_hip_factorize_values_device(A, V, C.byref(b), Lf, None, C.byref(S.cm))
    return ok, S.cm.status


def test_argument_checks_come_before_any_device():
    S, A, Lf, n = _cpu_factor()
    x_before = ch.FactorView(Lf).x.copy()
    # NULL pointers
    assert _call(S, None, Lf) == (0, ch.INVALID)
    assert _call(S, A, None) == (0, ch.INVALID)
    assert _call(S, A, Lf, V=None) == (0, ch.INVALID)
    # the GPU is off: no host fallback for device pointers, with or without hip_cpu_fallback
    assert _call(S, A, Lf) == (0, ch.INVALID)
    S.cm.hip_cpu_fallback = 1
    assert _call(S, A, Lf) == (0, ch.INVALID)
    S.cm.hip_cpu_fallback = 0
    # ... and with the GPU asked for, every check that needs no device: an L without the pattern record of a device
    # factorization (this one was factorized on the host), several ranks
    S.cm.useGPU = 1
    assert Lf.contents.hip_apat_valid == 0
    assert _call(S, A, Lf) == (0, ch.INVALID)
    S.cm.hip_world = 2
    assert _call(S, A, Lf) == (0, ch.INVALID)
    S.cm.hip_world = 1
    # A unpacked
    A.contents.packed = 0
    assert _call(S, A, Lf) == (0, ch.INVALID)
    A.contents.packed = 1
    # mismatched dimensions: a matrix of another size; a symmetric A that is not square
    n2, Ap2, Ai2, Ax2 = G.poisson3d(5)
    A2 = S.sparse(n2, Ap2, Ai2, Ax2, -1)
    assert _call(S, A2, Lf) == (0, ch.INVALID)
    S.free_sparse(A2)
    A.contents.ncol = n - 1
    assert _call(S, A, Lf) == (0, ch.INVALID)
    A.contents.ncol = n
    # complex / zomplex A or L
    for xt in (ch.COMPLEX, ch.ZOMPLEX):
        Lf.contents.xtype = xt
        assert _call(S, A, Lf) == (0, ch.NOT_INSTALLED)
        Lf.contents.xtype = ch.REAL
        A.contents.xtype = xt
        assert _call(S, A, Lf) == (0, ch.NOT_INSTALLED)
        A.contents.xtype = ch.REAL
    # a pattern-only A is what the call needs (A->x is never read): it gets as far as the record check
    A.contents.xtype = ch.PATTERN
    assert _call(S, A, Lf) == (0, ch.INVALID)
    A.contents.xtype = ch.REAL
    S.cm.useGPU = 0
    # none of this touched the factor
    assert np.array_equal(ch.FactorView(Lf).x, x_before) and Lf.contents.xtype == ch.REAL
    S.free_factor(Lf)
    S.free_sparse(A)
    assert S.cm.malloc_count == 0
    S.finish()


def test_symbolic_factor_is_refused():
    S, A, Lf, n = _cpu_factor(numeric=False)
    assert Lf.contents.xtype == ch.PATTERN
    assert _call(S, A, Lf) == (0, ch.INVALID)
    S.cm.useGPU = 1
    assert _call(S, A, Lf) == (0, ch.INVALID)
    S.cm.useGPU = 0
    S.free_factor(Lf)
    S.free_sparse(A)
    assert S.cm.malloc_count == 0
    S.finish()


def test_engine_refuses_a_host_only_plan_and_null_arguments():
    lib = ch.lib()
    n, Ap, Ai, Ax = G.poisson3d(5)
    O = OracleFactor(n, Ap, Ai, -1, perm=None, postorder=True)
    keep = [np.ascontiguousarray(getattr(O, k), dtype=np.int64) for k in ("super", "pi", "px", "s")]
    st = C.c_int(0)
    P = lib.cholmod_hip_plan_create(n, len(keep[0]) - 1, *(a.ctypes.data_as(C.c_void_p) for a in keep),
                                    ch.HIP_PLAN_HOST_ONLY, C.byref(st))
    assert P and st.value == 0
    minor = C.c_int64(-7)
    nz = int(Ap[-1])
    assert lib.cholmod_hip_factorize_values_device(P, FAKE_V, nz, 0.0, 0, None, C.byref(minor)) == ch.HIP_INVALID
    assert lib.cholmod_hip_factorize_values_device(None, FAKE_V, nz, 0.0, 0, None, C.byref(minor)) == ch.HIP_INVALID
    assert minor.value == -7
    cp = np.array([0, 1], dtype=np.int64)
    ia = np.zeros(1, dtype=np.int64)
    assert lib.cholmod_hip_set_product_map(P, cp.ctypes.data, ia.ctypes.data, ia.ctypes.data, 1, 1) == ch.HIP_INVALID
    assert lib.cholmod_hip_set_product_map(None, cp.ctypes.data, ia.ctypes.data, ia.ctypes.data, 1, 1) == ch.HIP_INVALID
    assert lib.cholmod_hip_set_product_map(P, None, None, None, 0, 0) == ch.HIP_INVALID
    out = np.zeros(nz)
    assert lib.cholmod_hip_download_matrix_values(P, out.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_download_matrix_values(None, out.ctypes.data) == ch.HIP_INVALID
    lib.cholmod_hip_plan_destroy(P)


def _rect(S, M, stype=0):
    m, n = M.shape
    A = S.L.cholmod_l_allocate_sparse(m, n, max(M.nnz, 1), 1, 1, stype, ch.REAL, C.byref(S.cm))
    assert A
    a = A.contents
    ch._view(a.p, n + 1, C.c_int64, np.int64)[:] = M.indptr
    ch._view(a.i, M.nnz, C.c_int64, np.int64)[:] = M.indices
    ch._view(a.x, M.nnz, C.c_double, np.float64)[:] = M.data
    return A


@pytest.mark.parametrize("which", ["afiro", "engineered", "one_by_one"])
def test_aat_product_map(which):
    """the map evaluated in numpy is tril (A @ A.T), entry by entry at the positions of the symbolic product; every list
    runs by ascending column of A; the pairs are sum_k c_k (c_k + 1) / 2 over the column counts c_k"""
    M = getattr(FM, which)()
    m, ncol = M.shape
    Cp, Ci = FM.symbolic_tril_aat(M)
    nc = len(Ci)
    S = ch.Session(use_gpu=0)
    S.cm.error_handler = ch.ERRFUNC(0)
    A = _rect(S, M)
    f = S.L.cholmod_l_hip_aat_product_map
    npairs = f(A, None, None, None, C.byref(S.cm))
    ck = np.diff(M.indptr).astype(np.int64)
    assert npairs == int((ck * (ck + 1) // 2).sum()) and S.cm.status == ch.OK
    cp = np.full(nc + 1, -1, dtype=np.int64)
    ia = np.full(max(npairs, 1), -1, dtype=np.int64)
    ib = np.full(max(npairs, 1), -1, dtype=np.int64)
    assert f(A, cp.ctypes.data, ia.ctypes.data, ib.ctypes.data, C.byref(S.cm)) == npairs
    assert cp[0] == 0 and cp[nc] == npairs and bool((np.diff(cp) >= 1).all())
    ia, ib = ia[:npairs], ib[:npairs]
    assert ia.min() >= 0 and ib.min() >= 0 and ia.max() < M.nnz and ib.max() < M.nnz
    colof = np.repeat(np.arange(ncol), ck)
    ref, mag, cnt = FM.exact_products(M, Cp, Ci)
    a = M.data
    jof = np.repeat(np.arange(m), np.diff(Cp))
    for c in range(nc):
        p0, p1 = cp[c], cp[c + 1]
        assert p1 - p0 == cnt[c], c
        # the pairs of entry (i, j): A (i,k) and A (j,k) over the columns k both rows have, k ascending
        assert np.array_equal(M.indices[ia[p0:p1]], np.full(p1 - p0, Ci[c])), c
        assert np.array_equal(M.indices[ib[p0:p1]], np.full(p1 - p0, jof[c])), c
        assert np.array_equal(colof[ia[p0:p1]], colof[ib[p0:p1]]), c
        assert bool((np.diff(colof[ia[p0:p1]]) > 0).all()), c
        val = 0.0
        for p in range(p0, p1):
            val += a[ia[p]] * a[ib[p]]
        assert abs(val - ref[c]) <= (cnt[c] + 2) * FM.EPS * mag[c], (c, val, ref[c])
    if which == "engineered":
        # the list lengths the product kernel's three classes are cut at: 1 .. 8, 9 .. 128, above
        lens = np.diff(cp)
        assert lens.min() == 1 and lens.max() == 131 and bool(((lens > 8) & (lens <= 128)).any())
        assert int(ck.max()) == m and int((ck == 2).sum()) == 130 and int((ck == 1).sum()) == 1 and int((ck == 0).sum()) == 1
    # invalid input: a symmetric matrix, a row index out of range
    A.contents.stype = -1
    assert f(A, None, None, None, C.byref(S.cm)) == -1 and S.cm.status == ch.INVALID
    A.contents.stype = 0
    S.cm.status = ch.OK
    Aiv = ch._view(A.contents.i, M.nnz, C.c_int64, np.int64)
    keep = Aiv[0]
    Aiv[0] = m
    assert f(A, None, None, None, C.byref(S.cm)) == -1 and S.cm.status == ch.INVALID
    Aiv[0] = keep
    S.cm.status = ch.OK
    assert f(None, None, None, None, C.byref(S.cm)) == -1
    S.free_sparse(A)
    assert S.cm.malloc_count == 0
    S.finish()
