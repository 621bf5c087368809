"""The bodies of tests/test_gpu_factorize_device.py, run in a process of their own: `python factorize_device_cases.py CASE
[ARG ...]`, torch imported FIRST (see solve_device_cases.py, whose helpers these cases share).  Exit status 0 = every
assertion held.

Session.factorize_device (cholmod_l_hip_factorize_values_device) takes new values of A from device memory.  For a symmetric
A the resident S receives exactly the values the host path's upload gives it, the assembly writes one value per entry of L
and the factorization is reproducible (tools/factor_digest.py relies on that): L is compared BIT FOR BIT with what
cholmod_l_factorize gives for the same values in a second session that took the same sequence of calls through the host.
For A*A' the device sums the products of an entry in another order than the host: every value of S within the bound of a
dot product of its length, (len + 2) 2^-53 sum |a_p| |a_q|, of the exact sum (nothing measured), L within the project's
1e-12 of the host's."""
import torch  # noqa: E402  (first)

import ctypes as C
import sys

import numpy as np
import scipy.sparse as sp

import solve_device_cases as SD
from solve_device_cases import TOL, _dev, _relcols
from residual_device_cases import Sym, _check1, _worst
import factorize_device_matrices as FM
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

EPS = 2.0 ** -53
NAN = float("nan")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _host_x(S, Lf):
    assert S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm)) == 1
    return ch.FactorView(Lf).x.copy()


def _resident_values(S, Lf, snz):
    out = np.full(snz, NAN)
    assert S.L.cholmod_hip_download_matrix_values(Lf.contents.hip_plan, out.ctypes.data) == 0
    return out


def _finish(S, Lf, *mats):
    torch.cuda.synchronize()
    S.free_factor(Lf)
    for A in mats:
        S.free_sparse(A)
    assert S.cm.malloc_count == 0, S.cm.malloc_count
    S.finish()


def _lower_of(n, Ap, Ai, Ax):
    """the symmetric matrix whose lower triangle (n, Ap, Ai, Ax) is, in full, as scipy CSC"""
    Lo = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    return (Lo + sp.tril(Lo, -1).T).tocsc()


def _permuted_lower(F, perm):
    """tril (P F P') by sorted columns: the resident S"""
    Sx = sp.tril(F[perm][:, perm], format="csc")
    Sx.sort_indices()
    return Sx


def _stored(n, Ap, Ai, Ax, how):
    """the lower triangle (n, Ap, Ai, Ax) as the caller stores it: (Ap, Ai, Ax, stype, used) -- `used`: the entries
    the library reads
      lower: stype -1        upper: stype 1 (the transpose)
      both:  stype -1 with the strictly upper triangle stored as well (ignored entries)"""
    Lo = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    if how == "lower":
        M, stype = Lo, -1
    elif how == "upper":
        M, stype = Lo.T.tocsc(), 1
    else:
        M, stype = (Lo + sp.tril(Lo, -1).T).tocsc(), -1
    M.sort_indices()
    cols = np.repeat(np.arange(n), np.diff(M.indptr))
    used = M.indices >= cols if stype < 0 else M.indices <= cols
    return M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.copy(), stype, used, M.indices == cols


def _new_values(v, diag):
    """diagonal shifted, off-diagonals scaled: one exactly specified IEEE operation per entry, so that numpy and torch
    give the same bits"""
    return np.where(diag, v + 0.75, v * 0.875)


def _new_values_dev(vd, diag_d):
    return torch.where(diag_d, vd + 0.75, vd * 0.875)


def _symmetric(n, Ap, Ai, Ax, perm, how, beta=0.0, postorder=True):
    """factorize from the host, then new values made on the device through factorize_device; a second session takes the
    same two steps through the host.  S and L bit for bit, twice."""
    Bp, Bi, Bx, stype, used, diag = _stored(n, Ap, Ai, Ax, how)
    v2 = _new_values(Bx, diag)
    S = ch.Session(postorder=postorder)
    S.cm.error_handler = ch.ERRFUNC(0)
    A = S.sparse(n, Bp, Bi, Bx, stype)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK and Lf.contents.hip_apat_valid == 1
    vd = _new_values_dev(_dev(Bx), _dev(diag))
    if not used.all():
        vd[_dev(~used)] = NAN                       # (entries the library ignores: it must not read them either)
    assert np.array_equal(_bits(vd.cpu().numpy()[used]), _bits(v2[used]))
    # the host values of A are not read: spoil them
    ch._view(A.contents.x, len(Bx), C.c_double, np.float64)[:] = NAN
    assert S.factorize_device(A, vd, Lf, beta) == 1 and S.cm.status == ch.OK
    assert Lf.contents.minor == n and Lf.contents.hip_on_device == 1
    x1 = _host_x(S, Lf)
    # the resident S: the permuted values, exactly
    F = _lower_of(n, Ap, Ai, _new_values(np.asarray(Ax, dtype=np.float64), np.asarray(Ai) == np.repeat(np.arange(n), np.diff(Ap))))
    P = ch.FactorView(Lf).Perm.copy()
    Sref = _permuted_lower(F, P)
    s1 = _resident_values(S, Lf, Sref.nnz)
    assert np.array_equal(_bits(s1), _bits(Sref.data))
    # once more on the same tensor: the same bits of S and of L
    assert S.factorize_device(A, vd, Lf, beta) == 1 and S.cm.status == ch.OK
    assert np.array_equal(_bits(_resident_values(S, Lf, Sref.nnz)), _bits(s1))
    assert np.array_equal(_bits(_host_x(S, Lf)), _bits(x1))
    # the second session, through the host
    S2 = ch.Session(postorder=postorder)
    A2 = S2.sparse(n, Bp, Bi, Bx, stype)
    L2 = S2.analyze(A2, perm)
    assert S2.factorize(A2, L2, beta) == 1
    v2h = v2.copy()
    v2h[~used] = NAN
    ch._view(A2.contents.x, len(Bx), C.c_double, np.float64)[:] = v2h
    assert S2.factorize(A2, L2, beta) == 1 and S2.cm.status == ch.OK and L2.contents.hip_apat_valid == 1
    x2 = _host_x(S2, L2)
    same = np.array_equal(_bits(x1), _bits(x2))
    print(f"{how} n={n} beta={beta}: L bit-identical to the host path's: {same}; max |dL| = {np.abs(x1 - x2).max():.3e}")
    assert same
    assert np.array_equal(_bits(_resident_values(S2, L2, Sref.nnz)), _bits(s1))
    # the host values-only path keeps working after the device entry, and gives these bits again
    ch._view(A.contents.x, len(Bx), C.c_double, np.float64)[:] = v2h
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK
    assert np.array_equal(_bits(_host_x(S, Lf)), _bits(x1))
    _finish(S2, L2, A2)
    return S, A, Lf, F, vd


def case_symmetric(stype):
    n, Ap, Ai, Ax = G.poisson3d(12)
    perm = G.geometric_nd(12, 12, 12, 4)
    S, A, Lf, F, vd = _symmetric(n, Ap, Ai, Ax, perm, "lower" if int(stype) < 0 else "upper")
    _finish(S, Lf, A)


def case_shape(kind):
    n, Ap, Ai, Ax = G.poisson3d(7)
    if kind == "natural":
        # natural ordering, packed lower A: S is A itself and the value map the identity
        S, A, Lf, F, vd = _symmetric(n, Ap, Ai, Ax, None, "lower", postorder=False)
        assert Lf.contents.ordering == ch.NATURAL and np.array_equal(ch.FactorView(Lf).Perm, np.arange(n))
    else:
        # both triangles stored under stype -1: more values than S has entries, the ignored ones are NaN on the device
        S, A, Lf, F, vd = _symmetric(n, Ap, Ai, Ax, G.geometric_nd(7, 7, 7, 3), "both")
        assert int(torch.isnan(vd).sum()) == len(Ai) - n
    _finish(S, Lf, A)


def case_beta():
    """beta != 0: the residual on the device after factorize_device is that of the NEW matrix and of this beta"""
    n, Ap, Ai, Ax = G.poisson3d(12)
    perm = G.geometric_nd(12, 12, 12, 4)
    beta = 0.375
    S, A, Lf, F, vd = _symmetric(n, Ap, Ai, Ax, perm, "lower", beta=beta)
    assert S.factorize_device(A, vd, Lf, beta) == 1 and S.cm.status == ch.OK
    Fl = sp.tril(F, format="csc")
    Fl.sort_indices()
    M = Sym(n, Fl.indptr, Fl.indices, Fl.data, beta)
    rng = np.random.default_rng(31)
    for nrhs in (3, 17):
        x, b = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
        R, nrm = S.residual_device(Lf, _dev(x), _dev(b), norms=True)
        _check1(M, R, nrm, x, b, f"beta={beta} nrhs={nrhs}")
    _finish(S, Lf, A)


def _rect(S, M, x=None):
    m, n = M.shape
    A = S.L.cholmod_l_allocate_sparse(m, n, max(M.nnz, 1), 1, 1, 0, ch.REAL, C.byref(S.cm))
    assert A
    a = A.contents
    ch._view(a.p, n + 1, C.c_int64, np.int64)[:] = M.indptr
    ch._view(a.i, M.nnz, C.c_int64, np.int64)[:] = M.indices
    ch._view(a.x, M.nnz, C.c_double, np.float64)[:] = M.data if x is None else x
    return A


def case_aat(which):
    M = getattr(FM, which)()
    m = M.shape[0]
    a2 = M.data * np.where(np.arange(M.nnz) % 3 == 0, 1.25, 0.75)         # new values: the ones the device call takes
    M2 = sp.csc_matrix((a2, M.indices, M.indptr), shape=M.shape)
    Cp, Ci = FM.symbolic_tril_aat(M2)
    ref, mag, cnt = FM.exact_products(M2, Cp, Ci)
    beta = 1e-3 * float(np.abs(ref).max()) if which == "afiro" else 0.0
    S = ch.Session(ordering="default")
    S.cm.error_handler = ch.ERRFUNC(0)
    A = _rect(S, M)
    Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
    assert Lf and S.cm.status == ch.OK and Lf.contents.n == m
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK and Lf.contents.hip_apat_valid == 1
    assert Lf.contents.hip_aat_valid == 0                                   # (the product map is built lazily)
    vd = _dev(a2)
    ch._view(A.contents.x, M.nnz, C.c_double, np.float64)[:] = NAN
    assert S.factorize_device(A, vd, Lf, beta) == 1 and S.cm.status == ch.OK
    assert Lf.contents.hip_aat_valid == 1 and Lf.contents.minor == m
    x1 = _host_x(S, Lf)
    # every value of the resident S = tril (P C P') against the exact sum of its products
    P = ch.FactorView(Lf).Perm.copy()
    cols = np.repeat(np.arange(m), np.diff(Cp))

    def resident(vals):
        Lo = sp.csc_matrix((vals, Ci, Cp), shape=(m, m))
        F = (Lo + sp.tril(Lo, -1).T).tocsc()
        return _permuted_lower(F, P)

    # (values that are zero would drop out of a scipy matrix: carry positions instead, 1-based)
    pos = resident(np.arange(1, len(Ci) + 1, dtype=np.float64))
    q = pos.data.astype(np.int64) - 1
    assert len(q) == len(Ci) and np.array_equal(np.sort(q), np.arange(len(Ci)))
    s1 = _resident_values(S, Lf, len(Ci))
    bound = (cnt[q] + 2) * EPS * mag[q]
    w = float((np.abs(s1 - ref[q]) / bound).max())
    print(f"aat {which}: nnz(C)={len(Ci)} list lengths {cnt.min()}..{cnt.max()} beta={beta:.3e}: worst |S - exact| / bound = {w:.3e}")
    assert w <= 1.0, w
    # twice: the same bits (one owner per entry, no atomics); the second call pays the hash of A only
    assert S.factorize_device(A, vd, Lf, beta) == 1 and S.cm.status == ch.OK
    assert np.array_equal(_bits(_resident_values(S, Lf, len(Ci))), _bits(s1))
    assert np.array_equal(_bits(_host_x(S, Lf)), _bits(x1))
    # L against the host's factorization of the same A
    S2 = ch.Session(ordering="default")
    A2 = _rect(S2, M2)
    L2 = S2.L.cholmod_l_analyze(A2, C.byref(S2.cm))
    assert S2.factorize(A2, L2, beta) == 1 and S2.cm.status == ch.OK
    x2 = _host_x(S2, L2)
    assert np.array_equal(ch.FactorView(L2).Perm, P)
    e = np.linalg.norm(x1 - x2) / np.linalg.norm(x2)
    print(f"aat {which}: ||L_dev - L_host|| / ||L_host|| = {e:.3e}")
    assert e < 1e-12, e
    _finish(S2, L2, A2)
    # solve + refine on the device; the residual against numpy: the bound of check 1 for the matrix numpy holds (the
    # correctly rounded C) plus what the entries of the device's S may differ from it by, sum_j |dC_ij| |x_j|
    Cd = sp.csc_matrix((ref, Ci, Cp), shape=(m, m))
    Sy = Sym(m, Cp, Ci, ref, beta)
    dC = sp.csc_matrix(((cnt + 2) * EPS * mag, Ci, Cp), shape=(m, m))
    Dy = Sym(m, Cp, Ci, dC.data, 0.0)
    rng = np.random.default_rng(32)
    for nrhs in (2, 9):
        b = rng.standard_normal((nrhs, m))
        B = _dev(b)
        X = S.solve_device(Lf, B)
        X, nrm = S.refine_device(Lf, B, X, steps=1, norms=True)
        R, nrmR = S.residual_device(Lf, X, B, norms=True)
        assert torch.equal(nrm, nrmR)
        x = X.cpu().numpy()
        r, bnd = Sy.residual(x, b)
        bnd = bnd + np.stack([Dy.mv(x[k], True) for k in range(nrhs)])
        wr = _worst(R.cpu().numpy(), r, bnd)
        xs = np.linalg.solve(Cd.toarray() + np.tril(Cd.toarray(), -1).T + beta * np.eye(m), b.T).T
        ex = _relcols(x, xs)
        print(f"aat {which} nrhs={nrhs}: residual worst / bound {wr:.3e}, max |r| {float(nrm.max()):.3e}, x vs numpy {ex:.3e}")
        assert wr <= 1.0, wr
        assert np.array_equal(_bits(nrm.cpu().numpy()), _bits(np.abs(R.cpu().numpy()).max(axis=1)))
        assert ex < TOL, ex
    # the host values-only path (tril (A*A') formed on the host) still works on this L
    ch._view(A.contents.x, M.nnz, C.c_double, np.float64)[:] = a2
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK
    assert np.linalg.norm(_host_x(S, Lf) - x2) / np.linalg.norm(x2) < 1e-12
    # ... and the device entry after it
    assert S.factorize_device(A, vd, Lf, beta) == 1 and S.cm.status == ch.OK
    assert np.array_equal(_bits(_host_x(S, Lf)), _bits(x1))
    _finish(S, Lf, A)


def case_not_posdef():
    """one diagonal entry negative: its column is the failing pivot (a_jj minus a sum of squares), as on the host path;
    good values afterwards succeed and match"""
    n, Ap, Ai, Ax = G.poisson3d(8)
    perm = G.geometric_nd(8, 8, 8, 3)
    diag = np.asarray(Ai) == np.repeat(np.arange(n), np.diff(Ap))
    j0 = n // 2 + 3
    bad = np.asarray(Ax, dtype=np.float64).copy()
    bad[np.nonzero(diag)[0][j0]] = -1.0
    good = _new_values(np.asarray(Ax, dtype=np.float64), diag)
    out = []
    for device in (True, False):
        S = ch.Session()
        S.cm.error_handler = ch.ERRFUNC(0)
        A = S.sparse(n, Ap, Ai, Ax, -1)
        Lf = S.analyze(A, perm)
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        res = []
        for vals in (bad, good):
            if device:
                ok = S.factorize_device(A, _dev(vals), Lf)
            else:
                ch._view(A.contents.x, len(Ax), C.c_double, np.float64)[:] = vals
                ok = S.factorize(A, Lf)
            res.append((ok, S.cm.status, int(Lf.contents.minor)))
            S.cm.status = ch.OK
        x = _host_x(S, Lf)
        k0 = int(np.nonzero(ch.FactorView(Lf).Perm == j0)[0][0])
        out.append((res, x, k0))
        _finish(S, Lf, A)
    (rd, xd, k0), (rh, xh, _) = out
    print("device:", rd, "host:", rh, "pivot column", k0)
    assert rd == rh
    assert rd[0] == (1, ch.NOT_POSDEF, k0) and rd[1] == (1, ch.OK, n)
    assert np.array_equal(_bits(xd), _bits(xh))


def case_stream():
    """the values come out of a side stream behind a large matmul; factorize_device and solve_device under that stream,
    no synchronisation in between"""
    n, Ap, Ai, Ax = G.poisson3d(12)
    perm = G.geometric_nd(12, 12, 12, 4)
    S, A, Lf = SD._factor(n, Ap, Ai, Ax, perm)
    diag = np.asarray(Ai) == np.repeat(np.arange(n), np.diff(Ap))
    v2 = _new_values(np.asarray(Ax, dtype=np.float64), diag)
    rng = np.random.default_rng(33)
    b = rng.standard_normal((3, n))
    src, Bh = _dev(v2), _dev(b)
    vals = torch.full((len(v2),), NAN, dtype=torch.float64, device="cuda")      # (read too early: NaN everywhere)
    W = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        Z = W
        for _ in range(3):
            Z = Z @ W
        vals.copy_(src + 0.0 * Z[0, 0])
        ok = S.factorize_device(A, vals, Lf)
        X = S.solve_device(Lf, Bh)
        Y = X + 0.0
    s.synchronize()
    assert ok == 1 and S.cm.status == ch.OK
    F = _lower_of(n, Ap, Ai, v2)
    xs = np.linalg.solve(F.toarray(), b.T).T
    e = _relcols(Y.cpu().numpy(), xs)
    print(f"stream: x vs numpy {e:.3e}")
    assert e < TOL, e
    _finish(S, Lf, A)


def case_pattern():
    """another pattern with the same count (one row index moved, as tests/test_values_upload.py builds it): CHOLMOD_INVALID,
    and the previous factor still solves"""
    n, Ap, Ai, Ax = G.poisson3d(10)
    perm = G.geometric_nd(10, 10, 10, 3)
    cols = np.repeat(np.arange(n), np.diff(Ap))
    Ai = np.asarray(Ai)
    q = next(q for q in range(len(Ai) - 1, 0, -1)
             if Ai[q] - 1 > cols[q] and (cols[q - 1] != cols[q] or Ai[q] - 1 > Ai[q - 1]))
    Ai3 = Ai.copy()
    Ai3[q] -= 1
    S, A, Lf = SD._factor(n, Ap, Ai, Ax, perm)
    S.cm.error_handler = ch.ERRFUNC(0)
    x0 = _host_x(S, Lf)
    A3 = S.sparse(n, Ap, Ai3, Ax, -1)
    vd = _dev(2.0 * np.asarray(Ax, dtype=np.float64))
    s0 = _resident_values(S, Lf, len(Ai))
    assert S.factorize_device(A3, vd, Lf) == 0 and S.cm.status == ch.INVALID
    S.cm.status = ch.OK
    # no device state was touched: the resident S, the factor; L still solves for the old matrix
    assert np.array_equal(_bits(_resident_values(S, Lf, len(Ai))), _bits(s0))
    assert Lf.contents.hip_on_device == 1 and Lf.contents.xtype == ch.REAL
    assert np.array_equal(_bits(_host_x(S, Lf)), _bits(x0))
    b = np.random.default_rng(34).standard_normal((2, n))
    X = S.solve_device(Lf, _dev(b))
    xs = np.linalg.solve(_lower_of(n, Ap, Ai, np.asarray(Ax, dtype=np.float64)).toarray(), b.T).T
    assert _relcols(X.cpu().numpy(), xs) < TOL
    # a tensor of another length, on the host, of another type: refused by the wrapper
    for bad, exc in ((vd[:-1], ValueError), (vd.cpu(), TypeError), (vd.float(), TypeError), (vd.reshape(1, -1), ValueError)):
        try:
            S.factorize_device(A, bad, Lf)
            raise AssertionError("accepted")
        except exc:
            pass
    # ... and the right pattern still goes through
    assert S.factorize_device(A, vd, Lf) == 1 and S.cm.status == ch.OK
    assert np.allclose(_host_x(S, Lf), np.sqrt(2.0) * x0, rtol=1e-13, atol=0)
    _finish(S, Lf, A, A3)


def case_n1():
    S = ch.Session()
    one = np.array([0, 1], dtype=np.int64)
    A = S.sparse(1, one, np.zeros(1, dtype=np.int64), np.array([4.0]), -1)
    Lf = S.analyze(A)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    assert S.factorize_device(A, _dev(np.array([9.0])), Lf, 7.0) == 1 and S.cm.status == ch.OK
    assert _host_x(S, Lf)[0] == 4.0
    X = S.solve_device(Lf, _dev(np.array([32.0])))
    assert float(X[0]) == 2.0
    # A*A' of a 1 x 1 matrix
    M = FM.one_by_one()
    A1 = _rect(S, M)
    L1 = S.L.cholmod_l_analyze(A1, C.byref(S.cm))
    assert L1 and S.factorize(A1, L1) == 1 and S.cm.status == ch.OK
    assert S.factorize_device(A1, _dev(np.array([3.0])), L1) == 1 and S.cm.status == ch.OK
    assert _host_x(S, L1)[0] == 3.0
    S.free_factor(L1)
    _finish(S, Lf, A, A1)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
