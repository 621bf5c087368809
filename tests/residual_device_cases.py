"""The bodies of tests/test_gpu_residual_device.py, run in a process of their own: `python residual_device_cases.py CASE
[ARG ...]`, torch imported FIRST (see solve_device_cases.py, whose matrices and helpers these cases share).  Exit status
0 = every assertion held; a line `RESULT <json>` carries figures back.

The componentwise bound of a residual ("check 1").  R = B - beta X - A X is, for every entry, one sum of at most m + 2
terms, m the largest number of entries in a row of the full symmetric A.  Whatever the order of summation, a computed sum of
k terms t_i is off by at most gamma_k sum |t_i|, gamma_k = k eps / (1 - k eps), and each product adds one rounding (none
where it is fused): (m + 3) eps (|B| + |beta| |X| + |A| |X|) bounds the error of either side, the device's and numpy's, and
twice that their difference.  eps = 2^-53.  Nothing is measured, and the scale of the matrix does not enter."""
import torch  # noqa: E402  (first)

import ctypes as C
import json
import os
import sys

import numpy as np

import solve_device_cases as SD
from solve_device_cases import CASES, REFERENCE_INPUTS, TOL, _dev, _done, _factor, _relcols
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

EPS = 2.0 ** -53
NRHS = [1, 2, 7, 8, 15, 16, 17, 40]


class Sym:
    """the symmetric matrix a factorization is of, lower triangle by columns, plus beta I"""

    def __init__(self, n, Ap, Ai, Ax, beta=0.0):
        self.n, self.Ap, self.Ai, self.Ax, self.beta = n, np.asarray(Ap), np.asarray(Ai), np.asarray(Ax, dtype=np.float64), beta
        cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.Ap))
        cnt = np.bincount(self.Ai, minlength=n) + np.bincount(cols[self.Ai != cols], minlength=n)
        self.m = int(cnt.max()) if n else 0

    def mv(self, x, absolute=False):
        return G.sym_matvec(self.n, self.Ap, self.Ai, np.abs(self.Ax) if absolute else self.Ax, -1, np.abs(x) if absolute else x)

    def residual(self, x, b):
        """(B - beta X - A X, its bound), row by row of the (nrhs, n) arrays"""
        x, b = np.atleast_2d(x), np.atleast_2d(b)
        r = np.stack([b[k] - self.beta * x[k] - self.mv(x[k]) for k in range(x.shape[0])])
        bound = np.stack([2 * (self.m + 3) * EPS * (np.abs(b[k]) + abs(self.beta) * np.abs(x[k]) + self.mv(x[k], True)) + 1e-300
                          for k in range(x.shape[0])])
        return r, bound


def _worst(Rd, ref, bound):
    """largest |Rd - ref| / bound over the entries (a NaN counts as a miss)"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.abs(np.atleast_2d(Rd) - ref) / bound
    return float(np.where(np.isfinite(q), q, 1e300).max()) if q.size else 0.0


def _check1(M, Rt, nrm, x, b, tag):
    """check 1 on a device residual Rt (and its norms, if any) for the host copies x, b of what it was formed from"""
    Rd = np.atleast_2d(Rt.cpu().numpy())
    ref, bound = M.residual(x, b)
    w = _worst(Rd, ref, bound)
    print(f"{tag}: m={M.m} worst |R_dev - R_ref| / bound = {w:.3e}")
    assert w <= 1.0, (tag, w)
    if nrm is not None:
        assert np.array_equal(nrm.cpu().numpy().view(np.int64), np.abs(Rd).max(axis=1).view(np.int64)), tag
    return w


def case_residual(name, beta):
    beta = float(beta)
    n, Ap, Ai, Ax, perm = CASES[name]()
    S = ch.Session()
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK
    M = Sym(n, Ap, Ai, Ax, beta)
    rng = np.random.default_rng(21)
    for nrhs in NRHS:
        x, b = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
        R, nrm = S.residual_device(Lf, _dev(x), _dev(b), norms=True)
        assert R.shape == (nrhs, n) and nrm.shape == (nrhs,)
        _check1(M, R, nrm, x, b, f"{name} beta={beta} nrhs={nrhs}")
    # a single vector of shape (n,)
    r1 = S.residual_device(Lf, _dev(x[0]), _dev(b[0]))
    assert r1.shape == (n,)
    _check1(M, r1, None, x[0], b[0], f"{name} beta={beta} vector")
    _done(S, A, Lf)


def case_reproducible():
    n, Ap, Ai, Ax, perm = CASES["box9r2_nd"]()
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    rng = np.random.default_rng(22)
    for nrhs in (5, 33):
        X, B = _dev(rng.standard_normal((nrhs, n))), _dev(rng.standard_normal((nrhs, n)))
        R1, n1 = S.residual_device(Lf, X, B, norms=True)
        R2, n2 = S.residual_device(Lf, X, B, norms=True)
        assert torch.equal(R1, R2) and torch.equal(n1, n2), nrhs
    _done(S, A, Lf)


def case_values(nrhs):
    """the second factorization of a pattern goes through the values-only upload: the residual is that of the new values"""
    nrhs = int(nrhs)
    n, Ap, Ai, Ax = SD._big_supernode_matrix(1.0)
    perm = np.arange(n, dtype=np.int64)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    rng = np.random.default_rng(23)
    x, b = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
    X, B = _dev(x), _dev(b)
    R, nrm = S.residual_device(Lf, X, B, norms=True)
    _check1(Sym(n, Ap, Ai, Ax), R, nrm, x, b, f"values nrhs={nrhs} first")
    r_a = R.cpu().numpy()
    _, _, _, Ax2 = SD._big_supernode_matrix(1.5)
    S.free_sparse(A)
    A = S.sparse(n, Ap, Ai, Ax2, -1)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    R, nrm = S.residual_device(Lf, X, B, norms=True)
    _check1(Sym(n, Ap, Ai, Ax2), R, nrm, x, b, f"values nrhs={nrhs} second")
    assert _relcols(R.cpu().numpy(), r_a) > 1e-6
    _done(S, A, Lf)


def case_layout():
    n, Ap, Ai, Ax, perm = CASES["p3d_12_nd"]()
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    M = Sym(n, Ap, Ai, Ax)
    rng = np.random.default_rng(24)
    ld = n + 7
    for nrhs in (1, 5, 18):
        x, b = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
        Xp = torch.full((nrhs, ld), 555.0, dtype=torch.float64, device="cuda")
        Bp = torch.full((nrhs, ld), -777.0, dtype=torch.float64, device="cuda")
        Rp = torch.full((nrhs, ld), 333.0, dtype=torch.float64, device="cuda")
        Xp[:, :n], Bp[:, :n] = _dev(x), _dev(b)
        X0, B0 = Xp.clone(), Bp.clone()
        out, nrm = S.residual_device(Lf, Xp[:, :n], Bp[:, :n], out=Rp[:, :n], norms=True)
        assert out.data_ptr() == Rp.data_ptr()
        assert torch.equal(Xp, X0) and torch.equal(Bp, B0)             # inputs and their padding rows unchanged
        assert bool((Rp[:, n:] == 333.0).all())                         # padding rows of R unchanged
        _check1(M, Rp[:, :n], nrm, x, b, f"layout nrhs={nrhs}")
        # in place, R is B: the same bits
        S.residual_device(Lf, Xp[:, :n], Bp[:, :n], out=Bp[:, :n])
        assert torch.equal(Bp[:, :n], Rp[:, :n]) and bool((Bp[:, n:] == -777.0).all()) and torch.equal(Xp, X0)
        # refinement in the padded layout: B and the padding of X untouched
        Bp[:, :n] = _dev(b)
        B0 = Bp.clone()
        S.refine_device(Lf, Bp[:, :n], Xp[:, :n], steps=1)
        assert torch.equal(Bp, B0) and bool((Xp[:, n:] == 555.0).all())
        assert _relcols(Xp[:, :n].cpu().numpy(), S.solve(Lf, b)) < TOL
    # nrhs == 0: TRUE, nothing touched
    E = torch.empty((0, n), dtype=torch.float64, device="cuda")
    assert S.residual_device(Lf, E, E.clone()).shape == (0, n)
    assert S.refine_device(Lf, E, E.clone()).shape == (0, n)
    Xk, Bk, Rk = (torch.full((2, n), v, dtype=torch.float64, device="cuda") for v in (3.0, 4.0, 5.0))
    ok = S.L.cholmod_l_hip_residual_device(Lf, Xk.data_ptr(), n, Bk.data_ptr(), n, Rk.data_ptr(), n, 0, None, None, C.byref(S.cm))
    assert ok == 1 and S.cm.status == ch.OK
    ok = S.L.cholmod_l_hip_refine_device(Lf, Bk.data_ptr(), n, Xk.data_ptr(), n, 0, 1, None, None, C.byref(S.cm))
    torch.cuda.synchronize()
    assert ok == 1 and S.cm.status == ch.OK
    assert bool((Xk == 3.0).all()) and bool((Bk == 4.0).all()) and bool((Rk == 5.0).all())
    # R must not be X
    S.cm.error_handler = ch.ERRFUNC(0)
    ok = S.L.cholmod_l_hip_residual_device(Lf, Xk.data_ptr(), n, Bk.data_ptr(), n, Xk.data_ptr(), n, 2, None, None, C.byref(S.cm))
    assert ok == 0 and S.cm.status == ch.INVALID
    _done(S, A, Lf)


def case_stream():
    n, Ap, Ai, Ax, perm = CASES["p2d_60_nd"]()
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    M = Sym(n, Ap, Ai, Ax)
    rng = np.random.default_rng(25)
    s = torch.cuda.Stream()
    for nrhs in (4, 33, 2, 1):                                       # the workspaces grow, then shrink
        b = rng.standard_normal((nrhs, n))
        c = rng.standard_normal((nrhs, n))
        half, Ct = _dev(0.5 * b), _dev(c)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            # B from a chain of torch ops on s, X from solve_device, R consumed on s; no synchronisation in between
            Bt = half
            for _ in range(20):
                Bt = Bt * 1.0 + 0.0
            Bt = Bt + half
            X = S.solve_device(Lf, Bt)
            R = S.residual_device(Lf, X, Ct)
            Y = R * 2.0
            Xr, nrm = S.refine_device(Lf, Bt, X.clone(), steps=1, norms=True)
            Z = Xr + 0.0
        s.synchronize()
        x = X.cpu().numpy()
        ref, bound = M.residual(x, c)
        w = _worst(Y.cpu().numpy(), 2.0 * ref, 2.0 * bound)
        print(f"stream nrhs={nrhs}: worst / bound {w:.3e}")
        assert w <= 1.0, (nrhs, w)
        assert _relcols(Z.cpu().numpy(), S.solve(Lf, b)) < TOL, nrhs
    _done(S, A, Lf)


def case_refine(name):
    n, Ap, Ai, Ax, perm = CASES[name]()
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    M = Sym(n, Ap, Ai, Ax)
    rng = np.random.default_rng(26)
    for nrhs in (3, 16, 20):
        b = rng.standard_normal((nrhs, n))
        xs = np.atleast_2d(S.solve(Lf, b))
        x0 = xs * (1.0 + 1e-3 * rng.standard_normal((nrhs, n)))
        B, X = _dev(b), _dev(x0)
        # steps = 0: X bit for bit, the norms of check 1
        X00 = X.clone()
        out, nrm0 = S.refine_device(Lf, B, X, steps=0, norms=True)
        assert out.data_ptr() == X.data_ptr() and torch.equal(X, X00)
        R, nrmR = S.residual_device(Lf, X, B, norms=True)
        _check1(M, R, nrmR, x0, b, f"refine {name} nrhs={nrhs} start")
        assert torch.equal(nrm0, nrmR)
        # one step: the solution, and what the same step gives on the host
        out = S.refine_device(Lf, B, X, steps=1)
        assert out.data_ptr() == X.data_ptr()
        x1 = X.cpu().numpy()
        r0 = np.stack([b[k] - M.mv(x0[k]) for k in range(nrhs)])
        host = x0 + np.atleast_2d(S.solve(Lf, r0))
        e1, e2 = _relcols(x1, xs), _relcols(x1, host)
        print(f"refine {name} nrhs={nrhs}: vs solve {e1:.2e}, vs host restatement {e2:.2e}")
        assert e1 < TOL and e2 < TOL, (nrhs, e1, e2)
        # two more steps from the converged X: the residual stays at rounding level
        _, nrm2 = S.refine_device(Lf, B, X, steps=2, norms=True)
        _, bound = M.residual(X.cpu().numpy(), b)
        n2, lim = nrm2.cpu().numpy(), 2.0 * bound.max(axis=1)
        print(f"refine {name} nrhs={nrhs}: norms after two more steps / (2 x bound) = {(n2 / lim).max():.3e}")
        assert bool((n2 <= lim).all()), (nrhs, n2, lim)
    _done(S, A, Lf)


def case_reference_inputs():
    """check 1, nrhs = 5, on every file of REFERENCE_INPUTS, set up as solve_device_cases.case_reference_inputs does"""
    from test_tcov_matrices import _load, _library_matrix
    out = {}
    for d, f in REFERENCE_INPUTS:
        case = _load(d, f)
        assert not case["cx"] and case["n"] > 0
        n = case["n"]
        S = ch.Session(postorder=True)
        S.cm.error_handler = ch.ERRFUNC(0)
        A = _library_matrix(S, case)
        Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
        assert Lf and S.cm.status == ch.OK
        b2 = (C.c_double * 2)(case["beta"], 0.0)
        assert S.L.cholmod_l_factorize_p(A, C.byref(b2), None, 0, Lf, C.byref(S.cm)) == 1 and S.cm.status == ch.OK
        M = Sym(n, case["Lp"], case["Li"], case["Lx"], case["beta"])
        rng = np.random.default_rng(1)
        x, b = rng.standard_normal((5, n)), rng.standard_normal((5, n))
        R, nrm = S.residual_device(Lf, _dev(x), _dev(b), norms=True)
        Rd = R.cpu().numpy()
        ref, bound = M.residual(x, b)
        w = _worst(Rd, ref, bound)
        same = bool(np.array_equal(nrm.cpu().numpy().view(np.int64), np.abs(Rd).max(axis=1).view(np.int64)))
        print(f"{d}/{f}: n={n} m={M.m} beta={case['beta']} worst / bound {w:.3e}, norms bit-equal {same}")
        out[f"{d}/{f}"] = [w, same]
        _done(S, A, Lf)
    print("RESULT " + json.dumps(out))


def case_poisson100(out_path=""):
    """Poisson 100^3, 16 right-hand sides: residual_device against solve_device in one process, torch events on the
    current stream, median of five after a warm-up.  The residual moves S and its index once and at most one 128-byte
    line of X per entry; the solve moves L twice."""
    n, Ap, Ai, Ax = G.poisson3d(100)
    perm = G.geometric_nd(100, 100, 100, 4)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    M = Sym(n, Ap, Ai, Ax)
    rng = np.random.default_rng(4)
    x, b = rng.standard_normal((16, n)), rng.standard_normal((16, n))
    X, B = _dev(x), _dev(b)
    R = torch.empty_like(X)
    Xs = torch.empty_like(X)

    def median(run):
        run()
        torch.cuda.synchronize()
        t = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return float(np.median(t))

    t_res = median(lambda: S.residual_device(Lf, X, B, out=R))
    t_nrm = median(lambda: S.residual_device(Lf, X, B, out=R, norms=True))
    t_sol = median(lambda: S.solve_device(Lf, B, out=Xs))
    t_ref = median(lambda: S.refine_device(Lf, B, Xs, steps=1))
    _check1(M, R, None, x, b, "100^3 nrhs=16")
    # traffic model of one call, bytes: the column walk (index + value, 16 B per entry of S), the transposed index (column,
    # position, value: 20 B per entry below the diagonal), one 128 B line of X per term, the row's own lines of X, B, R,
    # the pointers, and the two packs and the unpack (read 128 B, write 128 B per row each)
    nnz, low = int(Ap[-1]), int(Ap[-1]) - n
    model = 16 * nnz + 20 * low + 128 * (nnz + low) + 3 * 128 * n + 24 * n + 3 * 256 * n
    res = {"case": "poisson3d(100), geometric_nd, nrhs=16", "n": n, "nnz_lower": nnz,
           "residual_device_ms": t_res, "residual_device_with_norms_ms": t_nrm, "solve_device_ms": t_sol,
           "refine_device_1_step_ms": t_ref, "traffic_model_bytes": model, "residual_model_GBps": model / (1e6 * t_res),
           "timing": "torch.cuda.Event on the current stream around one call, median of five after a warm-up call"}
    print(f"100^3 nrhs=16: residual {t_res:.3f} ms ({res['residual_model_GBps']:.0f} GB/s of its model), with norms {t_nrm:.3f} ms, "
          f"solve {t_sol:.3f} ms, one refinement step {t_ref:.3f} ms")
    print("RESULT " + json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    assert t_res > 0 and t_sol > 0
    assert t_res < 0.5 * t_sol, (t_res, t_sol)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
