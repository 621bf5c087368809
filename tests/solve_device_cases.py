"""The bodies of tests/test_gpu_solve_device.py, run in a process of their own: `python solve_device_cases.py CASE [ARG]`.
torch is imported FIRST, before the engine library is loaded, so that torch and the engine share one HIP runtime (a
torch wheel brings its own; two runtimes in one process cannot both open the device).  The rest of the suite keeps the
system's runtime, which is why these cases do not run inside the pytest process.  Exit status 0 = every assertion
held; a line `RESULT <json>` carries figures back."""
import torch  # noqa: E402  (first: see above)

import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.oracle import OracleFactor, bind_blas
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

TOL = 1e-11
NRHS = [1, 2, 3, 15, 16, 17, 40]
CASES = {
    "p3d_12_nd": lambda: G.poisson3d(12) + (G.geometric_nd(12, 12, 12, 4),),
    "p2d_60_nd": lambda: G.poisson2d(60) + (G.geometric_nd(60, 60, 1, 4),),
    "box9r2_nd": lambda: G.box_stencil3d(9, 2) + (G.geometric_nd(9, 9, 9, 3),),
}


def _torch():
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _relcols(X, R):
    """largest relative 2-norm error over the columns (rows of the (nrhs, n) arrays)"""
    X, R = np.atleast_2d(X), np.atleast_2d(R)
    return max(np.linalg.norm(X[k] - R[k]) / np.linalg.norm(R[k]) for k in range(R.shape[0]))


def _factor(n, Ap, Ai, Ax, perm):
    S = ch.Session()
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    return S, A, Lf


def _done(S, A, Lf):
    _torch().cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def case_parity(name):
    n, Ap, Ai, Ax, perm = CASES[name]()
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    O = OracleFactor(n, Ap, Ai, -1, perm=perm, postorder=True)
    assert O.factorize(Ax) == 0
    rng = np.random.default_rng(11)
    for nrhs in NRHS:
        b = rng.standard_normal((nrhs, n))
        B = _dev(b)
        for sys in range(9):
            xh = np.atleast_2d(S.solve(Lf, b, sys))         # the unchanged host-array path
            xd = S.solve_device(Lf, B, sys).cpu().numpy()
            assert xd.shape == (nrhs, n)
            if sys in (ch.SYS_P, ch.SYS_Pt, ch.SYS_D):
                assert np.array_equal(xd, xh), (nrhs, sys)
                continue
            e = _relcols(xd, xh)
            print(f"{name} nrhs={nrhs} sys={sys}: device vs host path {e:.2e}")
            assert e < TOL, (nrhs, sys, e)
            if sys in (ch.SYS_L, ch.SYS_LD):
                assert _relcols(xd, O.lsolve(b)) < TOL, (nrhs, sys)
            elif sys in (ch.SYS_Lt, ch.SYS_DLt):
                assert _relcols(xd, O.ltsolve(b)) < TOL, (nrhs, sys)
            elif sys == ch.SYS_A:
                for k in range(nrhs):
                    r = G.sym_matvec(n, Ap, Ai, Ax, -1, xd[k]) - b[k]
                    assert np.linalg.norm(r) / np.linalg.norm(b[k]) < TOL, (nrhs, k)
        # a single vector of shape (n,)
        x1 = S.solve_device(Lf, B[0]).cpu().numpy()
        assert x1.shape == (n,) and _relcols(x1, S.solve(Lf, b[0])) < TOL
    _done(S, A, Lf)


def _big_supernode_matrix(scale):
    """a 1400-column supernode with 100 rows below it, followed by a dense 200-column root (the big-supernode walk
    in 256-column blocks with explicit 64 x 64 inverses)"""
    n1, n2 = 1400, 200
    n = n1 + n2
    rng = np.random.default_rng(7)
    M = rng.standard_normal((n, n)) * 0.05
    Ad = M @ M.T + np.eye(n) * 4.0
    mask = np.zeros((n, n), dtype=bool)
    mask[:n1, :n1] = True
    mask[n1:, n1:] = True
    mask[n1 + 100:, :n1] = True
    mask[:n1, n1 + 100:] = True
    Ad = np.where(mask, Ad, 0.0)
    Ad += np.eye(n) * (np.abs(Ad).sum(axis=1).max())
    Ad[:700, :700] *= scale                      # (scale != 1: other values on the same pattern, still diagonally dominant)
    ii, jj = np.nonzero(np.tril(mask))
    order = np.lexsort((ii, jj))
    Ai, cols = ii[order].astype(np.int64), jj[order]
    Ax = Ad[Ai, cols]
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    return n, Ap, Ai, Ax


def case_big_supernode(nrhs):
    nrhs = int(nrhs)
    n, Ap, Ai, Ax = _big_supernode_matrix(1.0)
    perm = np.arange(n, dtype=np.int64)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    fv = ch.FactorView(Lf)
    assert np.diff(fv.super).max() >= 1400 - 64
    rng = np.random.default_rng(3)
    b = rng.standard_normal((nrhs, n))
    B = _dev(b)

    def check(Ax_now):
        O = OracleFactor(n, Ap, Ai, -1, perm=perm, postorder=True)
        assert O.factorize(Ax_now) == 0
        y = S.solve_device(Lf, B, ch.SYS_L).cpu().numpy()
        assert _relcols(y, O.lsolve(b)) < TOL
        z = S.solve_device(Lf, B, ch.SYS_Lt).cpu().numpy()
        assert _relcols(z, O.ltsolve(b)) < TOL
        x = S.solve_device(Lf, B).cpu().numpy()
        for k in range(nrhs):
            r = G.sym_matvec(n, Ap, Ai, Ax_now, -1, x[k]) - b[k]
            assert np.linalg.norm(r) / np.linalg.norm(b[k]) < TOL
        assert _relcols(x, S.solve(Lf, b)) < TOL
        return x

    x_a = check(Ax)
    # a second factorization with other values: the cached inverses must follow them
    _, _, _, Ax2 = _big_supernode_matrix(1.5)
    S.free_sparse(A)
    A = S.sparse(n, Ap, Ai, Ax2, -1)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    x_b = check(Ax2)
    assert _relcols(x_b, x_a) > 1e-6             # the result follows the new values
    _done(S, A, Lf)


def case_layout():
    torch = _torch()
    n, Ap, Ai, Ax, perm = CASES["p3d_12_nd"]()
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    rng = np.random.default_rng(5)
    for nrhs in (1, 5, 18):
        b = rng.standard_normal((nrhs, n))
        ref = S.solve(Lf, b)
        ld = n + 7
        Bp = torch.full((nrhs, ld), -777.0, dtype=torch.float64, device="cuda")
        Xp = torch.full((nrhs, ld), 555.0, dtype=torch.float64, device="cuda")
        Bp[:, :n] = _dev(b)
        B0 = Bp.clone()
        out = S.solve_device(Lf, Bp[:, :n], out=Xp[:, :n])
        assert out.data_ptr() == Xp.data_ptr()
        assert torch.equal(Bp, B0)                                   # B and its padding rows unchanged
        assert bool((Xp[:, n:] == 555.0).all())                      # padding rows of X unchanged
        x = Xp[:, :n].cpu().numpy()
        assert _relcols(x, ref) < TOL
        # in place: the same X (the forward sweeps add into shared ancestor rows atomically, in either kind of
        # kernel, so two runs agree to rounding, not bit for bit: the project's bound)
        S.solve_device(Lf, Bp[:, :n], out=Bp[:, :n])
        assert _relcols(Bp[:, :n].cpu().numpy(), x) < TOL
        assert bool((Bp[:, n:] == -777.0).all())
    # nrhs == 0: TRUE, nothing touched
    E = torch.empty((0, n), dtype=torch.float64, device="cuda")
    assert S.solve_device(Lf, E).shape == (0, n)
    Bk = torch.full((2, n), 3.0, dtype=torch.float64, device="cuda")
    Xk = torch.full((2, n), 4.0, dtype=torch.float64, device="cuda")
    ok = S.L.cholmod_l_hip_solve_device(ch.SYS_A, Lf, Bk.data_ptr(), n, Xk.data_ptr(), n, 0, None, C.byref(S.cm))
    torch.cuda.synchronize()
    assert ok == 1 and S.cm.status == ch.OK
    assert bool((Bk == 3.0).all()) and bool((Xk == 4.0).all())
    _done(S, A, Lf)


def case_stream():
    torch = _torch()
    n, Ap, Ai, Ax, perm = CASES["p2d_60_nd"]()
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    rng = np.random.default_rng(9)
    s = torch.cuda.Stream()
    for nrhs in (4, 33, 2, 1):                                       # growth, then smaller again
        b = rng.standard_normal((nrhs, n))
        half = _dev(0.5 * b)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            # B is produced by a chain of torch ops on s, X is consumed on s; no synchronisation in between
            Bt = half
            for _ in range(20):
                Bt = Bt * 1.0 + 0.0
            Bt = Bt + half
            X = S.solve_device(Lf, Bt)
            Y = X * 2.0
        s.synchronize()
        ref = S.solve(Lf, b)
        assert _relcols(Y.cpu().numpy(), 2.0 * ref) < TOL, nrhs
    _done(S, A, Lf)


# the real-valued files of tests/test_tcov_matrices.py whose factorization returns CHOLMOD_OK (fixed on the CPU path)
REFERENCE_INPUTS = [
    ("tcov", "1_0"), ("tcov", "1e99"), ("tcov", "2.tri"), ("tcov", "20lo"), ("tcov", "2_3"), ("tcov", "2diag.tri"),
    ("tcov", "3_2"), ("tcov", "3b"), ("tcov", "4"), ("tcov", "4lo"), ("tcov", "5"), ("tcov", "5by50"), ("tcov", "C9840"),
    ("tcov", "a2"), ("tcov", "afiro"), ("tcov", "diag"), ("tcov", "ex5lo"), ("tcov", "galenet"), ("tcov", "ibm32"),
    ("tcov", "itest2"), ("tcov", "itest6"), ("tcov", "k01up"), ("tcov", "pi"), ("tcov", "plskz362.mtx"), ("tcov", "r5lo"),
    ("tcov", "r5lo2"), ("tcov", "r5up"), ("tcov", "r5up2"), ("tcov", "rza.mtx"), ("demo", "bcsstk01.tri"),
    ("demo", "bcsstk02.tri"), ("demo", "can___24.mtx"), ("demo", "lp_afiro.tri"), ("demo", "one.tri"),
    ("demo", "pts5ldd03.mtx"), ("demo", "two.tri"),
]


def case_reference_inputs():
    from test_tcov_matrices import _load, _library_matrix
    out = {}
    for d, f in REFERENCE_INPUTS:
        case = _load(d, f)
        assert not case["cx"] and case["n"] > 0
        n = case["n"]
        S = ch.Session(postorder=True)              # supernodal forced, natural ordering: as run_case sets a case up
        S.cm.error_handler = ch.ERRFUNC(0)
        A = _library_matrix(S, case)
        Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
        assert Lf and S.cm.status == ch.OK
        b2 = (C.c_double * 2)(case["beta"], 0.0)
        assert S.L.cholmod_l_factorize_p(A, C.byref(b2), None, 0, Lf, C.byref(S.cm)) == 1 and S.cm.status == ch.OK
        b = np.random.default_rng(1).standard_normal((5, n))
        xh = S.solve(Lf, b)
        xd = S.solve_device(Lf, _dev(b)).cpu().numpy()
        e = _relcols(xd, xh)
        print(f"{d}/{f}: n={n} device vs host path {e:.2e}")
        out[f"{d}/{f}"] = e if np.isfinite(e) else 1e300
        _done(S, A, Lf)
    print("RESULT " + json.dumps(out))


def case_poisson64():
    bind_blas()
    n, Ap, Ai, Ax = G.poisson3d(64)
    perm = G.geometric_nd(64, 64, 64, 4)
    O = OracleFactor(n, Ap, Ai, -1, perm=perm, postorder=True)
    assert O.factorize(Ax) == 0
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    b = np.random.default_rng(2).standard_normal((16, n))
    b[0] = G.demo_rhs(n)
    x = S.solve_device(Lf, _dev(b)).cpu().numpy()
    for k in range(16):
        xo = O.solve(b[k])
        e = np.linalg.norm(x[k] - xo) / np.linalg.norm(xo)
        print(f"64^3 column {k}: vs oracle {e:.2e}")
        assert e < 1e-10, (k, e)
    for k in (0, 15):
        e = _relcols(x[k], S.solve(Lf, b[k]))
        print(f"64^3 column {k}: vs host path {e:.2e}")
        assert e < TOL, (k, e)
    _done(S, A, Lf)


def case_poisson100():
    """Poisson 100^3, 16 right-hand sides: device time (stats [24], median of five after a warm-up) of the device
    path against the host-array path (the unchanged per-right-hand-side kernels) on the same factor.  The traffic
    argument gives 16 : 1; less than half is asked."""
    n, Ap, Ai, Ax = G.poisson3d(100)
    perm = G.geometric_nd(100, 100, 100, 4)
    S, A, Lf = _factor(n, Ap, Ai, Ax, perm)
    b = np.random.default_rng(4).standard_normal((16, n))
    B = _dev(b)

    def median(run):
        run()
        t = []
        for _ in range(5):
            run()
            t.append(float(S.hip_stats(Lf)[24]))
        return float(np.median(t))

    keep = {}
    t_host = median(lambda: keep.__setitem__("h", S.solve(Lf, b)))
    t_dev = median(lambda: keep.__setitem__("d", S.solve_device(Lf, B)))
    print(f"100^3 nrhs=16: host path {1e3 * t_host:.2f} ms, device path {1e3 * t_dev:.2f} ms, ratio {t_host / max(t_dev, 1e-30):.1f}")
    print("RESULT " + json.dumps({"host_ms": 1e3 * t_host, "device_ms": 1e3 * t_dev}))
    assert t_host > 0 and t_dev > 0
    assert _relcols(keep["d"].cpu().numpy(), keep["h"]) < TOL
    assert t_dev < 0.5 * t_host, (t_dev, t_host)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
