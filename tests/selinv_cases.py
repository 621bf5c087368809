"""The bodies of tests/test_gpu_selinv.py, run in a process of their own: `python selinv_cases.py CASE [ARG ...]`, torch
imported FIRST (see solve_device_cases.py).  Exit status 0 = every assertion held; a line `RESULT <json>` carries figures
back.  Matrices, the dense reference and the bar -- max |Z - Z_ref| <= max (1e-12, 20 eps / rcond) max |Z_ref| over the
stored lower trapezoids, rcond = (min L_jj / max L_jj)^2 -- come from tests/selinv_reference.py."""
import torch  # noqa: E402  (first)

import ctypes as C
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import selinv_reference as R
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

BETA = 0.375


def _done(S, A, Lf):
    torch.cuda.synchronize()
    S.free_factor(Lf)
    if A:
        S.free_sparse(A)
    S.finish()


def _info(S, Lf):
    out = np.zeros(8)
    assert S.L.cholmod_hip_selinv_info(Lf.contents.hip_plan, out.ctypes.data) == ch.HIP_OK
    return out


def _entry_positions(fv, rows, cols):
    """index in Zx of Z (r, c), r >= c in the factor's ordering (-1: outside the pattern of L)"""
    out = np.full(len(rows), -1, dtype=np.int64)
    t = np.searchsorted(fv.super, cols, side="right") - 1
    for k in range(len(rows)):
        trows = fv.s[fv.pi[t[k]]:fv.pi[t[k] + 1]]
        q = int(np.searchsorted(trows, rows[k]))
        if q < len(trows) and trows[q] == rows[k]:
            out[k] = fv.px[t[k]] + (cols[k] - fv.super[t[k]]) * len(trows) + q
    return out


def case_entries():
    """every matrix of the table with beta = 0 and beta = 0.375, and two once more through the generic kernels only:
    Session.selinv_host against the dense inverse, the dead upper triangles exact zeros"""
    out = {}
    runs = [(name, beta, 0) for name in sorted(R.CASES) for beta in (0.0, BETA)]
    runs += [(name, 0.0, ch.HIP_NO_SMALL_FRONTS) for name in ("p3d_12_nd", "box9r2_nd")]
    for name, beta, flags in runs:
        case = R.CASES[name]()
        S, A, Lf = R.factorized(case, use_gpu=1, beta=beta, hip_flags=flags)
        fv = ch.FactorView(Lf)
        Zx = S.selinv_host(Lf)
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        err, tol, dead = R.compare(ch.FactorView(Lf), Zx, case["n"], case["Lp"], case["Li"], case["Lx"], beta)
        info = _info(S, Lf)
        key = f"{name}|{beta}|{flags}"
        print(f"{key}: n={case['n']} nsuper={fv.nsuper} err={err:.2e} tol={tol:.2e} dead={dead} launches={int(info[1])}")
        out[key] = [err if np.isfinite(err) else 1e300, tol, dead]
        _done(S, A, Lf)
    print("RESULT " + json.dumps(out))


def _gather_check(S, A, Lf, case, Ap, Ai, stype, tag):
    """selinv_device on the matrix (Ap, Ai, stype): values and diagonal bit for bit those of Zx, NaN exactly where the
    factorization does not read A, and the dense inverse at the bar"""
    n = case["n"]
    Z, d = S.selinv_device(A, Lf)
    torch.cuda.synchronize()
    Z, d = Z.cpu().numpy(), d.cpu().numpy()
    Zx = S.selinv_host(Lf)
    S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    fv = ch.FactorView(Lf)
    iperm = np.empty(n, dtype=np.int64)
    iperm[fv.Perm] = np.arange(n)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    read = (Ai >= cols) if stype < 0 else (Ai <= cols)
    pr, pc = iperm[Ai], iperm[cols]
    pos = _entry_positions(fv, np.maximum(pr, pc), np.minimum(pr, pc))
    assert np.all(pos[read] >= 0), tag
    assert np.all(np.isnan(Z[~read])), tag
    assert np.array_equal(Z[read].view(np.int64), Zx[pos[read]].view(np.int64)), tag
    dpos = _entry_positions(fv, np.arange(n), np.arange(n))
    assert np.array_equal(d[fv.Perm].view(np.int64), Zx[dpos].view(np.int64)), tag
    Zd = np.linalg.inv(R.dense_symmetric(n, case["Lp"], case["Li"], case["Lx"]))
    tol = R.tolerance(R.factor_rcond(fv)) * np.abs(Zd).max()
    e1, e2 = np.abs(Z[read] - Zd[Ai[read], cols[read]]).max(), np.abs(d - np.diag(Zd)).max()
    print(f"{tag}: values {e1:.2e} diag {e2:.2e} tol {tol:.2e}, {int((~read).sum())} NaN")
    assert e1 <= tol and e2 <= tol, (tag, e1, e2, tol)
    return Zx, fv, dpos


def case_gather():
    case = R.CASES["p3d_12_nd"]()
    n = case["n"]
    Lo = sp.csc_matrix((case["Lx"], case["Li"], case["Lp"]), shape=(n, n))
    # lower-stored, upper-stored, and both triangles present with junk in the ignored (upper) one
    Up = sp.csc_matrix(Lo.T)
    junk = sp.csc_matrix(Lo + sp.triu(Up, 1) * 1e30)
    for tag, M, stype in (("lower", Lo, -1), ("upper", Up, 1), ("junk", junk, -1)):
        M.sort_indices()
        Ap, Ai, Ax = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)
        S = ch.Session()
        A = S.sparse(n, Ap, Ai, Ax, stype)
        Lf = S.analyze(A, case["perm"])
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        Zx, fv, dpos = _gather_check(S, A, Lf, case, Ap, Ai, stype, tag)
        if tag == "lower":
            # the diagonal at the engine level, in both orderings (Perm is no identity here)
            assert not np.array_equal(fv.Perm, np.arange(n))
            plan = Lf.contents.hip_plan
            for perm in (0, 1):
                dd = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
                assert S.L.cholmod_hip_selinv_gather_device(plan, None, 0, dd.data_ptr(), perm, None) == ch.HIP_OK
                torch.cuda.synchronize()
                got = dd.cpu().numpy()
                want = Zx[dpos]
                assert np.array_equal((got[fv.Perm] if perm else got).view(np.int64), want.view(np.int64)), perm
            # a wrong nvalues is refused
            zz = torch.zeros(len(Ai) + 1, dtype=torch.float64, device="cuda")
            assert S.L.cholmod_hip_selinv_gather_device(plan, zz.data_ptr(), len(Ai) + 1, None, 0, None) == ch.HIP_INVALID
        _done(S, A, Lf)


def case_stale():
    case = R.CASES["box9r2_nd"]()
    n = case["n"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    plan = Lf.contents.hip_plan
    lib = S.L
    xsize = int(Lf.contents.xsize)
    z1, z2, z3 = np.zeros(xsize), np.zeros(xsize), np.zeros(xsize)
    # nothing computed yet: gather and download are refused
    assert _info(S, Lf)[6] == 0
    dd = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert lib.cholmod_hip_selinv_download(plan, z1.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_selinv_gather_device(plan, None, 0, dd.data_ptr(), 0, None) == ch.HIP_INVALID
    # two calls: the same bits
    assert lib.cholmod_hip_selinv_device(plan, None) == ch.HIP_OK and _info(S, Lf)[6] == 1
    assert lib.cholmod_hip_selinv_download(plan, z1.ctypes.data) == ch.HIP_OK
    assert lib.cholmod_hip_selinv_device(plan, None) == ch.HIP_OK
    assert lib.cholmod_hip_selinv_download(plan, z2.ctypes.data) == ch.HIP_OK
    assert np.array_equal(z1.view(np.int64), z2.view(np.int64))
    # release, then a call: the same bits again
    assert lib.cholmod_hip_selinv_release(plan) == ch.HIP_OK and _info(S, Lf)[6] == 0 and _info(S, Lf)[4] == 0
    assert lib.cholmod_hip_selinv_download(plan, z3.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_selinv_device(plan, None) == ch.HIP_OK
    assert lib.cholmod_hip_selinv_download(plan, z3.ctypes.data) == ch.HIP_OK
    assert np.array_equal(z1.view(np.int64), z3.view(np.int64))
    # new values from the device: stale, refused, then the inverse of the new matrix
    scale = 1.0 + 0.5 * np.random.default_rng(32).uniform(size=n)
    cols = np.repeat(np.arange(n), np.diff(case["Lp"]))
    Lx2 = case["Lx"] * scale[case["Li"]] * scale[cols]
    assert S.factorize_device(A, torch.from_numpy(Lx2).cuda(), Lf) == 1 and S.cm.status == ch.OK
    assert _info(S, Lf)[6] == 0
    assert lib.cholmod_hip_selinv_download(plan, z3.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_selinv_gather_device(plan, None, 0, dd.data_ptr(), 0, None) == ch.HIP_INVALID
    Zx = S.selinv_host(Lf)
    assert _info(S, Lf)[6] == 1
    lib.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    err, tol, dead = R.compare(ch.FactorView(Lf), Zx, n, case["Lp"], case["Li"], Lx2)
    print(f"stale: after factorize_device err={err:.2e} tol={tol:.2e}")
    assert err <= tol and dead == 0
    assert not np.array_equal(Zx, z1)
    _done(S, A, Lf)
    # a small scratch budget cuts the batches into chunks (p3d_12_nd: two generic fronts below the root share a batch):
    # more launches, the same bits
    case = R.CASES["p3d_12_nd"]()
    got = []
    for mb in (None, "0.25"):
        if mb:
            os.environ["CHOLMOD_HIP_SELINV_BUDGET_MB"] = mb
        S, A, Lf = R.factorized(case, use_gpu=1)
        got.append((S.selinv_host(Lf), _info(S, Lf)[1], _info(S, Lf)[5]))
        _done(S, A, Lf)
    del os.environ["CHOLMOD_HIP_SELINV_BUDGET_MB"]
    print(f"stale: launches {int(got[0][1])} (scratch {int(got[0][2])} B), with a 0.25 MB budget {int(got[1][1])} ({int(got[1][2])} B)")
    assert np.array_equal(got[0][0].view(np.int64), got[1][0].view(np.int64))
    assert got[1][1] > got[0][1] and got[1][2] < got[0][2]


def _launch_bound(S, Lf):
    fv = ch.FactorView(Lf)
    batch = np.zeros(fv.nsuper, dtype=np.int64)
    S.L.cholmod_hip_get_batches(Lf.contents.hip_plan, batch.ctypes.data, None)
    nblk = (np.diff(fv.super) + 63) // 64
    most = np.zeros(int(batch.max()) + 1, dtype=np.int64)
    np.maximum.at(most, batch, nblk)
    return 8 * int(most.sum()) + 8 * len(most) + 16


def case_launches(name):
    if name == "p2d_60_nd":
        n, Ap, Ai, Ax = G.poisson2d(60)
        perm = G.geometric_nd(60, 60, 1, 4)
    else:
        n, Ap, Ai, Ax = G.poisson2d(300)
        perm = G.geometric_nd(300, 300, 1, 4)
    S = ch.Session()
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    _, d = S.selinv_device(None, Lf, values=False)
    torch.cuda.synchronize()
    info, bound = _info(S, Lf), _launch_bound(S, Lf)
    m = 60 if name == "p2d_60_nd" else 300
    ref = _poisson_inverse_trace(m, m)
    err = abs(float(d.sum().item()) - ref) / ref
    print(f"launches {name}: nsuper={int(Lf.contents.nsuper)} launches={int(info[1])} bound={bound} trace err {err:.2e}")
    assert 0 < info[1] <= bound, (info[1], bound)
    assert err <= 1e-12, err
    _done(S, A, Lf)


def _poisson_inverse_trace(*dims):
    """sum_k 1 / lambda_k of the Dirichlet Poisson matrix on a grid: lambda = 2 d - 2 sum cos (i pi / (m + 1))"""
    lam = np.zeros(1)
    for m in dims:
        lam = np.add.outer(lam, 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))).ravel()
    return float(np.sum(1.0 / np.sort(lam)[::-1]))


def case_poisson40():
    """Poisson 40^3 (n = 64 000): trace (A Z) = n from the entries on A's pattern, sum_j Z_jj in closed form, 16 columns of
    Z against Session.solve, and the launch bound"""
    m = 40
    n, Ap, Ai, Ax = G.poisson3d(m)
    perm = G.geometric_nd(m, m, m, 4)
    S = ch.Session()
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, perm)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    Z, d = S.selinv_device(A, Lf)
    torch.cuda.synchronize()
    Z, d = Z.cpu().numpy(), d.cpu().numpy()
    info, bound = _info(S, Lf), _launch_bound(S, Lf)
    print(f"40^3: selinv {1e3 * info[0]:.2f} ms, {int(info[1])} launches (bound {bound}), hot product "
          f"{info[2] / max(info[0], 1e-30) / 1e12:.2f} TFLOP/s, Zx {info[4] / 2**20:.0f} MiB, scratch {info[5] / 2**20:.0f} MiB")
    assert 0 < info[1] <= bound, (info[1], bound)
    cols = np.repeat(np.arange(n), np.diff(Ap))
    off = Ai != cols
    tr = float(np.sum(Ax[~off] * Z[~off]) + 2.0 * np.sum(Ax[off] * Z[off]))
    e_tr = abs(tr - n) / n
    ref = _poisson_inverse_trace(m, m, m)
    e_dg = abs(float(np.sum(d)) - ref) / ref
    print(f"40^3: |trace (A Z) - n| / n = {e_tr:.2e}, diagonal sum against the closed form {e_dg:.2e}")
    assert e_tr <= 1e-11 and e_dg <= 1e-12, (e_tr, e_dg)
    assert np.array_equal(d.view(np.int64), Z[~off].view(np.int64))      # the diagonal entries of A are its diagonal
    # 16 columns of Z at a fixed stride against solves with unit vectors
    Zx = S.selinv_host(Lf)
    S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    fv = ch.FactorView(Lf)
    tol = R.tolerance(R.factor_rcond(fv))
    worst, zmax = 0.0, 0.0
    for c in range(n // 32, n, n // 16)[:16]:
        k = int(np.searchsorted(fv.super, c, side="right")) - 1
        rows = fv.s[fv.pi[k]:fv.pi[k + 1]]
        jc = c - int(fv.super[k])
        col = Zx[int(fv.px[k]) + jc * len(rows) + jc:int(fv.px[k]) + (jc + 1) * len(rows)]
        e = np.zeros(n)
        e[fv.Perm[c]] = 1.0
        x = S.solve(Lf, e).ravel()
        want = x[fv.Perm[rows[jc:]]]
        worst, zmax = max(worst, float(np.abs(col - want).max())), max(zmax, float(np.abs(want).max()))
    print(f"40^3: 16 columns against solves: {worst / zmax:.2e} (tol {tol:.2e})")
    assert worst <= tol * zmax, (worst, zmax, tol)
    _done(S, A, Lf)


def case_stream():
    """selinv_device on a side stream behind the torch ops that produce the values and the factorization from them, its
    result consumed on that stream without a host wait; further calls allocate nothing"""
    case = R.CASES["p2d_60_nd"]()
    n = case["n"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    plan = Lf.contents.hip_plan
    s = torch.cuda.Stream()
    half = torch.from_numpy(0.5 * case["Lx"]).cuda()
    S.selinv_device(A, Lf)                  # (the workspaces exist from here on)
    torch.cuda.synchronize()
    for rep in range(2):
        with torch.cuda.stream(s):
            v = half
            for _ in range(20):
                v = v * 1.0 + 0.0
            v = v + half * (1.0 + rep)      # rep 0: A itself, rep 1: 1.5 A
            assert S.factorize_device(A, v, Lf) == 1 and S.cm.status == ch.OK
            Z, d = S.selinv_device(A, Lf)
            Y = d * 2.0
        s.synchronize()
        Zd = np.linalg.inv(R.dense_symmetric(n, case["Lp"], case["Li"], case["Lx"] * (1.0 + 0.5 * rep)))
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf))) * np.abs(Zd).max()
        err = np.abs(Y.cpu().numpy() - 2.0 * np.diag(Zd)).max()
        print(f"stream rep {rep}: diagonal {err:.2e} tol {2 * tol:.2e}")
        assert err <= 2 * tol, (rep, err, tol)
    # the engine's own calls, no torch allocation in between: the free memory of the device does not move
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        assert S.L.cholmod_hip_selinv_device(plan, s.cuda_stream) == ch.HIP_OK
        assert S.L.cholmod_hip_selinv_gather_device(plan, Z.data_ptr(), Z.numel(), d.data_ptr(), 1, s.cuda_stream) == ch.HIP_OK
    s.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    _done(S, A, Lf)


def case_refusals():
    # a complex factor: not installed
    n, Ap, Ai, Ax = G.poisson3d(6)
    Hx = G.hermitian_phases(n, Ap, Ai, Ax, seed=5)
    S = ch.Session()
    S.cm.error_handler = ch.ERRFUNC(0)
    A = S.sparse(n, Ap, Ai, Hx, -1)
    Lf = S.analyze(A)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    out = np.zeros(2 * int(Lf.contents.xsize) + 1)
    dd = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert S.L.cholmod_l_hip_selinv_to_host(Lf, out.ctypes.data, C.byref(S.cm)) == 0 and S.cm.status == ch.NOT_INSTALLED
    assert S.L.cholmod_l_hip_selinv_device(None, Lf, None, dd.data_ptr(), None, C.byref(S.cm)) == 0
    assert S.cm.status == ch.NOT_INSTALLED and np.all(out == 0)
    _done(S, A, Lf)
    # a factorization that is not positive definite: refused, L as it was
    from test_tcov_matrices import _load, _library_matrix
    case = _load("tcov", "2lo.tri")
    S = ch.Session()
    S.cm.error_handler = ch.ERRFUNC(0)
    A = _library_matrix(S, case)
    Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
    assert Lf and S.cm.status == ch.OK
    S.L.cholmod_l_factorize(A, Lf, C.byref(S.cm))
    assert S.cm.status == ch.NOT_POSDEF and Lf.contents.minor < Lf.contents.n
    S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    fv = ch.FactorView(Lf)
    x0, minor0 = None if fv.x is None else fv.x.copy(), fv.minor
    out = np.zeros(max(int(Lf.contents.xsize), 1))
    dd = torch.zeros(case["n"], dtype=torch.float64, device="cuda")
    assert S.L.cholmod_l_hip_selinv_to_host(Lf, out.ctypes.data, C.byref(S.cm)) == 0 and S.cm.status == ch.INVALID
    assert S.L.cholmod_l_hip_selinv_device(A, Lf, None, dd.data_ptr(), None, C.byref(S.cm)) == 0 and S.cm.status == ch.INVALID
    plan = Lf.contents.hip_plan
    if plan:
        assert S.L.cholmod_hip_selinv_device(plan, None) == ch.HIP_INVALID
    fv = ch.FactorView(Lf)
    assert fv.minor == minor0 and (x0 is None or np.array_equal(fv.x, x0)) and np.all(out == 0)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
