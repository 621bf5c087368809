"""The bodies of tests/test_gpu_factor_grad.py, run in a process of their own: `python factor_grad_cases.py CASE [ARG ...]`,
torch imported FIRST (see solve_device_cases.py).  Exit status 0 = every assertion held; a line `RESULT <json>` carries
figures back.  Matrices and the bar -- max |G - G_ref| <= max (1e-12, 20 eps / rcond) max |G_ref| over the stored lower
trapezoids, rcond = (min L_jj / max L_jj)^2 -- come from tests/selinv_reference.py, the dense formula of reverse-mode
Cholesky from tests/factor_grad_reference.py; every figure is printed before it is asserted."""
import torch  # noqa: E402  (first)

import ctypes as C
import json
import math
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import factor_grad_reference as F
import selinv_reference as R
from selinv_cases import _entry_positions, _launch_bound
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G
from suitesparse_amd.autograd import DeviceCholesky

BETA = 0.375
EPS = R.EPS


def _done(S, A, Lf):
    torch.cuda.synchronize()
    S.free_factor(Lf)
    if A:
        S.free_sparse(A)
    S.finish()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _info(S, Lf, which="factor_grad"):
    out = np.zeros(8)
    assert getattr(S.L, f"cholmod_hip_{which}_info")(Lf.contents.hip_plan, out.ctypes.data) == ch.HIP_OK
    return out


def _count(S, Lf):
    out = np.zeros(12, dtype=np.int64)
    assert S.L.cholmod_hip_progress(Lf.contents.hip_plan, out.ctypes.data) == ch.HIP_OK
    return int(out[0])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _host_factor(S, Lf):
    S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    return ch.FactorView(Lf)


def _dense_reference(case, fv, beta, Lbar_dense):
    """the dense formula on P (A + beta I) P' -> (G_ref sampled on the stored trapezoids, their mask)"""
    Ad = R.dense_symmetric(case["n"], case["Lp"], case["Li"], case["Lx"], beta)
    p = np.asarray(fv.Perm)
    Gd = F.dense_factor_grad(np.linalg.cholesky(Ad[np.ix_(p, p)]), Lbar_dense)
    return F.trapezoid_of(Gd, fv.super, fv.pi, fv.px, fv.s, fv.xsize)


def _compare(Gx, ref, mask):
    """-> (max |G - G_ref| / max |G_ref| over the stored trapezoids, entries != +0.0 bit for bit in the dead triangles)"""
    with np.errstate(invalid="ignore"):
        diff = np.abs(np.asarray(Gx)[mask] - ref[mask])
    err = float(np.where(np.isfinite(diff), diff, np.inf).max() / np.abs(ref[mask]).max())
    return err, int(np.count_nonzero(_bits(np.asarray(Gx)[~mask])))


def case_entries():
    """every matrix of the table with beta = 0 and beta = 0.375, and two once more through the generic kernels only: a
    seeded standard-normal Lbar on the lower trapezoids with 1e30 in the dead triangles, Session.factor_grad_host against
    the dense formula, the dead triangles of Gx exact zeros"""
    out = {}
    runs = [(name, beta, 0) for name in sorted(R.CASES) for beta in (0.0, BETA)]
    runs += [(name, 0.0, ch.HIP_NO_SMALL_FRONTS) for name in ("p3d_12_nd", "box9r2_nd")]
    for k, (name, beta, flags) in enumerate(runs):
        case = R.CASES[name]()
        S, A, Lf = R.factorized(case, use_gpu=1, beta=beta, hip_flags=flags)
        fv = _host_factor(S, Lf)
        Lbar_x, _ = F.random_lbar(fv, 100 + k, dead=1e30)
        S.factor_grad_device(A, Lf, _dev(Lbar_x))
        Gx = S.factor_grad_host(Lf)
        ref, mask = _dense_reference(case, fv, beta, F.dense_of_layout(fv, Lbar_x))
        err, dead = _compare(Gx, ref, mask)
        tol = R.tolerance(R.factor_rcond(fv))
        key = f"{name}|{beta}|{flags}"
        print(f"{key}: n={case['n']} nsuper={fv.nsuper} err={err:.2e} tol={tol:.2e} dead={dead} launches={int(_info(S, Lf)[1])}")
        out[key] = [err if np.isfinite(err) else 1e300, tol, dead]
        _done(S, A, Lf)
    print("RESULT " + json.dumps(out))


def case_selinv_special(name):
    """Lbar = diag (2 / L_jj): the gathered G is Z on the diagonal and 2 Z off it (selinv_device), +0.0 where Z is NaN, the
    trace is sum Z_ii, both within tol max |Z|"""
    case = R.CASES[name]()
    n, Ap, Ai = case["n"], case["Lp"], case["Li"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    fv = _host_factor(S, Lf)
    dpos = _entry_positions(fv, np.arange(n), np.arange(n))
    Lbar_x = np.zeros(fv.xsize)
    Lbar_x[dpos] = 2.0 / fv.x[dpos]
    Gv, tr = S.factor_grad_device(A, Lf, _dev(Lbar_x))
    Z, d = S.selinv_device(A, Lf)
    torch.cuda.synchronize()
    Gv, tr, Z, d = Gv.cpu().numpy(), float(tr), Z.cpu().numpy(), d.cpu().numpy()
    cols = np.repeat(np.arange(n), np.diff(Ap))
    nan = np.isnan(Z)
    m = np.where(Ai == cols, 1.0, 2.0)
    zmax = float(np.abs(Z[~nan]).max())
    tol = R.tolerance(R.factor_rcond(fv))
    e1 = float(np.abs(Gv[~nan] - m[~nan] * Z[~nan]).max())
    e2 = abs(tr - math.fsum(d))
    print(f"special {name}: |G - m Z| {e1:.2e}, |trace - sum Z_ii| {e2:.2e} (trace {tr!r}), bar {tol * zmax:.2e}; {int(nan.sum())} NaN")
    assert np.array_equal(_bits(Gv[nan]), np.zeros(int(nan.sum()), dtype=np.int64))
    assert e1 <= tol * zmax and e2 <= tol * zmax, (e1, e2, tol * zmax)
    _done(S, A, Lf)


def case_outer(name):
    """Lbar = alpha tril (P Q') formed on the device: nrhs 1, 3, 16, 17, once with ld > n, once with P and Q the same array;
    Gx against the dense formula at the bar; two calls give the same bits; nrhs = 0 gives all zeros"""
    case = R.CASES[name]()
    n = case["n"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    fv = _host_factor(S, Lf)
    tol = R.tolerance(R.factor_rcond(fv))
    rng = np.random.default_rng(21)
    for nrhs, alpha, variant in ((1, -1.0, ""), (3, -0.7, "wide"), (16, -1.0, "same"), (17, 1.3, "")):
        Pm = rng.standard_normal((nrhs, n))
        Qm = Pm if variant == "same" else rng.standard_normal((nrhs, n))
        if variant == "wide":           # ld > n: the rows of a wider tensor
            wide = torch.full((2 * nrhs, n + 5), float("nan"), dtype=torch.float64, device="cuda")
            wide[:nrhs, :n], wide[nrhs:, :n] = _dev(Pm), _dev(Qm)
            Pd, Qd = wide[:nrhs, :n], wide[nrhs:, :n]
        else:
            Pd = _dev(Pm)
            Qd = Pd if variant == "same" else _dev(Qm)
        Gv, tr = S.factor_outer_grad_device(A, Lf, Pd, Qd, alpha=alpha)
        Gx = S.factor_grad_host(Lf)
        Gv2, tr2 = S.factor_outer_grad_device(A, Lf, Pd, Qd, alpha=alpha)
        Gx2 = S.factor_grad_host(Lf)
        ref, mask = _dense_reference(case, fv, 0.0, alpha * np.tril(Pm.T @ Qm))
        err, dead = _compare(Gx, ref, mask)
        print(f"outer {name} nrhs={nrhs} alpha={alpha} {variant}: err={err:.2e} tol={tol:.2e} dead={dead}")
        assert err <= tol and dead == 0, (name, nrhs, err, tol, dead)
        assert np.array_equal(_bits(Gx), _bits(Gx2)), (name, nrhs)
        assert np.array_equal(_bits(Gv.cpu().numpy()), _bits(Gv2.cpu().numpy())) and _bits(tr.cpu().numpy()) == _bits(tr2.cpu().numpy())
    empty = torch.zeros((0, n), dtype=torch.float64, device="cuda")
    Gv, tr = S.factor_outer_grad_device(A, Lf, empty, empty)
    Gx = S.factor_grad_host(Lf)
    assert not Gx.any() and not Gv.cpu().numpy().any() and float(tr) == 0.0
    _done(S, A, Lf)


def case_gather():
    """factor_grad_device on lower-stored, upper-stored and junk-carrying input: G is the entries of Gx bit for bit, +0.0
    exactly where the selected inverse's gather gives NaN; the trace against math.fsum of the downloaded diagonal within
    (n + 2) eps sum |G_jj|; a wrong nvalues is refused; the autograd functions keep the +0.0 on entries that are not read"""
    case = R.CASES["p3d_12_nd"]()
    n = case["n"]
    Lo = sp.csc_matrix((case["Lx"], case["Li"], case["Lp"]), shape=(n, n))
    Up = sp.csc_matrix(Lo.T)
    junk = sp.csc_matrix(Lo + sp.triu(Up, 1) * 1e30)
    for tag, M, stype in (("lower", Lo, -1), ("upper", Up, 1), ("junk", junk, -1)):
        M.sort_indices()
        Ap, Ai, Ax = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)
        S = ch.Session()
        A = S.sparse(n, Ap, Ai, Ax, stype)
        Lf = S.analyze(A, case["perm"])
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        fv = _host_factor(S, Lf)
        Lbar_x, mask = F.random_lbar(fv, 31, dead=1e30)
        Gv, tr = S.factor_grad_device(A, Lf, _dev(Lbar_x))
        Gx = S.factor_grad_host(Lf)
        Z, _ = S.selinv_device(A, Lf, diag=False)
        torch.cuda.synchronize()
        Gv, tr, nan = Gv.cpu().numpy(), float(tr), np.isnan(Z.cpu().numpy())
        iperm = np.empty(n, dtype=np.int64)
        iperm[fv.Perm] = np.arange(n)
        cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
        read = (Ai >= cols) if stype < 0 else (Ai <= cols)
        pr, pc = iperm[Ai], iperm[cols]
        pos = _entry_positions(fv, np.maximum(pr, pc), np.minimum(pr, pc))
        assert np.array_equal(nan, ~read) and nan.any() == (tag == "junk") and np.all(pos[read] >= 0), tag
        assert np.array_equal(_bits(Gv[read]), _bits(Gx[pos[read]])), tag
        assert np.array_equal(_bits(Gv[nan]), np.zeros(int(nan.sum()), dtype=np.int64)), tag
        diag = Gx[_entry_positions(fv, np.arange(n), np.arange(n))]
        ref, bar = math.fsum(diag), (n + 2) * EPS * float(np.abs(diag).sum())
        print(f"gather {tag}: {int(read.sum())} entries bit for bit, {int(nan.sum())} zeros; trace {tr!r} against fsum {ref!r}: "
              f"{abs(tr - ref):.2e} (bar {bar:.2e})")
        assert abs(tr - ref) <= bar, tag
        plan = Lf.contents.hip_plan
        zz = torch.zeros(len(Ai) + 1, dtype=torch.float64, device="cuda")
        assert S.L.cholmod_hip_factor_grad_gather_device(plan, zz.data_ptr(), len(Ai) + 1, None, None) == ch.HIP_INVALID
        assert S.L.cholmod_hip_factor_grad_gather_device(plan, zz.data_ptr(), len(Ai), None, None) == ch.HIP_OK
        if tag == "junk":
            chol = DeviceCholesky(S, A, Lf)
            v = _dev(Ax).requires_grad_()
            z = _dev(np.random.default_rng(32).standard_normal((3, n)))
            (chol.solve_Lt(v, z).sum() + chol.solve_L(v, z).sum()).backward()
            g = v.grad.cpu().numpy()
            assert np.array_equal(_bits(g[~read]), np.zeros(int((~read).sum()), dtype=np.int64)) and np.all(g[read] != 0)
        _done(S, A, Lf)


def _torch_reference(n, Ap, Ai, Ax, perm, beta, Z, B, W, W2):
    """the loss (W . P' L^-T Z).sum () + (W2 . L^-1 P B).sum () from a dense float64 CPU matrix: torch.linalg.cholesky of the
    permuted matrix, then torch.linalg.solve_triangular; rows are right-hand sides"""
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    off = Ai != cols
    v = torch.tensor(Ax, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    Zt = torch.tensor(np.atleast_2d(Z), dtype=torch.float64, requires_grad=True)
    Bt = torch.tensor(np.atleast_2d(B), dtype=torch.float64, requires_grad=True)
    M = torch.zeros((n, n), dtype=torch.float64)
    M = M.index_put((torch.tensor(Ai), torch.tensor(cols)), v)
    M = M.index_put((torch.tensor(cols[off]), torch.tensor(Ai[off])), v[torch.tensor(np.nonzero(off)[0])])
    p = torch.tensor(np.asarray(perm))
    Mp = (M + b * torch.eye(n, dtype=torch.float64))[p][:, p]
    Mp.retain_grad()
    Lc = torch.linalg.cholesky(Mp)
    Xt = torch.linalg.solve_triangular(Lc.T, Zt.T, upper=True)                  # n x nrhs, the factor's ordering
    X = torch.zeros_like(Xt).index_put((p,), Xt).T
    Y = torch.linalg.solve_triangular(Lc, Bt.T[p], upper=False).T
    loss = (torch.tensor(np.atleast_2d(W)) * X).sum() + (torch.tensor(np.atleast_2d(W2)) * Y).sum()
    loss.backward()
    sh = np.shape(Z)
    return dict(X=X.detach().numpy().reshape(sh), Y=Y.detach().numpy().reshape(sh), gv=v.grad.numpy(), gZ=Zt.grad.numpy().reshape(sh),
                gB=Bt.grad.numpy().reshape(sh), gbeta=float(b.grad), diag_scale=float(Mp.grad.diagonal().abs().sum()))


def _check_autograd(tag, got, ref, tol):
    for key, scale in (("X", None), ("Y", None), ("gv", None), ("gZ", None), ("gB", None), ("gbeta", ref["diag_scale"])):
        bar = tol * (float(np.abs(ref[key]).max()) if scale is None else scale)
        err = float(np.abs(np.asarray(got[key]) - ref[key]).max())
        print(f"{tag}: {key} {err:.2e} (bar {bar:.2e})")
        assert err <= bar, (tag, key, err, bar)


def case_autograd(name):
    """loss = (W . chol.solve_Lt (v, Z)).sum () + (W2 . chol.solve_L (v, B)).sum () with beta a tensor that requires grad,
    beta 0 and 0.375, nrhs 1 and 19, against the dense torch reference: the forward within tol max |ref|, the gradients
    with respect to values, Z and B within tol max |ref gradient|, the one with respect to beta within tol sum |G_ref,jj|;
    +0.0 on entries that are not read; a second backward after the factor was replaced refactorizes from the saved values"""
    case = R.CASES[name]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    for beta in (0.0, BETA):
        S, A, Lf = R.factorized(case, use_gpu=1, beta=beta)
        fv = _host_factor(S, Lf)
        tol = R.tolerance(R.factor_rcond(fv))
        perm = fv.Perm.copy()
        bt = torch.tensor(beta, dtype=torch.float64, device="cuda", requires_grad=True)
        chol = DeviceCholesky(S, A, Lf, bt)
        other = _dev(Ax * np.where(Ai == cols, 2.0, 0.5))
        for nrhs in (1, 19):
            tag = f"autograd {name} beta={beta} nrhs={nrhs}"
            rng = np.random.default_rng(41)
            shape = (n,) if nrhs == 1 else (nrhs, n)
            Z, B, W, W2 = (rng.standard_normal(shape) for _ in range(4))
            ref = _torch_reference(n, Ap, Ai, Ax, perm, beta, Z, B, W, W2)
            v, Zd, Bd = _dev(Ax).requires_grad_(), _dev(Z).requires_grad_(), _dev(B).requires_grad_()
            c0 = _count(S, Lf)
            X, Y = chol.solve_Lt(v, Zd), chol.solve_L(v, Bd)
            assert _count(S, Lf) - c0 == 1 and X.shape == Zd.shape and Y.shape == Bd.shape, tag
            loss = (_dev(W) * X).sum() + (_dev(W2) * Y).sum()

            def grads():
                return dict(X=X.detach().cpu().numpy(), Y=Y.detach().cpu().numpy(), gv=v.grad.cpu().numpy(),
                            gZ=Zd.grad.cpu().numpy(), gB=Bd.grad.cpu().numpy(), gbeta=float(bt.grad))
            loss.backward(retain_graph=True)
            assert v.grad.shape == v.shape and Zd.grad.shape == Zd.shape and bt.grad.dim() == 0
            _check_autograd(tag, grads(), ref, tol)
            read = Ai >= cols
            assert np.array_equal(_bits(v.grad.cpu().numpy()[~read]), np.zeros(int((~read).sum()), dtype=np.int64))
            # the factor is replaced behind the wrapper's back: the second backward refactorizes from the saved values
            v.grad = Zd.grad = Bd.grad = bt.grad = None
            assert S.factorize_device(A, other, Lf, beta) == 1 and S.cm.status == ch.OK
            c1 = _count(S, Lf)
            loss.backward()
            assert _count(S, Lf) - c1 == 1, tag
            _check_autograd(tag + " (stale factor)", grads(), ref, tol)
            bt.grad = None
        _done(S, A, Lf)


def case_stale():
    """gather and download are refused before the first call and after factorize_device, and correct again after a new
    call; release followed by a new call gives the same bits; a 0.25 MB scratch budget gives more launches and the same bits;
    Zx and Gx are stale separately"""
    case = R.CASES["box9r2_nd"]()
    n = case["n"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    fv = _host_factor(S, Lf)
    plan, lib, xsize = Lf.contents.hip_plan, S.L, fv.xsize
    Lbar_x, _ = F.random_lbar(fv, 51, dead=1e30)
    Lb = _dev(Lbar_x)
    g1, g2, g3 = np.zeros(xsize), np.zeros(xsize), np.zeros(xsize)
    tr = torch.zeros((), dtype=torch.float64, device="cuda")
    assert _info(S, Lf)[6] == 0
    assert lib.cholmod_hip_factor_grad_download(plan, g1.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_factor_grad_gather_device(plan, None, 0, tr.data_ptr(), None) == ch.HIP_INVALID
    # a selected inverse does not make Gx current
    assert lib.cholmod_hip_selinv_device(plan, None) == ch.HIP_OK and _info(S, Lf, "selinv")[6] == 1 and _info(S, Lf)[6] == 0
    assert lib.cholmod_hip_factor_grad_download(plan, g1.ctypes.data) == ch.HIP_INVALID
    # two calls: the same bits
    assert lib.cholmod_hip_factor_grad_device(plan, Lb.data_ptr(), None) == ch.HIP_OK and _info(S, Lf)[6] == 1
    assert lib.cholmod_hip_factor_grad_download(plan, g1.ctypes.data) == ch.HIP_OK
    assert lib.cholmod_hip_factor_grad_device(plan, Lb.data_ptr(), None) == ch.HIP_OK
    assert lib.cholmod_hip_factor_grad_download(plan, g2.ctypes.data) == ch.HIP_OK
    assert np.array_equal(_bits(g1), _bits(g2))
    # release, then a call: the same bits again; the selected inverse keeps its array and the scratch
    assert lib.cholmod_hip_factor_grad_release(plan) == ch.HIP_OK and _info(S, Lf)[6] == 0 and _info(S, Lf)[4] == 0
    assert _info(S, Lf, "selinv")[6] == 1 and _info(S, Lf, "selinv")[4] > 0
    assert lib.cholmod_hip_factor_grad_download(plan, g3.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_factor_grad_device(plan, Lb.data_ptr(), None) == ch.HIP_OK
    assert lib.cholmod_hip_factor_grad_download(plan, g3.ctypes.data) == ch.HIP_OK
    assert np.array_equal(_bits(g1), _bits(g3))
    # new values from the device: stale, refused, then the gradient through the new factor
    scale = 1.0 + 0.5 * np.random.default_rng(52).uniform(size=n)
    cols = np.repeat(np.arange(n), np.diff(case["Lp"]))
    Lx2 = case["Lx"] * scale[case["Li"]] * scale[cols]
    assert S.factorize_device(A, _dev(Lx2), Lf) == 1 and S.cm.status == ch.OK
    assert _info(S, Lf)[6] == 0
    assert lib.cholmod_hip_factor_grad_download(plan, g3.ctypes.data) == ch.HIP_INVALID
    assert lib.cholmod_hip_factor_grad_gather_device(plan, None, 0, tr.data_ptr(), None) == ch.HIP_INVALID
    S.factor_grad_device(A, Lf, Lb)
    Gx = S.factor_grad_host(Lf)
    assert _info(S, Lf)[6] == 1
    fv = _host_factor(S, Lf)
    ref, mask = _dense_reference(dict(case, Lx=Lx2), fv, 0.0, F.dense_of_layout(fv, Lbar_x))
    err, dead = _compare(Gx, ref, mask)
    tol = R.tolerance(R.factor_rcond(fv))
    print(f"stale: after factorize_device err={err:.2e} tol={tol:.2e}")
    assert err <= tol and dead == 0 and not np.array_equal(Gx, g1)
    _done(S, A, Lf)
    # a small scratch budget cuts the batches into chunks: more launches, the same bits
    case = R.CASES["p3d_12_nd"]()
    got = []
    for mb in (None, "0.25"):
        if mb:
            os.environ["CHOLMOD_HIP_SELINV_BUDGET_MB"] = mb
        S, A, Lf = R.factorized(case, use_gpu=1)
        fv = _host_factor(S, Lf)
        S.factor_grad_device(A, Lf, _dev(F.random_lbar(fv, 53)[0]))
        got.append((S.factor_grad_host(Lf), _info(S, Lf)[1], _info(S, Lf)[5]))
        _done(S, A, Lf)
    del os.environ["CHOLMOD_HIP_SELINV_BUDGET_MB"]
    print(f"stale: launches {int(got[0][1])} (scratch {int(got[0][2])} B), with a 0.25 MB budget {int(got[1][1])} ({int(got[1][2])} B)")
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0]))
    assert got[1][1] > got[0][1] and got[1][2] < got[0][2]


def case_stream():
    """a forward and a backward on a side stream behind the torch ops that produce the values, the gradients consumed on
    that stream without a host wait; then three engine-level calls of each entry point leave the free memory of the device
    where it was; the launch count within the selected inverse's bound"""
    case = R.CASES["p2d_60_nd"]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    perm = _host_factor(S, Lf).Perm.copy()
    chol = DeviceCholesky(S, A, Lf)
    rng = np.random.default_rng(61)
    Z, B, W, W2 = (rng.standard_normal((3, n)) for _ in range(4))
    half, Zh, Bh, Wd, W2d = _dev(0.5 * Ax), _dev(Z), _dev(B), _dev(W), _dev(W2)
    s = torch.cuda.Stream()
    for rep in range(3):                # (rep 0 on the default stream: the workspaces exist from there on)
        scale = 1.0 + 0.5 * (rep % 2)
        st = s if rep else torch.cuda.default_stream()
        with torch.cuda.stream(st):
            v = half
            for _ in range(20):
                v = v * 1.0 + 0.0
            v = (v + half * (2.0 * scale - 1.0)).requires_grad_()
            Zd, Bd = (Zh * 1.0).requires_grad_(), (Bh * 1.0).requires_grad_()
            X, Y = chol.solve_Lt(v, Zd), chol.solve_L(v, Bd)
            ((Wd * X).sum() + (W2d * Y).sum()).backward()
            out = dict(X=X.detach() * 2.0, Y=Y.detach() * 2.0, gv=v.grad * 2.0, gZ=Zd.grad * 2.0, gB=Bd.grad * 2.0)
        st.synchronize()
        ref = _torch_reference(n, Ap, Ai, Ax * scale, perm, 0.0, Z, B, W, W2)
        tol = R.tolerance(R.factor_rcond(_host_factor(S, Lf)))
        ref["gbeta"] = 0.0
        _check_autograd(f"stream rep {rep}", dict({k: 0.5 * t.cpu().numpy() for k, t in out.items()}, gbeta=0.0), ref, tol)
    info, bound = _info(S, Lf), _launch_bound(S, Lf)
    print(f"stream: launches {int(info[1])}, the selected inverse's bound {bound}, {1e3 * info[0]:.3f} ms")
    assert 0 < info[1] <= bound, (info[1], bound)
    # the engine's own calls, no torch allocation in between: the free memory of the device does not move
    plan = Lf.contents.hip_plan
    Lb = torch.zeros(int(Lf.contents.xsize), dtype=torch.float64, device="cuda")
    Gv = torch.zeros(len(Ai), dtype=torch.float64, device="cuda")
    tr = torch.zeros((), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        assert S.L.cholmod_hip_factor_grad_device(plan, Lb.data_ptr(), s.cuda_stream) == ch.HIP_OK
        assert S.L.cholmod_hip_factor_outer_grad_device(plan, -1.0, Zh.data_ptr(), n, Bh.data_ptr(), n, 3, s.cuda_stream) == ch.HIP_OK
        assert S.L.cholmod_hip_factor_grad_gather_device(plan, Gv.data_ptr(), Gv.numel(), tr.data_ptr(), s.cuda_stream) == ch.HIP_OK
    s.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    _done(S, A, Lf)


def case_refusals():
    """a complex factor: CHOLMOD_NOT_INSTALLED; a factorization that was not positive definite (2lo.tri): CHOLMOD_INVALID, L
    as it was"""
    n, Ap, Ai, Ax = G.poisson3d(6)
    Hx = G.hermitian_phases(n, Ap, Ai, Ax, seed=5)
    S = ch.Session()
    S.cm.error_handler = ch.ERRFUNC(0)
    A = S.sparse(n, Ap, Ai, Hx, -1)
    Lf = S.analyze(A)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    out = np.zeros(2 * int(Lf.contents.xsize) + 1)
    buf = torch.zeros(2 * int(Lf.contents.xsize) + n + 1, dtype=torch.float64, device="cuda")
    cm = C.byref(S.cm)
    assert S.L.cholmod_l_hip_factor_grad_to_host(Lf, out.ctypes.data, cm) == 0 and S.cm.status == ch.NOT_INSTALLED
    assert S.L.cholmod_l_hip_factor_grad_device(None, Lf, buf.data_ptr(), None, buf.data_ptr(), None, cm) == 0
    assert S.cm.status == ch.NOT_INSTALLED
    assert S.L.cholmod_l_hip_factor_outer_grad_device(None, Lf, -1.0, buf.data_ptr(), n, buf.data_ptr(), n, 1, None,
                                                      buf.data_ptr(), None, cm) == 0
    assert S.cm.status == ch.NOT_INSTALLED and np.all(out == 0)
    _done(S, A, Lf)
    from test_tcov_matrices import _load, _library_matrix
    case = _load("tcov", "2lo.tri")
    S = ch.Session()
    S.cm.error_handler = ch.ERRFUNC(0)
    A = _library_matrix(S, case)
    Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
    assert Lf and S.cm.status == ch.OK
    S.L.cholmod_l_factorize(A, Lf, C.byref(S.cm))
    assert S.cm.status == ch.NOT_POSDEF and Lf.contents.minor < Lf.contents.n
    fv = _host_factor(S, Lf)
    x0, minor0 = None if fv.x is None else fv.x.copy(), fv.minor
    out = np.zeros(max(int(Lf.contents.xsize), 1))
    buf = torch.zeros(max(int(Lf.contents.xsize), 1) + case["n"], dtype=torch.float64, device="cuda")
    cm = C.byref(S.cm)
    assert S.L.cholmod_l_hip_factor_grad_to_host(Lf, out.ctypes.data, cm) == 0 and S.cm.status == ch.INVALID
    assert S.L.cholmod_l_hip_factor_grad_device(A, Lf, buf.data_ptr(), None, buf.data_ptr(), None, cm) == 0 and S.cm.status == ch.INVALID
    assert S.L.cholmod_l_hip_factor_outer_grad_device(A, Lf, -1.0, buf.data_ptr(), case["n"], buf.data_ptr(), case["n"], 1, None,
                                                      buf.data_ptr(), None, cm) == 0 and S.cm.status == ch.INVALID
    plan = Lf.contents.hip_plan
    if plan:
        assert S.L.cholmod_hip_factor_grad_device(plan, buf.data_ptr(), None) == ch.HIP_INVALID
    fv = ch.FactorView(Lf)
    assert fv.minor == minor0 and (x0 is None or np.array_equal(fv.x, x0)) and np.all(out == 0)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
