"""The bodies of tests/test_gpu_grad.py, run in a process of their own: `python grad_cases.py CASE [ARG ...]`, torch
imported FIRST (see solve_device_cases.py).  Exit status 0 = every assertion held.  Matrices and the parity bar
max (1e-12, 20 eps / rcond) come from tests/selinv_reference.py, the formulas and the dense torch reference from
tests/grad_reference.py; every figure is printed before it is asserted."""
import torch  # noqa: E402  (first)

import ctypes as C
import math
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import grad_reference as GR
import selinv_reference as R
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G
from suitesparse_amd.autograd import DeviceCholesky

BETA = 0.375
EPS = GR.EPS
NAN = float("nan")


def _done(S, A, Lf):
    torch.cuda.synchronize()
    S.free_factor(Lf)
    if A:
        S.free_sparse(A)
    S.finish()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _count(S, Lf):
    out = np.zeros(12, dtype=np.int64)
    assert S.L.cholmod_hip_progress(Lf.contents.hip_plan, out.ctypes.data) == ch.HIP_OK
    return int(out[0])


def _ld(t):
    return int(t.stride(0)) if t.dim() == 2 and t.shape[0] > 1 else int(t.shape[-1])


def _engine(S, Lf, perm, alpha, U, V, nnz, stream=None, out=None):
    """cholmod_hip_values_grad_device on (nrhs, n) tensors; dG pre-filled with NaN -> (status, G)"""
    Gd = torch.full((nnz,), NAN, dtype=torch.float64, device="cuda") if out is None else out
    rc = S.L.cholmod_hip_values_grad_device(Lf.contents.hip_plan, perm, alpha, U.data_ptr() or 1, _ld(U), V.data_ptr() or 1, _ld(V),
                                            U.shape[0], Gd.data_ptr(), nnz, stream)
    return rc, Gd


def _ints(rng, nrhs, n):
    return rng.integers(-8, 9, size=(nrhs, n)).astype(np.float64)


def case_exact(name):
    """small integers and alpha = -1: every product and every sum is exact in any order, so G equals the numpy reference
    exactly at every entry (equal doubles other than zero are equal bit for bit; the sign of a zero SUM depends on the
    order and is not compared).  Both sides of SD_BLOCK_MIN_NRHS, a partial last panel, three panels; the host layer
    (perm = 1) and the engine with perm = 1 and 0; once with ld > n and once with U and V the same array; dG pre-filled
    with NaN, which equals nothing"""
    case = R.CASES[name]()
    n, Ap, Ai = case["n"], case["Lp"], case["Li"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    P = ch.FactorView(Lf).Perm.copy()
    if name == "p3d_9_random_nopost":
        assert not np.array_equal(P, np.arange(n))
    rng = np.random.default_rng(11)
    for nrhs in (1, 3, 7, 8, 16, 19, 33):
        U, V = _ints(rng, nrhs, n), _ints(rng, nrhs, n)
        ref = GR.values_grad(Ap, Ai, -1, U, V, -1.0)
        Ud, Vd = _dev(U), _dev(V)
        out = torch.full((len(Ai),), NAN, dtype=torch.float64, device="cuda")
        g_host = S.values_grad_device(A, Lf, Ud, Vd, alpha=-1.0, out=out)
        rc1, g1 = _engine(S, Lf, 1, -1.0, Ud, Vd, len(Ai))
        rc0, g0 = _engine(S, Lf, 0, -1.0, _dev(U[:, P]), _dev(V[:, P]), len(Ai))
        # ld > n: the rows of a wider tensor
        wide = torch.full((2 * nrhs, n + 5), NAN, dtype=torch.float64, device="cuda")
        wide[:nrhs, :n], wide[nrhs:, :n] = Ud, Vd
        g_ld = S.values_grad_device(A, Lf, wide[:nrhs, :n], wide[nrhs:, :n], alpha=-1.0)
        # U and V one array
        rcs, g_same = _engine(S, Lf, 1, -1.0, Ud, Ud, len(Ai))
        torch.cuda.synchronize()
        assert rc1 == rc0 == rcs == ch.HIP_OK
        bad = {k: int((g.cpu().numpy() != ref).sum()) for k, g in (("host", g_host), ("perm1", g1), ("perm0", g0), ("ld", g_ld))}
        bad["same"] = int((g_same.cpu().numpy() != GR.values_grad(Ap, Ai, -1, U, U, -1.0)).sum())
        print(f"exact {name} nrhs={nrhs}: nnz={len(Ai)} entries that differ {bad}")
        assert not any(bad.values()), (name, nrhs, bad)
    # nrhs == 0: a success that zero-fills
    rc, g = _engine(S, Lf, 1, -1.0, torch.zeros((0, n), dtype=torch.float64, device="cuda"),
                    torch.zeros((0, n), dtype=torch.float64, device="cuda"), len(Ai))
    torch.cuda.synchronize()
    assert rc == ch.HIP_OK and np.array_equal(g.cpu().numpy().view(np.int64), np.zeros(len(Ai), dtype=np.int64))
    _done(S, A, Lf)


def case_rounded():
    """standard-normal U and V scaled per row by 2^+-20: per entry within 2 (2 nrhs + 2) eps |alpha| sum_r (|U_i V_j| + |U_j V_i|)
    of numpy -- a sum of 2 nrhs products in any order, with or without FMA, is within gamma_(2 nrhs) of exact, alpha adds
    one rounding, the numpy reference carries the same error --; two calls give the same bits"""
    alpha = -0.7
    for name in ("p3d_12_nd", "arrow300"):
        case = R.CASES[name]()
        n, Ap, Ai = case["n"], case["Lp"], case["Li"]
        S, A, Lf = R.factorized(case, use_gpu=1)
        rng = np.random.default_rng(12)
        for nrhs in (3, 8, 19, 33):
            U = rng.standard_normal((nrhs, n)) * np.exp2(rng.integers(-20, 21, size=n))
            V = rng.standard_normal((nrhs, n)) * np.exp2(rng.integers(-20, 21, size=n))
            ref = GR.values_grad(Ap, Ai, -1, U, V, alpha)
            bar = 2 * (2 * nrhs + 2) * EPS * abs(alpha) * GR.values_grad_magnitude(Ap, Ai, U, V)
            Ud, Vd = _dev(U), _dev(V)
            g1 = S.values_grad_device(A, Lf, Ud, Vd, alpha=alpha)
            g2 = S.values_grad_device(A, Lf, Ud, Vd, alpha=alpha)
            torch.cuda.synchronize()
            g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
            with np.errstate(invalid="ignore", divide="ignore"):
                w = float(np.nanmax(np.where(bar > 0, np.abs(g1 - ref) / bar, np.where(g1 == ref, 0.0, np.inf))))
            print(f"rounded {name} nrhs={nrhs}: worst |G - ref| / bar = {w:.3e}")
            assert np.all(np.isfinite(g1)) and w <= 1.0, (name, nrhs, w)
            assert np.array_equal(g1.view(np.int64), g2.view(np.int64)), (name, nrhs)
        _done(S, A, Lf)


def case_unread():
    """upper-stored input, and both triangles stored with 1e30 in the ignored one: G is exact +0.0 exactly where
    selinv_device gives NaN and the reference elsewhere"""
    case = R.CASES["p3d_12_nd"]()
    n = case["n"]
    Lo = sp.csc_matrix((case["Lx"], case["Li"], case["Lp"]), shape=(n, n))
    Up = sp.csc_matrix(Lo.T)
    junk = sp.csc_matrix(Lo + sp.triu(Up, 1) * 1e30)
    rng = np.random.default_rng(13)
    for tag, M, stype in (("upper", Up, 1), ("junk", junk, -1)):
        M.sort_indices()
        Ap, Ai, Ax = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)
        S = ch.Session()
        A = S.sparse(n, Ap, Ai, Ax, stype)
        Lf = S.analyze(A, case["perm"])
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        Z, _ = S.selinv_device(A, Lf, diag=False)
        for nrhs in (3, 19):
            U, V = _ints(rng, nrhs, n), _ints(rng, nrhs, n)
            out = torch.full((len(Ai),), NAN, dtype=torch.float64, device="cuda")
            g = S.values_grad_device(A, Lf, _dev(U), _dev(V), alpha=-1.0, out=out)
            torch.cuda.synchronize()
            g, nan = g.cpu().numpy(), np.isnan(Z.cpu().numpy())
            ref = GR.values_grad(Ap, Ai, stype, U, V, -1.0)
            read = GR.read_mask(Ap, Ai, stype)
            print(f"unread {tag} nrhs={nrhs}: {int(nan.sum())} NaN of selinv, {int((~read).sum())} entries not read, "
                  f"{int((g != ref).sum())} entries differ")
            assert nan.any() == (tag == "junk") and np.array_equal(nan, ~read)      # (upper-stored: every entry is read)
            assert np.array_equal(g[nan].view(np.int64), np.zeros(int(nan.sum()), dtype=np.int64))       # +0.0, bit for bit
            assert np.array_equal(g, ref)
        _done(S, A, Lf)


def _check_grads(tag, gv, gb, ref, tol, nrhs):
    bar_v, bar_b = GR.bars(ref, tol, nrhs)
    ev = float(np.abs(gv.cpu().numpy() - ref["grad_values"]).max())
    eb = float(np.abs(gb.cpu().numpy() - ref["grad_B"]).max())
    print(f"{tag}: grad_values {ev:.2e} (bar {bar_v:.2e}), grad_B {eb:.2e} (bar {bar_b:.2e})")
    assert ev <= bar_v and eb <= bar_b, (tag, ev, bar_v, eb, bar_b)


def case_autograd(name):
    """loss = (W . chol.solve (v, B)).sum () + 0.3 chol.logdet (v) against the same loss from a dense symmetric matrix with
    torch.linalg.solve / torch.logdet in float64 on the CPU, beta 0 and 0.375, nrhs 1 and 19; with
    tol = max (1e-12, 20 eps / rcond):  |grad_values - ref| <= tol (4 nrhs max |Lambda| max |X| + 0.6 max |Z|),
    |grad_B - ref| <= tol max |Lambda|,  |X - ref| <= tol max |X|,  |logdet - ref| <= 1e-11 sum |2 log L_jj|; one
    factorization for logdet + solve on one `values`; a second backward after an intervening factorize_device with other
    values still gives the first matrix's gradient"""
    case = R.CASES[name]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    for beta in (0.0, BETA):
        S, A, Lf = R.factorized(case, use_gpu=1, beta=beta)
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
        chol = DeviceCholesky(S, A, Lf, beta)
        other = _dev(Ax * np.where(Ai == GR.columns_of(Ap), 2.0, 0.5))
        for nrhs in (1, 19):
            tag = f"autograd {name} beta={beta} nrhs={nrhs}"
            B, W = GR.inputs(n, nrhs, 7)
            ref = GR.torch_reference(n, Ap, Ai, Ax, -1, beta, B, W)
            v, Bd, Wd = _dev(Ax).requires_grad_(), _dev(B).requires_grad_(), _dev(W)
            c0, f0 = _count(S, Lf), chol.factorizations
            ld = chol.logdet(v)
            X = chol.solve(v, Bd)
            assert _count(S, Lf) - c0 == 1 and chol.factorizations - f0 == 1, tag
            loss = (Wd * X).sum() + 0.3 * ld
            loss.backward(retain_graph=True)
            ex = float(np.abs(X.detach().cpu().numpy() - ref["X"]).max())
            el = abs(float(ld) - ref["logdet"])
            print(f"{tag}: tol {tol:.2e}, X {ex:.2e} (bar {tol * ref['x_max']:.2e}), logdet {el:.2e} "
                  f"(bar {1e-11 * ref['logdet_scale']:.2e})")
            assert ex <= tol * ref["x_max"] and el <= 1e-11 * ref["logdet_scale"], tag
            assert X.shape == Bd.shape and ld.dim() == 0 and v.grad.shape == v.shape and Bd.grad.shape == Bd.shape
            _check_grads(tag, v.grad, Bd.grad, ref, tol, nrhs)
            # the factor is replaced behind the wrapper's back: the second backward refactorizes from the saved values
            v.grad = Bd.grad = None
            assert S.factorize_device(A, other, Lf, beta) == 1 and S.cm.status == ch.OK
            c1 = _count(S, Lf)
            loss.backward()
            assert _count(S, Lf) - c1 == 1, tag
            _check_grads(tag + " (stale factor)", v.grad, Bd.grad, ref, tol, nrhs)
        _done(S, A, Lf)


def case_not_posdef():
    """a factorization that is not positive definite raises RuntimeError in the forward"""
    case = R.CASES["forest148"]()
    S, A, Lf = R.factorized(case, use_gpu=1)
    S.cm.error_handler = ch.ERRFUNC(0)
    chol = DeviceCholesky(S, A, Lf)
    v = _dev(-case["Lx"]).requires_grad_()
    for f in (lambda: chol.logdet(v), lambda: chol.solve(v, torch.ones(case["n"], dtype=torch.float64, device="cuda"))):
        try:
            f()
        except RuntimeError as e:
            print("not_posdef:", e)
        else:
            raise AssertionError("no RuntimeError")
    # ... and the wrapper recovers with good values
    ld = chol.logdet(_dev(case["Lx"]))
    assert np.isfinite(float(ld))
    _done(S, A, Lf)


def _diag_of(fv):
    d = []
    for k in range(fv.nsuper):
        nsrow, nscol = int(fv.pi[k + 1] - fv.pi[k]), int(fv.super[k + 1] - fv.super[k])
        d.append(fv.x[int(fv.px[k]) + (nsrow + 1) * np.arange(nscol)])
    return np.concatenate(d)


def case_logdet():
    """against 2 fsum (log d) of the downloaded diagonal within (n + 2) eps sum |2 log L_jj| (any summation order holds it,
    a dropped entry misses it by orders of magnitude); bit-identical across two calls and across a refactorization of the
    same values; Poisson 24^3 against the closed form at 1e-11; refused after 2lo.tri, L left as it was"""
    for name in ("arrow300", "forest148", "p3d_9_random_nopost", "p3d_12_nd"):
        case = R.CASES[name]()
        n = case["n"]
        S, A, Lf = R.factorized(case, use_gpu=1, beta=BETA)
        l1, l2 = S.logdet_device(Lf), S.logdet_device(Lf)
        assert S.factorize_device(A, _dev(case["Lx"]), Lf, BETA) == 1 and S.cm.status == ch.OK
        l3 = S.logdet_device(Lf)
        assert S.factorize_device(A, _dev(case["Lx"]), Lf, BETA) == 1 and S.cm.status == ch.OK
        l4 = S.logdet_device(Lf)
        torch.cuda.synchronize()
        assert l1.dim() == 0 and l1.dtype == torch.float64 and l1.is_cuda
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        logs = 2.0 * np.log(_diag_of(ch.FactorView(Lf)))
        ref, bar = math.fsum(logs), (n + 2) * EPS * float(np.abs(logs).sum())
        got = [float(x) for x in (l1, l2, l3, l4)]
        print(f"logdet {name}: {got[3]!r} against fsum {ref!r}: {abs(got[3] - ref):.2e} (bar {bar:.2e}); "
              f"after host factorize / two calls / factorize_device twice: {got}")
        assert abs(got[3] - ref) <= bar, name
        assert got[0] == got[1] and got[2] == got[3], name
        _done(S, A, Lf)
    m = 24
    n, Ap, Ai, Ax = G.poisson3d(m)
    S = ch.Session()
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, G.geometric_nd(m, m, m, 4))
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    got, ref = float(S.logdet_device(Lf)), G.poisson_logdet(m, m, m)
    half = S.factor_checks(Lf)["half_logdet"]
    print(f"logdet poisson {m}^3: {got!r} closed form {ref!r} rel {abs(got - ref) / abs(ref):.2e}; factor_checks {2 * half!r}")
    assert abs(got - ref) <= 1e-11 * abs(ref)
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
    out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    assert S.L.cholmod_l_hip_logdet_device(Lf, out.data_ptr(), None, C.byref(S.cm)) == 0 and S.cm.status == ch.INVALID
    if Lf.contents.hip_plan:
        assert S.L.cholmod_hip_logdet_device(Lf.contents.hip_plan, out.data_ptr(), None) == ch.HIP_INVALID
    torch.cuda.synchronize()
    fv = ch.FactorView(Lf)
    assert fv.minor == minor0 and (x0 is None or np.array_equal(fv.x, x0)) and float(out[0]) == 7.0
    _done(S, A, Lf)


def case_stream():
    """a forward and a backward on a side stream behind the torch ops that produce the values, the gradient consumed on
    that stream without a host wait; then three engine-level calls of each new entry point allocate nothing"""
    name = "p3d_9_random_nopost"
    case = R.CASES[name]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    chol = DeviceCholesky(S, A, Lf)
    nrhs = 19
    B, W = GR.inputs(n, nrhs, 9)
    half, Bh, Wd = _dev(0.5 * Ax), _dev(B), _dev(W)
    s = torch.cuda.Stream()
    for rep in range(3):                # (rep 0 on the default stream: the workspaces exist from there on)
        scale = 1.0 + 0.5 * (rep % 2)
        with torch.cuda.stream(s if rep else torch.cuda.default_stream()):
            v = half
            for _ in range(20):
                v = v * 1.0 + 0.0
            v = (v + half * (2.0 * scale - 1.0)).requires_grad_()
            Bd = (Bh * 1.0).requires_grad_()
            loss = (Wd * chol.solve(v, Bd)).sum() + 0.3 * chol.logdet(v)
            loss.backward()
            Y, Yb = v.grad * 2.0, Bd.grad * 2.0
        (s if rep else torch.cuda.default_stream()).synchronize()
        ref = GR.torch_reference(n, Ap, Ai, Ax * scale, -1, 0.0, B, W)
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
        _check_grads(f"stream rep {rep}", Y * 0.5, Yb * 0.5, ref, tol, nrhs)
    # the engine's own calls, no torch allocation in between: the free memory of the device does not move
    U3, V3 = _dev(B[:3]), _dev(W[:3])
    out, ld = torch.empty(len(Ai), dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    plan = Lf.contents.hip_plan
    assert _engine(S, Lf, 1, -1.0, U3, V3, len(Ai), s.cuda_stream, out)[0] == ch.HIP_OK      # (fewer than 8: its first call)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        assert _engine(S, Lf, 1, -1.0, U3, V3, len(Ai), s.cuda_stream, out)[0] == ch.HIP_OK
        assert _engine(S, Lf, 1, -1.0, Bh, Wd, len(Ai), s.cuda_stream, out)[0] == ch.HIP_OK
        assert S.L.cholmod_hip_logdet_device(plan, ld.data_ptr(), s.cuda_stream) == ch.HIP_OK
    s.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert np.array_equal(out.cpu().numpy(), S.values_grad_device(A, Lf, Bh, Wd, alpha=-1.0).cpu().numpy())
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
    U = torch.ones((3, n), dtype=torch.float64, device="cuda")
    g = torch.full((len(Ai),), 7.0, dtype=torch.float64, device="cuda")
    assert S.L.cholmod_l_hip_values_grad_device(A, Lf, -1.0, U.data_ptr(), n, U.data_ptr(), n, 3, g.data_ptr(), None,
                                                C.byref(S.cm)) == 0 and S.cm.status == ch.NOT_INSTALLED
    assert S.L.cholmod_l_hip_logdet_device(Lf, g.data_ptr(), None, C.byref(S.cm)) == 0 and S.cm.status == ch.NOT_INSTALLED
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())
    _done(S, A, Lf)
    # a wrong nvalues, a product map set: refused by the engine, dG untouched; without the map the call works again
    case = R.CASES["p3d_12_nd"]()
    n, Ap, Ai = case["n"], case["Lp"], case["Li"]
    nnz = len(Ai)
    S, A, Lf = R.factorized(case, use_gpu=1)
    plan = Lf.contents.hip_plan
    rng = np.random.default_rng(14)
    U, V = _ints(rng, 3, n), _ints(rng, 3, n)
    Ud, Vd = _dev(U), _dev(V)
    g = torch.full((nnz + 1,), 7.0, dtype=torch.float64, device="cuda")
    for nv in (nnz + 1, nnz - 1):
        assert _engine(S, Lf, 0, -1.0, Ud, Vd, nv, None, g)[0] == ch.HIP_INVALID
    for ld in (n - 1,):
        assert S.L.cholmod_hip_values_grad_device(plan, 0, -1.0, Ud.data_ptr(), ld, Vd.data_ptr(), n, 3, g.data_ptr(), nnz, None) == ch.HIP_INVALID
    assert S.L.cholmod_hip_values_grad_device(plan, 0, -1.0, Ud.data_ptr(), n, Vd.data_ptr(), n, -1, g.data_ptr(), nnz, None) == ch.HIP_INVALID
    cp, ia = np.arange(nnz + 1, dtype=np.int64), np.arange(nnz, dtype=np.int64)
    assert S.L.cholmod_hip_set_product_map(plan, cp.ctypes.data, ia.ctypes.data, ia.ctypes.data, nnz, nnz) == ch.HIP_OK
    assert _engine(S, Lf, 0, -1.0, Ud, Vd, nnz, None, g)[0] == ch.HIP_INVALID
    assert S.L.cholmod_hip_set_product_map(plan, None, None, None, 0, 0) == ch.HIP_OK
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())
    got = S.values_grad_device(A, Lf, Ud, Vd, alpha=-1.0).cpu().numpy()
    assert np.array_equal(got, GR.values_grad(Ap, Ai, -1, U, V, -1.0))
    # a matrix of another pattern: refused by the host layer, dG untouched
    S.cm.error_handler = ch.ERRFUNC(0)
    A2 = S.sparse(n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), np.ones(n), -1)
    g2 = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    try:
        S.values_grad_device(A2, Lf, Ud, Vd, out=g2)
    except RuntimeError as e:
        print("refusals:", e)
    else:
        raise AssertionError("no RuntimeError")
    torch.cuda.synchronize()
    assert S.cm.status == ch.INVALID and bool((g2 == 7.0).all())
    S.free_sparse(A2)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
