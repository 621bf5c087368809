"""The bodies of tests/test_gpu_schur.py, run in a process of their own: `python schur_cases.py CASE [ARG ...]`, torch
imported FIRST (see solve_device_cases.py).  Exit status 0 = every assertion held; a line `RESULT <json>` carries figures
back.  Matrices, the dense references, the list of m and the bar -- error <= max (1e-12, 20 eps / rcond) max |ref|,
rcond = (min L_jj / max L_jj)^2 -- come from tests/schur_reference.py."""
import torch  # noqa: E402  (first)

import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import schur_reference as R
from suitesparse_amd import cholmod as ch
from suitesparse_amd import generators as G

POISON = -7.25e300


def _done(S, A, Lf):
    torch.cuda.synchronize()
    S.free_factor(Lf)
    if A:
        S.free_sparse(A)
    S.finish()


def _host_factor(S, Lf):
    """FactorView of the factor the device holds (downloaded), its restated maps as a tuple, the bar"""
    S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    fv = ch.FactorView(Lf)
    return fv, (fv.super, fv.pi, fv.px, fv.s, fv.x), R.tolerance(R.factor_rcond(fv))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _padded(m):
    """an over-allocated, poisoned (m + 2) x (m + 3) buffer and its (m, m) corner (leading dimension m + 3)"""
    buf = torch.full((m + 2, m + 3), POISON, dtype=torch.float64, device="cuda")
    return buf, buf[:m, :m]


def _untouched(buf, m):
    b = buf.cpu().numpy()
    return bool(np.all(b[:m, m:] == POISON) and np.all(b[m:, :] == POISON))


def case_entries():
    """every matrix of the table with beta = 0 and 0.375, two once more through the generic kernels only, every m of the
    list: Sc against the dense Schur complement, bitwise symmetric, nothing written outside the m x m arrays; for m = n
    against the dense P (A + beta I) P' itself; F bit for bit the entries of the downloaded factor, exact +0.0 elsewhere;
    F F' against Sc"""
    out = {}
    runs = [(name, beta, 0) for name in sorted(R.CASES) for beta in R.BETAS]
    runs += [(name, 0.0, ch.HIP_NO_SMALL_FRONTS) for name in ("p3d_12_nd", "box9r2_nd")]
    for name, beta, flags in runs:
        case = R.CASES[name]()
        n = case["n"]
        S, A, Lf = R.factorized(case, use_gpu=1, beta=beta, hip_flags=flags)
        fv, fac, tol = _host_factor(S, Lf)
        M = R.permuted_dense(case, fv.Perm, beta)
        ms = R.m_list(fv)
        assert R.m_inside(fv) in ms and R.m_first_column(fv) in ms
        res = dict(err=0.0, sym=True, untouched=True, fbits=True, fft=0.0, mn=None, ms=ms, tol=tol)
        for m in ms:
            sbuf, sview = _padded(m)
            fbuf, fview = _padded(m)
            Sc, F = S.schur_device(Lf, m, factor=True, out=(sview, fview))
            torch.cuda.synchronize()
            assert tuple(Sc.shape) == (m, m) and tuple(F.shape) == (m, m)
            res["untouched"] &= _untouched(sbuf, m) and _untouched(fbuf, m)
            if m == 0:
                continue
            Sc, F = Sc.cpu().numpy(), F.cpu().numpy()
            res["sym"] &= bool(np.array_equal(_bits(Sc), _bits(Sc.T)))
            # (bitwise: the lower triangle is the factor's entries, everything else +0.0, whose bits are zero)
            res["fbits"] &= bool(np.array_equal(_bits(F), _bits(R.trailing_factor(*fac, n, m))))
            ref = R.dense_schur(M, m)
            scale = np.abs(ref).max()
            with np.errstate(invalid="ignore"):
                e1, e2 = np.abs(Sc - ref).max() / scale, np.abs(F @ F.T - Sc).max() / np.abs(Sc).max()
            e1, e2 = (float(e) if np.isfinite(e) else 1e300 for e in (e1, e2))
            res["err"], res["fft"] = max(res["err"], e1 / tol), max(res["fft"], e2 / tol)
            if m == n:
                e3 = np.abs(Sc - M).max() / np.abs(M).max()
                res["mn"] = float(e3 / tol) if np.isfinite(e3) else 1e300
        key = f"{name}|{beta}|{flags}"
        print(f"{key}: n={n} nsuper={fv.nsuper} tol={tol:.2e} m in {ms}: err/tol={res['err']:.3f} F F'/tol={res['fft']:.3f} "
              f"m=n/tol={res['mn']:.3f} sym={res['sym']} untouched={res['untouched']} fbits={res['fbits']}")
        out[key] = res
        _done(S, A, Lf)
    print("RESULT " + json.dumps(out))


def case_nesting():
    """the Schur complement of Sc (m2) onto its last m1 variables is Sc (m1): forest148 (the trailing supernodes are roots
    of different trees: L22 is block-sparse), arrow300 and dense200 with m2 = 137 inside a supernode wider than 64 columns"""
    for name, m2, m1 in (("forest148", 110, 37), ("arrow300", 137, 50), ("dense200", 137, 50), ("arrow300", 137, 70)):
        case = R.CASES[name]()
        S, A, Lf = R.factorized(case, use_gpu=1)
        fv, fac, tol = _host_factor(S, Lf)
        t2 = case["n"] - m2
        if name != "forest148":
            # a supernode with more than 64 contributing columns (dense200: the boundary lies inside it)
            assert max(int(fv.super[k + 1]) - max(int(fv.super[k]), t2) for k in range(fv.nsuper)) > 64, name
        else:
            F = R.trailing_factor(*fac, case["n"], m2)
            assert np.count_nonzero(np.tril(F)) < m2 * (m2 + 1) // 4            # block-sparse indeed
        S2, S1 = S.schur_device(Lf, m2).cpu().numpy(), S.schur_device(Lf, m1).cpu().numpy()
        ref = R.dense_schur(S2, m1)
        err = np.abs(S1 - ref).max() / np.abs(ref).max()
        print(f"nesting {name}: m2={m2} m1={m1} err={err:.2e} tol={tol:.2e}")
        assert err <= tol, (name, err, tol)
        _done(S, A, Lf)


def _multiply(S, Lf, m, trans, V):
    """the engine's trailing multiply on V (nrhs, m) -> (nrhs, m)"""
    out = torch.full(V.shape, POISON, dtype=torch.float64, device="cuda")
    rc = S.L.cholmod_hip_trailing_multiply_device(Lf.contents.hip_plan, m, trans, V.data_ptr(), m, out.data_ptr(), m,
                                                  V.shape[0], torch.cuda.current_stream().cuda_stream)
    assert rc == ch.HIP_OK
    return out


def case_samebits():
    case = R.CASES["box9r2_nd"]()
    n = case["n"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    fv, fac, tol = _host_factor(S, Lf)
    for m in (65, R.m_inside(fv), n // 2):
        a, fa = S.schur_device(Lf, m, factor=True)
        b, fb = S.schur_device(Lf, m, factor=True)
        assert torch.equal(a, b) and torch.equal(fa, fb)
        # the two products against numpy, L22' V twice: the same bits
        F = fa.cpu().numpy()
        V = torch.from_numpy(np.random.default_rng(m).standard_normal((9, m))).cuda()
        t1, t2, n1 = _multiply(S, Lf, m, 1, V), _multiply(S, Lf, m, 1, V), _multiply(S, Lf, m, 0, V)
        assert torch.equal(t1, t2)
        Vh = V.cpu().numpy()
        for got, want in ((t1, Vh @ F), (n1, Vh @ F.T)):
            err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
            print(f"samebits: m={m} product err={err:.2e} tol={tol:.2e}")
            assert err <= tol
        assert S.L.cholmod_hip_trailing_multiply_device(Lf.contents.hip_plan, m, 0, V.data_ptr(), m, V.data_ptr(), m, 9,
                                                        None) == ch.HIP_INVALID
    # new values from the device: the Schur complement of the new matrix
    m = n // 2
    old = S.schur_device(Lf, m)
    scale = 1.0 + 0.5 * np.random.default_rng(32).uniform(size=n)
    cols = np.repeat(np.arange(n), np.diff(case["Lp"]))
    case2 = dict(case, Lx=case["Lx"] * scale[case["Li"]] * scale[cols])
    assert S.factorize_device(A, torch.from_numpy(case2["Lx"]).cuda(), Lf) == 1 and S.cm.status == ch.OK
    new = S.schur_device(Lf, m).cpu().numpy()
    fv, fac, tol = _host_factor(S, Lf)
    ref = R.dense_schur(R.permuted_dense(case2, fv.Perm), m)
    err = np.abs(new - ref).max() / np.abs(ref).max()
    print(f"samebits: after factorize_device err={err:.2e} tol={tol:.2e}")
    assert err <= tol and not np.array_equal(new, old.cpu().numpy())
    _done(S, A, Lf)


def case_condensed():
    """reduce, a dense solve with F on the interface, expand: G against the dense condensed right-hand side, X against
    solve_device, its residual norm against solve_device's"""
    out = {}
    for name, mk in (("p3d_12_nd", "half"), ("p3d_12_nd", 65), ("forest148", 100), ("bcsstk01", 17)):
        case = R.CASES[name]()
        n = case["n"]
        m = n // 2 if mk == "half" else mk
        S, A, Lf = R.factorized(case, use_gpu=1)
        fv, fac, tol = _host_factor(S, Lf)
        M = R.permuted_dense(case, fv.Perm)
        Sc, F = S.schur_device(Lf, m, factor=True)
        assert np.array_equal(S.schur_index(Lf, m), fv.Perm[n - m:])
        for nrhs in (1, 7, 8, 17):
            Bh = np.random.default_rng(100 + nrhs).standard_normal((nrhs, n))
            B = torch.from_numpy(Bh).cuda()
            Gd, Y = S.schur_reduce_device(Lf, m, B)
            assert tuple(Gd.shape) == (nrhs, m) and tuple(Y.shape) == (nrhs, n)
            Gref = R.dense_reduce(M, m, Bh[:, fv.Perm].T).T
            eg = np.abs(Gd.cpu().numpy() - Gref).max() / np.abs(Gref).max()
            Y0 = Y.clone()
            xS = torch.cholesky_solve(Gd.t().contiguous(), F).t().contiguous()
            X = S.schur_expand_device(Lf, m, Y, xS)
            assert torch.equal(Y, Y0)                                   # Y is read only
            Xs = S.solve_device(Lf, B)
            ex = float((X - Xs).abs().max() / Xs.abs().max())
            # the trailing rows of X come out as x_S
            exs = float((X[:, torch.from_numpy(fv.Perm[n - m:].copy()).cuda()] - xS).abs().max() / xS.abs().max())
            _, r1 = S.refine_device(Lf, B, X, steps=0, norms=True)
            _, r0 = S.refine_device(Lf, B, Xs, steps=0, norms=True)
            r1, r0 = float(r1.max()), float(r0.max())
            bmax = float(np.abs(Bh).max())
            print(f"condensed {name} m={m} nrhs={nrhs}: G {eg:.2e} X {ex:.2e} X_S {exs:.2e} tol {tol:.2e}; residual {r1:.2e}, "
                  f"of solve_device {r0:.2e}, tol max |B| {tol * bmax:.2e}")
            out[f"{name}|{mk}|{nrhs}"] = [float(eg), ex, exs, tol, r1, r0, tol * bmax]
        _done(S, A, Lf)
    print("RESULT " + json.dumps(out))


def _p3d9_subset():
    n, Ap, Ai, Ax = G.poisson3d(9)
    sub = np.random.default_rng(5).permutation(n)[:40].astype(np.int64)
    case = dict(n=n, Lp=Ap, Li=Ai, Lx=Ax)
    Ad = R.dense_symmetric(n, Ap, Ai, Ax)
    keep = np.ones(n, dtype=bool)
    keep[sub] = False
    q = np.concatenate([np.flatnonzero(keep), sub])
    return case, sub, R.dense_schur(Ad[np.ix_(q, q)], len(sub))


def case_subset():
    case, sub, ref = _p3d9_subset()
    n, m = case["n"], len(sub)
    outcome = {}
    for postorder in (False, True):
        S = ch.Session(postorder=postorder)
        A = S.sparse(n, case["Lp"], case["Li"], case["Lx"], -1)
        perm = ch.Session.schur_perm(A, sub)
        Lf = S.analyze(A, perm)
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
        fv, fac, tol = _host_factor(S, Lf)
        try:
            Sc = S.schur_device(Lf, subset=sub).cpu().numpy()
        except ValueError as e:
            assert postorder and "postorder=False" in str(e), e
            assert set(fv.Perm[n - m:].tolist()) != set(sub.tolist())
            outcome[str(postorder)] = "refused"
        else:
            err = np.abs(Sc - ref).max() / np.abs(ref).max()
            print(f"subset postorder={postorder}: err={err:.2e} tol={tol:.2e}")
            assert err <= tol, (postorder, err, tol)
            outcome[str(postorder)] = "passed"
        # not the set of the last m variables: refused whatever the postorder
        other = sub.copy()
        other[0] = int(np.setdiff1d(np.arange(n), sub)[0])
        try:
            S.schur_device(Lf, subset=other)
            raise AssertionError("a subset that is not ordered last was accepted")
        except ValueError as e:
            assert "postorder=False" in str(e)
        _done(S, A, Lf)
    assert outcome["False"] == "passed"
    print("RESULT " + json.dumps(outcome))


def case_larger(k="24"):
    """Poisson k^3 with the geometric nested dissection: m = the top separator's supernode and m = 2000, which reaches
    into sibling separators that are not in each other's row lists.  Sc inv (A)_SS = I on 16 columns of S."""
    k = int(k)
    n, Ap, Ai, Ax = G.poisson3d(k)
    S = ch.Session()
    A = S.sparse(n, Ap, Ai, Ax, -1)
    Lf = S.analyze(A, G.geometric_nd(k, k, k, 4))
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    fv, fac, tol = _host_factor(S, Lf)
    top = int(fv.super[-1] - fv.super[-2])
    out = {}
    for m in (top, 2000):
        Sc = S.schur_device(Lf, m)
        idx = S.schur_index(Lf, m)
        js = np.arange(16) * (m // 16) + (m // 32)
        E = torch.zeros((16, n), dtype=torch.float64, device="cuda")
        E[torch.arange(16), torch.from_numpy(idx[js]).cuda()] = 1.0
        XS = S.solve_device(Lf, E)[:, torch.from_numpy(idx).cuda()]           # (16, m): columns j of inv (A)_SS
        P = (Sc @ XS.t()).cpu().numpy()                                         # (m, 16)
        want = np.zeros((m, 16))
        want[js, np.arange(16)] = 1.0
        err = float(np.abs(P - want).max())
        sym = bool(torch.equal(Sc, Sc.t()))
        print(f"larger {k}^3: n={n} m={m} (top separator {top}) |Sc inv (A)_SS - I| = {err:.2e} tol={tol:.2e} symmetric={sym}")
        assert sym
        out[str(m)] = [err, tol]
    _done(S, A, Lf)
    print("RESULT " + json.dumps(out))


def case_stream():
    """schur_device on a side stream behind the torch ops that produce the values and the factorization from them, its
    result consumed on that stream without a host wait; further calls allocate nothing"""
    case = R.CASES["p2d_60_nd"]()
    n, m = case["n"], 300
    S, A, Lf = R.factorized(case, use_gpu=1)
    plan = Lf.contents.hip_plan
    s = torch.cuda.Stream()
    half = torch.from_numpy(0.5 * case["Lx"]).cuda()
    Bt = torch.from_numpy(np.random.default_rng(1).standard_normal((9, n))).cuda()
    S.schur_device(Lf, m, factor=True)              # (the events and the workspaces exist from here on)
    S.schur_expand_device(Lf, m, *S.schur_reduce_device(Lf, m, Bt)[::-1])
    torch.cuda.synchronize()
    for rep in range(2):
        with torch.cuda.stream(s):
            v = half
            for _ in range(20):
                v = v * 1.0 + 0.0
            v = v + half * (1.0 + rep)      # rep 0: A itself, rep 1: 1.5 A
            assert S.factorize_device(A, v, Lf) == 1 and S.cm.status == ch.OK
            Sc = S.schur_device(Lf, m)
            Z = Sc * 2.0
        s.synchronize()
        fv, fac, tol = _host_factor(S, Lf)
        ref = R.dense_schur(R.permuted_dense(dict(case, Lx=case["Lx"] * (1.0 + 0.5 * rep)), fv.Perm), m)
        err = np.abs(Z.cpu().numpy() - 2.0 * ref).max() / np.abs(2.0 * ref).max()
        print(f"stream rep {rep}: {err:.2e} tol {tol:.2e}")
        assert err <= tol, (rep, err, tol)
    # the engine's own calls, no torch allocation in between: the free memory of the device does not move
    Fb, V, W = torch.empty_like(Sc), torch.ones((3, m), dtype=torch.float64, device="cuda"), torch.empty((3, m), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        assert S.L.cholmod_hip_schur_device(plan, m, Sc.data_ptr(), m, Fb.data_ptr(), m, s.cuda_stream) == ch.HIP_OK
        for trans in (0, 1):
            assert S.L.cholmod_hip_trailing_multiply_device(plan, m, trans, V.data_ptr(), m, W.data_ptr(), m, 3, s.cuda_stream) == ch.HIP_OK
    s.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    _done(S, A, Lf)


def _three(S, Lf, n, m=3):
    """status of the three host entry points on real device arrays"""
    t = [torch.zeros((2, k), dtype=torch.float64, device="cuda") for k in (n, n, n, m, m)]
    sq = torch.zeros((m, m), dtype=torch.float64, device="cuda")
    got = []
    S.cm.status = ch.OK
    got.append((S.L.cholmod_l_hip_schur_device(Lf, m, sq.data_ptr(), m, None, m, None, C.byref(S.cm)), S.cm.status))
    S.cm.status = ch.OK
    got.append((S.L.cholmod_l_hip_schur_reduce_device(Lf, m, t[0].data_ptr(), n, t[1].data_ptr(), n, t[3].data_ptr(), m, 2, None,
                                                      C.byref(S.cm)), S.cm.status))
    S.cm.status = ch.OK
    got.append((S.L.cholmod_l_hip_schur_expand_device(Lf, m, t[1].data_ptr(), n, t[4].data_ptr(), m, t[2].data_ptr(), n, 2, None,
                                                      C.byref(S.cm)), S.cm.status))
    torch.cuda.synchronize()
    assert all(float(x.abs().max()) == 0.0 for x in t + [sq])
    return got


def case_refusals():
    # a complex factor: not installed
    n, Ap, Ai, Ax = G.poisson3d(6)
    Hx = G.hermitian_phases(n, Ap, Ai, Ax, seed=5)
    S = ch.Session()
    S.cm.error_handler = ch.ERRFUNC(0)
    A = S.sparse(n, Ap, Ai, Hx, -1)
    Lf = S.analyze(A)
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    assert _three(S, Lf, n) == [(0, ch.NOT_INSTALLED)] * 3
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
    m = min(3, case["n"])
    assert _three(S, Lf, case["n"], m) == [(0, ch.INVALID)] * 3
    plan = Lf.contents.hip_plan
    if plan:
        sq = torch.zeros((m, m), dtype=torch.float64, device="cuda")
        assert S.L.cholmod_hip_schur_device(plan, m, sq.data_ptr(), m, None, m, None) == ch.HIP_INVALID
        assert S.L.cholmod_hip_trailing_multiply_device(plan, m, 1, sq.data_ptr(), m, sq.data_ptr() + 8 * m * m, m, 0, None) == ch.HIP_INVALID
    fv = ch.FactorView(Lf)
    assert fv.minor == minor0 and (x0 is None or np.array_equal(fv.x, x0))
    _done(S, A, Lf)
    # on a good factor: the engine's own refusals, and m = 0 / nrhs = 0 touch nothing
    case = R.CASES["bcsstk01"]()
    n = case["n"]
    S, A, Lf = R.factorized(case, use_gpu=1)
    plan = Lf.contents.hip_plan
    sq = torch.full((4, 4), POISON, dtype=torch.float64, device="cuda")
    p = sq.data_ptr()
    lib = S.L
    assert lib.cholmod_hip_schur_device(plan, -1, p, 4, None, 4, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_schur_device(plan, n + 1, p, n + 1, None, 4, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_schur_device(plan, 4, p, 3, None, 4, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_schur_device(plan, 4, None, 4, p, 3, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_schur_device(plan, 4, None, 4, None, 4, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_trailing_multiply_device(plan, 2, 0, p, 2, p + 64, 2, -1, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_trailing_multiply_device(plan, 2, 0, p, 1, p + 64, 2, 1, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_trailing_multiply_device(plan, 2, 0, p, 2, p, 2, 1, None) == ch.HIP_INVALID
    assert lib.cholmod_hip_schur_device(plan, 0, p, 0, None, 0, None) == ch.HIP_OK
    assert lib.cholmod_hip_trailing_multiply_device(plan, 2, 1, p, 2, p + 64, 2, 0, None) == ch.HIP_OK
    torch.cuda.synchronize()
    assert bool((sq == POISON).all())
    # an m = 0 expansion is the plain L' solve
    B = torch.from_numpy(np.random.default_rng(3).standard_normal((2, n))).cuda()
    Y = S.solve_device(Lf, S.solve_device(Lf, B, ch.SYS_P), ch.SYS_L)
    X = S.schur_expand_device(Lf, 0, Y, torch.zeros((2, 0), dtype=torch.float64, device="cuda"))
    Xp = S.solve_device(Lf, S.solve_device(Lf, Y, ch.SYS_Lt), ch.SYS_Pt)
    assert float((X - Xp).abs().max()) <= 1e-13 * float(Xp.abs().max())
    G0, Y0 = S.schur_reduce_device(Lf, 0, B)
    assert tuple(G0.shape) == (2, 0)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
