"""The bodies of tests/test_gpu_aat_grad.py, run in a process of their own: `python aat_grad_cases.py CASE [ARG ...]`, torch
imported FIRST (see solve_device_cases.py).  Exit status 0 = every assertion held.  Matrices: tests/aat_grad_matrices.py;
formulas, the dense torch reference and the bars: tests/aat_grad_reference.py; the helpers of tests/grad_cases.py are
shared.  Every figure is printed before it is asserted."""
import torch  # noqa: E402  (first)

import ctypes as C
import sys

import numpy as np

import grad_cases as GC
from grad_cases import NAN, _count, _dev, _ints, _ld
import aat_grad_matrices as AM
import aat_grad_reference as AR
import grad_reference as GR
import selinv_reference as R
from suitesparse_amd import cholmod as ch
from suitesparse_amd.autograd import DeviceCholesky

EPS53 = AR.EPS53


def _rect(S, M):
    m, n = M.shape
    A = S.L.cholmod_l_allocate_sparse(m, n, max(M.nnz, 1), 1, 1, 0, ch.REAL, C.byref(S.cm))
    assert A
    a = A.contents
    ch._view(a.p, n + 1, C.c_int64, np.int64)[:] = M.indptr
    ch._view(a.i, M.nnz, C.c_int64, np.int64)[:] = M.indices
    ch._view(a.x, M.nnz, C.c_double, np.float64)[:] = M.data
    return A


def _factorized(M, beta):
    """-> (Session, A, Lf): L L' = A A' + beta I factorized from the host; no product map yet"""
    S = ch.Session(ordering="default")
    S.cm.error_handler = ch.ERRFUNC(0)
    A = _rect(S, M)
    Lf = S.L.cholmod_l_analyze(A, C.byref(S.cm))
    assert Lf and S.cm.status == ch.OK and Lf.contents.n == M.shape[0]
    assert S.factorize(A, Lf, beta) == 1 and S.cm.status == ch.OK and Lf.contents.hip_apat_valid == 1
    assert Lf.contents.hip_aat_valid == 0
    return S, A, Lf


def _done(S, A, Lf):
    GC._done(S, A, Lf)


def _engine(S, Lf, perm, alpha, U, V, a, stream=None, out=None, navalues=None, ldu=None, nrhs=None):
    """cholmod_hip_product_values_grad_device on (nrhs, n) tensors; dGa pre-filled with NaN -> (status, dGa)"""
    na = a.shape[0] if navalues is None else navalues
    g = torch.full((a.shape[0],), NAN, dtype=torch.float64, device="cuda") if out is None else out
    rc = S.L.cholmod_hip_product_values_grad_device(Lf.contents.hip_plan, perm, alpha, U.data_ptr() or 1, _ld(U) if ldu is None else ldu,
                                                    V.data_ptr() or 1, _ld(V), U.shape[0] if nrhs is None else nrhs,
                                                    a.data_ptr() or 3, g.data_ptr() or 2, na, stream)
    return rc, g


def _maps(M):
    Cp, Ci, cp, ia, ib = AR.product_map(M)
    return (Cp, Ci, cp, ia, ib), AR.transpose_map(cp, ia, ib, M.nnz)


def case_exact(name):
    """small integers and alpha = -1: every product and every sum is exact in any order (|Gv| <= 2 * 33 * 64, |a| <= 8, at
    most 161 terms: far below 2^53), so dGa equals the numpy reference exactly.  Both sides of SD_BLOCK_MIN_NRHS, a partial
    last panel, three panels; the host layer and the engine with perm = 1 and 0; once with ld > n, once with U and V the
    same array; dGa pre-filled with NaN, which equals nothing.  The FIRST call builds the product map and its transpose:
    the factor comes from the host and no factorize_device has run."""
    M = AM.MATRICES[name]()
    m, nnz = M.shape[0], M.nnz
    a = AM.integer_values(name, M)
    (Cp, Ci, cp, ia, ib), (tp, tc, tpart) = _maps(M)
    S, A, Lf = _factorized(M, AM.shift_of(name, M))
    P = ch.FactorView(Lf).Perm.copy()
    ad = _dev(a)
    rng = np.random.default_rng(21)
    for nrhs in (1, 7, 8, 16, 19, 33):
        U, V = _ints(rng, nrhs, m), _ints(rng, nrhs, m)
        ref = AR.product_grad(tp, tc, tpart, GR.values_grad(Cp, Ci, -1, U, V, -1.0), a)
        Ud, Vd = _dev(U), _dev(V)
        out = torch.full((nnz,), NAN, dtype=torch.float64, device="cuda")
        g_host = S.aat_values_grad_device(A, Lf, ad, Ud, Vd, alpha=-1.0, out=out)
        assert Lf.contents.hip_aat_valid == 1
        rc1, g1 = _engine(S, Lf, 1, -1.0, Ud, Vd, ad)
        rc0, g0 = _engine(S, Lf, 0, -1.0, _dev(U[:, P]), _dev(V[:, P]), ad)
        wide = torch.full((2 * nrhs, m + 5), NAN, dtype=torch.float64, device="cuda")
        wide[:nrhs, :m], wide[nrhs:, :m] = Ud, Vd
        g_ld = S.aat_values_grad_device(A, Lf, ad, wide[:nrhs, :m], wide[nrhs:, :m], alpha=-1.0)
        rcs, g_same = _engine(S, Lf, 1, -1.0, Ud, Ud, ad)
        torch.cuda.synchronize()
        assert rc1 == rc0 == rcs == ch.HIP_OK
        bad = {k: int((g.cpu().numpy() != ref).sum()) for k, g in (("host", g_host), ("perm1", g1), ("perm0", g0), ("ld", g_ld))}
        ref_same = AR.product_grad(tp, tc, tpart, GR.values_grad(Cp, Ci, -1, U, U, -1.0), a)
        bad["same"] = int((g_same.cpu().numpy() != ref_same).sum())
        print(f"exact {name} nrhs={nrhs}: nnz={nnz} list lengths {np.diff(tp).min()}..{np.diff(tp).max()} entries that differ {bad}")
        assert not any(bad.values()), (name, nrhs, bad)
    # nrhs == 0: a success that zero-fills, whatever the values are
    z = torch.zeros((0, m), dtype=torch.float64, device="cuda")
    rc, g = _engine(S, Lf, 1, -1.0, z, z, torch.full((nnz,), NAN, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert rc == ch.HIP_OK and np.array_equal(g.cpu().numpy().view(np.int64), np.zeros(nnz, dtype=np.int64))
    _done(S, A, Lf)


def _z_at_entries(fv, Zx, Cp, Ci):
    """Z at the entries (i, j) of tril (A A') (the caller's ordering) from the selected inverse in the layout of L->x"""
    P = np.asarray(fv.Perm)
    ip = np.empty_like(P)
    ip[P] = np.arange(len(P))
    cols = GR.columns_of(Cp)
    out = np.empty(len(Ci))
    for c in range(len(Ci)):
        r, cc = max(ip[Ci[c]], ip[cols[c]]), min(ip[Ci[c]], ip[cols[c]])
        k = int(np.searchsorted(fv.super, cc, side="right")) - 1
        rows = fv.s[fv.pi[k]:fv.pi[k + 1]]
        q = int(np.searchsorted(rows, r))
        assert rows[q] == r
        out[c] = Zx[fv.px[k] + (cc - fv.super[k]) * len(rows) + q]
    return out


def case_logdet_grad(name):
    """with integer values a, aat_logdet_grad_device against the chain step applied in numpy to the Z of the SAME run
    (selinv_host: the device's own Zx), Gv = Z on the diagonal and 2 Z off it: the comparison isolates k_product_grad.
    Bit for bit against the sums taken in the kernel's documented order (fused multiply-adds, the butterfly), and within
    (len_q + 2) 2^-53 sum |Gv_c| |a_partner| of the plain numpy sum -- a dot product of len_q terms in any order; derived,
    not measured.  Then the engine's entry with OTHER small integers as dA on the same Zx: the kernel on its own."""
    M = AM.MATRICES[name]()
    nnz = M.nnz
    a = AM.integer_values(name, M)
    (Cp, Ci, cp, ia, ib), (tp, tc, tpart) = _maps(M)
    beta = AM.shift_of(name, M)
    S, A, Lf = _factorized(M, beta)
    ad = _dev(a)
    assert S.factorize_device(A, ad, Lf, beta) == 1 and S.cm.status == ch.OK and Lf.contents.minor == M.shape[0]
    out = torch.full((nnz,), NAN, dtype=torch.float64, device="cuda")
    g = S.aat_logdet_grad_device(A, Lf, ad, out=out)
    g2 = S.aat_logdet_grad_device(A, Lf, ad)
    a2 = np.random.default_rng(22).integers(-4, 5, size=nnz).astype(np.float64)
    g3 = torch.full((nnz,), NAN, dtype=torch.float64, device="cuda")
    assert S.L.cholmod_hip_product_logdet_grad_device(Lf.contents.hip_plan, _dev(a2).data_ptr(), g3.data_ptr(), nnz, None) == ch.HIP_OK
    torch.cuda.synchronize()
    Zx = S.selinv_host(Lf)
    S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    Z = _z_at_entries(ch.FactorView(Lf), Zx, Cp, Ci)
    Gv = np.where(Ci == GR.columns_of(Cp), 1.0, 2.0) * Z
    assert np.all(np.isfinite(Gv))
    for tag, got, av in (("host layer", g.cpu().numpy(), a), ("engine, other values", g3.cpu().numpy(), a2)):
        ordered = AR.product_grad_in_kernel_order(tp, tc, tpart, Gv, av)
        plain = AR.product_grad(tp, tc, tpart, Gv, av)
        bound = (np.diff(tp) + 2) * EPS53 * AR.product_grad_magnitude(tp, tc, tpart, Gv, av)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = float(np.max(np.where(bound > 0, np.abs(got - plain) / bound, np.where(got == plain, 0.0, np.inf))))
        nbits = int((got.view(np.int64) != ordered.view(np.int64)).sum())
        print(f"logdet_grad {name} ({tag}): {nbits} of {nnz} values differ in bits from the kernel-order sums; "
              f"worst |g - numpy| / bound = {w:.3e}")
        assert np.all(np.isfinite(got)) and w <= 1.0, (name, tag, w)
        assert nbits == 0, (name, tag, nbits)
    assert np.array_equal(g.cpu().numpy().view(np.int64), g2.cpu().numpy().view(np.int64))
    _done(S, A, Lf)


def case_rounded(name):
    """rows of U and V scaled by 2^+-20, a uniform in [0.5, 2): per value within
        (len_q + 2) 2^-53 sum |Gv_c a_partner|  +  sum |a_partner| 2 (2 nrhs + 2) 2^-53 |alpha| mag_c
    of numpy -- the chain step as a dot product of len_q terms, plus the bar of the sampled product
    (grad_cases.case_rounded) carried through the chain; two calls give the same bits, and so does a call after the product
    map was dropped and set again (the transposed map is rebuilt from it)"""
    alpha = -0.7
    M = AM.MATRICES[name]()
    m, nnz = M.shape[0], M.nnz
    (Cp, Ci, cp, ia, ib), (tp, tc, tpart) = _maps(M)
    S, A, Lf = _factorized(M, AM.shift_of(name, M))
    plan = Lf.contents.hip_plan
    rng = np.random.default_rng(23)
    a = rng.uniform(0.5, 2.0, nnz)
    ad = _dev(a)
    for nrhs in (3, 8, 19, 33):
        U = rng.standard_normal((nrhs, m)) * np.exp2(rng.integers(-20, 21, size=m))
        V = rng.standard_normal((nrhs, m)) * np.exp2(rng.integers(-20, 21, size=m))
        Gv = GR.values_grad(Cp, Ci, -1, U, V, alpha)
        ref = AR.product_grad(tp, tc, tpart, Gv, a)
        bar_c = 2 * (2 * nrhs + 2) * EPS53 * abs(alpha) * GR.values_grad_magnitude(Cp, Ci, U, V)
        bar = (np.diff(tp) + 2) * EPS53 * AR.product_grad_magnitude(tp, tc, tpart, Gv, a) \
            + AR.product_grad_magnitude(tp, tc, tpart, bar_c, a)
        Ud, Vd = _dev(U), _dev(V)
        g1 = S.aat_values_grad_device(A, Lf, ad, Ud, Vd, alpha=alpha)
        g2 = S.aat_values_grad_device(A, Lf, ad, Ud, Vd, alpha=alpha)
        torch.cuda.synchronize()
        # the product map dropped and set again: the transposed map goes with it and is built anew
        assert S.L.cholmod_hip_set_product_map(plan, None, None, None, 0, 0) == ch.HIP_OK
        assert _engine(S, Lf, 1, alpha, Ud, Vd, ad)[0] == ch.HIP_INVALID
        assert S.L.cholmod_hip_set_product_map(plan, cp.ctypes.data, ia.ctypes.data, ib.ctypes.data, len(Ci), nnz) == ch.HIP_OK
        rc, g3 = _engine(S, Lf, 1, alpha, Ud, Vd, ad)
        torch.cuda.synchronize()
        assert rc == ch.HIP_OK
        g1, g2, g3 = g1.cpu().numpy(), g2.cpu().numpy(), g3.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            w = float(np.nanmax(np.where(bar > 0, np.abs(g1 - ref) / bar, np.where(g1 == ref, 0.0, np.inf))))
        print(f"rounded {name} nrhs={nrhs}: worst |g - ref| / bar = {w:.3e}")
        assert np.all(np.isfinite(g1)) and w <= 1.0, (name, nrhs, w)
        assert np.array_equal(g1.view(np.int64), g2.view(np.int64)), (name, nrhs)
        assert np.array_equal(g1.view(np.int64), g3.view(np.int64)), (name, nrhs)
    _done(S, A, Lf)


def _check(tag, gv, gb, gbeta, ref, bars):
    ev = float(np.abs(gv.cpu().numpy() - ref["grad_values"]).max())
    eb = float(np.abs(gb.cpu().numpy() - ref["grad_B"]).max())
    ebeta = abs(float(gbeta) - ref["grad_beta"])
    print(f"{tag}: grad_values {ev:.2e} (bar {bars[0]:.2e}), grad_B {eb:.2e} (bar {bars[1]:.2e}), grad_beta {ebeta:.2e} (bar {bars[2]:.2e})")
    assert ev <= bars[0] and eb <= bars[1] and ebeta <= bars[2], (tag, ev, eb, ebeta, bars)


def case_autograd(name):
    """loss = (W . chol.solve (v, B)).sum () + 0.3 chol.logdet (v) through DeviceCholesky on an unsymmetric A with a tensor
    beta that requires grad (on the device for beta = 0, on the host for the other), against the same loss from the dense
    D D' + beta I with torch in float64 on the CPU; beta 0 and 0.375 (afiro: 1e-3 max |A A'|), nrhs 1 and 19; the bars of
    aat_grad_reference.bars; one factorization for logdet + solve; a second backward after an intervening factorize_device
    with other values still gives the first matrix's gradient; a Python-float beta gives the same gradients of values and B
    bit for bit"""
    M = AM.MATRICES[name]()
    m, nnz = M.shape[0], M.nnz
    a = M.data.copy()
    for k, beta in enumerate((0.0, AM.shift_of(name, M))):
        S, A, Lf = _factorized(M, beta)
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
        bt = torch.tensor(beta, dtype=torch.float64, device="cuda" if k == 0 else "cpu", requires_grad=True)
        chol, chol_f = DeviceCholesky(S, A, Lf, bt), DeviceCholesky(S, A, Lf, beta)
        other = _dev(a * np.where(np.arange(nnz) % 3 == 0, 1.25, 0.75))
        for nrhs in (1, 19):
            tag = f"autograd {name} beta={beta:.3e} nrhs={nrhs}"
            B, W = GR.inputs(m, nrhs, 7)
            ref = AR.torch_reference(M, a, beta, B, W)
            bars = AR.bars(M, a, ref, tol, nrhs)
            v, Bd, Wd = _dev(a).requires_grad_(), _dev(B).requires_grad_(), _dev(W)
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
            assert v.grad.shape == v.shape and Bd.grad.shape == Bd.shape and bt.grad.shape == () and bt.grad.device == bt.device
            _check(tag, v.grad, Bd.grad, bt.grad, ref, bars)
            gv1, gb1 = v.grad.clone(), Bd.grad.clone()
            # the factor is replaced behind the wrapper's back: the second backward refactorizes from the saved values
            v.grad = Bd.grad = bt.grad = None
            assert S.factorize_device(A, other, Lf, beta) == 1 and S.cm.status == ch.OK
            c1 = _count(S, Lf)
            loss.backward()
            assert _count(S, Lf) - c1 == 1, tag
            _check(tag + " (stale factor)", v.grad, Bd.grad, bt.grad, ref, bars)
            bt.grad = None
            # a Python-float beta: the same gradients of values and B, bit for bit
            v2, B2 = _dev(a).requires_grad_(), _dev(B).requires_grad_()
            ((Wd * chol_f.solve(v2, B2)).sum() + 0.3 * chol_f.logdet(v2)).backward()
            torch.cuda.synchronize()
            assert torch.equal(v2.grad.view(torch.int64), gv1.view(torch.int64)), tag
            assert torch.equal(B2.grad.view(torch.int64), gb1.view(torch.int64)), tag
        _done(S, A, Lf)


def case_symmetric_beta():
    """a symmetric A (p3d_12_nd) with a tensor beta that requires grad: the gradient with respect to beta against dense
    torch, beta 0 and 0.375, nrhs 1 and 19; values and B at the bars of tests/grad_cases.py"""
    case = R.CASES["p3d_12_nd"]()
    n, Ap, Ai, Ax = case["n"], case["Lp"], case["Li"], case["Lx"]
    for beta in (0.0, GC.BETA):
        S, A, Lf = R.factorized(case, use_gpu=1, beta=beta)
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
        bt = torch.tensor(beta, dtype=torch.float64, device="cuda", requires_grad=True)
        chol = DeviceCholesky(S, A, Lf, bt)
        for nrhs in (1, 19):
            B, W = GR.inputs(n, nrhs, 7)
            ref = AR.torch_reference_symmetric(n, Ap, Ai, Ax, -1, beta, B, W)
            v, Bd, Wd = _dev(Ax).requires_grad_(), _dev(B).requires_grad_(), _dev(W)
            ((Wd * chol.solve(v, Bd)).sum() + 0.3 * chol.logdet(v)).backward()
            bv, bb = GR.bars(ref, tol, nrhs)
            bbeta = tol * n * (2 * nrhs * ref["lam_max"] * ref["x_max"] + 0.3 * ref["z_max"])
            _check(f"symmetric_beta beta={beta} nrhs={nrhs}", v.grad, Bd.grad, bt.grad, ref, (bv, bb, bbeta))
            bt.grad = None
        _done(S, A, Lf)


def case_stream():
    """a forward and a backward on a side stream behind the torch ops that produce the values, the gradients consumed on
    that stream without a host wait; then three engine-level calls of each new entry point allocate nothing"""
    name = "engineered"
    M = AM.MATRICES[name]()
    m, nnz = M.shape[0], M.nnz
    a = M.data.copy()
    beta = 0.375
    S, A, Lf = _factorized(M, beta)
    bt = torch.tensor(beta, dtype=torch.float64, device="cuda", requires_grad=True)
    chol = DeviceCholesky(S, A, Lf, bt)
    nrhs = 19
    B, W = GR.inputs(m, nrhs, 9)
    half, Bh, Wd = _dev(0.5 * a), _dev(B), _dev(W)
    s = torch.cuda.Stream()
    for rep in range(3):                # (rep 0 on the default stream: the workspaces and the maps exist from there on)
        scale = 1.0 + 0.5 * (rep % 2)
        with torch.cuda.stream(s if rep else torch.cuda.default_stream()):
            v = half
            for _ in range(20):
                v = v * 1.0 + 0.0
            v = (v + half * (2.0 * scale - 1.0)).requires_grad_()
            Bd = (Bh * 1.0).requires_grad_()
            loss = (Wd * chol.solve(v, Bd)).sum() + 0.3 * chol.logdet(v)
            loss.backward()
            Y, Yb, Ybeta = v.grad * 2.0, Bd.grad * 2.0, bt.grad * 2.0
        (s if rep else torch.cuda.default_stream()).synchronize()
        bt.grad = None
        ref = AR.torch_reference(M, a * scale, beta, B, W)
        S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
        tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
        _check(f"stream rep {rep}", Y * 0.5, Yb * 0.5, Ybeta * 0.5, ref, AR.bars(M, a * scale, ref, tol, nrhs))
    # the engine's own calls, no torch allocation in between: the free memory of the device does not move
    plan = Lf.contents.hip_plan
    ad = _dev(a)
    U3, V3 = _dev(B[:3]), _dev(W[:3])
    out = torch.empty(nnz, dtype=torch.float64, device="cuda")
    assert S.L.cholmod_hip_selinv_device(plan, s.cuda_stream) == ch.HIP_OK
    assert _engine(S, Lf, 1, -1.0, U3, V3, ad, s.cuda_stream, out)[0] == ch.HIP_OK       # (fewer than 8: its first call)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        assert _engine(S, Lf, 1, -1.0, U3, V3, ad, s.cuda_stream, out)[0] == ch.HIP_OK
        assert S.L.cholmod_hip_product_logdet_grad_device(plan, ad.data_ptr(), out.data_ptr(), nnz, s.cuda_stream) == ch.HIP_OK
        assert _engine(S, Lf, 1, -1.0, Bh, Wd, ad, s.cuda_stream, out)[0] == ch.HIP_OK
    s.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert np.array_equal(out.cpu().numpy(), S.aat_values_grad_device(A, Lf, ad, Bh, Wd, alpha=-1.0).cpu().numpy())
    _done(S, A, Lf)


def case_refusals():
    """refused on a live device, dGa untouched in every case"""
    M = AM.MATRICES["engineered"]()
    m, nnz = M.shape[0], M.nnz
    (Cp, Ci, cp, ia, ib), _ = _maps(M)
    beta = 0.375
    S, A, Lf = _factorized(M, beta)
    plan = Lf.contents.hip_plan
    rng = np.random.default_rng(24)
    Ud, Vd, ad = _dev(_ints(rng, 3, m)), _dev(_ints(rng, 3, m)), _dev(M.data)
    g = torch.full((nnz + 1,), 7.0, dtype=torch.float64, device="cuda")
    inv = ch.HIP_INVALID
    # no product map set (the factor came from the host); the permutation is there, so that nothing else is missing
    assert S.L.cholmod_hip_set_perm(plan, ch.FactorView(Lf).Perm.ctypes.data) == ch.HIP_OK
    assert _engine(S, Lf, 1, -1.0, Ud, Vd, ad, None, g)[0] == inv
    assert S.L.cholmod_hip_product_logdet_grad_device(plan, ad.data_ptr(), g.data_ptr(), nnz, None) == inv
    # ... set by the factorization from device values; a stale Zx
    assert S.factorize_device(A, ad, Lf, beta) == 1 and S.cm.status == ch.OK and Lf.contents.hip_aat_valid == 1
    assert S.L.cholmod_hip_product_logdet_grad_device(plan, ad.data_ptr(), g.data_ptr(), nnz, None) == inv
    # a wrong navalues, ld < n, nrhs < 0
    for na in (nnz + 1, nnz - 1):
        assert _engine(S, Lf, 1, -1.0, Ud, Vd, ad, None, g, navalues=na)[0] == inv
        assert S.L.cholmod_hip_product_logdet_grad_device(plan, ad.data_ptr(), g.data_ptr(), na, None) == inv
    assert _engine(S, Lf, 1, -1.0, Ud, Vd, ad, None, g, ldu=m - 1)[0] == inv
    assert _engine(S, Lf, 1, -1.0, Ud, Vd, ad, None, g, nrhs=-1)[0] == inv
    # the old entry points still refuse a plan with a product map
    assert S.L.cholmod_hip_values_grad_device(plan, 1, -1.0, Ud.data_ptr(), m, Vd.data_ptr(), m, 3, g.data_ptr(), len(Ci), None) == inv
    assert S.L.cholmod_hip_selinv_device(plan, None) == ch.HIP_OK
    assert S.L.cholmod_hip_selinv_gather_device(plan, g.data_ptr(), len(Ci), None, 1, None) == inv
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())
    # (with the selected inverse current the call works)
    assert S.L.cholmod_hip_product_logdet_grad_device(plan, ad.data_ptr(), g.data_ptr(), nnz, None) == ch.HIP_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all()) and float(g[nnz]) == 7.0
    g.fill_(7.0)
    # a factor that is not positive definite: A A' - 1e6 I
    S.factorize_device(A, ad, Lf, -1e6)
    assert Lf.contents.minor < m
    assert S.L.cholmod_hip_product_logdet_grad_device(plan, ad.data_ptr(), g.data_ptr(), nnz, None) == inv
    assert S.L.cholmod_l_hip_aat_logdet_grad_device(A, Lf, ad.data_ptr(), g.data_ptr(), None, C.byref(S.cm)) == 0 and S.cm.status == ch.INVALID
    # a symmetric A at the host layer
    A.contents.stype = -1
    assert S.L.cholmod_l_hip_aat_values_grad_device(A, Lf, -1.0, Ud.data_ptr(), m, Vd.data_ptr(), m, 3, ad.data_ptr(), g.data_ptr(), None,
                                                    C.byref(S.cm)) == 0 and S.cm.status == ch.INVALID
    A.contents.stype = 0
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())
    _done(S, A, Lf)
    # a complex factor: not installed
    from suitesparse_amd import generators as G
    n, Ap, Ai, Ax = G.poisson3d(6)
    Hx = G.hermitian_phases(n, Ap, Ai, Ax, seed=5)
    S = ch.Session()
    S.cm.error_handler = ch.ERRFUNC(0)
    H = S.sparse(n, Ap, Ai, Hx, -1)
    Lf = S.analyze(H)
    assert S.factorize(H, Lf) == 1 and S.cm.status == ch.OK
    import scipy.sparse as sp
    A = _rect(S, sp.identity(n, format="csc"))
    U = torch.ones((3, n), dtype=torch.float64, device="cuda")
    g = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    assert S.L.cholmod_l_hip_aat_values_grad_device(A, Lf, -1.0, U.data_ptr(), n, U.data_ptr(), n, 3, g.data_ptr(), g.data_ptr(), None,
                                                    C.byref(S.cm)) == 0 and S.cm.status == ch.NOT_INSTALLED
    assert S.L.cholmod_l_hip_aat_logdet_grad_device(A, Lf, g.data_ptr(), g.data_ptr(), None, C.byref(S.cm)) == 0
    assert S.cm.status == ch.NOT_INSTALLED
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())
    S.free_sparse(H)
    _done(S, A, Lf)


if __name__ == "__main__":
    torch.cuda.init()
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
