"""The device fuzz, run in a process of its own (tests/test_gpu_device_fuzz.py): `python device_fuzz_runner.py SEED NCASE`,
torch imported FIRST (see solve_device_cases.py).  Every case of tests/device_fuzz_corpus.py goes through the
device-resident features -- factorization, solves, residual and refinement, selected inverse, log-determinant, the
gradients with respect to the values and through L, the Schur complement and the condensed solves (for the m of
device_fuzz_corpus.schur_ms, interleaved with the sweeps, the solves and the refactorization on the one plan),
refactorization from device values, the scratch budget, the complex solves, the complex block arrows with L judged by
supernode, the gradients through A A' + beta I and the Schur complement of that factor -- and every result is compared
with a dense float64 numpy / scipy / torch-CPU reference on P (A + beta I) P', P the factor's own Perm, at the bar the project already holds that feature to (named where
it is used).  The launches both sweeps report must be those of the launch program restated in device_fuzz_corpus.sweep_program:
a front that takes another kernel path than the class map says shows there even where both paths compute the same numbers.

A numerical mismatch prints `FAIL case K kind ... feature ...: err tol` and the run goes on; the run ends with
`RESULT {feature: [checks, failures, worst err / tol]}` and `device fuzz: N cases, F failures (seed S)`, exit status 0.
A HIP error -- a RuntimeError of torch or of a Session call, or a Session call that leaves Common->status at
CHOLMOD_GPU_PROBLEM -- ends the run at that point with a non-zero exit status: nothing more goes to the device."""
import torch  # noqa: E402  (first)

import ctypes as C
import json
import math
import os
import sys
import traceback

import numpy as np
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import aat_grad_reference as AR
import device_fuzz_corpus as DC
import factor_grad_reference as F
import grad_reference as GR
import selinv_reference as R
import residual_device_cases as RD
import schur_reference as SR
import solve_device_complex_cases as CX
from factor_grad_cases import _compare as _grad_compare
from grad_cases import _diag_of
from schur_cases import _multiply, _padded, _untouched
from selinv_cases import _entry_positions
from solve_device_cases import TOL as TOL_SOLVE, _relcols
from suitesparse_amd import cholmod as ch
from suitesparse_amd.autograd import DeviceCholesky

TOL_L = 1e-12           # tests/test_gpu_parity.py: TOL_L, ||L - L_ref||_F / ||L_ref||_F
TOL_REFINE = 1e-11      # the relative residual after one step (solve_device_complex_cases.case_residual_refine)
TOL_LOGDET = 1e-11      # relative to sum |2 log L_jj| (grad_cases.case_autograd, aat_grad_cases.case_autograd)
BUDGET = "CHOLMOD_HIP_SELINV_BUDGET_MB"
FEATURES = ("factor", "solve", "residual_refine", "selinv", "logdet", "values_grad", "factor_grad", "outer_grad",
            "factorize_device", "budget_bits", "complex_solve", "aat", "schur", "schur_condensed", "complex_arrow")
EXIT_HIP_ERROR = 3


class HipError(Exception):
    pass


class Book:
    def __init__(self):
        self.stats = {f: [0, 0, 0.0] for f in FEATURES}
        self.case, self.failed_cases = None, set()

    def check(self, feature, what, err, tol):
        """err <= tol (tol == 0: err counts mismatches and must be 0); a NaN is a miss"""
        err = float(err)
        ratio = (0.0 if err == 0.0 else math.inf) if tol == 0 else err / tol
        ok = ratio <= 1.0
        st = self.stats[feature]
        st[0] += 1
        st[1] += 0 if ok else 1
        st[2] = max(st[2], ratio if ratio == ratio else math.inf)
        if not ok:
            self.failed_cases.add(self.case["case"])
            print(f"FAIL {DC.describe(self.case)} feature {feature} ({what}): {err:.3e} {tol:.3e}", flush=True)
        return ok

    def result(self):
        return {f: [s[0], s[1], s[2] if math.isfinite(s[2]) else 1e300] for f, s in self.stats.items()}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _guard(S):
    if S.cm.status == ch.GPU_PROBLEM:
        raise HipError(f"Common->status is CHOLMOD_GPU_PROBLEM ({S.cm.status})")


def _info(S, Lf, which):
    out = np.zeros(8)
    rc = getattr(S.L, f"cholmod_hip_{which}_info")(Lf.contents.hip_plan, out.ctypes.data)
    if rc != ch.HIP_OK:
        raise HipError(f"cholmod_hip_{which}_info returned {rc}")
    return out


def _host_factor(S, Lf):
    S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm))
    _guard(S)
    return ch.FactorView(Lf)


def _done(S, A, Lf):
    torch.cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()


def _permuted(Ad, fv):
    p = np.asarray(fv.Perm)
    return Ad[np.ix_(p, p)]


def _check_factor(book, feature, fv, Lref, by_supernode=False):
    """L against the dense Cholesky factor at TOL_L (Frobenius), the dead triangles exact zeros; by_supernode (the block
    arrows): L by supernode at TOL_L as well, a wrong leaf that the norm over the whole factor would drown"""
    _, mask = F.trapezoid_of(np.zeros((fv.n, fv.n)), fv.super, fv.pi, fv.px, fv.s, fv.xsize)
    book.check(feature, "L", np.linalg.norm(F.dense_factor(fv) - Lref) / np.linalg.norm(Lref), TOL_L)
    book.check(feature, "dead triangles of L", np.count_nonzero(fv.x[~mask] != 0.0), 0)
    if by_supernode:
        _check_by_supernode(book, feature, fv, Lref)


def _check_by_supernode(book, feature, fv, Lref):
    """max |L - L_ref| over a supernode / max |L_ref| of it, the worst supernode, at TOL_L (not_posdef_cases.by_entry)"""
    worst, k, dead, imag = DC.by_supernode(fv, fv.x, Lref)
    shape = (int(fv.super[k + 1] - fv.super[k]), int(fv.pi[k + 1] - fv.pi[k])) if k >= 0 else None
    book.check(feature, f"L by supernode, the worst: supernode {k}, nscol x nsrow {shape}", worst, TOL_L)
    return dead, imag


def _check_schur(book, S, Lf, fv, Mp, ms, n):
    """schur_device (factor=True) for every m of ms into poisoned, over-allocated buffers: Sc against the dense Schur
    complement of Mp = P (A + beta I) P' (m = n: Mp itself) at the bar of schur_cases, relative to max |ref|; Sc bitwise
    symmetric; nothing written outside the two m x m corners; F bit for bit schur_reference.trailing_factor of the
    downloaded factor; a second call, into fresh tensors, gives the same bits -> {m: (Sc, F)}"""
    fac, tol = (fv.super, fv.pi, fv.px, fv.s, fv.x), R.tolerance(R.factor_rcond(fv))
    got = {}
    for m in ms:
        sbuf, sview = _padded(m)
        fbuf, fview = _padded(m)
        Sc, Fm = S.schur_device(Lf, m, factor=True, out=(sview, fview))
        torch.cuda.synchronize()
        _guard(S)
        book.check("schur", f"m {m}: entries written outside the m x m corners", int(not (_untouched(sbuf, m) and _untouched(fbuf, m))), 0)
        Sh, Fh = Sc.cpu().numpy(), Fm.cpu().numpy()
        ref = SR.dense_schur(Mp, m)
        with np.errstate(invalid="ignore"):
            book.check("schur", f"Sc m {m}" + (" = n, the permuted matrix itself" if m == n else ""),
                       np.abs(Sh - ref).max() / np.abs(ref).max(), tol)
        book.check("schur", f"Sc m {m} symmetric, bits", np.count_nonzero(_bits(Sh) != _bits(Sh.T)), 0)
        book.check("schur", f"F m {m}, bits", np.count_nonzero(_bits(Fh) != _bits(SR.trailing_factor(*fac, n, m))), 0)
        S2, F2 = S.schur_device(Lf, m, factor=True)
        book.check("schur", f"Sc m {m} twice, bits", np.count_nonzero(_bits(S2.cpu().numpy()) != _bits(Sh)), 0)
        book.check("schur", f"F m {m} twice, bits", np.count_nonzero(_bits(F2.cpu().numpy()) != _bits(Fh)), 0)
        _guard(S)
        got[m] = (Sh, Fh)
    return got


def _check_condensed(book, S, Lf, fv, Ad, Mp, got, ms, nrhs_list, rng):
    """reduce, the interface solve on the host with F, expand, for the first and the last m and the smallest and the largest
    nrhs: G against schur_reference.dense_reduce at the bar; X against the dense solve at solve_device_cases.TOL per column;
    X on schur_index against x_S at the bar; Y the same bits after the expansion AND after a solve_device call on other
    right-hand sides in between (the sweeps share the engine's panel).  The two trailing products against numpy at the bar,
    L22' V twice with the same bits."""
    n, P, tol = fv.n, np.asarray(fv.Perm), R.tolerance(R.factor_rcond(fv))
    for m in dict.fromkeys((ms[0], ms[-1])):
        Fh = got[m][1]
        idx = S.schur_index(Lf, m)
        book.check("schur_condensed", f"schur_index m {m}", np.count_nonzero(idx != P[n - m:]), 0)
        for nrhs in dict.fromkeys((nrhs_list[0], nrhs_list[-1])):
            b, other = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
            B = _dev(b)
            G, Y = S.schur_reduce_device(Lf, m, B)
            Gh, Y0 = G.cpu().numpy(), Y.clone()
            _guard(S)
            Gref = SR.dense_reduce(Mp, m, b[:, P].T).T
            book.check("schur_condensed", f"G m {m} nrhs {nrhs}", np.abs(Gh - Gref).max() / np.abs(Gref).max(), tol)
            xS = sla.cho_solve((Fh, True), Gh.T).T
            xo = S.solve_device(Lf, _dev(other)).cpu().numpy()
            book.check("schur_condensed", f"solve_device between reduce and expand, nrhs {nrhs}",
                       _relcols(xo, np.linalg.solve(Ad, other.T).T), TOL_SOLVE)
            X = S.schur_expand_device(Lf, m, Y, _dev(xS)).cpu().numpy()
            _guard(S)
            book.check("schur_condensed", f"Y m {m} nrhs {nrhs} unchanged, bits",
                       int((Y.view(torch.int64) != Y0.view(torch.int64)).sum()), 0)
            book.check("schur_condensed", f"X m {m} nrhs {nrhs}", _relcols(X, np.linalg.solve(Ad, b.T).T), TOL_SOLVE)
            book.check("schur_condensed", f"X on schur_index against x_S, m {m} nrhs {nrhs}",
                       np.abs(X[:, idx] - xS).max() / np.abs(xS).max(), tol)
        v = rng.standard_normal((nrhs_list[-1], m))
        V = _dev(v)
        t1, t2, n1 = _multiply(S, Lf, m, 1, V), _multiply(S, Lf, m, 1, V), _multiply(S, Lf, m, 0, V)
        _guard(S)
        book.check("schur_condensed", f"L22' V twice, m {m}, bits", int((t1.view(torch.int64) != t2.view(torch.int64)).sum()), 0)
        for name, out, want in (("L22' V", t1, v @ Fh), ("L22 V", n1, v @ Fh.T)):
            book.check("schur_condensed", f"{name} m {m}", np.abs(out.cpu().numpy() - want).max() / np.abs(want).max(), tol)


def _check_selinv(book, feature, S, A, Lf, fv, case, Ax, beta):
    """selinv_device, then selinv_host: selinv_reference.compare, the gathered values and the diagonal bit for bit -> Zx"""
    n, Ap, Ai = case["n"], case["Ap"], case["Ai"]
    Z, d = S.selinv_device(A, Lf)
    torch.cuda.synchronize()
    _guard(S)
    Z, d = Z.cpu().numpy(), d.cpu().numpy()
    Zx = S.selinv_host(Lf)
    err, tol, dead = R.compare(fv, Zx, n, Ap, Ai, Ax, beta)
    book.check(feature, "Zx against the dense inverse", err, tol)
    book.check(feature, "dead triangles of Zx", dead, 0)
    iperm = np.empty(n, dtype=np.int64)
    iperm[fv.Perm] = np.arange(n)
    cols = GR.columns_of(Ap)
    pr, pc = iperm[Ai], iperm[cols]
    pos = _entry_positions(fv, np.maximum(pr, pc), np.minimum(pr, pc))
    dpos = _entry_positions(fv, np.arange(n), np.arange(n))
    book.check(feature, "entries of A outside the pattern of L", np.count_nonzero(pos < 0), 0)
    book.check(feature, "gathered values, bits", np.count_nonzero(_bits(Z) != _bits(Zx[pos])), 0)
    book.check(feature, "gathered diagonal, bits", np.count_nonzero(_bits(d[fv.Perm]) != _bits(Zx[dpos])), 0)
    return Zx


def _check_factor_grad(book, feature, S, A, Lf, fv, Lref, seed):
    """factor_grad_device with a seeded normal Lbar and 1e30 in the dead triangles, then factor_grad_host: the dense formula
    at the bar, the dead entries +0.0 by bits -> (Gx, Lbar_x)"""
    Lbar_x, _ = F.random_lbar(fv, seed, dead=1e30)
    S.factor_grad_device(A, Lf, _dev(Lbar_x))
    Gx = S.factor_grad_host(Lf)
    _guard(S)
    Gd = F.dense_factor_grad(Lref, F.dense_of_layout(fv, Lbar_x))
    ref, mask = F.trapezoid_of(Gd, fv.super, fv.pi, fv.px, fv.s, fv.xsize)
    err, dead = _grad_compare(Gx, ref, mask)
    book.check(feature, "Gx against the dense formula", err, R.tolerance(R.factor_rcond(fv)))
    book.check(feature, "dead triangles of Gx, bits", dead, 0)
    return Gx, Lbar_x


def real_case(book, case, with_budget=True):
    """one Session, one factor: factorization, solves, residual and refinement, selected inverse, log-determinant, gradient
    with respect to the values, gradient through L (Lbar given, then formed from an outer product), refactorization from
    device values -> (Zx, Gx, launches of the two sweeps, chunks without and with the budget)"""
    n, Ap, Ai, Ax, beta = case["n"], case["Ap"], case["Ai"], case["Ax"], case["beta"]
    first = with_budget             # the second Session of a budgeted case repeats the two sweeps only
    if with_budget and case["budget"]:
        os.environ[BUDGET] = case["budget"]         # read when the plan's sweep program is built: before its first sweep
    try:
        rng = np.random.default_rng(case["rhs_seed"])
        # 1. the factorization
        S, A, Lf, ok = DC.factorized(case, use_gpu=1)
        _guard(S)
        if not ok:
            book.check("factor", f"factorize: status {S.cm.status} minor {int(Lf.contents.minor)}", 1, 0)
            _done(S, A, Lf)
            return None
        fv = _host_factor(S, Lf)
        Ad = R.dense_symmetric(n, Ap, Ai, Ax, beta)
        Lref = np.linalg.cholesky(_permuted(Ad, fv))
        if first:
            _check_factor(book, "factor", fv, Lref, by_supernode=case["kind"] == "arrow")
            # 2. the solves (solve_device_cases.TOL per column; P and Pt bit for bit)
            P = np.asarray(fv.Perm)
            xs = None
            for nrhs in case["nrhs"]:
                b = rng.standard_normal((nrhs, n))
                B = _dev(b)
                lower = sla.solve_triangular(Lref, b.T, lower=True).T
                upper = sla.solve_triangular(Lref, b.T, lower=True, trans="T").T
                full = np.linalg.solve(Ad, b.T).T
                both = np.linalg.solve(_permuted(Ad, fv), b.T).T        # (LDLt: L L' x = b, no permutation)
                ipb = np.empty_like(b)
                ipb[:, P] = b
                for name, sys_, ref in (("A", ch.SYS_A, full), ("L", ch.SYS_L, lower), ("Lt", ch.SYS_Lt, upper),
                                        ("LD", ch.SYS_LD, lower), ("DLt", ch.SYS_DLt, upper), ("LDLt", ch.SYS_LDLt, both)):
                    x = S.solve_device(Lf, B, sys_).cpu().numpy()
                    book.check("solve", f"{name} nrhs {nrhs}", _relcols(x, ref), TOL_SOLVE)
                    xs = x if sys_ == ch.SYS_A else xs
                for name, sys_, ref in (("P", ch.SYS_P, b[:, P]), ("Pt", ch.SYS_Pt, ipb)):
                    x = S.solve_device(Lf, B, sys_).cpu().numpy()
                    book.check("solve", f"{name} nrhs {nrhs}, bits", np.count_nonzero(_bits(x) != _bits(ref)), 0)
                _guard(S)
                # 3. the residual at the componentwise bound of residual_device_cases._check1, norms bit for bit
                M = RD.Sym(n, Ap, Ai, Ax, beta)
                x0 = rng.standard_normal((nrhs, n))
                Rt, nrm = S.residual_device(Lf, _dev(x0), B, norms=True)
                Rd = Rt.cpu().numpy()
                ref, bound = M.residual(x0, b)
                book.check("residual_refine", f"R nrhs {nrhs} (m = {M.m})", RD._worst(Rd, ref, bound), 1.0)
                book.check("residual_refine", f"norms nrhs {nrhs}, bits",
                           np.count_nonzero(_bits(nrm.cpu().numpy()) != _bits(np.abs(Rd).max(axis=1))), 0)
            # ... and the refinement, on the right-hand sides drawn last: steps = 0 leaves X alone, one step from an X
            # perturbed by 1e-6 brings the relative residual below 1e-11
            xp = xs * (1.0 + 1e-6 * rng.standard_normal(xs.shape))
            X = _dev(xp)
            X0 = X.clone()
            S.refine_device(Lf, B, X, steps=0)
            book.check("residual_refine", "steps = 0, bits", int((X.view(torch.int64) != X0.view(torch.int64)).sum()), 0)
            S.refine_device(Lf, B, X, steps=1)
            x1 = X.cpu().numpy()
            _guard(S)
            before = max(np.linalg.norm(b[k] - Ad @ xp[k]) / np.linalg.norm(b[k]) for k in range(len(b)))
            after = max(np.linalg.norm(b[k] - Ad @ x1[k]) / np.linalg.norm(b[k]) for k in range(len(b)))
            book.check("residual_refine", f"one step from {before:.1e}", after, TOL_REFINE)
        # 4. the selected inverse
        Zx = _check_selinv(book, "selinv" if first else "budget_bits", S, A, Lf, fv, case, Ax, beta)
        si_launches = int(_info(S, Lf, "selinv")[1])
        if first:
            # 5. the log-determinant: (n + 2) eps sum |2 log L_jj| around 2 fsum (log L_jj) (grad_cases.case_logdet)
            got = float(S.logdet_device(Lf))
            logs = 2.0 * np.log(_diag_of(fv))
            book.check("logdet", "against fsum", abs(got - math.fsum(logs)), (n + 2) * GR.EPS * float(np.abs(logs).sum()))
            # 6. the gradient with respect to the values: integers and alpha = -1, exact (grad_cases.case_exact)
            for nrhs in case["nrhs"]:
                U = rng.integers(-8, 9, size=(nrhs, n)).astype(np.float64)
                V = rng.integers(-8, 9, size=(nrhs, n)).astype(np.float64)
                g = S.values_grad_device(A, Lf, _dev(U), _dev(V), alpha=-1.0).cpu().numpy()
                book.check("values_grad", f"nrhs {nrhs}, entries that differ",
                           np.count_nonzero(g != GR.values_grad(Ap, Ai, -1, U, V, -1.0)), 0)
            _guard(S)
        # 7. the gradient through L
        Gx, _ = _check_factor_grad(book, "factor_grad" if first else "budget_bits", S, A, Lf, fv, Lref, 1000 + case["case"])
        fg_launches = int(_info(S, Lf, "factor_grad")[1])
        # ... and the launches of both sweeps: what the launch program gives for the classes of device_fuzz_corpus
        batch = DC.plan_batches(S, Lf)
        chunks = [DC.sweep_chunks(fv.super, fv.pi, batch, mb) for mb in (None, case["budget"])]
        want = DC.sweep_program(fv.super, fv.pi, batch, case["budget"] if with_budget else None)[1]
        book.check("selinv" if first else "budget_bits", f"launches {si_launches}, the program's {want}", int(si_launches != want), 0)
        book.check("factor_grad" if first else "budget_bits", f"launches {fg_launches}, the program's {want} + 1", int(fg_launches != want + 1), 0)
        if not first:
            _done(S, A, Lf)
            return Zx, Gx, si_launches, fg_launches, chunks
        nrhs = case["nrhs"][1]
        Pm, Qm = rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, n))
        S.factor_outer_grad_device(A, Lf, _dev(Pm), _dev(Qm), alpha=-1.0)
        Go = S.factor_grad_host(Lf)
        _guard(S)
        ref, mask = F.trapezoid_of(F.dense_factor_grad(Lref, -np.tril(Pm.T @ Qm)), fv.super, fv.pi, fv.px, fv.s, fv.xsize)
        err, dead = _grad_compare(Go, ref, mask)
        book.check("outer_grad", f"Gx against the dense formula, nrhs {nrhs}", err, R.tolerance(R.factor_rcond(fv)))
        book.check("outer_grad", "dead triangles of Gx, bits", dead, 0)
        # 7b. the Schur complements and the condensed solves, for the m of device_fuzz_corpus.schur_ms: after both backward
        # sweeps have used the plan, before the factor is replaced.  Their random inputs come from a generator of their own.
        rng7 = DC.schur_rng(case)
        ms = DC.case_ms(case, fv, rng7)
        Mp = _permuted(Ad, fv)
        sc = _check_schur(book, S, Lf, fv, Mp, ms, n)
        _check_condensed(book, S, Lf, fv, Ad, Mp, sc, ms, case["nrhs"], rng7)
        # 8. new values from the device and another beta: the old values scaled per row and column, as
        # selinv_cases.case_stale does; both sweeps' results are stale, then those of the new matrix
        scale = 1.0 + 0.5 * rng.uniform(size=n)
        Ax2 = Ax * scale[Ai] * scale[GR.columns_of(Ap)]
        ok2 = S.factorize_device(A, _dev(Ax2), Lf, case["beta2"]) == 1 and S.cm.status == ch.OK and int(Lf.contents.minor) == n
        _guard(S)
        book.check("factorize_device", f"status {S.cm.status} minor {int(Lf.contents.minor)}", 0 if ok2 else 1, 0)
        if ok2:
            book.check("factorize_device", "selinv_info [6]", _info(S, Lf, "selinv")[6], 0)
            book.check("factorize_device", "factor_grad_info [6]", _info(S, Lf, "factor_grad")[6], 0)
            fv = _host_factor(S, Lf)
            Lref2 = np.linalg.cholesky(_permuted(R.dense_symmetric(n, Ap, Ai, Ax2, case["beta2"]), fv))
            _check_factor(book, "factorize_device", fv, Lref2)
            if case["case"] % 2 == 0:
                _check_selinv(book, "factorize_device", S, A, Lf, fv, case, Ax2, case["beta2"])
            else:
                _check_factor_grad(book, "factorize_device", S, A, Lf, fv, Lref2, 2000 + case["case"])
                # ... and one Schur complement again: that of the new matrix, not the one formed before
                m = ms[0]
                new = S.schur_device(Lf, m).cpu().numpy()
                _guard(S)
                ref = SR.dense_schur(_permuted(R.dense_symmetric(n, Ap, Ai, Ax2, case["beta2"]), fv), m)
                book.check("schur", f"Sc m {m} of the new values", np.abs(new - ref).max() / np.abs(ref).max(),
                           R.tolerance(R.factor_rcond(fv)))
                book.check("schur", f"Sc m {m} of the new values is the old one", int(np.array_equal(new, sc[m][0])), 0)
        _done(S, A, Lf)
        return Zx, Gx, si_launches, fg_launches, chunks
    finally:
        os.environ.pop(BUDGET, None)


def budget_case(book, case, got):
    """9. a second Session on the same case without the budget: Zx and Gx bit for bit; strictly more launches under the budget
    wherever it cuts a batch of the plan into more chunks (device_fuzz_corpus.sweep_chunks), the same number elsewhere (a
    budget cuts nothing where no batch holds two generic fronts; tests/test_device_fuzz_corpus.py asks for three cases it cuts)"""
    free = real_case(book, case, with_budget=False)
    if free is None:
        return
    book.check("budget_bits", "Zx, bits", np.count_nonzero(_bits(got[0]) != _bits(free[0])), 0)
    book.check("budget_bits", "Gx, bits", np.count_nonzero(_bits(got[1]) != _bits(free[1])), 0)
    c0, cb = got[4]
    book.check("budget_bits", "the chunks from both plans", int(got[4] != free[4]), 0)
    for name, k in (("selinv", 2), ("factor_grad", 3)):
        wrong = not (got[k] > free[k]) if cb > c0 else got[k] != free[k]
        book.check("budget_bits", f"{name} launches {free[k]} -> {got[k]} with chunks {c0} -> {cb}", int(wrong), 0)


def complex_case(book, case):
    """all nine systems against dense references at the bars of solve_device_complex_cases._check_systems (TOL per column
    for the triangular systems, TOL_RES for the residual of A x = b, P / Pt / D bit for bit), the residual at 1e-11
    relative to |B|, one refinement step"""
    n, Ap, Ai, Ax, beta = case["n"], case["Ap"], case["Ai"], case["Ax"], case["beta"]
    feat = "complex_arrow" if case["leaves"] else "complex_solve"
    if case["twin"]:
        os.environ["CHOLMOD_HIP_CX_TWIN"] = "1"
    else:
        os.environ.pop("CHOLMOD_HIP_CX_TWIN", None)
    try:
        rng = np.random.default_rng(case["rhs_seed"])
        S, A, Lf, ok = DC.factorized(case, use_gpu=1)
        _guard(S)
        if not ok or Lf.contents.xtype != ch.COMPLEX:
            book.check(feat, f"factorize: status {S.cm.status} minor {int(Lf.contents.minor)}", 1, 0)
            _done(S, A, Lf)
            return
        twin = C.cast(Lf.contents.cx_twin, C.POINTER(ch.Factor)).contents.hip_is_twin
        book.check(feat, f"the storage asked for (hip_is_twin {twin})", int(twin != (1 if case["twin"] else 2)), 0)
        fv = _host_factor(S, Lf)
        Md = CX.full_hermitian(n, Ap, Ai, Ax).toarray() + beta * np.eye(n)
        P = np.asarray(fv.Perm)
        Mp = Md[np.ix_(P, P)]
        Lref = np.linalg.cholesky(Mp)
        book.check(feat, "L", np.linalg.norm(CX.dense_L(fv, fv.x) - Lref) / np.linalg.norm(Lref), TOL_L)
        if case["leaves"]:
            dead, imag = _check_by_supernode(book, feat, fv, Lref)
            book.check(feat, "dead triangles of L", dead, 0)
            book.check(feat, "imaginary parts of the diagonal of L", imag, 0)
        for nrhs in case["nrhs"]:
            b = CX._rhs(rng, nrhs, n)
            B = _dev(b)
            lower = sla.solve_triangular(Lref, b.T, lower=True).T
            upper = sla.solve_triangular(Lref, b.T, lower=True, trans="C").T
            ipb = np.empty_like(b)
            ipb[:, P] = b
            for name, sys_, ref in (("L", ch.SYS_L, lower), ("LD", ch.SYS_LD, lower), ("Lt", ch.SYS_Lt, upper), ("DLt", ch.SYS_DLt, upper)):
                x = S.solve_device(Lf, B, sys_).cpu().numpy()
                book.check(feat, f"{name} nrhs {nrhs}", CX._relcols(x, ref), CX.TOL)
            for name, sys_, Mx in (("A", ch.SYS_A, Md), ("LDLt", ch.SYS_LDLt, Mp)):       # (LDLt: L L' x = b, no permutation)
                x = S.solve_device(Lf, B, sys_).cpu().numpy()
                r = (Mx @ x.T).T - b
                book.check(feat, f"{name} nrhs {nrhs}, residual",
                           max(np.linalg.norm(r[k]) / np.linalg.norm(b[k]) for k in range(nrhs)), CX.TOL_RES)
            for name, sys_, ref in (("P", ch.SYS_P, b[:, P]), ("Pt", ch.SYS_Pt, ipb), ("D", ch.SYS_D, b)):
                x = S.solve_device(Lf, B, sys_).cpu().numpy()
                book.check(feat, f"{name} nrhs {nrhs}, entries that differ", np.count_nonzero(x != ref), 0)
            _guard(S)
            x0 = CX._rhs(rng, nrhs, n)
            r = S.residual_device(Lf, _dev(x0), B).cpu().numpy()
            ref = b - (Md @ x0.T).T
            book.check(feat, f"residual nrhs {nrhs}",
                       max(np.linalg.norm(r[k] - ref[k]) / np.linalg.norm(b[k]) for k in range(nrhs)), 1e-11)
        xs = S.solve_device(Lf, B).cpu().numpy()
        xp = xs * (1.0 + 1e-6 * CX._rhs(rng, len(b), n))
        X = _dev(xp)
        S.refine_device(Lf, B, X, steps=1)
        x1 = X.cpu().numpy()
        _guard(S)
        after = max(np.linalg.norm(b[k] - Md @ x1[k]) / np.linalg.norm(b[k]) for k in range(len(b)))
        book.check(feat, "one refinement step", after, TOL_REFINE)
        _done(S, A, Lf)
    finally:
        os.environ.pop("CHOLMOD_HIP_CX_TWIN", None)


def aat_case(book, case):
    """loss = (W . chol.solve (v, B)).sum () + 0.3 chol.logdet (v) through DeviceCholesky with a tensor beta, nrhs 1 and one
    drawn, against aat_grad_reference.torch_reference at aat_grad_reference.bars (as aat_grad_cases.case_autograd), and
    aat_logdet_grad_device against the same reference with W = 0 (the loss is 0.3 log det M then)"""
    M, beta = case["M"], case["beta"]
    m, a = M.shape[0], M.data.copy()
    S, A, Lf, ok = DC.factorized(case, use_gpu=1)
    _guard(S)
    if not ok:
        book.check("aat", f"factorize: status {S.cm.status} minor {int(Lf.contents.minor)}", 1, 0)
        _done(S, A, Lf)
        return
    fv = _host_factor(S, Lf)
    tol = R.tolerance(R.factor_rcond(fv))
    bt = torch.tensor(beta, dtype=torch.float64, device="cuda", requires_grad=True)
    chol = DeviceCholesky(S, A, Lf, bt)
    for nrhs in sorted({1, max(case["nrhs"])}):
        B, W = GR.inputs(m, nrhs, case["rhs_seed"] % 1000 + nrhs)
        ref = AR.torch_reference(M, a, beta, B, W)
        bars = AR.bars(M, a, ref, tol, nrhs)
        v, Bd, Wd = _dev(a).requires_grad_(), _dev(B).requires_grad_(), _dev(W)
        ld = chol.logdet(v)
        X = chol.solve(v, Bd)
        ((Wd * X).sum() + 0.3 * ld).backward()
        torch.cuda.synchronize()
        _guard(S)
        book.check("aat", f"X nrhs {nrhs}", np.abs(X.detach().cpu().numpy() - ref["X"]).max(), tol * ref["x_max"])
        book.check("aat", f"logdet nrhs {nrhs}", abs(float(ld) - ref["logdet"]), TOL_LOGDET * ref["logdet_scale"])
        book.check("aat", f"grad_values nrhs {nrhs}", np.abs(v.grad.cpu().numpy() - ref["grad_values"]).max(), bars[0])
        book.check("aat", f"grad_B nrhs {nrhs}", np.abs(Bd.grad.cpu().numpy() - ref["grad_B"]).max(), bars[1])
        book.check("aat", f"grad_beta nrhs {nrhs}", abs(float(bt.grad) - ref["grad_beta"]), bars[2])
        bt.grad = None
    B1 = GR.inputs(m, 1, 5)[0]
    ref = AR.torch_reference(M, a, beta, B1, np.zeros_like(B1))
    g = S.aat_logdet_grad_device(A, Lf, _dev(a)).cpu().numpy()
    _guard(S)
    book.check("aat", "aat_logdet_grad_device", np.abs(g - ref["grad_values"] / 0.3).max(), AR.bars(M, a, ref, tol, 1)[0] / 0.3)
    # the Schur complement of the A A' + beta I factor, for the edge draw of device_fuzz_corpus.schur_ms (the factor is the
    # one the calls above left: of the same values and beta)
    fv = _host_factor(S, Lf)
    _check_schur(book, S, Lf, fv, _permuted((M @ M.T).toarray() + beta * np.eye(m), fv), DC.case_ms(case, fv)[:1], m)
    _done(S, A, Lf)


def main():
    seed, ncase = int(sys.argv[1]), int(sys.argv[2])
    book = Book()
    torch.cuda.init()
    try:
        for case in DC.corpus(seed, ncase):
            book.case = case
            print(DC.describe(case), flush=True)
            if case["kind"] == "complex":
                complex_case(book, case)
            elif case["kind"] == "aat":
                aat_case(book, case)
            else:
                got = real_case(book, case)
                if got is not None and case["budget"]:
                    budget_case(book, case, got)
            torch.cuda.synchronize()
    except (RuntimeError, HipError):
        traceback.print_exc()
        print(f"HIP ERROR in {DC.describe(book.case)}: the run ends here", flush=True)
        print("RESULT " + json.dumps(book.result()))
        sys.stdout.flush()
        os._exit(EXIT_HIP_ERROR)
    print("RESULT " + json.dumps(book.result()))
    print(f"device fuzz: {ncase} cases, {len(book.failed_cases)} failures (seed {seed})")


if __name__ == "__main__":
    main()
