"""The bodies of tests/test_gpu_not_posdef.py, run in a process of their own: `python not_posdef_device_cases.py BODY
[ARG ...]`, torch imported FIRST (see solve_device_cases.py).  Exit status 0 = every assertion held; a line `RESULT <json>`
carries the worst by-entry figure back.

A case of tests/not_posdef_cases.py (several planted pivots) goes through one plan in this order:

    first       the FIRST factorization of the plan, with the planted values (k_assemble, the thin fronts record the map;
                small leaves run the one-wave k_thin_front)
    good        the positive definite values, values-only: the map a FAILED factorization recorded, the info array and
                the first-failure word of a factorization that failed in several supernodes
    mapped      the planted values, values-only (k_assemble_mapped; a launch of small leaves runs k_leaf_pair, two
                fronts to a wave: the "pair" group and the Poisson leaves)
    good        as above
    device      the planted values from a device tensor (Session.factorize_device; real cases), then the good ones

After every failed factorization: return value 1, status NOT_POSDEF, minor == min (K); the zero pattern over the lower
trapezoids exactly the references', the dead upper triangles zero; the values by entry below TOL_L against the oracle AND
against the dense restatement.  The three failed factors are the same BITS: the first factorization and the mapped path
assemble one value per entry of L and every kernel sums in a fixed order (profiles/heads_bit_identity.log), and
factorize_device gives the resident S the same values (tests/factorize_device_cases.py).  After every good one: status OK,
minor == n, the factor below TOL_L against the oracle.

What each part catches (tried on mutated builds of the engine): k_first_fail taking the largest reporting supernode gives
the larger planted column as minor in every case with two failing supernodes; first_zero = sbad + 1 whatever info and quick
leaves the valid columns of the failing supernode in place under quick return (the cases with info == 1 and no quick return
do not see it: the front kernels zero a front from its failing column on by themselves); an info array that is not cleared
turns the first good factorization after a failed one into NOT_POSDEF."""
import torch  # noqa: E402  (first)

import ctypes as C
import json
import os
import sys

import numpy as np

import not_posdef_cases as NP
from suitesparse_amd import cholmod as ch

TOL_SOLVE = 1e-11           # per right-hand side (tests/solve_device_cases.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _session(c):
    if c.storage == "twin":
        os.environ["CHOLMOD_HIP_CX_TWIN"] = "1"
    else:
        os.environ.pop("CHOLMOD_HIP_CX_TWIN", None)
    S = ch.Session(hip_flags=c.flags)
    S.cm.error_handler = ch.ERRFUNC(0)
    S.cm.quick_return_if_not_posdef = int(c.quick)
    if NP.matrix(c.key)["norelax"]:
        for k in range(3):
            S.cm.nrelax[k] = 0
            S.cm.zrelax[k] = 0.0
    return S


def _set(A, Ax):
    v = np.ascontiguousarray(Ax).view(np.float64)
    ch._view(A.contents.x, len(v), C.c_double, np.float64)[:] = v


def _x(S, Lf, device):
    if device:
        assert S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm)) == 1
    return ch.FactorView(Lf).x.copy()


def _failed(c, st, S, Lf, rc, device, tag):
    """the checks after a factorization of the planted values -> (x, worst by-entry figure)"""
    assert rc == 1 and S.cm.status == ch.NOT_POSDEF, (tag, rc, S.cm.status)            # TRUE, as the reference
    S.cm.status = ch.OK
    minor = int(Lf.contents.minor)
    assert minor == c.minor, (tag, "minor", minor, "expected", c.minor, "planted", c.K)
    x = _x(S, Lf, device)
    orc, ost, ominor, xo = NP.oracle_expectation(*c.ref_key)
    assert (orc, ost, ominor) == (1, ch.NOT_POSDEF, c.minor)
    eo = NP.check_factor(st, x, xo, f"{tag} against the oracle")
    ed = NP.check_factor(st, x, NP.dense_expectation(*c.ref_key)[1], f"{tag} against the dense restatement")
    print(f"{tag}: minor {minor}, by entry {eo:.2e} (oracle) {ed:.2e} (dense)")
    assert eo < NP.TOL_L and ed < NP.TOL_L, (tag, eo, ed)
    return x, max(eo, ed)


def _good(c, st, S, Lf, rc, device, tag):
    assert rc == 1 and S.cm.status == ch.OK, (tag, rc, S.cm.status)
    assert int(Lf.contents.minor) == st.n, (tag, int(Lf.contents.minor))
    e = NP.check_factor(st, _x(S, Lf, device), NP.oracle_expectation(c.key, (), False)[3], f"{tag} against the oracle")
    print(f"{tag}: positive definite again, by entry {e:.2e}")
    assert e < NP.TOL_L, (tag, e)
    return e


def run_case(c):
    M, st = NP.matrix(c.key), NP.structure(c.key)
    bad, good = NP.planted_values(c.key, c.K), M["Ax"]
    S = _session(c)
    A = S.sparse(M["n"], M["Ap"], M["Ai"], bad, -1)
    Lf = S.analyze(A, M["perm"])
    fv = ch.FactorView(Lf)
    for k in ("Perm", "super", "pi", "px", "s"):
        assert np.array_equal(getattr(fv, k), getattr(st, k)), (c.name, k)
    x1, worst = _failed(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} first")
    if c.storage:
        T = C.cast(Lf.contents.cx_twin, C.POINTER(ch.Factor))
        assert Lf.contents.xtype == ch.COMPLEX and T.contents.hip_is_twin == (2 if c.storage == "cx" else 1)
    else:
        assert Lf.contents.hip_plan and Lf.contents.hip_on_device == 1
    if c.group == "levels":
        sparent, level = np.empty(st.nsuper, dtype=np.int64), np.empty(st.nsuper, dtype=np.int64)
        assert S.L.cholmod_hip_get_maps(fv.hip_plan, sparent.ctypes.data, level.ctypes.data, None) == 0
        assert np.array_equal(sparent, st.sparent) and np.array_equal(level, st.level)
        assert level[c.fronts[0]] >= 2 and level[c.fronts[1]] == 0 and c.sbad == c.fronts[0]
    _set(A, good)
    worst = max(worst, _good(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} good after first"))
    _set(A, bad)
    x2, e = _failed(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} mapped")
    worst = max(worst, e)
    assert np.array_equal(_bits(x1), _bits(x2)), (c.name, "first and mapped differ", float(np.abs(x1 - x2).max()))
    _set(A, good)
    worst = max(worst, _good(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} good after mapped"))
    if not c.storage:
        bd, gd = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (bad, good))
        _set(A, np.full(len(good), np.nan))                                      # (the host values are not read)
        x3, e = _failed(c, st, S, Lf, S.factorize_device(A, bd, Lf), True, f"{c.name} device")
        worst = max(worst, e)
        assert np.array_equal(_bits(x1), _bits(x3)), (c.name, "first and device differ", float(np.abs(x1 - x3).max()))
        worst = max(worst, _good(c, st, S, Lf, S.factorize_device(A, gd, Lf), True, f"{c.name} good after device"))
        torch.cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    assert S.cm.malloc_count == 0, S.cm.malloc_count
    S.finish()
    return worst


def body_group(group, flags, storage="-"):
    """every case of the group under these flags (and this storage), both values of quick_return_if_not_posdef"""
    cases = NP.cases_of(group, flags=flags, storage=None if storage == "-" else storage)
    assert cases and {c.quick for c in cases} == {False, True}
    worst = 0.0
    for c in cases:
        worst = max(worst, run_case(c))
    print("RESULT " + json.dumps(dict(cases=len(cases), worst=worst)))


def body_resident():
    """the device-resident calls around a factorization that failed in two leaves and the root.  That the selected inverse
    and the log-determinant REFUSE a failed factor is tests/selinv_cases.py (case_refusals) and tests/grad_cases.py
    (case_logdet) already; cholmod_l_hip_solve_device documents no refusal for L->minor < n (include/cholmod.h).  Here:
    after the recovery none of them sees anything of the failed factorization -- solve_device gives the solution, the
    log-determinant and the diagonal of the selected inverse are the dense ones."""
    import selinv_reference as R
    c = next(c for c in NP.cases_of("two", quick=0) if len(c.K) == 3)
    M, st = NP.matrix(c.key), NP.structure(c.key)
    n = st.n
    S = _session(c)
    A = S.sparse(n, M["Ap"], M["Ai"], M["Ax"], -1)
    Lf = S.analyze(A, M["perm"])
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    Ad = R.dense_symmetric(n, M["Ap"], M["Ai"], M["Ax"])
    b = np.random.default_rng(41).standard_normal((3, n))
    xs = np.linalg.solve(Ad, b.T).T
    Bd = torch.from_numpy(b).cuda()
    Ld = np.linalg.cholesky(Ad[np.ix_(st.Perm, st.Perm)])
    logdet = 2.0 * float(np.log(np.diag(Ld)).sum())
    zdiag = np.diag(np.linalg.inv(Ad))
    _, d0 = S.selinv_device(A, Lf, values=False)                                  # (a resident inverse to go stale)
    bad = torch.from_numpy(NP.planted_values(c.key, c.K)).cuda()
    good = torch.from_numpy(np.ascontiguousarray(M["Ax"])).cuda()
    for how in ("host", "device"):
        if how == "host":
            _set(A, NP.planted_values(c.key, c.K))
            rc = S.factorize(A, Lf)
        else:
            rc = S.factorize_device(A, bad, Lf)
        assert rc == 1 and S.cm.status == ch.NOT_POSDEF and int(Lf.contents.minor) == c.minor
        S.cm.status = ch.OK
        if how == "host":
            _set(A, M["Ax"])
            rc = S.factorize(A, Lf)
        else:
            rc = S.factorize_device(A, good, Lf)
        assert rc == 1 and S.cm.status == ch.OK and int(Lf.contents.minor) == n
        X = S.solve_device(Lf, Bd).cpu().numpy()
        e = max(np.linalg.norm(X[k] - xs[k]) / np.linalg.norm(xs[k]) for k in range(len(xs)))
        # the log-determinant: n terms 2 log L_jj, every L_jj within the factor's bar TOL_L of the exact one
        ld = float(S.logdet_device(Lf))
        _, d = S.selinv_device(A, Lf, values=False)
        assert S.L.cholmod_l_factor_to_host(Lf, C.byref(S.cm)) == 1
        tol = R.tolerance(R.factor_rcond(ch.FactorView(Lf)))
        ez = float(np.abs(d.cpu().numpy() - zdiag).max() / np.abs(zdiag).max())
        print(f"resident, recovery through the {how}: solve {e:.2e}, logdet {ld!r} dense {logdet!r}, diag (Z) {ez:.2e} (bar {tol:.1e})")
        assert e < TOL_SOLVE, e
        assert abs(ld - logdet) <= 2 * n * NP.TOL_L, (ld, logdet)
        assert ez <= tol, (ez, tol)
        assert torch.equal(d, d0)                                                  # (the same factor, the same bits)
    torch.cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()
    print("RESULT " + json.dumps(dict(cases=1, worst=0.0)))


def body_dense(flags):
    """cholmod_hip_dense_partial_factor on the (200, 100) front of scaling_cases.dense_reference with the decoupled bad
    column of test_gpu_pivot_range.test_dense_front_zero_and_negative_denormal_pivots at 15, 64 and 99: rows 100 .. 199 of
    the columns BEFORE it.  What the probe promises there: its header (include/cholmod_hip.h) speaks of success only, but
    the probe runs the engine's own launches (engine.hip, cholmod_hip_dense_partial_factor: run_launch over
    schedule_dense), and the engine's protocol leaves the failing supernode as those launches left it (first_zero =
    sbad + 1 without quick return): k_trsm_mfma and its kin solve the info - 1 valid columns through every row (nvalid,
    kernels.hip.h and chain256_kernels.hip.h) and write zeros in the others.  So those rows are
    Fb [100:, :col] inv (chol (Fb [:col, :col]))', by entry at TOL_L."""
    import scaling_cases as SC
    flags = int(flags)
    L = ch.lib()
    assert L.cholmod_hip_probe() == 1, "no HIP device visible"
    Fm = SC.dense_reference(200, 100)[0]
    nsrow, nscol = 200, 100
    worst = 0.0
    for col in (15, 64, 99):
        Fb = Fm.copy()
        Fb[col, :] = 0.0
        Fb[:, col] = 0.0
        Fb[col, col] = NP.PLANT
        F = np.asfortranarray(Fb.copy())
        info = C.c_int64(-1)
        assert L.cholmod_hip_dense_partial_factor(F.ctypes.data, nsrow, nscol, flags, C.byref(info)) == 0
        assert info.value == col + 1, (flags, col, info.value)
        lead = np.linalg.cholesky(Fb[:col, :col])
        ref = Fb[nscol:, :col] @ np.linalg.inv(lead).T
        e = float(np.abs(F[nscol:, :col] - ref).max() / np.abs(ref).max())
        print(f"dense (200, 100) flags {flags} bad column {col}: rows 100 .. 199 of the valid columns, by entry {e:.2e}")
        assert e < NP.TOL_L, (flags, col, e)
        assert np.all(F[nscol:, col:nscol] == 0), (flags, col)
        worst = max(worst, e)
    print("RESULT " + json.dumps(dict(cases=3, worst=worst)))


if __name__ == "__main__":
    torch.cuda.init()
    globals()["body_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
