"""The bodies of tests/test_gpu_nonfinite.py, run in a process of their own: `python nonfinite_device_cases.py BODY
[ARG ...]`, torch imported FIRST (see solve_device_cases.py).  Exit status 0 = every assertion held; a line `RESULT <json>`
carries the set sizes back.  Session, value upload and factor download are those of tests/not_posdef_device_cases.py.

A case of tests/nonfinite_cases.py (one NaN or Inf in the matrix, perhaps a planted pivot) goes through one plan in this
order:

    first       the FIRST factorization of the plan, with the poisoned values
    good        the clean values, values-only: the plan's clean factor.  Every later good factor is THESE BITS
    mapped      the poisoned values, values-only (a launch of small leaves runs k_leaf_pair, two fronts to a wave)
    good
    device      the poisoned values from a device tensor (Session.factorize_device; real cases), then the good ones

After every poisoned factorization: status and minor as the table derives them; must <= non-finite entries <= may; every
supernode outside may the bits of the plan's clean factor (+0.0 after a failing supernode); the dead upper triangles zero;
the finite entries against the oracle's at TOL_L.  The three poisoned factors are the same bits, as int64 (NaN != NaN).
A good factorization that is not the clean bits is a cache that was not refreshed: info, the first-failure word, dinv, Winv."""
import torch  # noqa: E402  (first)

import ctypes as C
import json
import os
import sys

import numpy as np

import nonfinite_cases as NF
import not_posdef_cases as NP
import not_posdef_device_cases as D
from suitesparse_amd import cholmod as ch

SYS = {"A": ch.SYS_A, "L": ch.SYS_L, "Lt": ch.SYS_Lt}


def _poisoned(c, st, S, Lf, rc, device, tag):
    want = NF.sets(c)["minor"]
    failed = want < st.n
    assert rc == 1 and S.cm.status == (ch.NOT_POSDEF if failed else ch.OK), (tag, rc, S.cm.status, "a NaN pivot does not trip")
    S.cm.status = ch.OK
    minor = int(Lf.contents.minor)
    assert minor == want, (tag, "minor", minor, "expected", want)
    return D._x(S, Lf, device)


def _good(c, st, S, Lf, rc, device, tag, clean=None):
    assert rc == 1 and S.cm.status == ch.OK, (tag, rc, S.cm.status)
    assert int(Lf.contents.minor) == st.n, (tag, int(Lf.contents.minor))
    x = D._x(S, Lf, device)
    if clean is None:
        e = NP.check_factor(st, x, NF.clean_oracle(c.key), f"{tag} against the oracle")
        print(f"{tag}: the plan's clean factor, by entry {e:.2e} against the oracle")
        assert e < NF.TOL_L, (tag, e)
    else:
        same = NF.bits(x) == NF.bits(clean)
        assert same.all(), (tag, f"not the clean bits: {int((~same).sum())} words differ, {int((~np.isfinite(x)).sum())} non-finite")
    return x


def run_case(c):
    M, st = NP.matrix(c.key), NP.structure(c.key)
    bad, good = NF.poisoned_values(c), M["Ax"]
    os.environ.update(c.env)                    # (read when the plan is made; this process runs one group)
    S = D._session(c)
    A = S.sparse(M["n"], M["Ap"], M["Ai"], bad, -1)
    Lf = S.analyze(A, M["perm"])
    fv = ch.FactorView(Lf)
    for k in ("Perm", "super", "pi", "px", "s"):
        assert np.array_equal(getattr(fv, k), getattr(st, k)), (c.name, k)
    x1 = _poisoned(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} first")
    if c.storage:
        T = C.cast(Lf.contents.cx_twin, C.POINTER(ch.Factor))
        assert Lf.contents.xtype == ch.COMPLEX and T.contents.hip_is_twin == (2 if c.storage == "cx" else 1)
    else:
        assert Lf.contents.hip_plan and Lf.contents.hip_on_device == 1
    if c.group == "twokernel":
        kinds = set(S.launch_profile(Lf)["kind"].tolist())
        assert {NP.K_DIAG, NP.K_ROWSOLVE} <= kinds and NP.K_CHAINF not in kinds, kinds
    D._set(A, good)
    clean = _good(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} good after first")
    r = NF.check_contract(c, x1, clean, f"{c.name} first", oracle_x=NF.oracle_expectation(c)[3])
    print(f"{c.name}: minor {NF.sets(c)['minor']}, must {r['must']} <= device {r['nonfinite']} <= may {r['may']}")
    D._set(A, bad)
    x2 = _poisoned(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} mapped")
    NF.check_contract(c, x2, clean, f"{c.name} mapped", oracle_x=NF.oracle_expectation(c)[3])
    assert np.array_equal(NF.bits(x1), NF.bits(x2)), (c.name, "first and mapped differ", int((NF.bits(x1) != NF.bits(x2)).sum()))
    D._set(A, good)
    _good(c, st, S, Lf, S.factorize(A, Lf), False, f"{c.name} good after mapped", clean)
    if not c.storage:
        bd, gd = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (bad, good))
        D._set(A, np.full(len(good), 0.5))                                       # (the host values are not read)
        x3 = _poisoned(c, st, S, Lf, S.factorize_device(A, bd, Lf), True, f"{c.name} device")
        NF.check_contract(c, x3, clean, f"{c.name} device", oracle_x=NF.oracle_expectation(c)[3])
        assert np.array_equal(NF.bits(x1), NF.bits(x3)), (c.name, "first and device differ", int((NF.bits(x1) != NF.bits(x3)).sum()))
        _good(c, st, S, Lf, S.factorize_device(A, gd, Lf), True, f"{c.name} good after device", clean)
        torch.cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    assert S.cm.malloc_count == 0, S.cm.malloc_count
    S.finish()
    for k in c.env:
        del os.environ[k]
    return r


def body_group(group, flags, storage="-"):
    """every case of the group under these flags (and this storage)"""
    cases = NF.cases_of(group, flags=flags, storage=None if storage == "-" else storage)
    assert cases
    worst = None
    for c in cases:
        r = run_case(c)
        # the worst case of the group: the one whose device set is farthest above must
        if worst is None or r["nonfinite"] - r["must"] >= worst["nonfinite"] - worst["must"]:
            worst = dict(r, name=c.name)
    print("RESULT " + json.dumps(dict(cases=len(cases), worst=worst)))


# ---- the resident calls --------------------------------------------------------------------------------------------------

def _same(tag, got, clean, rows, repro):
    """the rows `rows` of one or several right-hand sides (the last axis is the row): the bits of the clean call where that
    is reproducible (NF.reproducible_rows), elsewhere finite and within 2 TOL_SOLVE of it in norm -- each call is within
    TOL_SOLVE of the exact solution (tests/solve_device_cases.py)"""
    got, clean = np.atleast_2d(got), np.atleast_2d(clean)
    exact, loose = rows & repro, rows & ~repro
    same = NF.bits(got[:, exact]) == NF.bits(clean[:, exact])
    assert same.all(), (tag, f"{int((~same).sum())} words of the reproducible rows are not the clean bits")
    if loose.any():
        assert np.isfinite(got[:, loose]).all(), (tag, "non-finite where nothing poisoned was read")
        for q in range(len(got)):
            e = float(np.linalg.norm(got[q, loose] - clean[q, loose]) / np.linalg.norm(clean[q, loose]))
            assert e <= 2 * D.TOL_SOLVE, (tag, q, "against the clean call", e)


def _rows_check(tag, got, clean, must, may, repro):
    """one right-hand side: must <= NaN rows <= may, the rows outside may those of the clean call (_same)"""
    got, clean = got.reshape(-1), clean.reshape(-1)
    nan = np.isnan(got)
    assert not (must & ~nan).any(), (tag, "must-rows finite", np.flatnonzero(must & ~nan)[:5])
    assert not (nan & ~may).any(), (tag, "NaN outside may", np.flatnonzero(nan & ~may)[:5])
    _same(tag, got, clean, ~may, repro)
    return int(nan.sum())


def _diag_index(st):
    return np.concatenate([st.px[k] + np.arange(st.nscol[k]) * (st.nsrow[k] + 1) for k in range(st.nsuper)])


def body_resident():
    """the factor checks, the solves and the residual around a NaN factor of "deep" (flags 0, the factor kept in HBM)"""
    c, c2 = NF.resident_case((129, 136), 64), NF.resident_case((16, 0), 3)
    M, st = NP.matrix(c.key), NP.structure(c.key)
    n = st.n
    S = D._session(c)
    S.cm.hip_factor_on_device = 1
    A = S.sparse(n, M["Ap"], M["Ai"], M["Ax"], -1)
    Lf = S.analyze(A, M["perm"])
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    rng = np.random.default_rng(43)
    b = rng.standard_normal((17, n))
    Bd = torch.from_numpy(b).cuda()
    NRHS = (1, 3, 16, 17)
    host0 = {k: np.atleast_2d(S.solve(Lf, b[:k])) for k in NRHS}
    dev0 = {(k, s): S.solve_device(Lf, Bd[:k], SYS[s]).cpu().numpy() for k in NRHS for s in SYS}
    counts = {}
    repro = {s: NF.reproducible_rows(c.key, s) for s in SYS}
    every = np.ones(n, dtype=bool)
    own = NF.rows_of_columns(c.key, np.arange(st.super[st.front((16, 0))], st.super[st.front((16, 0)) + 1]))
    assert repro["Lt"].all() and sorted(np.flatnonzero(repro["A"])) == sorted(own) and repro["L"].sum() == n - 140

    # -- a NaN in one row of one right-hand side, on the clean factor
    col_of_L = 200
    assert st.supernode_of(col_of_L) == st.front((129, 136))
    for nrhs, cols in ((17, (5, 16)), (3, (1,))):
        for s in SYS:
            row = int(NF.rows_of_columns(c.key, [col_of_L])[0]) if s == "A" else col_of_L
            must, may = NF.solve_sets(c.key, [row], s)
            assert 0 < must.sum() <= may.sum() < n
            for q in cols:
                Bn = Bd[:nrhs].clone()
                Bn[q, row] = float("nan")
                X = S.solve_device(Lf, Bn, SYS[s]).cpu().numpy()
                cnt = _rows_check(f"solve_device SYS_{s} nrhs {nrhs} column {q}", X[q], dev0[nrhs, s][q], must, may, repro[s])
                others = [k for k in range(nrhs) if k != q]
                _same(f"solve_device SYS_{s} nrhs {nrhs}, the columns other than {q}", X[others], dev0[nrhs, s][others], every, repro[s])
                counts[f"rhs SYS_{s} nrhs {nrhs} col {q}"] = (int(must.sum()), cnt, int(may.sum()))

    # -- the residual with clean A and X NaN in one row of one column
    Xd = torch.from_numpy(rng.standard_normal((17, n))).cuda()
    for nrhs, q, row in ((3, 1, 200), (16, 7, 0), (17, 16, 300), (17, 3, n - 1)):
        R0, n0 = S.residual_device(Lf, Xd[:nrhs], Bd[:nrhs], norms=True)
        Xn = Xd[:nrhs].clone()
        Xn[q, row] = float("nan")
        R1, n1 = S.residual_device(Lf, Xn, Bd[:nrhs], norms=True)
        R0, n0, R1, n1 = (t.cpu().numpy() for t in (R0, n0, R1, n1))
        rows = NF.residual_rows(c.key, row)
        assert 0 < rows.sum() < n
        assert np.array_equal(np.isnan(R1[q]), rows), (nrhs, q, row, "NaN rows", int(np.isnan(R1[q]).sum()), int(rows.sum()))
        assert np.array_equal(NF.bits(R1[q][~rows]), NF.bits(R0[q][~rows]))
        assert np.isnan(n1[q]), (nrhs, q, "the norm of a column with a NaN", n1[q])
        others = [k for k in range(nrhs) if k != q]
        assert np.array_equal(NF.bits(R1[others]), NF.bits(R0[others])) and np.array_equal(NF.bits(n1[others]), NF.bits(n0[others]))
        counts[f"residual nrhs {nrhs} col {q} row {row}"] = (int(rows.sum()), int(np.isnan(R1[q]).sum()), int(rows.sum()))

    # -- the NaN factor: the checks that read the resident factor
    diag = _diag_index(st)
    for case, nan_rows in ((c, 421), (c2, 16)):
        D._set(A, NF.poisoned_values(case))
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK and int(Lf.contents.minor) == n
        S0 = NF.sets(case)
        f = Lf.contents
        assert f.hip_on_device and not f.hip_host_valid        # (the values live in HBM only: rcond takes the device path)
        if case is c:
            rc = S.L.cholmod_l_rcond(Lf, C.byref(S.cm))
            assert rc == 0.0 and S.cm.status == ch.OK, ("rcond of a factor with a NaN diagonal", rc)
            out = np.zeros(3)
            assert S.L.cholmod_hip_diag_minmax(f.hip_plan, out.ctypes.data) == 0
            chk = S.factor_checks(Lf)
            dmust, dmay = int(S0["must"][diag].sum()), int(S0["may"][diag].sum())
            print(f"NaN factor: diag_minmax {out}, checks {chk}; diagonal must {dmust} may {dmay}, entries must "
                  f"{int(S0['must'].sum())} may {int(S0['may'].sum())}")
            assert 0 < dmust <= int(out[2]) <= dmay < n, (out, dmust, dmay)
            assert dmust <= chk["nonpositive_diag"] <= dmay, (chk, dmust, dmay)
            assert 0 < int(S0["must"].sum()) <= chk["nonfinite"] <= int(S0["may"].sum()), chk
            assert chk["upper_nonzeros"] == 0
            # include/cholmod_hip.h: dOut [0] = 2 sum_j log L_jj, over ALL n diagonal entries (only cholmod_hip_factor_checks
            # leaves the entries that are not > 0 out); minor == n, so nothing refuses.  log (NaN) is NaN and so is the sum
            ld = float(S.logdet_device(Lf))
            assert np.isnan(ld), ld
            counts["factor_checks nonfinite"] = (int(S0["must"].sum()), chk["nonfinite"], int(S0["may"].sum()))
            counts["diag_minmax out[2]"] = (dmust, int(out[2]), dmay)
        # the rows of A behind the columns of L that hold a NaN: their whole trees are NaN, the other tree the clean bits
        cols = np.flatnonzero(S0["must"][diag])
        must, may = NF.solve_sets(case.key, NF.rows_of_columns(case.key, cols), "A")
        assert must.sum() == nan_rows and np.array_equal(must, may)
        for nrhs in NRHS:
            X = S.solve_device(Lf, Bd[:nrhs]).cpu().numpy()
            for q in range(nrhs):
                assert _rows_check(f"solve_device on the NaN factor, nrhs {nrhs} column {q}", X[q], dev0[nrhs, "A"][q], must, may, repro["A"]) == nan_rows
        for nrhs in NRHS:
            X = np.atleast_2d(S.solve(Lf, b[:nrhs]))
            for q in range(nrhs):
                assert _rows_check(f"solve on the NaN factor, nrhs {nrhs} column {q}", X[q], host0[nrhs][q], must, may, repro["A"]) == nan_rows
        # -- the recovery: the clean bits everywhere, under every system
        D._set(A, M["Ax"])
        assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK and int(Lf.contents.minor) == n
        for nrhs in NRHS:
            for s in SYS:
                X = S.solve_device(Lf, Bd[:nrhs], SYS[s]).cpu().numpy()
                _same(f"solve_device after the recovery, SYS_{s} nrhs {nrhs}", X, dev0[nrhs, s], every, repro[s])
            X = np.atleast_2d(S.solve(Lf, b[:nrhs]))
            _same(f"solve after the recovery, nrhs {nrhs}", X, host0[nrhs], every, repro["A"])
        assert S.L.cholmod_l_rcond(Lf, C.byref(S.cm)) > 0
        assert np.isfinite(float(S.logdet_device(Lf)))
    torch.cuda.synchronize()
    S.free_factor(Lf)
    S.free_sparse(A)
    S.finish()
    for k, v in counts.items():
        print(f"{k}: must {v[0]} <= device {v[1]} <= may {v[2]}")
    print("RESULT " + json.dumps(dict(cases=2, worst=counts)))


if __name__ == "__main__":
    torch.cuda.init()
    globals()["body_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK")
