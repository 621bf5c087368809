"""The table of tests/nonfinite_cases.py (NaN and Inf in the matrix, the right-hand sides and the iterate) pinned on the
CPU, before any GPU sees it:

  * for every case the oracle's status and minor are what the table derives from the must set; its non-finite entries lie
    between must and may; its supernodes outside may are the bits of its own clean run;
  * every must set is non-empty and every may set leaves a supernode out (a case that poisons everything proves nothing)
    -- except the cases whose point is that nothing is NaN;
  * the same table through the product's CPU path (use_gpu=0, cpu_numeric.c) under the same contract, its finite entries
    against the oracle's at TOL_L, and the clean values in the same factor afterwards;
  * every poisoned front is factorized by the kernel the case names, under the case's flags;
  * the row sets of the solves and the residual, on the oracle's solves and the CPU path's."""
import numpy as np
import pytest

import nonfinite_cases as NF
import not_posdef_cases as NP
from suitesparse_amd import cholmod as ch

REFS = list({c.ref_key: c for c in NF.table()}.values())
NOTHING_IS_NAN = [c for c in REFS if NF.sets(c)["untouched"]]


def _id(c):
    return c.name.replace(":", "-")


def test_the_table_holds_what_it_is_meant_to():
    groups = {g: len(NF.cases_of(g)) for g in NF.GROUPS}
    print(f"{len(NF.table())} cases, {len(REFS)} distinct references: {groups}")
    assert groups == dict(leafdiag=20, twokernel=1, offdiag=4, sharedlaunch=12, mixed=10, levels=1, complex=4, inf=2)
    assert sum(groups.values()) == len(NF.table()) <= 70
    assert all(NP.structure(c.key).n <= 576 for c in NF.table())
    assert {c.flags for c in NF.cases_of("leafdiag")} == set(NF.DEEP_FLAGS)
    assert {c.flags for c in NF.cases_of("sharedlaunch")} == set(NF.THIN_FLAGS)
    assert {c.quick for c in NF.cases_of("mixed")} == {False, True}
    assert {c.storage for c in NF.cases_of("complex")} == {"cx", "twin"}
    assert [c.name for c in NOTHING_IS_NAN] == [c.name for c in REFS if "129x136@64:plant-7.0129x136@10" in c.name]
    # one NaN, +Inf or -Inf per case; the weak contract is the +Inf group and only it
    for c in NF.table():
        assert len(c.P) == 1 and c.weak == (c.group == "inf") == (c.P[0][3] == "+inf")
        v = NF.poisoned_values(c)
        bad = np.flatnonzero(~np.isfinite(v))
        assert len(bad) == 1 + (c.plant_value == NF.NINF), (c.name, bad)
    # the wave pairs of k_leaf_pair are the supernodes 0 | 1 and 2 | 3: each member in turn
    assert sorted(c.fronts[0] for c in NF.cases_of("sharedlaunch", flags=0, key="pair")) == [0, 1, 2, 3]


def test_the_mixed_cases_trip_where_they_should():
    st = NP.structure("deep")
    n, leaf, early, root = st.n, st.front((129, 136)), st.front((65, 71)), st.nsuper - 1
    assert early < leaf < root
    want = {"65x71@32:plant-7.0129x136@0": int(st.super[leaf]),         # the plant; the earlier NaN leaf keeps its values
            "129x136@64:plant-7.0129x136@10": int(st.super[leaf]) + 10,  # the plant comes first: nothing anywhere is NaN
            "129x136@64:plant-7.0140x0@2": int(st.super[root]) + 2,      # no leaf reaches root column 2
            "129x136@64:plant-7.0140x0@70": n,                           # the NaN reaches root column 70: it does not trip
            "65x71@32:plant-inf129x136@0": int(st.super[leaf])}          # -inf <= 0 trips
    seen = set()
    for c in NF.cases_of("mixed"):
        (tag,) = [t for t in want if f":{t}:" in c.name]
        seen.add(tag)
        S = NF.sets(c)
        assert S["minor"] == want[tag], (c.name, S["minor"])
        if "@10" in tag:
            assert not S["must"].any()
        elif want[tag] == int(st.super[leaf]):
            # the NaN leaf is before the failing supernode and stays as it is
            assert S["sbad"] == leaf and S["must"][st.px[early]:st.px[early + 1]].any()
        # after the failure nothing is in may, on the path or not: the tail of the failing supernode and every later one
        if S["minor"] < n:
            sb = S["sbad"]
            assert S["zero"][st.px[sb + 1]:][st.mask[st.px[sb + 1]:]].all() and not (S["zero"] & (S["may"] | S["must"])).any()
            assert S["zero"].sum() == (st.mask[st.px[sb]:].sum() - (st.mask[st.px[sb]:st.px[sb] + (S["valid"] - st.super[sb]) * st.nsrow[sb]]).sum())
            assert S["on_path"][root] and S["zero"][st.px[root]:][st.mask[st.px[root]:]].all() or sb == root
        else:
            assert not S["zero"].any()
    assert seen == set(want)
    # the leaf (129, 136) hangs on root column 140 - 136 = 4: column 2 is not reached, column 70 is
    rows = st.s[st.pi[leaf]:st.pi[leaf + 1]]
    assert rows[129] == st.super[root] + 4 and len(rows) == 129 + 136


@pytest.mark.parametrize("c", REFS, ids=_id)
def test_oracle_lies_between_must_and_may(c):
    st, S = NP.structure(c.key), NF.sets(c)
    rc, status, minor, x = NF.oracle_expectation(c)
    failed = S["minor"] < st.n
    assert (rc, status, minor) == ((1, ch.NOT_POSDEF, S["minor"]) if failed else (0, ch.OK, st.n)), (rc, status, minor, S["minor"])
    r = NF.check_contract(c, x, NF.clean_oracle(c.key), f"oracle {c.name}", dead=False)
    print(f"{c.name}: minor {minor}, must {r['must']} <= oracle {r['nonfinite']} <= may {r['may']}; "
          f"{int(S['on_path'].sum())} of {st.nsuper} supernodes on the path")
    # a condition on the case, not a measurement
    assert not S["on_path"].all()
    if c in NOTHING_IS_NAN:
        assert r["nonfinite"] == 0 and r["must"] == 0
    elif not c.weak:
        assert r["must"] > 0
    else:
        assert r["nonfinite"] >= 1                      # (the oracle: L (j, j) = +inf and zeros below it)


def test_the_oracle_shows_exactly_the_must_set_on_an_arrow():
    """deep, NaN at (129, 136)@64: the leaf NaN in exactly the lower parts of its columns 64 .. 128, the root in exactly
    the lower triangle from column 4 on; Poisson: 5 of 49 supernodes poisoned; +Inf: one inf, no NaN"""
    c = next(c for c in NF.cases_of("leafdiag", flags=0) if "129x136@64" in c.name)
    st = NP.structure("deep")
    x = NF.oracle_expectation(c)[3]
    leaf, root = st.front((129, 136)), st.nsuper - 1
    nf = ~np.isfinite(x) & st.mask
    L = nf[st.px[leaf]:st.px[leaf + 1]].reshape(129, 265)
    assert not L[:64].any() and all(L[j, j:].all() for j in range(64, 129))
    R = nf[st.px[root]:st.px[root + 1]].reshape(140, 140)
    assert not R[:4].any() and all(R[j, j:].all() for j in range(4, 140))
    assert nf.sum() == L.sum() + R.sum() == NF.sets(c)["must"].sum()
    (c,) = NF.cases_of("levels")
    st, S = NP.structure("poisson"), NF.sets(c)
    x = NF.oracle_expectation(c)[3]
    hit = np.add.reduceat((~np.isfinite(x)).astype(np.int64), st.px[:-1]) > 0
    assert st.nsuper == 49 and hit.sum() == 5 and np.array_equal(hit, S["on_path"])
    x = NF.oracle_expectation(NF.cases_of("inf", flags=0)[0])[3]
    assert np.isinf(x).sum() == 1 and not np.isnan(x).any()


def _cpu_session(c):
    S = ch.Session(use_gpu=0)
    S.cm.error_handler = ch.ERRFUNC(0)
    S.cm.quick_return_if_not_posdef = int(c.quick)
    if NP.matrix(c.key)["norelax"]:
        for k in range(3):
            S.cm.nrelax[k] = 0
            S.cm.zrelax[k] = 0.0
    return S


@pytest.mark.parametrize("c", REFS, ids=_id)
def test_cpu_path_keeps_the_contract(c):
    """cpu_numeric.c: clean, poisoned, clean again in one factor"""
    M, st, S0 = NP.matrix(c.key), NP.structure(c.key), NF.sets(c)
    S = _cpu_session(c)
    A = S.sparse(M["n"], M["Ap"], M["Ai"], M["Ax"], -1)
    Lf = S.analyze(A, M["perm"])
    fv = ch.FactorView(Lf)
    for k in ("Perm", "super", "pi", "px", "s"):
        assert np.array_equal(getattr(fv, k), getattr(st, k)), k
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    clean = ch.FactorView(Lf).x.copy()
    assert NP.check_factor(st, clean, NF.clean_oracle(c.key), f"CPU path, clean {c.name}") < NF.TOL_L
    B = S.sparse(M["n"], M["Ap"], M["Ai"], NF.poisoned_values(c), -1)
    failed = S0["minor"] < st.n
    assert S.factorize(B, Lf) == 1 and S.cm.status == (ch.NOT_POSDEF if failed else ch.OK)
    S.cm.status = ch.OK
    fv = ch.FactorView(Lf)
    assert fv.minor == S0["minor"], (fv.minor, S0["minor"])
    r = NF.check_contract(c, fv.x, clean, f"CPU path {c.name}", oracle_x=NF.oracle_expectation(c)[3])
    print(f"{c.name}: must {r['must']} <= CPU path {r['nonfinite']} <= may {r['may']}")
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    fv = ch.FactorView(Lf)
    assert fv.minor == st.n and np.array_equal(NF.bits(fv.x), NF.bits(clean)), "the clean factor after the poisoned one"
    S.free_factor(Lf)
    S.free_sparse(A)
    S.free_sparse(B)
    assert S.cm.malloc_count == 0
    S.finish()


def test_every_poisoned_front_meets_the_kernel_it_is_named_for(monkeypatch):
    reached = {}
    for c in NF.table():
        if c.storage:
            continue        # (a complex factor is scheduled on its twin's structure)
        got = NP.factor_kernel(c.key, c.flags, c.fronts[0])
        assert c.kernel == got, (c.name, c.kernel, got)
        reached.setdefault(got, set()).add(c.group)
    print("the kernel that meets the poisoned pivot:", {k: sorted(v) for k, v in sorted(reached.items())})
    assert set(reached) == {"generic", "thin4", "thin1", "thin1+pair"}
    # what "generic" is under each of the deep flags: the fused 64-column chain, launches of their own, the 256-column
    # chain (k_chainf and nothing else), no thin-front kernel at all
    kinds = {f: NP.launch_kinds("deep", f) for f in NF.DEEP_FLAGS}
    dense = {NP.K_POTRF, NP.K_TRSM, NP.K_TRSM_UPD, NP.K_UPD_PF}
    assert NP.K_TRSM_UPD in kinds[0] and NP.K_SMALL in kinds[0]
    assert {NP.K_POTRF, NP.K_TRSM} <= kinds[512 | 1024] and not {NP.K_TRSM_UPD, NP.K_UPD_PF} & kinds[512 | 1024]
    assert NP.K_CHAINF in kinds[8192] and not (dense | {NP.K_DIAG, NP.K_ROWSOLVE}) & kinds[8192]
    assert NP.K_SMALL not in kinds[16]
    # CHOLMOD_HIP_NO_CHAINF: k_diag + k_rowsolve take the place of k_chainf (the variable is read when the plan is made)
    (c,) = NF.cases_of("twokernel")
    assert c.flags == 8192 and c.env == {"CHOLMOD_HIP_NO_CHAINF": "1"}
    monkeypatch.setenv("CHOLMOD_HIP_NO_CHAINF", "1")
    two = set(k for k, _, _ in NP.launch_profile.__wrapped__("deep", 8192)[0])
    monkeypatch.delenv("CHOLMOD_HIP_NO_CHAINF")
    assert {NP.K_DIAG, NP.K_ROWSOLVE} <= two and not (dense | {NP.K_CHAINF}) & two
    # the shared launches: ONE thin launch holds all four leaves of "thin" (136 rows: four waves per front) and of "pair"
    # (32 rows, 16 columns: k_leaf_pair, two fronts to a wave, on the values-only paths under flags 0)
    for f in NF.THIN_FLAGS:
        (ln,) = NP.thin_launches("thin", f)
        assert ln["members"] == [0, 1, 2, 3] and ln["aux"] == 136
        (ln,) = NP.thin_launches("pair", f)
        assert ln["members"] == [0, 1, 2, 3] and ln["aux"] <= 32 and ln["pair"] == (f == 0)
    (c,) = NF.cases_of("levels")
    assert NP.structure("poisson").level[c.fronts[0]] == 0


# ---- solves and residual -----------------------------------------------------------------------------------------------

SOLVE_COL = 200             # a column of L in leaf (129, 136) of "deep"; SYS_A: the row of A that stands for it


def test_solve_sets_on_the_oracle():
    st = NP.structure("deep")
    n = st.n
    parent, root_of = NF.etree("deep")
    own = st.front((16, 0))
    assert set(np.unique(root_of)) == {n - 1, int(st.super[own + 1]) - 1}          # two trees: leaf (16, 0) and the rest
    assert (root_of != n - 1).sum() == 16
    assert st.supernode_of(SOLVE_COL) == st.front((129, 136))
    O = NP.new_oracle("deep")
    assert O.factorize(NP.matrix("deep")["Ax"]) == 0
    rng = np.random.default_rng(7)
    b = rng.standard_normal(n)
    for sys, fn in (("A", O.solve), ("L", O.lsolve), ("Lt", O.ltsolve)):
        row = int(NF.rows_of_columns("deep", [SOLVE_COL])[0]) if sys == "A" else SOLVE_COL
        bn = b.copy()
        bn[row] = np.nan
        x, xn = fn(b), fn(bn)
        must, may = NF.solve_sets("deep", [row], sys)
        nanrows = np.isnan(xn)
        print(f"SYS_{sys}: must {must.sum()} <= oracle {nanrows.sum()} <= may {may.sum()} of {n}")
        assert not (must & ~nanrows).any() and not (nanrows & ~may).any()
        assert np.array_equal(NF.bits(xn[~may]), NF.bits(x[~may]))
        assert 0 < must.sum() and may.sum() < n
    # a solve on the NaN factor: 421 rows NaN, the 16 of leaf (16, 0) the clean bits -- and the reverse
    x = O.solve(b)
    for front, col, nan_rows in (((129, 136), 64, 421), ((16, 0), 3, 16)):
        c = NF.resident_case(front, col)
        On = NP.new_oracle("deep")
        assert On.factorize(NF.poisoned_values(c)) == 0
        xn = On.solve(b)
        must, may = NF.solve_sets("deep", NF.rows_of_columns("deep", [int(st.super[c.fronts[0]]) + col]), "A")
        assert must.sum() == nan_rows and np.array_equal(np.isnan(xn), must)
        assert np.array_equal(NF.bits(xn[~must]), NF.bits(x[~must]))


def test_solve_sets_on_the_cpu_path():
    c = NF.resident_case()
    M, st = NP.matrix("deep"), NP.structure("deep")
    n = st.n
    S = _cpu_session(c)
    A = S.sparse(n, M["Ap"], M["Ai"], M["Ax"], -1)
    Lf = S.analyze(A, M["perm"])
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
    rng = np.random.default_rng(7)
    b = rng.standard_normal((3, n))
    for sys, code in (("A", ch.SYS_A), ("L", ch.SYS_L), ("Lt", ch.SYS_Lt)):
        row = int(NF.rows_of_columns("deep", [SOLVE_COL])[0]) if sys == "A" else SOLVE_COL
        bn = b.copy()
        bn[1, row] = np.nan
        x, xn = S.solve(Lf, b, code), S.solve(Lf, bn, code)
        must, may = NF.solve_sets("deep", [row], sys)
        nanrows = np.isnan(xn[1])
        assert not (must & ~nanrows).any() and not (nanrows & ~may).any()
        assert np.array_equal(NF.bits(xn[1][~may]), NF.bits(x[1][~may]))
        assert np.array_equal(NF.bits(xn[[0, 2]]), NF.bits(x[[0, 2]]))
    x = S.solve(Lf, b)
    B = S.sparse(n, M["Ap"], M["Ai"], NF.poisoned_values(c), -1)
    assert S.factorize(B, Lf) == 1 and S.cm.status == ch.OK
    xn = S.solve(Lf, b)
    must, _ = NF.solve_sets("deep", NF.rows_of_columns("deep", [int(st.super[c.fronts[0]]) + 64]), "A")
    assert must.sum() == 421 and all(np.array_equal(np.isnan(xn[k]), must) for k in range(3))
    assert np.array_equal(NF.bits(xn[:, ~must]), NF.bits(x[:, ~must]))
    S.free_factor(Lf)
    S.free_sparse(A)
    S.free_sparse(B)
    S.finish()


def test_residual_rows_against_a_dense_product():
    M = NP.matrix("deep")
    n = M["n"]
    st = NP.structure("deep")
    Ad = np.empty((n, n))
    Ad[np.ix_(st.Perm, st.Perm)] = NP.dense_permuted("deep", M["Ax"])   # A itself
    rng = np.random.default_rng(8)
    X = rng.standard_normal(n)
    for k in (0, 200, 300, n - 1):
        Xn = X.copy()
        Xn[k] = np.nan
        rows = NF.residual_rows("deep", k)
        # row j of A X reads X (k) exactly when A (j, k) is stored: a dense product would read it everywhere (0 * NaN)
        want = (Ad[:, k] != 0)
        want[k] = True
        assert np.array_equal(rows, want) and 0 < rows.sum() < n
