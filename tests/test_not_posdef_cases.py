"""The table of tests/not_posdef_cases.py (several failing pivots in one factorization) pinned on the CPU, before any GPU
sees it:

  * for every case the oracle returns not-positive-definite with minor == min (K);
  * the oracle's zero pattern is exactly the dense restatement's, and its values agree with it by entry within a TENTH of
    the bar TOL_L = 1e-12 (max |dL| over a supernode / max |L| of that supernode, the worst supernode): the references
    leave the device nine tenths of the bar.  The worst figure is printed;
  * the same table through the product's CPU path (use_gpu=0, cpu_numeric.c) against both references, at the bar;
  * every planted supernode has the shape class it is named for (device_fuzz_corpus.front_classes: the classes of the
    selected inverse's sweeps) AND is factorized by the kernel it is named for: the thin-front schedule is restated
    (not_posdef_cases.thin_launches) and held against the K_SMALL launches -- grid and aux -- of a schedule-only plan
    under the case's flags; the flags produce the launch kinds they are there for."""
import numpy as np
import pytest

import not_posdef_cases as NP
from suitesparse_amd import cholmod as ch

REFS = sorted({c.ref_key for c in NP.table()}, key=repr)


def test_the_table_holds_what_it_is_meant_to():
    groups = {g: len(NP.cases_of(g)) for g in ("two", "deep", "root", "thin", "pair", "levels", "complex")}
    print(f"{len(NP.table())} cases, {len(REFS)} distinct (matrix, plants, quick): {groups}")
    assert all(groups.values()) and sum(groups.values()) == len(NP.table())
    for c in NP.table():
        st = NP.structure(c.key)
        assert st.n <= 700 and c.minor == min(c.K) and len(set(c.fronts)) == len(c.fronts) >= 1
        assert c.group == "root" or len(c.fronts) >= 2               # several supernodes report
    # both quick values of everything
    assert {(c.key, c.K, c.flags, c.storage) for c in NP.table() if c.quick} == \
           {(c.key, c.K, c.flags, c.storage) for c in NP.table() if not c.quick}
    # a block arrow has exactly the supernodes asked for, the root last
    for key, leaves in NP.LEAVES.items():
        st = NP.structure(key)
        fronts = [(int(w), int(r)) for w, r in zip(st.nscol, st.nsrow)]
        assert fronts[-1] == (140, 140) and sorted(fronts[:-1]) == sorted((w, w + r) for w, r in leaves), (key, fronts)
    # info == 1 in the first failing supernode, in a later one, and neither
    assert {c.info == 1 for c in NP.table()} == {True, False}
    # the later leaf of the deep cases really is later, and the root cases leave every leaf before the failure
    for c in NP.cases_of("deep"):
        assert c.fronts[1] > c.fronts[0] == c.sbad < NP.structure(c.key).nsuper - 1
    for c in NP.cases_of("root"):
        assert c.sbad == NP.structure(c.key).nsuper - 1


def test_levels_case_is_high_in_one_subtree_and_in_a_leaf_of_another():
    st = NP.structure("poisson")
    a, b = NP.poisson_pair(st)
    print(f"poisson2d ({NP.POISSON}): {st.nsuper} supernodes, {st.level.max() + 1} levels; a = {a} (level {st.level[a]}, columns "
          f"{st.super[a]} .. {st.super[a + 1] - 1}), b = {b} (level 0, column {st.super[b]})")
    assert st.level[a] >= 2 and st.level[b] == 0 and st.super[b] > st.super[a + 1]
    assert b not in set(int(p) for p in st.sparent)
    for c in NP.cases_of("levels"):
        assert c.K == (int(st.super[a]) + 1, int(st.super[b])) and c.sbad == a and c.info == 2


@pytest.mark.parametrize("ref", REFS, ids=lambda r: f"{r[0]}-{'.'.join(map(str, r[1]))}-{'quick' if r[2] else 'full'}")
def test_oracle_and_dense_restatement_agree(ref):
    key, K, quick = ref
    st = NP.structure(key)
    rc, status, minor, xo = NP.oracle_expectation(key, K, quick)
    assert rc == 1 and status == ch.NOT_POSDEF and minor == min(K), (rc, status, minor, min(K))
    m, xd = NP.dense_expectation(key, K, quick)
    assert m == minor
    e = NP.check_factor(st, xo, xd, f"oracle against dense {ref}", dead=False)
    assert e < 0.1 * NP.TOL_L, e
    # the columns after the valid ones ARE zero in the reference: the case can tell a zeroed tail from a kept one
    assert np.all(xd[st.px[NP.structure(key).supernode_of(minor) + 1]:] == 0)


def test_the_reference_pair_uses_a_tenth_of_the_bar():
    worst, where = 0.0, None
    for key, K, quick in REFS:
        e = NP.by_entry(NP.structure(key), NP.oracle_expectation(key, K, quick)[3], NP.dense_expectation(key, K, quick)[1])
        if e >= worst:
            worst, where = e, (key, K, quick)
    for key in sorted({r[0] for r in REFS}):                           # ... and the positive definite factors of the recovery
        rc, status, minor, xo = NP.oracle_expectation(key, (), False)
        assert rc == 0 and minor == NP.structure(key).n
        e = NP.check_factor(NP.structure(key), xo, NP.dense_expectation(key, (), False)[1], key, dead=False)
        if e >= worst:
            worst, where = e, (key, (), False)
    print(f"oracle against dense restatement, worst by-entry figure over {len(REFS)} references: {worst:.3e} = "
          f"{worst / NP.TOL_L:.4f} of the bar {NP.TOL_L:g} ({where})")
    assert worst < 0.1 * NP.TOL_L


@pytest.mark.parametrize("ref", REFS, ids=lambda r: f"{r[0]}-{'.'.join(map(str, r[1]))}-{'quick' if r[2] else 'full'}")
def test_cpu_path_follows_the_protocol(ref):
    """cpu_numeric.c on the same table: the failed factorization, then the positive definite values in the same factor"""
    key, K, quick = ref
    M, st = NP.matrix(key), NP.structure(key)
    S = ch.Session(use_gpu=0)
    S.cm.error_handler = ch.ERRFUNC(0)
    S.cm.quick_return_if_not_posdef = int(quick)
    if M["norelax"]:
        for k in range(3):
            S.cm.nrelax[k] = 0
            S.cm.zrelax[k] = 0.0
    A = S.sparse(M["n"], M["Ap"], M["Ai"], NP.planted_values(key, K), -1)
    Lf = S.analyze(A, M["perm"])
    fv = ch.FactorView(Lf)
    for k in ("Perm", "super", "pi", "px", "s"):
        assert np.array_equal(getattr(fv, k), getattr(st, k)), k
    assert S.factorize(A, Lf) == 1 and S.cm.status == ch.NOT_POSDEF          # TRUE, as the reference
    fv = ch.FactorView(Lf)
    assert fv.minor == min(K)
    for what, ref_x in (("oracle", NP.oracle_expectation(key, K, quick)[3]), ("dense", NP.dense_expectation(key, K, quick)[1])):
        e = NP.check_factor(st, fv.x, ref_x, f"CPU path against {what} {ref}")
        assert e < NP.TOL_L, (what, e)
    B = S.sparse(M["n"], M["Ap"], M["Ai"], M["Ax"], -1)
    S.cm.status = ch.OK
    assert S.factorize(B, Lf) == 1 and S.cm.status == ch.OK
    fv = ch.FactorView(Lf)
    assert fv.minor == st.n
    assert NP.check_factor(st, fv.x, NP.oracle_expectation(key, (), False)[3], f"CPU path, recovery {ref}") < NP.TOL_L
    S.free_factor(Lf)
    S.free_sparse(A)
    S.free_sparse(B)
    assert S.cm.malloc_count == 0
    S.finish()


def test_every_case_has_the_shape_class_it_is_named_for():
    reached = set()
    for c in NP.table():
        st = NP.structure(c.key)
        got = NP.front_classes_of(st, c.fronts[0])
        assert set(c.classes) <= got, (c.name, c.classes, got)
        for k in c.fronts:
            reached |= NP.front_classes_of(st, k)
    print("classes of the planted supernodes:", sorted(reached))
    # the deep plants fall in the first, second and third 64-column block of a generic front with rows below -- the
    # (65, 71) leaf is generic under CHOLMOD_HIP_NO_SMALL_FRONTS only, a four-wave thin front otherwise
    blocks = {(int(st_n), j // 64) for c in NP.cases_of("deep") if c.kernel == "generic" for st_n, j in
              [(NP.structure(c.key).nscol[c.fronts[0]], c.info - 1)]}
    assert blocks == {(129, 0), (129, 1), (129, 2), (65, 0), (65, 1)}, blocks
    for f in NP.DEEP_FLAGS:
        got = {(int(NP.structure(c.key).nscol[c.fronts[0]]), (c.info - 1) // 64) for c in NP.cases_of("deep", flags=f) if c.kernel == "generic"}
        assert got >= {(129, 0), (129, 1), (129, 2)} and ((65, 1) in got) == bool(f & NP.NO_SMALL_FRONTS), (f, got)
    for c in NP.cases_of("deep") + NP.cases_of("complex"):
        assert NP.structure(c.key).nsrow[c.sbad] > NP.structure(c.key).nscol[c.sbad]


def test_the_restated_thin_schedule_is_the_plans():
    """grid and aux of every K_SMALL launch, in schedule order, for every (matrix, flags) of the table"""
    for key, flags in sorted({(c.key, c.flags) for c in NP.table() if not c.storage}):
        mine = [(len(ln["members"]), ln["aux"]) for ln in NP.thin_launches(key, flags)]
        plan = [(g, a) for k, g, a in NP.launch_profile(key, flags)[0] if k == NP.K_SMALL]
        assert mine == plan, (key, flags, mine, plan)


def test_every_case_is_factorized_by_the_kernel_it_is_named_for():
    reached = {}
    for c in NP.table():
        if c.storage:
            continue        # (a complex factor is scheduled on its twin's structure; it never takes leaf pairs)
        got = [NP.factor_kernel(c.key, c.flags, k) for k in c.fronts]
        assert c.kernel == got[0], (c.name, c.kernel, got)
        reached.setdefault(got[0], set()).add(c.group)
    print("the kernel that meets the winning pivot:", {k: sorted(v) for k, v in sorted(reached.items())})
    assert set(reached) == {"generic", "thin4", "thin1", "thin1+pair"}
    # the leaf-pair arrow: ONE thin launch, of its four leaves, the widest of 32 rows and 16 columns -- k_leaf_pair on the
    # values-only paths under flag 0, the one-wave k_thin_front under CHOLMOD_HIP_NO_LEAF_PAIRS and on a first factorization
    st = NP.structure("pair")
    leaves = sorted(set(range(st.nsuper)) - set(int(p) for p in st.sparent))
    for f in NP.THIN_FLAGS:
        small = [(g, a) for k, g, a in NP.launch_profile("pair", f)[0] if k == NP.K_SMALL]
        (ln,) = NP.thin_launches("pair", f)
        assert small == [(4, 32)] and ln["members"] == leaves == [0, 1, 2, 3] and ln["aux"] <= 32
        assert st.nscol[leaves].max() <= 16 and ln["pair"] == (f == 0)
    for c in NP.cases_of("pair"):
        assert all(NP.factor_kernel(c.key, c.flags, k) == c.kernel for k in c.fronts)       # BOTH failing fronts
    # both failing fronts in one wave of k_leaf_pair (supernodes 0 | 1, 2 | 3), and in two
    waves = {tuple(sorted(k // 2 for k in c.fronts)) for c in NP.cases_of("pair", flags=0)}
    assert waves == {(0, 0), (1, 1), (0, 1)}, waves
    # the thin arrow of the issue: one launch of aux 136, four waves per front, flag 4096 or not
    for f in NP.THIN_FLAGS:
        assert [(g, a) for k, g, a in NP.launch_profile("thin", f)[0] if k == NP.K_SMALL] == [(4, 136)]
    # the Poisson leaf b fails inside a leaf-pair launch, a in a one-wave thin launch
    c = NP.cases_of("levels")[0]
    assert [NP.factor_kernel(c.key, 0, k) for k in c.fronts] == ["thin1", "thin1+pair"]


def test_the_flags_produce_the_launches_they_are_there_for():
    prof = {f: NP.launch_profile("deep", f)[0] for f in NP.DEEP_FLAGS}
    kinds = {f: set(k for k, _, _ in p) for f, p in prof.items()}
    print({f: sorted(k) for f, k in kinds.items()})
    dense = {NP.K_POTRF, NP.K_TRSM, NP.K_TRSM_UPD, NP.K_UPD_PF}
    assert NP.K_SMALL in kinds[0] and NP.K_TRSM_UPD in kinds[0]                         # thin fronts, the fused chain
    assert NP.K_SMALL not in kinds[16] and dense & kinds[16]                            # no thin-front kernel
    assert {NP.K_POTRF, NP.K_TRSM} <= kinds[512 | 1024] and not {NP.K_TRSM_UPD, NP.K_UPD_PF} & kinds[512 | 1024]
    # the 256-column chain: NO other factorization launch is left in the plan, so every generic front -- the planted
    # (129, 136) leaf, the later (5, 137) leaf, the root -- goes through it; one k_chainf per batch that has one
    assert NP.K_CHAINF in kinds[8192] and not (dense | {NP.K_DIAG, NP.K_ROWSOLVE}) & kinds[8192]
    assert sum(k == NP.K_CHAINF for k, _, _ in prof[8192]) == len(set(NP.launch_profile("deep", 8192)[1]))
    # 4 | 128 (128-wide tiles on big regions, 2048-column outer blocks): at these sizes there is no big region and no
    # front wider than an outer block -- the schedule is that of flags 0, launch by launch.  The cases stay in the table
    # as the flag set that was asked for; what they run is what flags 0 runs.
    assert prof[4 | 128] == prof[0]
