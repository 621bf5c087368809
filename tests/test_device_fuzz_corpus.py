"""The corpus of the device fuzz (tests/device_fuzz_corpus.py) through the product's CPU path, over exactly the seeds and
case counts tests/test_gpu_device_fuzz.py runs: the conditions under which the GPU checks mean what they say.

  * every case factorizes with status OK and minor == n: the corpus holds no case a GPU check could skip;
  * every dispatch class of the two backward sweeps and of the device solves (device_fuzz_corpus.CLASSES) is reached by
    at least 3 real symmetric cases; the classes the thirteen hand-drawn selinv_reference.CASES reach are printed beside
    the histogram (reported, not asserted: that line documents the gap);
  * rcond >= 1e-3 on every real symmetric case, so the bar max (1e-12, 20 eps / rcond) stays within 1e-12 .. 5e-12;
  * on every real symmetric case the numpy restatements of the two recurrences (selinv_reference, factor_grad_reference)
    stay within 0.1 x bar of the dense inverse and of the dense formula: the references leave the kernels nine tenths of
    the bar;
  * a block arrow has exactly the supernodes that were asked for;
  * about one real symmetric case in three runs under a scratch budget, and the budget cuts a batch in at least 3."""
import numpy as np
import pytest

import device_fuzz_corpus as DC
import factor_grad_reference as F
import selinv_reference as R
from suitesparse_amd import cholmod as ch

_measured = {}


def _measure():
    """one pass over the corpus, shared by the tests of this file"""
    if _measured:
        return _measured
    rows = []
    for seed in DC.SEEDS:
        for case in DC.corpus(seed, DC.NCASE):
            S, A, Lf, ok = DC.factorized(case, use_gpu=0)
            fv = ch.FactorView(Lf)
            row = dict(seed=seed, case=case["case"], kind=case["kind"], n=case["n"], ok=ok, status=S.cm.status, tag=DC.describe(case))
            if ok and case["kind"] in DC.REAL_KINDS:
                n, beta = case["n"], case["beta"]
                row["classes"] = DC.front_classes(fv.super, fv.pi, fv.s)
                row["fronts"] = [(int(fv.super[k + 1] - fv.super[k]), int(fv.pi[k + 1] - fv.pi[k])) for k in range(fv.nsuper)]
                row["leaves"] = case["leaves"]
                batch = DC.plan_batches(S, Lf, case["hip_flags"])
                row["budget"] = case["budget"]
                row["chunks"] = [DC.sweep_chunks(fv.super, fv.pi, batch, mb) for mb in (None, case["budget"])]
                row["rcond"] = R.factor_rcond(fv)
                tol = R.tolerance(row["rcond"])
                # the selected inverse: the restated recurrence against the dense inverse
                Zx = R.selinv_reference(fv.super, fv.pi, fv.px, fv.s, fv.x)
                err, tol2, dead = R.compare(fv, Zx, n, case["Ap"], case["Ai"], case["Ax"], beta)
                assert tol2 == tol and dead == 0
                row["selinv"] = err / tol
                # the factor gradient: the restated recurrence against the dense formula
                Lbar_x, _ = F.random_lbar(fv, 1000 * seed + case["case"], dead=1e30)
                Gx = F.factor_grad_reference(fv.super, fv.pi, fv.px, fv.s, fv.x, Lbar_x)
                Ad = R.dense_symmetric(n, case["Ap"], case["Ai"], case["Ax"], beta)
                p = np.asarray(fv.Perm)
                Gd = F.dense_factor_grad(np.linalg.cholesky(Ad[np.ix_(p, p)]), F.dense_of_layout(fv, Lbar_x))
                ref, mask = F.trapezoid_of(Gd, fv.super, fv.pi, fv.px, fv.s, fv.xsize)
                row["factor_grad"] = float(np.abs(Gx[mask] - ref[mask]).max() / np.abs(ref[mask]).max()) / tol
            rows.append(row)
            S.free_factor(Lf)
            S.free_sparse(A)
            S.finish()
    _measured["rows"] = rows
    return _measured


def test_every_case_factorizes():
    bad = [r["tag"] + f" status {r['status']}" for r in _measure()["rows"] if not r["ok"]]
    assert not bad, bad
    kinds = {r["kind"] for r in _measure()["rows"]}
    assert kinds == set(DC.KINDS)


def test_every_dispatch_class_is_reached_by_three_cases():
    rows = [r for r in _measure()["rows"] if "classes" in r]
    hist = {c: sum(c in r["classes"] for r in rows) for c in DC.CLASSES}
    table = set()
    for name in sorted(R.CASES):
        S, A, Lf = R.factorized(R.CASES[name](), use_gpu=0)
        fv = ch.FactorView(Lf)
        table |= DC.front_classes(fv.super, fv.pi, fv.s)
        S.free_factor(Lf)
        S.free_sparse(A)
        S.finish()
    print(f"classes reached, cases of {len(rows)} real symmetric ones:")
    for c in DC.CLASSES:
        print(f"  {c:18s} {hist[c]:3d}   {'also in' if c in table else 'NOT in'} the hand-drawn table")
    print("classes the thirteen selinv_reference.CASES do not reach:", sorted(set(DC.CLASSES) - table))
    assert all(set(r["classes"]) <= set(DC.CLASSES) for r in rows)
    few = {c: k for c, k in hist.items() if k < 3}
    assert not few, few


def test_block_arrows_have_the_supernodes_asked_for():
    rows = [r for r in _measure()["rows"] if r["kind"] == "arrow"]
    assert rows
    for r in rows:
        want = [(w, w + b) for w, b in r["leaves"]] + [(DC.ARROW_ROOT, DC.ARROW_ROOT)]
        assert r["fronts"][-1] == want[-1] and sorted(r["fronts"]) == sorted(want), (r["tag"], r["fronts"], want)    # (the postorder moves leaves)
    # the edges of is_thin: 64 + 72 = SM_MAX stays thin, 64 + 73 and 65 + 71 do not
    assert DC.front_classes([0, 64, 204], [0, 136, 276], np.r_[0:64, 132:204, 64:204]) >= {"thin_w64", "thin_r136", "thin_lds2"}
    assert "gen_tall_narrow" in DC.front_classes([0, 64, 204], [0, 137, 277], np.r_[0:64, 131:204, 64:204])
    assert "gen_w65" in DC.front_classes([0, 65, 205], [0, 136, 276], np.r_[0:65, 134:205, 65:205])


def test_scratch_budgets_cut_batches():
    """about one real case in three has a scratch budget, and at least 3 of them have a batch the budget cuts into more
    chunks (from a schedule-only plan: device_fuzz_corpus.sweep_chunks): there the GPU run must show strictly more launches"""
    rows = [r for r in _measure()["rows"] if "chunks" in r]
    with_budget = [r for r in rows if r["budget"]]
    cut = [r for r in with_budget if r["chunks"][1] > r["chunks"][0]]
    print(f"{len(with_budget)} of {len(rows)} real symmetric cases have a budget; it cuts {len(cut)}: "
          + ", ".join(f"seed {r['seed']} case {r['case']} ({r['chunks'][0]} -> {r['chunks'][1]} chunks)" for r in cut))
    assert len(rows) / 5 <= len(with_budget) <= len(rows) / 2
    assert len(cut) >= 3
    assert all(r["chunks"][1] >= r["chunks"][0] for r in rows)


def test_the_bar_stays_at_1e_12():
    rows = [r for r in _measure()["rows"] if "rcond" in r]
    worst = min(rows, key=lambda r: r["rcond"])
    print(f"smallest rcond {worst['rcond']:.3e} ({worst['tag']}, seed {worst['seed']})")
    assert worst["rcond"] >= 1e-3, worst["tag"]
    assert all(1e-12 <= R.tolerance(r["rcond"]) <= 5e-12 for r in rows)


@pytest.mark.parametrize("which", ["selinv", "factor_grad"])
def test_the_references_leave_nine_tenths_of_the_bar(which):
    rows = [r for r in _measure()["rows"] if which in r]
    worst = max(rows, key=lambda r: r[which])
    print(f"{which}: worst restatement error / bar = {worst[which]:.4f} ({worst['tag']}, seed {worst['seed']}) over {len(rows)} cases")
    assert len(rows) == sum(r["kind"] in DC.REAL_KINDS for r in _measure()["rows"])
    assert worst[which] <= 0.1, worst["tag"]
