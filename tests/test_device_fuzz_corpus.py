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
  * about one real symmetric case in three runs under a scratch budget, and the budget cuts a batch in at least 3;
  * cases 0 .. 39 of both seeds are, by their digests, what they were before anything was appended to the corpus;
  * every class of k_schur_tile's walk (device_fuzz_corpus.SCHUR_CLASSES) is reached by at least 3 real symmetric cases with
    the m of device_fuzz_corpus.schur_ms, and every class of the twin-space fronts (CX_CLASSES) by at least 3 of the 12
    complex block arrows, which have exactly the supernodes asked for;
  * schur_reference.schur_restated stays within 0.1 x bar of the dense Schur complement on every (case, m), and the CPU
    path's complex factor within 0.1 x 1e-12 of numpy's, by supernode, on every complex arrow;
  * a tile-by-tile numpy restatement of k_schur_tile equals schur_restated to 1e-14, and three mutants of it -- the
    contraction one column short, c0 rounded down to a multiple of 4, an absent row fed from a listed one -- each exceed the
    bar of the GPU comparison on at least 3 (case, m): the corpus has the power to see such errors."""
import numpy as np
import pytest

import json
import os

import device_fuzz_corpus as DC
import factor_grad_reference as F
import schur_reference as SR
import selinv_reference as R
from suitesparse_amd import cholmod as ch

TOL_L = 1e-12           # device_fuzz_runner.TOL_L: L by supernode
MUTANTS = ("cend_early", "c0_floor4", "absent_nearest")
_measured = {}


def _schur_tiled(sup, pi, px, s, Lx, n, m, mutant=None):
    """k_schur_tile (schur_kernels.hip.h) restated tile by tile: one 64 x 64 accumulator per tile (I, J), I >= J, the walk
    over the trailing supernodes with its break and its two continues, c0 and cend of every panel, the local rows of the 64
    A rows and the 64 B rows looked up in the panel's row list, a row the list does not hold (or past n) fed as zeros, an
    entry at local row r of column k read only if r >= k; both triangles written from the accumulator.  mutant: one of
    MUTANTS -- the contraction ends one column early; c0 is rounded down to a multiple of 4; an absent row is fed from the
    nearest listed row (the one sc_lower_bound finds) instead of zeros."""
    sup, pi, px, s = (np.asarray(a) for a in (sup, pi, px, s))
    t0, nt, nsuper = n - m, (m + 63) // 64, len(sup) - 1
    Sc = np.zeros((m, m))
    s0 = int(np.searchsorted(sup, t0, side="right")) - 1
    panels = []
    for k in range(s0, nsuper):
        rows = s[pi[k]:pi[k + 1]]
        nscol, nsrow = int(sup[k + 1] - sup[k]), len(rows)
        P = np.array(Lx[px[k]:px[k] + nsrow * nscol]).reshape(nscol, nsrow).T
        P[:nscol] = np.tril(P[:nscol])                          # (kin && ia >= k) ? Pk [ia] : 0.0
        panels.append((int(sup[k]), nscol, nsrow, rows, P, np.searchsorted(rows, t0 + 64 * np.arange(nt + 1), side="left")))

    def operand(rows, nsrow, P, r0, c0, cend):
        g = r0 + np.arange(64)
        pos = np.minimum(np.searchsorted(rows, g, side="left"), nsrow - 1)
        held = (rows[pos] == g) & (g < n)
        if mutant == "absent_nearest":
            held = g < n
        return np.where(held[:, None], P[pos, c0:cend], 0.0)

    for J in range(nt):
        rJ = t0 + 64 * J
        for I in range(J, nt):
            rI = t0 + 64 * I
            acc = np.zeros((64, 64))
            for k1, nscol, nsrow, rows, P, bounds in panels:
                if k1 >= rJ + 64:
                    break
                c0 = max(0, t0 - k1)
                jlo, jhi = int(bounds[J]), int(bounds[J + 1])
                if jlo == jhi:
                    continue
                if bounds[I] == bounds[I + 1]:
                    continue
                cend = min(nscol, jhi)
                if mutant == "cend_early":
                    cend -= 1
                if mutant == "c0_floor4":
                    c0 -= c0 % 4
                if cend > c0:
                    acc += operand(rows, nsrow, P, rI, c0, cend) @ operand(rows, nsrow, P, rJ, c0, cend).T
            ni, nj = min(64, m - 64 * I), min(64, m - 64 * J)
            blk = acc[:ni, :nj] if I > J else np.tril(acc[:ni, :nj])
            Sc[64 * I:64 * I + ni, 64 * J:64 * J + nj] = blk
            if I > J:
                Sc[64 * J:64 * J + nj, 64 * I:64 * I + ni] = blk.T
            else:
                Sc[64 * I:64 * I + ni, 64 * J:64 * J + nj] += np.tril(blk, -1).T
    return Sc


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
            if ok and case["kind"] == "complex" and case["leaves"]:
                # a complex block arrow: its supernodes, their classes in twin space, L by supernode against numpy
                n = case["n"]
                row["leaves"], row["twin"] = case["leaves"], case["twin"]
                row["fronts"] = [(int(fv.super[k + 1] - fv.super[k]), int(fv.pi[k + 1] - fv.pi[k])) for k in range(fv.nsuper)]
                row["cx_classes"] = DC.cx_front_classes(fv.super, fv.pi)
                p = np.asarray(fv.Perm)
                Lref = np.linalg.cholesky(DC.dense_hermitian(n, case["Ap"], case["Ai"], case["Ax"], case["beta"])[np.ix_(p, p)])
                row["cx_L"], _, row["cx_dead"], row["cx_imag"] = DC.by_supernode(fv, fv.x, Lref)
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
                # the Schur complement for the m of the case: the classes of the tile kernel's walk, the panel restatement
                # against the dense Schur complement, the tile restatement against the panel one, the mutants of it
                fac = (fv.super, fv.pi, fv.px, fv.s, fv.x)
                row["schur"] = []
                for m in DC.case_ms(case, fv):
                    want = SR.dense_schur(Ad[np.ix_(p, p)], m)
                    scale = np.abs(want).max()
                    rest = SR.schur_restated(*fac, n, m)
                    rec = dict(m=m, classes=DC.schur_classes(fv.super, fv.pi, fv.s, n, m),
                               restated=float(np.abs(rest - want).max() / scale) / tol,
                               tiled=float(np.abs(_schur_tiled(*fac, n, m) - rest).max() / np.abs(rest).max()))
                    for name in MUTANTS:
                        rec[name] = float(np.abs(_schur_tiled(*fac, n, m, mutant=name) - want).max() / scale) / tol
                    row["schur"].append(rec)
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


def test_cases_0_to_39_are_those_of_the_golden_digests():
    """tests/golden/device_fuzz_corpus_digests.json holds device_fuzz_corpus.case_digest of cases 0 .. 39 of both seeds, taken
    before the complex block arrows and the Schur picks were added: nothing added since may draw from the corpus's generator"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_fuzz_corpus_digests.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(str(s) for s in DC.SEEDS)
    for seed in DC.SEEDS:
        got = [DC.case_digest(c) for c in DC.corpus(seed, DC.NCASE)]
        assert len(got) == DC.NCASE == DC.NBASE + DC.NCX_ARROW and len(golden[str(seed)]) == DC.NBASE == 40
        differ = [k for k in range(DC.NBASE) if got[k] != golden[str(seed)][k]]
        assert not differ, (seed, differ)
        assert [DC.case_digest(c) for c in DC.corpus(seed, DC.NBASE)] == got[:DC.NBASE]


def test_schur_ms_is_what_the_corpus_promises():
    """at most 4 values and n for every eighth case, each within 1 .. n; the edge draw first"""
    for r in (r for r in _measure()["rows"] if "schur" in r):
        ms = [x["m"] for x in r["schur"]]
        assert 1 <= len(ms) <= 4 + (r["case"] % 8 == 0) and len(set(ms)) == len(ms), (r["tag"], ms)
        assert all(1 <= m <= r["n"] for m in ms) and ms[0] in DC.SCHUR_EDGES, (r["tag"], ms)
        assert (r["n"] in ms) if r["case"] % 8 == 0 else True, (r["tag"], ms)


def test_every_schur_class_is_reached_by_three_cases():
    rows = [r for r in _measure()["rows"] if "schur" in r]
    reach = [set().union(*(x["classes"] for x in r["schur"])) for r in rows]
    hist = {c: sum(c in s for s in reach) for c in DC.SCHUR_CLASSES}
    pairs = {c: sum(c in x["classes"] for r in rows for x in r["schur"]) for c in DC.SCHUR_CLASSES}
    print(f"classes of k_schur_tile's walk reached, cases of {len(rows)} real symmetric ones ((case, m) pairs of "
          f"{sum(len(r['schur']) for r in rows)}):")
    for c in DC.SCHUR_CLASSES:
        print(f"  {c:20s} {hist[c]:3d}  ({pairs[c]:3d})")
    assert all(s <= set(DC.SCHUR_CLASSES) for s in reach)
    few = {c: k for c, k in hist.items() if k < 3}
    assert not few, few


def test_every_complex_front_class_is_reached_by_three_arrows():
    rows = [r for r in _measure()["rows"] if "cx_classes" in r]
    assert len(rows) == DC.NCX_ARROW * len(DC.SEEDS)
    hist = {c: sum(c in r["cx_classes"] for r in rows) for c in DC.CX_CLASSES}
    print(f"classes of the twin-space fronts reached, arrows of {len(rows)} complex ones:")
    for c in DC.CX_CLASSES:
        print(f"  {c:16s} {hist[c]:3d}")
    assert all(r["cx_classes"] <= set(DC.CX_CLASSES) for r in rows)
    few = {c: k for c, k in hist.items() if k < 3}
    assert not few, few
    # the edges in twin space: w + r = 68 is the last thin front, 2 w = 64 the panel, 2 w = 256 one whole column block
    assert DC.cx_front_classes([0, 32], [0, 68]) == {"cx_thin", "cx_thin_r136", "cx_panel_exact"}
    assert DC.cx_front_classes([0, 33], [0, 69]) == {"cx_generic", "cx_panel_over"}
    assert DC.cx_front_classes([0, 128], [0, 128]) == {"cx_generic", "cx_norows", "cx_chain_exact"}
    assert DC.cx_front_classes([0, 128], [0, 129]) == {"cx_generic", "cx_chain_exact", "cx_solve_big"}
    assert DC.cx_front_classes([0, 129], [0, 129]) == {"cx_generic", "cx_norows", "cx_solve_big"}


def test_complex_arrows_have_the_supernodes_asked_for_and_a_factor_within_a_tenth_of_the_bar():
    """the product's CPU path on the 12 complex block arrows against numpy.linalg.cholesky, L by supernode
    (device_fuzz_corpus.by_supernode): measured worst 1.14e-15 against 0.1 x TOL_L = 1e-13"""
    rows = [r for r in _measure()["rows"] if "cx_classes" in r]
    for r in rows:
        want = [(w, w + b) for w, b in r["leaves"]] + [(DC.CX_ROOT, DC.CX_ROOT)]
        assert r["fronts"][-1] == want[-1] and sorted(r["fronts"]) == sorted(want), (r["tag"], r["fronts"], want)
        assert r["leaves"][0] in DC.EDGE_PAIRS and r["n"] <= DC.CX_NMAX
        assert r["cx_dead"] == 0 and r["cx_imag"] == 0, r["tag"]
    worst = max(rows, key=lambda r: r["cx_L"])
    print(f"complex arrows, L by supernode on the CPU path: worst {worst['cx_L']:.3e} ({worst['tag']}, seed {worst['seed']})")
    assert worst["cx_L"] <= 0.1 * TOL_L, worst["tag"]
    assert [r["twin"] for r in rows] == [bool(k % 2) for k in range(DC.NCX_ARROW)] * len(DC.SEEDS)      # both storages


def test_the_schur_restatements_leave_nine_tenths_of_the_bar():
    """schur_reference.schur_restated against dense_schur on every (case, m): measured worst 0.0020 x bar; the tile-level
    restatement of k_schur_tile (_schur_tiled) against schur_restated: measured worst 2.4e-16 relative, bound 1e-14"""
    pairs = [(r, x) for r in _measure()["rows"] if "schur" in r for x in r["schur"]]
    r, x = max(pairs, key=lambda q: q[1]["restated"])
    print(f"schur_restated: worst error / bar = {x['restated']:.4f} (m {x['m']}, {r['tag']}, seed {r['seed']}) over {len(pairs)} (case, m)")
    assert x["restated"] <= 0.1, (r["tag"], x["m"])
    r, x = max(pairs, key=lambda q: q[1]["tiled"])
    print(f"tile restatement against schur_restated: worst {x['tiled']:.3e} (m {x['m']}, {r['tag']}, seed {r['seed']})")
    assert x["tiled"] <= 1e-14, (r["tag"], x["m"])


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_corpus_sees_a_wrong_tile_walk(mutant):
    """a tile kernel with this error would miss the bar of the GPU comparison on at least 3 (case, m) of the corpus"""
    pairs = [(r, x) for r in _measure()["rows"] if "schur" in r for x in r["schur"]]
    seen = [(r, x) for r, x in pairs if not x[mutant] <= 1.0]
    r, x = max(pairs, key=lambda q: q[1][mutant])
    print(f"mutant {mutant}: above the bar on {len(seen)} of {len(pairs)} (case, m), worst {x[mutant]:.3e} x bar (m {x['m']}, {r['tag']})")
    assert len(seen) >= 3
