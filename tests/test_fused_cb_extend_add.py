"""The contribution-block half of the extend-add fused into the update (plan flag CHOLMOD_HIP_FUSED_CB_EA, set by the host
layer unless CHOLMOD_HIP_NO_FUSED_CB_EA=1): the one update region that covers the whole contribution block of a front and
is the first to write all of it -- its carrier -- takes the children's entries that land there with it (k_update3f, through
inverse relative maps built on the device once per plan), and the second extend-add phase leaves that front out.

Host-only plans: without the flag every plan is what it was (tests/test_schedule_fingerprint.py and tests/test_front_heads.py
pin that; here the three entry points once more against each other); with it, the plans of a small battery are pinned in
tests/golden/fused_cb_ea_fingerprints.json (`python tests/test_fused_cb_extend_add.py write` re-records them), every front's
contribution-block columns are taken in exactly one place, and what the plan says of every (parent, child) pair equals a
count from the row lists.

GPU: every case is factored with the fusion and with CHOLMOD_HIP_NO_FUSED_CB_EA=1 -- the two factors agree entry by entry to
1e-13 relative, each agrees with the oracle to the project's 1e-12 in the Frobenius norm, and a solve leaves a small
residual.  The inverse maps live on the device only, so their comparison with a numpy inverse of the relative maps is a GPU
test as well.  (Where the carrier is the assigning first outer update the fused factor is bit for bit the unfused one: the
children are taken off the accumulators in child order, -(acc - c1 - c2) == (-acc + c1) + c2; behind a head the carrier
updates, C - (acc - c1 - c2) against ((C - acc) + c1) + c2: rounding.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import OracleFactor  # noqa: E402
from suitesparse_amd import cholmod as ch, generators as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_cb_ea_fingerprints.json")
KNOBS = ("CHOLMOD_HIP_NO_HEADS", "CHOLMOD_HIP_HEAD_NO_GATHER", "CHOLMOD_HIP_HEAD_ALL", "CHOLMOD_HIP_UPD3_MIN_TILES",
         "CHOLMOD_HIP_NO_FUSED_CB_EA", "CHOLMOD_HIP_UPD3_HALF_MAX")
MT16 = {"CHOLMOD_HIP_UPD3_MIN_TILES": "16"}
ALL16 = {"CHOLMOD_HIP_UPD3_MIN_TILES": "16", "CHOLMOD_HIP_HEAD_ALL": "1"}
K_UPD_W = 12


class knobs:
    """the environment knobs of a plan, set for a block and put back after it"""
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in KNOBS}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in self.saved.items():
            if v is not None:
                os.environ[k] = v


def problem(name):
    if name.startswith("p3d_"):
        m = int(name[4:])
        return G.poisson3d(m), G.geometric_nd(m, m, m, 4), True
    if name == "box12r2":
        return G.box_stencil3d(12, 2), G.geometric_nd(12, 12, 12, 3), True
    if name == "p2d_150":
        return G.poisson2d(150), G.geometric_nd(150, 150, 1, 4), True
    assert name == "rand16"          # a random permutation, not postordered: parents with one, three and more children
    return G.poisson3d(16), np.random.default_rng(7).permutation(16 ** 3), False


def plan_facts(L, p, nsuper, maps=False):
    """what the test hooks tell of plan p: per front (eligible, carriers, extend-add groups over its contribution-block
    columns, children), the (parent, child) pairs of the carriers (with their maps from the device if asked for) and the
    grid of every launch that holds a carrier"""
    out = np.zeros(4 * max(nsuper, 1), np.int64)
    assert L.cholmod_hip_debug_cb_extend_add(p, nsuper, out.ctypes.data) == nsuper
    npairs = L.cholmod_hip_debug_fused_pair(p, -1, None, None, None)
    pairs = []
    for q in range(npairs):
        d = np.zeros(8, np.int64)
        assert L.cholmod_hip_debug_fused_pair(p, q, d.ctypes.data, None, None) == npairs
        rec = dict(zip(("parent", "child", "pnscol", "pncb", "nc", "cbp", "mcb", "launch"), map(int, d)))
        if maps:
            rec["inv"], rec["rel"] = np.zeros(rec["pncb"], np.int32), np.zeros(rec["nc"], np.int32)
            assert L.cholmod_hip_debug_fused_pair(p, q, d.ctypes.data, rec["inv"].ctypes.data, rec["rel"].ctypes.data) == npairs
        pairs.append(rec)
    # (the carrier itself: region of its launch that writes the parent's contribution block -- does it assign or update?)
    for l in {r["launch"] for r in pairs}:
        ng = L.cholmod_hip_debug_launch_regions(p, l, 0, None)
        reg = np.zeros(12 * ng, np.int64)
        assert L.cholmod_hip_debug_launch_regions(p, l, ng, reg.ctypes.data) == ng
        reg = reg.reshape(-1, 12)
        for r in pairs:
            if r["launch"] == l:
                mine = reg[(reg[:, 9] == r["parent"]) & (reg[:, 4] == 1)]
                assert len(mine) == 1 and mine[0, 0] == mine[0, 1] == r["pncb"] and mine[0, 3] == 1
                r["assign"] = int(mine[0, 10])
    nl = L.cholmod_hip_get_launch_profile(p, 0, None, None, None, None, None, None)
    kind, grid = np.zeros(nl, np.int32), np.zeros(nl, np.int32)
    L.cholmod_hip_get_launch_profile(p, nl, kind.ctypes.data, grid.ctypes.data, None, None, None, None)
    assert all(kind[r["launch"]] == K_UPD_W for r in pairs)
    return out.reshape(-1, 4)[:nsuper], pairs, sorted({(r["launch"], int(grid[r["launch"]])) for r in pairs})


class Analysed:
    def __init__(self, name):
        (self.n, self.Ap, self.Ai, self.Ax), perm, post = problem(name)
        self.S = ch.Session(use_gpu=0, postorder=post)
        self.A = self.S.sparse(self.n, self.Ap, self.Ai, self.Ax, -1)
        self.Lf = self.S.analyze(self.A, perm)
        self.fv = ch.FactorView(self.Lf)

    def reach(self):
        rp = np.zeros(self.fv.nsuper + 1, np.int64)
        ln = self.S.L.cholmod_l_hip_front_reach(self.A, self.Lf, rp.ctypes.data, None, C.byref(self.S.cm))
        rf = np.zeros(max(ln, 1), np.int32)
        assert self.S.L.cholmod_l_hip_front_reach(self.A, self.Lf, rp.ctypes.data, rf.ctypes.data, C.byref(self.S.cm)) == ln
        return rp, rf

    def plan(self, entry="reach", fused=True, env=None):
        """host-only plan through one of the three entry points -> (hash words, facts)"""
        L, f, st = self.S.L, self.Lf.contents, C.c_int(0)
        flags = ch.HIP_PLAN_HOST_ONLY | (ch.HIP_FUSED_CB_EA if fused else 0)
        with knobs(env):
            a = (self.fv.n, self.fv.nsuper, f.super, f.pi, f.px, f.s, flags)
            if entry == "create":
                p = L.cholmod_hip_plan_create(*a, C.byref(st))
            elif entry == "dist":
                p = L.cholmod_hip_plan_create_dist(*a, 0, 1, C.byref(st))
            else:
                rp, rf = self.reach() if entry == "reach" else (None, None)
                p = L.cholmod_hip_plan_create_reach(*a, rp.ctypes.data if entry == "reach" else None,
                                                    rf.ctypes.data if entry == "reach" else None, C.byref(st))
            assert p and st.value == 0
            h = (C.c_uint64 * 16)()
            assert L.cholmod_hip_debug_schedule_hash(p, h) == 0
            facts = plan_facts(L, p, self.fv.nsuper)
            L.cholmod_hip_plan_destroy(p)
        return [f"{x:016x}" for x in h], facts

    def close(self):
        self.S.free_factor(self.Lf)
        self.S.free_sparse(self.A)
        self.S.finish()


VARIANTS = (("noreach", "noreach", {}), ("reach", "reach", {}), ("noreach_mt16", "noreach", MT16), ("reach_mt16", "reach", MT16),
            ("reach_all_mt16", "reach", ALL16))
BATTERY = ("p3d_24", "p3d_40", "box12r2", "p3d_64")


def fingerprints():
    out = {}
    for name in BATTERY:
        an = Analysed(name)
        try:
            for key, entry, env in VARIANTS:
                h, (fronts, pairs, launches) = an.plan(entry, env=env)
                out[f"{name}|{key}"] = h + [f"{int(fronts[:, 1].sum())} carriers, {len(pairs)} pairs"]
        finally:
            an.close()
    return out


def test_fused_plans_match_the_recorded_fingerprints():
    ref = json.load(open(GOLDEN))
    got = fingerprints()
    assert set(got) == set(ref)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, bad
    # the battery holds carriers behind a head, in launches of half tiles and of whole small regions
    assert got["p3d_64|reach_all_mt16"] != got["p3d_64|reach_mt16"]
    assert all(not ref[f"{n}|reach_mt16"][16].startswith("0 ") for n in BATTERY)


@pytest.mark.parametrize("name", ["p3d_24", "box12r2", "rand16"])
def test_without_the_flag_every_entry_point_builds_the_old_plan(name):
    an = Analysed(name)
    try:
        for env in ({}, MT16):
            old, (fronts, pairs, _) = an.plan("create", fused=False, env=env)
            assert fronts[:, 1].sum() == 0 and not pairs
            assert an.plan("dist", fused=False, env=env)[0] == old
            assert an.plan("noreach", fused=False, env=env)[0] == old
            new, (fronts, pairs, _) = an.plan("create", env=env)
            # where no region is a carrier the flag changes nothing at all; where one is, the side arrays enter the hash
            assert (new == old) == (len(pairs) == 0)
            assert an.plan("dist", env=env)[0] == new and an.plan("noreach", env=env)[0] == new
        assert len(pairs) > 0
    finally:
        an.close()


def check_one_place_and_pairs(an, fronts, pairs):
    """every front's contribution-block columns are extend-added in exactly one place; the pairs are the child lists of the
    carriers; what the plan says of a pair is what the row lists say"""
    fv = an.fv
    el = fronts[:, 0] == 1
    assert np.all(fronts[el, 1] + fronts[el, 2] == 1), np.nonzero(el & (fronts[:, 1] + fronts[:, 2] != 1))[0][:8]
    assert np.all(fronts[~el, 1] == 0)
    nscol, nsrow = np.diff(fv.super), np.diff(fv.pi)
    smap = np.repeat(np.arange(fv.nsuper), nscol)
    per_parent = {}
    for r in pairs:
        p, c = r["parent"], r["child"]
        per_parent[p] = per_parent.get(p, 0) + 1
        crows = fv.s[fv.pi[c] + nscol[c]:fv.pi[c + 1]]
        assert smap[crows[0]] == p and fronts[p, 1] == 1
        assert (r["pnscol"], r["pncb"], r["nc"]) == (nscol[p], nsrow[p] - nscol[p], len(crows))
        assert r["mcb"] == int(np.sum(crows >= fv.super[p + 1]))
    for p, cnt in per_parent.items():
        assert cnt == fronts[p, 3]


@pytest.mark.parametrize("name", ["p3d_24", "p3d_40", "box12r2", "p3d_64", "rand16", "p2d_150"])
def test_contribution_block_columns_are_taken_in_exactly_one_place(name):
    an = Analysed(name)
    try:
        total = 0
        for key, entry, env in VARIANTS + (("mt4", "noreach", {"CHOLMOD_HIP_UPD3_MIN_TILES": "4"}),):
            _, (fronts, pairs, _) = an.plan(entry, env=env)
            check_one_place_and_pairs(an, fronts, pairs)
            total += len(pairs)
        assert total > 0
        # not eligible, both phases kept: no flag, or the assigning update switched off
        _, (fronts, pairs, _) = an.plan("reach", fused=False, env=MT16)
        assert not pairs and np.all(fronts[fronts[:, 0] == 1, 2] == 1)
    finally:
        an.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------

# name -> (problem, knobs, what the plan must hold for the case to be the case the test is about)
CASES = {
    "p3d_24": ("p3d_24", MT16, dict(carriers=1)),
    "p3d_32": ("p3d_32", MT16, dict(carriers=1)),
    "box12r2": ("box12r2", MT16, dict(carriers=1, odd_ncb=True)),
    "p2d_150_packed_children": ("p2d_150", {"CHOLMOD_HIP_UPD3_MIN_TILES": "4"}, dict(carriers=1, packed=True)),
    "p3d_40_head_all": ("p3d_40", ALL16, dict(carriers=1, behind_head=True)),
    "rand16_no_postorder": ("rand16", MT16, dict(carriers=1, packed=True, nch=(1, 3))),
    "p3d_40_half_tiles": ("p3d_40", {}, dict(carriers=1, half=True)),
}


def factor_once(name, env, fused, beta=0.0, planted=None, maps=False):
    (n, Ap, Ai, Ax), perm, post = problem(name)
    if planted is not None:
        Ax = Ax.copy()
        Ax[Ap[planted]] = -1.0          # (lower storage: the first entry of a column is its diagonal)
    e = dict(env)
    if not fused:
        e["CHOLMOD_HIP_NO_FUSED_CB_EA"] = "1"
    with knobs(e):
        S = ch.Session(postorder=post)
        S.cm.error_handler = ch.ERRFUNC(0)
        A = S.sparse(n, Ap, Ai, Ax, -1)
        Lf = S.analyze(A, perm)
        assert S.factorize(A, Lf, beta) == 1
        fv = ch.FactorView(Lf)
        for k in ("super", "pi", "s"):          # (views of the factor: kept past its release as copies)
            setattr(fv, k, getattr(fv, k).copy())
        res = dict(status=S.cm.status, minor=fv.minor, x=fv.x.copy(), fv=fv, n=n, mat=(Ap, Ai, Ax), perm=perm, post=post,
                   stats=S.hip_stats(Lf))
        res["facts"] = plan_facts(S.L, Lf.contents.hip_plan, fv.nsuper, maps=maps)
        if S.cm.status == ch.OK:
            b = G.demo_rhs(n)
            y = S.solve(Lf, b)
            res["resid"] = np.linalg.norm(G.sym_matvec(n, Ap, Ai, Ax, -1, y) - b) / np.linalg.norm(b)
        S.free_factor(Lf)
        S.free_sparse(A)
        S.finish()
    return res


def entrywise(a, b):
    """largest |a - b| / |b| over the entries (0 where both are zero)"""
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / np.abs(b))
    return float(r.max()) if len(r) else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_factor_equals_the_unfused_one_and_the_oracle(case):
    name, env, want = CASES[case]
    on, off = factor_once(name, env, True), factor_once(name, env, False)
    fronts, pairs, launches = on["facts"]
    assert not off["facts"][1] and off["facts"][0][:, 1].sum() == 0
    assert len(pairs) >= want["carriers"]
    fv = on["fv"]
    if want.get("odd_ncb"):
        assert any(r["pncb"] % 2 == 1 and r["pncb"] % 64 != 0 for r in pairs)
    if want.get("packed"):
        assert any(r["cbp"] for r in pairs) and any(not r["cbp"] for r in pairs)
    if want.get("nch"):
        assert set(want["nch"]) <= set(int(v) for v in fronts[fronts[:, 1] == 1, 3])
    if want.get("half"):
        assert any(512 <= g < 10240 for _, g in launches), launches
    if want.get("behind_head"):
        # a carrier behind a head updates the block the head update has written; the others assign
        assert any(not r["assign"] for r in pairs) and any(r["assign"] for r in pairs)
    else:
        assert all(r["assign"] for r in pairs)
    assert on["stats"][10] < off["stats"][10]           # the extend-add's algorithmic bytes fall
    assert on["status"] == ch.OK and off["status"] == ch.OK
    rel = entrywise(on["x"], off["x"])
    n, (Ap, Ai, Ax) = on["n"], on["mat"]
    O = OracleFactor(n, Ap, Ai, -1, perm=on["perm"], postorder=on["post"])
    assert O.factorize(Ax) == 0
    m = O.lower_mask()
    errs = [np.linalg.norm((r["x"] - O.x)[m]) / np.linalg.norm(O.x[m]) for r in (on, off)]
    print(f"{case}: {len(pairs)} pairs in launches {launches[:6]}; fused vs unfused, entry by entry: {rel:.3e}; "
          f"against the oracle: fused {errs[0]:.3e} unfused {errs[1]:.3e}; residuals {on['resid']:.2e} {off['resid']:.2e}")
    assert rel <= 1e-13
    assert max(errs) <= 1e-12
    assert max(on["resid"], off["resid"]) < 1e-11


@pytest.mark.gpu
def test_inverse_maps_are_the_inverse_of_the_relative_maps():
    """the maps as the device holds them: the relative map of a pair against the row lists, its inverse against numpy"""
    res = factor_once("rand16", MT16, True, maps=True)
    fv, (fronts, pairs, _) = res["fv"], res["facts"]
    assert len(pairs) > 100
    for r in pairs:
        p, c = r["parent"], r["child"]
        prow = fv.s[fv.pi[p]:fv.pi[p + 1]]
        crow = fv.s[fv.pi[c] + (fv.super[c + 1] - fv.super[c]):fv.pi[c + 1]]
        assert np.array_equal(r["rel"], np.searchsorted(prow, crow))
        want = np.full(r["pncb"], -1, np.int32)
        j = np.nonzero(r["rel"] >= r["pnscol"])[0]
        want[r["rel"][j] - r["pnscol"]] = j
        assert np.array_equal(r["inv"], want)
        assert len(j) == r["mcb"]


@pytest.mark.gpu
def test_not_positive_definite_with_carriers_and_a_reference_matrix():
    """a failed front still writes its block, carriers take it like the extend-add did and the ancestors discard it: status,
    L->minor and the zeroed tail are the oracle's, with the fusion and without.  Poisson 24^3 with one diagonal entry made
    negative in the middle of the ordering (fronts with carriers above it), and an indefinite file of the reference's
    (tests/golden/tcov; thin fronts only: the protocol around the fused plans, not the carriers themselves)."""
    (n, Ap, Ai, Ax), perm, _ = problem("p3d_24")
    col = int(perm[n // 3])
    runs = [factor_once("p3d_24", MT16, f, planted=col) for f in (True, False)]
    Axp = runs[0]["mat"][2]
    O = OracleFactor(n, Ap, Ai, -1, perm=perm, postorder=True)
    assert O.factorize(Axp) == 1 and O.minor < n
    m = O.lower_mask()
    assert len(runs[0]["facts"][1]) > 0
    for r in runs:
        assert r["status"] == ch.NOT_POSDEF and r["minor"] == O.minor
        assert np.all(r["x"][~m] == 0)
        assert np.array_equal(r["x"][m] == 0, O.x[m] == 0)
        live = m & (O.x != 0) & np.isfinite(O.x)
        assert np.linalg.norm((r["x"] - O.x)[live]) <= 1e-11 * np.linalg.norm(O.x[live])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_tcov_matrices as T
    for e in ({}, {"CHOLMOD_HIP_NO_FUSED_CB_EA": "1"}):
        with knobs(e):
            T.run_case("tcov", "3singular", "default", 1, use_gpu=1)
            T.run_case("tcov", "2lo.tri", "default", 1, use_gpu=1)


if __name__ == "__main__" and sys.argv[1:] == ["write"]:
    fp = fingerprints()
    json.dump(fp, open(GOLDEN, "w"), indent=0, sort_keys=True)
    print("wrote", len(fp), "fingerprints to", GOLDEN)
