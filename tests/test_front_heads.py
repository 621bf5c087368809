"""Heads of the relaxed fronts (cholmod_hip_plan_create_reach): where the analysis finds the explicit zeros relaxed
amalgamation leaves in a front, the plan gives it a first outer block of H columns whose closing update runs over the rows
those columns reach only (schedule_dense.hip: add_head_gathered).

Host-only plans here: the reach the host layer computes against an independent count and against the exact patterns of the
zero-relaxation analysis, the flops the heads leave out (stats [40]) against a count from the reach, the knobs, the old
entry point, and the new plans' fingerprints (tests/golden/head_fingerprints.json; `python tests/test_front_heads.py write`
re-records them).  The GPU test factors with gathering on and off under the same heads: bit for bit the same factor."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from suitesparse_amd import cholmod as ch, generators as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "head_fingerprints.json")
KNOBS = ("CHOLMOD_HIP_NO_HEADS", "CHOLMOD_HIP_HEAD_NO_GATHER", "CHOLMOD_HIP_HEAD_ALL")
INT32_MAX = 2 ** 31 - 1
REACH_MIN_COLS = 512


def problem(name):
    if name.startswith("p3d_"):
        m = int(name[4:])
        return G.poisson3d(m), G.geometric_nd(m, m, m, 4)
    assert name == "box12r2"
    return G.box_stencil3d(12, 2), G.geometric_nd(12, 12, 12, 3)


class Analysed:
    def __init__(self, name, relax=True):
        (self.n, self.Ap, self.Ai, self.Ax), perm = problem(name)
        self.S = ch.Session(use_gpu=0)
        if not relax:
            for q in range(3):
                self.S.cm.nrelax[q] = 0
                self.S.cm.zrelax[q] = 0.0
        self.A = self.S.sparse(self.n, self.Ap, self.Ai, self.Ax, -1)
        self.Lf = self.S.analyze(self.A, perm)
        self.fv = ch.FactorView(self.Lf)

    def reach(self):
        rp = np.zeros(self.fv.nsuper + 1, np.int64)
        ln = self.S.L.cholmod_l_hip_front_reach(self.A, self.Lf, rp.ctypes.data, None, C.byref(self.S.cm))
        rf = np.zeros(max(ln, 1), np.int32)
        assert self.S.L.cholmod_l_hip_front_reach(self.A, self.Lf, rp.ctypes.data, rf.ctypes.data, C.byref(self.S.cm)) == ln
        return rp, rf[:ln]

    def plan(self, reach=True, env=None):
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        os.environ.update(env or {})
        try:
            f = self.Lf.contents
            st = C.c_int(0)
            if reach is None:
                p = self.S.L.cholmod_hip_plan_create_dist(self.fv.n, self.fv.nsuper, f.super, f.pi, f.px, f.s,
                                                          ch.HIP_PLAN_HOST_ONLY, 0, 1, C.byref(st))
            else:
                rp, rf = self.reach() if reach else (None, None)
                p = self.S.L.cholmod_hip_plan_create_reach(self.fv.n, self.fv.nsuper, f.super, f.pi, f.px, f.s,
                                                           ch.HIP_PLAN_HOST_ONLY, rp.ctypes.data if reach else None,
                                                           rf.ctypes.data if reach else None, C.byref(st))
            assert p and st.value == 0
            h = (C.c_uint64 * 16)()
            assert self.S.L.cholmod_hip_debug_schedule_hash(p, h) == 0
            s = np.zeros(ch.CHOLMOD_HIP_NSTATS)
            assert self.S.L.cholmod_hip_get_stats(p, s.ctypes.data) == 0
            self.S.L.cholmod_hip_plan_destroy(p)
            return [f"{x:016x}" for x in h], s
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
            for k, v in saved.items():
                if v is not None:
                    os.environ[k] = v

    def close(self):
        self.S.free_factor(self.Lf)
        self.S.free_sparse(self.A)
        self.S.finish()


def supernodal_children(fv):
    sup, pi, s = fv.super, fv.pi, fv.s
    smap = np.repeat(np.arange(fv.nsuper), np.diff(sup))
    kids = {}
    for c in range(fv.nsuper):
        nscol = sup[c + 1] - sup[c]
        if pi[c] + nscol < pi[c + 1]:
            kids.setdefault(int(smap[s[pi[c] + nscol]]), []).append(c)
    return kids


def independent_reach(an):
    """first column of every big front reaching each of its rows: A's pattern (permuted by L->Perm) in the front's columns
    and the contribution-block rows of the children, from the column where each child's block begins"""
    fv, n = an.fv, an.n
    Ap, Ai = np.asarray(an.Ap), np.asarray(an.Ai)
    inv = np.empty(n, np.int64)
    inv[fv.Perm] = np.arange(n)
    r, c = inv[Ai], inv[np.repeat(np.arange(n), np.diff(Ap))]
    rr, cc = np.concatenate([r, c]), np.concatenate([c, r])
    keep = rr > cc
    rr, cc = rr[keep], cc[keep]
    o = np.argsort(cc, kind="stable")
    rr, cc = rr[o], cc[o]
    cp = np.searchsorted(cc, np.arange(n + 1))
    kids = supernodal_children(fv)
    out = {}
    for s in range(fv.nsuper):
        k1, nscol = fv.super[s], fv.super[s + 1] - fv.super[s]
        if nscol < REACH_MIN_COLS:
            continue
        rows = fv.s[fv.pi[s]:fv.pi[s + 1]]
        first = np.full(len(rows), INT32_MAX, np.int64)
        first[:nscol] = np.arange(nscol)
        for j in range(nscol):
            pos = np.searchsorted(rows, rr[cp[k1 + j]:cp[k1 + j + 1]])
            np.minimum.at(first, pos, j)
        for ch_ in kids.get(s, []):
            cr = fv.s[fv.pi[ch_] + fv.super[ch_ + 1] - fv.super[ch_]:fv.pi[ch_ + 1]]
            pos = np.searchsorted(rows, cr)
            np.minimum.at(first, pos, cr[0] - k1)
        out[s] = first
    return out


def exact_reach(an, exact):
    """the same from the exact column patterns: the fundamental supernodes of the zero-relaxation analysis (column j of
    fundamental supernode t holds the rows of t from j on)"""
    ef = exact.fv
    assert np.array_equal(ef.Perm, an.fv.Perm)
    emap = np.repeat(np.arange(ef.nsuper), np.diff(ef.super))
    out = {}
    for s in range(an.fv.nsuper):
        k1, nscol = an.fv.super[s], an.fv.super[s + 1] - an.fv.super[s]
        if nscol < REACH_MIN_COLS:
            continue
        rows = an.fv.s[an.fv.pi[s]:an.fv.pi[s + 1]]
        first = np.full(len(rows), INT32_MAX, np.int64)
        for j in range(nscol):
            t = emap[k1 + j]
            col = ef.s[ef.pi[t]:ef.pi[t + 1]]
            col = col[col >= k1 + j]
            np.minimum.at(first, np.searchsorted(rows, col), j)
        out[s] = first
    return out


@pytest.mark.parametrize("name", ["p3d_24", "p3d_40", "box12r2", "p3d_64"])
def test_reach_equals_an_independent_count_and_covers_the_exact_patterns(name):
    an, ex = Analysed(name), Analysed(name, relax=False)
    try:
        rp, rf = an.reach()
        ind, exa = independent_reach(an), exact_reach(an, ex)
        big = [s for s in range(an.fv.nsuper) if an.fv.super[s + 1] - an.fv.super[s] >= REACH_MIN_COLS]
        assert sorted(ind) == big
        for s in range(an.fv.nsuper):
            got = rf[rp[s]:rp[s + 1]].astype(np.int64)
            if s not in ind:
                assert len(got) == 0
                continue
            assert np.array_equal(got, ind[s]), s
            # never smaller than the exact reach: every row an exact column pattern holds is reached by then
            assert np.all(got <= exa[s]), s
            # ... and equal to it at 64-column granularity
            assert np.array_equal(np.minimum(got, INT32_MAX) // 64, np.minimum(exa[s], INT32_MAX) // 64), s
    finally:
        an.close()
        ex.close()


def expected_skipped(an, rp, rf, all_heads):
    """stats [40] from the reach: the head every front takes (CHOLMOD_HIP_HEAD_ALL=1: the one that leaves out the most flops),
    its row maps paired from H and from nscol on, and the flops of the entries outside them"""
    assert all_heads
    fv = an.fv
    tri = lambda m: m * (m + 1) / 2                                     # noqa: E731
    tri_elems = lambda m, n: n * (n + 1) / 2 + (m - n) * n               # noqa: E731
    total = 0.0
    for s in range(fv.nsuper):
        if rp[s + 1] == rp[s]:
            continue
        first = rf[rp[s]:rp[s + 1]]
        nscol, nsrow = int(fv.super[s + 1] - fv.super[s]), int(fv.pi[s + 1] - fv.pi[s])
        ob = 4096 if nsrow >= 24000 else 2048 if nsrow >= 8000 else 1024 if nsrow >= 4000 else 512
        best, H = 0.0, 0
        for h in range(256, min(ob, nscol), 256):
            R = int(np.sum(first[h:] < h))
            g = 2.0 * h * (tri(nsrow - h) - tri(R))
            if g > best:
                best, H = g, h
        if H == 0:
            continue

        def paired(frm, ncols):
            rows = []
            for p in range(frm, nsrow, 2):
                if first[p] >= H and (p + 1 >= nsrow or first[p + 1] >= H):
                    continue
                rows += [p] + ([p + 1] if p + 1 < nsrow else [])
            return len(rows), sum(1 for p in rows if p < frm + ncols)
        ncb = nsrow - nscol
        m1, n1 = paired(H, nscol - H)
        done = tri_elems(m1, n1) if n1 else 0.0
        if ncb:
            m2, _ = paired(nscol, ncb)
            done += tri(m2)
        total += 2.0 * H * (tri_elems(nsrow - H, nscol - H) + tri(ncb) - done)
    return total


@pytest.mark.parametrize("name", ["p3d_40", "p3d_64"])
def test_skipped_flops_statistic_matches_the_reach(name):
    an = Analysed(name)
    try:
        rp, rf = an.reach()
        _, s = an.plan(env={"CHOLMOD_HIP_HEAD_ALL": "1"})
        want = expected_skipped(an, rp, rf, True)
        assert s[40] == pytest.approx(want, rel=1e-12, abs=0.5)
        if name == "p3d_64":
            assert want > 0.02 * s[1]
        assert s[1] == an.plan(reach=None)[1][1]         # stats [1] stays the supernodal count
    finally:
        an.close()


def test_old_entry_point_and_knobs():
    an = Analysed("p3d_64")
    try:
        old, s_old = an.plan(reach=None)
        assert s_old[40] == 0
        assert an.plan(reach=False)[0] == old                               # the new entry without reach information
        assert an.plan(env={"CHOLMOD_HIP_NO_HEADS": "1", "CHOLMOD_HIP_HEAD_ALL": "1"})[0] == old
        assert an.plan()[0] == old                                          # 64^3: no head pays at the default price
        g, s_g = an.plan(env={"CHOLMOD_HIP_HEAD_ALL": "1"})
        ng, s_ng = an.plan(env={"CHOLMOD_HIP_HEAD_ALL": "1", "CHOLMOD_HIP_HEAD_NO_GATHER": "1"})
        assert s_g[40] > 0 and s_ng[40] == 0
        assert g != old and ng != old and g != ng          # head boundaries without gathering: other regions, no gathered ones
    finally:
        an.close()


def fingerprints():
    out = {}
    for name in ("p3d_40", "box12r2", "p3d_64", "p3d_100"):
        an = Analysed(name)
        try:
            for key, env in (("default", {}), ("all", {"CHOLMOD_HIP_HEAD_ALL": "1"}),
                             ("all_nogather", {"CHOLMOD_HIP_HEAD_ALL": "1", "CHOLMOD_HIP_HEAD_NO_GATHER": "1"})):
                h, s = an.plan(env=env)
                out[f"{name}|{key}"] = h + [f"{s[40]:.6e}"]
        finally:
            an.close()
    return out


def test_head_plans_match_the_recorded_fingerprints():
    ref = json.load(open(GOLDEN))
    got = fingerprints()
    assert set(got) == set(ref)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, bad
    assert got["p3d_100|default"] != got["p3d_100|all"]         # 100^3: heads pay at the default price


@pytest.mark.gpu
def test_gathering_is_bit_for_bit_the_same_factor():
    """64^3 with a head on every front that has one: the factor with the head updates gathered equals, bit for bit, the factor
    with the same heads over all rows; both match the factor without heads to rounding, and solve"""
    import hashlib
    n, Ap, Ai, Ax = G.poisson3d(64)
    perm = G.geometric_nd(64, 64, 64, 4)
    res = {}
    for key, env in (("gather", {"CHOLMOD_HIP_HEAD_ALL": "1"}),
                     ("nogather", {"CHOLMOD_HIP_HEAD_ALL": "1", "CHOLMOD_HIP_HEAD_NO_GATHER": "1"}),
                     ("noheads", {"CHOLMOD_HIP_NO_HEADS": "1"})):
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        os.environ.update(env)
        try:
            S = ch.Session()
            A = S.sparse(n, Ap, Ai, Ax, -1)
            Lf = S.analyze(A, perm)
            assert S.factorize(A, Lf) == 1 and S.cm.status == ch.OK
            x = ch.FactorView(Lf).x.copy()
            st = S.hip_stats(Lf)
            b = G.demo_rhs(n)
            y = S.solve(Lf, b)
            r = np.linalg.norm(G.sym_matvec(n, Ap, Ai, Ax, -1, y) - b) / np.linalg.norm(b)
            res[key] = (hashlib.sha256(x.tobytes()).hexdigest(), x, st, r)
            S.free_factor(Lf); S.free_sparse(A); S.finish()
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
            for k, v in saved.items():
                if v is not None:
                    os.environ[k] = v
    assert res["gather"][2][40] > 0 and res["nogather"][2][40] == 0
    assert res["gather"][0] == res["nogather"][0]
    xg, xn = res["gather"][1], res["noheads"][1]
    assert np.max(np.abs(xg - xn)) <= 1e-12 * np.max(np.abs(xn))
    assert max(v[3] for v in res.values()) < 1e-11


if __name__ == "__main__" and sys.argv[1:] == ["write"]:
    fp = fingerprints()
    json.dump(fp, open(GOLDEN, "w"), indent=0, sort_keys=True)
    print("wrote", len(fp), "fingerprints to", GOLDEN)
