"""The case table of NaN and Inf values in the matrix, the right-hand sides and the iterate, and its references.  numpy and
the CPU oracle only: no torch, no GPU (tests/test_nonfinite_cases.py pins the table on the CPU,
tests/nonfinite_device_cases.py runs it on the device).  The matrices, the supernodal structure and the kernel pinning are
those of tests/not_posdef_cases.py.

A case is a matrix of that table, POISONED entries -- (front, column within it, row within it or "diag", value) with the
value NaN, +Inf or -Inf; "im": the imaginary part of a complex entry --, optional planted pivots (-7.0 or -Inf on a
diagonal), plan flags and quick_return_if_not_posdef.

Every pivot kernel follows dpotrf: a pivot <= 0 stops the factorization, a NaN pivot does not (`d <= 0.0` is false for a
NaN).  A blocked kernel and the reference's substitution loops may differ in WHERE inside a supernode a NaN shows (Winv
times a block whose upper triangle is zero spreads it up the block: 0 * NaN is NaN), so the oracle's NaN pattern is not
the bar by entry.  The bar is two sets, over the entries of L in the supernodal layout:

    must   the unblocked column Cholesky on the dense permuted matrix, restated as boolean masks over the SIMPLICIAL pattern
           of L (the supernodal pattern of a matrix without relaxed supernodes; for the Poisson case the pattern of a second
           OracleFactor with relaxation off):
               nan (i, j)  =  nanA (i, j)  or  nan (j, j)  or  some k < j with (i, k) and (j, k) on the pattern and one of
                                                                 them NaN.
           Only "not being read" removes a NaN: every implementation shows at least this set.
    may    every entry of every supernode on the path from a supernode that holds a poisoned entry to its root, in the
           supernodal tree.

    must  <=  { non-finite entries }  <=  may ;
    every supernode outside may is BIT-IDENTICAL to the same implementation's factor of the clean values ;
    status, minor and -- where both are finite -- the zero pattern and the values (TOL_L) are the oracle's.

A planted pivot whose diagonal entry is in must is NaN and does not trip; every other plant trips, the smallest gives minor
(a plant at column 10 of a leaf whose column 64 is poisoned is in may, not in must: no kernel may have looked at column 64
by then).  After a failure the columns from minor on (the whole failing supernode under quick return) and every later
supernode are +0.0, as tests/not_posdef_cases.py states, on the path or not: must and may are cut there, and those entries
are held to +0.0 as bits.  Where the failure comes in the poisoned supernode before its first poisoned column, nothing
anywhere is non-finite.

+Inf on a diagonal (group "inf") is held to the weaker contract only: the oracle gives L (j, j) = +inf and zeros below it,
the device NaN (sqrt_rsqrt: rsq (inf) = 0, inf * 0), so values inside may are not compared and no must set is asked for.

Solves with NaN at row i of a right-hand side: under SYS_L must = the etree path
from i to its root, may = all columns of the supernodes on that path; under SYS_A must = may = the whole tree (connected
component) of i.  Under SYS_Lt alone the back substitution carries a NaN DOWN the tree only -- x (j) reads x (i) for i > j
with (i, j) on the pattern --: must = the closure of that rule (the descendants of i; the oracle's ltsolve shows exactly
them), may = all columns of the supernodes that hold or read a must row.  Both lie inside the tree of i.  Residual R = B - A X with X NaN at row k: row j of R is NaN exactly when j == k or A (j, k) is
on the pattern.  Everything outside may is bit-identical to the clean call -- where the clean call itself is reproducible
(reproducible_rows: the forward solves are not, in the rows that sibling supernodes add into); the other rows agree with it
within twice the bar of a solve, each call being within that bar of the exact solution."""
import functools

import numpy as np

import not_posdef_cases as NP
from not_posdef_cases import DEEP_FLAGS, PLANT, ROOT, THIN_FLAGS, TOL_L, NO_SMALL_FRONTS, NO_LEAF_PAIRS  # noqa: F401

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
VALUES = {"nan": NAN, "+inf": PINF, "-inf": NINF}
_REG = {}                   # ref_key -> the first case that has it
GROUPS = ("leafdiag", "twokernel", "offdiag", "sharedlaunch", "mixed", "levels", "complex", "inf")


def _vname(v):
    return "nan" if v != v else ("+inf" if v > 0 else "-inf" if v == NINF else repr(v))


def _fname(f):
    return "x".join(map(str, f)) if isinstance(f, tuple) else "s" + str(f)


class Case:
    def __init__(self, group, key, poison, flags, quick=False, plants=(), plant_value=PLANT, storage=None, kernel=None,
                 weak=False, env=None):
        """poison: ((width, below-rows) of a front of the arrow | a supernode index, column within it, row within it
        (>= the column) or "diag", value [, "im"]) ...; plants: (front, column within it) ...: plant_value on that
        diagonal; kernel: what NP.factor_kernel says of the FIRST poisoned front under the case's flags; weak: the +Inf
        contract (no must set, values inside may not compared); env: variables the scheduler reads from the environment
        when the plan is made, set around the case"""
        st = NP.structure(key)
        self.group, self.key, self.flags, self.quick, self.storage = group, key, int(flags), bool(quick), storage
        self.kernel, self.weak, self.plant_value = kernel, bool(weak), float(plant_value)
        self.env = dict(env or {})
        P = []
        for f, j, i, v, *part in poison:
            k = st.front(f) if isinstance(f, tuple) else int(f)
            i = j if i == "diag" else int(i)
            assert 0 <= j < st.nscol[k] and j <= i < st.nsrow[k], (poison, k, j, i)
            assert part in ([], ["im"]) and (not part or (storage and i != j))
            P.append((k, int(j), i, _vname(float(v)), "im" if part else "re"))
        self.P = tuple(P)
        self.fronts = [p[0] for p in self.P]
        Kf = [st.front(f) if isinstance(f, tuple) else int(f) for f, _ in plants]
        self.K = tuple(int(st.super[k]) + j for k, (_, j) in zip(Kf, plants))
        tag = "+".join(f"{_fname(f)}@{j}" + ("" if i == "diag" else f"r{i}") + (":" + _vname(v) if v == v else "")
                       + ("i" if part else "") for f, j, i, v, *part in poison)
        if plants:
            tag += ":plant" + _vname(self.plant_value) + "+".join(f"{_fname(f)}@{j}" for f, j in plants)
        self.name = f"{group}:{key}:{tag}:f{self.flags}:{'quick' if quick else 'full'}" + (f":{storage}" if storage else "")
        self.name += "".join(f":{k}={v}" for k, v in sorted(self.env.items()))
        _REG.setdefault(self.ref_key, self)

    # what the CPU references depend on
    ref_key = property(lambda c: (c.key, c.P, c.K, c.plant_value, c.quick))


def _table():
    out = []
    # leafdiag: NaN on the diagonal of a generic leaf (first, second, third 64-column block) and of the (65, 71) leaf, which
    # is a four-wave thin front unless flag 16 forbids it; flags 8192: the 256-column chain
    for flags in DEEP_FLAGS:
        for j in (0, 64, 128):
            out.append(Case("leafdiag", "deep", [((129, 136), j, "diag", NAN)], flags, kernel="generic"))
        out.append(Case("leafdiag", "deep", [((65, 71), 64, "diag", NAN)], flags,
                        kernel="generic" if flags & NO_SMALL_FRONTS else "thin4"))
    # twokernel: the 256-column chain as k_diag + k_rowsolve (CHOLMOD_HIP_NO_CHAINF in the environment): the NaN pivot in the
    # second 64-column block of the sub-block, so that k_diag's own dinv and k_rowsolve's masking meet it
    out.append(Case("twokernel", "deep", [((129, 136), 64, "diag", NAN)], 8192, kernel="generic", env={"CHOLMOD_HIP_NO_CHAINF": "1"}))
    # offdiag: one below-row entry (row 129 + 50 of the front: a root row) and one entry inside the triangle, column 64
    for flags in (0, 8192):
        out.append(Case("offdiag", "deep", [((129, 136), 64, 129 + 50, NAN)], flags, kernel="generic"))
        out.append(Case("offdiag", "deep", [((129, 136), 64, 100, NAN)], flags, kernel="generic"))
    # sharedlaunch: four leaves in one four-wave launch; two fronts in one WAVE of k_leaf_pair (values-only paths)
    for flags in THIN_FLAGS:
        out.append(Case("sharedlaunch", "thin", [((15, 63), 7, "diag", NAN)], flags, kernel="thin4"))
        out.append(Case("sharedlaunch", "thin", [((64, 72), 63, "diag", NAN)], flags, kernel="thin4"))
        kern = "thin1" if flags & NO_LEAF_PAIRS else "thin1+pair"
        for f, j in (((1, 1), 0), ((4, 8), 2), ((12, 20), 6), ((16, 16), 15)):
            out.append(Case("sharedlaunch", "pair", [(f, j, "diag", NAN)], flags, kernel=kern))
    # mixed: NaN together with a failing pivot
    for quick in (False, True):
        out.append(Case("mixed", "deep", [((65, 71), 32, "diag", NAN)], 0, quick, plants=[((129, 136), 0)], kernel="thin4"))
        out.append(Case("mixed", "deep", [((129, 136), 64, "diag", NAN)], 0, quick, plants=[((129, 136), 10)], kernel="generic"))
        out.append(Case("mixed", "deep", [((129, 136), 64, "diag", NAN)], 0, quick, plants=[(ROOT, 2)], kernel="generic"))
        out.append(Case("mixed", "deep", [((129, 136), 64, "diag", NAN)], 0, quick, plants=[(ROOT, 70)], kernel="generic"))
        out.append(Case("mixed", "deep", [((65, 71), 32, "diag", NAN)], 0, quick, plants=[((129, 136), 0)], plant_value=NINF,
                        kernel="thin4"))
    # levels: a leaf of the Poisson tree (relaxed supernodes), inside a leaf-pair launch
    st = NP.structure("poisson")
    _, b = NP.poisson_pair(st)
    out.append(Case("levels", "poisson", [(b, 0, "diag", NAN)], 0, kernel="thin1+pair"))
    # complex Hermitian: the imaginary part of an off-diagonal entry, a real diagonal entry
    for storage in ("cx", "twin"):
        out.append(Case("complex", "cx", [((65, 71), 20, 40, NAN, "im")], 0, storage=storage))
        out.append(Case("complex", "cx", [((33, 136), 5, "diag", NAN)], 0, storage=storage))
    # +Inf on a diagonal: the weaker contract
    for flags in (0, 16):
        out.append(Case("inf", "deep", [((65, 71), 7, "diag", PINF)], flags, weak=True,
                        kernel="generic" if flags & NO_SMALL_FRONTS else "thin4"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def table():
    return tuple(_table())


def cases_of(group, flags=None, storage=None, key=None):
    return [c for c in table() if c.group == group and (flags is None or c.flags == int(flags))
            and (storage is None or c.storage == storage) and (key is None or c.key == key)]


def resident_case(front=(129, 136), col=64):
    """the factor of the resident checks and of the solves on a NaN factor: one NaN on a diagonal of "deep", flags 0"""
    return Case("resident", "deep", [(front, col, "diag", NAN)], 0)


# ---- values -------------------------------------------------------------------------------------------------------------

def _entry_of(key, k, j, i):
    """index into Ax of the stored (lower) entry of A that is entry (row i, column j) of supernode k"""
    M, st = NP.matrix(key), NP.structure(key)
    c = int(st.Perm[int(st.super[k]) + j])
    r = int(st.Perm[int(st.s[int(st.pi[k]) + i])])
    r, c = max(r, c), min(r, c)
    rows = M["Ai"][M["Ap"][c]:M["Ap"][c + 1]]
    p = int(np.searchsorted(rows, r))
    assert p < len(rows) and rows[p] == r, (key, k, j, i, "no such entry of A")
    return int(M["Ap"][c]) + p


def poisoned_values(c):
    """the case's values: plants on their diagonals, then the poisoned entries"""
    M, st = NP.matrix(c.key), NP.structure(c.key)
    Ax = M["Ax"].copy()
    for k in c.K:
        Ax[M["Ap"][int(st.Perm[k])]] = c.plant_value
    for k, j, i, v, part in c.P:
        p = _entry_of(c.key, k, j, i)
        Ax[p] = complex(Ax[p].real, VALUES[v]) if part == "im" else VALUES[v]
    return Ax


# ---- must and may ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def simplicial_pattern(key):
    """dense boolean lower triangle: the pattern of L without relaxed supernodes, in the permuted ordering"""
    M = NP.matrix(key)
    if M["norelax"]:
        S = NP.structure(key)
        sup, pi, s = S.super, S.pi, S.s
    else:
        O = NP.OracleFactor(M["n"], M["Ap"], M["Ai"], -1, perm=M["perm"], postorder=True, nrelax=[0, 0, 0], zrelax=[0.0, 0.0, 0.0])
        assert np.array_equal(O.Perm, NP.structure(key).Perm)
        sup, pi, s = np.array(O.super), np.array(O.pi), np.array(O.s)
    n = M["n"]
    pat = np.zeros((n, n), dtype=bool)
    for k in range(len(sup) - 1):
        rows = s[pi[k]:pi[k + 1]]
        for j in range(int(sup[k + 1] - sup[k])):
            pat[rows[j:], int(sup[k]) + j] = True
    assert np.all(np.diag(pat)) and not np.triu(pat, 1).any()
    pat.setflags(write=False)
    return pat


def boolean_cholesky(pat, nanA):
    """the must set, dense: nan (i, j) = nanA (i, j) or nan (j, j) or some k < j with (i, k), (j, k) on the pattern and one
    of them NaN -- column by column, left-looking, on the pattern only"""
    n = len(pat)
    assert not (nanA & ~pat).any()
    nan = np.zeros((n, n), dtype=bool)
    for j in range(n):
        ks = np.flatnonzero(pat[j, :j])
        if len(ks):
            rows = slice(j, n)
            hit = (pat[rows][:, ks] & (nan[rows][:, ks] | nan[j, ks])).any(axis=1)
        else:
            hit = np.zeros(n - j, dtype=bool)
        col = nanA[j:, j] | hit
        col |= col[0]                                   # nan (j, j)
        nan[j:, j] = col & pat[j:, j]
    return nan


def expected_minor(c):
    """(minor, must without the cut): a plant whose pivot is in must is NaN and does not trip; the smallest other one wins"""
    st = NP.structure(c.key)
    nanA = np.zeros((st.n, st.n), dtype=bool)
    for k, j, i, v, part in c.P:
        col, row = int(st.super[k]) + j, int(st.s[int(st.pi[k]) + i])
        nanA[max(row, col), min(row, col)] = True
    must = boolean_cholesky(simplicial_pattern(c.key), nanA)
    trip = [k for k in c.K if not must[k, k]]
    return (min(trip) if trip else st.n), must


@functools.lru_cache(maxsize=None)
def _sets(ref_key, key):
    c = _REG[ref_key]
    st = NP.structure(key)
    minor, must = expected_minor(c)
    sbad = st.supernode_of(minor) if minor < st.n else st.nsuper
    valid = minor if not (minor < st.n and c.quick) else int(st.super[sbad])
    must = must.copy()
    must[:, valid:] = False
    must_x = NP.read_on_pattern(st, must, st.n)
    on_path = np.zeros(st.nsuper, dtype=bool)
    for k in c.fronts:
        while k >= 0:
            on_path[k] = True
            k = int(st.sparent[k])
    # after a failure: the columns from `valid` on of the failing supernode and every later supernode, on the path or not
    zero_x = np.zeros(st.xsize, dtype=bool)
    if sbad < st.nsuper:
        zero_x[int(st.px[sbad]) + (valid - int(st.super[sbad])) * int(st.nsrow[sbad]):] = True
        zero_x &= st.mask
    may_x = np.repeat(on_path, np.diff(st.px)) & st.mask & ~zero_x
    assert not (must_x & ~may_x).any()
    # the failure comes in the poisoned supernode BEFORE its first poisoned column: nothing poisoned is ever read
    untouched = bool(c.P) and sbad < st.nsuper and all(k == sbad and minor < int(st.super[k]) + j for k, j, _, _, _ in c.P)
    for a in (must_x, may_x, zero_x, on_path):
        a.setflags(write=False)
    return dict(minor=minor, sbad=sbad, valid=valid, must=must_x, may=may_x, zero=zero_x, on_path=on_path, untouched=untouched)


def sets(c):
    """dict (minor, sbad: the failing supernode or nsuper, valid: the columns before it hold values, must / may: boolean over
    the supernodal layout, zero: the entries of the lower trapezoids that a failure leaves +0.0, on_path: boolean over the
    supernodes, untouched: the failure comes before anything poisoned is read -- nothing anywhere is non-finite)"""
    return _sets(c.ref_key, c.key)


# ---- the oracle --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle(ref_key, key):
    c = _REG[ref_key]
    O = NP.new_oracle(key)
    Ax = poisoned_values(c)
    cx = np.iscomplexobj(Ax)
    with np.errstate(all="ignore"):
        rc = O.factorize_complex(Ax, quick_return=c.quick) if cx else O.factorize(Ax, quick_return=c.quick)
    x = np.array(O.xc if cx else O.x)
    x.setflags(write=False)
    return rc, int(O.status), int(O.minor), x


def oracle_expectation(c):
    """(return value, status, minor, x) of the oracle for the case's values"""
    return _oracle(c.ref_key, c.key)


def clean_oracle(key):
    return NP.oracle_expectation(key, (), False)[3]


# ---- the contract ------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_contract(c, x, clean, tag, oracle_x=None, dead=True):
    """x: the factor of the case's values, clean: the SAME implementation's factor of the clean values, oracle_x: the
    oracle's factor of the case's values (None: x is the oracle's) -> dict (must, may, nonfinite: entry counts)"""
    st, S = NP.structure(c.key), sets(c)
    x, clean = np.asarray(x), np.asarray(clean)
    assert x.shape == clean.shape == (st.xsize,), (tag, x.shape, clean.shape)
    nf = ~np.isfinite(x)
    if dead:
        assert np.all(x[~st.mask] == 0), (tag, "dead upper triangle written", int((x[~st.mask] != 0).sum()))
    nf = nf & st.mask
    over = np.flatnonzero(nf & ~S["may"])
    if len(over):
        sn = np.searchsorted(st.px, over[0], side="right") - 1
        raise AssertionError(f"{tag}: {len(over)} non-finite entries outside may, the first in supernode {sn} "
                             f"(columns {st.super[sn]} .. {st.super[sn + 1] - 1}, entry {over[0] - st.px[sn]})")
    if not c.weak:
        miss = np.flatnonzero(S["must"] & ~nf)
        if len(miss):
            sn = np.searchsorted(st.px, miss[0], side="right") - 1
            raise AssertionError(f"{tag}: {len(miss)} must-entries are finite, the first in supernode {sn} "
                                 f"(columns {st.super[sn]} .. {st.super[sn + 1] - 1}, entry {miss[0] - st.px[sn]}): "
                                 f"{x[miss[0]]!r}")
    if S["untouched"]:
        assert not nf.any(), (tag, f"{int(nf.sum())} non-finite entries, and the failing pivot comes before the poisoned column")
    # after the failure, on the path or not: +0.0, as bits
    z = np.flatnonzero(S["zero"])
    notzero = (bits(x).reshape(st.xsize, -1)[z] != 0).any(axis=1)
    if notzero.any():
        sn = np.searchsorted(st.px, z[notzero][0], side="right") - 1
        raise AssertionError(f"{tag}: {int(notzero.sum())} entries after the failure are not +0.0, the first in supernode {sn} "
                             f"(columns {st.super[sn]} .. {st.super[sn + 1] - 1}, entry {z[notzero][0] - st.px[sn]}): "
                             f"{x[z[notzero][0]]!r}")
    # outside may, before the failing supernode: the bits of the clean factor
    for k in range(min(S["sbad"], st.nsuper)):
        if S["on_path"][k]:
            continue
        sl = slice(int(st.px[k]), int(st.px[k + 1]))
        same = bits(x[sl]) == bits(clean[sl])
        if dead is False:
            same = same | ~np.repeat(st.mask[sl], same.size // (sl.stop - sl.start))
        assert same.all(), (tag, f"supernode {k} (columns {st.super[k]} .. {st.super[k + 1] - 1}) outside may is not "
                                 f"the clean bits: {int((~same).sum())} words differ")
    # where both are finite: the oracle's zero pattern and values
    if oracle_x is not None:
        look = st.mask & np.isfinite(x) & np.isfinite(oracle_x)
        if c.weak:
            look &= ~S["may"]
        bad = np.flatnonzero(((x != 0) != (oracle_x != 0)) & look)
        assert not len(bad), (tag, f"zero pattern differs from the oracle's at {len(bad)} finite entries, the first {bad[:3]}")
        d = np.where(look, np.abs(np.where(look, x, 0) - np.where(look, oracle_x, 0)), 0.0)
        r = np.where(look, np.abs(np.where(look, oracle_x, 0)), 0.0)
        num, den = np.maximum.reduceat(d, st.px[:-1]), np.maximum.reduceat(r, st.px[:-1])
        assert not np.any((den == 0) & (num != 0)), tag
        e = float((num[den > 0] / den[den > 0]).max(initial=0.0))
        assert e < TOL_L, (tag, "finite entries against the oracle, by entry", e)
    return dict(must=int(S["must"].sum()), may=int(S["may"].sum()), nonfinite=int(nf.sum()))


# ---- solves and residual (natural ordering) ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def etree(key):
    """(parent: first row below the diagonal of every column of L, -1 for a root; root_of: the root of every column's tree)"""
    pat = simplicial_pattern(key)
    n = len(pat)
    parent = np.full(n, -1, dtype=np.int64)
    for j in range(n):
        below = np.flatnonzero(pat[j + 1:, j])
        if len(below):
            parent[j] = j + 1 + below[0]
    root_of = np.arange(n)
    for j in range(n - 1, -1, -1):
        if parent[j] >= 0:
            root_of[j] = root_of[parent[j]]
    return parent, root_of


def solve_sets(key, rows, sys):
    """(must, may): boolean over the rows of the solution, for NaN in the rows `rows` of the right-hand side under sys "A",
    "L" or "Lt".  SYS_A solves with A: its rows are rows of A, taken through Perm and back; SYS_L and SYS_Lt solve with the
    factor as it stands: their rows are columns of L.  (A solve on a NaN factor: rows_of_columns gives the rows of A
    that stand for the columns of L that hold a NaN.)"""
    st = NP.structure(key)
    parent, root_of = etree(key)
    must, may = np.zeros(st.n, dtype=bool), np.zeros(st.n, dtype=bool)
    if sys == "A":
        inv = np.empty(st.n, dtype=np.int64)
        inv[st.Perm] = np.arange(st.n)
        rows = inv[np.asarray(rows, dtype=np.int64)]
    for i in rows:
        if sys == "L":
            j = int(i)
            while j >= 0:
                must[j] = True
                k = st.supernode_of(j)
                may[st.super[k]:st.super[k + 1]] = True
                j = int(parent[j])
        elif sys == "A":
            must |= root_of == root_of[int(i)]
        else:
            must[int(i)] = True
    if sys == "Lt":
        # back substitution: x (j) reads x (i) for every i > j with (i, j) on the pattern
        pat = simplicial_pattern(key)
        for j in range(st.n - 1, -1, -1):
            must[j] |= bool((pat[j + 1:, j] & must[j + 1:]).any())
        for k in range(st.nsuper):
            if must[st.super[k]:st.super[k + 1]].any() or must[st.s[st.pi[k]:st.pi[k + 1]]].any():
                may[st.super[k]:st.super[k + 1]] = True
        return must, may
    if sys == "A":
        out = np.zeros(st.n, dtype=bool)
        out[st.Perm] = must
        return out, out.copy()
    return must, may


def rows_of_columns(key, cols):
    """the rows of A that the columns `cols` of L stand for"""
    return NP.structure(key).Perm[np.asarray(cols, dtype=np.int64)]


def reproducible_rows(key, sys):
    """boolean over the rows of a solution: the rows whose BITS two calls on the same inputs share.  The forward solves add
    the contributions of sibling supernodes into their common ancestor rows with floating-point atomics, in the order the
    workgroups happen to arrive (solve_kernels.hip.h: k_lsolve, k_sd_lsolve), so a row that a sum over two or more children
    reaches -- and under SYS_A, which goes back down, its whole tree -- is reproducible only to rounding.  Measured on one
    MI355X, "deep", 20 repeats of one clean call: up to 23 words of a 16-wide SYS_L panel differ, all in root rows.
    The backward solve of a supernode of at most 256 columns sums in a fixed order: SYS_Lt is reproducible everywhere."""
    st = NP.structure(key)
    assert st.nscol.max() <= 256
    if sys == "Lt":
        return np.ones(st.n, dtype=bool)
    ok = np.bincount(st.sparent[st.sparent >= 0], minlength=st.nsuper) <= 1
    for k in range(st.nsuper):                          # (postordered) ... and every supernode below it
        if st.sparent[k] >= 0 and not ok[k]:
            ok[st.sparent[k]] = False
    if sys == "A":
        for k in range(st.nsuper - 1, -1, -1):          # the whole tree: what the root is
            if st.sparent[k] >= 0:
                ok[k] = ok[st.sparent[k]]
    rows = np.repeat(ok, st.nscol)
    if sys == "A":
        out = np.zeros(st.n, dtype=bool)
        out[st.Perm] = rows
        return out
    return rows


def residual_rows(key, k):
    """rows of R = B - A X that are NaN for X NaN in row k: k and the rows j with A (j, k) on the pattern"""
    M = NP.matrix(key)
    n = M["n"]
    col = np.repeat(np.arange(n), np.diff(M["Ap"]))
    out = np.zeros(n, dtype=bool)
    out[k] = True
    out[M["Ai"][col == k]] = True
    out[col[M["Ai"] == k]] = True
    return out
