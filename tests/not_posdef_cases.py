"""The case table of the not-positive-definite protocol with SEVERAL failing pivots, and its two references.  numpy, scipy
and the CPU oracle only: no torch, no GPU (tests/test_not_posdef_cases.py pins the table on the CPU,
tests/not_posdef_device_cases.py runs it on the device).

A case is a matrix, a set K of planted columns (columns of the PERMUTED matrix: the diagonal entry of column Perm [k] of A
is set to -7.0, as tests/test_gpu_parity.py plants its one pivot), plan flags and quick_return_if_not_posdef.  A plant
cannot disturb the leading principal block before it, and a leading block that holds a negative diagonal entry is not
positive definite: the expected minor is min (K), whatever the other plants are.

Two expectations per case.  The oracle (OracleFactor.factorize / factorize_complex with quick_return) gives minor, the
values and the zero pattern.  The DENSE RESTATEMENT (dense_expectation) is independent of oracle and engine; it restates

    engine.hip:  *minor = f.k1 + binfo - 1 ;   i64 first_zero = sbad + ((binfo == 1 || quick) ? 0 : 1) ;

(t_cholmod_super_numeric.c:905-968) on the dense permuted matrix B = P A P' with m = min (K), sbad the supernode that
holds column m and info = m - super [sbad] + 1:

    L (:, 0 .. m-1) = [ chol (B (0..m-1, 0..m-1)) ; B (m.., 0..m-1) inv (chol (...))' ]   (np.linalg.cholesky and one
                                                                                            triangular solve)
    every column of a supernode before sbad holds those values on its supernodal pattern;
    in sbad the columns before m hold them -- none under quick return (and none if info == 1: there are none);
    everything else is +0.0: the columns of sbad from m on, every later supernode, the dead upper triangles.

The bar: by entry, max |L - L_ref| over a supernode / max |L_ref| of that supernode, the worst supernode, below
TOL_L = 1e-12 (tests/test_gpu_parity.py).  The reference pair alone stays below a tenth of it (test_not_posdef_cases.py)."""
import functools
import os
import sys

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import device_fuzz_corpus as DC  # noqa: E402
from oracle.oracle import OracleFactor  # noqa: E402
from suitesparse_amd import generators as G  # noqa: E402

TOL_L = 1e-12               # tests/test_gpu_parity.py
PLANT = -7.0
ROOT = (DC.ARROW_ROOT, 0)   # the root of a block arrow, as a (width, below-rows) pair

# block arrows: (width, below-rows) of the leaves.  The postorder sorts the leaves by their below-rows (a leaf hangs on
# root column 140 - r), ties in the order given: (5, 137) is what makes a leaf LATER than (129, 136) exist.
LEAVES = {
    "two": [(17, 72), (64, 72), (65, 71), (129, 136), (16, 0), (1, 1)],
    "deep": [(17, 72), (64, 72), (65, 71), (129, 136), (16, 0), (1, 1), (5, 137)],
    "thin": [(1, 1), (15, 63), (16, 64), (64, 72)],        # one K_SMALL launch of aux 136: the four-wave k_thin_front
    "pair": [(1, 1), (4, 8), (12, 20), (16, 16)],           # every leaf <= 32 rows, <= 16 columns: k_leaf_pair (values-only)
    "cx": [(17, 72), (65, 71), (33, 136)],
}
SEEDS = {"cx": 20, "deep": 21, "thin": 22, "two": 23, "pair": 24}
POISSON = 24                # G.poisson2d (24) under G.geometric_nd (24, 24, 1, 4): 576 columns, 7 levels

# launch kinds of the schedule (plan.hip.h, enum Kind)
K_POTRF, K_TRSM, K_SMALL, K_UPD_PF, K_TRSM_UPD, K_DIAG, K_ROWSOLVE, K_CHAINF = 2, 3, 8, 9, 10, 13, 14, 16
# the thin fronts of the FACTORIZATION, restated: plan_build.hip:322 (a front is thin on nsrow <= SM_MAX alone, unless
# CHOLMOD_HIP_NO_SMALL_FRONTS), :631 the size classes of schedule_thin, :644 a class of fewer than 256 fronts rides with the
# next larger one that has any, :687 leaf pairs; engine.hip:276 .. 291 which kernel a K_SMALL launch becomes
NO_SMALL_FRONTS, NO_LEAF_PAIRS = 16, 4096
SM_MAX, THIN_CLASSES, THIN_FILL = 136, (32, 48, 64, 96, 136), 256


# ---- matrices -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def matrix(key):
    """-> dict (n, Ap, Ai, Ax: lower CSC with the diagonal entry first in every column, perm: None = natural, norelax)"""
    if key == "poisson":
        n, Ap, Ai, Ax = G.poisson2d(POISSON)
        return dict(n=n, Ap=Ap, Ai=Ai, Ax=np.asarray(Ax, dtype=np.float64), perm=G.geometric_nd(POISSON, POISSON, 1, 4), norelax=False)
    rng = np.random.default_rng(SEEDS[key])
    n, Ap, Ai, Ax = DC.block_arrow(rng, LEAVES[key])
    if key == "cx":
        # Hermitian phases on the off-diagonal entries, a real diagonal (solve_device_complex_cases._big_supernode_matrix)
        ph = np.tril(np.exp(1j * rng.uniform(0, 2 * np.pi, (n, n))), -1)
        ph = ph + ph.conj().T + np.eye(n)
        Ax = Ax * ph[Ai, np.repeat(np.arange(n), np.diff(Ap))]
    assert np.array_equal(Ai[Ap[:-1]], np.arange(n))
    return dict(n=n, Ap=Ap, Ai=Ai, Ax=Ax, perm=None, norelax=True)


def new_oracle(key):
    M = matrix(key)
    kw = dict(nrelax=[0, 0, 0], zrelax=[0.0, 0.0, 0.0]) if M["norelax"] else {}
    return OracleFactor(M["n"], M["Ap"], M["Ai"], -1, perm=M["perm"], postorder=True, **kw)


class Structure:
    """the supernodal structure of a matrix of the table (copies: no view into an oracle object survives)"""

    def __init__(self, key):
        O = new_oracle(key)
        for k in ("Perm", "super", "pi", "px", "s"):
            setattr(self, k, np.array(getattr(O, k)))
        self.n, self.nsuper, self.xsize = int(O.n), int(O.nsuper), int(O.xsize)
        self.mask = O.lower_mask().copy()
        self.sparent = np.array(O.sparent())
        self.level = levels_of(self.sparent)
        self.nscol, self.nsrow = np.diff(self.super), np.diff(self.pi)

    def supernode_of(self, col):
        return int(np.searchsorted(self.super, col, side="right") - 1)

    def front(self, shape):
        """the supernode that is the leaf (w, r) -- or the root, ROOT -- of a block arrow"""
        w, r = shape
        hit = [k for k in range(self.nsuper) if (int(self.nscol[k]), int(self.nsrow[k])) == (w, w + r)]
        assert len(hit) == 1, (shape, hit)
        return hit[0]


def levels_of(sparent):
    """level 0: a leaf; a parent is one above its highest child (what cholmod_hip_get_maps reports)"""
    level = np.zeros(len(sparent), dtype=np.int64)
    for k in range(len(sparent)):                       # (postordered: children come before their parent)
        if sparent[k] >= 0:
            assert sparent[k] > k
            level[sparent[k]] = max(level[sparent[k]], level[k] + 1)
    return level


@functools.lru_cache(maxsize=None)
def structure(key):
    return Structure(key)


def poisson_pair(st):
    """(a, b): a the first supernode at level >= 2 with two columns or more, b the first leaf of ANOTHER subtree that
    comes after it (postordered: every descendant of a comes before a).  The leaf runs in the first batch, long before a."""
    for a in range(st.nsuper):
        if st.level[a] >= 2 and st.nscol[a] >= 2:
            for b in range(a + 1, st.nsuper):
                if st.level[b] == 0 and st.super[b] > st.super[a + 1]:
                    anc = b
                    while anc >= 0 and anc != a:
                        anc = int(st.sparent[anc])
                    assert anc < 0                      # a is no ancestor of b
                    return a, b
    raise AssertionError("no (a, b) pair in the Poisson case")


# ---- the table ----------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, group, key, plants, flags, quick, storage=None, classes=(), kernel=None):
        """plants: ((width, below-rows) of a front of the arrow | a supernode index, column within it) ...;
        classes: device_fuzz_corpus.front_classes names the FIRST planted front must reach (the shapes of the selected
        inverse's sweeps, NOT the factorization's kernels); kernel: what factor_kernel says of the first planted front under
        the case's flags, the kernel that meets the winning pivot"""
        st = structure(key)
        self.group, self.key, self.flags, self.quick, self.storage = group, key, int(flags), bool(quick), storage
        self.fronts = [st.front(f) if isinstance(f, tuple) else int(f) for f, _ in plants]
        for k, (_, j) in zip(self.fronts, plants):
            assert 0 <= j < st.nscol[k], (plants, k, j)
        self.K = tuple(int(st.super[k]) + j for k, (_, j) in zip(self.fronts, plants))
        self.minor = min(self.K)
        self.sbad = st.supernode_of(self.minor)
        self.info = self.minor - int(st.super[self.sbad]) + 1
        self.classes, self.kernel = tuple(classes), kernel
        tag = "+".join(f"{'x'.join(map(str, f)) if isinstance(f, tuple) else 's' + str(f)}@{j}" for f, j in plants)
        self.name = f"{group}:{key}:{tag}:f{self.flags}:{'quick' if quick else 'full'}" + (f":{storage}" if storage else "")

    # the (matrix, plants, quick) of a case: what the CPU references depend on
    ref_key = property(lambda c: (c.key, c.K, c.quick))


DEEP_FLAGS = [0, 512 | 1024, 8192, 16, 4 | 128]
THIN_FLAGS = [0, NO_LEAF_PAIRS]


def _table():
    out = []
    for quick in (False, True):
        # two leaves fail: the postorder of "two" is (16, 0) (1, 1) (65, 71) (17, 72) (64, 72) (129, 136) root
        for plants in ([((65, 71), 32), ((129, 136), 0)],           # middle of an early leaf, column 0 (info == 1) of a later one
                       [((17, 72), 0), ((64, 72), 32)],             # swapped: info == 1 in the first failing leaf
                       [((16, 0), 8), ((17, 72), 0)],               # the early leaf is a tree of its own
                       [((65, 71), 32), ((129, 136), 0), (ROOT, 70)]):  # ... and a third plant in the root
            out.append(Case("two", "two", plants, 0, quick, kernel="thin4"))   # (one launch holds the five thin leaves: aux 136)
        # deep in a generic leaf that has rows below, a second plant in the later leaf (5, 137)
        for flags in DEEP_FLAGS:
            for j in (63, 64, 65, 128):
                out.append(Case("deep", "deep", [((129, 136), j), ((5, 137), 2)], flags, quick,
                                classes=("gen_blocks3+", "gen_ragged_block", "gen_partial_slice"), kernel="generic"))
            # (65 + 71 = 136 rows: the factorization takes this leaf as a THIN front, four waves, unless flag 16 forbids it)
            for j in (64, 1):
                out.append(Case("deep", "deep", [((65, 71), j), ((5, 137), 0)], flags, quick,
                                classes=("gen_blocks2", "gen_w65", "gen_partial_slice"),
                                kernel="generic" if flags & NO_SMALL_FRONTS else "thin4"))
        # the root only: every leaf intact
        for j in (0, 63, 64, 139):
            out.append(Case("root", "two", [(ROOT, j)], 0, quick, classes=("gen_blocks3+", "gen_norows"), kernel="generic"))
        # thin fronts: first, a middle and the last column of two leaves at once.  These four leaves share one launch whose
        # widest member has 136 rows: the four-wave k_thin_front on every value path, with and without flag 4096
        for flags in THIN_FLAGS:
            for ja, jb in ((0, 0), (7, 31), (14, 63)):
                out.append(Case("thin", "thin", [((15, 63), ja), ((64, 72), jb)], flags, quick, classes=("thin_lds1",), kernel="thin4"))
            for jb in (0, 8, 15):
                out.append(Case("thin", "thin", [((1, 1), 0), ((16, 64), jb)], flags, quick, classes=("thin_lds0",), kernel="thin4"))
        # leaf pairs: every leaf of "pair" has <= 32 rows and <= 16 columns, so the values-only paths run k_leaf_pair (two
        # fronts to a wave: supernodes 0 | 1 and 2 | 3) and the first factorization -- every path under flag 4096 -- the
        # one-wave k_thin_front.  The two failing fronts in different waves, then in one wave
        for flags in THIN_FLAGS:
            kern = "thin1" if flags & NO_LEAF_PAIRS else "thin1+pair"
            for ja, jb in ((0, 0), (2, 8), (3, 15)):
                out.append(Case("pair", "pair", [((4, 8), ja), ((16, 16), jb)], flags, quick, classes=("thin_lds0",), kernel=kern))
            for jb in (0, 6, 11):
                out.append(Case("pair", "pair", [((1, 1), 0), ((12, 20), jb)], flags, quick, classes=("thin_lds0",), kernel=kern))
            out.append(Case("pair", "pair", [((1, 1), 0), ((4, 8), 2)], flags, quick, classes=("thin_lds0",), kernel=kern))
            out.append(Case("pair", "pair", [((16, 16), 15), ((12, 20), 0)], flags, quick, classes=("thin_lds0",), kernel=kern))
        # levels: a small column high in one subtree, a larger one in a leaf of another
        st = structure("poisson")
        a, b = poisson_pair(st)
        out.append(Case("levels", "poisson", [(a, 1), (b, 0)], 0, quick, kernel="thin1"))
        # complex Hermitian, in complex storage and as the full twin
        for storage in ("cx", "twin"):
            out.append(Case("complex", "cx", [((65, 71), 64), ((33, 136), 0)], 0, quick, storage=storage,
                            classes=("gen_blocks2", "gen_w65")))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=None)
def table():
    return tuple(_table())


def cases_of(group, flags=None, quick=None, storage=None):
    return [c for c in table() if c.group == group and (flags is None or c.flags == int(flags))
            and (quick is None or c.quick == bool(quick)) and (storage is None or c.storage == storage)]


# ---- values and references ----------------------------------------------------------------------------------------------

def planted_values(key, K):
    M, st = matrix(key), structure(key)
    Ax = M["Ax"].copy()
    for k in K:
        Ax[M["Ap"][int(st.Perm[k])]] = PLANT            # the diagonal entry of that column
    return Ax


def dense_permuted(key, Ax):
    M, st = matrix(key), structure(key)
    n = M["n"]
    Lo = sp.csc_matrix((Ax, M["Ai"], M["Ap"]), shape=(n, n)).toarray()
    F = Lo + np.tril(Lo, -1).conj().T
    return F[np.ix_(st.Perm, st.Perm)]


def read_on_pattern(st, Ld, ncols):
    """columns 0 .. ncols-1 of the dense lower-triangular Ld on the supernodal pattern of st, +0.0 everywhere else"""
    x = np.zeros(st.xsize, dtype=Ld.dtype)
    for k in range(st.nsuper):
        k1, nscol, nsrow = int(st.super[k]), int(st.nscol[k]), int(st.nsrow[k])
        rows = st.s[st.pi[k]:st.pi[k + 1]]
        for j in range(min(nscol, ncols - k1)):
            x[st.px[k] + j * nsrow + j:st.px[k] + (j + 1) * nsrow] = Ld[rows[j:], k1 + j]
    return x


@functools.lru_cache(maxsize=None)
def dense_expectation(key, K, quick):
    """(minor, x): the module's docstring.  K empty: the whole factor of the positive definite matrix."""
    st = structure(key)
    B = dense_permuted(key, planted_values(key, K))
    m = min(K) if K else st.n
    Ld = np.zeros_like(B)
    if m > 0:
        Ld[:m, :m] = np.linalg.cholesky(B[:m, :m])
        if m < st.n:
            Ld[m:, :m] = sla.solve_triangular(Ld[:m, :m], B[m:, :m].conj().T, lower=True).conj().T
    sbad = st.supernode_of(m) if K else st.nsuper
    valid = m if not (K and quick) else int(st.super[sbad])
    x = read_on_pattern(st, Ld, valid)
    x.setflags(write=False)
    return m, x


@functools.lru_cache(maxsize=None)
def oracle_expectation(key, K, quick):
    """(return value, status, minor, x) of the oracle for the planted values (K empty: the positive definite ones)"""
    O = new_oracle(key)
    Ax = planted_values(key, K)
    cx = np.iscomplexobj(Ax)
    rc = O.factorize_complex(Ax, quick_return=quick) if cx else O.factorize(Ax, quick_return=quick)
    x = np.array(O.xc if cx else O.x)
    x.setflags(write=False)
    return rc, int(O.status), int(O.minor), x


def by_entry(st, x, ref):
    """the bar's figure: over the lower trapezoids, max |x - ref| of a supernode / max |ref| of that supernode, the worst
    supernode.  A supernode whose reference is all zero must be all zero: inf otherwise."""
    d = np.where(st.mask, np.abs(np.asarray(x) - ref), 0.0)
    r = np.where(st.mask, np.abs(ref), 0.0)
    num, den = np.maximum.reduceat(d, st.px[:-1]), np.maximum.reduceat(r, st.px[:-1])
    if np.any((den == 0) & (num != 0)):
        return float("inf")
    return float((num[den > 0] / den[den > 0]).max(initial=0.0))


def check_factor(st, x, ref, tag, dead=True):
    """the zero pattern of x over the lower trapezoids is exactly that of ref, the dead upper triangles are zero (dead=False:
    not looked at -- the oracle's repeat pass leaves values there, and nobody reads them); returns by_entry (x, ref)"""
    x = np.asarray(x)
    assert x.shape == ref.shape, (tag, x.shape, ref.shape)
    assert not dead or np.all(x[~st.mask] == 0), (tag, "dead upper triangle written")
    want = ref != 0
    bad = np.flatnonzero(((x != 0) != want) & st.mask)
    if len(bad):
        sn = np.searchsorted(st.px, bad[0], side="right") - 1
        raise AssertionError(f"{tag}: zero pattern differs at {len(bad)} entries, the first in supernode {sn} "
                             f"(columns {st.super[sn]} .. {st.super[sn + 1] - 1}): expected {'a value' if want[bad[0]] else 'zero'}")
    return by_entry(st, x, ref)


def front_classes_of(st, k):
    """device_fuzz_corpus.front_classes of supernode k alone"""
    rows = st.s[st.pi[k]:st.pi[k + 1]]
    return DC.front_classes([int(st.super[k]), int(st.super[k + 1])], [0, len(rows)], rows)


@functools.lru_cache(maxsize=None)
def launch_profile(key, flags):
    """(launches: ((kind, grid, aux), ...), batch_of) of a schedule-only plan (CHOLMOD_HIP_PLAN_HOST_ONLY: no device is
    touched) of the matrix's supernodes under `flags`"""
    import ctypes as C
    from suitesparse_amd import cholmod as ch
    st = structure(key)
    L = ch.lib()
    sup, pi, px, s = (np.ascontiguousarray(a, dtype=np.int64) for a in (st.super, st.pi, st.px, st.s))
    rc = C.c_int(0)
    P = L.cholmod_hip_plan_create(st.n, st.nsuper, sup.ctypes.data, pi.ctypes.data, px.ctypes.data, s.ctypes.data,
                                  int(flags) | ch.HIP_PLAN_HOST_ONLY, C.byref(rc))
    assert P and rc.value == 0
    nl = L.cholmod_hip_get_launch_profile(P, 0, None, None, None, None, None, None)
    kind, grid, aux = (np.zeros(nl, dtype=np.int32) for _ in range(3))
    L.cholmod_hip_get_launch_profile(P, nl, kind.ctypes.data, grid.ctypes.data, aux.ctypes.data, None, None, None)
    batch = np.zeros(st.nsuper, dtype=np.int64)
    L.cholmod_hip_get_batches(P, batch.ctypes.data, None)
    L.cholmod_hip_plan_destroy(P)
    return tuple(zip(kind.tolist(), grid.tolist(), aux.tolist())), tuple(batch.tolist())


def launch_kinds(key, flags):
    """the launch kinds of that plan"""
    return set(k for k, _, _ in launch_profile(key, flags)[0])


def thin_launches(key, flags):
    """the K_SMALL launches of the plan, RESTATED from the structure and the batches (see THIN_CLASSES above), in schedule
    order: [dict (members, aux: rows of the widest member, pair: k_leaf_pair on the values-only paths)].
    test_not_posdef_cases.py holds (members, aux) against the launches the plan reports."""
    st, batch = structure(key), np.asarray(launch_profile(key, flags)[1])
    parents = set(int(p) for p in st.sparent if p >= 0)
    out = []
    for b in sorted(set(batch.tolist())):
        bucket = [[] for _ in THIN_CLASSES]
        for k in np.flatnonzero(batch == b):
            if not (flags & NO_SMALL_FRONTS) and st.nsrow[k] <= SM_MAX:
                bucket[int(np.searchsorted(THIN_CLASSES, st.nsrow[k]))].append(int(k))
        for c in range(len(THIN_CLASSES) - 1):
            up = next((u for u in range(c + 1, len(THIN_CLASSES)) if bucket[u]), None)
            if bucket[c] and len(bucket[c]) < THIN_FILL and up is not None:
                bucket[up], bucket[c] = sorted(bucket[up] + bucket[c]), []
        for members in bucket:
            if members:
                aux = int(st.nsrow[members].max())
                pair = (not (flags & NO_LEAF_PAIRS) and not parents & set(members) and aux <= 32
                        and int(st.nscol[members].max()) <= 16)
                out.append(dict(members=members, aux=aux, pair=pair))
    return out


def factor_kernel(key, flags, k):
    """the kernel that factorizes supernode k of a REAL matrix on one GPU: "generic" (the potrf / trsm / update launches or
    the 256-column chain), "thin4" / "thin1" (k_thin_front, four waves per front when the widest member of its launch
    has more than 64 rows, one otherwise), "thin1+pair" (k_leaf_pair on the values-only paths, the one-wave k_thin_front
    on the first factorization of the plan)"""
    for ln in thin_launches(key, flags):
        if k in ln["members"]:
            return "thin4" if ln["aux"] > 64 else "thin1+pair" if ln["pair"] else "thin1"
    return "generic"
