"""The seeded random corpus of the device fuzz (tests/test_device_fuzz_corpus.py without a GPU, tests/device_fuzz_runner.py
with one) and the map from a factor to the dispatch classes its fronts reach in the two backward sweeps and in the device
solves.  No torch, no GPU.

corpus (seed, ncase) yields fully determined cases: everything random comes from the one np.random.default_rng (seed), in a
fixed order, so a case number reproduces the case.  Kinds rotate with the case number, as tests/fuzz_runner.py rotates its
own (KINDS): Poisson 3D and 2D, banded and general rand_spd (diagonally dominant, always positive definite), a block arrow
with engineered front shapes, an unsymmetric A for M = A A' + beta I, and a complex Hermitian matrix on one of the real
patterns.  n <= 700 everywhere: the dense float64 references are what make the checks strong."""
import ctypes as C
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from fuzz_runner import rand_spd  # noqa: E402
from suitesparse_amd import generators as G  # noqa: E402

SEEDS = (3, 11)         # what tests/test_gpu_device_fuzz.py runs and tests/test_device_fuzz_corpus.py measures
NCASE = 40
NMAX = 700

KINDS = ("poisson3d", "poisson2d", "banded", "general", "arrow", "general", "aat", "complex")
REAL_KINDS = ("poisson3d", "poisson2d", "banded", "general", "arrow")
HIP_FLAGS = [0, 0, 0, 16, 512 | 1024, 8192, 4096]
NRHS = [1, 3, 7, 8, 15, 16, 17, 33]
ARROW_WIDTHS = [1, 15, 16, 17, 63, 64, 65, 128, 129]
ARROW_BELOW = [0, 1, 63, 64, 65, 71, 72, 73, 128, 135, 136]
ARROW_ROOT = 140
BETA = 0.375

CLASSES = ("thin_lds0", "thin_lds1", "thin_lds2", "thin_norows", "thin_1x1", "thin_w64", "thin_r136",
           "gen_blocks1", "gen_blocks2", "gen_blocks3+", "gen_ragged_block", "gen_exact_block",
           "gen_norows", "gen_partial_slice", "gen_exact_slice", "gen_multi_slice", "gen_tall_narrow", "gen_w65",
           "anc2+", "anc4+", "solve_big_walk")

# ---- the thresholds, restated -----------------------------------------------------------------------------------------
SI_NB = 64                  # sweep_device.hip.h:10  #define SI_NB 64 (column block of the recurrence)
SM_MAX = 136                # descriptors.hip.h:132  #define SM_MAX 136
THIN_LDS = (2048, 8192)     # selinv.hip:49          cls_doubles [3] = {2048, 8192, 1 << 30} (thin_launches)
SOLVE_BIG_COLS = 256        # descriptors.hip.h:157  #define SOLVE_BIG_COLS 256
SOLVE_BIG_ENTRIES = 1 << 16  # plan_build.hip:555    f.nscol > SOLVE_BIG_COLS || nsrow * nscol > (1 << 16)


def si_thin_lds(nscol, nsrow):
    """sweep_device.hip.h:127  doubles of LDS a thin front needs"""
    ncb = nsrow - nscol
    return (ncb | 1) * (ncb + nscol) + (nscol | 1) * nscol


def front_classes(sup, pi, s):
    """the set of class names (CLASSES) the supernodal factor (super, pi, s) reaches"""
    sup, pi, s = np.asarray(sup), np.asarray(pi), np.asarray(s)
    out = set()
    for k in range(len(sup) - 1):
        nscol, nsrow = int(sup[k + 1] - sup[k]), int(pi[k + 1] - pi[k])
        ncb = nsrow - nscol
        if nscol <= SI_NB and nsrow <= SM_MAX:          # selinv.hip:33  is_thin
            need = si_thin_lds(nscol, nsrow)            # selinv.hip:57 .. 58  the LDS class of thin_launches
            out.add("thin_lds0" if need <= THIN_LDS[0] else "thin_lds1" if need <= THIN_LDS[1] else "thin_lds2")
            if ncb == 0:
                out.add("thin_norows")
            if nsrow == 1:
                out.add("thin_1x1")
            if nscol == SI_NB:
                out.add("thin_w64")
            if nsrow == SM_MAX:
                out.add("thin_r136")
        else:
            nblk = (nscol + SI_NB - 1) // SI_NB         # selinv.hip:34  nblocks
            out.add("gen_blocks1" if nblk == 1 else "gen_blocks2" if nblk == 2 else "gen_blocks3+")
            out.add("gen_exact_block" if nscol % SI_NB == 0 else "gen_ragged_block")
            if ncb == 0:
                out.add("gen_norows")
            for b in range(nblk):                       # selinv.hip:107 .. 108  b0, nb, nR, ns of a step
                b0 = b * SI_NB
                nR = nsrow - b0 - min(SI_NB, nscol - b0)
                if nR > 0:
                    out.add("gen_exact_slice" if nR % 64 == 0 else "gen_partial_slice")
                    if nR > 64:
                        out.add("gen_multi_slice")
            if nscol <= SI_NB:
                out.add("gen_tall_narrow")
            if nscol == SI_NB + 1:
                out.add("gen_w65")
        if ncb > 0:                                     # sweep_device.hip.h:41  si_locate in the owners' panels
            owners = np.unique(np.searchsorted(sup, s[pi[k] + nscol:pi[k + 1]], side="right") - 1)
            if len(owners) >= 2:
                out.add("anc2+")
            if len(owners) >= 4:
                out.add("anc4+")
        if nscol > SOLVE_BIG_COLS or nsrow * nscol > SOLVE_BIG_ENTRIES:
            out.add("solve_big_walk")
    return out


def sweep_program(sup, pi, batch_of, budget_mb):
    """(chunks, launches) of the launch program the two backward sweeps share, under a scratch budget in MB (None: the
    default of 2048), restated from selinv.hip: scratch_budget and scratch_of (lines 26 .. 36) and Builder::build (134 ..
    149) -- per batch the generic fronts, widest first, a new chunk wherever the budget falls, then the thin fronts --,
    Builder::chunk (96 .. 124) -- one fill launch if a front of the chunk has below-rows, per block step a block launch if
    a front has rows after that block and a diagonal launch, one store launch -- and thin_launches (47 .. 65) -- one launch
    per LDS class that has a front.  The selected inverse reports `launches` (selinv.hip:204), the factor gradient one
    more (factor_grad.hip:89): a front that takes another path than front_classes says moves these counts."""
    budget = int(max(float(budget_mb) if budget_mb is not None else 2048.0, 0.0) * 1048576.0 / 8.0)
    sup, pi, batch_of = np.asarray(sup), np.asarray(pi), np.asarray(batch_of)
    nscol, nsrow = np.diff(sup).astype(np.int64), np.diff(pi).astype(np.int64)
    thin = (nscol <= SI_NB) & (nsrow <= SM_MAX)
    nchunks = launches = 0
    for b in np.unique(batch_of):
        ids = np.flatnonzero(batch_of == b)
        generic = sorted((int(k) for k in ids if not thin[k]), key=lambda k: -nscol[k])         # (stable, as std::stable_sort)
        chunks, cur, used = [], [], 0
        for k in generic:
            need = int(nsrow[k] * nsrow[k] + (nsrow[k] + 63) // 64 * SI_NB * SI_NB)
            if cur and used + need > budget:
                chunks.append(cur)
                cur, used = [], 0
            cur.append(k)
            used += need
        if cur:
            chunks.append(cur)
        nchunks += len(chunks)
        for c in chunks:
            launches += int(any(nsrow[k] > nscol[k] for k in c))                                 # fill
            for t in range(max(int(nscol[k] + SI_NB - 1) // SI_NB for k in c)):
                rows_after = False
                for k in c:
                    blk = int(nscol[k] + SI_NB - 1) // SI_NB - 1 - t
                    if blk >= 0 and nsrow[k] - blk * SI_NB - min(SI_NB, nscol[k] - blk * SI_NB) > 0:
                        rows_after = True
                launches += 1 + int(rows_after)                                                 # block, diagonal
            launches += 1                                                                       # store
        need = np.array([si_thin_lds(int(nscol[k]), int(nsrow[k])) for k in ids if thin[k]], dtype=np.int64)
        launches += len(set(np.searchsorted(THIN_LDS, need, side="left")))
    return nchunks, launches


def sweep_chunks(sup, pi, batch_of, budget_mb):
    """the chunks alone: every chunk is at least a diagonal and a store launch, so more chunks are strictly more launches"""
    return sweep_program(sup, pi, batch_of, budget_mb)[0]


# ---- matrices ---------------------------------------------------------------------------------------------------------

def block_arrow(rng, leaves, root=ARROW_ROOT):
    """dense leaves of w columns, each coupled to the last r rows of one dense root, natural ordering: with nrelax / zrelax
    zeroed the supernodes are exactly the leaves (w columns, r below-rows), in the order of the postorder, and the root last
    (tests/test_device_fuzz_corpus.py).  A strictly diagonally dominant matrix scaled symmetrically to a unit diagonal."""
    n = sum(w for w, _ in leaves) + root
    mask = np.zeros((n, n), dtype=bool)
    c = 0
    for w, r in leaves:
        mask[c:c + w, c:c + w] = True
        if r:
            mask[n - r:, c:c + w] = True
        c += w
    mask[c:, c:] = True
    mask = np.tril(mask)
    A = np.where(mask, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    A = np.tril(A, -1)
    A = A + A.T
    d = 2.0 * np.abs(A).sum(axis=1) + 1.0
    A = A / np.sqrt(np.outer(d, d)) + np.eye(n)
    ii, jj = np.nonzero(mask)
    order = np.lexsort((ii, jj))
    Ai, cols = ii[order].astype(np.int64), jj[order]
    Ap = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=Ap[1:])
    return n, Ap, Ai, A[Ai, cols]


def _arrow_leaves(rng):
    """leaf (width, below-rows) pairs drawn from ARROW_WIDTHS x ARROW_BELOW until the next would pass NMAX"""
    leaves, used = [], ARROW_ROOT
    for _ in range(int(rng.integers(6, 15))):
        w, r = int(rng.choice(ARROW_WIDTHS)), int(rng.choice(ARROW_BELOW))
        if used + w > NMAX:
            continue
        leaves.append((w, r))
        used += w
    return leaves


def rect_aat(rng):
    """the unsymmetric A (scipy CSC, m rows) of M = A A' + beta I: column j < m holds row j with |value| in [1, 2) and up to
    three more entries of magnitude < 0.3 (a strictly column-dominant square part: A has full row rank, no row is empty and
    M is positive definite for beta = 0 too); the columns after it hold 1 to 4 entries each"""
    m = int(rng.integers(20, 301))
    ncol = m + int(rng.integers(0, m + 1))
    rows, cols, vals = [], [], []
    for j in range(ncol):
        c = int(rng.integers(1, 5))
        if j < m:
            r = np.unique(np.concatenate([[j], rng.integers(0, m, size=c - 1)]))
            v = np.where(r == j, rng.uniform(1.0, 2.0) * rng.choice([-1.0, 1.0]), rng.uniform(-0.3, 0.3, len(r)) / 3.0)
        else:
            r = np.unique(rng.integers(0, m, size=c))
            v = rng.uniform(-1.0, 1.0, len(r))
        rows += r.tolist()
        cols += [j] * len(r)
        vals += np.asarray(v, dtype=np.float64).tolist()
    M = sp.csc_matrix((np.array(vals), (rows, cols)), shape=(m, ncol))
    M.sort_indices()
    assert M.nnz == len(rows)
    return M


def _real_matrix(rng, kind):
    if kind == "poisson3d":
        return G.poisson3d(int(rng.integers(3, 9)), int(rng.integers(3, 9)), int(rng.integers(3, 9)))
    if kind == "poisson2d":
        return G.poisson2d(int(rng.integers(5, 30)), int(rng.integers(5, 25)))
    if kind == "banded":
        n = int(rng.integers(150, NMAX + 1))
        return (n,) + rand_spd(rng, n, 30.0 / n, True)
    if kind == "general":
        n = int(rng.integers(2, NMAX + 1))
        return (n,) + rand_spd(rng, n, rng.uniform(1.0, 8.0) / n, bool(rng.integers(2)))
    raise KeyError(kind)


def corpus(seed, ncase):
    """yields dict (case, kind, n, Ap, Ai, Ax: the matrix, lower CSC (kind "aat": M, the scipy CSC rectangular A, n its rows);
    order: "natural" | "nesdis" | "perm" with perm the explicit permutation; postorder, norelax, hip_flags, beta, beta2 (the
    shift of the refactorization from device values), nrhs: the right-hand-side counts, budget: CHOLMOD_HIP_SELINV_BUDGET_MB
    as a string or None, twin: CHOLMOD_HIP_CX_TWIN=1 (complex), leaves: the (w, r) of a block arrow, rhs_seed)"""
    rng = np.random.default_rng(seed)
    narrow = ncx = 0
    for it in range(ncase):
        kind = KINDS[it % len(KINDS)]
        case = dict(case=it, kind=kind, perm=None, order="natural", postorder=True, norelax=False, budget=None, twin=False,
                    leaves=None, M=None)
        if kind == "arrow":
            case["leaves"] = _arrow_leaves(rng)
            n, Ap, Ai, Ax = block_arrow(rng, case["leaves"])
            case["norelax"] = True
        elif kind == "aat":
            case["M"] = rect_aat(rng)
            n, Ap, Ai, Ax = case["M"].shape[0], None, None, None
        else:
            base = REAL_KINDS[int(rng.integers(4))] if kind == "complex" else kind
            n, Ap, Ai, Ax = _real_matrix(rng, base)
        if kind not in ("arrow", "aat"):
            case["order"] = ("natural", "nesdis", "perm")[int(rng.integers(3))]
            if case["order"] == "perm":
                case["perm"] = rng.permutation(n).astype(np.int64)
            case["postorder"] = bool(rng.integers(4))           # off one time in four
            case["norelax"] = int(rng.integers(3)) == 0          # nrelax / zrelax zeroed one time in three
        if kind == "complex":                                   # the random phases of tests/fuzz_runner.py
            Ax = Ax.astype(np.complex128)
            off = Ai != np.repeat(np.arange(n), np.diff(Ap))
            Ax[off] *= np.exp(1j * rng.uniform(0, 2 * np.pi, int(off.sum())))
            case["twin"] = bool(ncx % 2)
            ncx += 1
        case.update(n=n, Ap=Ap, Ai=Ai, Ax=Ax, hip_flags=int(rng.choice(HIP_FLAGS)))
        case["beta"] = (0.0, BETA)[it // len(KINDS) % 2] if kind != "arrow" else (0.0, BETA)[int(rng.integers(2))]
        case["beta2"] = float(rng.uniform(0.0, 0.5))
        case["nrhs"] = sorted(int(x) for x in rng.choice(NRHS, size=3, replace=False))
        if kind in REAL_KINDS:
            # one real case in three: every second block arrow (its leaves share a batch, so the budget cuts it) and one in
            # three of the others
            mb = f"{rng.uniform(0.05, 0.5):.3f}"
            if (narrow % 2 == 0) if kind == "arrow" else (int(rng.integers(3)) == 0):
                case["budget"] = mb
            narrow += kind == "arrow"
        case["rhs_seed"] = int(rng.integers(1 << 30))
        yield case


# ---- a case through the library ---------------------------------------------------------------------------------------

def rect_sparse(S, M):
    """the library's cholmod_sparse (stype 0) of the scipy CSC matrix M"""
    from suitesparse_amd import cholmod as ch
    m, ncol = M.shape
    A = S.L.cholmod_l_allocate_sparse(m, ncol, max(M.nnz, 1), 1, 1, 0, ch.REAL, C.byref(S.cm))
    assert A
    a = A.contents
    ch._view(a.p, ncol + 1, C.c_int64, np.int64)[:] = M.indptr
    ch._view(a.i, M.nnz, C.c_int64, np.int64)[:] = M.indices
    ch._view(a.x, M.nnz, C.c_double, np.float64)[:] = M.data
    return A


def factorized(case, use_gpu):
    """-> (Session, A, Lf, ok): the case analyzed and factorized with its own ordering, flags and beta; ok: the factorization
    returned 1 with status CHOLMOD_OK and minor == n.  The environment (scratch budget, complex storage) is the caller's."""
    from suitesparse_amd import cholmod as ch
    aat = case["kind"] == "aat"
    S = ch.Session(use_gpu=use_gpu, postorder=case["postorder"], hip_flags=case["hip_flags"],
                   ordering="default" if aat else "nesdis" if case["order"] == "nesdis" else "natural")
    S.cm.error_handler = ch.ERRFUNC(0)
    if case["norelax"]:
        for k in range(3):
            S.cm.nrelax[k] = 0
            S.cm.zrelax[k] = 0.0
    A = rect_sparse(S, case["M"]) if aat else S.sparse(case["n"], case["Ap"], case["Ai"], case["Ax"], -1)
    Lf = S.analyze(A, case["perm"])
    ok = S.factorize(A, Lf, case["beta"]) == 1 and S.cm.status == ch.OK and int(Lf.contents.minor) == case["n"]
    return S, A, Lf, ok


def plan_batches(S, Lf, hip_flags=0):
    """the batch of every supernode: from the factor's own plan, or (a CPU-path factor has none) from a schedule-only plan
    of the same supernodes and flags"""
    from suitesparse_amd import cholmod as ch
    f = Lf.contents
    batch = np.zeros(int(f.nsuper), dtype=np.int64)
    if f.hip_plan:
        S.L.cholmod_hip_get_batches(f.hip_plan, batch.ctypes.data, None)
        return batch
    st = C.c_int(0)
    P = S.L.cholmod_hip_plan_create(int(f.n), int(f.nsuper), f.super, f.pi, f.px, f.s, ch.HIP_PLAN_HOST_ONLY | hip_flags, C.byref(st))
    assert P and st.value == 0
    S.L.cholmod_hip_get_batches(P, batch.ctypes.data, None)
    S.L.cholmod_hip_plan_destroy(P)
    return batch


def describe(case):
    return (f"case {case['case']} kind {case['kind']} n {case['n']} order {case['order']} postorder {int(case['postorder'])} "
            f"norelax {int(case['norelax'])} flags {case['hip_flags']} beta {case['beta']} nrhs {case['nrhs']} budget {case['budget']}")
