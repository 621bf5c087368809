"""The seeded random corpus of the device fuzz (tests/test_device_fuzz_corpus.py without a GPU, tests/device_fuzz_runner.py
with one) and the maps from a factor to the classes it reaches: the dispatch classes of its fronts in the two backward sweeps
and in the device solves (front_classes), the paths of the Schur complement's tile kernel for a given m (schur_classes) and
the twin-space front shapes of a complex factor (cx_front_classes).  No torch, no GPU.

corpus (seed, ncase) yields fully determined cases.  Cases 0 .. NBASE - 1: everything random comes from the one
np.random.default_rng (seed), in a fixed order, so a case number reproduces the case.  Kinds rotate with the case number, as
tests/fuzz_runner.py rotates its own (KINDS): Poisson 3D and 2D, banded and general rand_spd (diagonally dominant, always
positive definite), a block arrow with engineered front shapes, an unsymmetric A for M = A A' + beta I, and a complex
Hermitian matrix on one of the real patterns.  Cases NBASE .. NCASE - 1 are complex Hermitian block arrows whose leaves sit on
the edges of the complex kernels in twin space; they draw from np.random.default_rng ([seed, 1]).  The m of the Schur
complements (schur_ms) and every other random input of the Schur steps come from np.random.default_rng ([rhs_seed, 7]).
Nothing added later draws from the first generator: case_digest and tests/golden/device_fuzz_corpus_digests.json pin cases
0 .. NBASE - 1.  n <= 700 everywhere: the dense float64 references are what make the checks strong."""
import ctypes as C
import hashlib
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
NBASE = 40              # cases 0 .. 39 rotate through KINDS, from the one generator of the seed
NCX_ARROW = 6           # cases 40 .. 45: complex block arrows, from a generator of their own
NCASE = NBASE + NCX_ARROW
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

# the Schur complement (schur_classes): the values of m around the 64 x 64 tiles of k_schur_tile, and the classes of its walk
SCHUR_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193]
SCHUR_CLASSES = ("nt1", "nt2", "nt3+", "edge_exact", "edge_ragged", "m_n", "boundary_first_col", "boundary_inside",
                 "boundary_unaligned", "supers1", "supers2+", "panel_wide", "col_rows>256", "skip_no_cols", "skip_no_rows",
                 "walk_break", "cend_cut", "k_tail", "row_absent", "offdiag_contrib")

# the complex block arrows (cx_front_classes): w complex columns and r rows below are a 2 w x 2 (w + r) front of the twin
CX_WIDTHS = [1, 7, 8, 9, 31, 32, 33, 64, 65, 128, 129]
CX_BELOW = [0, 1, 31, 32, 33, 35, 36, 37, 67, 68, 69]
CX_ROOT = 72
CX_NMAX = 500
EDGE_PAIRS = [(32, 36), (33, 35), (31, 37), (1, 67)]        # w + r = 68: 2 (w + r) = SM_MAX
CX_CLASSES = ("cx_thin", "cx_thin_r136", "cx_generic", "cx_norows", "cx_panel_under", "cx_panel_exact", "cx_panel_over",
              "cx_chain_exact", "cx_solve_big")

# ---- the thresholds, restated -----------------------------------------------------------------------------------------
SI_NB = 64                  # sweep_device.hip.h:10  #define SI_NB 64 (column block of the recurrence)
SM_MAX = 136                # descriptors.hip.h:132  #define SM_MAX 136
THIN_LDS = (2048, 8192)     # selinv.hip:49          cls_doubles [3] = {2048, 8192, 1 << 30} (thin_launches)
PF_NB = 64                  # descriptors.hip.h:127  #define PF_NB 64 (the column panel of the pivot kernels)
SOLVE_SB = 256              # descriptors.hip.h:156  #define SOLVE_SB 256 (column block of the big-front walk)
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


def cx_front_classes(sup, pi):
    """the set of class names (CX_CLASSES) the fronts of a COMPLEX factor (its own super, pi) reach.  The engine's plan is
    that of the real twin in both storages (host/complex.c:95 .. 100: Tsuper = 2 Super, Tpi = 2 Lpi): a supernode of w
    columns and r rows below is the front nscol = 2 w, nsrow = 2 (w + r) there, and the thresholds fall on that shape."""
    sup, pi = np.asarray(sup), np.asarray(pi)
    out = set()
    for k in range(len(sup) - 1):
        nscol, nsrow = 2 * int(sup[k + 1] - sup[k]), 2 * int(pi[k + 1] - pi[k])
        if nsrow <= SM_MAX:                             # plan_build.hip:322  f.cbp = ... f.nsrow <= SM_MAX ... (324: 2 in complex storage)
            out.add("cx_thin")
            if nsrow == SM_MAX:
                out.add("cx_thin_r136")
        else:
            out.add("cx_generic")
        if nsrow == nscol:
            out.add("cx_norows")
        if nscol in (PF_NB - 2, PF_NB, PF_NB + 2):      # descriptors.hip.h:127  #define PF_NB 64: the panel of the pivot kernels
            out.add({PF_NB - 2: "cx_panel_under", PF_NB: "cx_panel_exact", PF_NB + 2: "cx_panel_over"}[nscol])
        if nscol == SOLVE_SB:                           # descriptors.hip.h:156  #define SOLVE_SB 256: one whole column block
            out.add("cx_chain_exact")
        if nscol > SOLVE_BIG_COLS or nsrow * nscol > SOLVE_BIG_ENTRIES:     # plan_build.hip:555
            out.add("cx_solve_big")
    return out


def dense_hermitian(n, Ap, Ai, Ax, beta=0.0):
    """the dense Hermitian A + beta I of a lower-stored complex CSC matrix"""
    Al = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n)).toarray()
    return Al + np.tril(Al, -1).conj().T + beta * np.eye(n)


def by_supernode(fv, x, Lref):
    """(worst, k, dead, imag): L by supernode, the measure of not_posdef_cases.by_entry -- over the lower trapezoid of a
    supernode, max |L - L_ref| / max |L_ref| of that supernode -- of the worst supernode k (a NaN counts as the worst); the
    number of non-zero entries in the dead upper triangles; the number of diagonal entries with a non-zero imaginary part.
    x: the factor's values in its own layout (real or complex), Lref: the dense factor of the permuted matrix."""
    sup, pi, px, s = (np.asarray(getattr(fv, k)) for k in ("super", "pi", "px", "s"))
    worst, at, dead, imag = 0.0, -1, 0, 0
    for k in range(len(sup) - 1):
        rows = s[pi[k]:pi[k + 1]]
        nscol, nsrow = int(sup[k + 1] - sup[k]), len(rows)
        P = np.asarray(x[px[k]:px[k] + nsrow * nscol]).reshape(nscol, nsrow).T
        live = np.ones((nsrow, nscol), dtype=bool)
        live[:nscol] = np.tril(live[:nscol])
        ref = Lref[np.ix_(rows, rows[:nscol])]
        e = float(np.abs(P - ref)[live].max() / np.abs(ref[live]).max())
        if not e <= worst:
            worst, at = (e if e == e else float("inf")), k
        dead += int(np.count_nonzero(P[~live]))
        imag += int(np.count_nonzero(np.imag(np.diagonal(P))))
    return worst, at, dead, imag


def schur_ms(fv, n, rng, with_n=False):
    """at most 4 values of m (and n itself: with_n) for the Schur complement of a real factor (fv.super, fv.nsuper), in this
    order, a value that came before dropped: one of SCHUR_EDGES within 1 .. n; one with n - m the first column of a
    supernode of the upper half; one with n - m strictly inside one of the last four supernodes of at least 3 columns, if
    there is one; one uniform in 1 .. n."""
    sup, nsuper = np.asarray(fv.super), int(fv.nsuper)
    ms = [int(rng.choice([m for m in SCHUR_EDGES if m <= n]))]
    ms.append(n - int(sup[int(rng.integers(nsuper // 2, nsuper))]))
    wide = np.flatnonzero(np.diff(sup[:nsuper + 1]) >= 3)[-4:]
    if len(wide):
        k = int(rng.choice(wide))
        ms.append(n - int(rng.integers(sup[k] + 1, sup[k + 1])))
    ms.append(int(rng.integers(1, n + 1)))
    if with_n:
        ms.append(n)
    return list(dict.fromkeys(ms))


def schur_rng(case):
    """the generator of everything random in the Schur steps of a case; schur_ms draws from it first"""
    return np.random.default_rng([case["rhs_seed"], 7])


def case_ms(case, fv, rng=None):
    """the m of a case: schur_ms on the case's own generator, m = n added for every eighth case"""
    return schur_ms(fv, case["n"], schur_rng(case) if rng is None else rng, with_n=case["case"] % 8 == 0)


def schur_classes(sup, pi, s, n, m):
    """the set of class names (SCHUR_CLASSES) the Schur complement onto the last m >= 1 variables reaches: the walk of
    k_schur_tile (schur_kernels.hip.h) over every tile of the lower triangle, and the column loops of the two products"""
    sup, pi, s = np.asarray(sup), np.asarray(pi), np.asarray(s)
    nsuper = len(sup) - 1
    t0 = n - m                                          # schur_kernels.hip.h:55  t0 = n - m
    nt = (m + 63) // 64                                 # schur.hip:46  nt = (m + 63) / 64
    out = {"nt1" if nt == 1 else "nt2" if nt == 2 else "nt3+", "edge_exact" if m % 64 == 0 else "edge_ragged"}
    if m == n:
        out.add("m_n")
    s0 = int(np.searchsorted(sup, t0, side="right")) - 1        # schur.hip:52  P->supermap [n - m]
    out.add("boundary_first_col" if t0 == sup[s0] else "boundary_inside")
    if (t0 - sup[s0]) % 4:
        out.add("boundary_unaligned")                   # the kc loop of line 85 starts at a c0 that is no multiple of 4
    out.add("supers1" if s0 == nsuper - 1 else "supers2+")
    rows_of, bounds = {}, {}
    for k in range(s0, nsuper):
        c0 = max(0, t0 - int(sup[k]))                   # :67  c0 = f.k1 < t0 ? t0 - f.k1 : 0
        if int(sup[k + 1] - sup[k]) - c0 > 64:
            out.add("panel_wide")
        if int(pi[k + 1] - pi[k]) - c0 > 256:           # :144, :177  for (r = cl + tid ; r < f.nsrow ; r += 256)
            out.add("col_rows>256")
        rows_of[k] = s[pi[k]:pi[k + 1]]
        bounds[k] = np.searchsorted(rows_of[k], t0 + 64 * np.arange(nt + 1), side="left")      # :33  sc_lower_bound
    for J in range(nt):                                 # :42  sc_tile_of: (I, J), I >= J
        rJ = t0 + 64 * J
        for I in range(J, nt):
            rI = t0 + 64 * I
            for k in range(s0, nsuper):                 # :61  for (s = s0 ; s < nsuper ; s++)
                if sup[k] >= rJ + 64:                   # :66  if (f.k1 >= rJ + 64) break
                    out.add("walk_break")
                    break
                nscol = int(sup[k + 1] - sup[k])
                c0 = max(0, t0 - int(sup[k]))
                jlo, jhi = int(bounds[k][J]), int(bounds[k][J + 1])     # :68
                if jlo == jhi:                          # :69  continue
                    out.add("skip_no_cols")
                    continue
                ilo, ihi = int(bounds[k][I]), int(bounds[k][I + 1])     # :70
                if ilo == ihi:                          # :71  continue
                    out.add("skip_no_rows")
                    continue
                cend = min(nscol, jhi)                  # :84  cend = min (f.nscol, jhi)
                if cend < nscol:
                    out.add("cend_cut")
                if (cend - c0) % 4:                     # :88  kin = k < cend
                    out.add("k_tail")
                if ihi - ilo < min(64, n - rI) or jhi - jlo < min(64, n - rJ):      # :72 .. 79  sc_local_row gives -1
                    out.add("row_absent")
                if I > J:
                    out.add("offdiag_contrib")
    return out


def sweep_program(sup, pi, batch_of, budget_mb):
    """(chunks, launches) of the launch program the two backward sweeps share, under a scratch budget in MB (None: the
    default of 2048), restated from selinv.hip: scratch_budget and scratch_of (lines 26 .. 36) and Builder::build (126 ..
    151) -- per batch the generic fronts, widest first, a new chunk wherever the budget falls, then the thin fronts --,
    Builder::chunk (82 .. 125) -- one fill launch if a front of the chunk has below-rows, per block step a block launch if
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


def _cx_arrow_leaves(rng):
    """the leaves of a complex block arrow: one of EDGE_PAIRS (w + r = 68: the twin front has SM_MAX rows), then 5 to 9
    draws from CX_WIDTHS x CX_BELOW, a draw that would pass CX_NMAX dropped"""
    leaves = [EDGE_PAIRS[int(rng.integers(len(EDGE_PAIRS)))]]
    used = CX_ROOT + leaves[0][0]
    for _ in range(int(rng.integers(5, 10))):
        w, r = int(rng.choice(CX_WIDTHS)), int(rng.choice(CX_BELOW))
        if used + w > CX_NMAX:
            continue
        leaves.append((w, r))
        used += w
    return leaves


def _cx_arrows(seed, first, count):
    """the complex block arrows appended to the corpus as cases first .. first + count - 1.  Everything random comes from
    np.random.default_rng ([seed, 1]): the generator of cases 0 .. NBASE - 1 is not touched.  block_arrow with a root of
    CX_ROOT columns, nrelax / zrelax zeroed, natural ordering, hip_flags 0 (16 would take the thin form away that
    cx_front_classes counts), unit phases on the off-diagonal entries: |a_ij| is what it was, so the matrix stays strictly
    diagonally dominant with a real positive diagonal, Hermitian positive definite."""
    rng = np.random.default_rng([seed, 1])
    for k in range(count):
        case = dict(case=first + k, kind="complex", perm=None, order="natural", postorder=True, norelax=True, budget=None,
                    twin=bool(k % 2), M=None, hip_flags=0)
        case["leaves"] = _cx_arrow_leaves(rng)
        n, Ap, Ai, Ax = block_arrow(rng, case["leaves"], root=CX_ROOT)
        Ax = Ax.astype(np.complex128)
        off = Ai != np.repeat(np.arange(n), np.diff(Ap))
        Ax[off] *= np.exp(1j * rng.uniform(0, 2 * np.pi, int(off.sum())))
        case.update(n=n, Ap=Ap, Ai=Ai, Ax=Ax, beta=(0.0, BETA)[int(rng.integers(2))], beta2=float(rng.uniform(0.0, 0.5)))
        case["nrhs"] = sorted(int(x) for x in rng.choice(NRHS, size=3, replace=False))
        case["rhs_seed"] = int(rng.integers(1 << 30))
        yield case


def corpus(seed, ncase):
    """yields dict (case, kind, n, Ap, Ai, Ax: the matrix, lower CSC (kind "aat": M, the scipy CSC rectangular A, n its rows);
    order: "natural" | "nesdis" | "perm" with perm the explicit permutation; postorder, norelax, hip_flags, beta, beta2 (the
    shift of the refactorization from device values), nrhs: the right-hand-side counts, budget: CHOLMOD_HIP_SELINV_BUDGET_MB
    as a string or None, twin: CHOLMOD_HIP_CX_TWIN=1 (complex), leaves: the (w, r) of a block arrow, rhs_seed).  Cases
    0 .. NBASE - 1 rotate through KINDS; cases NBASE .. NCASE - 1 are the complex block arrows (_cx_arrows), kind "complex"
    with leaves."""
    yield from _rotating(seed, min(ncase, NBASE))
    yield from _cx_arrows(seed, NBASE, min(max(ncase - NBASE, 0), NCX_ARROW))


def _rotating(seed, ncase):
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


def case_digest(case):
    """sha256 over everything that determines a case: n, the matrix (Ap, Ai, Ax; kind "aat": M.indptr, M.indices, M.data;
    indices as int64, values as float64 or complex128), perm, order, postorder, norelax, hip_flags, beta, beta2, nrhs, budget,
    twin, leaves, rhs_seed.  tests/golden/device_fuzz_corpus_digests.json holds those of cases 0 .. 39 of both seeds as they
    were before cases were appended (tests/test_device_fuzz_corpus.py)."""
    h = hashlib.sha256()
    M = case["M"]
    arrays = (M.indptr, M.indices, M.data) if case["kind"] == "aat" else (case["Ap"], case["Ai"], case["Ax"])
    h.update(repr(int(case["n"])).encode())
    for a, cx in zip(arrays, (False, False, True)):
        a = np.asarray(a)
        a = a.astype(np.complex128 if np.iscomplexobj(a) else np.float64) if cx else a.astype(np.int64)
        h.update(str(a.dtype).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(b"None" if case["perm"] is None else np.ascontiguousarray(case["perm"], dtype=np.int64).tobytes())
    leaves = None if case["leaves"] is None else [(int(w), int(r)) for w, r in case["leaves"]]
    h.update(repr((str(case["order"]), bool(case["postorder"]), bool(case["norelax"]), int(case["hip_flags"]), float(case["beta"]),
                   float(case["beta2"]), [int(x) for x in case["nrhs"]], case["budget"], bool(case["twin"]), leaves,
                   int(case["rhs_seed"]))).encode())
    return h.hexdigest()


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
