/* cholmod_hip.h -- thin C-ABI shim of the MI355X (gfx950) supernodal Cholesky
 * engine.  Plain pointers and sizes only; no CHOLMOD structs, no torch types.
 *
 * This is the boundary a CHOLMOD maintainer binds: each entry point names the
 * reference interface it replaces (paths relative to the reference root).
 * The host layer in include/cholmod.h (cholmod_l_* mirror) is built on exactly
 * these calls; INTEGRATION.md shows the same calls made from the reference's
 * own cholmod_super_numeric.c.
 *
 * Index type is int64 (the reference's GPU path exists only in the
 * cholmod_l_* / DLONG build: CHOLMOD/Include/cholmod_internal.h:250-251).
 * All functions return 0 on success unless stated otherwise.
 */
#ifndef CHOLMOD_HIP_H
#define CHOLMOD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes (engine level; the host layer maps them to Common->status) */
#define CHOLMOD_HIP_OK            0
#define CHOLMOD_HIP_NOT_POSDEF    1     /* success, but minor < n            */
#define CHOLMOD_HIP_NO_DEVICE   (-1)    /* no usable gfx950 device / runtime */
#define CHOLMOD_HIP_OUT_OF_MEMORY (-2)
#define CHOLMOD_HIP_TOO_LARGE   (-3)    /* n or nsuper beyond the engine's 32-bit maps */
#define CHOLMOD_HIP_INVALID     (-4)
#define CHOLMOD_HIP_GPU_PROBLEM (-5)    /* a HIP call or kernel failed       */

/* plan flags */
#define CHOLMOD_HIP_PLAN_DEFAULT   0
#define CHOLMOD_HIP_TILE128         4    /* tuning: 128x128 update tiles on big regions
                                           (default: 64x64 everywhere, which fills the
                                           256 CUs on mid-size fronts)               */
#define CHOLMOD_HIP_NO_SMALL_FRONTS 16   /* tuning: no fused LDS-resident kernel for
                                           thin fronts (generic kernels everywhere)  */
#define CHOLMOD_HIP_NO_XCD_SWIZZLE 32    /* tuning: plain block -> tile order          */
#define CHOLMOD_HIP_FIXED_OB       64    /* tuning: 512-column outer blocks everywhere  */
#define CHOLMOD_HIP_WIDE_OB       128    /* tests: 2048-column outer blocks everywhere  */
#define CHOLMOD_HIP_NO_CB_ASSIGN   2048   /* tuning: zero-fill every contribution block and
                                           extend-add before the dense phase           */
#define CHOLMOD_HIP_NO_FUSED_POTRF 512   /* tuning: every diagonal block through a k_potrf_mfma
                                         * launch of its own (no k_update2f)                 */
#define CHOLMOD_HIP_NO_FUSED_TRSM 1024   /* tuning: the K = 64 steps of the panel chain as separate
                                         * solve and update launches (no k_trsm_upd)               */
#define CHOLMOD_HIP_NO_LEAF_PAIRS 4096    /* tuning: leaf fronts one per wave like every other thin
                                         * front (no k_leaf_pair)                                */
#define CHOLMOD_HIP_NO_EXCHANGE_LOOKAHEAD 256 /* multi-GPU: all-reduce a block column only
                                         * when it is due (no overlap with updates)  */
#define CHOLMOD_HIP_CHAIN256     8192    /* tuning / tests: the panel chain in 256-column sub-blocks -- one launch per sub-block
                                         * (k_chainf: the diagonal sub-block spread over four workgroups that hand their row
                                         * block of L to the row workgroups through flags; CHOLMOD_HIP_NO_CHAINF=1: the two
                                         * kernels of round 3, k_diag + k_rowsolve) -- instead of the 64-column chain
                                         * (k_potrf_mfma, k_trsm_mfma, k_trsm_upd, k_update2f).  On one GPU within +-2 % of the
                                         * 64-column chain; the default for the batches of a multi-GPU
                                         * plan that hold a front shared between ranks */
#define CHOLMOD_HIP_PHI_TWIN    16384    /* the structure is the real twin of a complex factor (every supernode, row and
                                         * column doubled, host/complex.c; checked at plan creation): the update kernels
                                         * contract over the even panel columns only and rebuild the 2 x 2 blocks of the
                                         * embedding in the lanes -- a complex multiply-add as 4 real ones, not 8
                                         * (reference zherk / zgemm, t_cholmod_super_numeric.c:41-83, :682-717).  Set by
                                         * cholmod_l_super_numeric for complex / zomplex A; CHOLMOD_HIP_TWIN_FULL_K=1
                                         * in the environment keeps the plain embedding (A/B timing, tests) */
#define CHOLMOD_HIP_CX_STORAGE   32768    /* a complex factor in its own storage: super / pi / s are those of the twin (as
                                         * CHOLMOD_HIP_PHI_TWIN, implied), px [s] = 2 x the complex factor's px [s]: of
                                         * every front only the even twin columns exist -- nsrow_twin x nscol_twin / 2
                                         * doubles, i.e. the interleaved complex panel of the reference's L->x
                                         * (t_cholmod_super_numeric.c:41-83, L_ENTRY 2): 2 xsize doubles of HBM instead of
                                         * the twin's 4 xsize, contribution blocks likewise.  Kernels rebuild the odd
                                         * columns (rotations of the even ones) on the way into LDS / registers.  One
                                         * rank, generic kernels only (no thin-front kernels).  cholmod_hip_download_factor
                                         * then returns the complex factor itself */
#define CHOLMOD_HIP_FUSED_CB_EA   65536    /* one GPU, real fronts: the update that first writes the whole contribution block of a
                                         * front also adds the children's entries that land there (k_update3f, through inverse
                                         * relative maps built once per plan), and the second extend-add phase leaves those
                                         * columns out: 16 B less traffic per child entry.  The factor changes by rounding at
                                         * most.  Set by cholmod_l_super_numeric unless CHOLMOD_HIP_NO_FUSED_CB_EA=1 is in the
                                         * environment; without it a plan is what it was before the flag existed */
#define CHOLMOD_HIP_PLAN_HOST_ONLY 2    /* build the schedule only, touch no device
                                           (CPU-side tests of the host logic)       */

typedef struct cholmod_hip_plan cholmod_hip_plan ;  /* opaque, one per symbolic L */

/* replaces cholmod_l_gpu_probe (CHOLMOD/GPU/cholmod_gpu.c:170-205):
 * returns 1 if a device is usable, 0 otherwise. */
int cholmod_hip_probe (void) ;

/* replaces cholmod_l_gpu_memorysize (CHOLMOD/GPU/cholmod_gpu.c:71-160):
 * returns 0 and fills total/available bytes, or 1 if there is no device. */
int cholmod_hip_memorysize (size_t *total_mem, size_t *available_mem) ;

/* Select the device for this process (one process per GPU). */
int cholmod_hip_set_device (int device) ;
/* Devices this process can see (a launcher checks it before it starts one rank per GPU);
 * no counterpart in the reference, which drives device 0 only (CHOLMOD/GPU/cholmod_gpu.c:160-164). */
int cholmod_hip_device_count (int *count) ;

/* Build the device plan of a supernodal symbolic factor: uploads the index
 * maps (super/pi/px/s exactly as in cholmod_factor, CHOLMOD/Include/
 * cholmod_core.h:1673-1798), derives the supernodal etree, its level sets, the
 * child->parent relative row maps (the reference's RelativeMap,
 * CHOLMOD/Supernodal/t_cholmod_super_numeric.c:743-750, computed on the device)
 * and the batched launch schedule.  Replaces r_cholmod_l_gpu_init
 * (CHOLMOD/GPU/t_cholmod_gpu.c:79-205) and cholmod_l_gpu_allocate
 * (CHOLMOD/GPU/cholmod_gpu.c:364-486): all device memory for L (xsize doubles)
 * and for the contribution-block arena is reserved here.
 * On failure returns NULL and stores a CHOLMOD_HIP_* code in *status. */
cholmod_hip_plan *cholmod_hip_plan_create (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px,
    const int64_t *s, int flags, int *status) ;

void cholmod_hip_plan_destroy (cholmod_hip_plan *plan) ;

/* The same plan (one GPU) with what the analysis knows of the explicit zeros of the relaxed fronts: for every supernode s
 * with reach_p [s+1] > reach_p [s] (= its row count), reach_first [reach_p [s] + p] is the first column of s, counted from
 * its first column, whose pattern in L holds the row at position p of its row list (INT32_MAX: none).  The plan gives
 * the big ones a head -- a first outer block of H columns whose closing update runs over the rows those columns reach
 * only -- where that pays (stats [40]).  reach_p == NULL: exactly the plan of cholmod_hip_plan_create. */
cholmod_hip_plan *cholmod_hip_plan_create_reach (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px,
    const int64_t *s, int flags, const int64_t *reach_p, const int32_t *reach_first, int *status) ;

/* ---- multi-GPU (one process per GPU; no counterpart in the reference, which is
 * single-GPU: CHOLMOD/GPU/cholmod_gpu.c:160-164) -------------------------------
 * Every rank builds the same plan from the same symbolic factor and passes its
 * rank / world size.  The supernodal etree is mapped proportionally: the root's
 * front is *shared* by all ranks, the heavy children of a shared front split
 * its rank group [first, first+size) between them where their weights allow,
 * and the light subtrees below are dealt to the ranks of the group they hang
 * off (largest first).  A shared front lives on every rank of its group as a
 * partial sum; the group factors its panels redundantly and deals the tiles of
 * its trailing updates round-robin.  The only exchange is an in-place sum
 * all-reduce, over the front's group, of a 512-column block column right
 * before it is factored; the engine asks the host for it through this callback
 * (bench.py / the tests implement it with torch.distributed: RCCL over xGMI,
 * or gloo in CPU tests).  group_first/group_size name the contiguous rank range
 * that takes part (every rank of the range makes the same call, in the same
 * order; ranks outside do not call).  The callback is entered with the data
 * ready and must return only when the result is visible to later device work.
 * Returns 0 on success. */
typedef int (*cholmod_hip_allreduce_fn) (void *dev_ptr, int64_t count_doubles,
    int group_first, int group_size, void *user) ;
cholmod_hip_plan *cholmod_hip_plan_create_dist (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px,
    const int64_t *s, int flags, int rank, int world, int *status) ;
int cholmod_hip_set_allreduce (cholmod_hip_plan *plan,
    cholmod_hip_allreduce_fn fn, void *user) ;
/* Native exchange: instead of the host callback the engine calls RCCL itself
 * (librccl bound with dlopen), stream-ordered on its own streams -- no host
 * synchronisation per block column, usable from a plain C caller.  One rank
 * obtains a 128-byte id with cholmod_hip_rccl_unique_id and hands it to the
 * others by any means (MPI_Bcast, a file, torch.distributed); every rank then
 * calls cholmod_hip_rccl_attach on its plan: ncclCommInitRank over the world and
 * one ncclCommSplit per rank group the plan shares fronts over (collective:
 * all ranks must call it).  The callback, if set, is then no longer used. */
int cholmod_hip_rccl_unique_id (void *id128) ;
int cholmod_hip_rccl_attach (cholmod_hip_plan *plan, const void *id128) ;
/* back to the callback (destroys the plan's communicators) */
int cholmod_hip_rccl_detach (cholmod_hip_plan *plan) ;
/* test hook (several ranks): the (contributor d, shared ancestor a) pairs whose contributions this rank routes straight into a's
 * windows, and per front the block [cb_lo, cb_hi) of contribution-block columns the rank stores (-1: not distributed).
 * Returns the number of pairs, fills at most cap. */
int64_t cholmod_hip_debug_routing (cholmod_hip_plan *plan, int64_t cap, int64_t *pair_d, int64_t *pair_a,
    int64_t *cb_lo, int64_t *cb_hi) ;
/* test hook: fingerprint (16 words) of the rank's plan -- fronts, routing, layout, every group array, the launch list */
int cholmod_hip_debug_schedule_hash (cholmod_hip_plan *plan, uint64_t *out16) ;
/* test hooks (plans with CHOLMOD_HIP_FUSED_CB_EA).  cholmod_hip_debug_cb_extend_add: per front 4 numbers -- [0] 1 if it is a
 * generic front with children and a contribution block, [1] regions that take the contribution-block half of its
 * extend-add with them, [2] extend-add groups that cover its contribution-block columns, [3] its children; returns nsuper,
 * fills at most cap fronts.  cholmod_hip_debug_fused_pair: (parent, child) pair `pair` of those regions -- desc [8] = parent,
 * child, columns of the parent, rows of its contribution block, rows of the child's, 1 if the child's block is a packed
 * triangle, child rows that land in the parent's block, launch that holds the region; inv (rows of the parent's block) and
 * rel (rows of the child's) receive, if not NULL and the plan is on a device, the pair's inverse and relative map as the
 * device holds them.  Returns the number of pairs. */
int64_t cholmod_hip_debug_cb_extend_add (cholmod_hip_plan *plan, int64_t cap, int64_t *out) ;
int64_t cholmod_hip_debug_fused_pair (cholmod_hip_plan *plan, int64_t pair, int64_t *desc, int32_t *inv, int32_t *rel) ;
/* Progress of the factorization that is running (or ran last) on this plan, for a watchdog thread of the caller (bench.py
 * --gpus N: a hung collective must end in an error line, not in the driver's kill).  cholmod_hip_progress_enable (plan, 1)
 * allocates two words of pinned host memory the device marks, in stream order, around every block-column exchange.
 * cholmod_hip_progress: out [12] = [0] factorizations started, [1] launches of the schedule enqueued by the host in the current
 * one, [2] launches in the schedule, [3] exchanges enqueued, [4] exchanges in the schedule, [5] / [6] exchange the DEVICE has
 * entered / left (-1 without markers), and of the exchange entered and not left: [7] kind (7 = reduce-scatter + broadcast of
 * the diagonal block, 11 = all-gather), [8] first rank and [9] size of its rank group, [10] columns of the block column,
 * [11] rows below its diagonal block.  May be called from another thread while a factorization runs. */
int cholmod_hip_progress_enable (cholmod_hip_plan *plan, int enable) ;
int cholmod_hip_progress (cholmod_hip_plan *plan, int64_t *out12) ;
/* The batch order every rank of a partition must derive alike (the collectives of a group are issued in batch order):
 * batch_of[s] = index of the batch front s is factored in, counted over ALL fronts, *global_arena = length (doubles) of the
 * contribution-block arena laid out over all fronts, from which the memory-aware split was chosen; returns the number of
 * subtrees swept one after the other (1 = plain level order).  Either pointer may be NULL. */
int64_t cholmod_hip_get_batches (cholmod_hip_plan *plan, int64_t *batch_of, int64_t *global_arena) ;
/* owner[s] = rank that factors supernode s, -1 for the shared fronts */
int cholmod_hip_get_partition (cholmod_hip_plan *plan, int64_t *owner) ;
/* rank group of every supernode: ranks [first[s], first[s]+size[s]) hold it
 * (size 1 = private to owner[s]) */
int cholmod_hip_get_groups (cholmod_hip_plan *plan, int64_t *first, int64_t *size) ;
/* Several ranks: a rank allocates L only for the fronts it holds (its subtrees and the shared
 * fronts of its groups, packed; cholmod_hip_get_stats [36] bytes against [5] for the whole
 * factor).  This call builds the COMPLETE factor in the reference layout on every rank (a second,
 * full-size array: each front written by the first rank of its group, one sum over all ranks);
 * solves, downloads and checks of a multi-rank plan need it.  If the full array does not fit
 * next to the rank's part, the contribution-block arena makes room and is allocated again by the
 * next factorization.  The next factorization invalidates the gathered copy. */
int cholmod_hip_gather_factor (cholmod_hip_plan *plan) ;

/* Numeric factorization  L L' = S + beta*I  of the already permuted,
 * lower-stored matrix S = tril(P A P') (packed or unpacked CSC on the host:
 * Snz may be NULL), the whole of cholmod_l_super_numeric's loop
 * (CHOLMOD/Supernodal/t_cholmod_super_numeric.c:93-1079: assemble, descendant
 * updates, dpotrf, dtrsm, not-positive-definite protocol :883-968).
 * The factor stays resident in HBM; if Lx_host != NULL the packed Lx array
 * (xsize doubles, reference layout) is also copied back.
 * *minor receives L->minor (== n when positive definite).
 * Returns CHOLMOD_HIP_OK, CHOLMOD_HIP_NOT_POSDEF, or a negative error.
 *
 * Supported pivot range (this entry point, cholmod_hip_factorize_resident and
 * cholmod_hip_dense_partial_factor).  A pivot is the diagonal entry as the elimination
 * reaches it.
 *  - Any normal double, DBL_MIN .. DBL_MAX: L(j,j) is within 1 ulp of sqrt (pivot); the
 *    kernels rescale by 2^+-512 outside [1e-290, 1e290], nothing else depends on the
 *    magnitude.  The factorization commutes with a scaling D A D by powers of two
 *    (L becomes D L, to rounding) as long as the entries of D A D and of D L stay normal
 *    doubles and max |A| < 2^1020: the columns are eliminated unscaled (an LDL' step with
 *    1 / pivot), so the entries of A, not only of L, must leave that room.
 *  - pivot <= 0 -- +0.0, -0.0, any negative value down to -5e-324 -- is a failure at
 *    that column (LAPACK's ajj <= 0): *minor / info name it, the columns from it on are
 *    zero.  NaN pivots do not stop the factorization.
 *  - A positive subnormal pivot (5e-324 .. DBL_MIN) is not a failure either.  Its square
 *    root takes the same rescaled sequence (no accuracy is promised for it; the tests
 *    measure it), but 1 / pivot overflows: the entries below it in its column are not
 *    finite unless the column has none (a 1 x 1 front, a last column).  Not supported. */
int cholmod_hip_factorize (cholmod_hip_plan *plan, const int64_t *Sp,
    const int64_t *Si, const int64_t *Snz, const double *Sx, double beta,
    int quick_return_if_not_posdef, double *Lx_host, int64_t *minor) ;

/* The same in two steps, so that a caller (bench.py) can time the factorization
 * with the input already resident in HBM: upload S once, refactorize often. */
int cholmod_hip_upload_matrix (cholmod_hip_plan *plan, const int64_t *Sp,
    const int64_t *Si, const int64_t *Snz, const double *Sx) ;
int cholmod_hip_factorize_resident (cholmod_hip_plan *plan, double beta,
    int quick_return_if_not_posdef, int64_t *minor) ;

/* New values for the resident S when only the VALUES of the caller's matrix changed
 * (cholmod_l_factorize called again with the same pattern: the common case of a
 * nonlinear or time-stepping loop).  cholmod_hip_set_value_map hands over, once per
 * upload, where every entry of the resident packed S came from in the caller's value
 * array: src [q] in [0, nvalues); CHOLMOD_HIP_INVALID without a resident packed S of snz
 * entries.  A later call then sends the values only -- no host-side permutation, no
 * pattern upload, the assembly map stays valid -- as a pipeline the caller drives:
 * cholmod_hip_values_begin hands out a PINNED staging buffer owned by the plan and the
 * gather index: *buffer [k] must receive values [index [k]] for k < *count, or, with
 * *index == NULL (no batch order: several ranks, CHOLMOD_HIP_VALUES_IN_BATCH_ORDER=0, ...),
 * values [k] for k < *count = nvalues; it enqueues the clearing of L at once.  The caller
 * fills the buffer chunk by chunk (*chunk_len positions, a multiple of 32768) and calls
 * cholmod_hip_values_push_chunk (c) for c = 0, 1, ... in order as each chunk is complete --
 * an asynchronous DMA -- or (-1) to cancel; cholmod_hip_factorize_resident, called once
 * after begin from any thread, waits for the chunks it needs (values.hip has the protocol)
 * and returns an error after a cancel. */
int cholmod_hip_set_value_map (cholmod_hip_plan *plan, const int64_t *src, int64_t snz,
    int64_t nvalues) ;
int cholmod_hip_values_begin (cholmod_hip_plan *plan, double **buffer, const int64_t **index,
    int64_t *count, int64_t *chunk_len) ;
int cholmod_hip_values_push_chunk (cholmod_hip_plan *plan, int64_t chunk) ;

/* The same values-only factorization for values that already live in device memory (a matrix assembled on the GPU):
 * dvalues is a DEVICE pointer to the caller's value array, nvalues doubles in the order cholmod_hip_set_value_map was
 * given for, read only.  The engine stream waits for an event recorded on `stream` (the caller's hipStream_t, NULL: the
 * null stream), exactly as cholmod_hip_solve_device does; the values are gathered from dvalues straight into the resident
 * S -- no copy into the plan's value buffer, no pinned staging, nothing crosses PCIe -- and the factorization runs as
 * cholmod_hip_factorize_resident runs it on a resident S with a valid assembly map: every entry of L receives exactly one
 * value of S.  PRECONDITION: a resident packed S with its value map (cholmod_hip_upload_matrix, a factorization,
 * cholmod_hip_set_value_map): the first factorization of a pattern still comes from the host.
 * THE CALL RETURNS WHEN THE FACTORIZATION HAS FINISHED ON THE DEVICE: it reports *minor and CHOLMOD_HIP_NOT_POSDEF as
 * cholmod_hip_factorize_resident does.  `stream` then waits for the engine's completion event, so later work on it (a
 * cholmod_hip_solve_device, say) needs no host synchronisation, and dvalues may be overwritten once the call has
 * returned.  The resident S is current afterwards: cholmod_hip_residual_device / _refine_device use the new matrix.
 * CHOLMOD_HIP_INVALID, before any device call: a NULL plan or pointer, a host-only plan, a plan of several ranks, no value
 * map for the current resident S, nvalues other than the value map's nvalues (the product map's navalues when one is
 * set), a host upload under way (cholmod_hip_values_begin without its factorization), the plans of complex factors
 * (CHOLMOD_HIP_PHI_TWIN, CHOLMOD_HIP_CX_STORAGE).  Must not be called while `stream` is being captured into a graph. */
int cholmod_hip_factorize_values_device (cholmod_hip_plan *plan, const double *dvalues, int64_t nvalues,
    double beta, int quick_return_if_not_posdef, void *stream, int64_t *minor) ;

/* The nc = nvalues values of the value map are then not given but COMPUTED on the device: value c is
 *     sum over p = cp [c] .. cp [c+1]-1 of a [ia [p]] * a [ib [p]]
 * over the navalues values a of the array cholmod_hip_factorize_values_device is then passed (S = tril (A A') from the
 * values of A: the normal equations).  The sums are formed into the plan's own value buffer on the engine stream and
 * gathered into S from there; each is added up by one owner in an order that depends on its list alone, without
 * floating-point atomics: the same values give the same bits.  Every index is validated here, on the host
 * (0 <= ia, ib < navalues, cp [0] == 0 and monotone, nc equal to the value map's nvalues: anything else is
 * CHOLMOD_HIP_INVALID), so the kernel reads nothing outside a [0 .. navalues); more than INT32_MAX pairs or values is
 * CHOLMOD_HIP_TOO_LARGE.  The map costs 16 bytes of HBM per pair.  cholmod_hip_set_value_map and
 * cholmod_hip_upload_matrix drop it; so does cp == NULL.  The host value upload above is not affected by it. */
int cholmod_hip_set_product_map (cholmod_hip_plan *plan, const int64_t *cp, const int64_t *ia, const int64_t *ib,
    int64_t nc, int64_t navalues) ;

/* The values of the resident S (snz doubles, the order of the uploaded pattern) to the host; waits for the engine stream. */
int cholmod_hip_download_matrix_values (cholmod_hip_plan *plan, double *Sx_host) ;

/* Copy the device-resident packed Lx (xsize doubles) to the host. */
int cholmod_hip_download_factor (cholmod_hip_plan *plan, double *Lx_host) ;
/* Even columns only, packed (xsize / 2 doubles): for a plan built on the doubled
 * structure of a complex factor (the real embedding, csrc/host/complex.c) these are the
 * interleaved complex columns of L, i.e. the reference's complex L->x, gathered on the
 * device. */
int cholmod_hip_download_even_columns (cholmod_hip_plan *plan, double *out_host) ;
/* Replace the device-resident Lx by host values (e.g. a factor computed
 * elsewhere), so the device solves can be used with it. */
int cholmod_hip_upload_factor (cholmod_hip_plan *plan, const double *Lx_host) ;

/* (This entry point and the two after it: csrc/hip/solve.hip.)
 * Supernodal triangular solves on the device-resident factor, in place on the
 * host array X (n-by-nrhs, leading dimension ldx), in the permuted ordering:
 * replace cholmod_l_super_lsolve / cholmod_l_super_ltsolve
 * (CHOLMOD/Supernodal/t_cholmod_super_solve.c:14-220, :222-411).
 * which: 0 = L then L' (both), 1 = L only, 2 = L' only. */
int cholmod_hip_solve (cholmod_hip_plan *plan, int which, double *X,
    int64_t nrhs, int64_t ldx) ;

/* The fill-reducing permutation of the plan (n entries, a permutation of 0 .. n-1:
 * anything else is CHOLMOD_HIP_INVALID), copied to the device once per plan so that
 * the solve below can gather and scatter by it.  CHOLMOD_HIP_NO_DEVICE on a
 * CHOLMOD_HIP_PLAN_HOST_ONLY plan (after the validation). */
int cholmod_hip_set_perm (cholmod_hip_plan *plan, const int64_t *Perm) ;

/* The same solves with the right-hand sides in device memory, ordered on the caller's
 * stream: dB (n-by-nrhs, column-major, leading dimension ldb) is read only, dX
 * (leading dimension ldx) receives the solution; dB == dX with ldb == ldx is legal
 * (in place).  Rows n .. ld-1 of either array are neither read nor written.
 *   which     0 = L then L', 1 = L, 2 = L', 3 = neither (permutation only)
 *   perm_in   gather B through Perm on the way in  (y [k] = B [Perm [k]])
 *   perm_out  scatter through Perm on the way out  (X [Perm [k]] = y [k])
 *   stream    the caller's hipStream_t (NULL: the null stream).  The engine's stream
 *             waits for an event recorded on it, runs the solve, and `stream` waits
 *             for the engine's completion event: no host synchronisation, no copy
 *             between host and device, and no allocation once the workspaces exist
 *             (they do after the first call with fewer than 8 and the first with
 *             more right-hand sides).  Must not be called while `stream` is being
 *             captured into a graph.
 * Fewer than 8 right-hand sides run the kernels of the host-array solve above on the
 * permuted columns (a panel costs about 3.5 of their sweeps); 8 or more travel in panels
 * of 16 (W [n][16], right-hand side fastest), L is read once per panel and the products
 * run on v_mfma_f64_16x16x4.
 * Needs a numeric factor on the device (several ranks: after the gather, as above) and,
 * for perm_in / perm_out, the permutation.  CHOLMOD_HIP_INVALID for a host-only plan,
 * NULL pointers, ld < n, nrhs < 0 and a missing permutation; nrhs == 0 is a success that
 * touches nothing.
 * The plan of a complex factor is served too.  Its n, ld and permutation are the twin's: a
 * column is 2 n_complex doubles, the interleaved (re, im) entries, and the permutation is
 * the expanded one (2 Perm [k], 2 Perm [k] + 1).  The full twin (CHOLMOD_HIP_PHI_TWIN alone)
 * is an ordinary real factor and runs the real kernels; in complex storage
 * (CHOLMOD_HIP_CX_STORAGE) both kernel families read the interleaved complex panels, half
 * the twin's bytes, and rebuild the odd twin columns on the way in.  stats [24] is read from the solve's two events when the statistics
 * are asked for, which may wait for the solve. */
int cholmod_hip_solve_device (cholmod_hip_plan *plan, int which, int perm_in, int perm_out,
    const double *dB, int64_t ldb, double *dX, int64_t ldx, int64_t nrhs, void *stream) ;

/* (This entry point and the next: csrc/hip/residual.hip.)
 * R = B - (A + beta I) X for the symmetric A whose permuted lower triangle is the resident S (cholmod_hip_upload_matrix,
 * kept current by the value uploads) and the beta of the last factorization.  X, B, R: n-by-nrhs in device memory,
 * column-major, leading dimensions ldx / ldb / ldr.  perm = 1: in the caller's ordering (rows gathered / scattered through
 * Perm, cholmod_hip_set_perm first); perm = 0: in the factor's ordering (S itself).  dX, dB are read only; dR may be dB
 * (same ld), must not be dX.  dRnorm: NULL, or nrhs doubles on the device that receive max_i |R (i,k)|.
 * Every entry of R is summed by one owner in a fixed order and the norms go through an integer maximum: the same
 * inputs give the same bits, call after call.  Fewer than 8 right-hand sides run column by column, 8 or more in panels of
 * 16 (the layout of the solve above); any nrhs >= 0, nrhs == 0 or n == 0 is a success that touches nothing.
 * The first call after a cholmod_hip_upload_matrix builds a transposed index of S's pattern (one download, a host pass,
 * one upload: it waits for the engine stream) and the two further panels [n][16]; after that nothing is allocated, and the
 * call is ordered on `stream` exactly as cholmod_hip_solve_device is (not during capture).
 * CHOLMOD_HIP_INVALID, before any device call: NULL plan or pointers, a host-only plan, a plan of several ranks, ld < n,
 * nrhs < 0, dR == dX, perm without a stored permutation, no resident S (a factor brought in by cholmod_hip_upload_factor
 * only).
 * The plan of a complex factor (CHOLMOD_HIP_PHI_TWIN, CHOLMOD_HIP_CX_STORAGE) is served like a real one: its resident S is
 * the real symmetric phi (S) of the twin, X, B and R are the interleaved complex columns (2 n_complex doubles each, ld in
 * doubles), and dRnorm [k] = max_i max (|re R (i,k)|, |im R (i,k)|). */
int cholmod_hip_residual_device (cholmod_hip_plan *plan, int perm, const double *dX, int64_t ldx, const double *dB,
    int64_t ldb, double *dR, int64_t ldr, int64_t nrhs, double *dRnorm, void *stream) ;

/* `steps` rounds of  X += (LL')^-1 (B - (A + beta I) X)  in place on dX (perm as above), then the residual norms of
 * the final X into dRnorm (NULL allowed).  steps == 0: X untouched, norms only.  The iteration stays in the factor's
 * ordering: B and X pass through Perm once on the way in, X once on the way out.  Needs what the residual needs and,
 * for steps > 0, the numeric factor as cholmod_hip_solve_device does; steps < 0 is CHOLMOD_HIP_INVALID.  The plans of
 * complex factors as for the residual and the solve. */
int cholmod_hip_refine_device (cholmod_hip_plan *plan, int perm, const double *dB, int64_t ldb, double *dX, int64_t ldx,
    int64_t nrhs, int steps, double *dRnorm, void *stream) ;

/* (This entry point and the four after it: csrc/hip/selinv.hip.)
 * The selected inverse: Zx = the entries of Z = (L L')^-1 = (P (A + beta I) P')^-1 on the pattern of L, a second array of
 * xsize doubles in HBM in exactly the layout of Lx -- supernode s holds, column-major nsrow x nscol at px [s], the values
 * Z (s [pi [s] + i], super [s] + j) for i >= j; the dead strictly-upper triangle of every diagonal block is exact zero.
 * The reference computes the same subset column by column on a simplicial LDL' (MATLAB_Tools/sparseinv/sparseinv.c,
 * Takahashi's equations); here it is the multifrontal factorization run backwards: the plan's batches from the last to
 * the first, per front 64-column blocks from the last to the first, Z [R, b] = -Z [R, R] L [R, b] inv (L_bb) on
 * v_mfma_f64_16x16x4 (R = the front's rows behind the block), Z [b, b] from two triangular solves; a front's Z on its
 * below-rows is gathered from the finished panels of its ancestors.  Every entry has one owner and a fixed summation
 * order: two calls on the same factor give the same bits.
 * Ordered on `stream` exactly as cholmod_hip_solve_device is: the engine stream waits for an event recorded on it, `stream`
 * waits for the engine's completion event; the first call builds the launch program and allocates Zx and the scratch
 * (the squares of the fronts in flight, CHOLMOD_HIP_SELINV_BUDGET_MB of them at most at a time, 2048 by default, and the
 * partial sums of the diagonal blocks), after that nothing is allocated and the host does not wait.  Not during capture.
 * Zx stays resident until cholmod_hip_selinv_release or cholmod_hip_plan_destroy; any factorization,
 * cholmod_hip_upload_factor or cholmod_hip_upload_matrix marks it stale.
 * All five return CHOLMOD_HIP_INVALID, before any device call, for a NULL plan, a host-only plan, several ranks, no numeric
 * factor on the device, a last factorization that was not positive definite, and the plans of complex factors
 * (CHOLMOD_HIP_PHI_TWIN, CHOLMOD_HIP_CX_STORAGE); CHOLMOD_HIP_OUT_OF_MEMORY when Zx and the scratch do not fit: what the
 * call allocated is freed, the factor is untouched. */
int cholmod_hip_selinv_device (cholmod_hip_plan *plan, void *stream) ;
/* What a caller takes from a current Zx, on the device and ordered on `stream` as above; either pointer may be NULL.
 * dZvalues [k], k < nvalues in the order of the value map (the array cholmod_hip_factorize_values_device takes), receives Z
 * at the position of the caller's entry k; a value the resident S does not read -- the ignored triangle, all but the last
 * of equal neighbours, entries outside the pattern of L -- receives a quiet NaN (the convention of cholmod_l_solve2's
 * subsets).  dDiag [i] receives (A + beta I)^-1 (i, i): in the caller's ordering with perm = 1 (cholmod_hip_set_perm
 * first), in the factor's with perm = 0.  A pure gather, bit-identical to the entries of Zx; the position of an entry
 * comes from the supernode map and a search in the supernode's row list.  CHOLMOD_HIP_INVALID also: no current Zx;
 * dZvalues without a value map of the current resident packed S, with another nvalues than the map's, or with a product
 * map set (the caller's values are then not the entries of S); perm without a permutation. */
int cholmod_hip_selinv_gather_device (cholmod_hip_plan *plan, double *dZvalues, int64_t nvalues, double *dDiag, int perm,
    void *stream) ;
/* Zx (xsize doubles) to the host; waits for the engine stream.  CHOLMOD_HIP_INVALID without a current Zx. */
int cholmod_hip_selinv_download (cholmod_hip_plan *plan, double *Zx_host) ;
/* frees Zx and the scratch -- unless a Gx of the factor gradient shares it -- (the launch program stays); the next cholmod_hip_selinv_device allocates them again */
int cholmod_hip_selinv_release (cholmod_hip_plan *plan) ;
/* out8: [0] device seconds of the last cholmod_hip_selinv_device (two events, read here: may wait for it)  [1] its kernel
 * launches  [2] flops of the hot product, sum of 2 |R|^2 nb over the blocks  [3] all flops  [4] bytes of Zx  [5] bytes of
 * scratch  [6] 1 if Zx is current  [7] reserved, zero */
int cholmod_hip_selinv_info (cholmod_hip_plan *plan, double *out8) ;

/* (This entry point and the next: csrc/hip/schur.hip.)
 * The Schur complement onto the LAST m variables of the factor's ordering.  With L the resident factor of
 * P (A + beta I) P', I its first n - m positions and S its last m,  L = [L11 0 ; L21 L22]  and
 *     Sc = (A + beta I)_SS - (A + beta I)_SI inv ((A + beta I)_II) (A + beta I)_IS = L22 L22',
 * so that L22 is the Cholesky factor of Sc.  Row i of Sc and of L22 is position n - m + i of the factor's ordering.  Any m
 * may be chosen after the factorization, and several from one factor; the factorization and its schedule are untouched.
 * dS: Sc, m-by-m, column-major, lds >= m, BOTH triangles written, bitwise symmetric.  dF: the dense L22, m-by-m,
 * column-major, ldf >= m: lower triangle = L (n-m+i, n-m+j), strict upper = +0.0; entries of L outside its pattern = +0.0.
 * Either pointer may be NULL, not both.  Nothing outside the m-by-m arrays is written.  0 <= m <= n; m == 0 is a success
 * that touches nothing.
 * One workgroup owns one 64 x 64 tile of the lower triangle of Sc and walks the supernodes that hold trailing columns in
 * ascending order, on v_mfma_f64_16x16x4; the strictly upper triangle of every diagonal block counts as zero whatever Lx
 * holds there.  One owner and one summation order, no floating-point atomics: two calls give the same bits.  The work is
 * the sum over the trailing supernodes of (rows from the first trailing column down)^2 x (trailing columns) multiply-adds,
 * at most about m^3 / 3.
 * Ordered on `stream` exactly as the selected inverse is: the engine stream waits for an event recorded on it, `stream`
 * waits for the engine's completion event; nothing is allocated and the host does not wait.  No host-device copy.  Not during capture.
 * CHOLMOD_HIP_INVALID, before any device call, for a NULL plan, a host-only plan, several ranks, the plan of a complex factor,
 * no positive definite numeric factor on the device, m < 0 or m > n, a leading dimension < m, both outputs NULL. */
int cholmod_hip_schur_device (cholmod_hip_plan *plan, int64_t m, double *dS, int64_t lds, double *dF, int64_t ldf,
    void *stream) ;
/* dOut (m-by-nrhs, column-major, ldo >= m) = L22 dV (trans = 0) or L22' dV (trans = 1), dV m-by-nrhs, ldv >= m, read only;
 * dOut != dV.  With the L and L' sweeps of the device solve these give the condensed right-hand side (L22 times the last m
 * rows of inv (L) P b) and the back-expansion.  L22' dV: one owner per row of dOut and a fixed summation tree, the same
 * inputs give the same bits.  L22 dV: the columns add into the cleared dOut atomically, as the forward solve does into
 * its right-hand side: the result is reproducible to rounding only.  Ordered on `stream` as above.  CHOLMOD_HIP_INVALID as
 * above and for a NULL array, nrhs < 0, dOut == dV; m == 0 or nrhs == 0 is a success that touches nothing. */
int cholmod_hip_trailing_multiply_device (cholmod_hip_plan *plan, int64_t m, int trans, const double *dV, int64_t ldv,
    double *dOut, int64_t ldo, int64_t nrhs, void *stream) ;

/* (This entry point and the five after it: csrc/hip/factor_grad.hip.)
 * The gradient through the factor (reverse-mode Cholesky): given Lbar = df/dL on the pattern of L, Gx = df/dS on the
 * pattern of L, where S = L L' = P (A + beta I) P' is LOWER-STORED -- an off-diagonal entry stands for two entries of the
 * symmetric matrix, Gx at (i, j), i >= j, is the derivative with respect to that stored entry.  Gx is a further array of
 * xsize doubles in HBM in exactly the layout of Lx, the dead strictly-upper triangle of every diagonal block exact +0.0.
 * dLbar: xsize doubles on the device in the layout of Lx, read only; what stands in its dead triangles is ignored.
 * The sweep is that of the selected inverse -- its launch program, its scratch, both shared -- with another recurrence:
 * per block, with W = Gx [R, R] and M = W + W', Gx [R, b] = (Lbar [R, b] - M L [R, b]) inv (L_bb) on v_mfma_f64_16x16x4,
 * Gx [b, b] from tril (Lbar [b, b]) - tril (Gx [R, b]' L [R, b]) through a triangular product and two triangular solves.
 * The selected inverse is the special case Lbar = diag (2 / L_jj): then Gx = Z on the diagonal and 2 Z off it.  Every
 * entry has one owner and a fixed summation order: two calls on the same inputs give the same bits.
 * Ordered on `stream` exactly as cholmod_hip_selinv_device is; the first call allocates Gx (and the program and the
 * scratch, if the selected inverse has not), after that nothing is allocated and the host does not wait.  Not during
 * capture.  Gx stays resident until cholmod_hip_factor_grad_release or cholmod_hip_plan_destroy; any factorization,
 * cholmod_hip_upload_factor or cholmod_hip_upload_matrix marks it stale.  Zx and Gx are separate arrays with separate
 * staleness.
 * All six return CHOLMOD_HIP_INVALID, before any device call, for a NULL plan or pointer, a host-only plan, several ranks,
 * no numeric factor on the device, a last factorization that was not positive definite, and the plans of complex factors;
 * CHOLMOD_HIP_OUT_OF_MEMORY when Gx and the scratch do not fit: what the call allocated is freed, the factor is untouched. */
int cholmod_hip_factor_grad_device (cholmod_hip_plan *plan, const double *dLbar, void *stream) ;
/* The same sweep with Lbar (i, j) = alpha sum_{r < nrhs} P (i, r) Q (j, r) on the pattern of L, r in index order, formed by a
 * kernel straight into Gx: no xsize array of the caller exists.  dP, dQ: n-by-nrhs, column-major, on the device, in the
 * FACTOR's ordering, read only (dP == dQ is legal); nrhs == 0 gives a zero Lbar.  With x = inv (L') z, an incoming gx and
 * u = inv (L) gx:  P = x, Q = u, alpha = -1 is the gradient through the solve with L', and gz = u; with y = inv (L) b, an
 * incoming gy and v = inv (L') gy:  P = v, Q = y, alpha = -1 the one through the solve with L, and gb = v.
 * CHOLMOD_HIP_INVALID also for ldp < n, ldq < n, nrhs < 0. */
int cholmod_hip_factor_outer_grad_device (cholmod_hip_plan *plan, double alpha, const double *dP, int64_t ldp, const double *dQ,
    int64_t ldq, int64_t nrhs, void *stream) ;
/* What a caller takes from a current Gx, on the device and ordered on `stream` as above; either pointer may be NULL.
 * dG [k], k < nvalues in the order of the value map, receives Gx at the entry the resident S reads value k into -- the
 * gradient with respect to that value -- and exact +0.0 where the factorization does not read the value (the rule of
 * cholmod_hip_values_grad_device, not the NaN of cholmod_hip_selinv_gather_device).  dTrace [0] receives sum_j Gx (j, j), the
 * gradient with respect to beta, summed in a fixed tree without floating-point atomics.  CHOLMOD_HIP_INVALID also: no
 * current Gx; dG without a value map of the current resident packed S, with another nvalues than the map's, or with a
 * product map set. */
int cholmod_hip_factor_grad_gather_device (cholmod_hip_plan *plan, double *dG, int64_t nvalues, double *dTrace, void *stream) ;
/* Gx (xsize doubles) to the host; waits for the engine stream.  CHOLMOD_HIP_INVALID without a current Gx. */
int cholmod_hip_factor_grad_download (cholmod_hip_plan *plan, double *Gx_host) ;
/* frees Gx, and the scratch unless a Zx shares it (the launch program stays); the next sweep allocates them again */
int cholmod_hip_factor_grad_release (cholmod_hip_plan *plan) ;
/* out8: the figures of cholmod_hip_selinv_info for the last sweep of the two entry points above: [0] its device seconds
 * [1] its launches (the program's and the one that forms Lbar)  [2] flops of the hot product  [3] all flops of the
 * program  [4] bytes of Gx  [5] bytes of scratch  [6] 1 if Gx is current  [7] reserved, zero */
int cholmod_hip_factor_grad_info (cholmod_hip_plan *plan, double *out8) ;

/* (This entry point and the next: csrc/hip/grad.hip.)
 * The gradient with respect to the values of A, sampled on the pattern of the resident S.  dU, dV: n-by-nrhs, column-major,
 * in device memory, read only (dU == dV is legal); with perm = 1 in the caller's ordering (cholmod_hip_set_perm first),
 * with perm = 0 in the factor's.  dG: nvalues doubles in the order of the value map (the array
 * cholmod_hip_factorize_values_device takes).  For the caller's value k that the resident S reads as entry (i, j)
 *     G [k] = alpha sum_{r < nrhs} ( U [i, r] V [j, r] + [i != j] U [j, r] V [i, r] )
 * -- with U = Lambda = (A + beta I)^-1 gX, V = X = (A + beta I)^-1 B and alpha = -1 the gradient of a scalar through the
 * solve.  "Reads" is the rule of the factorization and of cholmod_hip_selinv_gather_device: on or below the diagonal of the
 * permuted S, row < n, the last of equal neighbours; every other value has no influence on L and receives exact +0.0
 * (where the gather of the selected inverse writes NaN).  All of dG [0 .. nvalues) is written.
 * One owner per entry of G, a fixed summation order, no floating-point atomics: the same inputs give the same bits.  With
 * SD_BLOCK_MIN_NRHS (8) right-hand sides or more U and V are packed through Perm into panels [n][16] and a group of 16
 * lanes reads a row as one 128-byte line; with fewer they are read in place, right-hand sides in index order.  The two
 * paths may differ by rounding.
 * Ordered on `stream` exactly as cholmod_hip_solve_device is (not during capture).  The first call of either path
 * allocates its workspace (two panels [n][16]); after that nothing is allocated and the host does not wait.
 * Work is divided by entries of S; the column of an entry comes from an i32 column-of-entry array (4 bytes of HBM per
 * entry of S) that the first call after a cholmod_hip_upload_matrix builds on the device, without a host wait.
 * Needs a resident packed S with its value map, not a numeric factor.  CHOLMOD_HIP_INVALID, before any device call: a NULL
 * plan or pointer, a host-only plan, several ranks, ld < n, nrhs < 0, nvalues other than the map's, no value map for the
 * current resident S, a product map set (the caller's values are then not entries of S), perm without a stored
 * permutation, the plans of complex factors (CHOLMOD_HIP_PHI_TWIN, CHOLMOD_HIP_CX_STORAGE).  nrhs == 0 is a success that
 * zero-fills dG; n == 0 or nvalues == 0 touches nothing. */
int cholmod_hip_values_grad_device (cholmod_hip_plan *plan, int perm, double alpha, const double *dU, int64_t ldu,
    const double *dV, int64_t ldv, int64_t nrhs, double *dG, int64_t nvalues, void *stream) ;
/* dOut [0] (device memory) = 2 sum_j log L_jj = log det (A + beta I) of the resident factor: one pass over the n diagonal
 * entries, per-workgroup partial sums in a fixed tree, then one workgroup over the partials in index order -- no
 * floating-point atomics, the same factor gives the same bits (cholmod_hip_factor_checks returns the half of it to the
 * host, waits for the stream and is not reproducible).  Ordered on `stream` as above; the first call allocates the
 * partials (n / 256 doubles), after that nothing is allocated and the host does not wait.  CHOLMOD_HIP_INVALID, before any
 * device call: a NULL plan or pointer, a host-only plan, several ranks, no numeric factor on the device, a last
 * factorization that was not positive definite, the plans of complex factors. */
int cholmod_hip_logdet_device (cholmod_hip_plan *plan, double *dOut, void *stream) ;
/* The same two gradients THROUGH A PRODUCT MAP (cholmod_hip_set_product_map: the resident S = tril (A A') is computed from
 * the navalues values a of the caller's array, M = A A' + beta I): the gradient with respect to a.  With Gv [c] the gradient
 * with respect to value c of the value map -- the sampled product above for a solve; Z once on the diagonal and twice off
 * it for log det M; +0.0 where the resident S does not read the value, never the NaN of the selected inverse's gather --
 *     dGa [q] = sum_{p : ia [p] = q} Gv [c (p)] a [ib [p]]  +  sum_{p : ib [p] = q} Gv [c (p)] a [ia [p]]
 * (a pair with ia [p] == ib [p] == q is in both sums).  Gv goes into a scratch of the plan (nc doubles), by the kernels of
 * cholmod_hip_values_grad_device or by the gather of the selected inverse; k_product_grad, the transpose of
 * k_product_values, then reads it and dA (navalues doubles on the device, the values the factor was computed from, read
 * only) into dGa: a group of 1, 16 or 64 lanes owns one q, by the length of its list, and adds its half-pairs in a fixed
 * order -- no floating-point atomics, the same inputs give the same bits.  All of dGa [0 .. navalues) is written; a value
 * that is in no pair receives +0.0.
 * The TRANSPOSED MAP (per value q its half-pairs (c, partner): 16 bytes of HBM per pair, as the forward map) is built by
 * the first of these calls after a cholmod_hip_set_product_map -- the forward lists are downloaded once, one stable
 * counting pass on the host, one upload; that call waits for the host -- and freed with the map: a caller who never
 * differentiates pays nothing.  After it nothing is allocated and the host does not wait.  Ordered on `stream` exactly as
 * cholmod_hip_values_grad_device is (not during capture).
 * cholmod_hip_product_logdet_grad_device needs a current selected inverse (cholmod_hip_selinv_device after the last
 * factorization).
 * CHOLMOD_HIP_INVALID, before any device call: a NULL plan or pointer, a host-only plan, several ranks, the plans of complex
 * factors, ld < n, nrhs < 0, NO product map set, navalues other than the product map's, no value map for the current
 * resident S, perm without a stored permutation; for the log-determinant no current selected inverse or a last
 * factorization that was not positive definite.  nrhs == 0 is a success that zero-fills dGa; n == 0 or navalues == 0
 * touches nothing.  cholmod_hip_values_grad_device and cholmod_hip_selinv_gather_device go on refusing a plan with a
 * product map: their output is in the order of the value map, which is not the caller's array then. */
int cholmod_hip_product_values_grad_device (cholmod_hip_plan *plan, int perm, double alpha, const double *dU, int64_t ldu,
    const double *dV, int64_t ldv, int64_t nrhs, const double *dA, double *dGa, int64_t navalues, void *stream) ;
int cholmod_hip_product_logdet_grad_device (cholmod_hip_plan *plan, const double *dA, double *dGa, int64_t navalues,
    void *stream) ;

/* Parity hooks: copy derived integer maps back to the host.
 *  sparent  [nsuper]     supernodal etree (reference :1025)
 *  level    [nsuper]     height of s in that tree (leaves 0)
 *  relmap   [ssize - n]  relative row maps, relmap[pi[d]-super[d] + i] = local
 *                        row in the parent of row i below d's diagonal block */
int cholmod_hip_get_maps (cholmod_hip_plan *plan, int64_t *sparent,
    int64_t *level, int64_t *relmap) ;

/* out3 = {min L_jj, max L_jj, number of NaN or negative diagonal entries} of the resident factor (one pass over the n
 * diagonal entries on the device): what cholmod_l_rcond needs (CHOLMOD/Cholesky/cholmod_rcond.c:64-161).  The extremes
 * are taken over the entries >= 0 only (+inf and 0 if there is none) and are those entries bit for bit, except that a zero
 * diagonal entry of either sign gives the minimum +0.0 (-0.0 is not a negative entry).  Several ranks: after
 * cholmod_hip_gather_factor. */
int cholmod_hip_diag_minmax (cholmod_hip_plan *plan, double *out3) ;
/* Size-independent invariants of the device-resident factor, one pass over Lx
 * (the checks CHOLMOD/Check/cholmod_check.c:1823-2000 cannot do on values, at
 * sizes no CPU oracle reaches):  out5[0] = sum_j log L(j,j)  (= logdet(A)/2,
 * known in closed form for the Poisson grids);  out5[1] = entries != 0 in the
 * dead strictly-upper triangles of the diagonal blocks (a NaN counts, -0.0
 * does not);  out5[2] = non-finite entries of the lower trapezoids;
 * out5[3] = ||L||_F^2 over the finite entries of the lower trapezoids;
 * out5[4] = diagonal entries that are not > 0: zero of either sign, negative
 * or NaN (out5[0] sums over the others only). */
int cholmod_hip_factor_checks (cholmod_hip_plan *plan, double *out5) ;
/* The same five numbers over the fronts this rank answers for (the first rank of a front's group),
 * from the rank's own part of a distributed factor: their sums over the ranks are the invariants
 * of the complete factor, no gathered copy needed. */
int cholmod_hip_factor_checks_local (cholmod_hip_plan *plan, double *out5) ;

/* Statistics of the last factorization / of the plan (doubles):
 *  [0] device seconds, whole factorization (HIP events on the engine stream)
 *  [1] executed flops (updates + panel factorizations, as SURVEY.md 8d)
 *  [2] kernel launches   [3] levels   [4] arena bytes   [5] Lx bytes
 *  [6] seconds in the 64x64 dense-update kernel   [7] its launches
 *  [8] its algorithmic flops (2*k per updated lower-trapezoid entry)
 *  [14] seconds in the 128x128 dense-update kernel (CHOLMOD_HIP_TILE128 only)
 *  [15] its algorithmic flops
 *  [16] algorithmic bytes of the 64x64 update launches: 16 B read-modify-write
 *       per updated entry + 8 B per operand entry (each panel entry once per
 *       update region)     [17] all-reduce calls   [18] all-reduce bytes
 *  [19] seconds in the fused small-front kernel  [20] its algorithmic HBM bytes
 *       (A entries aside: children CBs in, panel + CB out)   [21] fronts it handled
 *  [23] the part of [6] spent in K < 512 (panel-level) update launches
 *  [22] subtrees the schedule sweeps one after the other to fit the CB arena
 *       next to L (1 = plain level order)
 *  [9] seconds in extend-add kernels    [10] algorithmic bytes of extend-add
 *  [11] seconds in potrf kernels        [12] seconds in trsm kernels
 *  [13] seconds in assemble (memset + A scatter)
 *  [24] device seconds of the last solve of either kind (its kernels, without the
 *       copies of the right-hand side)
 *  [25] bytes of the all-gathers of [18] (as segments sent)   [39] those of them the main stream waits for at once: the
 *       near-row chunks of every block column and the far-row chunks of the last block column of an outer block (the other
 *       far-row gathers run on the exchange stream beside the chain of the following block columns)
 *  [26] trailing-update launches that also factor the next diagonal block (k_update2f: the
 *       K < 512 updates of the panel chain; NOT counted in [6]-[8], [16], [23])
 *  [27] their seconds   [28] their flops   [29] their algorithmic bytes
 *  [30] seconds of the fused solve + K = 64 update + factorization launches (k_trsm_upd)
 *  [31] their number
 *  [32] seconds in the one-wave-per-tile dense-update kernel (k_update3: the regions with
 *       >= 2048 tiles)   [33] its launches   [34] its algorithmic flops   [35] its algorithmic bytes
 *       (as [16]); the regions below that size stay with [6]-[8]
 *  [36] bytes of L this rank allocates: the fronts it holds -- of a shared front the column slabs it owns -- packed,
 *       plus the windows of the shared fronts (= [5] with one rank)
 *  [37] block columns of distributed fronts opened into their windows   [38] those whose window has a negative
 *       virtual base (the window is addressed as if the whole front were there: tests make sure both signs occur)
 *  [40] algorithmic flops the head updates leave out: the products of rows the head does not reach (exact zeros); not in
 *       [34] nor executed, still in [1]
 * Per-class seconds are only collected when profiling is enabled with
 * cholmod_hip_set_profiling(plan, 1) (it serialises the stream with events). */
#define CHOLMOD_HIP_NSTATS 41
int cholmod_hip_get_stats (cholmod_hip_plan *plan, double *stats) ;
int cholmod_hip_set_profiling (cholmod_hip_plan *plan, int on) ;
/* The launch list of the plan and, after a factorization with profiling on, the
 * device milliseconds of every launch (tuning; tools/launch_profile.py).
 * kind: 0 zero, 1 extend-add, 2 potrf, 3 trsm, 4 update(128), 5 update(64),
 * 7 all-reduce, 8 thin fronts, 9 update + factorization of the next diagonal block,
 * 10 solve + K = 64 update + factorization of the next diagonal block, 11 all-gather of a shared block column,
 * 12 update (one wave per tile, k_update3), 13 / 14 the 256-column chain as two kernels (k_diag, k_rowsolve), 15 window moves of
 * a distributed front (k_win_move), 16 the 256-column chain in one launch (k_chainf).  Fills at most cap entries of the arrays that are
 * not NULL, returns the number of launches. */
int64_t cholmod_hip_get_launch_profile (cholmod_hip_plan *plan, int64_t cap, int32_t *kind,
    int32_t *grid, int32_t *aux, double *ms, double *flops, double *bytes) ;

/* Tuning probe (plans created with CHOLMOD_HIP_THIN_TIMING set): shader cycles one
 * front of thin-front launch `launch` spent per phase: [0] requests + zero, [1] A,
 * [2] children, [3] panel chain, [4] publish + row solves, [5] store + barrier,
 * [6] trailing update / contribution block. */
int cholmod_hip_debug_thin_cycles (cholmod_hip_plan *plan, int64_t launch, long long *out10) ;
/* tuning: the update regions of one update launch, 12 numbers each (m, n, k, tri, c_in_cb, lda,
 * ldc, ntiles, nblk, front, assign, swz); returns the number of regions (tools/launch_profile.py) */
int64_t cholmod_hip_debug_launch_regions (cholmod_hip_plan *plan, int64_t launch, int64_t cap, int64_t *out) ;

/* Test hook: run the engine's dense partial factorization on ONE dense front
 * given on the host (column-major nsrow-by-nsrow, lower; the first nscol
 * columns are eliminated; on return F holds [L11; L21] in the first nscol
 * columns and the Schur complement in the rest).  Exercises potrf/trsm/update
 * kernels without any sparse structure. */
int cholmod_hip_dense_partial_factor (double *F, int64_t nsrow, int64_t nscol,
    int flags, int64_t *info) ;

const char *cholmod_hip_version (void) ;

#ifdef __cplusplus
}
#endif
#endif
