/* cholmod.h -- host-side C API of the MI355X supernodal Cholesky build.
 *
 * Mirrors the subset of the reference's cholmod_l_* API that lies on the
 * supernodal path analyze -> factorize -> solve, with
 * the same names, argument meaning and error behaviour, so a user of
 *     cholmod_l_start / cholmod_l_analyze[_p] / cholmod_l_factorize /
 *     cholmod_l_solve / cholmod_l_free_* / cholmod_l_finish
 * with Common->useGPU can switch to this library.  Reference declarations:
 *     CHOLMOD/Include/cholmod_core.h      (objects, :416 common, :1243 sparse,
 *                                          :1673 factor, :1976 dense)
 *     CHOLMOD/Include/cholmod_cholesky.h  (:89 analyze, :113 analyze_p,
 *                                          :160 factorize, :183 factorize_p,
 *                                          :216 solve, :281 etree, :311
 *                                          rowcolcounts, :634 postorder)
 *     CHOLMOD/Include/cholmod_supernodal.h(:73 super_symbolic, :100
 *                                          super_symbolic2, :126 super_numeric,
 *                                          :151 super_lsolve, :176 super_ltsolve)
 *     CHOLMOD/Include/cholmod_gpu.h       (:60-93 gpu_memorysize/probe/
 *                                          allocate/deallocate/end)
 *     CHOLMOD/Include/cholmod_check.h     (:110 gpu_stats), cholmod_matrixops.h
 *
 * Only the 64-bit integer flavour exists (the reference's GPU path is
 * cholmod_l_* only, CHOLMOD/Include/cholmod_internal.h:250-251); double
 * precision; real, complex and zomplex matrices (complex input is carried by the
 * real embedding, csrc/host/complex.c).  Common->useGPU selects the numeric path
 * as in the reference: 1 = the HIP engine (include/cholmod_hip.h), 0 = the CPU
 * supernodal path (csrc/host/cpu_numeric.c), -1 = decided by CHOLMOD_USE_GPU
 * (unset: CPU).  The struct members carry the reference's names; the structs are
 * this library's own (compile against this header).
 *
 * Where this library deliberately differs from the reference:
 *  - Common->supernodal = CHOLMOD_AUTO always picks the supernodal path (the
 *    simplicial branch is not built; CHOLMOD_SIMPLICIAL: CHOLMOD_NOT_INSTALLED);
 *  - orderings: UserPerm, natural, or the built-in nested dissection (any request
 *    for AMD / METIS / NESDIS / COLAMD maps to it, L->ordering = CHOLMOD_NESDIS);
 *  - a GPU request that cannot be served fails loudly (CHOLMOD_GPU_PROBLEM /
 *    CHOLMOD_OUT_OF_MEMORY) unless Common->hip_cpu_fallback asks for the
 *    reference's silent degradation to the CPU path;
 *  - the supernode partition is the CPU one on both paths (no devBuffSize splits);
 *  - an unsymmetric A (stype 0: factorize A*A' + beta*I) is served by forming tril (A*A') on
 *    the host and taking the symmetric path (real A; a column subset fset: A(:,f)*A(:,f)', the columns cut out first);
 *  - cholmod_l_solve2 with a sparse right-hand side (Bset) reads the columns the reference's supernodal -> simplicial
 *    conversion would produce in place (same pattern, same reach, same Xset order) and leaves L supernodal
 *    (host/subset_solve.c; the reference leaves it simplicial, Cholesky/cholmod_solve.c:1158-1180);
 *  - update/downdate and every simplicial form of L, complex triplets and
 *    complex Matrix Market files: CHOLMOD_NOT_INSTALLED / CHOLMOD_INVALID.
 */
#ifndef CHOLMOD_AMD_H
#define CHOLMOD_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int64_t SuiteSparse_long ;

#define CHOLMOD_MAIN_VERSION 3
#define CHOLMOD_SUB_VERSION 0
#define CHOLMOD_SUBSUB_VERSION 14

#ifndef TRUE
#define TRUE 1
#define FALSE 0
#endif

/* itype / dtype / xtype (cholmod_core.h:310-333) */
#define CHOLMOD_INT 0
#define CHOLMOD_INTLONG 1
#define CHOLMOD_LONG 2
#define CHOLMOD_DOUBLE 0
#define CHOLMOD_SINGLE 1
#define CHOLMOD_PATTERN 0
#define CHOLMOD_REAL 1
#define CHOLMOD_COMPLEX 2
#define CHOLMOD_ZOMPLEX 3

/* Common->status (cholmod_core.h:386-393) */
#define CHOLMOD_OK 0
#define CHOLMOD_NOT_INSTALLED (-1)
#define CHOLMOD_OUT_OF_MEMORY (-2)
#define CHOLMOD_TOO_LARGE (-3)
#define CHOLMOD_INVALID (-4)
#define CHOLMOD_GPU_PROBLEM (-5)
#define CHOLMOD_NOT_POSDEF (1)
#define CHOLMOD_DSMALL (2)

/* orderings (cholmod_core.h:397-409) */
#define CHOLMOD_NATURAL 0
#define CHOLMOD_GIVEN 1
#define CHOLMOD_AMD 2
#define CHOLMOD_METIS 3
#define CHOLMOD_NESDIS 4
#define CHOLMOD_COLAMD 5
#define CHOLMOD_POSTORDERED 6

/* Common->supernodal (cholmod_core.h:412-414) */
#define CHOLMOD_SIMPLICIAL 0
#define CHOLMOD_AUTO 1
#define CHOLMOD_SUPERNODAL 2

/* cholmod_l_solve systems (cholmod_cholesky.h:194-202) */
#define CHOLMOD_A 0
#define CHOLMOD_LDLt 1
#define CHOLMOD_LD 2
#define CHOLMOD_DLt 3
#define CHOLMOD_L 4
#define CHOLMOD_Lt 5
#define CHOLMOD_D 6
#define CHOLMOD_P 7
#define CHOLMOD_Pt 8

#define CHOLMOD_ANALYZE_FOR_SPQR 0
#define CHOLMOD_ANALYZE_FOR_CHOLESKY 1
#define CHOLMOD_ANALYZE_FOR_SPQRGPU 2

#define CHOLMOD_MAXMETHODS 9

typedef struct cholmod_method_struct
{
    double lnz ;            /* nnz(L) found by this method */
    double fl ;             /* flop count found by this method */
    int ordering ;
} cholmod_method ;

typedef struct cholmod_common_struct
{
    /* parameters (defaults: reference Core/cholmod_common.c:244-330) */
    int supernodal ;                /* CHOLMOD_AUTO by default */
    double supernodal_switch ;      /* 40 */
    int final_asis, final_super, final_ll, final_pack, final_monotonic,
        final_resymbol ;
    double zrelax [3] ;             /* 0.8, 0.1, 0.05 */
    size_t nrelax [3] ;             /* 4, 16, 48 */
    int prefer_upper ;
    int quick_return_if_not_posdef ;
    int print ;
    int nmethods ;
    int current, selected ;
    cholmod_method method [CHOLMOD_MAXMETHODS + 1] ;
    int postorder ;                 /* TRUE */
    int try_catch ;
    void (*error_handler) (int status, const char *file, int line,
        const char *message) ;
    int itype, dtype ;
    int status ;
    /* statistics */
    double fl, lnz, anz, modfl ;
    size_t malloc_count, memory_usage, memory_inuse ;
    double nrealloc_col, nrealloc_factor, ndbounds_hit ;
    double rowfacfl, aatfl ;
    int called_nd ;
    int blas_ok ;
    /* GPU control (cholmod_core.h:958-1000) */
    int useGPU ;                    /* -1: decide from CHOLMOD_USE_GPU, 0, 1 */
    size_t maxGpuMemBytes ;
    double maxGpuMemFraction ;
    size_t gpuMemorySize ;
    double gpuKernelTime ;
    SuiteSparse_long gpuFlops ;
    int gpuNumKernelLaunches ;
    size_t devBuffSize ;
    int ibuffer ;
    double syrkStart ;
    /* timers / counters printed by cholmod_l_gpu_stats (cholmod_core.h:1004) */
    double cholmod_cpu_gemm_time, cholmod_cpu_syrk_time, cholmod_cpu_trsm_time,
        cholmod_cpu_potrf_time ;
    double cholmod_gpu_gemm_time, cholmod_gpu_syrk_time, cholmod_gpu_trsm_time,
        cholmod_gpu_potrf_time ;
    double cholmod_assemble_time, cholmod_assemble_time2 ;
    size_t cholmod_cpu_gemm_calls, cholmod_cpu_syrk_calls, cholmod_cpu_trsm_calls,
        cholmod_cpu_potrf_calls ;
    size_t cholmod_gpu_gemm_calls, cholmod_gpu_syrk_calls, cholmod_gpu_trsm_calls,
        cholmod_gpu_potrf_calls ;
    /* this library: keep the numeric factor in HBM only (L->x stays NULL until
     * cholmod_l_factor_to_host is called); solves then run on the device */
    int hip_factor_on_device ;
    int hip_flags ;                 /* CHOLMOD_HIP_* plan flags */
    int hip_profile ;               /* collect per-kernel-class device times */
    /* multi-GPU, one process per GPU (see cholmod_hip.h): rank / world size of
     * this process and the host-provided sum all-reduce on device memory */
    int hip_rank, hip_world ;
    int (*hip_allreduce) (void *dev_ptr, int64_t count_doubles, int group_first,
        int group_size, void *user) ;
    void *hip_allreduce_user ;
    /* Common->useGPU == 1 but no usable device (none present, or no HBM for this
     * factor): 0 (default) = fail loudly with CHOLMOD_GPU_PROBLEM / CHOLMOD_OUT_OF_MEMORY;
     * 1 = degrade to the CPU path with status CHOLMOD_OK, as the reference does
     * (CHOLMOD/Supernodal/t_cholmod_super_numeric.c:183-192).  The environment
     * variable CHOLMOD_HIP_CPU_FALLBACK=1 sets it in cholmod_l_start. */
    int hip_cpu_fallback ;
    int prefer_zomplex ;            /* X of cholmod_l_solve: zomplex instead of complex
                                     * (reference cholmod_core.h, Cholesky/cholmod_solve.c:1112) */
    int prefer_binary ;             /* cholmod_l_read_*: a symmetric pattern-only file keeps all-one values instead of
                                     * diagonal = 1 + degree, off-diagonal = -1 (cholmod_core.h:545-560) */
    int hip_lazy_plan ;             /* 0 (default): cholmod_l_analyze of a real matrix with Common->useGPU on builds the
                                     * engine's plan -- schedule, maps, the HBM reservation for L and the contribution
                                     * blocks -- as the reference cuts its device pools inside the analysis
                                     * (cholmod_super_symbolic.c:243-327); a failure there is not an error of the analysis,
                                     * the first factorization tries again and reports.  1: at the first factorization
                                     * (or cholmod_l_hip_prepare), as until round 5 -- for callers that analyse more
                                     * patterns than the device could hold factors of */
    double hip_plan_seconds ;       /* out: what the last creation of an engine plan took (inside cholmod_l_analyze, the
                                     * first factorization or cholmod_l_hip_prepare) */
} cholmod_common ;

typedef struct cholmod_sparse_struct
{
    size_t nrow, ncol, nzmax ;
    void *p, *i, *nz, *x, *z ;
    int stype ;     /* 0 unsymmetric, >0 upper stored, <0 lower stored */
    int itype, xtype, dtype ;
    int sorted, packed ;
} cholmod_sparse ;

typedef struct cholmod_dense_struct
{
    size_t nrow, ncol, nzmax, d ;
    void *x, *z ;
    int xtype, dtype ;
} cholmod_dense ;

typedef struct cholmod_triplet_struct
{
    size_t nrow, ncol, nzmax, nnz ;
    void *i, *j, *x, *z ;
    int stype, itype, xtype, dtype ;
} cholmod_triplet ;

typedef struct cholmod_factor_struct
{
    size_t n, minor ;
    void *Perm, *ColCount, *IPerm ;
    size_t nzmax ;
    void *p, *i, *x, *z, *nz, *next, *prev ;      /* simplicial part: unused */
    size_t nsuper, ssize, xsize, maxcsize, maxesize ;
    void *super, *pi, *px, *s ;
    int ordering, is_ll, is_super, is_monotonic ;
    int itype, xtype, dtype ;
    int useGPU ;
    /* this library: the device plan + resident numeric factor */
    void *hip_plan ;
    int hip_on_device ;     /* numeric values currently valid in HBM */
    int hip_host_valid ;    /* L->x holds the current numeric values */
    /* complex factors (L->xtype == CHOLMOD_COMPLEX): the real supernodal factor of the
     * 2n x 2n embedding [re -im ; im re] the engine actually computes; the complex
     * L->x is its even columns */
    void *cx_twin ;
    /* pattern of the last matrix cholmod_l_factorize handed to the engine (hash of its
     * p / i arrays, its nnz): a call with the same pattern only refreshes the values of
     * the resident matrix (cholmod_hip_values_begin / _push_chunk) */
    uint64_t hip_apat_hash ;
    size_t hip_apat_nnz ;
    int hip_apat_valid ;
    uint64_t hip_apat_hash2 ;   /* second, independent fingerprint of the same pattern */
    int hip_is_twin ;           /* this factor IS the real twin of a complex factor (its owner's cx_twin): 1 = the
                                 * full twin (x: 4 xsize doubles), 2 = engine-only, complex storage (px = 2 x the
                                 * complex px; CHOLMOD_HIP_CX_STORAGE) */
    void *bset_work ;           /* cholmod_l_solve2 with Bset: column -> supernode, flags (2n + 1 integers, built by the first call) */
    int hip_plan_ahead ;        /* != 0: hip_plan was built inside cholmod_l_analyze and no factorization has used it yet (plan flags + 1) */
    int hip_perm_set ;          /* hip_plan holds L->Perm (cholmod_l_hip_solve_device hands it over on first use); on the twin
                                 * of a complex factor: the expanded permutation 2 Perm [k], 2 Perm [k] + 1 of that factor */
    /* cholmod_l_hip_factorize_values_device with an unsymmetric A (stype 0): hip_apat_hash is then the hash of tril (A*A')'s
     * pattern; once A's product map is on the plan these hold the hash of A's OWN pattern, all a later call pays for */
    uint64_t hip_aat_hash, hip_aat_hash2 ;
    size_t hip_aat_nnz ;
    int hip_aat_valid ;
} cholmod_factor ;

/* ---- Core ---------------------------------------------------------------- */
int cholmod_l_start (cholmod_common *Common) ;
int cholmod_l_finish (cholmod_common *Common) ;
int cholmod_l_defaults (cholmod_common *Common) ;
int cholmod_l_error (int status, const char *file, int line, const char *message,
    cholmod_common *Common) ;
void *cholmod_l_malloc (size_t n, size_t size, cholmod_common *Common) ;
void *cholmod_l_calloc (size_t n, size_t size, cholmod_common *Common) ;
void *cholmod_l_free (size_t n, size_t size, void *p, cholmod_common *Common) ;
/* CHOLMOD/Core/cholmod_memory.c:232-330; *n: current size in, new size out (unchanged on failure, old block returned) */
void *cholmod_l_realloc (size_t nnew, size_t size, void *p, size_t *n, cholmod_common *Common) ;

cholmod_sparse *cholmod_l_allocate_sparse (size_t nrow, size_t ncol, size_t nzmax,
    int sorted, int packed, int stype, int xtype, cholmod_common *Common) ;
int cholmod_l_free_sparse (cholmod_sparse **A, cholmod_common *Common) ;
cholmod_sparse *cholmod_l_copy_sparse (cholmod_sparse *A, cholmod_common *Common) ;
SuiteSparse_long cholmod_l_nnz (cholmod_sparse *A, cholmod_common *Common) ;
/* values: 0 pattern, 1 array transpose, 2 complex conjugate (== 1 for real) */
cholmod_sparse *cholmod_l_ptranspose (cholmod_sparse *A, int values,
    SuiteSparse_long *Perm, SuiteSparse_long *fset, size_t fsize,
    cholmod_common *Common) ;
cholmod_sparse *cholmod_l_transpose (cholmod_sparse *A, int values,
    cholmod_common *Common) ;

cholmod_triplet *cholmod_l_allocate_triplet (size_t nrow, size_t ncol, size_t nzmax,
    int stype, int xtype, cholmod_common *Common) ;
int cholmod_l_free_triplet (cholmod_triplet **T, cholmod_common *Common) ;
cholmod_sparse *cholmod_l_triplet_to_sparse (cholmod_triplet *T, size_t nzmax,
    cholmod_common *Common) ;

cholmod_dense *cholmod_l_allocate_dense (size_t nrow, size_t ncol, size_t d,
    int xtype, cholmod_common *Common) ;
cholmod_dense *cholmod_l_zeros (size_t nrow, size_t ncol, int xtype, cholmod_common *Common) ;
cholmod_dense *cholmod_l_ones (size_t nrow, size_t ncol, int xtype, cholmod_common *Common) ;
cholmod_dense *cholmod_l_copy_dense (cholmod_dense *X, cholmod_common *Common) ;
int cholmod_l_free_dense (cholmod_dense **X, cholmod_common *Common) ;

int cholmod_l_free_factor (cholmod_factor **L, cholmod_common *Common) ;

/* ---- Check / IO ------------------------------------------------------------ */
/* Check/cholmod_read.c (cholmod_check.h:251-330): triplet ("coordinate") and dense ("array") files, Matrix Market banner
 * optional, real / complex / pattern */
#define CHOLMOD_SPARSE 1            /* *mtype of cholmod_l_read_matrix (cholmod_core.h:300-303) */
#define CHOLMOD_DENSE 3
#define CHOLMOD_TRIPLET 4
cholmod_sparse *cholmod_l_read_sparse (FILE *f, cholmod_common *Common) ;
cholmod_triplet *cholmod_l_read_triplet (FILE *f, cholmod_common *Common) ;
cholmod_dense *cholmod_l_read_dense (FILE *f, cholmod_common *Common) ;
void *cholmod_l_read_matrix (FILE *f, int prefer, int *mtype, cholmod_common *Common) ;
int cholmod_l_check_factor (cholmod_factor *L, cholmod_common *Common) ;
int cholmod_l_check_sparse (cholmod_sparse *A, cholmod_common *Common) ;
int cholmod_l_gpu_stats (cholmod_common *Common) ;

/* ---- MatrixOps --------------------------------------------------------------- */
int cholmod_l_sdmult (cholmod_sparse *A, int transpose, double alpha [2],
    double beta [2], cholmod_dense *X, cholmod_dense *Y, cholmod_common *Common) ;
double cholmod_l_norm_dense (cholmod_dense *X, int norm, cholmod_common *Common) ;
double cholmod_l_norm_sparse (cholmod_sparse *A, int norm, cholmod_common *Common) ;

/* ---- Cholesky ---------------------------------------------------------------- */
cholmod_factor *cholmod_l_analyze (cholmod_sparse *A, cholmod_common *Common) ;
cholmod_factor *cholmod_l_analyze_p (cholmod_sparse *A, SuiteSparse_long *UserPerm,
    SuiteSparse_long *fset, size_t fsize, cholmod_common *Common) ;
cholmod_factor *cholmod_l_analyze_p2 (int for_whom, cholmod_sparse *A,
    SuiteSparse_long *UserPerm, SuiteSparse_long *fset, size_t fsize,
    cholmod_common *Common) ;
int cholmod_l_factorize (cholmod_sparse *A, cholmod_factor *L, cholmod_common *Common) ;
int cholmod_l_factorize_p (cholmod_sparse *A, double beta [2], SuiteSparse_long *fset,
    size_t fsize, cholmod_factor *L, cholmod_common *Common) ;
cholmod_dense *cholmod_l_solve (int sys, cholmod_factor *L, cholmod_dense *B,
    cholmod_common *Common) ;
int cholmod_l_solve2 (int sys, cholmod_factor *L, cholmod_dense *B, cholmod_sparse *Bset,
    cholmod_dense **X_Handle, cholmod_sparse **Xset_Handle, cholmod_dense **Y_Handle,
    cholmod_dense **E_Handle, cholmod_common *Common) ;
/* CHOLMOD/Include/cholmod_cholesky.h:601-614: (min diag L / max diag L)^2; -1 error, 0 singular / NaN / failed factor */
double cholmod_l_rcond (cholmod_factor *L, cholmod_common *Common) ;
/* CHOLMOD/Include/cholmod_core.h:1852-1872; here: supernodal symbolic <-> supernodal numeric (the simplicial forms:
 * CHOLMOD_NOT_INSTALLED) */
int cholmod_l_change_factor (int to_xtype, int to_ll, int to_super, int to_packed, int to_monotonic,
    cholmod_factor *L, cholmod_common *Common) ;
int cholmod_l_etree (cholmod_sparse *A, SuiteSparse_long *Parent, cholmod_common *Common) ;
SuiteSparse_long cholmod_l_postorder (SuiteSparse_long *Parent, size_t n,
    SuiteSparse_long *Weight, SuiteSparse_long *Post, cholmod_common *Common) ;
int cholmod_l_rowcolcounts (cholmod_sparse *A, SuiteSparse_long *fset, size_t fsize,
    SuiteSparse_long *Parent, SuiteSparse_long *Post, SuiteSparse_long *RowCount,
    SuiteSparse_long *ColCount, SuiteSparse_long *First, SuiteSparse_long *Level,
    cholmod_common *Common) ;

/* ---- Supernodal -------------------------------------------------------------- */
int cholmod_l_super_symbolic (cholmod_sparse *A, cholmod_sparse *F,
    SuiteSparse_long *Parent, cholmod_factor *L, cholmod_common *Common) ;
int cholmod_l_super_symbolic2 (int for_whom, cholmod_sparse *A, cholmod_sparse *F,
    SuiteSparse_long *Parent, cholmod_factor *L, cholmod_common *Common) ;
int cholmod_l_super_numeric (cholmod_sparse *A, cholmod_sparse *F, double beta [2],
    cholmod_factor *L, cholmod_common *Common) ;
int cholmod_l_super_lsolve (cholmod_factor *L, cholmod_dense *X, cholmod_dense *E,
    cholmod_common *Common) ;
int cholmod_l_super_ltsolve (cholmod_factor *L, cholmod_dense *X, cholmod_dense *E,
    cholmod_common *Common) ;

/* ---- GPU --------------------------------------------------------------------- */
int cholmod_l_gpu_memorysize (size_t *total_mem, size_t *available_mem,
    cholmod_common *Common) ;
int cholmod_l_gpu_probe (cholmod_common *Common) ;
int cholmod_l_gpu_deallocate (cholmod_common *Common) ;
void cholmod_l_gpu_end (cholmod_common *Common) ;
int cholmod_l_gpu_allocate (cholmod_common *Common) ;
/* int-flavour counterparts: inert, as in the reference (cholmod_gpu.c:84-86) */
int cholmod_gpu_memorysize (size_t *total_mem, size_t *available_mem, cholmod_common *Common) ;
int cholmod_gpu_probe (cholmod_common *Common) ;
int cholmod_gpu_deallocate (cholmod_common *Common) ;
void cholmod_gpu_end (cholmod_common *Common) ;
int cholmod_gpu_allocate (cholmod_common *Common) ;

/* ---- this library only --------------------------------------------------------- */
/* Materialise L->x on the host from the device-resident factor. */
int cholmod_l_factor_to_host (cholmod_factor *L, cholmod_common *Common) ;
/* Device time and per-class statistics of the last factorization
 * (CHOLMOD_HIP_NSTATS doubles, see cholmod_hip.h). */
int cholmod_l_hip_stats (cholmod_factor *L, double *stats, cholmod_common *Common) ;
/* cholmod_l_solve for right-hand sides that live in device memory: B_dev (n-by-nrhs doubles, column-major, leading
 * dimension ldb, read only) and X_dev (leading dimension ldx; B_dev == X_dev with ldb == ldx is legal) are device pointers,
 * `stream` is the caller's hipStream_t (NULL: the null stream).  The solve is ordered on that stream -- behind what the caller
 * has enqueued, ahead of what it enqueues next -- and the host neither waits for it nor copies anything (see
 * cholmod_hip_solve_device in cholmod_hip.h; not during stream capture).  sys: the nine codes, with the meaning
 * cholmod_l_solve gives them for an LL' factor.  Real supernodal numeric factors with Common->useGPU on only: there is no
 * host fallback for device pointers (Common->hip_cpu_fallback does not apply).  FALSE with CHOLMOD_INVALID for a NULL
 * pointer, sys out of range, ld < n, a symbolic L or the GPU switched off; with CHOLMOD_NOT_INSTALLED for a complex or
 * zomplex L -- all checked before a device is touched.  nrhs == 0 is a success that touches nothing. */
int cholmod_l_hip_solve_device (int sys, cholmod_factor *L, const double *B_dev, size_t ldb, double *X_dev, size_t ldx,
    size_t nrhs, void *stream, cholmod_common *Common) ;
/* What follows a device solve, without leaving the device.  R_dev = B_dev - A X_dev (cholmod_l_hip_residual_device) and
 * `steps` rounds of iterative refinement X_dev += (LL')^-1 (B_dev - A X_dev), in place (cholmod_l_hip_refine_device), in
 * the caller's ordering.  "A" is the matrix L was last factorized from on the device, which is still resident there: A
 * itself for a symmetric A, A*A' for stype == 0, A(:,f)*A(:,f)' with an fset, each plus beta*I with the beta of that
 * factorization.  Arrays, leading dimensions and `stream` as for cholmod_l_hip_solve_device; X_dev and B_dev are read only
 * by the residual, R_dev may be B_dev (same ld) but not X_dev.  Rnorm_dev: NULL, or nrhs doubles on the device that
 * receive max_i |R (i,k)| (refine: of the final X; steps == 0 leaves X untouched and only reports them).  Two calls on the
 * same inputs give bit-identical R and norms (cholmod_hip_residual_device in cholmod_hip.h).
 * FALSE with CHOLMOD_INVALID for a NULL pointer, ld < n, steps < 0, R_dev == X_dev, a symbolic L, the GPU switched off
 * (no host fallback: Common->hip_cpu_fallback does not apply; host arrays are cholmod_l_sdmult's) or an L that was not
 * factorized on the device (no resident matrix); with CHOLMOD_NOT_INSTALLED for a complex or zomplex L -- all checked
 * before a device is touched.  One rank only.  nrhs == 0 is a success that touches nothing. */
int cholmod_l_hip_residual_device (cholmod_factor *L, const double *X_dev, size_t ldx, const double *B_dev, size_t ldb,
    double *R_dev, size_t ldr, size_t nrhs, double *Rnorm_dev, void *stream, cholmod_common *Common) ;
int cholmod_l_hip_refine_device (cholmod_factor *L, const double *B_dev, size_t ldb, double *X_dev, size_t ldx,
    size_t nrhs, int steps, double *Rnorm_dev, void *stream, cholmod_common *Common) ;
/* The same three for a complex factor: L is the complex supernodal factor of a Hermitian A (computed from complex or
 * zomplex input) whose last factorization ran on the engine, one rank.  B_dev, X_dev and R_dev hold interleaved complex
 * doubles (re, im), n-by-nrhs, column-major, leading dimensions in COMPLEX elements; rows n .. ld-1 are neither read nor
 * written; B_dev == X_dev with equal ld is legal, R_dev may be B_dev and must not be X_dev.  sys as in cholmod_l_solve:
 * CHOLMOD_Lt and CHOLMOD_DLt mean L^H, D is the identity.  Rnorm_dev [k] (nrhs real doubles, NULL allowed) is what the
 * engine forms on the real twin of L: max_i max (|re R (i,k)|, |im R (i,k)|), not the complex modulus.  Stream ordering,
 * the bit-identical residual of two calls and "nothing allocated after the first call" are those of the real entry points
 * above; the solves run on the twin's plan (8 or more right-hand sides in panels of 16 on v_mfma_f64_16x16x4, L read once
 * per panel in its complex storage).
 * FALSE, before any device call: with CHOLMOD_INVALID for a NULL pointer, sys out of range, ld < n, steps < 0,
 * R_dev == X_dev, a real, pattern or simplicial L (a real L has the entry points above), the GPU switched off, several
 * ranks, or an L whose factor is not on the device (there is never a host fallback); with CHOLMOD_NOT_INSTALLED for a
 * zomplex L.  nrhs == 0 or n == 0 is a success that touches nothing. */
int cholmod_l_hip_solve_device_complex (int sys, cholmod_factor *L, const void *B_dev, size_t ldb, void *X_dev, size_t ldx,
    size_t nrhs, void *stream, cholmod_common *Common) ;
int cholmod_l_hip_residual_device_complex (cholmod_factor *L, const void *X_dev, size_t ldx, const void *B_dev, size_t ldb,
    void *R_dev, size_t ldr, size_t nrhs, double *Rnorm_dev, void *stream, cholmod_common *Common) ;
int cholmod_l_hip_refine_device_complex (cholmod_factor *L, const void *B_dev, size_t ldb, void *X_dev, size_t ldx,
    size_t nrhs, int steps, double *Rnorm_dev, void *stream, cholmod_common *Common) ;
/* The selected inverse (the sparse inverse subset; the reference ships it as MATLAB_Tools/sparseinv): the entries of
 * Z = (A + beta I)^-1 on the pattern of L -- hence on the pattern of A -- for the A and beta L was last factorized from ON
 * THE DEVICE, computed there from the resident factor (cholmod_hip_selinv_device: supernodal Takahashi on fp64 MFMA).
 * Marginal variances of a Gaussian Markov random field, the gradient of log det A, trace estimators.
 * cholmod_l_hip_selinv_device: Z_dev (NULL, or a device pointer to nnz (A) doubles) receives Z at every entry of A, in A's
 * entry order -- a quiet NaN where the factorization does not read A (the ignored triangle of a symmetric A, entries
 * outside L's pattern); diag_dev (NULL, or n doubles on the device) receives diag (Z) in A's ordering.  A gives the
 * PATTERN only and is hashed against the record of the values-only path (L->hip_apat_valid) exactly as
 * cholmod_l_hip_factorize_values_device does: a mismatch touches no device state; A == NULL is legal when Z_dev is.
 * The inverse is computed if the resident one is stale (any factorization makes it so), then gathered; the call takes its
 * place on `stream` as cholmod_l_hip_solve_device does and the host does not wait once the workspaces exist.
 * FALSE with CHOLMOD_INVALID for a NULL L, both outputs NULL, a symbolic L, L->minor < n, the GPU switched off (no host
 * fallback: Common->hip_cpu_fallback does not apply), several ranks, an L not factorized on the device; with Z_dev also
 * for a NULL, unsymmetric (stype == 0: A*A' and column subsets are not served) or unpacked A, mismatched dimensions, an L
 * without the pattern record; with CHOLMOD_NOT_INSTALLED for a complex or zomplex A or L -- all before a device is touched. */
int cholmod_l_hip_selinv_device (cholmod_sparse *A, cholmod_factor *L, double *Z_dev, double *diag_dev, void *stream,
    cholmod_common *Common) ;
/* The whole subset on the host: Zx receives L->xsize doubles indexed by L->super / pi / px / s exactly like L->x
 * (Z (s [pi [k] + i], super [k] + j), i >= j, at px [k] + i + j nsrow; zeros above the diagonal of the diagonal blocks), in
 * the factor's ordering.  Computes the inverse if it is stale and waits for it.  Refusals as above. */
int cholmod_l_hip_selinv_to_host (cholmod_factor *L, double *Zx, cholmod_common *Common) ;
/* The Schur complement onto a set S of m variables and the two condensed solves that go with it (csrc/host/schur.c), for
 * the A and beta L was last factorized from ON THE DEVICE.  S is the LAST m positions of the factor's ordering:
 *     row i of Sc, F, G and XS is variable L->Perm [n - m + i] of the caller's matrix
 * -- that is the contract.  With a nested-dissection ordering these are the top separators; to condense onto a chosen set,
 * order it last (analyze with a permutation that ends with it, Common->postorder = FALSE).  Any m may be chosen after the
 * factorization, and several from one factor; the factorization itself is not touched.  With I the other n - m variables:
 * cholmod_l_hip_schur_device: S_dev (NULL, or m-by-m doubles on the device, column-major, lds >= m) receives
 *     Sc = (A + beta I)_SS - (A + beta I)_SI inv ((A + beta I)_II) (A + beta I)_IS,
 * both triangles, bitwise symmetric -- the marginal precision of x_S of a Gaussian Markov random field, the interface matrix
 * of a substructure; F_dev (NULL, or m-by-m, ldf >= m) its Cholesky factor, Sc = F F': the trailing triangle of L, dense,
 * exact +0.0 above the diagonal.  Not both NULL.  The same factor gives the same bits.
 * cholmod_l_hip_schur_reduce_device: B_dev (n-by-nrhs, column-major, ldb >= n, the caller's ordering, read only); Y_dev
 * (n-by-nrhs, ldy >= n) receives inv (L) P B in the FACTOR's ordering, which the caller keeps for the expansion; G_dev
 * (m-by-nrhs, ldg >= m) receives the condensed right-hand side B_S - (A + beta I)_SI inv ((A + beta I)_II) B_I.
 * cholmod_l_hip_schur_expand_device: XS_dev (m-by-nrhs, ldxs >= m, read only) is the solution on S -- of Sc x_S = G, or of
 * whatever the caller has added to both --; Y_dev is what the reduction left, read only; X_dev (n-by-nrhs, ldx >= n, not
 * Y_dev, not overlapping XS_dev) receives the solution on all variables in the caller's ordering: x_S on S, and
 * inv ((A + beta I)_II) (B_I - (A + beta I)_IS x_S) on I.  With m == 0 it is the plain solve P' inv (L') Y.
 * All three take their place on `stream` as cholmod_l_hip_solve_device does; the host does not wait once the workspaces
 * exist.  m == 0 (but for the expansion) or nrhs == 0: success, nothing touched.
 * FALSE with CHOLMOD_INVALID for a NULL L or array, m > n, a leading dimension too small, a symbolic or simplicial L,
 * L->minor < n, the GPU switched off (no host fallback: Common->hip_cpu_fallback does not apply), several ranks, an L not
 * factorized on the device; with CHOLMOD_NOT_INSTALLED for a complex or zomplex L -- all before a device is touched. */
int cholmod_l_hip_schur_device (cholmod_factor *L, size_t m, double *S_dev, size_t lds, double *F_dev, size_t ldf,
    void *stream, cholmod_common *Common) ;
int cholmod_l_hip_schur_reduce_device (cholmod_factor *L, size_t m, const double *B_dev, size_t ldb, double *Y_dev, size_t ldy,
    double *G_dev, size_t ldg, size_t nrhs, void *stream, cholmod_common *Common) ;
int cholmod_l_hip_schur_expand_device (cholmod_factor *L, size_t m, const double *Y_dev, size_t ldy, const double *XS_dev,
    size_t ldxs, double *X_dev, size_t ldx, size_t nrhs, void *stream, cholmod_common *Common) ;
/* What backpropagation through the device path needs (csrc/host/grad.c; suitesparse_amd/autograd.py ties them into
 * torch.autograd.Functions).  cholmod_l_hip_values_grad_device: G_dev (nnz (A) doubles on the device, A's entry order)
 * receives, for every entry (i, j) of A the factorization reads,
 *     alpha sum_{r < nrhs} ( U [i, r] V [j, r] + [i != j] U [j, r] V [i, r] )
 * and exact +0.0 at every other entry (the ignored triangle, where the selected inverse gives NaN).  U_dev, V_dev: n-by-nrhs,
 * column-major, on the device, in A's ordering, read only; they may be the same array.  With X = (A + beta I)^-1 B,
 * Lambda = (A + beta I)^-1 gX, U = Lambda, V = X and alpha = -1 this is the gradient of a scalar with respect to A's values
 * through the solve; the gradient with respect to B is Lambda itself.  A gives the PATTERN only and is hashed against
 * L->hip_apat_* exactly as cholmod_l_hip_selinv_device does; a mismatch touches no device state.  Perm is handed to the
 * plan on first use, as cholmod_l_hip_solve_device does.  Ordered on `stream`; the same inputs give the same bits.
 * cholmod_l_hip_logdet_device: out_dev [0] (one double on the device) = log det (A + beta I) = 2 sum log L_jj of the factor
 * resident on the device, in stream order and with the same bits every time; its gradient with respect to A's values is
 * the selected inverse, once on the diagonal and twice off it.
 * Both return FALSE with CHOLMOD_INVALID for NULL pointers, an unpacked A, an A with stype == 0, mismatched dimensions, a
 * leading dimension smaller than n, a symbolic L, the GPU switched off (no host fallback), several ranks, an L not
 * factorized on the device or without the pattern record -- the log-determinant also for L->minor < n --, with
 * CHOLMOD_NOT_INSTALLED for a complex or zomplex A or L: all before a device is touched. */
int cholmod_l_hip_values_grad_device (cholmod_sparse *A, cholmod_factor *L, double alpha, const double *U_dev, size_t ldu,
    const double *V_dev, size_t ldv, size_t nrhs, double *G_dev, void *stream, cholmod_common *Common) ;
int cholmod_l_hip_logdet_device (cholmod_factor *L, double *out_dev, void *stream, cholmod_common *Common) ;
/* The same two gradients for an UNSYMMETRIC A (stype == 0), through L L' = M = A*A' + beta*I as
 * cholmod_l_hip_factorize_values_device forms it: the gradient with respect to the nnz (A) values of A, in A's entry order.
 * Avalues_dev: the values L was factorized from (nnz (A) doubles on the device, read only; A->x is never read), G_dev:
 * nnz (A) doubles on the device, all written.
 * cholmod_l_hip_aat_values_grad_device: with G = alpha (U V' + V U') sampled on tril (M) as above (twice off the diagonal),
 *     G_dev [q] = sum over the entries (j, k) of column k of the entry q = (i, k):  G (i, j) a (j, k)       (2 G (i, i) a_q at j == i)
 * -- with U = Lambda = M^-1 gX, V = X = M^-1 B and alpha = -1 the gradient of a scalar through the solve, -(Lambda X' +
 * X Lambda') A sampled on A; the gradient with respect to beta is alpha sum_r sum_i U [i, r] V [i, r], a reduction the caller
 * forms.  cholmod_l_hip_aat_logdet_grad_device: the gradient of log det M, 2 (Z A) sampled on A with Z = M^-1 the selected
 * inverse, computed now if the resident one is stale; with respect to beta it is trace Z (cholmod_l_hip_selinv_device's
 * diag_dev, summed).
 * The product map is built by the first call for this pattern if cholmod_l_hip_factorize_values_device has not built it
 * (the same host pass), its transpose by the first gradient call after that: one download of the lists, a counting pass
 * on the host, 16 more bytes of HBM per pair; a caller who never differentiates pays nothing.  Ordered on `stream`; one
 * owner per entry of G_dev, a fixed summation order, no floating-point atomics: the same inputs give the same bits.
 * FALSE with CHOLMOD_INVALID for NULL pointers, a SYMMETRIC A (stype != 0: cholmod_l_hip_values_grad_device), an unpacked A,
 * A->nrow != L->n, a leading dimension smaller than n, a symbolic L, the GPU switched off (no host fallback), several
 * ranks, an L not factorized on the device or without the pattern record, an A*A' of another pattern than L was factorized
 * from (an fset is not supported) -- the log-determinant also for L->minor < n --, with CHOLMOD_NOT_INSTALLED for a
 * complex or zomplex A or L: all before a device is touched. */
int cholmod_l_hip_aat_values_grad_device (cholmod_sparse *A, cholmod_factor *L, double alpha, const double *U_dev, size_t ldu,
    const double *V_dev, size_t ldv, size_t nrhs, const double *Avalues_dev, double *G_dev, void *stream,
    cholmod_common *Common) ;
int cholmod_l_hip_aat_logdet_grad_device (cholmod_sparse *A, cholmod_factor *L, const double *Avalues_dev, double *G_dev,
    void *stream, cholmod_common *Common) ;
/* The gradient THROUGH THE FACTOR (csrc/host/factor_grad.c; the engine's cholmod_hip_factor_grad_*: reverse-mode Cholesky,
 * the sweep of the selected inverse with another recurrence).  For a scalar f of the entries of L -- a reparameterised
 * sample P' inv (L') z, a whitened vector inv (L) P b, any function of L --, with L L' = P (A + beta I) P':
 * cholmod_l_hip_factor_grad_device takes Lbar_dev = df/dL (L->xsize doubles on the device in the layout of L->x, read only;
 * the dead upper triangles of the diagonal blocks are ignored); cholmod_l_hip_factor_outer_grad_device forms
 * Lbar (i, j) = alpha sum_{r < nrhs} P (i, r) Q (j, r) on the pattern of L itself, P_dev and Q_dev n-by-nrhs, column-major, on
 * the device, in the FACTOR's ordering (what cholmod_l_hip_solve_device returns for CHOLMOD_L and CHOLMOD_Lt), read only,
 * possibly the same array.  For x = inv (L') z and an incoming gx, with u = inv (L) gx:  P = x, Q = u, alpha = -1, and the
 * gradient with respect to z is u; for y = inv (L) b and gy, with v = inv (L') gy:  P = v, Q = y, alpha = -1, and the one
 * with respect to b is v.
 * G_dev (NULL, or nnz (A) doubles on the device, A's entry order) receives df/d (the value of A at that entry): for an entry
 * the factorization reads, df/dS at the stored entry of the lower-stored S it is read into; exact +0.0 at every other
 * entry.  trace_dev (NULL, or one double on the device) receives df/dbeta, the trace of df/dS.  A gives the PATTERN only and
 * is hashed against L->hip_apat_* exactly as cholmod_l_hip_selinv_device does; A == NULL is legal when G_dev is.
 * cholmod_l_hip_factor_grad_to_host: Gx receives the whole of df/dS on the pattern of L, L->xsize doubles indexed like L->x,
 * of the last of the two calls above; it waits for it.  A factorization since then makes it stale: CHOLMOD_INVALID.
 * The calls take their place on `stream` as cholmod_l_hip_selinv_device does; the same inputs give the same bits.
 * FALSE with CHOLMOD_INVALID for NULL pointers, a symbolic L, L->minor < n, the GPU switched off (no host fallback), several
 * ranks, an L not factorized on the device, a leading dimension smaller than n; with G_dev also for an unsymmetric
 * (stype == 0) or unpacked A, mismatched dimensions, an L without the pattern record; with CHOLMOD_NOT_INSTALLED for a complex
 * or zomplex A or L -- all before a device is touched. */
int cholmod_l_hip_factor_grad_device (cholmod_sparse *A, cholmod_factor *L, const double *Lbar_dev, double *G_dev,
    double *trace_dev, void *stream, cholmod_common *Common) ;
int cholmod_l_hip_factor_outer_grad_device (cholmod_sparse *A, cholmod_factor *L, double alpha, const double *P_dev, size_t ldp,
    const double *Q_dev, size_t ldq, size_t nrhs, double *G_dev, double *trace_dev, void *stream, cholmod_common *Common) ;
int cholmod_l_hip_factor_grad_to_host (cholmod_factor *L, double *Gx, cholmod_common *Common) ;
/* cholmod_l_factorize for new VALUES of A that already live in device memory (a matrix assembled on the GPU: the step of a
 * Newton, time-stepping or interior-point loop), without a trip through the host.  A supplies the PATTERN only (p, i,
 * stype, packed; A->x is never read and may be NULL); Ax_dev is a device pointer to nnz (A) doubles in A's own entry
 * order, read only; `stream` is the caller's hipStream_t (NULL: the null stream), and the call takes its place on it as
 * cholmod_l_hip_solve_device does: behind what the caller has enqueued (the kernels that produce Ax_dev), ahead of what it
 * enqueues next (not during stream capture).
 * PRECONDITION: L was last factorized on the device by cholmod_l_factorize (_p) from a HOST matrix of this pattern, without
 * an fset -- that call left the plan, the resident matrix, its value map and the pattern hash.  The call hashes A's
 * pattern as the values-only path of cholmod_l_factorize does; on a mismatch it returns FALSE with CHOLMOD_INVALID,
 * touches no device state and L keeps its factor.
 * stype == 0: L L' = A*A' + beta*I.  The resident matrix is tril (A*A') and its values are formed on the device from
 * Ax_dev (cholmod_hip_set_product_map); the first such call forms the pattern of A*A' symbolically, checks its hash and
 * builds the product map (cholmod_l_hip_aat_product_map) -- a host pass and 16 bytes of HBM per pair that a caller who
 * never uses this entry does not pay --, later calls hash A only.
 * THE CALL RETURNS WHEN THE FACTORIZATION HAS FINISHED ON THE DEVICE, with the result of cholmod_l_factorize: L->minor is
 * set, CHOLMOD_NOT_POSDEF is a warning status with TRUE, the host copy L->x is stale (cholmod_l_factor_to_host; with
 * Common->hip_factor_on_device off it is downloaded as usual).  Ax_dev may be overwritten once the call has returned.
 * The host values-only path keeps working afterwards, and the device solve, residual and refinement see the new matrix.
 * FALSE with CHOLMOD_INVALID for NULL pointers, an unpacked A, mismatched dimensions, a symbolic L, an L without the
 * pattern record (L->hip_apat_valid unset), several ranks, the GPU switched off (no host fallback for device pointers:
 * Common->hip_cpu_fallback does not apply); with CHOLMOD_NOT_INSTALLED for a complex or zomplex A or L -- all checked
 * before a device is touched. */
int cholmod_l_hip_factorize_values_device (cholmod_sparse *A, const double *Ax_dev, double beta [2],
    cholmod_factor *L, void *stream, cholmod_common *Common) ;
/* The values of C = tril (A*A') as sums of products of the values of an unsymmetric A (stype 0): entry c of C, in the
 * entry order of the lower triangle by sorted columns, is sum over p = cp [c] .. cp [c+1]-1 of Ax [ia [p]] * Ax [ib [p]],
 * the pairs of a list by ascending column of A.  Pure integer work on the host; returns the number of pairs, -1 on invalid
 * input; cp [0 .. nnz (C)], ia, ib are filled where they are not NULL (all NULL: the count only). */
int64_t cholmod_l_hip_aat_product_map (cholmod_sparse *A, int64_t *cp, int64_t *ia, int64_t *ib, cholmod_common *Common) ;
/* Where the relaxed fronts of an analysed L hold explicit zeros (cholmod_hip_plan_create_reach's reach_p / reach_first for
 * A's pattern and L's permutation): fills reach_p [0 .. nsuper] and, if reach_first is not NULL, reach_first; returns the
 * length of reach_first, -1 on invalid input.  cholmod_l_analyze computes the same for the plan it builds. */
int64_t cholmod_l_hip_front_reach (cholmod_sparse *A, cholmod_factor *L, int64_t *reach_p, int32_t *reach_first,
    cholmod_common *Common) ;
/* Create the device plan of a symbolic factor now (HBM reservation for L and the
 * contribution blocks) instead of at the first numeric factorization; FALSE with
 * CHOLMOD_OUT_OF_MEMORY if the device cannot hold it. */
int cholmod_l_hip_prepare (cholmod_factor *L, cholmod_common *Common) ;
/* Multi-GPU: complete the factor on every rank after a distributed
 * factorization (needed before cholmod_l_solve / cholmod_l_factor_to_host). */
int cholmod_l_gather_factor (cholmod_factor *L, cholmod_common *Common) ;
/* Re-run the numeric factorization on the matrix already resident in HBM. */
int cholmod_l_refactorize_resident (double beta [2], cholmod_factor *L,
    cholmod_common *Common) ;

#ifdef __cplusplus
}
#endif
#endif
