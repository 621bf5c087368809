/* numeric.c -- cholmod_l_factorize / cholmod_l_super_numeric / cholmod_l_solve
 * and the cholmod_l_gpu_* entry points of the host layer.  With Common->useGPU
 * the arithmetic is done by the HIP engine behind include/cholmod_hip.h; this
 * file checks arguments, permutes the input (ptranspose), moves vectors and
 * maps engine return codes to Common->status.  With Common->useGPU == 0, or when
 * no device can be used, the CPU path of cpu_numeric.c runs instead, as in the
 * reference (t_cholmod_super_numeric.c:183-192).
 *
 * Reference files: CHOLMOD/Cholesky/cholmod_factorize.c, cholmod_solve.c;
 * CHOLMOD/Supernodal/cholmod_super_numeric.c, cholmod_super_solve.c;
 * CHOLMOD/GPU/cholmod_gpu.c. */
#include "host_internal.h"
#ifdef _OPENMP
#include <omp.h>
#else
static int omp_get_thread_num (void) { return 0 ; }
#endif
#include <time.h>

/* ---- GPU entry points (reference CHOLMOD/GPU/cholmod_gpu.c:71-486) ---------------- */

int cholmod_l_gpu_memorysize (size_t *total_mem, size_t *available_mem, cholmod_common *Common)
{
    if (total_mem) *total_mem = 0 ;
    if (available_mem) *available_mem = 0 ;
    if (!Common) return 1 ;
    return cholmod_hip_memorysize (total_mem, available_mem) ;
}

int cholmod_l_gpu_probe (cholmod_common *Common)
{
    if (!Common) return 0 ;
    if (!cholmod_hip_probe ()) return 0 ;
    size_t t = 0, a = 0 ;
    if (cholmod_hip_memorysize (&t, &a) == 0) Common->gpuMemorySize = a ;
    return 1 ;
}

/* The reference carves Common->dev_mempool / host_pinned_mempool here
 * (cholmod_gpu.c:364-486).  The HIP engine keeps L itself resident and sizes
 * its HBM reservation per symbolic factor (cholmod_hip_plan_create), so these
 * two calls only validate that a device exists.  0 = ok, as in the reference. */
/* int-flavour symbols: present and inert in the reference (#ifndef DLONG return 0,
 * CHOLMOD/GPU/cholmod_gpu.c:84-86, :176, :216, :262, :372); kept so that code linking
 * both flavours resolves. */
int cholmod_gpu_memorysize (size_t *total_mem, size_t *available_mem, cholmod_common *Common)
{
    (void) Common ;
    if (total_mem) *total_mem = 0 ;
    if (available_mem) *available_mem = 0 ;
    return 0 ;
}
int cholmod_gpu_probe (cholmod_common *Common) { (void) Common ; return 0 ; }
int cholmod_gpu_deallocate (cholmod_common *Common) { (void) Common ; return 0 ; }
void cholmod_gpu_end (cholmod_common *Common) { (void) Common ; }
int cholmod_gpu_allocate (cholmod_common *Common) { (void) Common ; return 0 ; }

int cholmod_l_gpu_allocate (cholmod_common *Common)
{
    if (!Common) return 1 ;
    return cholmod_hip_probe () ? 0 : 1 ;
}

int cholmod_l_gpu_deallocate (cholmod_common *Common)
{
    if (!Common) return 1 ;
    return 0 ;
}

void cholmod_l_gpu_end (cholmod_common *Common)
{
    (void) Common ;
}

/* ---- plan management ------------------------------------------------------------------ */

static int map_hip_status (int rc, cholmod_common *Common, const char *what)
{
    switch (rc)
    {
        case CHOLMOD_HIP_OK: return TRUE ;
        case CHOLMOD_HIP_NOT_POSDEF: return TRUE ;
        case CHOLMOD_HIP_OUT_OF_MEMORY: ERROR (CHOLMOD_OUT_OF_MEMORY, what) ; return FALSE ;
        case CHOLMOD_HIP_INVALID: ERROR (CHOLMOD_INVALID, what) ; return FALSE ;
        case CHOLMOD_HIP_TOO_LARGE: ERROR (CHOLMOD_TOO_LARGE, "problem too large for the HIP engine (32-bit maps)") ; return FALSE ;
        case CHOLMOD_HIP_NO_DEVICE:
            ERROR (CHOLMOD_GPU_PROBLEM, "no usable HIP device: the numeric factorization of this "
                "library runs only on the GPU engine") ;
            return FALSE ;
        default: ERROR (CHOLMOD_GPU_PROBLEM, what) ; return FALSE ;
    }
}

/* A factor analysed with CHOLMOD_ANALYZE_FOR_SPQR carries the row structure only:
 * px [0] = 123456, the other px zero, xsize = 1 (cholmod_super_symbolic.c:662-663, :749-771).
 * Nothing numeric may be built on it. */
int ssamd_factor_has_cholesky_sizes (const cholmod_factor *L)
{
    if (!L || !L->is_super || !L->px || !L->super || !L->pi) return FALSE ;
    const Int *px = L->px ;
    if (L->nsuper > 0 && px [0] == 123456) return FALSE ;
    return (size_t) px [L->nsuper] <= L->xsize ;
}

/* the plan flags a factorization of L would ask for now */
static int plan_flags_of (const cholmod_factor *L, const cholmod_common *Common)
{
    int flags = Common->hip_flags ;
    /* the real twin of a complex factor (complex.c): the update kernels contract over the even
     * panel columns only -- the complex multiply-add as four real ones (zherk / zgemm,
     * t_cholmod_super_numeric.c:41-83) instead of the eight of the plain embedding */
    if (L->hip_is_twin == 2) flags |= CHOLMOD_HIP_CX_STORAGE ;      /* the complex factor in its own storage */
    else if (L->hip_is_twin)
    {
        const char *e = getenv ("CHOLMOD_HIP_TWIN_FULL_K") ;
        if (!(e && atoi (e) != 0)) flags |= CHOLMOD_HIP_PHI_TWIN ;
    }
    return flags ;
}

/* ... and what the host layer adds to them for the engine on its own account (not part of what L->hip_plan_ahead records of
 * the caller's Common->hip_flags).  Ordinary real factorizations on one GPU: the contribution-block half of the extend-add
 * rides with the update that first writes the block (cholmod_hip.h: CHOLMOD_HIP_FUSED_CB_EA); CHOLMOD_HIP_NO_FUSED_CB_EA=1
 * in the environment, read when the plan is built, keeps the two-phase extend-add everywhere */
static int engine_flags_of (const cholmod_factor *L, const cholmod_common *Common)
{
    const char *e = getenv ("CHOLMOD_HIP_NO_FUSED_CB_EA") ;
    if (L->hip_is_twin || Common->hip_world > 1 || (e && atoi (e) != 0)) return 0 ;
    return CHOLMOD_HIP_FUSED_CB_EA ;
}

static int ensure_plan_with (cholmod_factor *L, cholmod_common *Common, const int64_t *reach_p, const int32_t *reach_first) ;
int ssamd_ensure_plan (cholmod_factor *L, cholmod_common *Common) { return ensure_plan_with (L, Common, NULL, NULL) ; }

static int ensure_plan_with (cholmod_factor *L, cholmod_common *Common, const int64_t *reach_p, const int32_t *reach_first)
{
    if (!ssamd_factor_has_cholesky_sizes (L))
    { ERROR (CHOLMOD_INVALID, "L was analysed for SPQR (no Cholesky sizes)") ; return FALSE ; }
    int st = 0 ;
    int world = Common->hip_world > 1 ? Common->hip_world : 1 ;
    const int flags = plan_flags_of (L, Common) ;
    if (L->hip_plan && L->hip_plan_ahead && !L->hip_on_device && (L->hip_plan_ahead - 1 != flags || world > 1))
    {
        /* a plan built inside the analysis, and Common->hip_flags / hip_world have changed since: build it again */
        cholmod_hip_plan_destroy ((cholmod_hip_plan *) L->hip_plan) ;
        L->hip_plan = NULL ;
    }
    L->hip_plan_ahead = 0 ;
    if (L->hip_plan) return TRUE ;
    const double t_plan = omp_get_wtime () ;
    cholmod_hip_plan *P = (reach_p && world == 1)
        ? cholmod_hip_plan_create_reach ((int64_t) L->n, (int64_t) L->nsuper, L->super, L->pi, L->px, L->s,
            flags | engine_flags_of (L, Common), reach_p, reach_first, &st)
        : cholmod_hip_plan_create_dist ((int64_t) L->n, (int64_t) L->nsuper,
            L->super, L->pi, L->px, L->s, flags | engine_flags_of (L, Common), world > 1 ? Common->hip_rank : 0, world, &st) ;
    Common->hip_plan_seconds = omp_get_wtime () - t_plan ;
    if (!P) return map_hip_status (st ? st : CHOLMOD_HIP_GPU_PROBLEM, Common, "HIP plan creation failed") ;
    /* (several ranks need an exchange: the Common->hip_allreduce callback, or the
     * native RCCL path attached to L->hip_plan with cholmod_hip_rccl_attach after
     * cholmod_l_hip_prepare; without either the factorization returns CHOLMOD_INVALID) */
    if (Common->hip_allreduce)
        cholmod_hip_set_allreduce (P, Common->hip_allreduce, Common->hip_allreduce_user) ;
    L->hip_plan = P ;
    L->hip_perm_set = FALSE ;
    return TRUE ;
}

/* The plan at the end of cholmod_l_analyze (Common->hip_lazy_plan == 0; one GPU -- the ranks of a multi-GPU run attach their
 * exchange to the plan after cholmod_l_hip_prepare).  Not an error of the analysis when it cannot be built: L stays without
 * a plan, the first factorization tries again and reports. */
/* ---- where the relaxed fronts hold explicit zeros ------------------------------------------------------------------------
 * For every supernode s of at least REACH_MIN_COLS columns: reach_first [reach_p [s] + p] = the first column of s (counted
 * from its first column) whose pattern holds the row at position p of its row list, INT32_MAX if none does.  Column k of L
 * gets its pattern from A's column k, from the contribution blocks of the children whose first row past their own columns
 * is k, and from the earlier columns of its own supernode; so the rows the columns [0, H) of s reach are the rows of A's
 * pattern in those columns and the contribution-block rows of the children attached to them -- the prefix union is closed
 * under the third source.  The children's row lists are relaxed (a superset of their exact patterns), so the reach is
 * never smaller than the exact one.  U: the upper pattern of P A P' with the factor's own permutation (L->Perm).
 * Returns the length of reach_first (reach_first == NULL: only reach_p is filled), -1 on failure. */
#define REACH_MIN_COLS 512
int64_t ssamd_front_reach (const cholmod_sparse *U, const cholmod_factor *L, int64_t *reach_p, int32_t *reach_first)
{
    const Int nsuper = (Int) L->nsuper, n = (Int) L->n ;
    const Int *super = L->super, *pi = L->pi, *Ls = L->s ;
    if (!U || !L->is_super || (Int) U->ncol != n) return -1 ;
    reach_p [0] = 0 ;
    for (Int s = 0 ; s < nsuper ; s++)
    {
        const Int nscol = super [s + 1] - super [s], nsrow = pi [s + 1] - pi [s] ;
        reach_p [s + 1] = reach_p [s] + (nscol >= REACH_MIN_COLS ? nsrow : 0) ;
    }
    if (!reach_first || reach_p [nsuper] == 0) return reach_p [nsuper] ;
    Int *smap = malloc ((size_t) (n > 0 ? n : 1) * sizeof (Int)) ;
    if (!smap) return -1 ;
    for (Int s = 0 ; s < nsuper ; s++)
        for (Int k = super [s] ; k < super [s + 1] ; k++) smap [k] = s ;
    for (int64_t q = 0 ; q < reach_p [nsuper] ; q++) reach_first [q] = INT32_MAX ;
    for (Int s = 0 ; s < nsuper ; s++)
        if (reach_p [s + 1] > reach_p [s])
            for (Int p = 0 ; p < super [s + 1] - super [s] ; p++) reach_first [reach_p [s] + p] = (int32_t) p ;
    /* position of row i in the row list of s (sorted), or -1 */
    #define ROW_POS(s, i, pos) do { Int lo_ = pi [s], hi_ = pi [s + 1] ; \
        while (lo_ < hi_) { Int mid_ = (lo_ + hi_) >> 1 ; if (Ls [mid_] < (i)) lo_ = mid_ + 1 ; else hi_ = mid_ ; } \
        (pos) = (lo_ < pi [s + 1] && Ls [lo_] == (i)) ? lo_ - pi [s] : -1 ; } while (0)
    /* A: column i of U holds the rows k <= i, i.e. column k of the lower part holds row i */
    const Int *Up = U->p, *Ui = U->i, *Unz = U->nz ;
    for (Int i = 0 ; i < n ; i++)
    {
        const Int pend = U->packed ? Up [i + 1] : Up [i] + Unz [i] ;
        for (Int q = Up [i] ; q < pend ; q++)
        {
            const Int k = Ui [q], s = (k < i) ? smap [k] : -1 ;
            if (s < 0 || reach_p [s + 1] == reach_p [s]) continue ;
            Int pos ;
            ROW_POS (s, i, pos) ;
            int32_t *fp = reach_first + reach_p [s] + pos ;
            if (pos >= 0 && *fp > (int32_t) (k - super [s])) *fp = (int32_t) (k - super [s]) ;
        }
    }
    /* children: their contribution-block rows, from the column of the parent where the block begins */
    for (Int c = 0 ; c < nsuper ; c++)
    {
        const Int nscol = super [c + 1] - super [c], p0 = pi [c] + nscol ;
        if (p0 >= pi [c + 1]) continue ;
        const Int s = smap [Ls [p0]] ;
        if (reach_p [s + 1] == reach_p [s]) continue ;
        const int32_t f = (int32_t) (Ls [p0] - super [s]) ;
        Int pos = 0 ;
        for (Int q = p0 ; q < pi [c + 1] ; q++)
        {
            while (pi [s] + pos < pi [s + 1] && Ls [pi [s] + pos] < Ls [q]) pos++ ;     /* (both lists sorted) */
            if (pi [s] + pos < pi [s + 1] && Ls [pi [s] + pos] == Ls [q] && reach_first [reach_p [s] + pos] > f)
                reach_first [reach_p [s] + pos] = f ;
        }
    }
    #undef ROW_POS
    free (smap) ;
    return reach_p [nsuper] ;
}

void ssamd_front_reach_alloc (const cholmod_sparse *U, const cholmod_factor *L, int64_t **reach_p, int32_t **reach_first)
{
    *reach_p = malloc (((size_t) L->nsuper + 1) * sizeof (int64_t)) ;
    *reach_first = NULL ;
    int64_t len = *reach_p ? ssamd_front_reach (U, L, *reach_p, NULL) : -1 ;
    if (len > 0) *reach_first = malloc ((size_t) len * sizeof (int32_t)) ;
    if (len > 0 && *reach_first && ssamd_front_reach (U, L, *reach_p, *reach_first) == len) return ;
    free (*reach_p) ; free (*reach_first) ;
    *reach_p = NULL ; *reach_first = NULL ;
}

/* the same for a caller's A and an analysed L (tests, tools): A lower or upper stored, real or pattern */
int64_t cholmod_l_hip_front_reach (cholmod_sparse *A, cholmod_factor *L, int64_t *reach_p, int32_t *reach_first,
    cholmod_common *Common)
{
    if (!A || !L || !reach_p || !L->is_super || !L->Perm || A->stype == 0 || A->nrow != L->n) return -1 ;
    cholmod_sparse *U = NULL, *Lw = NULL ;
    if (A->stype < 0) U = cholmod_l_ptranspose (A, 0, L->Perm, NULL, 0, Common) ;
    else
    {
        Lw = cholmod_l_ptranspose (A, 0, L->Perm, NULL, 0, Common) ;
        if (Lw) U = cholmod_l_ptranspose (Lw, 0, NULL, NULL, 0, Common) ;
    }
    const int64_t len = U ? ssamd_front_reach (U, L, reach_p, reach_first) : -1 ;
    cholmod_l_free_sparse (&U, Common) ;
    cholmod_l_free_sparse (&Lw, Common) ;
    return len ;
}

void ssamd_plan_ahead (cholmod_factor *L, cholmod_common *Common, const int64_t *reach_p, const int32_t *reach_first)
{
    if (!L || !L->is_super || !L->useGPU || L->hip_plan || Common->useGPU != 1) return ;
    if (Common->hip_world > 1 || Common->hip_allreduce) return ;
    if (!ssamd_factor_has_cholesky_sizes (L) || !cholmod_hip_probe ()) return ;
    const int st = Common->status, tc = Common->try_catch ;
    Common->try_catch = TRUE ;
    if (ensure_plan_with (L, Common, reach_p, reach_first)) L->hip_plan_ahead = plan_flags_of (L, Common) + 1 ;
    Common->try_catch = tc ; Common->status = st ;
}

static void absorb_stats (cholmod_factor *L, cholmod_common *Common)
{
    double s [CHOLMOD_HIP_NSTATS] ;
    if (cholmod_hip_get_stats ((cholmod_hip_plan *) L->hip_plan, s) != CHOLMOD_HIP_OK) return ;
    /* keep the reference's counters meaningful (cholmod_core.h:1004-1024): the
     * engine's dense updates play the role of the dsyrk+dgemm calls */
    Common->gpuKernelTime = s [0] ;
    Common->gpuFlops = (SuiteSparse_long) s [1] ;
    Common->gpuNumKernelLaunches = (int) s [2] ;
    Common->cholmod_gpu_syrk_time = s [6] + s [14] + s [27] + s [32] ;
    Common->cholmod_gpu_syrk_calls = (size_t) (s [7] + s [26] + s [33]) ;
    Common->cholmod_gpu_gemm_time = 0 ; Common->cholmod_gpu_gemm_calls = 0 ;
    Common->cholmod_gpu_potrf_time = s [11] ;
    Common->cholmod_gpu_trsm_time = s [12] ;
    Common->cholmod_assemble_time = s [13] ;
    Common->cholmod_assemble_time2 = s [9] ;
    Common->cholmod_cpu_gemm_time = Common->cholmod_cpu_syrk_time = 0 ;
    Common->cholmod_cpu_trsm_time = Common->cholmod_cpu_potrf_time = 0 ;
    Common->cholmod_cpu_gemm_calls = Common->cholmod_cpu_syrk_calls = 0 ;
    Common->cholmod_cpu_trsm_calls = Common->cholmod_cpu_potrf_calls = 0 ;
}

/* ---- cholmod_l_super_numeric ------------------------------------------------------------ */

/* a factorization that cannot hand its result over leaves L symbolic, as the reference does when it runs out of memory on
 * a symbolic L (cholmod_super_numeric.c:235-248): the values on the device are forgotten, the plan stays */
static int back_to_symbolic (cholmod_factor *L)
{
    L->xtype = CHOLMOD_PATTERN ; L->minor = L->n ;
    L->hip_on_device = FALSE ; L->hip_host_valid = FALSE ;
    return FALSE ;
}

/* the device copy of L is void: a numeric L keeps the values it has on the host, if it has them (the reference leaves the old
 * values of a numeric L in place); otherwise L is symbolic again -- never a "numeric" L whose device factor is a zeroed,
 * partial or foreign one */
static void forget_device_factor (cholmod_factor *L)
{
    if (L->x && L->hip_host_valid) L->hip_on_device = FALSE ;
    else back_to_symbolic (L) ;
}

static int finish_numeric (int rc, int64_t minor, cholmod_factor *L, cholmod_common *Common)
{
    const int was_symbolic = (L->xtype == CHOLMOD_PATTERN && !L->x) ;
    if (rc < 0)
    {
        forget_device_factor (L) ;         /* (whatever L was on entry: run_factorize clears it first) */
        return map_hip_status (rc, Common, "HIP factorization failed") ;
    }
    L->xtype = CHOLMOD_REAL ;
    L->dtype = CHOLMOD_DOUBLE ;
    L->is_ll = TRUE ;
    L->minor = (size_t) minor ;
    L->hip_on_device = TRUE ;
    L->hip_host_valid = FALSE ;
    if (!Common->hip_factor_on_device)
    {
        if (Common->hip_world > 1)
        {
            int rg = cholmod_hip_gather_factor ((cholmod_hip_plan *) L->hip_plan) ;
            if (rg != CHOLMOD_HIP_OK) { if (was_symbolic) back_to_symbolic (L) ; return map_hip_status (rg, Common, "factor gather failed") ; }
        }
        if (!L->x) L->x = cholmod_l_malloc (L->xsize, sizeof (double), Common) ;
        if (!L->x) return was_symbolic ? back_to_symbolic (L) : FALSE ;     /* (found by the fault loop, tests/test_memory_faults.py) */
        int r2 = cholmod_hip_download_factor ((cholmod_hip_plan *) L->hip_plan, L->x) ;
        if (r2 != CHOLMOD_HIP_OK)
        {
            if (was_symbolic) { L->x = cholmod_l_free (L->xsize, sizeof (double), L->x, Common) ; back_to_symbolic (L) ; }
            return map_hip_status (r2, Common, "factor download failed") ;
        }
        L->hip_host_valid = TRUE ;
    }
    absorb_stats (L, Common) ;
    if (rc == CHOLMOD_HIP_NOT_POSDEF)
        ERROR (CHOLMOD_NOT_POSDEF, "matrix not positive definite") ;
    return TRUE ;     /* TRUE also when not positive definite, as the reference */
}

/* reference: Supernodal/cholmod_super_numeric.c:97-308.  A must be the
 * permuted matrix in symmetric-lower form (stype < 0). */
int cholmod_l_super_numeric (cholmod_sparse *A, cholmod_sparse *F, double beta [2],
    cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (A, FALSE) ;
    if (A->xtype < CHOLMOD_REAL || A->xtype > CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_INVALID, "A must be numeric") ; return FALSE ; }
    if (A->stype == 0)
    {
        /* L L' = A*F + beta*I with F = A(:,f)' (t_cholmod_super_numeric.c:223-237, :385-418: the reference assembles every
         * column of A*F on the fly): tril (A*F) is formed on the host (core.c: ssamd_aat) and factorized as the symmetric
         * matrix it is */
        if (!F) { ERROR (CHOLMOD_INVALID, "F is required for the unsymmetric case") ; return FALSE ; }
        if (F->xtype != A->xtype) { ERROR (CHOLMOD_INVALID, "A and F must have the same xtype") ; return FALSE ; }
        if (A->nrow != L->n) { ERROR (CHOLMOD_INVALID, "invalid dimensions") ; return FALSE ; }
        cholmod_sparse *C = ssamd_aat (A, F, 1, TRUE, Common) ;
        if (!C) return FALSE ;
        int okc = cholmod_l_super_numeric (C, NULL, beta, L, Common) ;
        cholmod_l_free_sparse (&C, Common) ;
        return okc ;
    }
    /* a numeric L keeps its kind: real for real A, complex for complex or zomplex A
     * (reference cholmod_super_numeric.c:160-175) */
    const int want = (A->xtype == CHOLMOD_REAL) ? CHOLMOD_REAL : CHOLMOD_COMPLEX ;
    if (L->xtype != CHOLMOD_PATTERN && L->xtype != want)
    { ERROR (CHOLMOD_INVALID, "complex type mismatch") ; return FALSE ; }
    if (A->stype > 0) { ERROR (CHOLMOD_INVALID, "symmetric upper case not supported") ; return FALSE ; }
    if (A->nrow != A->ncol || A->nrow != L->n) { ERROR (CHOLMOD_INVALID, "invalid dimensions") ; return FALSE ; }
    if (!L->is_super) { ERROR (CHOLMOD_INVALID, "L not supernodal") ; return FALSE ; }
    if (!ssamd_factor_has_cholesky_sizes (L))
    { ERROR (CHOLMOD_INVALID, "L was analysed for SPQR (no Cholesky sizes): it cannot be factorized") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    double b = beta ? beta [0] : 0.0 ;
    /* complex / zomplex A: the real factorization of the embedded matrix (complex.c) */
    if (want == CHOLMOD_COMPLEX) return ssamd_complex_super_numeric (A, b, L, Common) ;
    /* GPU or CPU (reference t_cholmod_super_numeric.c:183-192: the GPU is used only
     * if Common->useGPU == 1 and the analysis found one, L->useGPU; a device that
     * cannot be initialised degrades to the CPU path).  A factor that already lives
     * on the engine stays there. */
    int want_gpu = (ssamd_resolve_use_gpu (Common) == 1) ;
    if (want_gpu && !(L->useGPU || L->hip_plan) && Common->hip_cpu_fallback) want_gpu = FALSE ;
    if (want_gpu)
    {
        int was_ok = Common->status ;
        void (*eh) (int, const char *, int, const char *) = Common->error_handler ;
        Common->error_handler = NULL ;                  /* a failed device probe is not an error yet */
        int have = ssamd_ensure_plan (L, Common) ;
        Common->error_handler = eh ;
        if (have)
        {
            int64_t minor = (int64_t) L->n ;
            int rc = cholmod_hip_factorize ((cholmod_hip_plan *) L->hip_plan, A->p, A->i,
                A->packed ? NULL : A->nz, A->x, b, Common->quick_return_if_not_posdef, NULL, &minor) ;
            return finish_numeric (rc, minor, L, Common) ;
        }
        /* no device / no HBM for this factor: loud by default; degrade to the CPU path
         * only if the caller asked for the reference's behaviour (several ranks
         * cannot degrade on their own) */
        if (!Common->hip_cpu_fallback || Common->hip_world > 1 || Common->status == CHOLMOD_INVALID
            || Common->status == CHOLMOD_TOO_LARGE)
        {
            int st = Common->status ;
            Common->status = was_ok ;
            ERROR (st, "HIP plan creation failed") ;
            return FALSE ;
        }
        Common->status = CHOLMOD_OK ;
        L->useGPU = 0 ;
    }
    /* ---- CPU path */
    if (L->hip_is_twin == 2) { ERROR (CHOLMOD_GPU_PROBLEM, "a complex factor in engine storage has no CPU form") ; return FALSE ; }
    int was_symbolic = (L->x == NULL) ;
    if (!L->x) L->x = cholmod_l_malloc (L->xsize, sizeof (double), Common) ;
    if (!L->x) return FALSE ;           /* out of memory: L is returned symbolic (cholmod_super_numeric.c:235-248) */
    (void) was_symbolic ;
    L->xtype = CHOLMOD_REAL ; L->dtype = CHOLMOD_DOUBLE ; L->is_ll = TRUE ;
    if (!ssamd_cpu_super_numeric (A, b, L, Common))
    {
        if (was_symbolic) { cholmod_l_free (L->xsize, sizeof (double), L->x, Common) ; L->x = NULL ; L->xtype = CHOLMOD_PATTERN ; }
        return FALSE ;
    }
    L->hip_on_device = FALSE ;
    L->hip_host_valid = TRUE ;
    Common->gpuKernelTime = 0 ; Common->gpuFlops = 0 ; Common->gpuNumKernelLaunches = 0 ;
    return TRUE ;
}

int cholmod_l_refactorize_resident (double beta [2], cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (L->cx_twin)
    {
        cholmod_factor *T = L->cx_twin ;
        const int keep = Common->hip_factor_on_device ;
        Common->hip_factor_on_device = TRUE ;       /* the complex L->x is gathered on the device */
        int ok = cholmod_l_refactorize_resident (beta, T, Common) ;
        Common->hip_factor_on_device = keep ;
        if (!ok) return FALSE ;
        int status = Common->status ;
        L->minor = (T->minor >= T->n) ? L->n : T->minor / 2 ;
        L->hip_on_device = T->hip_on_device ; L->hip_host_valid = FALSE ;
        if (!keep && !ssamd_complex_sync_host (L, Common)) return FALSE ;
        Common->status = status ;
        return TRUE ;
    }
    if (!L->hip_plan) { ERROR (CHOLMOD_INVALID, "no resident matrix") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    int64_t minor = (int64_t) L->n ;
    int rc = cholmod_hip_factorize_resident ((cholmod_hip_plan *) L->hip_plan, beta ? beta [0] : 0.0,
        Common->quick_return_if_not_posdef, &minor) ;
    return finish_numeric (rc, minor, L, Common) ;
}

/* ---- cholmod_l_factorize ---------------------------------------------------------------- */

static double api_now (void)
{
    struct timespec ts ;
    clock_gettime (CLOCK_MONOTONIC, &ts) ;
    return (double) ts.tv_sec + 1e-9 * (double) ts.tv_nsec ;
}

/* Two independent 64-bit fingerprints of the pattern (p and i arrays): the values-only fast
 * path of cholmod_l_factorize trusts them as proof that the resident S and its value map still
 * fit A.  Each is a sum of position-keyed, avalanche-mixed words (order-independent, hence
 * parallel and deterministic); the two use different keys, different mixers (the splitmix64
 * and murmur3 finalisers) and are folded differently, so a pattern change must defeat 128
 * bits, not 64 (round-2 review: one 64-bit sum folded by addition was thin). */
/* Threads for the two short host loops of every cholmod_l_factorize call (staging copy of A->x, pattern hash: a few hundred
 * microseconds each).  Measured on the 2 x 64-core box (2D 1259^2, wall around the call, resident step 5.26 ms): a team of 32
 * 7.4 / 8.5 / 10.6 ms in three runs, 16 threads 6.14 / 6.15 / 6.26 ms, 8 threads 6.83 ms -- waking a wide team costs more
 * than its bandwidth returns.  CHOLMOD_API_THREADS overrides. */
static int api_threads (void)
{
    const char *e = getenv ("CHOLMOD_API_THREADS") ;
    if (e && atoi (e) > 0) return atoi (e) ;
    const int nt = ssamd_host_threads () ;
    return nt > 16 ? 16 : nt ;
}

typedef struct { uint64_t hp, gp, hi, gi ; } pat_sums ;

/* the pattern is hashed in pieces of HASH_PIECE entries: the ncol + 1 column pointers first, then the row indices */
#define HASH_PIECE ((int64_t) 1 << 16)

static int64_t hash_pieces (const cholmod_sparse *A)
{
    const int64_t ncol = (int64_t) A->ncol, nz = ((Int *) A->p) [ncol] ;
    return (ncol + HASH_PIECE) / HASH_PIECE + (nz + HASH_PIECE - 1) / HASH_PIECE ;
}

/* piece k into the four sums (order-independent: any thread may take any piece) */
static void hash_piece (const cholmod_sparse *A, int64_t k, pat_sums *S)
{
    const Int *Ap = A->p, *Ai = A->i ;
    const int64_t ncol = (int64_t) A->ncol, nz = Ap [ncol], nhp = (ncol + HASH_PIECE) / HASH_PIECE ;
    uint64_t h = 0, g = 0 ;
    if (k < nhp)
    {
        const int64_t j1 = ((k + 1) * HASH_PIECE < ncol + 1) ? (k + 1) * HASH_PIECE : ncol + 1 ;
        for (int64_t j = k * HASH_PIECE ; j < j1 ; j++)
        {
            uint64_t x = (uint64_t) Ap [j] + 0x9E3779B97F4A7C15ull * (uint64_t) (j + 1) ;
            x ^= x >> 30 ; x *= 0xbf58476d1ce4e5b9ull ; x ^= x >> 27 ; x *= 0x94d049bb133111ebull ; x ^= x >> 31 ;
            h += x ;
            uint64_t y = ((uint64_t) Ap [j] ^ 0xA24BAED4963EE407ull) * (2 * (uint64_t) j + 0x632BE59BD9B4E019ull) ;
            y ^= y >> 33 ; y *= 0xff51afd7ed558ccdull ; y ^= y >> 33 ; y *= 0xc4ceb9fe1a85ec53ull ; y ^= y >> 33 ;
            g += y ;
        }
        S->hp += h ; S->gp += g ;
    }
    else
    {
        const int64_t p0 = (k - nhp) * HASH_PIECE, p1 = (p0 + HASH_PIECE < nz) ? p0 + HASH_PIECE : nz ;
        for (int64_t p = p0 ; p < p1 ; p++)
        {
            uint64_t x = (uint64_t) Ai [p] + 0xD1B54A32D192ED03ull * (uint64_t) (p + 1) ;
            x ^= x >> 30 ; x *= 0xbf58476d1ce4e5b9ull ; x ^= x >> 27 ; x *= 0x94d049bb133111ebull ; x ^= x >> 31 ;
            h += x ;
            uint64_t y = ((uint64_t) Ai [p] ^ 0x8EBC6AF09C88C6E3ull) * (2 * (uint64_t) p + 0x589965CC75374CC3ull) ;
            y ^= y >> 33 ; y *= 0xff51afd7ed558ccdull ; y ^= y >> 33 ; y *= 0xc4ceb9fe1a85ec53ull ; y ^= y >> 33 ;
            g += y ;
        }
        S->hi += h ; S->gi += g ;
    }
}

static uint64_t pattern_hash_fold (cholmod_sparse *A, const pat_sums *S, uint64_t *second)
{
    const Int ncol = (Int) A->ncol, nz = ((Int *) A->p) [ncol] ;
    uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t) A->nrow * 0xff51afd7ed558ccdull) ^ ((uint64_t) (A->stype + 2) << 56) ;
    uint64_t g = S->gp ^ ((S->gi << 23) | (S->gi >> 41)) ^ ((uint64_t) nz * 0x9FB21C651E98DF25ull) ;
    g ^= g >> 32 ; g *= 0xd6e8feb86659fd93ull ; g ^= g >> 32 ;
    *second = g ^ ((uint64_t) ncol << 17) ;
    return h ^ S->hp ^ (S->hi * 0x2545F4914F6CDD1Dull) ;
}

static uint64_t pattern_hash (cholmod_sparse *A, uint64_t *second)
{
    const int64_t npiece = hash_pieces (A) ;
    uint64_t hp = 0, gp = 0, hi = 0, gi = 0 ;
#pragma omp parallel for schedule(static) num_threads(api_threads ()) reduction(+:hp,gp,hi,gi)
    for (int64_t k = 0 ; k < npiece ; k++)
    {
        pat_sums T = {0, 0, 0, 0} ;
        hash_piece (A, k, &T) ;
        hp += T.hp ; gp += T.gp ; hi += T.hi ; gi += T.gi ;
    }
    const pat_sums S = {hp, gp, hi, gi} ;
    return pattern_hash_fold (A, &S, second) ;
}

/* The values-only path of cholmod_l_factorize: A has the nnz of the matrix whose S the engine holds, and only A->x travels
 * -- staged into the plan's pinned buffer in the order the engine asks for (cholmod_hip_values_begin: by the launch that
 * needs it, or S's own), every chunk by DMA as soon as it is full -- while the factorization is already enqueued, its
 * clearing of L first.  The proof that the resident S and its value map fit A, the pattern hash, is taken meanwhile and
 * checked after the fact.  Roles come from the team the runtime actually gives (a thread limit, a call from inside a
 * parallel region: it may be smaller than asked for), so that nobody waits for work only a missing thread would do:
 *     team >= 3: thread 0 factorizes, thread 1 pushes, the others stage; all but thread 0 then hash;
 *     team 2:    thread 0 stages, pushes, then factorizes; thread 1 hashes;
 *     team 1:    thread 0 does all four in that order.
 * Returns what cholmod_l_factorize returns, or -1: take the long way -- hash [0 .. 1] then holds A's pattern hash and L
 * no longer claims a factor on the device. */
uint64_t ssamd_pattern_hash (cholmod_sparse *A, uint64_t *second) { return pattern_hash (A, second) ; }

static int factorize_values_only (cholmod_sparse *A, double beta, cholmod_factor *L, cholmod_common *Common, uint64_t hash [2])
{
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    const int64_t annz = ((Int *) A->p) [A->ncol] ;
    const int timing = getenv ("CHOLMOD_API_TIMING") != NULL ;
    const double t0 = timing ? api_now () : 0 ;
    double t1 = t0 ;
    /* (one counter per chunk, allocated before anything is enqueued: a chunk holds at least one staging piece) */
    const size_t maxchunk = (size_t) (annz / 16384 + 1) ;
    int64_t *chunk_done = cholmod_l_calloc (maxchunk, sizeof (int64_t), Common) ;
    if (!chunk_done) return FALSE ;
    double *stage = NULL ;
    const int64_t *index = NULL ;
    int64_t count = 0, CH = 0 ;
    if (cholmod_hip_values_begin (plan, &stage, &index, &count, &CH) != CHOLMOD_HIP_OK)
    {
        cholmod_l_free (maxchunk, sizeof (int64_t), chunk_done, Common) ;
        forget_device_factor (L) ;          /* (the clearing of L may have been enqueued) */
        hash [0] = pattern_hash (A, &hash [1]) ;
        return -1 ;
    }
    /* staging pieces: 128 KB gathered in batch order, 256 KB copied in S order; a chunk is a whole number of pieces */
    const int64_t PIECE = index ? 16384 : 32768 ;
    const int fits = (count <= annz && CH >= PIECE && CH % PIECE == 0) ;     /* (the header's promise; else: cancel) */
    const int64_t nchunk = fits ? (count + CH - 1) / CH : 0, npiece = fits ? (count + PIECE - 1) / PIECE : 0 ;
    const int64_t nhash = hash_pieces (A) ;
    const double *Ax = A->x ;
    int64_t next_piece = 0, next_hash = 0, minor = (int64_t) L->n ;
    pat_sums tot = {0, 0, 0, 0} ;
    int rcf = CHOLMOD_HIP_OK ;
#pragma omp parallel num_threads(api_threads ())
    {
        const int me = omp_get_thread_num (), team = omp_get_num_threads () ;
        const int stager = (team >= 3) ? (me >= 2) : (me == 0), pusher = (team >= 3) ? (me == 1) : (me == 0) ;
        const int hasher = (team >= 3) ? (me >= 1) : (me == team - 1) ;
        if (stager)
            for (int64_t k ; (k = __atomic_fetch_add (&next_piece, 1, __ATOMIC_RELAXED)) < npiece ; )
            {
                const int64_t q0 = k * PIECE, q1 = (q0 + PIECE < count) ? q0 + PIECE : count ;
                if (!index) memcpy (stage + q0, Ax + q0, (size_t) (q1 - q0) * sizeof (double)) ;
                else for (int64_t q = q0 ; q < q1 ; q++)
                {
                    /* (the index rises inside a batch: mostly the next cache lines, the prefetch covers the gaps) */
                    if (q + 24 < q1) __builtin_prefetch (Ax + index [q + 24], 0, 0) ;
                    stage [q] = Ax [index [q]] ;
                }
                __atomic_fetch_add (&chunk_done [q0 / CH], 1, __ATOMIC_RELEASE) ;
            }
        if (pusher)
        {
            if (!fits) (void) cholmod_hip_values_push_chunk (plan, -1) ;
            for (int64_t c = 0 ; c < nchunk ; c++)
            {
                const int64_t o = c * CH, need = (((count - o < CH) ? count - o : CH) + PIECE - 1) / PIECE ;
                while (__atomic_load_n (&chunk_done [c], __ATOMIC_ACQUIRE) < need) { /* (microseconds) */ }
                if (cholmod_hip_values_push_chunk (plan, c) != CHOLMOD_HIP_OK) break ;      /* (the engine has cancelled) */
            }
            if (timing) t1 = api_now () ;
        }
        if (me == 0) rcf = cholmod_hip_factorize_resident (plan, beta, Common->quick_return_if_not_posdef, &minor) ;
        if (hasher)
        {
            pat_sums mine = {0, 0, 0, 0} ;
            for (int64_t k ; (k = __atomic_fetch_add (&next_hash, 1, __ATOMIC_RELAXED)) < nhash ; ) hash_piece (A, k, &mine) ;
#pragma omp critical (ssamd_pattern_hash)
            { tot.hp += mine.hp ; tot.gp += mine.gp ; tot.hi += mine.hi ; tot.gi += mine.gi ; }
        }
    }
    cholmod_l_free (maxchunk, sizeof (int64_t), chunk_done, Common) ;
    hash [0] = pattern_hash_fold (A, &tot, &hash [1]) ;
    if (L->hip_apat_hash == hash [0] && L->hip_apat_hash2 == hash [1])
    {
        if (timing) fprintf (stderr, "cholmod_l_factorize (values only, in %s order): last push at %.3f ms, factorization + hash done at %.3f ms\n",
            index ? "batch" : "S", 1e3 * (t1 - t0), 1e3 * (api_now () - t0)) ;
        return finish_numeric (rcf, minor, L, Common) ;
    }
    forget_device_factor (L) ;              /* (another pattern after all: what the device computed is void) */
    return -1 ;
}

/* reference: Cholesky/cholmod_factorize.c:97-300, supernodal symmetric branch
 * (:177-288): S = tril(P A P') by one permuted transpose when A is stored
 * upper (:225-232) or two when it is stored lower (:233-244). */
int cholmod_l_factorize_p (cholmod_sparse *A, double beta [2], SuiteSparse_long *fset, size_t fsize,
    cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (A, FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (A->xtype < CHOLMOD_REAL || A->xtype > CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_INVALID, "A must be numeric") ; return FALSE ; }
    if (A->nrow != L->n) { ERROR (CHOLMOD_INVALID, "A and L dimensions do not match") ; return FALSE ; }
    if (!L->is_super) { ERROR (CHOLMOD_NOT_INSTALLED, "simplicial factorization not built") ; return FALSE ; }
    if (A->stype == 0)
    {
        /* factorize A*A' + beta*I (cholmod_factorize.c:197-224: S = A(p,f), F = S', super_numeric (S, F, beta)): tril (A*A')
         * is formed on the host and takes the symmetric branch below -- permutation, upload and, from the second call with
         * the same pattern on, the values-only path included.  A column subset f: A(:,f)*A(:,f)', the columns cut out first. */
        cholmod_sparse *Af = fset ? ssamd_column_subset (A, fset, fsize, 1, Common) : NULL ;
        if (fset && !Af) return FALSE ;
        cholmod_sparse *C = ssamd_aat (Af ? Af : A, NULL, 1, TRUE, Common) ;
        if (Af) cholmod_l_free_sparse (&Af, Common) ;
        if (!C) return FALSE ;
        int okc = cholmod_l_factorize_p (C, beta, NULL, 0, L, Common) ;
        cholmod_l_free_sparse (&C, Common) ;
        return okc ;
    }
    if (A->nrow != A->ncol) { ERROR (CHOLMOD_INVALID, "A and L dimensions do not match") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    double zero [2] = {0, 0} ;
    /* Same pattern as the matrix the engine already holds (hash of p / i, nnz): only the
     * values travel -- H2D of A->x and a gather into the resident S on the device; the
     * host-side permutation, the pattern upload and the assembly search are skipped. */
    const int vmap_ok = (A->xtype == CHOLMOD_REAL && A->packed && L->hip_plan && Common->hip_world <= 1
        && ssamd_resolve_use_gpu (Common) == 1) ;
    uint64_t hash [2] = {0, 0} ;
    int hashed = FALSE ;
    size_t annz = vmap_ok ? (size_t) ((Int *) A->p) [A->ncol] : 0 ;
    if (vmap_ok && L->hip_apat_valid && L->hip_apat_nnz == annz && (L->xtype == CHOLMOD_REAL || L->xtype == CHOLMOD_PATTERN))
    {
        const int ok = factorize_values_only (A, beta ? beta [0] : 0.0, L, Common, hash) ;
        if (ok >= 0) return ok ;
        hashed = TRUE ;
        L->hip_apat_valid = FALSE ;         /* no usable map after all: the long way */
    }
    const int ltiming = getenv ("CHOLMOD_API_TIMING") != NULL ;
    double tl0 = ltiming ? api_now () : 0, tl1 = 0, tl2 = 0, tl3 = 0 ;
    if (vmap_ok && !hashed) hash [0] = pattern_hash (A, &hash [1]) ;
    cholmod_sparse *S = NULL ;
    Int *src = NULL ;
    int natural = (L->ordering == CHOLMOD_NATURAL) ;
    Int *Perm = natural ? NULL : (Int *) L->Perm ;
    if (natural && A->packed && A->stype < 0)
    {
        S = A ;
    }
    else
    {
        /* S = tril (P A P'): upper-stored A by the conjugate permuted transpose of the
         * reference (:225-232); lower-stored A: the reference transposes twice (:233-244),
         * here one symmetric permutation lands in the lower triangle directly */
        S = ssamd_sym_permute_src (A, 2, Perm, FALSE, vmap_ok || (A->xtype == CHOLMOD_REAL && A->packed) ? &src : NULL, Common) ;
    }
    if (!S) return FALSE ;
    L->hip_apat_valid = FALSE ;
    L->hip_aat_valid = FALSE ;              /* (the engine drops a product map with the value map it belongs to) */
    if (ltiming) tl1 = api_now () ;
    int ok = cholmod_l_super_numeric (S, NULL, beta ? beta : zero, L, Common) ;
    if (ltiming) tl2 = api_now () ;
    /* the engine now holds S: tell it where S's values come from in A */
    if (ok && L->hip_plan && L->hip_on_device && A->xtype == CHOLMOD_REAL && A->packed && Common->hip_world <= 1
        && (S == A || src))
    {
        size_t snz = (size_t) ((Int *) S->p) [S->ncol] ;
        size_t an = (size_t) ((Int *) A->p) [A->ncol] ;
        Int *id = NULL ;
        if (S == A)
        {
            id = cholmod_l_malloc (snz > 0 ? snz : 1, sizeof (Int), Common) ;
            if (id) for (size_t q = 0 ; q < snz ; q++) id [q] = (Int) q ;
        }
        if ((S == A ? id : src) && cholmod_hip_set_value_map ((cholmod_hip_plan *) L->hip_plan,
                S == A ? id : src, (int64_t) snz, (int64_t) an) == CHOLMOD_HIP_OK)
        {
            if (!vmap_ok) hash [0] = pattern_hash (A, &hash [1]) ;
            L->hip_apat_hash = hash [0] ; L->hip_apat_hash2 = hash [1] ;
            L->hip_apat_nnz = an ;
            L->hip_apat_valid = TRUE ;
        }
        if (id) cholmod_l_free (snz > 0 ? snz : 1, sizeof (Int), id, Common) ;
    }
    if (src) cholmod_l_free (((Int *) S->p) [S->ncol] > 0 ? ((Int *) S->p) [S->ncol] : 1, sizeof (Int), src, Common) ;
    if (S != A) cholmod_l_free_sparse (&S, Common) ;
    if (ltiming)
    {
        tl3 = api_now () ;
        fprintf (stderr, "cholmod_l_factorize (long way): hash + permutation %.3f s, plan + upload + factorization %.3f s, value map %.3f s\n",
            tl1 - tl0, tl2 - tl1, tl3 - tl2) ;
    }
    return ok ;
}

/* The product map of the resident tril (A*A') of L's plan (cholmod_hip_set_product_map), for the unsymmetric A whose pattern
 * hashes to `hash` and has annz entries: built by the first call for that pattern -- cholmod_l_hip_factorize_values_device or
 * a gradient through it (grad.c) --, a comparison of three numbers after that.  TRUE: the map is set for A
 * (L->hip_aat_valid); FALSE with Common->status set: A*A' does not have the pattern L was last factorized from, or the map
 * could not be built. */
int ssamd_aat_product_map_ready (cholmod_sparse *A, cholmod_factor *L, size_t annz, const uint64_t hash [2], cholmod_common *Common)
{
    if (L->hip_aat_valid && L->hip_aat_nnz == annz && L->hip_aat_hash == hash [0] && L->hip_aat_hash2 == hash [1]) return TRUE ;
    /* the resident matrix is tril (A*A'): its pattern from A's, against the record; then the lists of products */
    cholmod_sparse *Cm = ssamd_aat (A, NULL, 0, TRUE, Common) ;
    if (!Cm) return FALSE ;
    uint64_t chash [2] ;
    chash [0] = pattern_hash (Cm, &chash [1]) ;
    const size_t cnz = (size_t) ((Int *) Cm->p) [Cm->ncol] ;
    cholmod_l_free_sparse (&Cm, Common) ;
    if (L->hip_apat_nnz != cnz || L->hip_apat_hash != chash [0] || L->hip_apat_hash2 != chash [1])
    { ERROR (CHOLMOD_INVALID, "A*A' does not have the pattern L was last factorized from") ; return FALSE ; }
    const int64_t npairs = cholmod_l_hip_aat_product_map (A, NULL, NULL, NULL, Common) ;
    if (npairs < 0) return FALSE ;
    if (npairs > INT32_MAX) { ERROR (CHOLMOD_TOO_LARGE, "too many products for the product map") ; return FALSE ; }
    const size_t np1 = npairs > 0 ? (size_t) npairs : 1 ;
    int64_t *cp = cholmod_l_malloc (cnz + 1, sizeof (int64_t), Common) ;
    int64_t *ia = cholmod_l_malloc (np1, sizeof (int64_t), Common) ;
    int64_t *ib = cholmod_l_malloc (np1, sizeof (int64_t), Common) ;
    int rm = CHOLMOD_HIP_OUT_OF_MEMORY ;
    if (cp && ia && ib && cholmod_l_hip_aat_product_map (A, cp, ia, ib, Common) == npairs)
        rm = cholmod_hip_set_product_map ((cholmod_hip_plan *) L->hip_plan, cp, ia, ib, (int64_t) cnz, (int64_t) annz) ;
    if (cp) cholmod_l_free (cnz + 1, sizeof (int64_t), cp, Common) ;
    if (ia) cholmod_l_free (np1, sizeof (int64_t), ia, Common) ;
    if (ib) cholmod_l_free (np1, sizeof (int64_t), ib, Common) ;
    L->hip_aat_valid = FALSE ;
    if (rm != CHOLMOD_HIP_OK)
    {
        if (Common->status < CHOLMOD_OK) return FALSE ;       /* (out of host memory: reported already) */
        return map_hip_status (rm, Common, "the product map could not be stored on the device") ;
    }
    L->hip_aat_hash = hash [0] ; L->hip_aat_hash2 = hash [1] ; L->hip_aat_nnz = annz ;
    L->hip_aat_valid = TRUE ;
    return TRUE ;
}

/* cholmod_l_factorize for values of A that live in device memory (cholmod.h).  The proof that the resident matrix and its
 * value map fit A is the pattern hash, taken BEFORE anything is enqueued here (the host path overlaps it with the upload;
 * there is no upload to hide it behind): a mismatch touches no device state. */
int cholmod_l_hip_factorize_values_device (cholmod_sparse *A, const double *Ax_dev, double beta [2],
    cholmod_factor *L, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (A, FALSE) ;
    RETURN_IF_NULL (Ax_dev, FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (A->p, FALSE) ;
    if (A->xtype == CHOLMOD_COMPLEX || A->xtype == CHOLMOD_ZOMPLEX || L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX)
    { ERROR (CHOLMOD_NOT_INSTALLED, "a factorization from device values of a complex matrix or factor is not supported") ; return FALSE ; }
    if (A->xtype != CHOLMOD_REAL && A->xtype != CHOLMOD_PATTERN) { ERROR (CHOLMOD_INVALID, "invalid xtype") ; return FALSE ; }
    if (!A->packed) { ERROR (CHOLMOD_INVALID, "A must be packed") ; return FALSE ; }
    if (A->nrow != L->n || (A->stype != 0 && A->nrow != A->ncol)) { ERROR (CHOLMOD_INVALID, "A and L dimensions do not match") ; return FALSE ; }
    if (L->xtype != CHOLMOD_REAL || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a numeric supernodal factor (factorize from the host first)") ; return FALSE ; }
    /* device pointers cannot be read on the host: no fallback, whatever Common->hip_cpu_fallback says */
    if (ssamd_resolve_use_gpu (Common) != 1) { ERROR (CHOLMOD_INVALID, "a factorization from device values needs Common->useGPU") ; return FALSE ; }
    if (Common->hip_world > 1) { ERROR (CHOLMOD_INVALID, "the factorization from device values runs on one rank only") ; return FALSE ; }
    if (!L->hip_plan || !L->hip_apat_valid)
    { ERROR (CHOLMOD_INVALID, "L holds no pattern record: cholmod_l_factorize from a host matrix of this pattern first") ; return FALSE ; }
    const size_t annz = (size_t) ((Int *) A->p) [A->ncol] ;
    if (annz > 0 && !A->i) { ERROR (CHOLMOD_INVALID, "argument missing") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    uint64_t hash [2] ;
    hash [0] = pattern_hash (A, &hash [1]) ;
    if (A->stype != 0)
    {
        if (L->hip_apat_nnz != annz || L->hip_apat_hash != hash [0] || L->hip_apat_hash2 != hash [1])
        { ERROR (CHOLMOD_INVALID, "A does not have the pattern L was last factorized from") ; return FALSE ; }
    }
    else if (!ssamd_aat_product_map_ready (A, L, annz, hash, Common)) return FALSE ;
    int64_t minor = (int64_t) L->n ;
    const int rc = cholmod_hip_factorize_values_device (plan, Ax_dev, (int64_t) annz, beta ? beta [0] : 0.0,
        Common->quick_return_if_not_posdef, stream, &minor) ;
    /* (the engine refuses before it touches the device: L keeps its factor) */
    if (rc == CHOLMOD_HIP_INVALID) { ERROR (CHOLMOD_INVALID, "the plan holds no value map for this matrix") ; return FALSE ; }
    return finish_numeric (rc, minor, L, Common) ;
}

int cholmod_l_factorize (cholmod_sparse *A, cholmod_factor *L, cholmod_common *Common)
{
    double zero [2] = {0, 0} ;
    return cholmod_l_factorize_p (A, zero, NULL, 0, L, Common) ;
}

int cholmod_l_factor_to_host (cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (L->hip_host_valid) return TRUE ;
    if (L->cx_twin) return ssamd_complex_sync_host (L, Common) ;
    if (!L->hip_plan || !L->hip_on_device) { ERROR (CHOLMOD_INVALID, "no numeric factor") ; return FALSE ; }
    if (!L->x) L->x = cholmod_l_malloc (L->xsize, sizeof (double), Common) ;
    if (!L->x) return FALSE ;
    int rc = cholmod_hip_download_factor ((cholmod_hip_plan *) L->hip_plan, L->x) ;
    if (rc != CHOLMOD_HIP_OK) return map_hip_status (rc, Common, "factor download failed") ;
    L->hip_host_valid = TRUE ;
    return TRUE ;
}

/* ---- cholmod_l_rcond -------------------------------------------------------------------------- */

/* reference: Cholesky/cholmod_rcond.c:64-161.  (min L_jj / max L_jj)^2 over the diagonal of the supernodal LL' factor:
 * -1 on error, 1 for a 0-by-0 matrix, 0 if the factorization failed (L->minor < n) or a diagonal entry is NaN.  A factor
 * that lives in HBM is not downloaded for this: one pass over its n diagonal entries on the device
 * (cholmod_hip_diag_minmax) returns the two extremes. */
double cholmod_l_rcond (cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (EMPTY) ;
    RETURN_IF_NULL (L, EMPTY) ;
    if (L->xtype < CHOLMOD_REAL || L->xtype > CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_INVALID, "invalid xtype") ; return EMPTY ; }
    Common->status = CHOLMOD_OK ;
    if (L->n == 0) return 1 ;
    if (L->minor < L->n) return 0 ;
    if (!L->is_super) { ERROR (CHOLMOD_NOT_INSTALLED, "simplicial factors not built") ; return EMPTY ; }
    double lmin, lmax ;
    cholmod_factor *D = L->cx_twin ? (cholmod_factor *) L->cx_twin : L ;      /* (complex L: the engine's factor) */
    if (D->hip_plan && D->hip_on_device && !L->hip_host_valid)
    {
        if (Common->hip_world > 1)
        {
            int rg = cholmod_hip_gather_factor ((cholmod_hip_plan *) D->hip_plan) ;
            if (rg != CHOLMOD_HIP_OK) { map_hip_status (rg, Common, "factor gather failed") ; return EMPTY ; }
        }
        double out [3] ;
        int rc = cholmod_hip_diag_minmax ((cholmod_hip_plan *) D->hip_plan, out) ;
        if (rc != CHOLMOD_HIP_OK) { map_hip_status (rc, Common, "diagonal scan failed") ; return EMPTY ; }
        if (out [2] > 0) return 0 ;             /* a NaN on the diagonal (:31-41) */
        lmin = out [0] ; lmax = out [1] ;
    }
    else
    {
        if (!L->x) { ERROR (CHOLMOD_INVALID, "no numeric values") ; return EMPTY ; }
        const Int *Super = L->super, *Lpi = L->pi, *Lpx = L->px ;
        const double *Lx = L->x ;
        const Int e = (L->xtype == CHOLMOD_COMPLEX) ? 2 : 1 ;
        lmin = lmax = Lx [0] ;
        if (lmin != lmin) return 0 ;
        for (Int s = 0 ; s < (Int) L->nsuper ; s++)
        {
            const Int nscol = Super [s+1] - Super [s], nsrow = Lpi [s+1] - Lpi [s], psx = Lpx [s] ;
            for (Int jj = 0 ; jj < nscol ; jj++)
            {
                const double ljj = Lx [e * (psx + jj + jj * nsrow)] ;
                if (ljj != ljj) return 0 ;
                if (ljj < lmin) lmin = ljj ; else if (ljj > lmax) lmax = ljj ;
            }
        }
    }
    double rcond = lmin / lmax ;
    if (L->is_ll) rcond = rcond * rcond ;
    return rcond ;
}

/* ---- cholmod_l_change_factor ---------------------------------------------------------------------- */

/* reference: Core/cholmod_change_factor.c:1005-1230, the supernodal conversions (the simplicial forms are not built):
 *   supernodal numeric  -> supernodal symbolic  (ll_super_to_super_symbolic, :373-393): the values are discarded -- L->x
 *                                                freed, the engine's resident copy forgotten (the plan, a function of the
 *                                                symbolic factor, stays) --, xtype = PATTERN, minor = n;
 *   supernodal symbolic -> supernodal numeric   (super_symbolic_to_ll_super, :946-989): L->x allocated, contents
 *                                                undefined, xtype = to_xtype, minor = n -- what cholmod_l_super_numeric
 *                                                does on entry (cholmod_super_numeric.c:212-223);
 *   supernodal numeric  -> supernodal numeric   nothing to do.
 * to_ll / to_packed / to_monotonic only concern simplicial factors.  A failed conversion leaves L as it was. */
int cholmod_l_change_factor (int to_xtype, int to_ll, int to_super, int to_packed, int to_monotonic,
    cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    (void) to_ll ; (void) to_packed ; (void) to_monotonic ;
    if (L->xtype < CHOLMOD_PATTERN || L->xtype > CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_INVALID, "invalid xtype") ; return FALSE ; }
    if (to_xtype < CHOLMOD_PATTERN || to_xtype > CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_INVALID, "xtype invalid") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (to_super && to_xtype == CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_INVALID, "supernodal zomplex L not supported") ; return FALSE ; }
    if (!to_super || !L->is_super)
    {
        /* any conversion from or to a simplicial factor (:1053-1062, :1138-1224) */
        ERROR (CHOLMOD_NOT_INSTALLED, "simplicial factors are not built: only supernodal symbolic <-> numeric") ;
        return FALSE ;
    }
    if (to_xtype == CHOLMOD_PATTERN)
    {
        if (L->xtype == CHOLMOD_PATTERN) return TRUE ;
        const size_t w = (L->xtype == CHOLMOD_COMPLEX) ? 2 : 1 ;
        if (L->x) L->x = cholmod_l_free (L->xsize, w * sizeof (double), L->x, Common) ;
        if (L->cx_twin) cholmod_l_free_factor ((cholmod_factor **) &L->cx_twin, Common) ;
        L->xtype = CHOLMOD_PATTERN ; L->dtype = CHOLMOD_DOUBLE ;
        L->minor = L->n ; L->is_ll = TRUE ;
        L->hip_on_device = FALSE ; L->hip_host_valid = FALSE ; L->hip_apat_valid = FALSE ; L->hip_aat_valid = FALSE ;
        return TRUE ;
    }
    if (L->xtype != CHOLMOD_PATTERN) return TRUE ;       /* already numeric (:1129-1136: nothing to do) */
    if (!ssamd_factor_has_cholesky_sizes (L))
    { ERROR (CHOLMOD_INVALID, "L was analysed for SPQR (no Cholesky sizes)") ; return FALSE ; }
    const size_t w = (to_xtype == CHOLMOD_REAL) ? 1 : 2 ;
    double *Lx = cholmod_l_malloc (L->xsize, w * sizeof (double), Common) ;
    if (!Lx) return FALSE ;                                 /* out of memory: L unchanged */
    if (L->xsize == 1) { Lx [0] = 0 ; if (w == 2) Lx [1] = 0 ; }
    L->x = Lx ; L->xtype = to_xtype ; L->dtype = CHOLMOD_DOUBLE ; L->minor = L->n ; L->is_ll = TRUE ;
    L->hip_on_device = FALSE ; L->hip_host_valid = TRUE ;   /* (what the caller sees is L->x) */
    return TRUE ;
}

int cholmod_l_hip_prepare (cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (!L->is_super) { ERROR (CHOLMOD_INVALID, "L not supernodal") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (L->cx_twin) return ssamd_ensure_plan ((cholmod_factor *) L->cx_twin, Common) ;
    return ssamd_ensure_plan (L, Common) ;
}

int cholmod_l_gather_factor (cholmod_factor *L, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    if (L->cx_twin) return cholmod_l_gather_factor ((cholmod_factor *) L->cx_twin, Common) ;
    if (!L->hip_plan || !L->hip_on_device) { ERROR (CHOLMOD_INVALID, "no numeric factor") ; return FALSE ; }
    int rc = cholmod_hip_gather_factor ((cholmod_hip_plan *) L->hip_plan) ;
    if (rc != CHOLMOD_HIP_OK) return map_hip_status (rc, Common, "factor gather failed") ;
    return TRUE ;
}

int cholmod_l_hip_stats (cholmod_factor *L, double *stats, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (stats, FALSE) ;
    if (L->cx_twin) L = (cholmod_factor *) L->cx_twin ;
    if (!L->hip_plan) { ERROR (CHOLMOD_INVALID, "no plan") ; return FALSE ; }
    return cholmod_hip_get_stats ((cholmod_hip_plan *) L->hip_plan, stats) == CHOLMOD_HIP_OK ;
}

/* ---- triangular solves ---------------------------------------------------------------------- */

/* make sure the device holds the numeric values the caller sees in L->x */
static int factor_on_device (cholmod_factor *L, cholmod_common *Common)
{
    if (L->xtype != CHOLMOD_REAL || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a numeric supernodal factor") ; return FALSE ; }
    if (!ssamd_ensure_plan (L, Common)) return FALSE ;
    if (!L->hip_on_device)
    {
        if (!L->x) { ERROR (CHOLMOD_INVALID, "L has no values") ; return FALSE ; }
        int rc = cholmod_hip_upload_factor ((cholmod_hip_plan *) L->hip_plan, L->x) ;
        if (rc != CHOLMOD_HIP_OK) return map_hip_status (rc, Common, "factor upload failed") ;
        L->hip_on_device = TRUE ;
    }
    return TRUE ;
}

/* cholmod_l_solve with B and X in device memory, ordered on the caller's stream (cholmod.h) */
int cholmod_l_hip_solve_device (int sys, cholmod_factor *L, const double *B_dev, size_t ldb, double *X_dev, size_t ldx,
    size_t nrhs, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (B_dev, FALSE) ;
    RETURN_IF_NULL (X_dev, FALSE) ;
    if (sys < CHOLMOD_A || sys > CHOLMOD_Pt) { ERROR (CHOLMOD_INVALID, "invalid system") ; return FALSE ; }
    if (ldb < L->n || ldx < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX)
    { ERROR (CHOLMOD_NOT_INSTALLED, "a device solve with a complex factor is not supported") ; return FALSE ; }
    if (L->xtype != CHOLMOD_REAL || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a numeric supernodal factor") ; return FALSE ; }
    /* device pointers cannot be solved against on the host: no fallback, whatever Common->hip_cpu_fallback says */
    if (ssamd_resolve_use_gpu (Common) != 1) { ERROR (CHOLMOD_INVALID, "a device solve needs Common->useGPU") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (!factor_on_device (L, Common)) return FALSE ;
    if (nrhs == 0 || L->n == 0) return TRUE ;
    cholmod_hip_plan *plan = (cholmod_hip_plan *) L->hip_plan ;
    /* what the engine does for each system (as cholmod_l_solve2 below does on the host) */
    const int perm_in = (sys == CHOLMOD_A || sys == CHOLMOD_P), perm_out = (sys == CHOLMOD_A || sys == CHOLMOD_Pt) ;
    const int which = (sys == CHOLMOD_A || sys == CHOLMOD_LDLt) ? 0
                    : (sys == CHOLMOD_L || sys == CHOLMOD_LD) ? 1
                    : (sys == CHOLMOD_Lt || sys == CHOLMOD_DLt) ? 2 : 3 ;
    if ((perm_in || perm_out) && !ssamd_perm_ready (L, Common)) return FALSE ;
    int rc = cholmod_hip_solve_device (plan, which, perm_in, perm_out, B_dev, (int64_t) ldb, X_dev, (int64_t) ldx,
        (int64_t) nrhs, stream) ;
    return (rc == CHOLMOD_HIP_OK) ? TRUE : map_hip_status (rc, Common, "HIP device solve failed") ;
}

/* what cholmod_l_hip_residual_device and cholmod_l_hip_refine_device check alike, in the order of the solve above; then
 * the permutation goes to the plan.  TRUE: *plan is ready (NULL: nothing to do). */
static int residual_ready (cholmod_factor *L, size_t ld1, size_t ld2, size_t ld3, size_t nrhs, cholmod_hip_plan **plan,
    cholmod_common *Common)
{
    *plan = NULL ;
    if (ld1 < L->n || ld2 < L->n || ld3 < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
    if (L->xtype == CHOLMOD_COMPLEX || L->xtype == CHOLMOD_ZOMPLEX)
    { ERROR (CHOLMOD_NOT_INSTALLED, "a device residual with a complex factor is not supported") ; return FALSE ; }
    if (L->xtype != CHOLMOD_REAL || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a numeric supernodal factor") ; return FALSE ; }
    if (ssamd_resolve_use_gpu (Common) != 1) { ERROR (CHOLMOD_INVALID, "a device residual needs Common->useGPU") ; return FALSE ; }
    if (Common->hip_world > 1) { ERROR (CHOLMOD_INVALID, "the device residual runs on one rank only") ; return FALSE ; }
    if (!L->hip_plan || !L->hip_on_device)
    { ERROR (CHOLMOD_INVALID, "no resident matrix: L was not factorized on the device") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (nrhs == 0 || L->n == 0) return TRUE ;
    if (!ssamd_perm_ready (L, Common)) return FALSE ;
    *plan = (cholmod_hip_plan *) L->hip_plan ;
    return TRUE ;
}

/* (everything else that is invalid has been checked above: what the engine still refuses is a plan without a matrix) */
static int residual_status (int rc, cholmod_common *Common, const char *what)
{
    if (rc == CHOLMOD_HIP_OK) return TRUE ;
    if (rc == CHOLMOD_HIP_INVALID)
    { ERROR (CHOLMOD_INVALID, "no resident matrix: the plan holds a factor that was not computed from a matrix on the device") ; return FALSE ; }
    return map_hip_status (rc, Common, what) ;
}

/* R = B - A X with all three in device memory, A the matrix L was last factorized from on the device (cholmod.h) */
int cholmod_l_hip_residual_device (cholmod_factor *L, const double *X_dev, size_t ldx, const double *B_dev, size_t ldb,
    double *R_dev, size_t ldr, size_t nrhs, double *Rnorm_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (X_dev, FALSE) ;
    RETURN_IF_NULL (B_dev, FALSE) ;
    RETURN_IF_NULL (R_dev, FALSE) ;
    if (R_dev == X_dev) { ERROR (CHOLMOD_INVALID, "R must not be X") ; return FALSE ; }
    cholmod_hip_plan *plan ;
    if (!residual_ready (L, ldx, ldb, ldr, nrhs, &plan, Common)) return FALSE ;
    if (!plan) return TRUE ;
    return residual_status (cholmod_hip_residual_device (plan, 1, X_dev, (int64_t) ldx, B_dev, (int64_t) ldb, R_dev,
        (int64_t) ldr, (int64_t) nrhs, Rnorm_dev, stream), Common, "HIP device residual failed") ;
}

/* `steps` rounds of iterative refinement of X against B, in place in device memory (cholmod.h) */
int cholmod_l_hip_refine_device (cholmod_factor *L, const double *B_dev, size_t ldb, double *X_dev, size_t ldx,
    size_t nrhs, int steps, double *Rnorm_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (B_dev, FALSE) ;
    RETURN_IF_NULL (X_dev, FALSE) ;
    if (steps < 0) { ERROR (CHOLMOD_INVALID, "steps must not be negative") ; return FALSE ; }
    cholmod_hip_plan *plan ;
    if (!residual_ready (L, ldb, ldx, ldx, nrhs, &plan, Common)) return FALSE ;
    if (!plan) return TRUE ;
    return residual_status (cholmod_hip_refine_device (plan, 1, B_dev, (int64_t) ldb, X_dev, (int64_t) ldx, (int64_t) nrhs,
        steps, Rnorm_dev, stream), Common, "HIP device refinement failed") ;
}

/* ---- the same three for a complex factor (cholmod.h) ----------------------------------------------------------------
 * The solves with L and L^H are the real solves with the twin on the interleaved right-hand side, the same bytes
 * (complex.c): the twin's plan gets 2 ld doubles per column and the same nrhs.  The twin's own Perm is the identity (the
 * matrix it was factorized from is already permuted), so the plan is handed the complex factor's permutation expanded
 * to the twin's rows, once per twin (T->hip_perm_set; a new plan clears it). */

/* what the three check alike, before any device call; TRUE: *plan is the twin's, ready (NULL: nothing to do) */
static int complex_device_ready (cholmod_factor *L, size_t ld1, size_t ld2, size_t ld3, size_t nrhs, cholmod_hip_plan **plan,
    cholmod_common *Common)
{
    *plan = NULL ;
    if (ld1 < L->n || ld2 < L->n || ld3 < L->n) { ERROR (CHOLMOD_INVALID, "leading dimension smaller than n") ; return FALSE ; }
    if (L->xtype == CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_NOT_INSTALLED, "zomplex factors are not supported") ; return FALSE ; }
    if (L->xtype != CHOLMOD_COMPLEX || !L->is_super)
    { ERROR (CHOLMOD_INVALID, "L must be a complex numeric supernodal factor (a real L: cholmod_l_hip_solve_device)") ; return FALSE ; }
    if (ssamd_resolve_use_gpu (Common) != 1) { ERROR (CHOLMOD_INVALID, "device arrays need Common->useGPU") ; return FALSE ; }
    if (Common->hip_world > 1) { ERROR (CHOLMOD_INVALID, "complex device arrays are served on one rank only") ; return FALSE ; }
    cholmod_factor *T = (cholmod_factor *) L->cx_twin ;
    if (!T || !T->hip_plan || !T->hip_on_device)
    { ERROR (CHOLMOD_INVALID, "L was not factorized on the device") ; return FALSE ; }
    Common->status = CHOLMOD_OK ;
    if (nrhs == 0 || L->n == 0) return TRUE ;
    if (!T->hip_perm_set)
    {
        const Int n = (Int) L->n, *Perm = L->Perm ;
        int64_t *P2 = cholmod_l_malloc (2 * (size_t) n, sizeof (int64_t), Common) ;
        if (!P2) return FALSE ;
        for (Int k = 0 ; k < n ; k++) { P2 [2*k] = 2 * (int64_t) Perm [k] ; P2 [2*k+1] = 2 * (int64_t) Perm [k] + 1 ; }
        int rc = cholmod_hip_set_perm ((cholmod_hip_plan *) T->hip_plan, P2) ;
        cholmod_l_free (2 * (size_t) n, sizeof (int64_t), P2, Common) ;
        if (rc != CHOLMOD_HIP_OK) return map_hip_status (rc, Common, "the permutation could not be stored on the device") ;
        T->hip_perm_set = TRUE ;
    }
    *plan = (cholmod_hip_plan *) T->hip_plan ;
    return TRUE ;
}

int cholmod_l_hip_solve_device_complex (int sys, cholmod_factor *L, const void *B_dev, size_t ldb, void *X_dev, size_t ldx,
    size_t nrhs, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (B_dev, FALSE) ;
    RETURN_IF_NULL (X_dev, FALSE) ;
    if (sys < CHOLMOD_A || sys > CHOLMOD_Pt) { ERROR (CHOLMOD_INVALID, "invalid system") ; return FALSE ; }
    cholmod_hip_plan *plan ;
    if (!complex_device_ready (L, ldb, ldx, ldx, nrhs, &plan, Common)) return FALSE ;
    if (!plan) return TRUE ;
    /* as in cholmod_l_hip_solve_device: L' of the twin is L^H of the complex factor */
    const int perm_in = (sys == CHOLMOD_A || sys == CHOLMOD_P), perm_out = (sys == CHOLMOD_A || sys == CHOLMOD_Pt) ;
    const int which = (sys == CHOLMOD_A || sys == CHOLMOD_LDLt) ? 0
                    : (sys == CHOLMOD_L || sys == CHOLMOD_LD) ? 1
                    : (sys == CHOLMOD_Lt || sys == CHOLMOD_DLt) ? 2 : 3 ;
    int rc = cholmod_hip_solve_device (plan, which, perm_in, perm_out, (const double *) B_dev, (int64_t) (2 * ldb),
        (double *) X_dev, (int64_t) (2 * ldx), (int64_t) nrhs, stream) ;
    return (rc == CHOLMOD_HIP_OK) ? TRUE : map_hip_status (rc, Common, "HIP device solve failed") ;
}

int cholmod_l_hip_residual_device_complex (cholmod_factor *L, const void *X_dev, size_t ldx, const void *B_dev, size_t ldb,
    void *R_dev, size_t ldr, size_t nrhs, double *Rnorm_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (X_dev, FALSE) ;
    RETURN_IF_NULL (B_dev, FALSE) ;
    RETURN_IF_NULL (R_dev, FALSE) ;
    if (R_dev == X_dev) { ERROR (CHOLMOD_INVALID, "R must not be X") ; return FALSE ; }
    cholmod_hip_plan *plan ;
    if (!complex_device_ready (L, ldx, ldb, ldr, nrhs, &plan, Common)) return FALSE ;
    if (!plan) return TRUE ;
    return residual_status (cholmod_hip_residual_device (plan, 1, (const double *) X_dev, (int64_t) (2 * ldx),
        (const double *) B_dev, (int64_t) (2 * ldb), (double *) R_dev, (int64_t) (2 * ldr), (int64_t) nrhs, Rnorm_dev, stream),
        Common, "HIP device residual failed") ;
}

int cholmod_l_hip_refine_device_complex (cholmod_factor *L, const void *B_dev, size_t ldb, void *X_dev, size_t ldx,
    size_t nrhs, int steps, double *Rnorm_dev, void *stream, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (B_dev, FALSE) ;
    RETURN_IF_NULL (X_dev, FALSE) ;
    if (steps < 0) { ERROR (CHOLMOD_INVALID, "steps must not be negative") ; return FALSE ; }
    cholmod_hip_plan *plan ;
    if (!complex_device_ready (L, ldb, ldx, ldx, nrhs, &plan, Common)) return FALSE ;
    if (!plan) return TRUE ;
    return residual_status (cholmod_hip_refine_device (plan, 1, (const double *) B_dev, (int64_t) (2 * ldb), (double *) X_dev,
        (int64_t) (2 * ldx), (int64_t) nrhs, steps, Rnorm_dev, stream), Common, "HIP device refinement failed") ;
}

/* the triangular solves run where the factor is: on the host when the values are
 * in L->x and the engine is not to be used (Common->useGPU == 0, no device, or a
 * factor the CPU path computed) */
static int solve_on_host (cholmod_factor *L, cholmod_common *Common)
{
    if (L->xtype != CHOLMOD_REAL || !L->is_super || !L->x) return FALSE ;
    if (L->hip_on_device && !L->hip_host_valid) return FALSE ;      /* current values only in HBM */
    if (L->hip_on_device) return FALSE ;                            /* resident copy: use it */
    if (ssamd_resolve_use_gpu (Common) != 1) return TRUE ;
    /* a GPU was asked for: the host solve is only the opted-in degradation */
    return Common->hip_cpu_fallback && (!L->useGPU || !cholmod_hip_probe ()) ;
}

static int super_solve (int which, cholmod_factor *L, cholmod_dense *X, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (X, FALSE) ;
    /* L and X must be of the same kind (reference cholmod_super_solve.c:70-75); a complex
     * X against a complex L is the real system of the twin on the same bytes (complex.c) */
    Int ldx = (Int) X->d ;
    if (L->xtype == CHOLMOD_COMPLEX && L->cx_twin)
    {
        if (X->xtype != CHOLMOD_COMPLEX) { ERROR (CHOLMOD_INVALID, "L and X must both be complex") ; return FALSE ; }
        if (X->nrow != L->n || X->d < X->nrow) { ERROR (CHOLMOD_INVALID, "X and L dimensions must match") ; return FALSE ; }
        L = (cholmod_factor *) L->cx_twin ;
        ldx *= 2 ;
    }
    else
    {
        if (X->xtype != CHOLMOD_REAL) { ERROR (CHOLMOD_INVALID, "X must be real") ; return FALSE ; }
        if (X->nrow != L->n || X->d < X->nrow) { ERROR (CHOLMOD_INVALID, "X and L dimensions must match") ; return FALSE ; }
    }
    Common->status = CHOLMOD_OK ;
    if (solve_on_host (L, Common))
    {
        ssamd_cpu_super_solve (which, L, X->x, (Int) X->ncol, ldx) ;
        return Common->blas_ok ;
    }
    if (!factor_on_device (L, Common)) return FALSE ;
    int rc = cholmod_hip_solve ((cholmod_hip_plan *) L->hip_plan, which, X->x, (int64_t) X->ncol, (int64_t) ldx) ;
    if (rc != CHOLMOD_HIP_OK) return map_hip_status (rc, Common, "HIP solve failed") ;
    return Common->blas_ok ;
}

/* reference: Supernodal/cholmod_super_solve.c:43-134 / :136-231.  E (workspace
 * in the reference) is accepted and ignored. */
int cholmod_l_super_lsolve (cholmod_factor *L, cholmod_dense *X, cholmod_dense *E, cholmod_common *Common)
{
    (void) E ;
    return super_solve (1, L, X, Common) ;
}

int cholmod_l_super_ltsolve (cholmod_factor *L, cholmod_dense *X, cholmod_dense *E, cholmod_common *Common)
{
    (void) E ;
    return super_solve (2, L, X, Common) ;
}

/* reference: Cholesky/cholmod_solve.c:946-1030 and the supernodal branch of
 * solve2 (:1541-1580): Y = P B, L solves, X = P' Y.  LL' factors only, so the
 * LDL' system codes collapse as in the reference (D = I). */
cholmod_dense *cholmod_l_solve (int sys, cholmod_factor *L, cholmod_dense *B, cholmod_common *Common)
{
    cholmod_dense *X = NULL ;
    if (!cholmod_l_solve2 (sys, L, B, NULL, &X, NULL, NULL, NULL, Common))
        cholmod_l_free_dense (&X, Common) ;
    return X ;
}

/* entry (k, r) of a dense matrix of any numeric kind */
static inline void dense_get (const cholmod_dense *B, Int k, Int r, double *re, double *im)
{
    size_t q = (size_t) k + (size_t) r * B->d ;
    const double *x = B->x ;
    if (B->xtype == CHOLMOD_COMPLEX) { *re = x [2*q] ; *im = x [2*q+1] ; }
    else { *re = x [q] ; *im = (B->xtype == CHOLMOD_ZOMPLEX) ? ((const double *) B->z) [q] : 0.0 ; }
}

static inline void dense_put (cholmod_dense *X, Int k, Int r, double re, double im)
{
    size_t q = (size_t) k + (size_t) r * X->d ;
    double *x = X->x ;
    if (X->xtype == CHOLMOD_COMPLEX) { x [2*q] = re ; x [2*q+1] = im ; }
    else { x [q] = re ; if (X->xtype == CHOLMOD_ZOMPLEX) ((double *) X->z) [q] = im ; }
}

int cholmod_l_solve2 (int sys, cholmod_factor *L, cholmod_dense *B, cholmod_sparse *Bset,
    cholmod_dense **X_Handle, cholmod_sparse **Xset_Handle, cholmod_dense **Y_Handle,
    cholmod_dense **E_Handle, cholmod_common *Common)
{
    RETURN_IF_NULL_COMMON (FALSE) ;
    RETURN_IF_NULL (L, FALSE) ;
    RETURN_IF_NULL (B, FALSE) ;
    RETURN_IF_NULL (X_Handle, FALSE) ;
    (void) E_Handle ;
    if (sys < CHOLMOD_A || sys > CHOLMOD_Pt) { ERROR (CHOLMOD_INVALID, "invalid system") ; return FALSE ; }
    if (B->xtype < CHOLMOD_REAL || B->xtype > CHOLMOD_ZOMPLEX) { ERROR (CHOLMOD_INVALID, "B must be numeric") ; return FALSE ; }
    if (B->d < L->n || B->nrow != L->n) { ERROR (CHOLMOD_INVALID, "dimensions of L and B do not match") ; return FALSE ; }
    if (Bset)
    {
        /* (reference cholmod_solve.c:1081-1094) */
        if (B->ncol != 1) { ERROR (CHOLMOD_INVALID, "Bset requires a single right-hand side") ; return FALSE ; }
        if (L->xtype != B->xtype) { ERROR (CHOLMOD_INVALID, "Bset requires xtype of L and B to match") ; return FALSE ; }
    }
    Common->status = CHOLMOD_OK ;
    Int n = (Int) L->n, nrhs = (Int) B->ncol ;
    const int Lcomplex = (L->xtype == CHOLMOD_COMPLEX) ;
    const int Bcomplex = (B->xtype != CHOLMOD_REAL) ;
    /* kind of X (reference cholmod_solve.c:1112-1134): real if L and B are real (P, Pt:
     * if B is real), else the preferred complex kind */
    const int ctype = Common->prefer_zomplex ? CHOLMOD_ZOMPLEX : CHOLMOD_COMPLEX ;
    int xtype = (sys == CHOLMOD_P || sys == CHOLMOD_Pt) ? (Bcomplex ? ctype : CHOLMOD_REAL)
              : (!Lcomplex && !Bcomplex) ? CHOLMOD_REAL : ctype ;
    cholmod_dense *X = *X_Handle ;
    if (!X || X->nrow != (size_t) n || X->ncol != (size_t) nrhs || X->xtype != xtype)
    {
        cholmod_l_free_dense (X_Handle, Common) ;
        X = cholmod_l_allocate_dense (n, nrhs, n, xtype, Common) ;
        if (!X) return FALSE ;
        *X_Handle = X ;
    }
    /* a sparse right-hand side: the entries of X on the pattern Bset reaches, subset_solve.c */
    if (Bset) return ssamd_solve_subset (sys, L, B, Bset, X, Xset_Handle, Y_Handle, Common) ;
    const Int *Perm = L->Perm ;
    double re, im ;
    if (sys == CHOLMOD_P || sys == CHOLMOD_Pt || sys == CHOLMOD_D)
    {
        for (Int r = 0 ; r < nrhs ; r++)
            for (Int k = 0 ; k < n ; k++)
            {
                dense_get (B, sys == CHOLMOD_P ? Perm [k] : k, r, &re, &im) ;
                dense_put (X, sys == CHOLMOD_Pt ? Perm [k] : k, r, re, im) ;
            }
        return TRUE ;
    }
    int which = (sys == CHOLMOD_A || sys == CHOLMOD_LDLt) ? 0
              : (sys == CHOLMOD_L || sys == CHOLMOD_LD) ? 1 : 2 ;
    /* the system the engine sees: a complex L is the real twin of order 2n acting on
     * interleaved vectors (complex.c); a real L against a complex B solves the real and
     * the imaginary parts as 2 nrhs real right-hand sides (the reference's "dual" Y,
     * cholmod_solve.c:1553) */
    cholmod_factor *Lr = L ;
    if (Lcomplex)
    {
        if (!L->cx_twin) { ERROR (CHOLMOD_INVALID, "complex L without its engine factor") ; return FALSE ; }
        Lr = (cholmod_factor *) L->cx_twin ;
    }
    const Int yn = Lcomplex ? 2 * n : n ;
    const Int ycols = (!Lcomplex && Bcomplex) ? 2 * nrhs : nrhs ;
    int on_host = solve_on_host (Lr, Common) ;
    if (!on_host && !factor_on_device (Lr, Common)) return FALSE ;
    cholmod_dense *Y = cholmod_l_allocate_dense (yn, ycols, yn, CHOLMOD_REAL, Common) ;
    if (!Y) return FALSE ;
    double *Yx = Y->x ;
    const int nth = ssamd_host_threads () ;
    for (Int r = 0 ; r < nrhs ; r++)
    {
#pragma omp parallel for schedule(static) num_threads(nth) if (n > 100000)
        for (Int k = 0 ; k < n ; k++)
        {
            double re, im ;
            dense_get (B, sys == CHOLMOD_A ? Perm [k] : k, r, &re, &im) ;
            if (Lcomplex) { Yx [2*k + r*yn] = re ; Yx [2*k+1 + r*yn] = im ; }
            else { Yx [k + r*yn] = re ; if (Bcomplex) Yx [k + (nrhs + r)*yn] = im ; }
        }
    }
    int ok = TRUE ;
    if (on_host) ssamd_cpu_super_solve (which, Lr, Yx, ycols, yn) ;
    else
    {
        int rc = cholmod_hip_solve ((cholmod_hip_plan *) Lr->hip_plan, which, Yx, ycols, yn) ;
        ok = (rc == CHOLMOD_HIP_OK) ? TRUE : map_hip_status (rc, Common, "HIP solve failed") ;
    }
    if (ok)
        for (Int r = 0 ; r < nrhs ; r++)
        {
#pragma omp parallel for schedule(static) num_threads(nth) if (n > 100000)
            for (Int k = 0 ; k < n ; k++)
            {
                double re, im ;
                if (Lcomplex) { re = Yx [2*k + r*yn] ; im = Yx [2*k+1 + r*yn] ; }
                else { re = Yx [k + r*yn] ; im = Bcomplex ? Yx [k + (nrhs + r)*yn] : 0.0 ; }
                dense_put (X, sys == CHOLMOD_A ? Perm [k] : k, r, re, im) ;
            }
        }
    cholmod_l_free_dense (&Y, Common) ;
    return ok ;
}
