// grad.hip -- what backpropagation through a device-resident factorization needs, without leaving the device: the
// gradient with respect to the values of A sampled on the pattern of the resident S (cholmod_hip_values_grad_device: for
// X = (A + beta I)^-1 B and Lambda = (A + beta I)^-1 gX it is -(Lambda X' + X Lambda') on A's entries) and log det
// (A + beta I) of the resident factor as a device scalar (cholmod_hip_logdet_device; its gradient is the selected
// inverse, selinv.hip).  Kernels: grad_kernels.hip.h; the pack kernel of the panels comes through solve_internal.hip.h.
// No test hook reaches this file: it is built once for both libraries.
#include "grad_kernels.hip.h"
#include "solve_internal.hip.h"

struct Grad {
    double *d_U = nullptr, *d_V = nullptr ;     // the panels [n][16] of U and V in the factor's ordering
    double *d_part = nullptr ;                  // partial sums of the log-determinant, one per 256 columns
    i32 *d_col = nullptr ; i64 col_cap = 0 ;    // the column of every entry of the resident S (P->gr_index_valid)
    hipEvent_t ev_in = nullptr, ev_out = nullptr ;
} ;

namespace {

#define GR_TRY(call) do { int rc_ = (call) ; if (rc_ != CHOLMOD_HIP_OK) return rc_ ; } while (0)

// what both entry points refuse, before any device call
static bool bad_plan (const cholmod_hip_plan *P)
{
    if (!P || P->host_only || P->world > 1) return true ;
    return (P->flags & (CHOLMOD_HIP_CX_STORAGE | CHOLMOD_HIP_PHI_TWIN)) != 0 ;          // real factors only
}

static int alloc (double **into, i64 count)
{
    if (*into) return CHOLMOD_HIP_OK ;
    const hipError_t e = hipMalloc ((void **) into, (size_t) std::max<i64> (count, 1) * sizeof (double)) ;
    if (e == hipSuccess) return CHOLMOD_HIP_OK ;
    (void) hipGetLastError () ;
    *into = nullptr ;
    return e == hipErrorOutOfMemory ? CHOLMOD_HIP_OUT_OF_MEMORY : CHOLMOD_HIP_GPU_PROBLEM ;
}

// The column-of-entry array of the resident S, next to the residual's transposed index: void when S is uploaded anew,
// built by the first call after that -- on the engine stream, from Sp alone, without a host wait; its buffer is kept
// and grows only with a larger S.
static int ensure_index (cholmod_hip_plan *P)
{
    Grad *g = P->gr ;
    const i64 nz = P->s_cur_nz ;
    if (P->gr_index_valid) return CHOLMOD_HIP_OK ;
    if (nz > g->col_cap || !g->d_col)
    {
        if (g->d_col) { HIPCHK (hipStreamSynchronize (P->stream)) ; (void) hipFree (g->d_col) ; g->d_col = nullptr ; g->col_cap = 0 ; }
        const hipError_t e = hipMalloc ((void **) &g->d_col, (size_t) std::max<i64> (nz, 1) * sizeof (i32)) ;
        if (e != hipSuccess)
        {
            (void) hipGetLastError () ;
            g->d_col = nullptr ;
            return e == hipErrorOutOfMemory ? CHOLMOD_HIP_OUT_OF_MEMORY : CHOLMOD_HIP_GPU_PROBLEM ;
        }
        g->col_cap = std::max<i64> (nz, 1) ;
    }
    if (nz > 0)
        hipLaunchKernelGGL (k_gr_column_index, dim3 ((unsigned) ((nz + 255) / 256)), dim3 (256), 0, P->stream, P->n, nz, P->d_Sp, g->d_col) ;
    P->gr_index_valid = true ;
    return CHOLMOD_HIP_OK ;
}

// the events; `panels`: the two panels; `partials`: the buffer of the log-determinant.  Nothing is allocated once they exist.
static int ensure (cholmod_hip_plan *P, bool panels, bool partials)
{
    if (!P->gr) P->gr = new (std::nothrow) Grad ;
    Grad *g = P->gr ;
    if (!g) return CHOLMOD_HIP_OUT_OF_MEMORY ;
    if (!g->ev_in) HIPCHK (hipEventCreateWithFlags (&g->ev_in, hipEventDisableTiming)) ;
    if (!g->ev_out) HIPCHK (hipEventCreateWithFlags (&g->ev_out, hipEventDisableTiming)) ;
    if (panels)
    {
        GR_TRY (alloc (&g->d_U, P->n * GR_NP)) ;
        GR_TRY (alloc (&g->d_V, P->n * GR_NP)) ;
    }
    if (partials) GR_TRY (alloc (&g->d_part, (P->n + 255) / 256)) ;
    return CHOLMOD_HIP_OK ;
}

// the engine stream takes its place in the caller's order: behind what the caller has enqueued ...
static int enter (cholmod_hip_plan *P, hipStream_t user)
{
    HIPCHK (hipEventRecord (P->gr->ev_in, user)) ;
    HIPCHK (hipStreamWaitEvent (P->stream, P->gr->ev_in, 0)) ;
    return CHOLMOD_HIP_OK ;
}

// ... and ahead of what the caller enqueues next
static int leave (cholmod_hip_plan *P, hipStream_t user)
{
    HIPCHK (hipGetLastError ()) ;
    HIPCHK (hipEventRecord (P->gr->ev_out, P->stream)) ;
    HIPCHK (hipStreamWaitEvent (user, P->gr->ev_out, 0)) ;
    return CHOLMOD_HIP_OK ;
}

static unsigned blocks_of (i64 count) { return (unsigned) ((count + 255) / 256) ; }

} // namespace

void grad_free (cholmod_hip_plan *P)
{
    Grad *g = P->gr ;
    P->gr = nullptr ;
    if (!g) return ;
    P->gr_index_valid = false ;
    for (void *d : {(void *) g->d_U, (void *) g->d_V, (void *) g->d_part, (void *) g->d_col}) if (d) (void) hipFree (d) ;
    for (hipEvent_t e : {g->ev_in, g->ev_out}) if (e) (void) hipEventDestroy (e) ;
    delete g ;
}

extern "C" {

int cholmod_hip_values_grad_device (cholmod_hip_plan *P, int perm, double alpha, const double *dU, int64_t ldu,
    const double *dV, int64_t ldv, int64_t nrhs, double *dG, int64_t nvalues, void *stream)
{
    if (bad_plan (P) || !dU || !dV || !dG || nrhs < 0 || ldu < P->n || ldv < P->n) return CHOLMOD_HIP_INVALID ;
    // the value map of the current resident packed S, and values that are given, not computed
    if (!P->d_Sp || !P->d_vsrc || P->s_unpacked || P->vsrc_nz != P->s_cur_nz || nvalues != P->vals_n || P->pm_set)
        return CHOLMOD_HIP_INVALID ;
    if (perm && !P->d_perm) return CHOLMOD_HIP_INVALID ;                                // cholmod_hip_set_perm first
    const i64 n = P->n, nz = P->s_cur_nz ;
    if (n == 0 || nvalues == 0) return CHOLMOD_HIP_OK ;
    const bool columns = nrhs < SD_BLOCK_MIN_NRHS ;
    GR_TRY (ensure (P, !columns, false)) ;
    GR_TRY (ensure_index (P)) ;
    const i32 *col = P->gr->d_col ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    GR_TRY (enter (P, user)) ;
    // every value the factorization does not read: +0.0, in a pass of its own ahead of the writes through src []
    hipLaunchKernelGGL (k_gr_zero_fill, dim3 (blocks_of (nvalues)), dim3 (256), 0, st, (i64) nvalues, dG) ;
    const i64 *pm = perm ? P->d_perm : nullptr ;
    if (nz > 0 && nrhs > 0 && columns)
        hipLaunchKernelGGL (k_gr_columns, dim3 (blocks_of (nz)), dim3 (256), 0, st, n, nz, P->d_Sp, P->d_Si, col, P->d_vsrc, pm,
            dU, (i64) ldu, dV, (i64) ldv, (int) nrhs, alpha, dG) ;
    else if (nz > 0 && nrhs > 0)
    {
        const bool same = (dU == dV && ldu == ldv) ;
        double *Wu = P->gr->d_U, *Wv = same ? Wu : P->gr->d_V ;
        for (i64 r0 = 0 ; r0 < nrhs ; r0 += GR_NP)
        {
            const int pw = (int) std::min<i64> (GR_NP, nrhs - r0) ;
            sd_pack (st, n, pm, dU + r0 * ldu, ldu, pw, Wu) ;
            if (!same) sd_pack (st, n, pm, dV + r0 * ldv, ldv, pw, Wv) ;
            hipLaunchKernelGGL (k_gr_panel, dim3 (blocks_of (nz)), dim3 (256), 0, st, n, nz, P->d_Sp, P->d_Si, col, P->d_vsrc,
                (const double *) Wu, (const double *) Wv, r0 == 0 ? 1 : 0, r0 + GR_NP >= nrhs ? 1 : 0, alpha, dG) ;
        }
    }
    return leave (P, user) ;
}

int cholmod_hip_logdet_device (cholmod_hip_plan *P, double *dOut, void *stream)
{
    if (bad_plan (P) || !dOut) return CHOLMOD_HIP_INVALID ;
    if (P->factor_state != 1 || !P->d_Lx) return CHOLMOD_HIP_INVALID ;  // no numeric factor on the device, or one that is not positive definite
    GR_TRY (ensure (P, false, true)) ;
    const i64 n = P->n, nparts = (n + 255) / 256 ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    GR_TRY (enter (P, user)) ;
    if (nparts > 0)
        hipLaunchKernelGGL (k_gr_logdet_partial, dim3 ((unsigned) nparts), dim3 (256), 0, st, n, P->d_supermap, P->d_fr, P->d_Lx, P->gr->d_part) ;
    hipLaunchKernelGGL (k_gr_logdet_final, dim3 (1), dim3 (256), 0, st, nparts, (const double *) P->gr->d_part, dOut) ;
    return leave (P, user) ;
}

} // extern "C"
