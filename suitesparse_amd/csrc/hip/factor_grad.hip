// factor_grad.hip -- the gradient through the factor on the device: given Lbar = df/dL on the pattern of L -- an array of
// the caller's (cholmod_hip_factor_grad_device) or a sampled outer product alpha P Q' formed here
// (cholmod_hip_factor_outer_grad_device: the gradients of the two triangular solves) --, Gx = df/dS on the pattern of L in
// the layout of Lx, S = L L' = P (A + beta I) P' lower-stored, and what a caller takes from it without leaving the device
// (cholmod_hip_factor_grad_gather_device: the gradient with respect to the values of its matrix, and the trace, which is the
// gradient with respect to beta).  Reverse-mode Cholesky as a supernodal sweep from the roots down: the sweep of the
// selected inverse with another recurrence (factor_grad_kernels.hip.h).  It RUNS THE PROGRAM OF THE SELECTED INVERSE --
// the same batches, chunks, slots, tasks and partial offsets, built once by selinv.hip -- on the same scratch
// (selinv_internal.hip.h); only Gx, the partial sums of the trace and the clock are its own.  The sweep works in place: Gx
// holds Lbar when it begins.  No test hook reaches this file: it is built once for both libraries.
#include "factor_grad_kernels.hip.h"
#include "selinv_internal.hip.h"

namespace {

// Gx, the scratch and the program (sweep_ensure), the partial sums of the trace, the attributes of the kernels; nothing is
// allocated once they exist
static int ensure (cholmod_hip_plan *P)
{
    HIP_TRY (sweep_ensure (P, &SelInv::d_Gx)) ;
    SelInv *S = P->si ;
    if (!S->d_tr)
    {
        const int rc = device_alloc (&S->d_tr, (P->n + 255) / 256) ;
        if (rc != CHOLMOD_HIP_OK)
        {
            sweep_release (P, &SelInv::d_Gx) ;          // (the factor is untouched)
            return rc ;
        }
    }
    if (!S->fg_ready)
    {
        HIPCHK (hipFuncSetAttribute ((const void *) k_fg_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int) SI_BLOCK_LDS)) ;
        HIPCHK (hipFuncSetAttribute ((const void *) k_fg_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int) SI_BLOCK_LDS)) ;
        HIPCHK (hipFuncSetAttribute ((const void *) k_fg_thin, hipFuncAttributeMaxDynamicSharedMemorySize, SI_THIN_LDS_MAX)) ;
        S->fg_ready = true ;
    }
    return CHOLMOD_HIP_OK ;
}

// the program of the selected inverse with the kernels of the recurrence, in place on Gx
static void run (cholmod_hip_plan *P, hipStream_t st)
{
    SelInv *S = P->si ;
    const FrontD *fr = P->d_fr ;
    const double *Lx = P->d_Lx ;
    for (const SelInv::Step &s : S->steps)
    {
        const SiTask *t = S->d_tasks + s.first ;
        const dim3 grid (s.grid), wg (256) ;
        switch (s.kind)
        {
            case SelInv::THIN:
                hipLaunchKernelGGL (k_fg_thin, grid, wg, s.lds, st, S->d_thin + s.first, fr, P->d_supermap, P->d_Ls, Lx, S->d_Gx) ;
                break ;
            case SelInv::FILL:
                hipLaunchKernelGGL (k_fg_fill, grid, wg, 0, st, t, s.ntasks, S->d_slots, fr, P->d_supermap, P->d_Ls, S->d_Gx, S->d_M) ;
                break ;
            case SelInv::BLOCK:
                hipLaunchKernelGGL (k_fg_block, grid, wg, s.lds, st, t, s.ntasks, S->d_slots, fr, Lx, S->d_Gx, S->d_M, S->d_P) ;
                break ;
            case SelInv::DIAG:
                hipLaunchKernelGGL (k_fg_diag, grid, wg, SI_BLOCK_LDS, st, t, S->d_slots, fr, Lx, S->d_Gx, S->d_M, S->d_P) ;
                break ;
            case SelInv::STORE:
                hipLaunchKernelGGL (k_fg_store, grid, wg, 0, st, t, s.ntasks, S->d_slots, fr, S->d_M, S->d_Gx) ;
                break ;
        }
    }
}

// One sweep behind the caller's stream: `seed` enqueues what leaves Lbar in Gx (a launch that the clock and info [1] count)
template <typename F> static int sweep (cholmod_hip_plan *P, void *stream, F seed)
{
    HIP_TRY (ensure (P)) ;
    SelInv *S = P->si ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    P->fg_valid = false ;
    HIP_TRY (stream_enter (P, user)) ;
    HIPCHK (hipEventRecord (S->fg_clock.ev0, st)) ;
    if (P->xsize > 0) HIP_TRY (seed (S->d_Gx, st)) ;
    run (P, st) ;
    HIPCHK (hipEventRecord (S->fg_clock.ev1, st)) ;
    HIP_TRY (stream_leave (P, user)) ;
    S->fg_clock.launches = (long) S->steps.size () + 1 ;
    S->fg_clock.pending = true ;
    P->fg_valid = true ;
    return CHOLMOD_HIP_OK ;
}

static bool no_gx (const cholmod_hip_plan *P) { return !P->fg_valid || !P->si || !P->si->d_Gx ; }

} // namespace

extern "C" {

int cholmod_hip_factor_grad_device (cholmod_hip_plan *P, const double *dLbar, void *stream)
{
    if (sweep_bad_plan (P) || !dLbar) return CHOLMOD_HIP_INVALID ;
    const size_t bytes = (size_t) P->xsize * sizeof (double) ;
    return sweep (P, stream, [=] (double *Gx, hipStream_t st) -> int
    {
        HIPCHK (hipMemcpyAsync (Gx, dLbar, bytes, hipMemcpyDeviceToDevice, st)) ;
        return CHOLMOD_HIP_OK ;
    }) ;
}

int cholmod_hip_factor_outer_grad_device (cholmod_hip_plan *P, double alpha, const double *dP, int64_t ldp, const double *dQ,
    int64_t ldq, int64_t nrhs, void *stream)
{
    if (sweep_bad_plan (P) || !dP || !dQ || nrhs < 0 || nrhs > INT32_MAX || ldp < P->n || ldq < P->n) return CHOLMOD_HIP_INVALID ;
    return sweep (P, stream, [=] (double *Gx, hipStream_t st) -> int
    {
        hipLaunchKernelGGL (k_fg_outer, dim3 ((unsigned) P->n), dim3 (256), 0, st, P->d_supermap, P->d_fr, P->d_Ls, alpha, dP, (i64) ldp,
            dQ, (i64) ldq, (int) nrhs, Gx) ;
        return CHOLMOD_HIP_OK ;
    }) ;
}

int cholmod_hip_factor_grad_gather_device (cholmod_hip_plan *P, double *dG, int64_t nvalues, double *dTrace, void *stream)
{
    if (sweep_bad_plan (P) || no_gx (P)) return CHOLMOD_HIP_INVALID ;
    if (dG)
    {
        // the value map of the current resident packed S, and values that are given, not computed
        if (!P->d_Sp || !P->d_vsrc || P->s_unpacked || P->vsrc_nz != P->s_cur_nz || nvalues != P->vals_n || P->pm_set)
            return CHOLMOD_HIP_INVALID ;
    }
    if (!dG && !dTrace) return CHOLMOD_HIP_OK ;
    const i64 n = P->n, nparts = (n + 255) / 256 ;
    SelInv *S = P->si ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (stream_enter (P, user)) ;
    if (dG && nvalues > 0)
    {
        // every value the factorization does not read: +0.0, in a pass of its own ahead of the writes through src []
        hipLaunchKernelGGL (k_fg_zero_fill, dim3 ((unsigned) ((nvalues + 255) / 256)), dim3 (256), 0, st, (i64) nvalues, dG) ;
        if (n > 0)
            hipLaunchKernelGGL (k_fg_gather_values, dim3 ((unsigned) nparts), dim3 (256), 0, st, n, P->d_Sp, P->d_Si, P->d_vsrc,
                P->d_supermap, P->d_fr, P->d_Ls, (const double *) S->d_Gx, dG) ;
    }
    if (dTrace)
    {
        if (nparts > 0)
            hipLaunchKernelGGL (k_fg_trace_partial, dim3 ((unsigned) nparts), dim3 (256), 0, st, n, P->d_supermap, P->d_fr,
                (const double *) S->d_Gx, S->d_tr) ;
        hipLaunchKernelGGL (k_fg_trace_final, dim3 (1), dim3 (256), 0, st, nparts, (const double *) S->d_tr, dTrace) ;
    }
    return stream_leave (P, user) ;
}

int cholmod_hip_factor_grad_download (cholmod_hip_plan *P, double *Gx_host)
{
    if (sweep_bad_plan (P) || !Gx_host || no_gx (P)) return CHOLMOD_HIP_INVALID ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    if (P->xsize > 0) HIPCHK (hipMemcpy (Gx_host, P->si->d_Gx, (size_t) P->xsize * sizeof (double), hipMemcpyDeviceToHost)) ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_factor_grad_release (cholmod_hip_plan *P)
{
    if (sweep_bad_plan (P)) return CHOLMOD_HIP_INVALID ;
    P->fg_valid = false ;
    if (!P->si) return CHOLMOD_HIP_OK ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    if (P->si->d_tr) (void) hipFree (P->si->d_tr) ;
    P->si->d_tr = nullptr ;
    sweep_release (P, &SelInv::d_Gx) ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_factor_grad_info (cholmod_hip_plan *P, double *out8)
{
    if (sweep_bad_plan (P) || !out8) return CHOLMOD_HIP_INVALID ;
    for (int k = 0 ; k < 8 ; k++) out8 [k] = 0 ;
    SelInv *S = P->si ;
    if (!S) return CHOLMOD_HIP_OK ;
    sweep_info (S, S->fg_clock, out8) ;
    out8 [4] = S->d_Gx ? 8.0 * (double) std::max<i64> (P->xsize, 1) : 0.0 ;
    out8 [5] = S->d_Gx ? 8.0 * (double) (std::max<i64> (S->m_len, 1) + std::max<i64> (S->p_len, 1)) : 0.0 ;
    out8 [6] = P->fg_valid ? 1.0 : 0.0 ;
    return CHOLMOD_HIP_OK ;
}

} // extern "C"
