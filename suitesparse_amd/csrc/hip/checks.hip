// checks.hip -- the read-only passes over a finished factor that is resident on the device: its size-independent invariants
// (cholmod_hip_factor_checks, cholmod_hip_factor_checks_local), its extreme diagonal entries (cholmod_hip_diag_minmax) and
// its even columns (cholmod_hip_download_even_columns).  Kernels: check_kernels.hip.h.  Nothing here touches the
// factorization or its schedule: the kernels read Lx, the front descriptors and the supernode map and write a few doubles of
// scratch.  No test hook reaches this file: it is built once for both libraries.
#include "check_kernels.hip.h"
#include "plan.hip.h"

/* the tasks of the checks over the whole factor (one per CHK_COLS columns of a supernode) and their five doubles of
 * scratch, once per plan */
static int ensure_check_tasks (cholmod_hip_plan *P)
{
    if (P->d_chk) return CHOLMOD_HIP_OK ;
    std::vector<CheckTask> t ;
    for (i64 s = 0 ; s < P->nsuper ; s++)
        for (int c0 = 0 ; c0 < P->fr [s].nscol ; c0 += CHK_COLS) t.push_back (CheckTask {(i32) s, c0}) ;
    hipError_t e ;
    P->d_chk = dupload (t, e) ; HIPCHK (e) ;
    P->nchk = (i64) t.size () ;
    HIPCHK (hipMalloc ((void **) &P->d_chk_out, 5 * sizeof (double))) ;
    return CHOLMOD_HIP_OK ;
}

extern "C" {

int cholmod_hip_factor_checks (cholmod_hip_plan *P, double *out5)
{
    if (!P || P->host_only || !out5) return CHOLMOD_HIP_INVALID ;
    for (int q = 0 ; q < 5 ; q++) out5 [q] = 0 ;
    if (P->nsuper == 0) return CHOLMOD_HIP_OK ;
    HIP_TRY (ensure_check_tasks (P)) ;
    HIPCHK (hipMemsetAsync (P->d_chk_out, 0, 5 * sizeof (double), P->stream)) ;
    // (several ranks: the complete factor exists only after cholmod_hip_gather_factor)
    if (!whole_factor (P) || !whole_fronts (P)) return CHOLMOD_HIP_INVALID ;
    const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;
    CXS_LAUNCH (k_factor_checks, dim3 ((unsigned) P->nchk), dim3 (256), 0, P->stream,
        P->d_chk, whole_fronts (P), whole_factor (P), P->d_chk_out) ;
    HIPCHK (hipGetLastError ()) ;
    HIPCHK (hipMemcpyAsync (out5, P->d_chk_out, 5 * sizeof (double), hipMemcpyDeviceToHost, P->stream)) ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    return CHOLMOD_HIP_OK ;
}

/* Smallest and largest diagonal entry of the resident factor, and the number of NaN / negative ones: what
 * cholmod_l_rcond needs (reference CHOLMOD/Cholesky/cholmod_rcond.c:102-124 walks Lx [psx + jj + jj nsrow] on the host;
 * here L stays in HBM and three numbers come back).  Several ranks: after cholmod_hip_gather_factor. */
int cholmod_hip_diag_minmax (cholmod_hip_plan *P, double *out3)
{
    if (!P || P->host_only || !out3) return CHOLMOD_HIP_INVALID ;
    out3 [0] = out3 [1] = out3 [2] = 0 ;
    if (P->n == 0) return CHOLMOD_HIP_OK ;
    if (!whole_factor (P) || !whole_fronts (P)) return CHOLMOD_HIP_INVALID ;
    HIP_TRY (ensure_check_tasks (P)) ;     // (d_chk_out: five doubles of scratch)
    unsigned long long seed [3] ;
    const double inf = INFINITY, zero = 0.0 ;
    memcpy (&seed [0], &inf, 8) ; memcpy (&seed [1], &zero, 8) ; seed [2] = 0 ;
    HIPCHK (hipMemcpyAsync (P->d_chk_out, seed, sizeof (seed), hipMemcpyHostToDevice, P->stream)) ;
    const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;
    CXS_LAUNCH (k_diag_minmax, dim3 ((unsigned) ((P->n + 255) / 256)), dim3 (256), 0, P->stream,
        P->n, P->d_supermap, whole_fronts (P), whole_factor (P), (unsigned long long *) P->d_chk_out) ;
    HIPCHK (hipGetLastError ()) ;
    HIPCHK (hipMemcpyAsync (seed, P->d_chk_out, sizeof (seed), hipMemcpyDeviceToHost, P->stream)) ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    memcpy (&out3 [0], &seed [0], 8) ; memcpy (&out3 [1], &seed [1], 8) ; out3 [2] = (double) seed [2] ;
    return CHOLMOD_HIP_OK ;
}

/* The same invariants over the fronts THIS rank answers for in a distributed factor (every front
 * belongs to the first rank of its group), read from the rank's own part of L -- no gathered copy
 * needed: the sums of out5 over all ranks are the invariants of the complete factor.  (One rank:
 * the same numbers as cholmod_hip_factor_checks.) */
int cholmod_hip_factor_checks_local (cholmod_hip_plan *P, double *out5)
{
    if (!P || P->host_only || !out5) return CHOLMOD_HIP_INVALID ;
    for (int q = 0 ; q < 5 ; q++) out5 [q] = 0 ;
    if (P->nsuper == 0) return CHOLMOD_HIP_OK ;
    if (!P->d_Lx) return CHOLMOD_HIP_INVALID ;          // (released by a host-staged gather: the gathered factor is what there is)
    std::vector<CheckTask> t ;
    for (i64 s = 0 ; s < P->nsuper ; s++)
        if (P->lpx [s] >= 0 && (P->fr [s].own_w || P->rank == P->grp0 [s]))
            for (int c0 = 0 ; c0 < P->fr [s].nscol ; c0 += CHK_COLS)
                if (col_owned (P->fr [s], c0)) t.push_back (CheckTask {(i32) s, c0}) ;       // (a slab is a multiple of CHK_COLS columns)
    if (t.empty ()) return CHOLMOD_HIP_OK ;
    hipError_t e ;
    CheckTask *dt = dupload (t, e) ; HIPCHK (e) ;
    double *dout = nullptr ;
    if (hipMalloc ((void **) &dout, 5 * sizeof (double)) != hipSuccess) { (void) hipGetLastError () ; (void) hipFree (dt) ; return CHOLMOD_HIP_OUT_OF_MEMORY ; }
    (void) hipMemsetAsync (dout, 0, 5 * sizeof (double), P->stream) ;
    const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;
    CXS_LAUNCH (k_factor_checks, dim3 ((unsigned) t.size ()), dim3 (256), 0, P->stream, dt, P->d_fr, P->d_Lx, dout) ;
    e = hipGetLastError () ;
    if (e == hipSuccess) e = hipMemcpyAsync (out5, dout, 5 * sizeof (double), hipMemcpyDeviceToHost, P->stream) ;
    if (e == hipSuccess) e = hipStreamSynchronize (P->stream) ;
    (void) hipFree (dt) ; (void) hipFree (dout) ;
    return e == hipSuccess ? CHOLMOD_HIP_OK : CHOLMOD_HIP_GPU_PROBLEM ;
}

int cholmod_hip_download_even_columns (cholmod_hip_plan *P, double *out_host)
{
    if (!P || P->host_only || !out_host) return CHOLMOD_HIP_INVALID ;
    if (P->nsuper == 0 || P->xsize == 0) return CHOLMOD_HIP_OK ;
    if (P->flags & CHOLMOD_HIP_CX_STORAGE)
    {
        // the factor is stored as its even columns: it IS the interleaved complex factor
        if (!whole_factor (P)) return CHOLMOD_HIP_INVALID ;
        HIPCHK (hipMemcpy (out_host, whole_factor (P), (size_t) P->xsize * sizeof (double), hipMemcpyDeviceToHost)) ;
        return CHOLMOD_HIP_OK ;
    }
    HIP_TRY (ensure_check_tasks (P)) ;
    double *tmp = nullptr ;
    const size_t bytes = (size_t) (P->xsize / 2) * sizeof (double) ;
    if (hipMalloc ((void **) &tmp, bytes) != hipSuccess) { (void) hipGetLastError () ; return CHOLMOD_HIP_OUT_OF_MEMORY ; }
    if (!whole_factor (P)) { (void) hipFree (tmp) ; return CHOLMOD_HIP_INVALID ; }
    hipLaunchKernelGGL (k_even_columns, dim3 ((unsigned) P->nchk), dim3 (256), 0, P->stream,
        P->d_chk, whole_fronts (P), whole_factor (P), tmp) ;
    hipError_t e = hipGetLastError () ;
    if (e == hipSuccess) e = hipMemcpyAsync (out_host, tmp, bytes, hipMemcpyDeviceToHost, P->stream) ;
    if (e == hipSuccess) e = hipStreamSynchronize (P->stream) ;
    (void) hipFree (tmp) ;
    return e == hipSuccess ? CHOLMOD_HIP_OK : CHOLMOD_HIP_GPU_PROBLEM ;
}

} // extern "C"
