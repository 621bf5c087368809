// schur.hip -- the Schur complement onto the last m variables of the factor's ordering, from the factor that is resident
// on the device: Sc = L22 L22' with L22 = L [n-m:, n-m:] (cholmod_hip_schur_device, which also hands out L22 itself, the
// Cholesky factor of Sc), and the products L22 V and L22' V that turn the L and L' sweeps of solve.hip into the condensed
// right-hand side and the back-expansion (cholmod_hip_trailing_multiply_device).  Kernels: schur_kernels.hip.h.  Nothing
// here touches the factorization, its schedule or its workspaces: the kernels read Lx, the row lists, the front
// descriptors and the supernode map, which are on the device already, and write the caller's arrays only: nothing is
// allocated here.  No test hook reaches this file: it is built once for both libraries.
#include "schur_kernels.hip.h"
#include "selinv_internal.hip.h"

extern "C" {

int cholmod_hip_schur_device (cholmod_hip_plan *P, int64_t m, double *dS, int64_t lds, double *dF, int64_t ldf, void *stream)
{
    if (sweep_bad_plan (P) || m < 0 || m > P->n || (!dS && !dF)) return CHOLMOD_HIP_INVALID ;
    if ((dS && lds < m) || (dF && ldf < m)) return CHOLMOD_HIP_INVALID ;
    if (m == 0) return CHOLMOD_HIP_OK ;
    const i64 n = P->n ;
    const i64 nt = (m + 63) / 64, ntiles = nt * (nt + 1) / 2 ;
    if (ntiles > INT32_MAX) return CHOLMOD_HIP_INVALID ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (stream_enter (P, user)) ;
    if (dS)
        hipLaunchKernelGGL (k_schur_tile, dim3 ((unsigned) ntiles), dim3 (256), 0, st, n, (i64) m, (int) nt,
            (int) P->supermap [n - m], (int) P->nsuper, P->d_fr, P->d_Ls, P->d_Lx, dS, (i64) lds) ;
    if (dF)
        hipLaunchKernelGGL (k_schur_factor, dim3 ((unsigned) m), dim3 (256), 0, st, n, (i64) m, P->d_supermap, P->d_fr, P->d_Ls,
            P->d_Lx, dF, (i64) ldf) ;
    return stream_leave (P, user) ;
}

int cholmod_hip_trailing_multiply_device (cholmod_hip_plan *P, int64_t m, int trans, const double *dV, int64_t ldv, double *dOut,
    int64_t ldo, int64_t nrhs, void *stream)
{
    if (sweep_bad_plan (P) || m < 0 || m > P->n || nrhs < 0 || !dV || !dOut || dOut == dV || ldv < m || ldo < m)
        return CHOLMOD_HIP_INVALID ;
    if (m == 0 || nrhs == 0) return CHOLMOD_HIP_OK ;
    const i64 n = P->n ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (stream_enter (P, user)) ;
    if (trans)
        hipLaunchKernelGGL (k_schur_mult_t, dim3 ((unsigned) m), dim3 (256), 0, st, n, (i64) m, P->d_supermap, P->d_fr, P->d_Ls,
            P->d_Lx, dV, (i64) ldv, dOut, (i64) ldo, (i64) nrhs) ;
    else
    {
        hipLaunchKernelGGL (k_schur_clear, dim3 ((unsigned) ((m * nrhs + 255) / 256)), dim3 (256), 0, st, (i64) m, (i64) nrhs,
            dOut, (i64) ldo) ;
        hipLaunchKernelGGL (k_schur_mult_n, dim3 ((unsigned) m), dim3 (256), 0, st, n, (i64) m, P->d_supermap, P->d_fr, P->d_Ls,
            P->d_Lx, dV, (i64) ldv, dOut, (i64) ldo, (i64) nrhs) ;
    }
    return stream_leave (P, user) ;
}

} // extern "C"
