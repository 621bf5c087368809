// grad.hip -- what backpropagation through a device-resident factorization needs, without leaving the device: the
// gradient with respect to the values of A sampled on the pattern of the resident S (cholmod_hip_values_grad_device: for
// X = (A + beta I)^-1 B and Lambda = (A + beta I)^-1 gX it is -(Lambda X' + X Lambda') on A's entries) and log det
// (A + beta I) of the resident factor as a device scalar (cholmod_hip_logdet_device; its gradient is the selected
// inverse, selinv.hip).  Where the values of the resident S are computed from the caller's by a product map (S = tril (A A')),
// the same two gradients with respect to the values of the value map go into a scratch of the plan and through the
// transpose of the product kernel to the caller's values (cholmod_hip_product_values_grad_device,
// cholmod_hip_product_logdet_grad_device).  Kernels: grad_kernels.hip.h; the pack kernel of the panels comes through
// solve_internal.hip.h.  No test hook reaches this file: it is built once for both libraries.
#include "grad_kernels.hip.h"
#include "solve_internal.hip.h"

struct Grad {
    double *d_U = nullptr, *d_V = nullptr ;     // the panels [n][16] of U and V in the factor's ordering
    double *d_part = nullptr ;                  // partial sums of the log-determinant, one per 256 columns
    i32 *d_col = nullptr ; i64 col_cap = 0 ;    // the column of every entry of the resident S (P->gr_index_valid)
} ;

namespace {

static int alloc (double **into, i64 count) { return *into ? CHOLMOD_HIP_OK : device_alloc (into, count) ; }

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
        HIP_TRY (device_alloc (&g->d_col, nz)) ;
        g->col_cap = std::max<i64> (nz, 1) ;
    }
    if (nz > 0)
        hipLaunchKernelGGL (k_gr_column_index, dim3 ((unsigned) ((nz + 255) / 256)), dim3 (256), 0, P->stream, P->n, nz, P->d_Sp, g->d_col) ;
    P->gr_index_valid = true ;
    return CHOLMOD_HIP_OK ;
}

// `panels`: the two panels; `partials`: the buffer of the log-determinant.  Nothing is allocated once they exist.
static int ensure (cholmod_hip_plan *P, bool panels, bool partials)
{
    if (!P->gr) P->gr = new (std::nothrow) Grad ;
    Grad *g = P->gr ;
    if (!g) return CHOLMOD_HIP_OUT_OF_MEMORY ;
    if (panels)
    {
        HIP_TRY (alloc (&g->d_U, P->n * GR_NP)) ;
        HIP_TRY (alloc (&g->d_V, P->n * GR_NP)) ;
    }
    if (partials) HIP_TRY (alloc (&g->d_part, (P->n + 255) / 256)) ;
    return CHOLMOD_HIP_OK ;
}

static unsigned blocks_of (i64 count) { return (unsigned) ((count + 255) / 256) ; }

// The sampled product of cholmod_hip_values_grad_device into dG, nvalues doubles in the order of the value map, enqueued on
// the engine stream: +0.0 everywhere first, then the entries the resident S reads.  The workspaces (ensure, ensure_index)
// exist; nvalues > 0.
static void sampled_product (cholmod_hip_plan *P, int perm, double alpha, const double *dU, i64 ldu, const double *dV, i64 ldv,
    i64 nrhs, double *dG, i64 nvalues)
{
    const i64 n = P->n, nz = P->s_cur_nz ;
    const i32 *col = P->gr->d_col ;
    hipStream_t st = P->stream ;
    // every value the factorization does not read: +0.0, in a pass of its own ahead of the writes through src []
    hipLaunchKernelGGL (k_gr_zero_fill, dim3 (blocks_of (nvalues)), dim3 (256), 0, st, nvalues, dG) ;
    const i64 *pm = perm ? P->d_perm : nullptr ;
    if (nz > 0 && nrhs > 0 && nrhs < SD_BLOCK_MIN_NRHS)
        hipLaunchKernelGGL (k_gr_columns, dim3 (blocks_of (nz)), dim3 (256), 0, st, n, nz, P->d_Sp, P->d_Si, col, P->d_vsrc, pm,
            dU, ldu, dV, ldv, (int) nrhs, alpha, dG) ;
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
}

// ---- through a product map ---------------------------------------------------------------------------------------------------

// what the two product entry points ask of the plan beyond real_device_plan: the value map of the current resident packed S, and a
// product map from navalues values onto it
static bool bad_product_plan (const cholmod_hip_plan *P, i64 navalues)
{
    if (!P->d_Sp || !P->d_vsrc || P->s_unpacked || P->vsrc_nz != P->s_cur_nz) return true ;
    return !P->pm_set || navalues != P->pm_na ;
}

template <typename T> static int upload (T **into, const std::vector<T> &v)
{
    hipError_t e = hipMalloc ((void **) into, std::max<size_t> (v.size (), 1) * sizeof (T)) ;
    if (e == hipSuccess && !v.empty ()) e = hipMemcpy (*into, v.data (), v.size () * sizeof (T), hipMemcpyHostToDevice) ;
    return e == hipSuccess ? CHOLMOD_HIP_OK : alloc_failure (e) ;
}

// The transposed product map and the scratch of vals_n doubles, built by the first gradient call after a
// cholmod_hip_set_product_map (a caller who never differentiates pays nothing) and freed with the map (values.hip:
// drop_product_map).  The forward lists come down once (no kernel writes them); one stable counting pass on the host --
// pairs in ascending p, the ia half of a pair before its ib half, so that the order of a list is a function of the map
// alone --, a counting sort of the values into the kernel's three length classes (inside a class they keep their order),
// and the result goes up: the residual's transposed index is built the same way (residual.hip).
static int ensure_transposed (cholmod_hip_plan *P)
{
    if (P->pt_built) return CHOLMOD_HIP_OK ;
    const i64 nc = P->vals_n, na = P->pm_na ;
    if (na > INT32_MAX || nc > INT32_MAX) return CHOLMOD_HIP_TOO_LARGE ;
    std::vector<i64> cp ((size_t) nc + 1, 0) ;
    HIPCHK (hipMemcpy (cp.data (), P->d_pm_cp, cp.size () * sizeof (i64), hipMemcpyDeviceToHost)) ;
    const i64 np = cp [nc] ;
    std::vector<i64> ia ((size_t) np), ib ((size_t) np) ;
    if (np > 0)
    {
        HIPCHK (hipMemcpy (ia.data (), P->d_pm_ia, (size_t) np * sizeof (i64), hipMemcpyDeviceToHost)) ;
        HIPCHK (hipMemcpy (ib.data (), P->d_pm_ib, (size_t) np * sizeof (i64), hipMemcpyDeviceToHost)) ;
    }
    std::vector<i64> tp ((size_t) na + 1, 0) ;
    for (i64 p = 0 ; p < np ; p++) { tp [ia [p] + 1]++ ; tp [ib [p] + 1]++ ; }
    for (i64 q = 0 ; q < na ; q++) tp [q + 1] += tp [q] ;
    std::vector<i32> tc ((size_t) (2 * np)), tpart ((size_t) (2 * np)) ;
    {
        std::vector<i64> next (tp.begin (), tp.end () - 1) ;
        for (i64 c = 0 ; c < nc ; c++)
            for (i64 p = cp [c] ; p < cp [c + 1] ; p++)
            {
                i64 h = next [ia [p]]++ ;
                tc [h] = (i32) c ; tpart [h] = (i32) ib [p] ;
                h = next [ib [p]]++ ;
                tc [h] = (i32) c ; tpart [h] = (i32) ia [p] ;
            }
    }
    auto cls = [&] (i64 q) { const i64 len = tp [q + 1] - tp [q] ; return len <= PM_LEN1 ? 0 : len <= PM_LEN16 ? 1 : 2 ; } ;
    i64 first [4] = {0, 0, 0, 0} ;
    for (i64 q = 0 ; q < na ; q++) first [cls (q) + 1]++ ;
    for (int k = 0 ; k < 3 ; k++) first [k + 1] += first [k] ;
    std::vector<i32> order ((size_t) na) ;
    {
        i64 next [3] = {first [0], first [1], first [2]} ;
        for (i64 q = 0 ; q < na ; q++) order [next [cls (q)]++] = (i32) q ;
    }
    int rc = upload (&P->d_pt_ptr, tp) ;
    if (rc == CHOLMOD_HIP_OK) rc = upload (&P->d_pt_c, tc) ;
    if (rc == CHOLMOD_HIP_OK) rc = upload (&P->d_pt_partner, tpart) ;
    if (rc == CHOLMOD_HIP_OK) rc = upload (&P->d_pt_order, order) ;
    if (rc == CHOLMOD_HIP_OK) rc = alloc (&P->d_pt_gvals, nc) ;
    if (rc != CHOLMOD_HIP_OK)
    {
        for (void *d : {(void *) P->d_pt_ptr, (void *) P->d_pt_c, (void *) P->d_pt_partner, (void *) P->d_pt_order, (void *) P->d_pt_gvals})
            if (d) (void) hipFree (d) ;
        P->d_pt_ptr = nullptr ; P->d_pt_c = P->d_pt_partner = P->d_pt_order = nullptr ; P->d_pt_gvals = nullptr ;
        return rc ;
    }
    for (int k = 0 ; k < 4 ; k++) P->pt_class [k] = first [k] ;
    P->pt_built = true ;
    return CHOLMOD_HIP_OK ;
}

// dGa [q] = the chain rule through the product map applied to the scratch, for every q < pm_na, on the engine stream
static void product_grad (cholmod_hip_plan *P, const double *dA, double *dGa)
{
    const i64 *c = P->pt_class ;
#define PT_LAUNCH(G_, K_) if (c [K_ + 1] > c [K_]) \
        hipLaunchKernelGGL (k_product_grad<G_>, dim3 (blocks_of ((c [K_ + 1] - c [K_]) * G_)), dim3 (256), 0, P->stream, \
            c [K_ + 1] - c [K_], P->d_pt_order + c [K_], P->d_pt_ptr, P->d_pt_c, P->d_pt_partner, (const double *) P->d_pt_gvals, dA, dGa)
    PT_LAUNCH (1, 0) ; PT_LAUNCH (16, 1) ; PT_LAUNCH (64, 2) ;
#undef PT_LAUNCH
}

} // namespace

void grad_free (cholmod_hip_plan *P)
{
    Grad *g = P->gr ;
    P->gr = nullptr ;
    if (!g) return ;
    P->gr_index_valid = false ;
    for (void *d : {(void *) g->d_U, (void *) g->d_V, (void *) g->d_part, (void *) g->d_col}) if (d) (void) hipFree (d) ;
    delete g ;
}

extern "C" {

int cholmod_hip_values_grad_device (cholmod_hip_plan *P, int perm, double alpha, const double *dU, int64_t ldu,
    const double *dV, int64_t ldv, int64_t nrhs, double *dG, int64_t nvalues, void *stream)
{
    if (!real_device_plan (P) || !dU || !dV || !dG || nrhs < 0 || ldu < P->n || ldv < P->n) return CHOLMOD_HIP_INVALID ;
    // the value map of the current resident packed S, and values that are given, not computed
    if (!P->d_Sp || !P->d_vsrc || P->s_unpacked || P->vsrc_nz != P->s_cur_nz || nvalues != P->vals_n || P->pm_set)
        return CHOLMOD_HIP_INVALID ;
    if (perm && !P->d_perm) return CHOLMOD_HIP_INVALID ;                                // cholmod_hip_set_perm first
    if (P->n == 0 || nvalues == 0) return CHOLMOD_HIP_OK ;
    HIP_TRY (ensure (P, nrhs >= SD_BLOCK_MIN_NRHS, false)) ;
    HIP_TRY (ensure_index (P)) ;
    hipStream_t user = (hipStream_t) stream ;
    HIP_TRY (stream_enter (P, user)) ;
    sampled_product (P, perm, alpha, dU, (i64) ldu, dV, (i64) ldv, (i64) nrhs, dG, (i64) nvalues) ;
    return stream_leave (P, user) ;
}

int cholmod_hip_logdet_device (cholmod_hip_plan *P, double *dOut, void *stream)
{
    if (!real_device_plan (P) || !dOut) return CHOLMOD_HIP_INVALID ;
    if (P->factor_state != 1 || !P->d_Lx) return CHOLMOD_HIP_INVALID ;  // no numeric factor on the device, or one that is not positive definite
    HIP_TRY (ensure (P, false, true)) ;
    const i64 n = P->n, nparts = (n + 255) / 256 ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (stream_enter (P, user)) ;
    if (nparts > 0)
        hipLaunchKernelGGL (k_gr_logdet_partial, dim3 ((unsigned) nparts), dim3 (256), 0, st, n, P->d_supermap, P->d_fr, P->d_Lx, P->gr->d_part) ;
    hipLaunchKernelGGL (k_gr_logdet_final, dim3 (1), dim3 (256), 0, st, nparts, (const double *) P->gr->d_part, dOut) ;
    return stream_leave (P, user) ;
}

int cholmod_hip_product_values_grad_device (cholmod_hip_plan *P, int perm, double alpha, const double *dU, int64_t ldu,
    const double *dV, int64_t ldv, int64_t nrhs, const double *dA, double *dGa, int64_t navalues, void *stream)
{
    if (!real_device_plan (P) || !dU || !dV || !dA || !dGa || nrhs < 0 || ldu < P->n || ldv < P->n) return CHOLMOD_HIP_INVALID ;
    if (bad_product_plan (P, navalues)) return CHOLMOD_HIP_INVALID ;
    if (perm && !P->d_perm) return CHOLMOD_HIP_INVALID ;                                // cholmod_hip_set_perm first
    if (P->n == 0 || navalues == 0) return CHOLMOD_HIP_OK ;
    hipStream_t user = (hipStream_t) stream ;
    if (nrhs == 0 || P->vals_n == 0)                    // nothing to sample: the gradient is +0.0 whatever dA holds
    {
        HIP_TRY (ensure (P, false, false)) ;
        HIP_TRY (stream_enter (P, user)) ;
        hipLaunchKernelGGL (k_gr_zero_fill, dim3 (blocks_of (navalues)), dim3 (256), 0, P->stream, (i64) navalues, dGa) ;
        return stream_leave (P, user) ;
    }
    HIP_TRY (ensure (P, nrhs >= SD_BLOCK_MIN_NRHS, false)) ;
    HIP_TRY (ensure_index (P)) ;
    HIP_TRY (ensure_transposed (P)) ;
    HIP_TRY (stream_enter (P, user)) ;
    sampled_product (P, perm, alpha, dU, (i64) ldu, dV, (i64) ldv, (i64) nrhs, P->d_pt_gvals, P->vals_n) ;
    product_grad (P, dA, dGa) ;
    return stream_leave (P, user) ;
}

int cholmod_hip_product_logdet_grad_device (cholmod_hip_plan *P, const double *dA, double *dGa, int64_t navalues, void *stream)
{
    if (!real_device_plan (P) || !dA || !dGa || bad_product_plan (P, navalues)) return CHOLMOD_HIP_INVALID ;
    // a current selected inverse of a positive definite factor (cholmod_hip_selinv_device first)
    if (P->factor_state != 1 || !P->si_valid || !P->si) return CHOLMOD_HIP_INVALID ;
    if (P->n == 0 || navalues == 0) return CHOLMOD_HIP_OK ;
    hipStream_t user = (hipStream_t) stream ;
    HIP_TRY (ensure (P, false, false)) ;
    HIP_TRY (ensure_index (P)) ;
    HIP_TRY (ensure_transposed (P)) ;
    HIP_TRY (stream_enter (P, user)) ;
    // Z at the values S reads, once on the diagonal and twice off it; +0.0, never the gather's NaN, at every other value
    hipLaunchKernelGGL (k_gr_zero_fill, dim3 (blocks_of (std::max<i64> (P->vals_n, 1))), dim3 (256), 0, P->stream, P->vals_n, P->d_pt_gvals) ;
    selinv_gather_logdet_grad (P, P->gr->d_col, P->d_pt_gvals, P->stream) ;
    product_grad (P, dA, dGa) ;
    return stream_leave (P, user) ;
}

} // extern "C"
