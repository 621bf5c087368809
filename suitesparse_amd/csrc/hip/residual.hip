// residual.hip -- what a caller does after a device-resident solve, without leaving the device: the residual
// R = B - (A + beta I) X on the resident S = tril (P A P') (cholmod_hip_residual_device) and iterative refinement with it
// (cholmod_hip_refine_device: X += (LL')^-1 R, the sweeps of solve.hip on the workspace the residual was formed in).
// Kernels: residual_kernels.hip.h; the sweeps, the pack / unpack kernels and the workspaces of the solves come through
// solve_internal.hip.h.  No test hook reaches this file: it is built once for both libraries.
#include "residual_kernels.hip.h"
#include "solve_internal.hip.h"

namespace {

// The transposed index of the resident S: its pattern comes back from the device once, the rows are counted and filled
// column by column on the host (so a row lists its entries by ascending column: the order is a function of S alone),
// and the three arrays go up.  Entries above the diagonal and all but the last of equal neighbours are left out, as in
// the column walk of the kernels.  Synchronous, once per uploaded pattern.
static int build_index (cholmod_hip_plan *P)
{
    const i64 n = P->n, nz = P->s_cur_nz ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    std::vector<i64> Sp ((size_t) n + 1), Snz, Si ((size_t) std::max<i64> (nz, 1)) ;
    HIPCHK (hipMemcpy (Sp.data (), P->d_Sp, (n + 1) * sizeof (i64), hipMemcpyDeviceToHost)) ;
    if (P->s_unpacked)
    {
        Snz.resize ((size_t) n) ;
        HIPCHK (hipMemcpy (Snz.data (), P->d_Snz, n * sizeof (i64), hipMemcpyDeviceToHost)) ;
    }
    if (nz) HIPCHK (hipMemcpy (Si.data (), P->d_Si, nz * sizeof (i64), hipMemcpyDeviceToHost)) ;
    std::vector<i64> Tp ((size_t) n + 1, 0) ;
    auto each = [&] (auto &&f)
    {
        for (i64 j = 0 ; j < n ; j++)
        {
            const i64 p0 = Sp [j], pend = P->s_unpacked ? p0 + Snz [j] : Sp [j + 1] ;
            for (i64 p = p0 ; p < pend ; p++)
            {
                const i64 i = Si [p] ;
                if (i <= j || i >= n || (p + 1 < pend && Si [p + 1] == i)) continue ;
                f (i, j, p) ;
            }
        }
    } ;
    each ([&] (i64 i, i64, i64) { Tp [i + 1]++ ; }) ;
    for (i64 i = 0 ; i < n ; i++) Tp [i + 1] += Tp [i] ;
    std::vector<i32> Tj ((size_t) Tp [n]) ;
    std::vector<i64> Tq ((size_t) Tp [n]), next (Tp.begin (), Tp.end () - 1) ;
    each ([&] (i64 i, i64 j, i64 p) { const i64 q = next [i]++ ; Tj [q] = (i32) j ; Tq [q] = p ; }) ;
    for (void *d : {(void *) P->d_rs_Tp, (void *) P->d_rs_Tj, (void *) P->d_rs_Tq}) if (d) (void) hipFree (d) ;
    P->d_rs_Tp = P->d_rs_Tq = nullptr ; P->d_rs_Tj = nullptr ;
    hipError_t e ;
    P->d_rs_Tp = dupload (Tp, e) ; HIPCHK (e) ;
    P->d_rs_Tj = dupload (Tj, e) ; HIPCHK (e) ;
    P->d_rs_Tq = dupload (Tq, e) ; HIPCHK (e) ;
    P->rs_index_valid = true ;
    return CHOLMOD_HIP_OK ;
}

// what both entry points refuse, before any device call.  (The twin of a complex factor is served like a real one: its
// resident phi (S) is a real symmetric matrix, n, ld and the permutation are the twin's.)
static bool bad_plan (const cholmod_hip_plan *P, int perm)
{
    if (!P || P->host_only || P->world > 1) return true ;
    if (perm && !P->d_perm) return true ;                                               // cholmod_hip_set_perm first
    return !P->d_Sp ;                                                                   // no resident matrix (it may have no entry)
}

// workspaces and index; nothing is allocated once they exist
static int rs_ensure (cholmod_hip_plan *P, bool with_factor, bool columns)
{
    HIP_TRY (sd_ensure (P, with_factor, columns)) ;
    const size_t panel = (size_t) P->n * SD_NP * sizeof (double) ;
    if (!P->d_rs_X) HIPCHK (hipMalloc ((void **) &P->d_rs_X, panel)) ;
    if (!P->d_rs_B) HIPCHK (hipMalloc ((void **) &P->d_rs_B, panel)) ;
    return P->rs_index_valid ? CHOLMOD_HIP_OK : build_index (P) ;
}

// One group of right-hand sides in the factor's ordering: `w` of them as [w][n] (columns) or as one panel [n][16].
struct Group {
    const cholmod_hip_plan *P ; hipStream_t st ; bool columns ; int w ;
    i64 count () const { return P->n * (columns ? (i64) w : (i64) SD_NP) ; }
    // R = B - (S + beta I) X (R may be B)
    void residual (const double *X, const double *B, double *R) const
    {
        const i64 n = P->n ;
        const i64 *Snz = P->s_unpacked ? P->d_Snz : nullptr ;
        if (columns)
            hipLaunchKernelGGL (k_rs_columns, dim3 ((unsigned) ((n + 255) / 256), (unsigned) w), dim3 (256), 0, st, n, P->d_Sp, Snz,
                P->d_Si, P->d_Sx, P->d_rs_Tp, P->d_rs_Tj, P->d_rs_Tq, P->cur_beta, X, n, B, n, R, n) ;
        else
            hipLaunchKernelGGL (k_rs_panel, dim3 ((unsigned) ((n + 15) / 16)), dim3 (256), 0, st, n, P->d_Sp, Snz,
                P->d_Si, P->d_Sx, P->d_rs_Tp, P->d_rs_Tj, P->d_rs_Tq, P->cur_beta, X, B, R) ;
    }
    // norms [0 .. w) = column max-norms of R (zeroed by the caller)
    void norms (const double *R, double *out) const
    {
        if (!out) return ;
        const i64 n = P->n ;
        const unsigned nblk = (unsigned) ((n + RS_NORM_ROWS - 1) / RS_NORM_ROWS) ;
        if (columns) hipLaunchKernelGGL (k_rs_norm_columns, dim3 (nblk, (unsigned) w), dim3 (256), 0, st, n, R, n, (unsigned long long *) out) ;
        else hipLaunchKernelGGL (k_rs_norm_panel, dim3 (nblk), dim3 (256), 0, st, n, R, w, (unsigned long long *) out) ;
    }
    // the caller's columns into the group's layout, and back
    int load (const i64 *perm, const double *src, i64 ld, double *dst) const
    {
        if (columns) return sd_move_columns (st, P->n, w, perm, 0, src, ld, dst, P->n) ;
        sd_pack (st, P->n, perm, src, ld, w, dst) ;
        return CHOLMOD_HIP_OK ;
    }
    int store (const i64 *perm, const double *src, double *dst, i64 ld) const
    {
        if (columns) return sd_move_columns (st, P->n, w, perm, 1, src, P->n, dst, ld) ;
        sd_unpack (st, P->n, perm, src, w, dst, ld) ;
        return CHOLMOD_HIP_OK ;
    }
    // W = (LL')^-1 W, then X += W
    void correct (const FrontD *frw, const double *Lw, double *W, double *X) const
    {
        const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;
        if (columns) sd_sweeps_columns (P, 0, frw, Lw, cxs, st, W, P->n, w) ;
        else sd_sweeps_panel (P, 0, frw, Lw, cxs, st, W) ;
        hipLaunchKernelGGL (k_rs_add, dim3 ((unsigned) ((count () + 255) / 256)), dim3 (256), 0, st, count (), X, (const double *) W) ;
    }
} ;

// behind what the caller has enqueued (stream_enter), the norms begin at zero
static int enter (cholmod_hip_plan *P, hipStream_t user, double *dRnorm, i64 nrhs)
{
    HIP_TRY (stream_enter (P, user)) ;
    if (dRnorm) HIPCHK (hipMemsetAsync (dRnorm, 0, nrhs * sizeof (double), P->stream)) ;
    return CHOLMOD_HIP_OK ;
}

} // namespace

int cholmod_hip_residual_device (cholmod_hip_plan *P, int perm, const double *dX, int64_t ldx, const double *dB,
    int64_t ldb, double *dR, int64_t ldr, int64_t nrhs, double *dRnorm, void *stream)
{
    if (bad_plan (P, perm) || !dX || !dB || !dR || dR == dX || nrhs < 0 || ldx < P->n || ldb < P->n || ldr < P->n)
        return CHOLMOD_HIP_INVALID ;
    const i64 n = P->n ;
    if (nrhs == 0 || n == 0) return CHOLMOD_HIP_OK ;
    const bool columns = nrhs < SD_BLOCK_MIN_NRHS ;
    HIP_TRY (rs_ensure (P, false, columns)) ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (enter (P, user, dRnorm, nrhs)) ;
    const i64 *pm = perm ? P->d_perm : nullptr ;
    double *W = P->d_sd_W, *Xp = P->d_rs_X ;
    const i64 step = columns ? nrhs : SD_NP ;
    for (i64 r0 = 0 ; r0 < nrhs ; r0 += step)
    {
        const Group g {P, st, columns, (int) std::min<i64> (step, nrhs - r0)} ;
        HIP_TRY (g.load (pm, dX + r0 * ldx, ldx, Xp)) ;
        HIP_TRY (g.load (pm, dB + r0 * ldb, ldb, W)) ;
        g.residual (Xp, W, W) ;
        g.norms (W, dRnorm ? dRnorm + r0 : nullptr) ;
        HIP_TRY (g.store (pm, W, dR + r0 * ldr, ldr)) ;
    }
    return stream_leave (P, user) ;
}

int cholmod_hip_refine_device (cholmod_hip_plan *P, int perm, const double *dB, int64_t ldb, double *dX, int64_t ldx,
    int64_t nrhs, int steps, double *dRnorm, void *stream)
{
    if (bad_plan (P, perm) || !dB || !dX || nrhs < 0 || steps < 0 || ldb < P->n || ldx < P->n) return CHOLMOD_HIP_INVALID ;
    const i64 n = P->n ;
    if (nrhs == 0 || n == 0) return CHOLMOD_HIP_OK ;
    const double *Lw = whole_factor (P) ;
    const FrontD *frw = whole_fronts (P) ;
    if (steps > 0 && (!Lw || !frw)) return CHOLMOD_HIP_INVALID ;
    const bool columns = nrhs < SD_BLOCK_MIN_NRHS ;
    HIP_TRY (rs_ensure (P, steps > 0, columns)) ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (enter (P, user, dRnorm, nrhs)) ;
    if (steps > 0) refresh_inverses (P, frw, Lw, (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0) ;
    const i64 *pm = perm ? P->d_perm : nullptr ;
    double *W = P->d_sd_W, *Xp = P->d_rs_X, *Bp = P->d_rs_B ;
    const i64 step = columns ? nrhs : SD_NP ;
    for (i64 r0 = 0 ; r0 < nrhs ; r0 += step)
    {
        // the whole iteration in the factor's ordering: B and X pass through Perm once each way
        const Group g {P, st, columns, (int) std::min<i64> (step, nrhs - r0)} ;
        HIP_TRY (g.load (pm, dB + r0 * ldb, ldb, Bp)) ;
        HIP_TRY (g.load (pm, dX + r0 * ldx, ldx, Xp)) ;
        for (int s = 0 ; s < steps ; s++)
        {
            g.residual (Xp, Bp, W) ;
            g.correct (frw, Lw, W, Xp) ;
        }
        if (dRnorm)
        {
            g.residual (Xp, Bp, W) ;
            g.norms (W, dRnorm + r0) ;
        }
        if (steps > 0) HIP_TRY (g.store (pm, Xp, dX + r0 * ldx, ldx)) ;
    }
    return stream_leave (P, user) ;
}
