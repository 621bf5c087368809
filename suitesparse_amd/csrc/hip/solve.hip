// solve.hip -- the triangular solves with the device-resident factor: cholmod_hip_solve (right-hand sides on the host),
// cholmod_hip_solve_device (right-hand sides in HBM) and cholmod_hip_set_perm.  Both walk the plan's level schedule
// (plan_build.hip: sv_ptr, sb_launch, sb_commit_launch) through one driver, solve_sweeps; what differs is the kernel
// family a step launches (solve_kernels.hip.h).  No test hook reaches this file: it is built once for both libraries.
#include "solve_kernels.hip.h"
#include "solve_internal.hip.h"

namespace {

using SbLaunch = cholmod_hip_plan::SbLaunch ;

// The seven steps of the sweeps with the kernels that take one right-hand side at a time: nrhs columns x [nrhs][ldx],
// in place; d_solved is the side vector of the forward walk over a big supernode, d_sv_acc the accumulators of the
// backward one.
struct ColumnKernels {
    const cholmod_hip_plan *P ; const FrontD *frw ; const double *Lw ; hipStream_t st ;
    double *x ; i64 ldx ; int nrhs ; bool cxs ;
    void lsolve (const SolveTask *t, int nf) const
    {
        CXS_LAUNCH (k_lsolve, dim3 (nf), dim3 (256), 0, st, t, frw, P->d_Ls, Lw, x, ldx, nrhs) ;
    }
    void fwd_diag (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_solve_fwd_diag, dim3 (B.ntasks), dim3 (256), 0, st,
            P->d_sb_tasks + B.first, frw, Lw, P->d_winv, x, ldx, nrhs, P->d_solved) ;
    }
    void fwd_apply (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_solve_fwd_apply, dim3 (B.grid), dim3 (256), 0, st,
            P->d_sb_tasks + B.first, (int) B.ntasks, frw, P->d_Ls, Lw, x, ldx, nrhs, P->d_solved) ;
    }
    void commit (const SbLaunch &C) const
    {
        hipLaunchKernelGGL (k_solve_commit, dim3 (C.grid), dim3 (256), 0, st,
            P->d_sb_commit + C.first, (int) C.ntasks, frw, x, ldx, nrhs, P->d_solved) ;
    }
    void bwd_apply (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_solve_bwd_apply, dim3 (B.grid), dim3 (256), 0, st,
            P->d_sb_tasks + B.first, (int) B.ntasks, frw, P->d_Ls, Lw, x, ldx, nrhs, P->d_sv_acc) ;
    }
    void bwd_diag (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_solve_bwd_diag, dim3 (B.ntasks), dim3 (256), 0, st,
            P->d_sb_tasks + B.first, frw, Lw, P->d_winv, x, ldx, nrhs, P->d_sv_acc) ;
    }
    void ltsolve (const SolveTask *t, int nf) const
    {
        CXS_LAUNCH (k_ltsolve, dim3 (nf), dim3 (256), 0, st, t, frw, P->d_Ls, Lw, x, ldx, nrhs) ;
    }
} ;

// ... and with the 16-wide ones: a panel of up to 16 right-hand sides, in place on W [n][16], L read once.  They update W
// as they go, so there is nothing to commit.  cxs: L is a complex factor in its own storage (W is the twin's either way).
struct PanelKernels {
    const cholmod_hip_plan *P ; const FrontD *frw ; const double *Lw ; hipStream_t st ;
    double *W ; bool cxs ;
    void lsolve (const SolveTask *t, int nf) const
    {
        CXS_LAUNCH (k_sd_lsolve, dim3 (nf), dim3 (256), 0, st, t, frw, P->d_Ls, Lw, W) ;
    }
    void fwd_diag (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_sd_fwd_diag, dim3 (B.ntasks), dim3 (256), 0, st, P->d_sb_tasks + B.first, frw, Lw, P->d_winv, W) ;
    }
    void fwd_apply (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_sd_fwd_apply, dim3 (B.grid), dim3 (256), 0, st,
            P->d_sb_tasks + B.first, (int) B.ntasks, frw, P->d_Ls, Lw, W) ;
    }
    void commit (const SbLaunch &) const {}
    void bwd_apply (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_sd_bwd_apply, dim3 (B.grid), dim3 (256), 0, st,
            P->d_sb_tasks + B.first, (int) B.ntasks, frw, P->d_Ls, Lw, W, P->d_sd_acc) ;
    }
    void bwd_diag (const SbLaunch &B) const
    {
        CXS_LAUNCH (k_sd_bwd_diag, dim3 (B.ntasks), dim3 (256), 0, st,
            P->d_sb_tasks + B.first, frw, Lw, P->d_winv, W, P->d_sd_acc) ;
    }
    void ltsolve (const SolveTask *t, int nf) const
    {
        CXS_LAUNCH (k_sd_ltsolve, dim3 (nf), dim3 (256), 0, st, t, frw, P->d_Ls, Lw, W) ;
    }
} ;

// The schedule of a solve (which: 0 = L then L', 1 = L only, 2 = L' only).  Forward, level by level from the leaves: the
// supernodes one workgroup handles whole, then the big ones block by block (diagonal block, then the rows below it),
// then their side vectors into x.  Backward, the same in reverse.
template <class Kernels>
static void solve_sweeps (const cholmod_hip_plan *P, int which, const Kernels &k)
{
    if (which == 0 || which == 1)
    {
        for (int l = 0 ; l < P->nlevels ; l++)
        {
            int nf = P->sv_ptr [l+1] - P->sv_ptr [l] ;
            if (nf) k.lsolve (P->d_sv + P->sv_ptr [l], nf) ;
            for (int q = P->sb_lvl_ptr [l] ; q < P->sb_lvl_ptr [l+1] ; q++)
            {
                const auto &B = P->sb_launch [q] ;
                k.fwd_diag (B) ;
                if (B.grid > 0) k.fwd_apply (B) ;
            }
            const auto &Cm = P->sb_commit_launch [l] ;
            if (Cm.ntasks) k.commit (Cm) ;
        }
    }
    if (which == 0 || which == 2)
    {
        for (int l = P->nlevels - 1 ; l >= 0 ; l--)
        {
            for (int q = P->sb_lvl_ptr [l+1] - 1 ; q >= P->sb_lvl_ptr [l] ; q--)
            {
                const auto &B = P->sb_launch [q] ;
                if (B.grid > 0) k.bwd_apply (B) ;
                k.bwd_diag (B) ;
            }
            int nf = P->sv_ptr [l+1] - P->sv_ptr [l] ;
            if (nf) k.ltsolve (P->d_sv + P->sv_ptr [l], nf) ;
        }
    }
}

// frees *p and allocates `count` doubles in its place, zeroed if asked
static int regrow (double **p, i64 count, bool zero)
{
    if (*p) (void) hipFree (*p) ;
    *p = nullptr ;
    HIPCHK (hipMalloc ((void **) p, count * sizeof (double))) ;
    if (zero) HIPCHK (hipMemset (*p, 0, count * sizeof (double))) ;
    return CHOLMOD_HIP_OK ;
}

// Workspace of the walk over the big supernodes (none: nothing to do), shared by both entry points: the task lists and
// the room of the 64 x 64 inverses once per plan; at least `solved` doubles of side vector and accumulators for
// `acc_nrhs` right-hand sides (the per-column kernels), grown when a call needs more; the accumulators of the 16-wide
// backward walk, once, if `panel_acc`.  Every accumulator is zero between solves.
static int solve_workspace (cholmod_hip_plan *P, i64 solved, i64 acc_nrhs, bool panel_acc)
{
    if (P->inv_tasks.empty ()) return CHOLMOD_HIP_OK ;
    if (!P->d_winv)
    {
        hipError_t e ;
        HIPCHK (hipMalloc ((void **) &P->d_winv, P->inv_tasks.size () * 8192 * sizeof (double))) ;
        P->d_inv_tasks = dupload (P->inv_tasks, e) ; HIPCHK (e) ;
        P->d_sb_tasks = dupload (P->sb_tasks, e) ; HIPCHK (e) ;
        P->d_sb_commit = dupload (P->sb_commit, e) ; HIPCHK (e) ;
        P->winv_valid = false ;
    }
    if (solved > P->solved_cap)
    {
        P->solved_cap = solved ;
        HIP_TRY (regrow (&P->d_solved, solved, false)) ;
    }
    const i64 acc = (i64) P->sb_max_tasks * SOLVE_SB * acc_nrhs ;
    if (acc > P->sv_acc_cap)
    {
        P->sv_acc_cap = acc ;
        HIP_TRY (regrow (&P->d_sv_acc, acc, true)) ;
    }
    if (panel_acc && !P->d_sd_acc)
        return regrow (&P->d_sd_acc, (i64) std::max (P->sb_max_tasks, 1) * SOLVE_SB * SD_NP, true) ;
    return CHOLMOD_HIP_OK ;
}

} // namespace

namespace sship {

// the explicit inverses of the diagonal blocks of the big supernodes follow the factor: recomputed, on the engine
// stream, by the first solve after it changed
void refresh_inverses (cholmod_hip_plan *P, const FrontD *frw, const double *Lw, bool cxs)
{
    if (P->inv_tasks.empty () || P->winv_valid) return ;
    CXS_LAUNCH (k_diag_inv64, dim3 ((unsigned) P->inv_tasks.size ()), dim3 (64), 0, P->stream,
        P->d_inv_tasks, frw, Lw, P->d_winv) ;
    P->winv_valid = true ;
}

} // namespace sship

int cholmod_hip_solve (cholmod_hip_plan *P, int which, double *X, int64_t nrhs, int64_t ldx)
{
    if (!P || P->host_only || !X || nrhs < 0 || ldx < P->n) return CHOLMOD_HIP_INVALID ;
    if (nrhs == 0 || P->n == 0) return CHOLMOD_HIP_OK ;
    const double *Lw = whole_factor (P) ;
    const FrontD *frw = whole_fronts (P) ;
    if (!Lw || !frw) return CHOLMOD_HIP_INVALID ;  // several ranks: cholmod_hip_gather_factor first
    const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;
    i64 need = ldx * nrhs ;
    if (need > P->x_cap)
    {
        if (P->d_X) (void) hipFree (P->d_X) ;
        P->d_X = nullptr ;
        HIPCHK (hipMalloc ((void **) &P->d_X, need * sizeof (double))) ;
        P->x_cap = need ;
    }
    hipStream_t st = P->stream ;
    HIP_TRY (solve_workspace (P, need, nrhs, false)) ;
    refresh_inverses (P, frw, Lw, cxs) ;
    HIPCHK (hipMemcpyAsync (P->d_X, X, need * sizeof (double), hipMemcpyHostToDevice, st)) ;
    HIPCHK (hipEventRecord (P->ev0, st)) ;
    solve_sweeps (P, which, ColumnKernels {P, frw, Lw, st, P->d_X, (i64) ldx, (int) nrhs, cxs}) ;
    HIPCHK (hipGetLastError ()) ;
    HIPCHK (hipEventRecord (P->ev1, st)) ;
    HIPCHK (hipMemcpyAsync (X, P->d_X, need * sizeof (double), hipMemcpyDeviceToHost, st)) ;
    HIPCHK (hipStreamSynchronize (st)) ;
    {
        float ms = 0 ;
        if (hipEventElapsedTime (&ms, P->ev0, P->ev1) == hipSuccess) P->solve_seconds = 1e-3 * ms ;
    }
    return CHOLMOD_HIP_OK ;
}

// ---- solves whose right-hand sides live in HBM ---------------------------------------------------------------------------

int cholmod_hip_set_perm (cholmod_hip_plan *P, const int64_t *Perm)
{
    if (!P || !Perm) return CHOLMOD_HIP_INVALID ;
    const i64 n = P->n ;
    {
        // a permutation of 0 .. n-1, checked before anything on the device may index with it
        std::vector<char> seen ((size_t) std::max<i64> (n, 1), 0) ;
        for (i64 k = 0 ; k < n ; k++)
        {
            const i64 p = Perm [k] ;
            if (p < 0 || p >= n || seen [p]) return CHOLMOD_HIP_INVALID ;
            seen [p] = 1 ;
        }
    }
    if (P->host_only) return CHOLMOD_HIP_NO_DEVICE ;
    if (!P->d_perm) HIPCHK (hipMalloc ((void **) &P->d_perm, std::max<i64> (n, 1) * sizeof (i64))) ;
    // (a solve in flight on the engine stream may still read the old one)
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    if (n) HIPCHK (hipMemcpy (P->d_perm, Perm, n * sizeof (i64), hipMemcpyHostToDevice)) ;
    return CHOLMOD_HIP_OK ;
}

namespace sship {

// workspaces of a device-resident solve; nothing is allocated once they exist
int sd_ensure (cholmod_hip_plan *P, bool with_factor, bool columns)
{
    const i64 n = P->n ;
    if (!P->sd_ev0)
    {
        HIPCHK (hipEventCreate (&P->sd_ev0)) ;
        HIPCHK (hipEventCreate (&P->sd_ev1)) ;
    }
    if (!P->d_sd_W) HIPCHK (hipMalloc ((void **) &P->d_sd_W, (size_t) n * SD_NP * sizeof (double))) ;
    if (!with_factor) return CHOLMOD_HIP_OK ;
    // a few right-hand sides run the kernels of cholmod_hip_solve: its side vector and accumulators, sized once for
    // the most that come this way
    const i64 most = SD_BLOCK_MIN_NRHS - 1 ;
    return columns ? solve_workspace (P, n * most, most, false) : solve_workspace (P, 0, 0, true) ;
}

// the columns src [nrhs][lds] into dst [nrhs][ldd], through the permutation if there is one (inverse: scattered by it)
int sd_move_columns (hipStream_t st, i64 n, i64 nrhs, const i64 *perm, int inverse, const double *src, i64 lds, double *dst, i64 ldd)
{
    if (perm) for (i64 r = 0 ; r < nrhs ; r++)
        hipLaunchKernelGGL (k_perm, dim3 ((unsigned) ((n + 255) / 256)), dim3 (256), 0, st, n, perm, src + r * lds, dst + r * ldd, inverse) ;
    else HIPCHK (hipMemcpy2DAsync (dst, ldd * sizeof (double), src, lds * sizeof (double), n * sizeof (double), (size_t) nrhs,
        hipMemcpyDeviceToDevice, st)) ;
    return CHOLMOD_HIP_OK ;
}

void sd_pack (hipStream_t st, i64 n, const i64 *perm, const double *B, i64 ldb, int pw, double *W)
{
    hipLaunchKernelGGL (k_sd_pack, dim3 ((unsigned) ((n + 255) / 256)), dim3 (256), 0, st, n, perm, B, ldb, pw, W) ;
}

void sd_unpack (hipStream_t st, i64 n, const i64 *perm, const double *W, int pw, double *X, i64 ldx)
{
    hipLaunchKernelGGL (k_sd_unpack, dim3 ((unsigned) ((n + 255) / 256)), dim3 (256), 0, st, n, perm, W, pw, X, ldx) ;
}

void sd_sweeps_columns (const cholmod_hip_plan *P, int which, const FrontD *frw, const double *Lw, bool cxs, hipStream_t st, double *x, i64 ldx, int nrhs)
{
    solve_sweeps (P, which, ColumnKernels {P, frw, Lw, st, x, ldx, nrhs, cxs}) ;
}

void sd_sweeps_panel (const cholmod_hip_plan *P, int which, const FrontD *frw, const double *Lw, bool cxs, hipStream_t st, double *W)
{
    solve_sweeps (P, which, PanelKernels {P, frw, Lw, st, W, cxs}) ;
}

} // namespace sship

int cholmod_hip_solve_device (cholmod_hip_plan *P, int which, int perm_in, int perm_out, const double *dB, int64_t ldb,
    double *dX, int64_t ldx, int64_t nrhs, void *stream)
{
    if (!P || P->host_only || !dB || !dX || nrhs < 0 || ldb < P->n || ldx < P->n || which < 0 || which > 3)
        return CHOLMOD_HIP_INVALID ;
    if ((perm_in || perm_out) && !P->d_perm) return CHOLMOD_HIP_INVALID ;       // cholmod_hip_set_perm first
    const i64 n = P->n ;
    if (nrhs == 0 || n == 0) return CHOLMOD_HIP_OK ;
    const double *Lw = nullptr ;
    const FrontD *frw = nullptr ;
    if (which != 3)
    {
        Lw = whole_factor (P) ;
        frw = whole_fronts (P) ;
        if (!Lw || !frw) return CHOLMOD_HIP_INVALID ;  // several ranks: cholmod_hip_gather_factor first
    }
    // a complex factor: the full twin (CHOLMOD_HIP_PHI_TWIN alone) is an ordinary real factor; in its own storage the
    // kernels rebuild the odd twin columns as they read (n, ld and the permutation are the twin's either way)
    const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;
    const bool columns = nrhs < SD_BLOCK_MIN_NRHS ;
    HIP_TRY (sd_ensure (P, which != 3, columns)) ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (stream_enter (P, user)) ;
    if (which != 3) refresh_inverses (P, frw, Lw, cxs) ;
    HIPCHK (hipEventRecord (P->sd_ev0, st)) ;
    const i64 *pin = perm_in ? P->d_perm : nullptr, *pout = perm_out ? P->d_perm : nullptr ;
    const unsigned nblk = (unsigned) ((n + 255) / 256) ;
    double *W = P->d_sd_W ;
    if (columns)
    {
        // directly on the permuted columns, W as [nrhs][n]
        HIP_TRY (sd_move_columns (st, n, nrhs, pin, 0, dB, ldb, W, n)) ;
        if (which != 3) solve_sweeps (P, which, ColumnKernels {P, frw, Lw, st, W, n, (int) nrhs, cxs}) ;
        HIP_TRY (sd_move_columns (st, n, nrhs, pout, 1, W, n, dX, ldx)) ;
    }
    else for (i64 r0 = 0 ; r0 < nrhs ; r0 += SD_NP)
    {
        const int pw = (int) std::min<i64> (SD_NP, nrhs - r0) ;
        hipLaunchKernelGGL (k_sd_pack, dim3 (nblk), dim3 (256), 0, st, n, pin, dB + r0 * ldb, (i64) ldb, pw, W) ;
        if (which != 3) solve_sweeps (P, which, PanelKernels {P, frw, Lw, st, W, cxs}) ;
        hipLaunchKernelGGL (k_sd_unpack, dim3 (nblk), dim3 (256), 0, st, n, pout, (const double *) W, pw, dX + r0 * ldx, (i64) ldx) ;
    }
    HIPCHK (hipGetLastError ()) ;
    HIPCHK (hipEventRecord (P->sd_ev1, st)) ;
    // the way out of stream_enter on the timed event: ahead of what the caller enqueues next
    HIPCHK (hipStreamWaitEvent (user, P->sd_ev1, 0)) ;
    // stats [24]: the two events are read by cholmod_hip_get_stats (a cholmod_hip_solve in between overwrites the mark)
    P->solve_seconds = -1.0 ;
    P->sd_time_pending = true ;
    return CHOLMOD_HIP_OK ;
}
