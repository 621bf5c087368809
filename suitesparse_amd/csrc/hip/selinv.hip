// selinv.hip -- the selected inverse on the device: Zx = the entries of (L L')^-1 = (P (A + beta I) P')^-1 on the pattern of
// L, in the layout of Lx (cholmod_hip_selinv_device), and what a caller takes from it without leaving the device
// (cholmod_hip_selinv_gather_device: the values at the entries of its matrix, the diagonal).  Supernodal Takahashi: the
// factorization run backwards, the plan's batches from the last to the first, so that a front finds Z on its below-rows
// finished in the panels of its ancestors.  Kernels: selinv_kernels.hip.h.  No test hook reaches this file: it is built
// once for both libraries.
//
// Workspace.  A front's Z [I, I] is GATHERED from Zx -- for every column of I the owning ancestor through the supernode
// map, the row by a search in that ancestor's row list -- straight into the front's square, instead of being mailed by
// the parent through the contribution-block arena.  That costs a binary search per entry of Z [I, I] and buys three
// things: the arena stays untouched (its slots are the factorization's, in any batch order), every square entry has one
// writer by construction, and a batch may be cut into chunks anywhere.  The scratch is the squares of one chunk plus
// one 64 x 64 partial per 64-row slice of its fronts; thin fronts need none (LDS).  info [5] counts both buffers.
//
// The launch program built here (Builder) and the scratch are shared with the factor gradient
// (factor_grad.hip, through selinv_internal.hip.h: sweep_ensure, sweep_release, sweep_info): it
// runs the same steps with kernels of its own, on the engine stream like this sweep, so the scratch has one user at a time.
#include "selinv_kernels.hip.h"
#include "selinv_internal.hip.h"

namespace {

// doubles of scratch the chunks of a batch may take (the largest front always fits): CHOLMOD_HIP_SELINV_BUDGET_MB, 2 GiB
static i64 scratch_budget ()
{
    const char *e = getenv ("CHOLMOD_HIP_SELINV_BUDGET_MB") ;
    const double mb = e ? atof (e) : 2048.0 ;
    return (i64) (std::max (mb, 0.0) * 1048576.0 / 8.0) ;
}

static bool is_thin (const FrontD &f) { return f.nscol <= SI_NB && f.nsrow <= SM_MAX ; }
static int nblocks (const FrontD &f) { return (f.nscol + SI_NB - 1) / SI_NB ; }
static i64 slices_of (const FrontD &f) { return (f.nsrow + 63) / 64 ; }
static i64 scratch_of (const FrontD &f) { return (i64) f.nsrow * f.nsrow + slices_of (f) * SI_PTILE ; }

struct Builder {
    const cholmod_hip_plan *P ; SelInv &S ;
    void flops (const FrontD &f, int b0, int nb)
    {
        const double r = f.nsrow - b0 - nb, w = nb ;
        S.hot_flops += 2 * r * r * w ;
        S.all_flops += 2 * r * r * w + 3 * r * w * w + 2 * w * w * w ;     // ... L_Rb' T, the solve of Z_Rb, the two of Z_bb
    }
    // the thin fronts of a batch: one launch per LDS class, so that small fronts share a CU
    void thin_launches (const std::vector<i32> &ids)
    {
        static const int cls_doubles [3] = {2048, 8192, 1 << 30} ;
        for (int c = 0 ; c < 3 ; c++)
        {
            const i64 first = (i64) S.thin.size () ;
            int most = 0 ;
            for (i32 s : ids)
            {
                const FrontD &f = P->fr [s] ;
                const int need = si_thin_lds (f.nscol, f.nsrow) ;
                if (need > cls_doubles [c] || (c > 0 && need <= cls_doubles [c - 1])) continue ;
                S.thin.push_back (s) ;
                most = std::max (most, need) ;
                flops (f, 0, f.nscol) ;
            }
            const int nt = (int) ((i64) S.thin.size () - first) ;
            if (nt > 0) S.steps.push_back ({SelInv::THIN, first, nt, (unsigned) nt, (size_t) most * sizeof (double)}) ;
        }
    }
    // one launch whose tasks own `count (slot)` workgroups each
    template <typename F> void per_slot (int kind, size_t slot0, size_t slot1, F count)
    {
        const i64 first = (i64) S.tasks.size () ;
        i64 wg = 0 ;
        for (size_t q = slot0 ; q < slot1 ; q++)
        {
            const int c = count (P->fr [S.slots [q].front]) ;
            if (c <= 0) continue ;
            S.tasks.push_back ({(i32) q, 0, 0, (i32) wg, 0, 0, 0}) ;
            wg += c ;
        }
        if (wg > 0) S.steps.push_back ({kind, first, (int) ((i64) S.tasks.size () - first), (unsigned) wg, 0}) ;
    }
    // a chunk of generic fronts: fill, then step t = block (last - t) of every front that has one, then the panels out
    void chunk (const std::vector<i32> &ids)
    {
        const size_t slot0 = S.slots.size () ;
        i64 moff = 0 ;
        int most = 0 ;
        for (i32 s : ids)
        {
            const FrontD &f = P->fr [s] ;
            S.slots.push_back ({s, 0, moff}) ;
            moff += (i64) f.nsrow * f.nsrow ;
            most = std::max (most, nblocks (f)) ;
        }
        S.m_len = std::max (S.m_len, moff) ;
        const size_t slot1 = S.slots.size () ;
        per_slot (SelInv::FILL, slot0, slot1, [] (const FrontD &f) { return f.nsrow - f.nscol ; }) ;
        for (int t = 0 ; t < most ; t++)
        {
            // (block and diagonal tasks of the step side by side: the same b0, nb, nslices, poff)
            std::vector<SiTask> blk, dg ;
            i64 wg = 0, poff = 0 ;
            for (size_t q = slot0 ; q < slot1 ; q++)
            {
                const FrontD &f = P->fr [S.slots [q].front] ;
                const int b = nblocks (f) - 1 - t ;
                if (b < 0) continue ;
                const int b0 = b * SI_NB, nb = std::min<int> (SI_NB, f.nscol - b0), nR = f.nsrow - b0 - nb ;
                const int ns = (nR + 63) / 64 ;
                const SiTask T = {(i32) q, b0, nb, (i32) wg, ns, 0, poff} ;
                if (ns > 0) blk.push_back (T) ;
                dg.push_back (T) ;
                wg += ns ; poff += ns ;
                flops (f, b0, nb) ;
            }
            S.p_len = std::max (S.p_len, poff * SI_PTILE) ;
            if (!blk.empty ())
            {
                S.steps.push_back ({SelInv::BLOCK, (i64) S.tasks.size (), (int) blk.size (), (unsigned) wg, SI_BLOCK_LDS}) ;
                S.tasks.insert (S.tasks.end (), blk.begin (), blk.end ()) ;
            }
            S.steps.push_back ({SelInv::DIAG, (i64) S.tasks.size (), (int) dg.size (), (unsigned) dg.size (), 0}) ;
            S.tasks.insert (S.tasks.end (), dg.begin (), dg.end ()) ;
        }
        per_slot (SelInv::STORE, slot0, slot1, [] (const FrontD &f) { return (int) f.nscol ; }) ;
    }
    void build ()
    {
        // the plan's batches, the last first: every front after its parent
        i32 nbatch = 0 ;
        for (i64 s = 0 ; s < P->nsuper ; s++) nbatch = std::max (nbatch, P->batch_of [s] + 1) ;
        std::vector<std::vector<i32>> batches (nbatch) ;
        for (i64 s = 0 ; s < P->nsuper ; s++) batches [P->batch_of [s]].push_back ((i32) s) ;
        const i64 budget = scratch_budget () ;
        for (i32 b = nbatch - 1 ; b >= 0 ; b--)
        {
            std::vector<i32> thin, generic ;
            for (i32 s : batches [b]) (is_thin (P->fr [s]) ? thin : generic).push_back (s) ;
            // widest fronts first: the later chunks of a batch have the shorter block chains
            std::stable_sort (generic.begin (), generic.end (), [&] (i32 x, i32 y) { return P->fr [x].nscol > P->fr [y].nscol ; }) ;
            std::vector<i32> cur ;
            i64 used = 0 ;
            for (i32 s : generic)
            {
                const i64 need = scratch_of (P->fr [s]) ;
                if (!cur.empty () && used + need > budget) { chunk (cur) ; cur.clear () ; used = 0 ; }
                cur.push_back (s) ; used += need ;
            }
            if (!cur.empty ()) chunk (cur) ;
            thin_launches (thin) ;
        }
    }
} ;

// once per plan: the program, its task lists on the device, the clocks
static int prepare (cholmod_hip_plan *P, SelInv *S)
{
    Builder {P, *S}.build () ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_si_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int) SI_BLOCK_LDS)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_si_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int) SI_BLOCK_LDS)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_si_thin, hipFuncAttributeMaxDynamicSharedMemorySize, SI_THIN_LDS_MAX)) ;
    hipError_t e ;
    S->d_tasks = dupload (S->tasks, e) ; HIPCHK (e) ;
    S->d_slots = dupload (S->slots, e) ; HIPCHK (e) ;
    S->d_thin = dupload (S->thin, e) ; HIPCHK (e) ;
    for (SweepClock *c : {&S->si_clock, &S->fg_clock})
    {
        HIPCHK (hipEventCreate (&c->ev0)) ;
        HIPCHK (hipEventCreate (&c->ev1)) ;
    }
    S->built = true ;
    return CHOLMOD_HIP_OK ;
}

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
                hipLaunchKernelGGL (k_si_thin, grid, wg, s.lds, st, S->d_thin + s.first, fr, P->d_supermap, P->d_Ls, Lx, S->d_Zx) ;
                break ;
            case SelInv::FILL:
                hipLaunchKernelGGL (k_si_fill, grid, wg, 0, st, t, s.ntasks, S->d_slots, fr, P->d_supermap, P->d_Ls, S->d_Zx, S->d_M) ;
                break ;
            case SelInv::BLOCK:
                hipLaunchKernelGGL (k_si_block, grid, wg, s.lds, st, t, s.ntasks, S->d_slots, fr, Lx, S->d_M, S->d_P) ;
                break ;
            case SelInv::DIAG:
                hipLaunchKernelGGL (k_si_diag, grid, wg, SI_BLOCK_LDS, st, t, S->d_slots, fr, Lx, S->d_M, S->d_P) ;
                break ;
            case SelInv::STORE:
                hipLaunchKernelGGL (k_si_store, grid, wg, 0, st, t, s.ntasks, S->d_slots, fr, S->d_M, S->d_Zx) ;
                break ;
        }
    }
    S->si_clock.launches = (long) S->steps.size () ;
}

} // namespace

int sweep_ensure (cholmod_hip_plan *P, double *SelInv::*result)
{
    if (!P->si) P->si = new (std::nothrow) SelInv ;
    SelInv *S = P->si ;
    if (!S) return CHOLMOD_HIP_OUT_OF_MEMORY ;
    if (!S->built)
    {
        const int rc = prepare (P, S) ;
        if (rc != CHOLMOD_HIP_OK) { selinv_free (P) ; return rc ; }
    }
    const i64 want [3] = {P->xsize, S->m_len, S->p_len} ;
    double **into [3] = {&(S->*result), &S->d_M, &S->d_P} ;
    bool mine [3] = {false, false, false} ;
    for (int k = 0 ; k < 3 ; k++)
    {
        if (*into [k]) continue ;
        const int rc = device_alloc (into [k], want [k]) ;
        mine [k] = (rc == CHOLMOD_HIP_OK) ;
        if (mine [k]) continue ;
        for (int q = 0 ; q < k ; q++) if (mine [q]) { (void) hipFree (*into [q]) ; *into [q] = nullptr ; }   // (the factor is untouched)
        return rc ;
    }
    return CHOLMOD_HIP_OK ;
}

void sweep_release (cholmod_hip_plan *P, double *SelInv::*result)
{
    SelInv *S = P->si ;
    if (S->*result) (void) hipFree (S->*result) ;
    S->*result = nullptr ;
    if (S->d_Zx || S->d_Gx) return ;
    for (void *d : {(void *) S->d_M, (void *) S->d_P}) if (d) (void) hipFree (d) ;
    S->d_M = S->d_P = nullptr ;
}

void sweep_info (SelInv *S, SweepClock &c, double *out8)
{
    if (c.pending)
    {
        float ms = 0 ;
        if (hipEventSynchronize (c.ev1) == hipSuccess && hipEventElapsedTime (&ms, c.ev0, c.ev1) == hipSuccess)
            c.seconds = ms * 1e-3 ;
        else (void) hipGetLastError () ;
        c.pending = false ;
    }
    out8 [0] = c.seconds ;
    out8 [1] = (double) c.launches ;
    out8 [2] = S->hot_flops ;
    out8 [3] = S->all_flops ;
}

void selinv_free (cholmod_hip_plan *P)
{
    SelInv *S = P->si ;
    P->si = nullptr ; P->si_valid = P->fg_valid = false ;
    if (!S) return ;
    for (void *d : {(void *) S->d_Zx, (void *) S->d_Gx, (void *) S->d_tr, (void *) S->d_M, (void *) S->d_P, (void *) S->d_tasks,
        (void *) S->d_slots, (void *) S->d_thin}) if (d) (void) hipFree (d) ;
    for (hipEvent_t e : {S->si_clock.ev0, S->si_clock.ev1, S->fg_clock.ev0, S->fg_clock.ev1})
        if (e) (void) hipEventDestroy (e) ;
    delete S ;
}

void selinv_gather_logdet_grad (cholmod_hip_plan *P, const i32 *colof, double *out, hipStream_t st)
{
    const i64 nz = P->s_cur_nz ;
    if (nz > 0)
        hipLaunchKernelGGL (k_si_gather_logdet_grad, dim3 ((unsigned) ((nz + 255) / 256)), dim3 (256), 0, st, P->n, nz, P->d_Sp, P->d_Si,
            colof, P->d_vsrc, P->d_supermap, P->d_fr, P->d_Ls, P->si->d_Zx, out) ;
}

extern "C" {

int cholmod_hip_selinv_device (cholmod_hip_plan *P, void *stream)
{
    if (sweep_bad_plan (P)) return CHOLMOD_HIP_INVALID ;
    HIP_TRY (sweep_ensure (P, &SelInv::d_Zx)) ;
    SelInv *S = P->si ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    P->si_valid = false ;
    HIP_TRY (stream_enter (P, user)) ;
    HIPCHK (hipEventRecord (S->si_clock.ev0, st)) ;
    run (P, st) ;
    HIPCHK (hipEventRecord (S->si_clock.ev1, st)) ;
    HIP_TRY (stream_leave (P, user)) ;
    S->si_clock.pending = true ;
    P->si_valid = true ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_selinv_gather_device (cholmod_hip_plan *P, double *dZvalues, int64_t nvalues, double *dDiag, int perm,
    void *stream)
{
    if (sweep_bad_plan (P) || !P->si_valid || !P->si || !P->si->d_Zx) return CHOLMOD_HIP_INVALID ;
    if (dZvalues)
    {
        // the value map of the current resident packed S, and values that are given, not computed
        if (!P->d_Sp || !P->d_vsrc || P->s_unpacked || P->vsrc_nz != P->s_cur_nz || nvalues != P->vals_n || P->pm_set)
            return CHOLMOD_HIP_INVALID ;
    }
    if (dDiag && perm && !P->d_perm) return CHOLMOD_HIP_INVALID ;
    if ((!dZvalues && !dDiag) || P->n == 0) return CHOLMOD_HIP_OK ;
    const i64 n = P->n ;
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (stream_enter (P, user)) ;
    const unsigned ncol = (unsigned) ((n + 255) / 256) ;
    if (dZvalues)
    {
        if (nvalues > 0)
            hipLaunchKernelGGL (k_si_nan_fill, dim3 ((unsigned) ((nvalues + 255) / 256)), dim3 (256), 0, st, (i64) nvalues, dZvalues) ;
        hipLaunchKernelGGL (k_si_gather_values, dim3 (ncol), dim3 (256), 0, st, n, P->d_Sp, P->d_Si, P->d_vsrc, P->d_supermap,
            P->d_fr, P->d_Ls, P->si->d_Zx, dZvalues) ;
    }
    if (dDiag)
        hipLaunchKernelGGL (k_si_gather_diag, dim3 (ncol), dim3 (256), 0, st, n, perm ? P->d_perm : nullptr, P->d_supermap,
            P->d_fr, P->si->d_Zx, dDiag) ;
    return stream_leave (P, user) ;
}

int cholmod_hip_selinv_download (cholmod_hip_plan *P, double *Zx_host)
{
    if (sweep_bad_plan (P) || !Zx_host || !P->si_valid || !P->si || !P->si->d_Zx) return CHOLMOD_HIP_INVALID ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    if (P->xsize > 0) HIPCHK (hipMemcpy (Zx_host, P->si->d_Zx, (size_t) P->xsize * sizeof (double), hipMemcpyDeviceToHost)) ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_selinv_release (cholmod_hip_plan *P)
{
    if (sweep_bad_plan (P)) return CHOLMOD_HIP_INVALID ;
    P->si_valid = false ;
    if (!P->si) return CHOLMOD_HIP_OK ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    sweep_release (P, &SelInv::d_Zx) ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_selinv_info (cholmod_hip_plan *P, double *out8)
{
    if (sweep_bad_plan (P) || !out8) return CHOLMOD_HIP_INVALID ;
    for (int k = 0 ; k < 8 ; k++) out8 [k] = 0 ;
    SelInv *S = P->si ;
    if (!S) return CHOLMOD_HIP_OK ;
    sweep_info (S, S->si_clock, out8) ;
    out8 [4] = S->d_Zx ? 8.0 * (double) std::max<i64> (P->xsize, 1) : 0.0 ;
    out8 [5] = S->d_Zx ? 8.0 * (double) (std::max<i64> (S->m_len, 1) + std::max<i64> (S->p_len, 1)) : 0.0 ;
    out8 [6] = P->si_valid ? 1.0 : 0.0 ;
    return CHOLMOD_HIP_OK ;
}

} // extern "C"
