// engine.hip -- host side of the MI355X supernodal Cholesky engine that touches the device: upload of a plan
// (plan_build.hip / schedule_dense.hip derive it), the runner of its launch list, and the extern "C" shim declared in
// include/cholmod_hip.h (the exchange between ranks and the gather: exchange.hip; the triangular solves: solve.hip; the
// matrix-values pipeline: values.hip; the checks on a finished factor: checks.hip).  One process drives one GPU.
#include "update_launch.hip.h"
#include "chain256_kernels.hip.h"
#include "exchange_internal.hip.h"
#include "engine_internal.hip.h"
#include <thread>

namespace {

static void free_device (cholmod_hip_plan *P)
{
    drop_product_map (P) ;
    selinv_free (P) ;
    grad_free (P) ;
    if (P->prog_dev) { (void) hipHostFree (P->prog_dev) ; P->prog_dev = nullptr ; }
    if (P->h_vals) { (void) hipHostFree (P->h_vals) ; P->h_vals = nullptr ; }
    for (auto e : P->chunk_ev) (void) hipEventDestroy (e) ;
    P->chunk_ev.clear () ;
    if (P->d_vorder) { (void) hipFree (P->d_vorder) ; P->d_vorder = nullptr ; }
    exchange_release (P) ;
    if (P->ar_done) (void) hipEventDestroy (P->ar_done) ;
    void *ptrs [] = {P->d_Ls, P->d_fr, P->d_supermap, P->d_child, P->d_relmap, P->d_info,
        P->d_lvl_list, P->d_Lx, P->d_cb, P->d_zg, P->d_eg, P->d_pg, P->d_tg, P->d_tu_cnt, P->d_cdesc, P->d_smd, P->d_sp01, P->d_gg, P->d_sm,
        P->d_Sp, P->d_Si, P->d_Snz, P->d_Sx, P->d_amap, P->d_X, P->d_perm, P->d_xchg, P->d_stage, P->d_ag, P->d_agf, P->d_Lx_full, P->d_fr_full, P->d_dg, P->d_rg, P->d_wg, P->d_cg, P->d_cflags, P->d_crel, P->d_relpairs, P->d_dinv, P->d_sv,
        P->d_inv_tasks, P->d_winv, P->d_solved, P->d_sv_acc, P->d_sd_W, P->d_sd_acc, P->d_chk, P->d_chk_out, P->d_thin_tim, P->d_sb_tasks, P->d_sb_commit, P->d_first_fail, P->d_vsrc, P->d_vals,
        P->d_xg, P->d_gmap, P->d_fz, P->d_gfz, P->d_invmap, P->d_rs_Tp, P->d_rs_Tj, P->d_rs_Tq, P->d_rs_X, P->d_rs_B} ;
    for (void *p : ptrs) if (p) (void) hipFree (p) ;
    for (auto e : P->evpool) (void) hipEventDestroy (e) ;
    for (auto e : P->sync_ev) (void) hipEventDestroy (e) ;
    if (P->stream2) (void) hipStreamDestroy (P->stream2) ;
    if (P->ev0) (void) hipEventDestroy (P->ev0) ;
    if (P->ev1) (void) hipEventDestroy (P->ev1) ;
    for (hipEvent_t e : {P->user_ev_in, P->user_ev_out, P->sd_ev0, P->sd_ev1}) if (e) (void) hipEventDestroy (e) ;
    if (P->stream) (void) hipStreamDestroy (P->stream) ;
}

static int upload_plan (cholmod_hip_plan *P)
{
    hipError_t e ;
    const bool ptiming = getenv ("CHOLMOD_HIP_PLAN_TIMING") != nullptr ;
    auto pnow = [] () { return std::chrono::duration<double> (std::chrono::steady_clock::now ().time_since_epoch ()).count () ; } ;
    double tu0 = pnow () ;
    HIPCHK (hipStreamCreate (&P->stream)) ;
    HIPCHK (hipEventCreateWithFlags (&P->user_ev_in, hipEventDisableTiming)) ;
    HIPCHK (hipEventCreateWithFlags (&P->user_ev_out, hipEventDisableTiming)) ;
    if (const char *e = TEST_ENV ("CHOLMOD_HIP_TEST_JITTER"))
    {
        unsigned long long seed = 0 ; int mx = 2000 ;
        if (sscanf (e, "%llu:%d", &seed, &mx) >= 1 && mx > 0)
        {
            P->jitter_us = mx ;
            P->jitter_state = seed * 0x9E3779B97F4A7C15ull + (unsigned long long) (P->rank + 1) * 0xD1B54A32D192ED03ull ;
        }
    }
    { const char *e = TEST_ENV ("CHOLMOD_HIP_TEST_DROP_WAITS") ; P->test_drop_waits = e ? std::max (atoi (e), 1) : 0 ; }
    if (const char *e = TEST_ENV ("CHOLMOD_HIP_TEST_HANG_EXCHANGE")) (void) sscanf (e, "%d:%ld:%ld", &P->test_hang_rank, &P->test_hang_xchg, &P->test_hang_fact) ;
    // several ranks: k_update3 with four tiles per workgroup, so that the exchange stream's (and RCCL's) four-wave workgroups
    // find room beside a trailing update (rocprofv3, rank 0 of 8 at 200^3: k_win_move 959 -> 94 ms in all, longest launch
    // 79 -> 1.2 ms; the update itself 2351 -> 2378 ms).  (its knob, measured both ways in round 4, is gone.)
    P->upd3_wg4 = P->world > 1 || P->force_shared ;
    {
        // The exchange stream runs BESIDE the rest of a trailing update (look-ahead: window open, extend-add, pack, the
        // collective): its small workgroups must get the wave slots the update's tiles free up, ahead of the update's own
        // remaining tiles -- at default priority rocprofv3 shows k_win_move stretched over the whole 78 ms of the update it
        // was meant to hide behind (round 4).  
        int least = 0, greatest = 0 ;
        if (hipDeviceGetStreamPriorityRange (&least, &greatest) == hipSuccess && greatest != least)
            HIPCHK (hipStreamCreateWithPriority (&P->stream2, hipStreamDefault, greatest)) ;
        else HIPCHK (hipStreamCreate (&P->stream2)) ;
    }
    for (int q = 0 ; q < P->sch.nevents ; q++)
    {
        hipEvent_t e ;
        HIPCHK (hipEventCreateWithFlags (&e, hipEventDisableTiming)) ;
        P->sync_ev.push_back (e) ;
    }
    HIPCHK (hipEventCreate (&P->ev0)) ;
    HIPCHK (hipEventCreate (&P->ev1)) ;
    size_t freeb = 0, totalb = 0 ;
    HIPCHK (hipMemGetInfo (&freeb, &totalb)) ;
    double need = 8.0 * P->lx_local + 8.0 * P->arena + 8.0 * P->ssize + 4.0 * P->relsize
        + sizeof (GemmGroup) * (double) P->sch.gg.size () + 64.0 * P->nsuper + (double) (64 << 20) + 4.0 * P->sch.invsize ;
    if (need > (double) freeb)
    {
        fprintf (stderr, "cholmod_hip: factor needs %.2f GB of HBM, %.2f GB free\n",
            need / 1e9, freeb / 1e9) ;
        return CHOLMOD_HIP_OUT_OF_MEMORY ;
    }
    double tu1 = pnow () ;
    P->d_Ls = dupload (P->Ls, e) ; HIPCHK (e) ;
    P->d_fr = dupload (P->fr, e) ; HIPCHK (e) ;
    P->d_supermap = dupload (P->supermap, e) ; HIPCHK (e) ;
    P->d_child = dupload (P->child, e) ; HIPCHK (e) ;
    P->d_crel = dupload (P->crel, e) ; HIPCHK (e) ;
    P->d_relpairs = dupload (P->relpairs, e) ; HIPCHK (e) ;
    {
        std::vector<ChildD> cdv (P->child.size ()) ;
        for (size_t q = 0 ; q < P->child.size () ; q++)
        {
            if (P->child [q] < 0 || (size_t) P->child [q] >= P->fr.size ()) { cdv [q] = ChildD {0, 0, 0, 1} ; continue ; }   // (padding entry of an empty list)
            const FrontD &cf = P->fr [P->child [q]] ;
            cdv [q] = ChildD {cf.cb, cf.rel, cf.ncb, cf.cbp} ;
        }
        P->d_cdesc = dupload (cdv, e) ; HIPCHK (e) ;
    }
    P->d_lvl_list = dupload (P->lvl_list, e) ; HIPCHK (e) ;
    P->d_zg = dupload (P->sch.zg, e) ; HIPCHK (e) ;
    P->d_eg = dupload (P->sch.eg, e) ; HIPCHK (e) ;
    P->d_pg = dupload (P->sch.pg, e) ; HIPCHK (e) ;
    P->d_tg = dupload (P->sch.tg, e) ; HIPCHK (e) ;
    HIPCHK (hipMalloc ((void **) &P->d_tu_cnt, std::max<size_t> (P->sch.tg.size (), 1) * sizeof (i32))) ;
    P->d_gg = dupload (P->sch.gg, e) ; HIPCHK (e) ;
    P->d_dg = dupload (P->sch.dg, e) ; HIPCHK (e) ;
    P->d_rg = dupload (P->sch.rg, e) ; HIPCHK (e) ;
    P->d_wg = dupload (P->sch.wg, e) ; HIPCHK (e) ;
    P->d_cg = dupload (P->sch.cg, e) ; HIPCHK (e) ;
    P->d_xg = dupload (P->sch.xg, e) ; HIPCHK (e) ;
    P->d_gmap = dupload (P->sch.gmap, e) ; HIPCHK (e) ;
    if (!P->sch.fz.empty ())
    {
        // (the regions that carry their children's contribution-block entries: one entry per region of the schedule)
        std::vector<i32> gfz (P->sch.gfz) ;
        gfz.resize (P->sch.gg.size (), -1) ;
        P->d_fz = dupload (P->sch.fz, e) ; HIPCHK (e) ;
        P->d_gfz = dupload (gfz, e) ; HIPCHK (e) ;
        HIPCHK (hipMalloc ((void **) &P->d_invmap, std::max<i64> (P->sch.invsize, 1) * sizeof (i32))) ;
    }
    HIPCHK (hipMalloc ((void **) &P->d_cflags, (4 * (size_t) P->sch.ncflags + 4) * sizeof (int))) ;
    HIPCHK (hipMalloc ((void **) &P->d_dinv, (size_t) std::max (P->sch.max_dinv_slots, 1) * 4096 * sizeof (double))) ;
    P->d_sm = dupload (P->sch.sm, e) ; HIPCHK (e) ;
    {
        std::vector<FrontD> smd (P->sch.sm.size ()) ;
        for (size_t q = 0 ; q < smd.size () ; q++) smd [q] = P->fr [P->sch.sm [q]] ;
        P->d_smd = dupload (smd, e) ; HIPCHK (e) ;
        HIPCHK (hipMalloc ((void **) &P->d_sp01, std::max<size_t> (2 * smd.size (), 1) * sizeof (i64))) ;
    }
    P->d_sv = dupload (P->sv_tasks, e) ; HIPCHK (e) ;
    double tu2 = pnow () ;
    HIPCHK (hipMalloc ((void **) &P->d_relmap, std::max<i64> (std::max (P->relsize, P->relsize_all), 1) * sizeof (i32))) ;
    HIPCHK (hipMalloc ((void **) &P->d_info, std::max<i64> (P->nsuper, 1) * sizeof (i32))) ;
    HIPCHK (hipMalloc ((void **) &P->d_first_fail, sizeof (int))) ;
    // test hook: behave as if the reservation of L failed (degradation tests)
    if (TEST_ENV ("CHOLMOD_HIP_TEST_FAIL_ALLOC")) return CHOLMOD_HIP_OUT_OF_MEMORY ;
    HIPCHK (hipMalloc ((void **) &P->d_Lx, (std::max<i64> (P->lx_local, 1) + UPD3_LX_PAD) * sizeof (double))) ;
    HIPCHK (hipMalloc ((void **) &P->d_cb, std::max<i64> (P->arena, 1) * sizeof (double))) ;
    HIPCHK (hipMalloc ((void **) &P->d_xchg, 3 * (size_t) P->world * sizeof (double))) ;
    {
        i64 mx = 1, mxg = 1, mxf = 1 ;
        for (const Launch &L : P->sch.launches)
            if (L.kind == K_XCHG_RS || L.kind == K_XCHG_AG)
            {
                mx = std::max (mx, ((i64) L.xd.w * L.xd.w + ((i64) L.xd.R + L.xd.Rf) * L.xd.w) * L.xd.g) ;
                mxg = std::max (mxg, (i64) L.xd.R * L.xd.w * L.xd.g) ;
                mxf = std::max (mxf, (i64) L.xd.Rf * L.xd.w * L.xd.g) ;
            }
        HIPCHK (hipMalloc ((void **) &P->d_stage, (size_t) mx * sizeof (double))) ;
        HIPCHK (hipMalloc ((void **) &P->d_ag, (size_t) mxg * sizeof (double))) ;
        HIPCHK (hipMalloc ((void **) &P->d_agf, (size_t) mxf * sizeof (double))) ;
        P->agf_len = mxf ;
        P->stage_len = mx ; P->ag_len = mxg ;
    }
    double tu3 = pnow () ;
    if (getenv ("CHOLMOD_HIP_THIN_TIMING"))
    {
        HIPCHK (hipMalloc ((void **) &P->d_thin_tim, (P->sch.launches.size () + 1) * 10 * sizeof (long long))) ;
        HIPCHK (hipMemset (P->d_thin_tim, 0, (P->sch.launches.size () + 1) * 10 * sizeof (long long))) ;
    }
    if (P->nsuper > 0)
    {
        int grid = (int) ((P->nsuper * 64 + 255) / 256) ;
        hipLaunchKernelGGL (k_relmap, dim3 (grid), dim3 (256), 0, P->stream,
            (int) P->nsuper, P->d_fr, P->d_Ls, P->d_relmap) ;
        if (!P->relpairs.empty ())
            hipLaunchKernelGGL (k_relmap_pairs, dim3 ((unsigned) ((P->relpairs.size () * 64 + 255) / 256)), dim3 (256), 0, P->stream,
                (int) P->relpairs.size (), P->d_relpairs, P->d_fr, P->d_Ls, P->d_relmap) ;
        InvPair *d_ivp = nullptr ;
        if (!P->sch.ivp.empty ())
        {
            d_ivp = dupload (P->sch.ivp, e) ;
            if (e == hipSuccess) hipLaunchKernelGGL (k_invmap, dim3 ((unsigned) P->sch.ivp.size ()), dim3 (256), 0, P->stream, d_ivp, P->d_relmap, P->d_invmap) ;
        }
        hipError_t e1 = hipGetLastError (), e2 = hipStreamSynchronize (P->stream) ;
        if (d_ivp) (void) hipFree (d_ivp) ;
        HIPCHK (e) ; HIPCHK (e1) ; HIPCHK (e2) ;
    }
    if (ptiming) fprintf (stderr, "cholmod_hip upload_plan: streams/events %.3f s, maps + schedule H2D %.3f s, hipMalloc (L %.1f GB, arena %.1f GB) %.3f s, relmap kernel %.3f s\n",
        tu1 - tu0, tu2 - tu1, 8e-9 * P->lx_local, 8e-9 * P->arena, tu3 - tu2, pnow () - tu3) ;
    return CHOLMOD_HIP_OK ;
}

// k_trsm's dynamic LDS exceeds the 64 KB default limit for 64-wide panels
static int raise_lds_limits ()
{
    static bool done = false ;
    if (done) return CHOLMOD_HIP_OK ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_trsm_mfma<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_trsm_mfma<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_trsm_mfma<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_trsm_upd<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_trsm_upd<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_rowsolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int) rowsolve_lds_bytes ())) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_chainf, hipFuncAttributeMaxDynamicSharedMemorySize, (int) chainf_lds_bytes ())) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_thin_front<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_thin_front<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    HIPCHK (hipFuncSetAttribute ((const void *) k_thin_front<4, false, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024)) ;
    done = true ;
    return CHOLMOD_HIP_OK ;
}

// waves per SIMD the one-wave thin-front kernel is compiled for, by size class (<= 32 / 48 / 64 rows): 4 / 4 / 3
// (measured on the 2D 1259^2 problem in round 2: 6 everywhere 1.044 ms, 4 / 4 / 3 1.004 ms; the knob and the other
// instantiations are gone)
static int thin_minw (int cls) { return cls == 2 ? 3 : 4 ; }

static int run_launch (cholmod_hip_plan *P, const Launch &L, bool serial)
{
    hipStream_t st = (serial || L.stream == 0 || !P->stream2) ? P->stream : P->stream2 ;
    const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;     // a complex factor in its own storage (device_util.hip.h: ldcx / stcx; CXS_LAUNCH)
    const bool twin = !cxs && (P->flags & CHOLMOD_HIP_PHI_TWIN) != 0 ;     // update kernels contract over the even columns
    const int tw = cxs ? 2 : twin ? 1 : 0 ;                         // the update kernels' TW (update_launch.hip.h: with_tw)
    // (test hook CHOLMOD_HIP_TEST_DROP_WAITS=1: the cross-stream waits of the schedule are skipped -- the mutation the jitter
    // test must catch, tests/test_gpu_scale.py::test_stream_jitter_catches_a_dropped_wait; =2: only the joins with the far-row
    // gathers of the shared fronts, tests/test_dist.py)
    const bool drop_wait = P->test_drop_waits == 1 || (P->test_drop_waits == 2 && L.kind == K_JOIN) ;
    if (!serial && L.wait_ev >= 0 && L.kind != K_XCHG_RS && !drop_wait) HIPCHK (hipStreamWaitEvent (st, P->sync_ev [L.wait_ev], 0)) ;
    if (P->jitter_us > 0 && !serial)
    {
        // test hook CHOLMOD_HIP_TEST_JITTER=seed[:max_us]: ahead of one launch in three, its stream is held up for a random
        // time (mostly tens of microseconds, now and then max_us): a launch whose input comes from the OTHER stream without
        // an event between them then runs before its producer -- with the arena and the windows poisoned that shows in
        // the factor (tests/test_dist.py, tools/dist_soak.py).  The schedule itself is what ships.
        P->jitter_state = P->jitter_state * 6364136223846793005ull + 1442695040888963407ull ;
        const unsigned r = (unsigned) (P->jitter_state >> 33) ;
        if (r % 3 == 0)
        {
            const unsigned u = (r >> 8) % 100 ;
            const long long us = u < 90 ? 5 + (long long) ((r >> 16) % 60) : (long long) ((r >> 16) % (unsigned) P->jitter_us) ;
            hipLaunchKernelGGL (k_spin, dim3 (1), dim3 (64), 0, st, us * 100) ;
        }
    }
    switch (L.kind)
    {
        case K_JOIN: break ;        // (no launch of its own: a cross-stream wait, done above)
        case K_SMALL:
            { int rl = raise_lds_limits () ; if (rl != CHOLMOD_HIP_OK) return rl ; }
            // fronts of <= 64 rows run one wave per front (lane = row, no cross-wave
            // hand-off), wider ones four
            {
                // tuning: per-phase shader cycles of one front per launch (CHOLMOD_HIP_THIN_TIMING)
                long long *tim = P->d_thin_tim ? P->d_thin_tim + 10 * (size_t) (&L - P->sch.launches.data ()) : nullptr ;
// (CX_: a complex factor in its own storage; it is never timed)
#define THIN_LAUNCH(NW_, TIMED_, MINW_, CX_) \
                hipLaunchKernelGGL ((k_thin_front<NW_, TIMED_, MINW_, CX_>), dim3 (L.grid), dim3 (64 * NW_), thin_front_lds_bytes (L.aux), st, \
                    P->d_sm + L.goff, P->d_smd + L.goff, P->d_sp01 + 2 * L.goff, P->d_cdesc, P->d_relmap, P->d_Ls, P->d_Sp, \
                    P->s_unpacked ? P->d_Snz : nullptr, P->d_Si, P->d_Sx, P->cur_beta, \
                    P->d_Lx, P->d_cb, P->d_info, L.aux, P->d_amap, P->cur_mapped, (TIMED_) ? tim : (long long *) nullptr)
                // complex storage: one wave per front up to 64 twin rows, four above
                if (cxs) { if (L.aux > 64) THIN_LAUNCH (4, false, 2, true) ; else THIN_LAUNCH (1, false, 4, true) ; }
                else if (L.leaf_pw && P->cur_mapped && !P->s_unpacked && !tim)
                {
                    // leaf fronts two to a wave, once the assembly map of the resident S exists
#define LEAF_LAUNCH(PW_, MINW_) \
                    hipLaunchKernelGGL ((k_leaf_pair<PW_, MINW_>), dim3 ((L.grid + 1) / 2), dim3 (64), (size_t) (2 * L.leaf_T + 128) * sizeof (double), st, \
                        P->d_sm + L.goff, L.grid, P->d_smd + L.goff, P->d_sp01 + 2 * L.goff, P->d_Sx, P->d_amap, P->cur_beta, P->d_Lx, P->d_cb, P->d_info, L.leaf_T)
#define LEAF_PW(MINW_) \
                    { if (L.leaf_pw <= 4) LEAF_LAUNCH (4, MINW_) ; else if (L.leaf_pw <= 8) LEAF_LAUNCH (8, MINW_) ; \
                      else if (L.leaf_pw <= 12) LEAF_LAUNCH (12, MINW_) ; else LEAF_LAUNCH (16, MINW_) ; }
                    // (measured on the 2D 1259^2 leaf level: 4 waves per SIMD 0.112 ms, 5: 0.191, 6: 0.245)
                    LEAF_PW (4)
#undef LEAF_PW
#undef LEAF_LAUNCH
                }
                else if (tim) { if (L.aux <= 64) THIN_LAUNCH (1, true, 4, false) ; else THIN_LAUNCH (4, true, 2, false) ; }
                else if (L.aux > 64) THIN_LAUNCH (4, false, 2, false) ;
                else
                {
                    // one wave per front: the register budget (waves per SIMD the compiler must
                    // allow) by size class -- the LDS of the wider classes caps the occupancy
                    // anyway (9.6 / 16.9 KB per front), and 80 registers spill
                    const int w = thin_minw (L.aux <= 32 ? 0 : L.aux <= 48 ? 1 : 2) ;
                    if (w == 3) THIN_LAUNCH (1, false, 3, false) ;
                    else THIN_LAUNCH (1, false, 4, false) ;
                }
#undef THIN_LAUNCH
            }
            break ;
        case K_XCHG_RS:
        case K_XCHG_AG:
            { const int rx = run_exchange (P, L, st, serial) ; if (rx != CHOLMOD_HIP_OK) return rx ; }
            break ;
        case K_CHAINF:
            { int rl = raise_lds_limits () ; if (rl != CHOLMOD_HIP_OK) return rl ; }
            hipLaunchKernelGGL (k_chainf, dim3 (L.grid), dim3 (256), chainf_lds_bytes (), st,
                P->d_cg + L.goff, L.ng, L.ndiag, P->d_Lx, P->d_info, P->d_dinv, P->d_cflags, P->d_cflags + 4 * (size_t) P->sch.ncflags) ;
            break ;
        case K_WIN:
            // (one-wave workgroups on the exchange stream: see k_extend_add)
            hipLaunchKernelGGL (k_win_move, dim3 (L.grid), dim3 (L.stream == 1 && !serial && narrow_xs () ? 64 : 256), 0, st, P->d_wg + L.goff, L.ng, P->d_Lx) ; break ;
        case K_ZERO:
            hipLaunchKernelGGL (k_zero, dim3 (L.grid), dim3 (256), 0, st,
                P->d_zg + L.goff, L.ng, P->d_cb) ; break ;
        case K_EA:
            CXS_LAUNCH (k_extend_add, dim3 (L.grid), dim3 (L.stream == 1 && !serial && narrow_xs () ? 64 : 256), 0, st,
                P->d_eg + L.goff, L.ng, P->d_fr, P->d_child, P->d_crel, P->d_relmap, P->d_Lx, P->d_cb, L.aux > 0 ? L.aux : EA_TW) ; break ;
        case K_POTRF:
            if (cxs) hipLaunchKernelGGL ((k_potrf_mfma<false, true>), dim3 (L.grid), dim3 (256), 0, st,
                P->d_pg + L.goff, P->d_Lx, P->d_info, (long long *) nullptr) ;
            else hipLaunchKernelGGL ((k_potrf_mfma<false, false>), dim3 (L.grid), dim3 (256), 0, st,
                P->d_pg + L.goff, P->d_Lx, P->d_info, (long long *) nullptr) ;
            break ;
        case K_TRSM:
            { int rl = raise_lds_limits () ; if (rl != CHOLMOD_HIP_OK) return rl ; }
            if (cxs) hipLaunchKernelGGL ((k_trsm_mfma<false, true>), dim3 (L.grid), dim3 (256), trsm_mfma_lds_bytes (L.aux), st,
                P->d_tg + L.goff, L.ng, P->d_Lx, P->d_info, L.aux, (long long *) nullptr) ;
            else hipLaunchKernelGGL ((k_trsm_mfma<false, false>), dim3 (L.grid), dim3 (256), trsm_mfma_lds_bytes (L.aux), st,
                P->d_tg + L.goff, L.ng, P->d_Lx, P->d_info, L.aux, (long long *) nullptr) ;
            break ;
        case K_TRSM_UPD:
            { int rl = raise_lds_limits () ; if (rl != CHOLMOD_HIP_OK) return rl ; }
            CXS_LAUNCH (k_trsm_upd, dim3 (L.grid), dim3 (256), trsm_upd_lds_bytes (), st,
                P->d_tg + L.goff, L.ng, P->d_Lx, P->d_info, P->d_tu_cnt + L.goff) ;
            break ;
        case K_UPD_BIG:
            hipLaunchKernelGGL ((k_update2<BIG, BIG, BKK, 2, false>), dim3 (L.grid), dim3 (256), 0, st,
                P->d_gg + L.goff, L.ng, P->d_Lx, P->d_cb) ;
            break ;
        case K_UPD_SMALL:
            with_tw (tw, [&] (auto TW)
            {
                hipLaunchKernelGGL ((k_update2<SMALL, SMALL, BKK, 2, false, decltype (TW)::value>), dim3 (L.grid), dim3 (256), 0, st,
                    P->d_gg + L.goff, L.ng, P->d_Lx, P->d_cb) ;
            }) ;
            break ;
        case K_DIAG:
            hipLaunchKernelGGL (k_diag<false>, dim3 (L.grid), dim3 (256), 0, st, P->d_dg + L.goff, P->d_Lx, P->d_info, P->d_dinv, (long long *) nullptr) ;
            break ;
        case K_ROWSOLVE:
            { int rl = raise_lds_limits () ; if (rl != CHOLMOD_HIP_OK) return rl ; }
            hipLaunchKernelGGL (k_rowsolve, dim3 (L.grid), dim3 (256), rowsolve_lds_bytes (), st,
                P->d_rg + L.goff, L.ng, P->d_Lx, P->d_info, P->d_dinv) ;
            break ;
        case K_UPD_W:
            {
                // (a fused launch: a region takes its children's contribution-block entries with it, k_update3f)
                const Upd3Fuse fz {P->d_gfz ? P->d_gfz + L.goff : nullptr, P->d_fz, P->d_cdesc, P->d_invmap} ;
                const int rl = launch_update3 (st, P->d_gg + L.goff, L.ng, P->d_Lx, P->d_cb,
                    Upd3Shape {L.grid, L.aux, L.half != 0, P->upd3_wg4, tw}, L.fused ? &fz : nullptr) ;
                if (rl != CHOLMOD_HIP_OK) return rl ;
            }
            break ;
        case K_UPD_G:
            // head updates over the rows their heads reach (schedule_dense.hip: add_head_gathered), sized as K_UPD_W
            {
                const int rl = launch_update3g (st, P->d_xg + L.goff, L.ng, P->d_gmap, P->d_Lx, P->d_cb,
                    Upd3Shape {L.grid, L.aux, L.half != 0, P->upd3_wg4, tw}) ;
                if (rl != CHOLMOD_HIP_OK) return rl ;
            }
            break ;
        case K_UPD_PF:
            with_tw (tw, [&] (auto TW)
            {
                hipLaunchKernelGGL ((k_update2f<decltype (TW)::value>), dim3 (L.grid), dim3 (256), 0, st,
                    P->d_gg + L.goff, L.ng, P->d_Lx, P->d_cb, P->d_info) ;
            }) ;
            break ;
    }
    if (!serial && L.rec_ev >= 0) HIPCHK (hipEventRecord (P->sync_ev [L.rec_ev], st)) ;
    return CHOLMOD_HIP_OK ;
}

/* host side: until the caller has pushed chunk c (cholmod_hip_values_push_chunk); an error if it cancelled */
static int wait_pushed (cholmod_hip_plan *P, long c)
{
    for (long spin = 0 ; ; spin++)
    {
        const long have = P->chunks_pushed.load (std::memory_order_acquire) ;
        if (have < 0) return CHOLMOD_HIP_GPU_PROBLEM ;
        if (have > c) return CHOLMOD_HIP_OK ;
        if ((spin & 1023) == 1023) std::this_thread::yield () ;
    }
}

/* the chunks 0 .. need-1 into S and L, on the main stream, as soon as each has been pushed and copied */
static int apply_value_chunks (cholmod_hip_plan *P, long need)
{
    while (P->chunks_applied < need)
    {
        const long c = P->chunks_applied ;
        const int rw = wait_pushed (P, c) ;
        if (rw != CHOLMOD_HIP_OK) return rw ;
        HIPCHK (hipStreamWaitEvent (P->stream, P->chunk_ev [c], 0)) ;
        const i64 k0 = c * P->chunk_len, k1 = std::min<i64> (k0 + P->chunk_len, P->s_cur_nz) ;
        hipLaunchKernelGGL (k_values_chunk, dim3 ((unsigned) ((k1 - k0 + 255) / 256)), dim3 (256), 0, P->stream,
            k0, k1, P->d_vorder, P->d_vals, P->d_amap, P->d_Sx, P->d_Lx) ;
        P->chunks_applied = c + 1 ;
    }
    return CHOLMOD_HIP_OK ;
}

} // namespace

// what values.hip calls (engine_internal.hip.h)
namespace sship {

/* What a factorization enqueues before it touches a value: the start event, (re)allocation of what a gather released, the
 * clearing of L and of the per-factorization counters.  cholmod_hip_values_begin calls it ahead of time, so that the
 * clearing runs beside the upload of the values. */
int factorize_prologue (cholmod_hip_plan *P)
{
    hipStream_t st = P->stream ;
    P->winv_valid = false ;                 // the diagonal-block inverses follow the factor
    P->si_valid = P->fg_valid = false ; P->factor_state = 0 ;     // ... and so do the selected inverse and the factor gradient
    HIPCHK (hipEventRecord (P->ev0, st)) ;
    // Lx := 0 (several ranks: the rank's own fronts -- its d_Lx holds nothing else); the complete
    // factor a gather may have left in d_Lx_full is stale from here on
    P->full_valid = false ;
    if (!P->d_Lx)
    {
        // (the gather went through the host and released the rank's own array: cholmod_hip_gather_factor)
        if (P->d_Lx_full) { (void) hipFree (P->d_Lx_full) ; P->d_Lx_full = nullptr ; }
        HIPCHK (hipMalloc ((void **) &P->d_Lx, (std::max<i64> (P->lx_local, 1) + UPD3_LX_PAD) * sizeof (double))) ;
    }
    if (!P->d_cb)
    {
        // (the arena made room for the gathered factor, see cholmod_hip_gather_factor)
        if (hipMalloc ((void **) &P->d_cb, std::max<i64> (P->arena, 1) * sizeof (double)) != hipSuccess)
        {
            (void) hipGetLastError () ;
            if (P->d_Lx_full) { (void) hipFree (P->d_Lx_full) ; P->d_Lx_full = nullptr ; }
            HIPCHK (hipMalloc ((void **) &P->d_cb, std::max<i64> (P->arena, 1) * sizeof (double))) ;
        }
    }
    // test hook CHOLMOD_HIP_TEST_POISON_ARENA=1: the contribution-block arena (and the exchange staging) start every
    // factorization as NaNs -- an entry somebody reads before anybody has written it then shows in the factor,
    // whatever a fresh allocation happens to hold (tests/test_gpu_parity.py, tests/test_dist.py)
    const bool poison = TEST_ENV ("CHOLMOD_HIP_TEST_POISON_ARENA") != nullptr ;
    if (poison)
    {
        HIPCHK (hipMemsetAsync (P->d_cb, 0xFF, std::max<i64> (P->arena, 1) * sizeof (double), st)) ;
        if (P->d_stage) HIPCHK (hipMemsetAsync (P->d_stage, 0xFF, (size_t) P->stage_len * sizeof (double), st)) ;
        if (P->lx_local > P->lx_fronts) HIPCHK (hipMemsetAsync (P->d_Lx + P->lx_fronts, 0xFF, (size_t) (P->lx_local - P->lx_fronts) * sizeof (double), st)) ;
        if (P->d_ag) HIPCHK (hipMemsetAsync (P->d_ag, 0xFF, (size_t) P->ag_len * sizeof (double), st)) ;
        if (P->d_agf) HIPCHK (hipMemsetAsync (P->d_agf, 0xFF, (size_t) P->agf_len * sizeof (double), st)) ;
        // (... and the padding behind L that partial tiles of k_update3 may read -- into accumulators nobody stores: a NaN
        // that reaches the factor from there shows in every poisoned parity test; round-5 advisor)
        HIPCHK (hipMemsetAsync (P->d_Lx + std::max<i64> (P->lx_local, 1), 0xFF, (size_t) UPD3_LX_PAD * sizeof (double), st)) ;
    }
    HIPCHK (hipMemsetAsync (P->d_Lx, 0, std::max<i64> (poison ? P->lx_fronts : P->lx_local, 1) * sizeof (double), st)) ;
    HIPCHK (hipMemsetAsync (P->d_info, 0, std::max<i64> (P->nsuper, 1) * sizeof (i32), st)) ;
    HIPCHK (hipMemsetAsync (P->d_tu_cnt, 0, std::max<size_t> (P->sch.tg.size (), 1) * sizeof (i32), st)) ;
    if (P->d_cflags) HIPCHK (hipMemsetAsync (P->d_cflags, 0, (4 * (size_t) P->sch.ncflags + 4) * sizeof (int), st)) ;
    return CHOLMOD_HIP_OK ;
}

// Run the numeric factorization on the resident S.  Leaves Lx on the device.
int run_factorize (cholmod_hip_plan *P, double beta, int quick, i64 *minor)
{
    hipStream_t st = P->stream ;
    const bool cxs = (P->flags & CHOLMOD_HIP_CX_STORAGE) != 0 ;
    if (!P->d_Sp) return CHOLMOD_HIP_INVALID ;
    bool prof = P->profiling ;
    static const bool host_timing = getenv ("CHOLMOD_HIP_HOST_TIMING") != nullptr ;
    auto now = [] () { return std::chrono::duration<double> (std::chrono::steady_clock::now ().time_since_epoch ()).count () ; } ;
    double th0 = now () ;
    P->cur_beta = beta ;
    P->cur_mapped = P->amap_valid ? 1 : 0 ;     // thin fronts: A through the map the first assembly recorded
    size_t nl = P->sch.launches.size () ;
    if (prof)
    {
        while (P->evpool.size () < 2 * (nl + 1))
        {
            hipEvent_t e ; HIPCHK (hipEventCreate (&e)) ; P->evpool.push_back (e) ;
        }
    }
    int poisoned = CHOLMOD_HIP_OK ;
    bool building_map = false ;
    if (prof) HIPCHK (hipEventRecord (P->evpool [0], st)) ;
    const bool begun = P->values_begun, chunked = begun && P->values_in_batch_order ;
    P->values_begun = false ;
    if (!begun)
    {
        const int rp = factorize_prologue (P) ;
        if (rp != CHOLMOD_HIP_OK) return rp ;
    }
    else if (!chunked && P->nchunks > 0)
    {
        // (cholmod_hip_values_begin in S order: the push of the last chunk gathers the new values into S on the exchange
        // stream; the clearing of L ran beside their upload, the assembly is the first to read them)
        const int rw = wait_pushed (P, P->nchunks - 1) ;
        if (rw != CHOLMOD_HIP_OK) return rw ;
        HIPCHK (hipStreamWaitEvent (st, P->chunk_ev [P->nchunks - 1], 0)) ;
    }
    if (chunked)
    {
        // (in batch order: the diagonal shift first, every chunk is added into the cleared L right before the first launch
        // of the first batch that needs it)
        if (beta != 0.0 && P->n > 0)
            hipLaunchKernelGGL (k_add_beta<false>, dim3 ((unsigned) ((P->n + 255) / 256)), dim3 (256), 0, st,
                P->n, P->d_supermap, P->d_fr, P->d_Lx, beta) ;
    }
    else if (P->n > 0 && P->amap_valid)
    {
        // the resident S was assembled before: stream it through its map
        if (P->s_nz > 0)
            hipLaunchKernelGGL (k_assemble_mapped, dim3 ((unsigned) ((P->s_nz + 255) / 256)), dim3 (256), 0, st,
                P->s_nz, P->d_amap, P->d_Sx, P->d_Lx) ;
        if (beta != 0.0)
            CXS_LAUNCH (k_add_beta, dim3 ((unsigned) ((P->n + 255) / 256)), dim3 (256), 0, st,
                P->n, P->d_supermap, P->d_fr, P->d_Lx, beta) ;
    }
    else if (P->n > 0)
    {
        HIPCHK (hipMemsetAsync (P->d_amap, 0xFF, std::max<i64> (P->s_nz, 1) * sizeof (i64), st)) ;     // -1: not in L
        CXS_LAUNCH (k_assemble, dim3 ((unsigned) ((P->n + 255) / 256)), dim3 (256), 0, st,
            P->n, P->d_Sp, P->s_unpacked ? P->d_Snz : nullptr, P->d_Si, P->d_Sx,
            P->d_supermap, P->d_fr, P->d_Ls, P->d_Lx, beta, P->d_amap) ;
        building_map = true ;       // (the thin-front kernels record their part; valid once every launch has run)
    }
    if (prof) HIPCHK (hipEventRecord (P->evpool [1], st)) ;
    int fail_rank = -1 ; long fail_launch = -1 ;
    if (const char *e = TEST_ENV ("CHOLMOD_HIP_TEST_FAIL_LAUNCH")) (void) sscanf (e, "%d:%ld", &fail_rank, &fail_launch) ;
    P->prog_fact = P->prog_fact + 1 ; P->prog_launch = 0 ; P->prog_xchg_enq = 0 ;
    for (size_t q = 0 ; q < nl ; q++)
    {
        const Launch &L = P->sch.launches [q] ;
        P->prog_launch = (long long) q + 1 ;
        if (chunked)
        {
            const int rv = apply_value_chunks (P, P->launch_need_chunks [q]) ;
            if (rv != CHOLMOD_HIP_OK) return rv ;
        }
        if (prof && poisoned == CHOLMOD_HIP_OK) HIPCHK (hipEventRecord (P->evpool [2 * (q + 1)], st)) ;
        if (poisoned != CHOLMOD_HIP_OK)
        {
            // A launch of this rank failed.  The other ranks of its groups are about to
            // block in the collectives that follow: keep taking part in them (the data no
            // longer matters) and report the failure through the agreement exchange at
            // the end, so that every rank returns an error instead of hanging.
            if (L.kind == K_XCHG_RS || L.kind == K_XCHG_AG) (void) run_launch (P, L, true) ;
            continue ;
        }
        int rl = run_launch (P, L, prof) ;
        // test hook "rank:launch": that launch of that rank reports a failure
        if (fail_rank == P->rank && fail_launch == (long) q) rl = CHOLMOD_HIP_GPU_PROBLEM ;
        if (rl != CHOLMOD_HIP_OK)
        {
            if (P->world == 1) return rl ;
            poisoned = rl ;
            continue ;
        }
        if (prof) HIPCHK (hipEventRecord (P->evpool [2 * (q + 1) + 1], st)) ;
    }
    if (chunked)
    {
        // (whatever the schedule did not ask for -- nothing, normally -- so that the resident S is complete)
        const int rv = apply_value_chunks (P, P->nchunks) ;
        if (rv != CHOLMOD_HIP_OK) return rv ;
    }
    if (poisoned == CHOLMOD_HIP_OK && hipGetLastError () != hipSuccess) poisoned = CHOLMOD_HIP_GPU_PROBLEM ;
    if (poisoned != CHOLMOD_HIP_OK && P->world == 1) return poisoned ;
    (void) hipEventRecord (P->ev1, st) ;
    double th1 = now () ;
    // not-positive-definite protocol (t_cholmod_super_numeric.c:905-968): the first
    // failing supernode and its info, reduced on the device
    float ms = 0 ;
    i64 sbad = -1, binfo = 0 ;
    if (poisoned == CHOLMOD_HIP_OK)
    {
        int first = (int) P->nsuper ;
        i32 inf = 0 ;
        bool ok = hipMemcpyAsync (P->d_first_fail, &first, sizeof (int), hipMemcpyHostToDevice, st) == hipSuccess ;
        if (ok && P->nsuper > 0)
            hipLaunchKernelGGL (k_first_fail, dim3 ((unsigned) ((P->nsuper + 255) / 256)), dim3 (256), 0, st,
                P->nsuper, P->d_info, P->d_first_fail) ;
        // (k_chainf: a workgroup that waited longer than its budget for another one's flag says so here)
        int chain_err = 0 ;
        if (P->sch.ncflags > 0)
            ok = ok && hipMemcpyAsync (&chain_err, P->d_cflags + 4 * (size_t) P->sch.ncflags, sizeof (int), hipMemcpyDeviceToHost, st) == hipSuccess ;
        ok = ok && hipMemcpyAsync (&first, P->d_first_fail, sizeof (int), hipMemcpyDeviceToHost, st) == hipSuccess
            && hipStreamSynchronize (st) == hipSuccess
            && hipEventElapsedTime (&ms, P->ev0, P->ev1) == hipSuccess ;
        if (ok && first < (int) P->nsuper)
        {
            ok = hipMemcpy (&inf, P->d_info + first, sizeof (i32), hipMemcpyDeviceToHost) == hipSuccess ;
            sbad = first ; binfo = inf ;
        }
        if (chain_err != 0)
        {
            fprintf (stderr, "cholmod_hip: k_chainf: a workgroup waited for a flag beyond its budget (hand-off between workgroups failed)\n") ;
            ok = false ;
        }
        if (!ok)
        {
            if (P->world == 1) return CHOLMOD_HIP_GPU_PROBLEM ;
            poisoned = CHOLMOD_HIP_GPU_PROBLEM ;
        }
        else if (building_map) P->amap_valid = true ;
    }
    double th2 = now () ;
    if (host_timing)
        fprintf (stderr, "cholmod_hip: host enqueue %.3f ms, wait+info copy %.3f ms, device %.3f ms, %zu launches\n",
            1e3 * (th1 - th0), 1e3 * (th2 - th1), (double) ms, nl) ;
    double *S = P->stats ;
    for (int q = 0 ; q < CHOLMOD_HIP_NSTATS ; q++) S [q] = 0 ;
    S [0] = ms * 1e-3 ;
    S [1] = P->exec_flops ;
    S [2] = (double) nl + 3 ;
    S [3] = P->nlevels ;
    S [4] = 8.0 * P->arena ;
    S [5] = 8.0 * P->xsize ;
    S [36] = 8.0 * P->lx_local ;
    exchange_volume (P, S) ;
    for (size_t q = 0 ; q < nl ; q++)
    {
        const Launch &L = P->sch.launches [q] ;
        if (L.kind == K_UPD_SMALL) { S [7] += 1 ; S [8] += L.flops ; S [16] += L.bytes ; }
        if (L.kind == K_UPD_W || L.kind == K_UPD_G) { S [33] += 1 ; S [34] += L.flops ; S [35] += L.bytes ; }
        if (L.kind == K_UPD_G) S [40] += L.skipped ;
        if (L.kind == K_UPD_PF) { S [26] += 1 ; S [28] += L.flops ; S [29] += L.bytes ; }
        if (L.kind == K_TRSM_UPD) S [31] += 1 ;
        if (L.kind == K_SMALL) { S [20] += L.bytes ; S [21] += L.ng ; }
        S [22] = P->nsplit ;
        if (L.kind == K_UPD_BIG) { S [15] += L.flops ; }
        if (L.kind == K_EA) S [10] += L.bytes ;
        if (L.kind == K_WIN)
            for (int w = 0 ; w < L.ng ; w++)
            {
                const WinD &Wd = P->sch.wg [L.goff + w] ;
                if (Wd.mode == 0) { S [37] += 1 ; if (Wd.win < 0) S [38] += 1 ; }
            }
    }
    if (prof && poisoned == CHOLMOD_HIP_OK)
    {
        float t = 0 ;
        HIPCHK (hipEventElapsedTime (&t, P->evpool [0], P->evpool [1])) ;
        S [13] = t * 1e-3 ;
        P->launch_ms.assign (nl, 0.0f) ;
        for (size_t q = 0 ; q < nl ; q++)
        {
            const Launch &L = P->sch.launches [q] ;
            HIPCHK (hipEventElapsedTime (&t, P->evpool [2 * (q + 1)], P->evpool [2 * (q + 1) + 1])) ;
            P->launch_ms [q] = t ;
            double sec = t * 1e-3 ;
            switch (L.kind)
            {
                case K_UPD_SMALL: S [6] += sec ; if (L.aux < MB) { S [23] += sec ; } break ;
                case K_UPD_PF: S [27] += sec ; break ;
                case K_UPD_W: case K_UPD_G: S [32] += sec ; break ;
                case K_UPD_BIG: S [14] += sec ; break ;
                case K_EA: case K_ZERO: case K_WIN: S [9] += sec ; break ;
                case K_POTRF: case K_DIAG: case K_CHAINF: S [11] += sec ; break ;
                case K_ROWSOLVE: S [12] += sec ; break ;
                case K_SMALL: S [19] += sec ; break ;
                case K_TRSM: S [12] += sec ; break ;
                case K_TRSM_UPD: S [30] += sec ; break ;
            }
        }
    }
    if (P->world > 1 || P->force_shared)
    {
        const int ra = agree_first_fail (P, poisoned, &sbad, &binfo) ;
        if (ra != CHOLMOD_HIP_OK) return ra ;
    }
    *minor = P->n ;
    P->factor_state = sbad < 0 ? 1 : 2 ;
    if (sbad < 0) return CHOLMOD_HIP_OK ;
    const FrontD &f = P->fr [sbad] ;
    *minor = f.k1 + binfo - 1 ;
    // everything from supernode sbad + 1 on (from sbad itself when it has no valid column, or on
    // a quick return) is zero: in the rank's own array, the fronts it holds with those indices
    // (held fronts are packed in supernode order, so that is one tail of the array)
    i64 first_zero = sbad + ((binfo == 1 || quick) ? 0 : 1) ;
    i64 zero_from = P->lx_fronts ;
    for (i64 q = first_zero ; q < P->nsuper ; q++) if (P->lpx [q] >= 0) { zero_from = P->lpx [q] ; break ; }
    if (zero_from < P->lx_fronts)
        HIPCHK (hipMemsetAsync (P->d_Lx + zero_from, 0, (P->lx_fronts - zero_from) * sizeof (double), st)) ;
    HIPCHK (hipStreamSynchronize (st)) ;
    return CHOLMOD_HIP_NOT_POSDEF ;
}

} // namespace sship

// ============================================================================
// extern "C" shim
// ============================================================================

extern "C" {

const char *cholmod_hip_version (void) { return "suitesparse_amd cholmod_hip 0.1 (gfx950)" ; }

int cholmod_hip_probe (void)
{
    int cnt = 0 ;
    if (hipGetDeviceCount (&cnt) != hipSuccess) return 0 ;
    return cnt > 0 ? 1 : 0 ;
}

int cholmod_hip_device_count (int *count)
{
    if (!count) return CHOLMOD_HIP_INVALID ;
    *count = 0 ;
    int cnt = 0 ;
    if (hipGetDeviceCount (&cnt) != hipSuccess) { (void) hipGetLastError () ; return CHOLMOD_HIP_NO_DEVICE ; }
    *count = cnt ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_memorysize (size_t *total_mem, size_t *available_mem)
{
    if (total_mem) *total_mem = 0 ;
    if (available_mem) *available_mem = 0 ;
    if (!cholmod_hip_probe ()) return 1 ;
    size_t f = 0, t = 0 ;
    if (hipMemGetInfo (&f, &t) != hipSuccess) return 1 ;
    if (total_mem) *total_mem = t ;
    if (available_mem) *available_mem = f ;
    return 0 ;
}

int cholmod_hip_set_device (int device)
{
    return hipSetDevice (device) == hipSuccess ? CHOLMOD_HIP_OK : CHOLMOD_HIP_NO_DEVICE ;
}

static cholmod_hip_plan *plan_create_impl (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px, const int64_t *s,
    int flags, int rank, int world, int *status, const int64_t *reach_p = nullptr, const int32_t *reach_first = nullptr) ;

cholmod_hip_plan *cholmod_hip_plan_create_dist (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px, const int64_t *s,
    int flags, int rank, int world, int *status)
{
    int st_local ;
    if (!status) status = &st_local ;
    // the plan builder works in C++ containers: their allocation failures end here, as a status, not in the caller's C frames
    try { return plan_create_impl (n, nsuper, super, pi, px, s, flags, rank, world, status) ; }
    catch (const std::bad_alloc &) { *status = CHOLMOD_HIP_OUT_OF_MEMORY ; return nullptr ; }
}

cholmod_hip_plan *cholmod_hip_plan_create_reach (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px, const int64_t *s,
    int flags, const int64_t *reach_p, const int32_t *reach_first, int *status)
{
    int st_local ;
    if (!status) status = &st_local ;
    try { return plan_create_impl (n, nsuper, super, pi, px, s, flags, 0, 1, status, reach_p, reach_first) ; }
    catch (const std::bad_alloc &) { *status = CHOLMOD_HIP_OUT_OF_MEMORY ; return nullptr ; }
}

static cholmod_hip_plan *plan_create_impl (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px, const int64_t *s,
    int flags, int rank, int world, int *status, const int64_t *reach_p, const int32_t *reach_first)
{
    *status = CHOLMOD_HIP_OK ;
    if (n < 0 || nsuper < 0 || !super || !pi || !px || !s || world < 1 || rank < 0 || rank >= world)
    { *status = CHOLMOD_HIP_INVALID ; return nullptr ; }
    // front descriptors, relative maps and the supernode map are 32-bit on the device
    if (n > INT32_MAX || nsuper > INT32_MAX) { *status = CHOLMOD_HIP_TOO_LARGE ; return nullptr ; }
    bool host_only = (flags & CHOLMOD_HIP_PLAN_HOST_ONLY) != 0 ;
    if (!host_only && !cholmod_hip_probe ()) { *status = CHOLMOD_HIP_NO_DEVICE ; return nullptr ; }
    const double tpc = std::chrono::duration<double> (std::chrono::steady_clock::now ().time_since_epoch ()).count () ;
    if (flags & CHOLMOD_HIP_CX_STORAGE)
    {
        // complex storage: the twin's index space, the generic kernels only (the LDS-resident thin-front
        // kernels and the 256-column chain have no complex-storage form), one rank
        if (world > 1) { if (status) *status = CHOLMOD_HIP_INVALID ; return nullptr ; }
        // (round 4: the thin-front kernel has a complex-storage form, k_thin_front<..., CX>; CHOLMOD_HIP_CX_NO_THIN=1: the
        // generic kernels for every front, as before)
        flags |= CHOLMOD_HIP_PHI_TWIN ;
        if (getenv ("CHOLMOD_HIP_CX_NO_THIN")) flags |= CHOLMOD_HIP_NO_SMALL_FRONTS ;
        flags &= ~(CHOLMOD_HIP_CHAIN256 | CHOLMOD_HIP_TILE128) ;
    }
    if (flags & CHOLMOD_HIP_PHI_TWIN)
    {
        // a twin has every supernode boundary and row in (2i, 2i+1) pairs
        bool ok = (n % 2 == 0) ;
        for (i64 q = 0 ; ok && q <= nsuper ; q++) ok = (super [q] % 2 == 0) && (pi [q] % 2 == 0) ;
        for (i64 q = 0 ; ok && q + 1 < pi [nsuper] ; q += 2) ok = (s [q] % 2 == 0) && (s [q + 1] == s [q] + 1) ;
        if (!ok) { if (status) *status = CHOLMOD_HIP_INVALID ; return nullptr ; }
    }
    // (the plan is allocated only once the flags and the twin structure are known to be valid:
    // nothing to release on the early returns above)
    cholmod_hip_plan *P = new (std::nothrow) cholmod_hip_plan ;
    if (!P) { *status = CHOLMOD_HIP_OUT_OF_MEMORY ; return nullptr ; }
    // (whatever way this function is left without handing P over -- a failed step, a std::bad_alloc on its way to the
    // caller's catch -- the plan and what it holds on the device are released)
    struct Guard { cholmod_hip_plan *P ; ~Guard () { if (P) { free_device (P) ; delete P ; } } } guard {P} ;
    P->n = n ; P->nsuper = nsuper ; P->flags = flags ; P->host_only = host_only ;
    P->rank = rank ; P->world = world ;
    P->super.assign (super, super + nsuper + 1) ;
    P->pi.assign (pi, pi + nsuper + 1) ;
    P->px.assign (px, px + nsuper + 1) ;
    P->ssize = pi [nsuper] ; P->xsize = px [nsuper] ;
    P->Ls.assign (s, s + std::max<i64> (P->ssize, 1)) ;
    if (reach_p && reach_first)
    {
        // (a front the analysis looked at has one entry per row of its row list, the others none)
        for (i64 q = 0 ; q < nsuper ; q++)
        {
            const i64 len = reach_p [q + 1] - reach_p [q] ;
            if (len < 0 || (len != 0 && len != pi [q + 1] - pi [q])) { *status = CHOLMOD_HIP_INVALID ; return nullptr ; }
        }
        P->reach_p.assign (reach_p, reach_p + nsuper + 1) ;
        P->reach_first.assign (reach_first + reach_p [0], reach_first + reach_p [nsuper]) ;
        for (i64 &v : P->reach_p) v -= reach_p [0] ;
    }
    // memory budget of the contribution-block arena (see build_host): what is left
    // of the HBM next to L and the index maps.  Several ranks must derive the same
    // schedule, so they use a nominal capacity instead of their momentary free
    // memory.  CHOLMOD_HIP_ARENA_BUDGET_MB overrides (tests, tuning).
    {
        const char *e = getenv ("CHOLMOD_HIP_ARENA_BUDGET_MB") ;
        double fixed = 8.0 * P->xsize + 8.0 * P->ssize + 4.0 * (P->ssize - n) + 3e9 ;
        if (e && atof (e) > 0) P->arena_budget = (i64) (atof (e) * 1048576.0) ;
        else if (world > 1) P->arena_budget = -1 ;         // (build_host: from the largest part of L any rank holds)
        else if (!host_only)
        {
            size_t freeb = 0, totalb = 0 ;
            if (hipMemGetInfo (&freeb, &totalb) == hipSuccess)
                P->arena_budget = (i64) std::max (1e9, (double) freeb - fixed) ;
        }
    }
    const bool ptiming = getenv ("CHOLMOD_HIP_PLAN_TIMING") != nullptr ;
    auto pnow = [] () { return std::chrono::duration<double> (std::chrono::steady_clock::now ().time_since_epoch ()).count () ; } ;
    double tp0 = pnow () ;
    *status = build_host (P) ;
    double tp1 = pnow () ;
    if (*status == CHOLMOD_HIP_OK && !host_only) *status = upload_plan (P) ;
    if (ptiming) fprintf (stderr, "cholmod_hip_plan_create: copy maps %.3f s, build_host %.3f s, upload_plan %.3f s\n",
        tp0 - tpc, tp1 - tp0, pnow () - tp1) ;
    if (*status != CHOLMOD_HIP_OK) return nullptr ;
    guard.P = nullptr ;
    return P ;
}

cholmod_hip_plan *cholmod_hip_plan_create (int64_t n, int64_t nsuper,
    const int64_t *super, const int64_t *pi, const int64_t *px, const int64_t *s,
    int flags, int *status)
{
    return cholmod_hip_plan_create_dist (n, nsuper, super, pi, px, s, flags, 0, 1, status) ;
}

int cholmod_hip_get_groups (cholmod_hip_plan *P, int64_t *first, int64_t *size)
{
    if (!P || !first || !size) return CHOLMOD_HIP_INVALID ;
    for (i64 q = 0 ; q < P->nsuper ; q++) { first [q] = P->grp0 [q] ; size [q] = P->grpn [q] ; }
    return CHOLMOD_HIP_OK ;
}

/* test hook: the (contributor, ancestor) pairs of this rank's plan -- front d extend-adds into the windows of the shared
 * front a through a map of its own (contributions routed past the contribution blocks in between); and per front the block
 * [cb_lo, cb_hi) of contribution-block columns this rank stores (-1, -1: the whole block, or not held).  Returns the number of
 * pairs; fills at most cap of them. */
int64_t cholmod_hip_debug_routing (cholmod_hip_plan *P, int64_t cap, int64_t *pair_d, int64_t *pair_a, int64_t *cb_lo, int64_t *cb_hi)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    for (size_t q = 0 ; q < P->relpairs.size () && (i64) q < cap ; q++)
    {
        if (pair_d) pair_d [q] = P->relpairs [q].d ;
        if (pair_a) pair_a [q] = P->relpairs [q].a ;
    }
    for (i64 s = 0 ; s < P->nsuper ; s++)
    {
        const FrontD &f = P->fr [s] ;
        if (cb_lo) cb_lo [s] = f.cbd ? f.cb_lo : -1 ;
        if (cb_hi) cb_hi [s] = f.cbd ? f.cb_hi : -1 ;
    }
    return (int64_t) P->relpairs.size () ;
}

int64_t cholmod_hip_get_batches (cholmod_hip_plan *P, int64_t *batch_of, int64_t *global_arena)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    if (batch_of) for (i64 q = 0 ; q < P->nsuper ; q++) batch_of [q] = P->batch_of [q] ;
    if (global_arena) *global_arena = P->global_arena ;
    return P->nsplit ;
}

int cholmod_hip_get_partition (cholmod_hip_plan *P, int64_t *owner)
{
    if (!P || !owner) return CHOLMOD_HIP_INVALID ;
    for (i64 q = 0 ; q < P->nsuper ; q++) owner [q] = P->owner [q] ;
    return CHOLMOD_HIP_OK ;
}

void cholmod_hip_plan_destroy (cholmod_hip_plan *P)
{
    if (!P) return ;
    free_device (P) ;
    delete P ;
}

int cholmod_hip_factorize_resident (cholmod_hip_plan *P, double beta,
    int quick_return_if_not_posdef, int64_t *minor)
{
    if (!P || P->host_only) return CHOLMOD_HIP_INVALID ;
    i64 m = P->n ;
    int rc = run_factorize (P, beta, quick_return_if_not_posdef, &m) ;
    if (minor) *minor = m ;
    return rc ;
}

int cholmod_hip_download_factor (cholmod_hip_plan *P, double *Lx_host)
{
    if (!P || P->host_only || !Lx_host) return CHOLMOD_HIP_INVALID ;
    const double *Lw = whole_factor (P) ;
    if (!Lw) return CHOLMOD_HIP_INVALID ;           // several ranks: cholmod_hip_gather_factor first
    HIPCHK (hipMemcpy (Lx_host, Lw, P->xsize * sizeof (double), hipMemcpyDeviceToHost)) ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_upload_factor (cholmod_hip_plan *P, const double *Lx_host)
{
    if (!P || P->host_only || !Lx_host) return CHOLMOD_HIP_INVALID ;
    double *Lw = P->d_Lx ;
    if (P->world > 1)
    {
        // several ranks: the complete factor lives beside the rank's own part
        if (!P->d_Lx_full) HIPCHK (hipMalloc ((void **) &P->d_Lx_full, std::max<i64> (P->xsize, 1) * sizeof (double))) ;
        if (!P->d_fr_full)
        {
            std::vector<FrontD> ff (P->fr) ;
            for (i64 q = 0 ; q < P->nsuper ; q++) { ff [q].psx = P->px [q] ; ff [q].own_w = 0 ; ff [q].own_g = 1 ; ff [q].own_r = 0 ; }
            hipError_t e ;
            P->d_fr_full = dupload (ff, e) ; HIPCHK (e) ;
        }
        Lw = P->d_Lx_full ;
    }
    HIPCHK (hipMemcpy (Lw, Lx_host, P->xsize * sizeof (double), hipMemcpyHostToDevice)) ;
    P->winv_valid = false ;
    P->si_valid = P->fg_valid = false ; P->factor_state = 1 ;
    P->full_valid = P->world > 1 ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_factorize (cholmod_hip_plan *P, const int64_t *Sp, const int64_t *Si,
    const int64_t *Snz, const double *Sx, double beta, int quick_return_if_not_posdef,
    double *Lx_host, int64_t *minor)
{
    int rc = cholmod_hip_upload_matrix (P, Sp, Si, Snz, Sx) ;
    if (rc != CHOLMOD_HIP_OK) return rc ;
    rc = cholmod_hip_factorize_resident (P, beta, quick_return_if_not_posdef, minor) ;
    if (rc < 0) return rc ;
    if (Lx_host)
    {
        int rc2 = cholmod_hip_download_factor (P, Lx_host) ;
        if (rc2 != CHOLMOD_HIP_OK) return rc2 ;
    }
    return rc ;
}

int cholmod_hip_get_maps (cholmod_hip_plan *P, int64_t *sparent, int64_t *level, int64_t *relmap)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    for (i64 s = 0 ; s < P->nsuper ; s++)
    {
        if (sparent) sparent [s] = P->fr [s].parent ;
        if (level) level [s] = P->level [s] ;
    }
    if (relmap)
    {
        if (P->host_only) return CHOLMOD_HIP_NO_DEVICE ;
        std::vector<i32> tmp (std::max<i64> (P->relsize, 1)) ;
        HIPCHK (hipMemcpy (tmp.data (), P->d_relmap, tmp.size () * sizeof (i32), hipMemcpyDeviceToHost)) ;
        // fronts without a parent have no entries; the compact layout has none either
        for (i64 q = 0 ; q < P->relsize ; q++) relmap [q] = tmp [q] ;
    }
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_get_stats (cholmod_hip_plan *P, double *stats)
{
    if (!P || !stats) return CHOLMOD_HIP_INVALID ;
    P->stats [1] = P->exec_flops ;
    P->stats [2] = (double) P->sch.launches.size () + 3 ;
    P->stats [3] = P->nlevels ;
    P->stats [4] = 8.0 * P->arena ;
    P->stats [5] = 8.0 * P->xsize ;
    P->stats [36] = 8.0 * P->lx_local ;
    P->stats [22] = P->nsplit ;
    if (P->sd_time_pending && P->solve_seconds < 0)
    {
        // the last solve was a cholmod_hip_solve_device: its events are read here, not in the call
        float ms = 0 ;
        if (hipEventSynchronize (P->sd_ev1) == hipSuccess && hipEventElapsedTime (&ms, P->sd_ev0, P->sd_ev1) == hipSuccess)
            P->solve_seconds = 1e-3 * ms ;
        else { (void) hipGetLastError () ; P->solve_seconds = 0 ; }
    }
    P->sd_time_pending = false ;
    P->stats [24] = P->solve_seconds ;
    exchange_volume (P, P->stats) ;
    for (int q = 0 ; q < CHOLMOD_HIP_NSTATS ; q++) stats [q] = P->stats [q] ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_debug_thin_cycles (cholmod_hip_plan *P, int64_t launch, long long *out10)
{
    if (!P || !P->d_thin_tim || launch < 0 || launch >= (i64) P->sch.launches.size ()) return CHOLMOD_HIP_INVALID ;
    HIPCHK (hipMemcpy (out10, P->d_thin_tim + 10 * launch, 10 * sizeof (long long), hipMemcpyDeviceToHost)) ;
    return CHOLMOD_HIP_OK ;
}

int64_t cholmod_hip_get_launch_profile (cholmod_hip_plan *P, int64_t cap, int32_t *kind, int32_t *grid,
    int32_t *aux, double *ms, double *flops, double *bytes)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    i64 nl = (i64) P->sch.launches.size () ;
    for (i64 q = 0 ; q < nl && q < cap ; q++)
    {
        const Launch &L = P->sch.launches [q] ;
        if (kind) kind [q] = L.kind ;
        if (grid) grid [q] = L.grid ;
        if (aux) aux [q] = L.aux ;
        if (ms) ms [q] = q < (i64) P->launch_ms.size () ? P->launch_ms [q] : 0.0 ;
        if (flops) flops [q] = L.flops ;
        if (bytes) bytes [q] = L.bytes ;
    }
    return nl ;
}

// test hook: a fingerprint of everything build_host derives for this rank -- fronts, child lists and routing pairs, the
// rank's layout of L and of the arena, every group array and the launch list (FNV-1a over the fields).  Host-only plans
// have it too: tests/test_schedule_fingerprint.py pins the schedules of a battery of problems, worlds and flags, so that a
// restructuring of the scheduler that changes any launch is caught without a GPU.
int cholmod_hip_debug_schedule_hash (cholmod_hip_plan *P, uint64_t *out16)
{
    if (!P || !out16) return CHOLMOD_HIP_INVALID ;
    auto fnv = [] (uint64_t h, const void *p, size_t nbytes) -> uint64_t
    {
        const unsigned char *b = (const unsigned char *) p ;
        for (size_t q = 0 ; q < nbytes ; q++) { h ^= b [q] ; h *= 0x100000001b3ull ; }
        return h ;
    } ;
    const uint64_t H0 = 0xcbf29ce484222325ull ;
    auto hv = [&] (const auto &v) -> uint64_t
    {
        return v.empty () ? H0 : fnv (H0, v.data (), v.size () * sizeof (v [0])) ;
    } ;
    const Schedule &S = P->sch ;
    out16 [0] = hv (S.zg) ; out16 [1] = hv (S.eg) ; out16 [2] = hv (S.pg) ; out16 [3] = hv (S.tg) ;
    out16 [4] = hv (S.gg) ;
    // (gathered head regions and their row maps: folded in only where a plan has them, so plans without heads hash as before)
    if (!S.xg.empty ()) out16 [4] = fnv (fnv (out16 [4], S.xg.data (), S.xg.size () * sizeof (GatherGroup)), S.gmap.data (), S.gmap.size () * sizeof (i32)) ;
    // (likewise the regions that carry their children's contribution-block entries, their list by region and their pairs)
    if (!S.fz.empty ())
    {
        const i64 w [] = {(i64) S.invsize, (i64) S.gfz.size ()} ;
        out16 [4] = fnv (fnv (fnv (fnv (out16 [4], S.fz.data (), S.fz.size () * sizeof (FuseD)), S.gfz.data (), S.gfz.size () * sizeof (i32)),
            S.ivp.data (), S.ivp.size () * sizeof (InvPair)), w, sizeof (w)) ;
    }
    out16 [5] = hv (S.dg) ; out16 [6] = hv (S.rg) ; out16 [7] = hv (S.wg) ;
    out16 [8] = hv (S.cg) ; out16 [9] = hv (S.sm) ;
    uint64_t h = H0 ;
    for (const Launch &L : S.launches)
    {
        const i64 v [] = {L.kind, L.grid, L.ng, (i64) L.goff, L.stream, L.wait_ev, L.rec_ev, L.ar_g0, L.ar_gn, L.aux, L.leaf_T, L.leaf_pw, L.ndiag, L.half,
            L.xd.slab, L.xd.lda, L.xd.w, L.xd.mb, L.xd.R, L.xd.g, L.xd.r, L.xd.fo, L.xd.mf, L.xd.Rf, L.far} ;
        h = fnv (h, v, sizeof (v)) ;
        const double d [] = {L.flops, L.bytes} ;
        h = fnv (h, d, sizeof (d)) ;
    }
    out16 [10] = h ;
    out16 [11] = hv (P->fr) ;
    out16 [12] = fnv (hv (P->child), P->crel.data (), P->crel.size () * sizeof (i64)) ;
    out16 [13] = P->relpairs.empty () ? H0 : fnv (H0, P->relpairs.data (), P->relpairs.size () * sizeof (RelPair)) ;
    const i64 w [] = {S.ncflags, S.max_dinv_slots, S.nevents, P->arena, P->lx_local, P->lx_fronts, P->nsplit, P->relsize_all, P->global_arena} ;
    out16 [14] = fnv (H0, w, sizeof (w)) ;
    out16 [15] = fnv (fnv (hv (P->lpx), P->win_off.data (), P->win_off.size () * sizeof (i64)), P->assign_cb.data (), P->assign_cb.size ()) ;
    return CHOLMOD_HIP_OK ;
}

int64_t cholmod_hip_debug_cb_extend_add (cholmod_hip_plan *P, int64_t cap, int64_t *out)
{
    if (!P || !out) return CHOLMOD_HIP_INVALID ;
    const Schedule &S = P->sch ;
    std::vector<i64> v (4 * (size_t) std::max<i64> (P->nsuper, 1), 0) ;
    for (i64 s = 0 ; s < P->nsuper ; s++)
    {
        const FrontD &f = P->fr [s] ;
        v [4 * s] = (!f.cbp && f.ncb > 0 && f.child_end > f.child_begin) ? 1 : 0 ;
        v [4 * s + 3] = f.child_end - f.child_begin ;
    }
    for (const FuseD &Z : S.fz) v [4 * (size_t) Z.front + 1]++ ;
    for (const EaGroup &E : S.eg) if (E.c_lo <= P->fr [E.front].nscol && E.c_hi == P->fr [E.front].nsrow && P->fr [E.front].ncb > 0) v [4 * (size_t) E.front + 2]++ ;
    for (i64 s = 0 ; s < P->nsuper && s < cap ; s++) for (int t = 0 ; t < 4 ; t++) out [4 * s + t] = v [4 * s + t] ;
    return P->nsuper ;
}

int64_t cholmod_hip_debug_fused_pair (cholmod_hip_plan *P, int64_t pair, int64_t *desc, int32_t *inv, int32_t *rel)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    const Schedule &S = P->sch ;
    const i64 np = (i64) S.ivp.size () ;
    if (pair < 0 || pair >= np || !desc) return np ;
    const InvPair &R = S.ivp [pair] ;
    i64 launch = -1 ;
    for (size_t z = 0 ; z < S.fz.size () && launch < 0 ; z++)
    {
        if (S.fz [z].front != R.parent) continue ;
        const size_t q = (size_t) (std::find (S.gfz.begin (), S.gfz.end (), (i32) z) - S.gfz.begin ()) ;
        for (size_t l = 0 ; l < S.launches.size () ; l++)
            if (S.launches [l].kind == K_UPD_W && q >= S.launches [l].goff && q < S.launches [l].goff + S.launches [l].ng) launch = (i64) l ;
    }
    const i64 d [8] = {R.parent, R.child, R.pnscol, R.pncb, R.nc, P->fr [R.child].cbp, R.mcb, launch} ;
    for (int t = 0 ; t < 8 ; t++) desc [t] = d [t] ;
    if (inv && P->d_invmap) HIPCHK (hipMemcpy (inv, P->d_invmap + R.inv, (size_t) R.pncb * sizeof (i32), hipMemcpyDeviceToHost)) ;
    if (rel && P->d_relmap) HIPCHK (hipMemcpy (rel, P->d_relmap + R.rel, (size_t) R.nc * sizeof (i32), hipMemcpyDeviceToHost)) ;
    return np ;
}

// tuning: the update regions of launch `launch` (an update launch of any kind), 12 numbers per
// region: m, n, k, tri, c_in_cb, lda, ldc, ntiles, nblk, front, assign, swz
int64_t cholmod_hip_debug_launch_regions (cholmod_hip_plan *P, int64_t launch, int64_t cap, int64_t *out)
{
    if (!P || launch < 0 || launch >= (i64) P->sch.launches.size ()) return CHOLMOD_HIP_INVALID ;
    const Launch &L = P->sch.launches [launch] ;
    if (L.kind != K_UPD_W && L.kind != K_UPD_SMALL && L.kind != K_UPD_BIG && L.kind != K_UPD_PF) return 0 ;
    for (i64 q = 0 ; q < L.ng && q < cap ; q++)
    {
        const GemmGroup &G = P->sch.gg [L.goff + q] ;
        const i64 v [12] = {G.m, G.n, G.k, G.tri, G.c_in_cb, G.lda, G.ldc, G.ntiles, G.nblk, G.front, G.assign, G.swz} ;
        for (int t = 0 ; t < 12 ; t++) out [12 * q + t] = v [t] ;
    }
    return L.ng ;
}

int cholmod_hip_set_profiling (cholmod_hip_plan *P, int on)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    P->profiling = on != 0 ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_dense_partial_factor (double *F, int64_t nsrow, int64_t nscol, int flags,
    int64_t *info_out)
{
    if (!F || nsrow <= 0 || nscol <= 0 || nscol > nsrow) return CHOLMOD_HIP_INVALID ;
    if (!cholmod_hip_probe ()) return CHOLMOD_HIP_NO_DEVICE ;
    FrontD f ;
    memset (&f, 0, sizeof (f)) ;
    f.nscol = (i32) nscol ; f.nsrow = (i32) nsrow ; f.ncb = (i32) (nsrow - nscol) ; f.parent = -1 ;
    std::vector<FrontD> fr (1, f) ;
    Schedule S ;
    i32 id = 0 ;
    double fl = 0 ;
    schedule_dense (fr, &id, 1, S, flags, nullptr, nullptr, nullptr, 0, 1) ;
    (void) fl ;
    cholmod_hip_plan P ;
    P.flags = flags ;
    hipError_t e ;
    HIPCHK (hipStreamCreate (&P.stream)) ;
    HIPCHK (hipStreamCreate (&P.stream2)) ;
    for (int q = 0 ; q < S.nevents ; q++)
    {
        hipEvent_t ev ;
        HIPCHK (hipEventCreateWithFlags (&ev, hipEventDisableTiming)) ;
        P.sync_ev.push_back (ev) ;
    }
    i64 ncb = nsrow - nscol ;
    HIPCHK (hipMalloc ((void **) &P.d_Lx, (nsrow * nscol + UPD3_LX_PAD) * sizeof (double))) ;
    HIPCHK (hipMalloc ((void **) &P.d_cb, std::max<i64> (ncb * ncb, 1) * sizeof (double))) ;
    HIPCHK (hipMalloc ((void **) &P.d_info, sizeof (i32))) ;
    HIPCHK (hipMemset (P.d_info, 0, sizeof (i32))) ;
    P.d_pg = dupload (S.pg, e) ; HIPCHK (e) ;
    P.d_tg = dupload (S.tg, e) ; HIPCHK (e) ;
    HIPCHK (hipMalloc ((void **) &P.d_tu_cnt, std::max<size_t> (S.tg.size (), 1) * sizeof (i32))) ;
    HIPCHK (hipMemset (P.d_tu_cnt, 0, std::max<size_t> (S.tg.size (), 1) * sizeof (i32))) ;
    P.d_gg = dupload (S.gg, e) ; HIPCHK (e) ;
    P.d_dg = dupload (S.dg, e) ; HIPCHK (e) ;
    P.d_rg = dupload (S.rg, e) ; HIPCHK (e) ;
    P.d_cg = dupload (S.cg, e) ; HIPCHK (e) ;
    P.sch.ncflags = S.ncflags ;
    HIPCHK (hipMalloc ((void **) &P.d_cflags, (4 * (size_t) S.ncflags + 4) * sizeof (int))) ;
    HIPCHK (hipMemset (P.d_cflags, 0, (4 * (size_t) S.ncflags + 4) * sizeof (int))) ;
    HIPCHK (hipMalloc ((void **) &P.d_dinv, (size_t) std::max (S.max_dinv_slots, 1) * 4096 * sizeof (double))) ;
    HIPCHK (hipMemcpy (P.d_Lx, F, nsrow * nscol * sizeof (double), hipMemcpyHostToDevice)) ;
    if (ncb > 0)
        HIPCHK (hipMemcpy2D (P.d_cb, ncb * sizeof (double), F + nscol + nscol * nsrow,
            nsrow * sizeof (double), ncb * sizeof (double), ncb, hipMemcpyHostToDevice)) ;
    HIPCHK (hipDeviceSynchronize ()) ;       // uploads above used the null stream
    for (const Launch &L : S.launches) run_launch (&P, L, false) ;
    HIPCHK (hipGetLastError ()) ;
    HIPCHK (hipStreamSynchronize (P.stream2)) ;
    HIPCHK (hipStreamSynchronize (P.stream)) ;
    HIPCHK (hipMemcpy (F, P.d_Lx, nsrow * nscol * sizeof (double), hipMemcpyDeviceToHost)) ;
    if (ncb > 0)
        HIPCHK (hipMemcpy2D (F + nscol + nscol * nsrow, nsrow * sizeof (double), P.d_cb,
            ncb * sizeof (double), ncb * sizeof (double), ncb, hipMemcpyDeviceToHost)) ;
    i32 inf = 0 ;
    HIPCHK (hipMemcpy (&inf, P.d_info, sizeof (i32), hipMemcpyDeviceToHost)) ;
    if (info_out) *info_out = inf ;
    free_device (&P) ;
    P.stream = nullptr ; P.stream2 = nullptr ; P.sync_ev.clear () ;
    P.d_Lx = P.d_cb = nullptr ; P.d_info = nullptr ;
    P.d_pg = nullptr ; P.d_tg = nullptr ; P.d_gg = nullptr ; P.d_tu_cnt = nullptr ;
    P.d_dg = nullptr ; P.d_rg = nullptr ; P.d_dinv = nullptr ; P.d_cg = nullptr ; P.d_cflags = nullptr ;
    return CHOLMOD_HIP_OK ;
}

} // extern "C"
