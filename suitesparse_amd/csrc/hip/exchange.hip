// exchange.hip -- what lets several ranks share a front: the collective library bound at run time, the exchange of a
// shared front's block column (the K_XCHG_RS / K_XCHG_AG launches), the agreement on a factorization's outcome, the gather
// of the complete factor and the progress marks a watchdog reads; engine.hip calls it through exchange_internal.hip.h.
// A rank that stays away from a collective hangs its peers: every sum over ranks goes through sum_over_ranks.  Holds
// test hooks: built twice, like engine.hip.
#include "exchange_kernels.hip.h"
#include "exchange_internal.hip.h"

#include <dlfcn.h>
#include <unistd.h>

namespace sship {
RcclApi *rccl_api ()
{
    static RcclApi api ;
    static bool tried = false ;
    if (tried) return api.h ? &api : nullptr ;
    tried = true ;
    // CHOLMOD_HIP_RCCL_LIBRARY names the collective library to bind instead of the system's RCCL
    // (any library exporting the nccl* entry points below; tests/standin_rccl lets several ranks
    // share one GPU, which RCCL itself refuses).  No fallback to RCCL when it is set and missing.
    const char *over = getenv ("CHOLMOD_HIP_RCCL_LIBRARY") ;
    const char *names [] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", nullptr} ;
    void *h = nullptr ;
    if (over && *over)
    {
        h = dlopen (over, RTLD_NOW | RTLD_LOCAL) ;
        if (!h) fprintf (stderr, "cholmod_hip: CHOLMOD_HIP_RCCL_LIBRARY=%s: %s\n", over, dlerror ()) ;
    }
    else for (int q = 0 ; names [q] && !h ; q++) h = dlopen (names [q], RTLD_NOW | RTLD_LOCAL) ;
    if (!h) return nullptr ;
    api.GetUniqueId = (decltype (api.GetUniqueId)) dlsym (h, "ncclGetUniqueId") ;
    api.CommInitRank = (decltype (api.CommInitRank)) dlsym (h, "ncclCommInitRank") ;
    api.CommSplit = (decltype (api.CommSplit)) dlsym (h, "ncclCommSplit") ;
    api.AllReduce = (decltype (api.AllReduce)) dlsym (h, "ncclAllReduce") ;
    api.ReduceScatter = (decltype (api.ReduceScatter)) dlsym (h, "ncclReduceScatter") ;
    api.AllGather = (decltype (api.AllGather)) dlsym (h, "ncclAllGather") ;
    api.Broadcast = (decltype (api.Broadcast)) dlsym (h, "ncclBroadcast") ;
    api.CommDestroy = (decltype (api.CommDestroy)) dlsym (h, "ncclCommDestroy") ;
    api.GetErrorString = (decltype (api.GetErrorString)) dlsym (h, "ncclGetErrorString") ;
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommSplit || !api.AllReduce || !api.ReduceScatter || !api.AllGather || !api.Broadcast || !api.CommDestroy) return nullptr ;
    api.h = h ;
    return &api ;
}

#define RCCLCHK(call) do { ncclResult_t r_ = (call) ; if (r_ != ncclSuccess) { \
    fprintf (stderr, "cholmod_hip: %s failed: %s (%s:%d)\n", #call, \
        (rccl_api () && rccl_api ()->GetErrorString) ? rccl_api ()->GetErrorString (r_) : "?", __FILE__, __LINE__) ; \
    return CHOLMOD_HIP_GPU_PROBLEM ; } } while (0)

// The sum of n doubles at d (device memory, in place) over the ranks [g0, g0 + gn), whose communicator is comm.  RCCL
// attached: an all-reduce in stream order on st (the caller synchronizes st where it needs the result on the host);
// otherwise the host callback, once st has drained.  Every rank enters every collective, or none does: a rank whose
// stream has failed still makes the call its peers wait in and reports the failure afterwards.  (That there is a
// transport at all the callers check up front.)
static int sum_over_ranks (cholmod_hip_plan *P, double *d, i64 n, int g0, int gn, ncclComm_t comm, hipStream_t st)
{
    if (P->nccl_world) RCCLCHK (rccl_api ()->AllReduce (d, d, (size_t) n, ncclDouble, ncclSum, comm, st)) ;
    else
    {
        const hipError_t drained = hipStreamSynchronize (st) ;
        const bool summed = P->ar_fn (d, n, g0, gn, P->ar_user) == 0 ;
        HIPCHK (drained) ;
        if (!summed) return CHOLMOD_HIP_GPU_PROBLEM ;
    }
    return CHOLMOD_HIP_OK ;
}

// ... of the n numbers x on the host (n <= 3 world: through d_xchg), there and back on the main stream.  A failed upload
// does not keep the rank out of the collective either.
static int sum_small (cholmod_hip_plan *P, double *x, i64 n, int g0, int gn, ncclComm_t comm)
{
    const hipError_t uploaded = hipMemcpyAsync (P->d_xchg, x, (size_t) n * sizeof (double), hipMemcpyHostToDevice, P->stream) ;
    const int rc = sum_over_ranks (P, P->d_xchg, n, g0, gn, comm, P->stream) ;
    HIPCHK (uploaded) ;
    if (rc != CHOLMOD_HIP_OK) return rc ;
    HIPCHK (hipMemcpyAsync (x, P->d_xchg, (size_t) n * sizeof (double), hipMemcpyDeviceToHost, P->stream)) ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    return CHOLMOD_HIP_OK ;
}

// CHOLMOD_HIP_NARROW_EXCHANGE_KERNELS=1 (tuning): the kernels of the exchange stream (window open, extend-add into the window,
// pack) as ONE-wave workgroups.  Beside a trailing update whose one-wave tiles refill every register-file slot as it frees
// up, a four-wave workgroup needs room on all four SIMDs of a CU at once and starves until the update ends (rocprofv3:
// k_win_move stretched over the update's 78 ms); one-wave workgroups do get in (0.3 ms) -- but run at a fraction of the
// four-wave kernels' rate and cost a rank of 8 30 ms of compute (1.083 against 1.053 s), more than the early reduce-scatter of
// one block column in eight can return.  Measured, left off.
bool narrow_xs ()
{
    static const bool v = [] () { const char *e = getenv ("CHOLMOD_HIP_NARROW_EXCHANGE_KERNELS") ; return e && atoi (e) != 0 ; } () ;
    return v ;
}

// One K_XCHG_RS / K_XCHG_AG launch of the schedule, on stream st (run_launch has made st wait for the launch's event,
// except for a reduce-scatter ahead of time: that one waits here, on the exchange stream).
int run_exchange (cholmod_hip_plan *P, const Launch &L, hipStream_t st, bool serial)
{
    // Native exchange (cholmod_hip_rccl_attach): everything stream-ordered, the host
    // never waits.  A reduce-scatter ahead of time (wait_ev >= 0) runs on the second
    // stream behind the event of the update that completed the block column, while
    // the main stream goes on with the rest of the trailing update; the main stream
    // then waits (on the device) for the sum before it touches the block column.
    // The all-gather of the far chunks (L.far, L.stream == 1) runs on the second stream
    // behind the event of the block column's chain (waited for above, like any launch's);
    // the main stream meets it at a K_JOIN ahead of the outer update.
    // Host callback (gloo tests, --exchange callback): it only knows a sum
    // all-reduce, so the reduce-scatter is an all-reduce of all segments and the
    // all-gather a sum of buffers that are zero outside the sender's chunk.
    const bool rs = L.kind == K_XCHG_RS ;
    const XchgD &X = L.xd ;
    RcclApi *R = P->nccl_world ? rccl_api () : nullptr ;
    if (!R && !P->ar_fn) return CHOLMOD_HIP_INVALID ;
    bool ahead = rs && !serial && L.wait_ev >= 0 && P->stream2 ;
    hipStream_t cs = ahead ? P->stream2 : st ;
    if (ahead)
    {
        if (R) HIPCHK (hipStreamWaitEvent (cs, P->sync_ev [L.wait_ev], 0)) ;
        else HIPCHK (hipEventSynchronize (P->sync_ev [L.wait_ev])) ;
    }
    ncclComm_t comm = P->nccl_world ;
    if (R && L.ar_gn != P->world)
    {
        auto it = P->nccl_group.find (((i64) L.ar_g0 << 16) | (i64) L.ar_gn) ;
        if (it == P->nccl_group.end ()) return CHOLMOD_HIP_INVALID ;
        comm = it->second ;
    }
    const i64 seg = (i64) X.w * X.w + ((i64) X.R + X.Rf) * X.w, chunk = (i64) (L.far ? X.Rf : X.R) * X.w ;
    double *agb = L.far ? P->d_agf : P->d_ag ;
    const long long xseq = ++P->prog_xchg_enq ;
    if (P->prog_dev) hipLaunchKernelGGL (k_mark, dim3 (1), dim3 (1), 0, cs, P->prog_dev, (P->prog_fact << 32) | xseq) ;
#ifdef CHOLMOD_HIP_TEST_HOOKS
    // test hook CHOLMOD_HIP_TEST_HANG_EXCHANGE=rank:seq[:fact]: that rank never issues exchange `seq` of its
    // factorization number `fact` (default: the second; its host thread sleeps here, nothing hangs on the
    // device) -- its peers then wait for it in the collective, which is what bench.py's watchdog must turn into
    // an error line (tests/test_bench_contract.py)
    if (P->rank == P->test_hang_rank && xseq == P->test_hang_xchg && P->prog_fact >= P->test_hang_fact)
    {
        (void) hipStreamSynchronize (cs) ;
        for ( ; ; ) sleep (3600) ;
    }
#endif
    auto move = [&] (int mode, i64 total)
    {
        if (total <= 0) return ;
        // (one workgroup per column and part: k_xchg_move)
        const unsigned parts = mode == 0 ? 2u * (unsigned) X.g + 1 : (mode == 3 || mode == 5) ? (unsigned) X.g : mode == 1 ? 3u : 1u ;
        const bool narrow = (ahead || (L.stream == 1 && !serial)) && narrow_xs () ;
        hipLaunchKernelGGL (k_xchg_move, dim3 ((unsigned) X.w * parts), dim3 (narrow ? 64 : 256), 0, cs, X, mode, P->d_Lx, P->d_stage, agb) ;
    } ;
    if (rs)
    {
        move (0, seg * X.g) ;
        if (R)
        {
            RCCLCHK (R->ReduceScatter (P->d_stage, P->d_stage + (i64) X.r * seg, (size_t) seg, ncclDouble, ncclSum, comm, cs)) ;
            // The w x w diagonal block travels in every segment, and a ring sums every segment in another
            // order: the members' copies of it would differ in their last bits, each would factor its own,
            // and a borderline pivot could fail on one member only.  One copy for all: the first member's
            // (2 MB at w = 512, next to the block column's 8 (w + rows) w bytes).
            if (X.g > 1) RCCLCHK (R->Broadcast (P->d_stage, P->d_stage + (i64) X.r * seg, (size_t) X.w * X.w, ncclDouble, 0, comm, cs)) ;
        }
        else
        {
            const int rc = sum_over_ranks (P, P->d_stage, seg * X.g, L.ar_g0, L.ar_gn, comm, cs) ;
            if (rc != CHOLMOD_HIP_OK) return rc ;
        }
        move (1, seg) ;
    }
    else
    {
        if (!R) HIPCHK (hipMemsetAsync (agb, 0, (size_t) (chunk * X.g) * sizeof (double), cs)) ;
        move (L.far ? 4 : 2, chunk) ;
        if (R) RCCLCHK (R->AllGather (agb + (i64) X.r * chunk, agb, (size_t) chunk, ncclDouble, comm, cs)) ;
        else
        {
            const int rc = sum_over_ranks (P, agb, chunk * X.g, L.ar_g0, L.ar_gn, comm, cs) ;
            if (rc != CHOLMOD_HIP_OK) return rc ;
        }
        move (L.far ? 5 : 3, chunk * X.g) ;
    }
    if (P->prog_dev) hipLaunchKernelGGL (k_mark, dim3 (1), dim3 (1), 0, cs, P->prog_dev + 1, (P->prog_fact << 32) | xseq) ;
    if (ahead)
    {
        if (R)
        {
            HIPCHK (hipEventRecord (P->ar_done, cs)) ;
            HIPCHK (hipStreamWaitEvent (st, P->ar_done, 0)) ;
        }
        else HIPCHK (hipStreamSynchronize (cs)) ;
    }
    return CHOLMOD_HIP_OK ;
}

// what the plan exchanges per factorization (stats [17], [18], [25], [39]; a property of the launch list)
void exchange_volume (const cholmod_hip_plan *P, double *S)
{
    S [17] = S [18] = S [25] = S [39] = 0 ;
    const size_t nl = P->sch.launches.size () ;
    for (size_t q = 0 ; q < nl ; q++)
    {
        const Launch &L = P->sch.launches [q] ;
        if (L.kind != K_XCHG_RS && L.kind != K_XCHG_AG) continue ;
        S [17] += 1 ; S [18] += L.bytes ;
        if (L.kind != K_XCHG_AG) continue ;
        // an all-gather the main stream waits for at once: in line, or on the exchange stream with the join right behind it
        S [25] += L.bytes ;
        bool inl = L.stream == 0 ;
        for (size_t p = q + 1 ; !inl && p < nl ; p++)
        {
            const Launch &N = P->sch.launches [p] ;
            if (N.kind == K_JOIN) inl = true ;
            else if (!(N.kind == K_XCHG_AG && N.stream == 1)) break ;
        }
        if (inl) S [39] += L.bytes ;
    }
}

// The end of a factorization on several ranks.  poisoned: what a launch of this rank failed with (CHOLMOD_HIP_OK: none);
// *sbad / *binfo: this rank's first failing supernode (-1: none) and its info, replaced by the first one of all ranks.
int agree_first_fail (cholmod_hip_plan *P, int poisoned, i64 *sbad, i64 *binfo)
{
    // agree on the first failing supernode: every rank publishes its own
    // candidate in its slot of a small device array, the sum-all-reduce
    // makes all slots visible everywhere
    if (!P->ar_fn && !P->nccl_world) return CHOLMOD_HIP_INVALID ;
    std::vector<double> x (3 * (size_t) P->world, 0.0) ;
    x [P->rank] = (double) (*sbad >= 0 ? *sbad : P->nsuper) ;
    x [P->world + P->rank] = (double) *binfo ;
    x [2 * P->world + P->rank] = (poisoned != CHOLMOD_HIP_OK) ? 1.0 : 0.0 ;     // a launch of this rank failed
    const int rc = sum_small (P, x.data (), (i64) x.size (), 0, P->world, P->nccl_world) ;
    if (rc != CHOLMOD_HIP_OK) return rc ;
    for (int r = 0 ; r < P->world ; r++)
        if (x [2 * P->world + r] != 0.0) return poisoned != CHOLMOD_HIP_OK ? poisoned : CHOLMOD_HIP_GPU_PROBLEM ;
    i64 best = P->nsuper ;
    for (int r = 0 ; r < P->world ; r++)
        if ((i64) x [r] < best) { best = (i64) x [r] ; *binfo = (i64) x [P->world + r] ; }
    *sbad = best < P->nsuper ? best : -1 ;
    return CHOLMOD_HIP_OK ;
}

// the communicators of the native exchange, destroyed (a plan on its way out, cholmod_hip_rccl_detach)
void exchange_release (cholmod_hip_plan *P)
{
    if (RcclApi *R = (P->nccl_world ? rccl_api () : nullptr))
    {
        for (auto &g : P->nccl_group) (void) R->CommDestroy (g.second) ;
        (void) R->CommDestroy (P->nccl_world) ;
    }
    P->nccl_group.clear () ; P->nccl_world = nullptr ;
}

} // namespace sship

extern "C" {

int cholmod_hip_set_allreduce (cholmod_hip_plan *P, cholmod_hip_allreduce_fn fn, void *user)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    P->ar_fn = fn ; P->ar_user = user ;
    return CHOLMOD_HIP_OK ;
}

/* Progress of the factorization that is running (or ran last), for a watchdog thread of the caller:
 * enable != 0 allocates two words of pinned host memory the device marks, in stream order, around every block-column
 * exchange (two one-thread kernels per exchange: microseconds next to the collective). */
int cholmod_hip_progress_enable (cholmod_hip_plan *P, int enable)
{
    if (!P || P->host_only) return CHOLMOD_HIP_INVALID ;
    if (enable && !P->prog_dev)
    {
        HIPCHK (hipHostMalloc ((void **) &P->prog_dev, 2 * sizeof (long long), hipHostMallocDefault)) ;
        P->prog_dev [0] = P->prog_dev [1] = 0 ;
    }
    else if (!enable && P->prog_dev)
    {
        (void) hipStreamSynchronize (P->stream) ;
        if (P->stream2) (void) hipStreamSynchronize (P->stream2) ;
        (void) hipHostFree (P->prog_dev) ; P->prog_dev = nullptr ;
    }
    return CHOLMOD_HIP_OK ;
}

/* out [0] factorizations started on this plan, [1] launches of the schedule the host has enqueued in the current one,
 * [2] launches in the schedule, [3] exchanges enqueued, [4] exchanges in the schedule, [5] / [6] exchange the DEVICE has
 * entered / left in the current factorization (markers; -1 without cholmod_hip_progress_enable), and of the exchange
 * entered and not left ([5] > [6]): [7] kind (7 = reduce-scatter + broadcast, 11 = all-gather), [8] first rank and [9]
 * size of its group, [10] columns of its block column, [11] rows below that block column's diagonal block.  Safe to call from another thread while a factorization runs. */
int cholmod_hip_progress (cholmod_hip_plan *P, int64_t *out)
{
    if (!P || !out) return CHOLMOD_HIP_INVALID ;
    for (int q = 0 ; q < 12 ; q++) out [q] = 0 ;
    const long long fact = P->prog_fact ;
    out [0] = fact ; out [1] = P->prog_launch ; out [2] = (int64_t) P->sch.launches.size () ; out [3] = P->prog_xchg_enq ;
    i64 nx = 0 ;
    for (const Launch &L : P->sch.launches) if (L.kind == K_XCHG_RS || L.kind == K_XCHG_AG) nx++ ;
    out [4] = nx ; out [5] = out [6] = -1 ;
    if (P->prog_dev)
    {
        const long long a = ((volatile long long *) P->prog_dev) [0], b = ((volatile long long *) P->prog_dev) [1] ;
        out [5] = (a >> 32) == fact ? (a & 0xFFFFFFFFll) : 0 ;
        out [6] = (b >> 32) == fact ? (b & 0xFFFFFFFFll) : 0 ;
        if (out [5] > out [6])
        {
            i64 seq = 0 ;
            for (const Launch &L : P->sch.launches)
                if ((L.kind == K_XCHG_RS || L.kind == K_XCHG_AG) && ++seq == out [5])
                {
                    out [7] = L.kind ; out [8] = L.ar_g0 ; out [9] = L.ar_gn ; out [10] = L.xd.w ; out [11] = L.xd.mb + L.xd.mf ;
                    break ;
                }
        }
    }
    return CHOLMOD_HIP_OK ;
}

/* After a distributed factorization every rank holds, in its own packed array, the shared
 * fronts of its groups and its own subtrees.  The gather builds the complete factor in the
 * reference layout (L->px) on EVERY rank: each front is written into a zeroed full-size array by
 * exactly one rank (the first of its group), and a sum over all ranks completes it everywhere.
 * The full array needs 8 xsize bytes next to the rank's own part; if that does not fit, the
 * contribution-block arena (dead between factorizations) makes room and is allocated again by
 * the next factorization. */
int cholmod_hip_gather_factor (cholmod_hip_plan *P)
{
    if (!P || P->host_only) return CHOLMOD_HIP_INVALID ;
    if (P->world == 1) return CHOLMOD_HIP_OK ;
    if (!P->ar_fn && !P->nccl_world) return CHOLMOD_HIP_INVALID ;
    P->winv_valid = false ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    // test hooks: CHOLMOD_HIP_TEST_FAIL_GATHER=r: rank r finds no room for the complete factor at all;
    // CHOLMOD_HIP_TEST_GATHER_STAGED=r: rank r finds none next to its own part (the host-staged way below)
    const char *tfg = TEST_ENV ("CHOLMOD_HIP_TEST_FAIL_GATHER"), *tgs = TEST_ENV ("CHOLMOD_HIP_TEST_GATHER_STAGED") ;
    const bool fail_here = tfg && atoi (tfg) == P->rank, staged_here = tgs && atoi (tgs) == P->rank ;
    // (nothing newer than the gathered copy: the same on every rank -- full_valid is set by a complete gather
    // and cleared by a factorization, collectively both)
    if (P->full_valid && P->d_Lx_full && !fail_here && !staged_here) return CHOLMOD_HIP_OK ;
    if ((fail_here || staged_here) && P->d_Lx_full) { (void) hipFree (P->d_Lx_full) ; P->d_Lx_full = nullptr ; }
    std::unique_ptr<double []> own_host ;   // the rank's own part of L on the host (staged way only)
    bool staged = false ;
    auto restore_own = [&] () -> bool       // the rank's own array back from the host copy
    {
        if (hipMalloc ((void **) &P->d_Lx, (std::max<i64> (P->lx_local, 1) + UPD3_LX_PAD) * sizeof (double)) == hipSuccess
            && hipMemcpy (P->d_Lx, own_host.get (), (size_t) P->lx_local * sizeof (double), hipMemcpyHostToDevice) == hipSuccess) return true ;
        (void) hipGetLastError () ;
        fprintf (stderr, "cholmod_hip_gather_factor: rank %d lost its part of the factor\n", P->rank) ;
        if (P->d_Lx) { (void) hipFree (P->d_Lx) ; P->d_Lx = nullptr ; }
        return false ;
    } ;
    auto try_full = [&] () -> bool
    {
        if (hipMalloc ((void **) &P->d_Lx_full, std::max<i64> (P->xsize, 1) * sizeof (double)) == hipSuccess) return true ;
        (void) hipGetLastError () ;
        P->d_Lx_full = nullptr ;
        return false ;
    } ;
    if (!P->d_Lx_full && !fail_here && P->d_Lx)
    {
        bool got = !staged_here && try_full () ;
        if (!got && !staged_here)
        {
            // the contribution-block arena is dead between factorizations: it makes room
            if (P->d_cb) { (void) hipFree (P->d_cb) ; P->d_cb = nullptr ; }
            got = try_full () ;
        }
        if (!got)
        {
            // Still no room next to the rank's own part (two ranks at Poisson 200^3: 117 GB + 181.6 GB): the own
            // part takes a detour through host memory -- download, release it (and the arena), reserve the complete
            // array, upload the fronts this rank contributes straight into their places.  The next factorization
            // reserves the rank's own array again (run_factorize).
            // (only with plenty of host memory to spare -- the other ranks of the node may be doing the same, and an
            // over-committed allocation fails when it is touched, not here: 40 % of what /proc/meminfo calls available)
            double avail = 0 ;
            if (FILE *mf = fopen ("/proc/meminfo", "r"))
            {
                char line [256] ;
                while (fgets (line, sizeof (line), mf))
                    if (strncmp (line, "MemAvailable:", 13) == 0) { avail = 1024.0 * atof (line + 13) ; break ; }
                fclose (mf) ;
            }
            if (8.0 * (double) P->lx_local <= 0.4 * avail)
                own_host.reset (new (std::nothrow) double [(size_t) std::max<i64> (P->lx_local, 1)]) ;
            if (own_host && hipMemcpy (own_host.get (), P->d_Lx, (size_t) P->lx_local * sizeof (double), hipMemcpyDeviceToHost) == hipSuccess)
            {
                if (P->d_cb) { (void) hipFree (P->d_cb) ; P->d_cb = nullptr ; }
                (void) hipFree (P->d_Lx) ; P->d_Lx = nullptr ;
                if (try_full ()) staged = true ;
                else (void) restore_own () ;        // (not even alone: the rank's part goes back where it was)
            }
            else (void) hipGetLastError () ;
            if (!P->d_Lx_full)
                fprintf (stderr, "cholmod_hip_gather_factor: no room for the complete factor (%.1f GB) on rank %d\n", 8e-9 * P->xsize, P->rank) ;
        }
    }
    // everything local that can still fail comes BEFORE the agreement, and its outcome is part of the vote
    bool setup_ok = true ;
    if (!P->d_fr_full)
    {
        // (descriptors of the complete factor: the global offsets, every column in place)
        std::vector<FrontD> ff (P->fr) ;
        for (i64 q = 0 ; q < P->nsuper ; q++) { ff [q].psx = P->px [q] ; ff [q].own_w = 0 ; ff [q].own_g = 1 ; ff [q].own_r = 0 ; }
        hipError_t e ;
        P->d_fr_full = dupload (ff, e) ;
        if (e != hipSuccess) { (void) hipGetLastError () ; if (P->d_fr_full) (void) hipFree (P->d_fr_full) ; P->d_fr_full = nullptr ; setup_ok = false ; }
    }
    // one number summed over all ranks, in d_xchg; < 0: the exchange itself failed
    auto agree = [&] (double mine) -> double
    {
        double any = mine ;
        if (sum_small (P, &any, 1, 0, P->world, P->nccl_world) != CHOLMOD_HIP_OK) { (void) hipGetLastError () ; return -1.0 ; }
        return any + (mine != 0.0 && any == 0.0 ? 1.0 : 0.0) ;
    } ;
    {
        // every rank must enter the sums below or none: a rank without room tells the others first
        // (a rank that returned on its own would leave them waiting in the collective)
        double any = agree ((P->d_Lx_full && setup_ok) ? 0.0 : 1.0) ;
        if (any != 0.0)
        {
            if (P->d_Lx_full) { (void) hipFree (P->d_Lx_full) ; P->d_Lx_full = nullptr ; }
            P->full_valid = false ;
            if (staged && !restore_own ()) return CHOLMOD_HIP_GPU_PROBLEM ;     // (another rank had no room: this one keeps its part)
            return any < 0.0 ? CHOLMOD_HIP_GPU_PROBLEM : (setup_ok ? CHOLMOD_HIP_OUT_OF_MEMORY : CHOLMOD_HIP_GPU_PROBLEM) ;
        }
    }
    // From here on every rank enters every collective, whatever happens to it locally: a failure is kept in
    // `bad`, the remaining sums are still entered (their data no longer matters), and a trailing agreement
    // tells everybody.
    int bad = CHOLMOD_HIP_OK ;
    auto hold = [&] (hipError_t e) { if (e != hipSuccess) { (void) hipGetLastError () ; if (bad == CHOLMOD_HIP_OK) { bad = CHOLMOD_HIP_GPU_PROBLEM ;
        fprintf (stderr, "cholmod_hip_gather_factor: %s on rank %d\n", hipGetErrorString (e), P->rank) ; } } } ;
    hold (hipMemsetAsync (P->d_Lx_full, 0, std::max<i64> (P->xsize, 1) * sizeof (double), P->stream)) ;
    auto put = [&] (i64 dst, i64 src, i64 len)      // a piece of the rank's part into its place in the complete factor
    {
        if (len <= 0) return ;
        if (staged) hold (hipMemcpyAsync (P->d_Lx_full + dst, own_host.get () + src, (size_t) len * sizeof (double), hipMemcpyHostToDevice, P->stream)) ;
        else hold (hipMemcpyAsync (P->d_Lx_full + dst, P->d_Lx + src, (size_t) len * sizeof (double), hipMemcpyDeviceToDevice, P->stream)) ;
    } ;
    for (i64 q = 0 ; q < P->nsuper ; )
    {
        if (P->lpx [q] < 0) { q++ ; continue ; }
        const FrontD &f = P->fr [q] ;
        if (f.own_w)
        {
            // a distributed front: the slabs this rank owns (whole columns, contiguous in both arrays)
            for (int c0 = 0 ; c0 < f.nscol ; c0 += f.own_w)
                if (col_owned (f, c0))
                    put (P->px [q] + (i64) c0 * f.nsrow, P->lpx [q] + (i64) col_local (f, c0) * f.nsrow, (i64) std::min (f.own_w, f.nscol - c0) * f.nsrow) ;
            q++ ;
            continue ;
        }
        // runs of consecutive fronts this rank contributes: contiguous in both arrays
        if (P->rank != P->grp0 [q]) { q++ ; continue ; }
        i64 e = q ;
        while (e < P->nsuper && P->lpx [e] >= 0 && !P->fr [e].own_w && P->rank == P->grp0 [e] && P->lpx [e] - P->lpx [q] == P->px [e] - P->px [q]) e++ ;
        put (P->px [q], P->lpx [q], P->px [e] - P->px [q]) ;
        q = e ;
    }
    hold (hipStreamSynchronize (P->stream)) ;
    const i64 chunk = (i64) 1 << 27 ;
    for (i64 off = 0 ; off < P->xsize ; off += chunk)
    {
        i64 cnt = std::min (chunk, P->xsize - off) ;
        const int rc = sum_over_ranks (P, P->d_Lx_full + off, cnt, 0, P->world, P->nccl_world, P->stream) ;
        if (rc != CHOLMOD_HIP_OK) { (void) hipGetLastError () ; if (bad == CHOLMOD_HIP_OK) bad = rc ; }
    }
    hold (hipStreamSynchronize (P->stream)) ;
    {
        double any = agree (bad == CHOLMOD_HIP_OK ? 0.0 : 1.0) ;
        if (any != 0.0)
        {
            // somebody's copy is not the factor: nobody keeps one; a rank that staged its part through the host gets it back
            (void) hipFree (P->d_Lx_full) ; P->d_Lx_full = nullptr ;
            P->full_valid = false ;
            if (staged) (void) restore_own () ;
            return bad != CHOLMOD_HIP_OK ? bad : CHOLMOD_HIP_GPU_PROBLEM ;
        }
    }
    P->full_valid = true ;
    return CHOLMOD_HIP_OK ;
}

/* ---- native exchange over RCCL ------------------------------------------------- */

int cholmod_hip_rccl_unique_id (void *id128)
{
    RcclApi *R = rccl_api () ;
    if (!R || !id128) return CHOLMOD_HIP_NO_DEVICE ;
    static_assert (sizeof (ncclUniqueId) == 128, "ncclUniqueId is 128 bytes") ;
    ncclUniqueId id ;
    RCCLCHK (R->GetUniqueId (&id)) ;
    memcpy (id128, &id, sizeof (id)) ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_rccl_attach (cholmod_hip_plan *P, const void *id128)
{
    if (!P || P->host_only || !id128) return CHOLMOD_HIP_INVALID ;
    RcclApi *R = rccl_api () ;
    if (!R) return CHOLMOD_HIP_NO_DEVICE ;
    if (P->nccl_world) return CHOLMOD_HIP_OK ;
    ncclUniqueId id ;
    memcpy (&id, id128, sizeof (id)) ;
    RCCLCHK (R->CommInitRank (&P->nccl_world, P->world, id, P->rank)) ;
    // one communicator per rank group the plan shares fronts over; every rank of
    // the world walks the same sorted list (the split is collective over the world)
    std::map<i64, int> groups ;
    for (i64 s = 0 ; s < P->nsuper ; s++)
        if (P->grpn [s] > 1 && P->grpn [s] < P->world) groups [((i64) P->grp0 [s] << 16) | (i64) P->grpn [s]] = 1 ;
    int color = 0 ;
    for (auto &g : groups)
    {
        int g0 = (int) (g.first >> 16), gn = (int) (g.first & 0xffff) ;
        bool member = P->rank >= g0 && P->rank < g0 + gn ;
        ncclComm_t sub = nullptr ;
        RCCLCHK (R->CommSplit (P->nccl_world, member ? color : NCCL_SPLIT_NOCOLOR, P->rank, &sub, nullptr)) ;
        if (member) P->nccl_group [g.first] = sub ;
        color++ ;
    }
    if (!P->ar_done) HIPCHK (hipEventCreateWithFlags (&P->ar_done, hipEventDisableTiming)) ;
    // self check: a sum of ones over every communicator this rank belongs to must give
    // the size of its group (catches a wrong split before any factor data moves)
    {
        std::vector<std::pair<ncclComm_t, int>> mine ;
        mine.push_back ({P->nccl_world, P->world}) ;
        for (auto &g : P->nccl_group) mine.push_back ({g.second, (int) (g.first & 0xffff)}) ;
        for (auto &c : mine)
        {
            double got = 1.0 ;
            const int rc = sum_small (P, &got, 1, 0, c.second, c.first) ;       // (attached: the communicator is the group)
            if (rc != CHOLMOD_HIP_OK) return rc ;
            if (got != (double) c.second)
            {
                fprintf (stderr, "cholmod_hip_rccl_attach: self check failed (sum %g over a group of %d)\n", got, c.second) ;
                return CHOLMOD_HIP_GPU_PROBLEM ;
            }
        }
    }
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_rccl_detach (cholmod_hip_plan *P)
{
    if (!P) return CHOLMOD_HIP_INVALID ;
    exchange_release (P) ;
    return CHOLMOD_HIP_OK ;
}

} // extern "C"
