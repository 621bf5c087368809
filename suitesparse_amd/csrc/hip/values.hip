// values.hip -- the matrix-values pipeline of the engine: the upload of a matrix into the resident S
// (cholmod_hip_upload_matrix), the value map and the product map that say where new values of the same pattern go
// (cholmod_hip_set_value_map, cholmod_hip_set_product_map), the chunked upload of such values from the host
// (cholmod_hip_values_begin / _values_push_chunk), the factorization from values that are in device memory already
// (cholmod_hip_factorize_values_device) and the way back (cholmod_hip_download_matrix_values).  Kernels:
// values_kernels.hip.h.  The factorization itself is engine.hip's (engine_internal.hip.h: factorize_prologue, run_factorize),
// and so is what its launch loop does with the pushed chunks (wait_pushed, apply_value_chunks, k_values_chunk).  No test hook
// reaches this file: it is built once for both libraries.
#include "values_kernels.hip.h"
#include "engine_internal.hip.h"
#include <thread>

namespace sship {

/* the product map of the value map goes with it (cholmod_hip_set_product_map) */
void drop_product_map (cholmod_hip_plan *P)
{
    for (void *d : {(void *) P->d_pm_cp, (void *) P->d_pm_ia, (void *) P->d_pm_ib, (void *) P->d_pm_order}) if (d) (void) hipFree (d) ;
    P->d_pm_cp = P->d_pm_ia = P->d_pm_ib = nullptr ; P->d_pm_order = nullptr ;
    P->pm_set = false ; P->pm_na = 0 ;
    /* ... and its transpose, where a gradient call has built it (grad.hip) */
    for (void *d : {(void *) P->d_pt_ptr, (void *) P->d_pt_c, (void *) P->d_pt_partner, (void *) P->d_pt_order, (void *) P->d_pt_gvals})
        if (d) (void) hipFree (d) ;
    P->d_pt_ptr = nullptr ; P->d_pt_c = P->d_pt_partner = P->d_pt_order = nullptr ; P->d_pt_gvals = nullptr ;
    P->pt_built = false ;
}

} // namespace sship

extern "C" {

int cholmod_hip_upload_matrix (cholmod_hip_plan *P, const int64_t *Sp, const int64_t *Si,
    const int64_t *Snz, const double *Sx)
{
    if (!P || P->host_only || !Sp || !Si || !Sx) return CHOLMOD_HIP_INVALID ;
    i64 n = P->n ;
    i64 nz = 0 ;
    if (Snz) { for (i64 j = 0 ; j < n ; j++) nz = std::max<i64> (nz, Sp [j] + Snz [j]) ; }
    else nz = Sp [n] ;
    if (nz > P->s_nz || !P->d_Sp)
    {
        if (P->d_Sp) { (void) hipFree (P->d_Sp) ; (void) hipFree (P->d_Si) ; (void) hipFree (P->d_Sx) ; (void) hipFree (P->d_Snz) ; (void) hipFree (P->d_amap) ; }
        P->d_Sp = P->d_Si = P->d_Snz = P->d_amap = nullptr ; P->d_Sx = nullptr ;
        HIPCHK (hipMalloc ((void **) &P->d_Sp, (n + 1) * sizeof (i64))) ;
        HIPCHK (hipMalloc ((void **) &P->d_Snz, std::max<i64> (n, 1) * sizeof (i64))) ;
        HIPCHK (hipMalloc ((void **) &P->d_Si, std::max<i64> (nz, 1) * sizeof (i64))) ;
        HIPCHK (hipMalloc ((void **) &P->d_Sx, std::max<i64> (nz, 1) * sizeof (double))) ;
        HIPCHK (hipMalloc ((void **) &P->d_amap, std::max<i64> (nz, 1) * sizeof (i64))) ;
        P->s_nz = nz ;
    }
    HIPCHK (hipMemcpyAsync (P->d_Sp, Sp, (n + 1) * sizeof (i64), hipMemcpyHostToDevice, P->stream)) ;
    if (Snz) HIPCHK (hipMemcpyAsync (P->d_Snz, Snz, n * sizeof (i64), hipMemcpyHostToDevice, P->stream)) ;
    if (nz) HIPCHK (hipMemcpyAsync (P->d_Si, Si, nz * sizeof (i64), hipMemcpyHostToDevice, P->stream)) ;
    if (nz) HIPCHK (hipMemcpyAsync (P->d_Sx, Sx, nz * sizeof (double), hipMemcpyHostToDevice, P->stream)) ;
    if (!P->sch.sm.empty ())
    {
        // the range of S every thin front's columns occupy, in the block order of its launch
        std::vector<i64> sp01 (2 * P->sch.sm.size ()) ;
        for (size_t q = 0 ; q < P->sch.sm.size () ; q++)
        {
            const FrontD &f = P->fr [P->sch.sm [q]] ;
            sp01 [2 * q] = Sp [f.k1] ; sp01 [2 * q + 1] = Sp [f.k1 + f.nscol] ;
        }
        HIPCHK (hipMemcpyAsync (P->d_sp01, sp01.data (), sp01.size () * sizeof (i64), hipMemcpyHostToDevice, P->stream)) ;
        HIPCHK (hipStreamSynchronize (P->stream)) ;     // (sp01 is a local)
    }
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    P->s_unpacked = (Snz != nullptr) ;
    P->amap_valid = false ;         // a new pattern may have come with the new values
    P->rs_index_valid = false ;     // ... and the transposed index of the residual goes with the old one
    P->gr_index_valid = false ;     // ... and the column-of-entry array of the gradient
    P->si_valid = P->fg_valid = false ;         // ... and the selected inverse and the factor gradient are those of the old matrix
    P->s_cur_nz = nz ;
    P->vsrc_nz = 0 ;                // ... and the value map of the previous one is void
    drop_product_map (P) ;          // ... with its product map
    P->h_vgather.clear () ; P->nchunks = 0 ;
    if (!Snz && P->world == 1) P->h_Sp.assign (Sp, Sp + n + 1) ; else P->h_Sp.clear () ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_set_value_map (cholmod_hip_plan *P, const int64_t *src, int64_t snz, int64_t nvalues)
{
    if (!P || P->host_only || !src || !P->d_Sp || P->s_unpacked || snz != P->s_cur_nz || nvalues < 0) return CHOLMOD_HIP_INVALID ;
    for (i64 q = 0 ; q < snz ; q++) if (src [q] < 0 || src [q] >= nvalues) return CHOLMOD_HIP_INVALID ;
    drop_product_map (P) ;          // (a product map describes the values of ONE value map)
    if (P->d_vsrc) { (void) hipFree (P->d_vsrc) ; P->d_vsrc = nullptr ; }
    if (P->d_vals) { (void) hipFree (P->d_vals) ; P->d_vals = nullptr ; }
    HIPCHK (hipMalloc ((void **) &P->d_vsrc, std::max<i64> (snz, 1) * sizeof (i64))) ;
    HIPCHK (hipMalloc ((void **) &P->d_vals, std::max<i64> (nvalues, 1) * sizeof (double))) ;
    if (snz) HIPCHK (hipMemcpy (P->d_vsrc, src, snz * sizeof (i64), hipMemcpyHostToDevice)) ;
    P->vsrc_nz = snz ; P->vals_n = nvalues ;
    // the same map in the order the factorization asks for the values: entries of S sorted by the LAUNCH that needs them
    // first -- a thin front's entries by its own launch (the thin-front kernels read their columns of S themselves), a
    // generic front's by the first launch of its batch behind the thin ones (k_values_chunk has then put them into L) --
    // and by source position inside such a class.  One rank, packed S.
    P->h_vgather.clear () ; P->launch_need_chunks.clear () ;
    if (P->d_vorder) { (void) hipFree (P->d_vorder) ; P->d_vorder = nullptr ; }
    static const bool chunked_off = getenv ("CHOLMOD_HIP_VALUES_IN_BATCH_ORDER") && !strcmp (getenv ("CHOLMOD_HIP_VALUES_IN_BATCH_ORDER"), "0") ;
    if (!chunked_off && P->world == 1 && !(P->flags & CHOLMOD_HIP_CX_STORAGE) && (i64) P->h_Sp.size () == P->n + 1 && snz > 0 && snz <= nvalues
        && !P->batch_launch0.empty () && !P->force_shared)
    {
        const size_t nb = P->batch_launch0.size (), nl = P->sch.launches.size () ;
        // need [sf]: the launch before which front sf's entries must have been applied
        std::vector<i32> need ((size_t) std::max<i64> (P->nsuper, 1), -1) ;
        std::vector<i32> generic_launch (nb, 0) ;
        bool okn = true ;
        for (size_t b = 0 ; b < nb ; b++)
        {
            const size_t q0 = P->batch_launch0 [b], q1 = (b + 1 < nb) ? P->batch_launch0 [b + 1] : nl ;
            size_t q = q0 ;
            for ( ; q < q1 && P->sch.launches [q].kind == K_SMALL ; q++)
            {
                const Launch &Lq = P->sch.launches [q] ;
                for (size_t e = Lq.goff ; e < Lq.goff + (size_t) Lq.ng ; e++) need [P->sch.sm [e]] = (i32) q ;
            }
            generic_launch [b] = (i32) std::min (q, q1 > 0 ? q1 - 1 : 0) ;
        }
        for (i64 sf = 0 ; sf < P->nsuper && okn ; sf++)
        {
            const i32 b = P->batch_of [sf] ;
            if (b < 0 || (size_t) b >= nb) { okn = false ; break ; }
            if (need [sf] < 0) need [sf] = generic_launch [b] ;
        }
        if (okn && nl > 0)
        {
            // buckets by need, filled in source order on a few threads: the caller's staging copy (stage [k] = values
            // [index [k]]) then walks its value array front to back once per class -- sequential reads with gaps -- and the
            // scatter to S's order is left to the device, where it costs nothing.  (S's own order made that copy a random
            // gather: 1.7 ms for the 4.75 M entries of the 2D stand-in against 0.4 ms for a plain copy.)
            std::vector<i64> order ((size_t) snz) ;
            P->h_vgather.resize ((size_t) snz) ;
            std::vector<i64> cnt (nl + 1, 0) ;
            {
                std::vector<i32> needq ((size_t) snz) ;
                std::vector<i64> inv ((size_t) nvalues, -1) ;
                const int T = (int) std::max<i64> (1, std::min<i64> (8, snz / 200000)) ;
                auto par = [&] (auto fn) {
                    std::vector<std::thread> th ;
                    for (int t = 1 ; t < T ; t++) th.emplace_back (fn, t) ;
                    fn (0) ;
                    for (auto &x : th) x.join () ;
                } ;
                par ([&] (int t) {
                    const i64 s0 = P->nsuper * t / T, s1 = P->nsuper * (t + 1) / T ;
                    for (i64 sf = s0 ; sf < s1 ; sf++)
                        for (i64 q = P->h_Sp [P->super [sf]] ; q < P->h_Sp [P->super [sf + 1]] ; q++) { needq [q] = need [sf] ; inv [src [q]] = q ; }
                }) ;
                std::vector<std::vector<i64>> tcnt (T, std::vector<i64> (nl, 0)) ;
                par ([&] (int t) {
                    const i64 a0 = nvalues * t / T, a1 = nvalues * (t + 1) / T ;
                    for (i64 a = a0 ; a < a1 ; a++) if (inv [a] >= 0) tcnt [t][needq [inv [a]]]++ ;
                }) ;
                for (size_t q = 0 ; q < nl ; q++)
                {
                    i64 off = cnt [q] ;
                    for (int t = 0 ; t < T ; t++) { const i64 c = tcnt [t][q] ; tcnt [t][q] = off ; off += c ; }
                    cnt [q + 1] = off ;
                }
                par ([&] (int t) {
                    const i64 a0 = nvalues * t / T, a1 = nvalues * (t + 1) / T ;
                    for (i64 a = a0 ; a < a1 ; a++)
                    {
                        const i64 q = inv [a] ;
                        if (q < 0) continue ;
                        const i64 k = tcnt [t][needq [q]]++ ;
                        order [k] = q ; P->h_vgather [k] = a ;
                    }
                }) ;
            }
            HIPCHK (hipMalloc ((void **) &P->d_vorder, (size_t) snz * sizeof (i64))) ;
            HIPCHK (hipMemcpy (P->d_vorder, order.data (), (size_t) snz * sizeof (i64), hipMemcpyHostToDevice)) ;
            // chunks a launch needs = those that hold the entries of every class up to its own
            P->launch_need_chunks.assign (nl + 1, (i32) ((snz + P->chunk_len - 1) / P->chunk_len)) ;
            for (size_t q = 0 ; q < nl ; q++) P->launch_need_chunks [q] = (i32) ((cnt [q + 1] + P->chunk_len - 1) / P->chunk_len) ;
        }
    }
    return CHOLMOD_HIP_OK ;
}

/* The value upload of a call with the pattern of the resident S (cholmod_l_factorize), driven by the caller's threads:
 *   * cholmod_hip_values_begin: the plan's pinned staging buffer, and where staged position k comes from in the caller's
 *     value array -- in batch order (the entries of S sorted by the launch that first needs them, set_value_map above) --
 *     or NULL: in S order, the caller's array as it is.  The clearing of L is enqueued at once (it runs beside the
 *     upload), the chunk counters are reset;
 *   * cholmod_hip_factorize_resident follows.  In batch order its launch loop waits -- host side for the push, device side
 *     for the copy -- only for the chunks the next batch needs, applies them (k_values_chunk) and goes on; in S order
 *     every launch needs every value: it waits for the last push, whose gather into S the assembly waits for on the device;
 *   * cholmod_hip_values_push_chunk (plan, c) for c = 0, 1, ... as chunks are staged (one thread, in order; a DMA on the
 *     exchange stream, no host wait); (plan, -1) cancels: the waiting factorization returns an error.
 * Nothing of this touches the resident S before the factorization's turn. */
int cholmod_hip_values_begin (cholmod_hip_plan *P, double **buffer, const int64_t **index, int64_t *count, int64_t *chunk_len)
{
    if (!P || P->host_only || !buffer || !index || !count || !chunk_len || !P->d_vsrc || P->vsrc_nz != P->s_cur_nz)
        return CHOLMOD_HIP_INVALID ;
    const bool batch = !P->h_vgather.empty () && (i64) P->h_vgather.size () == P->s_cur_nz && P->amap_valid && P->d_vorder
        && P->launch_need_chunks.size () == P->sch.launches.size () + 1 ;
    if (!P->h_vals || P->h_vals_n != P->vals_n)
    {
        if (P->h_vals) { (void) hipHostFree (P->h_vals) ; P->h_vals = nullptr ; }
        if (hipHostMalloc ((void **) &P->h_vals, (size_t) std::max<i64> (P->vals_n, 1) * sizeof (double), hipHostMallocDefault) != hipSuccess)
        {
            (void) hipGetLastError () ;
            P->h_vals = nullptr ;
            return CHOLMOD_HIP_OUT_OF_MEMORY ;
        }
        P->h_vals_n = P->vals_n ;
    }
    const i64 staged = batch ? P->s_cur_nz : P->vals_n ;
    P->nchunks = (long) ((staged + P->chunk_len - 1) / P->chunk_len) ;
    while ((long) P->chunk_ev.size () < P->nchunks)
    {
        hipEvent_t e ; HIPCHK (hipEventCreateWithFlags (&e, hipEventDisableTiming)) ; P->chunk_ev.push_back (e) ;
    }
    const int rc = factorize_prologue (P) ;
    if (rc != CHOLMOD_HIP_OK) return rc ;
    P->chunks_pushed.store (0) ;
    P->chunks_applied = 0 ;
    P->values_begun = true ;
    P->values_in_batch_order = batch ;
    *buffer = P->h_vals ; *index = batch ? P->h_vgather.data () : nullptr ;
    *count = staged ; *chunk_len = P->chunk_len ;
    return CHOLMOD_HIP_OK ;
}

int cholmod_hip_values_push_chunk (cholmod_hip_plan *P, int64_t c)
{
    if (!P || !P->h_vals) return CHOLMOD_HIP_INVALID ;
    if (c < 0 || c >= P->nchunks) { P->chunks_pushed.store (-1) ; return CHOLMOD_HIP_INVALID ; }
    const bool s_order = !P->values_in_batch_order ;
    const i64 k0 = c * P->chunk_len, k1 = std::min<i64> (k0 + P->chunk_len, s_order ? P->vals_n : P->s_cur_nz) ;
    bool ok = hipMemcpyAsync (P->d_vals + k0, P->h_vals + k0, (size_t) (k1 - k0) * sizeof (double), hipMemcpyHostToDevice, P->stream2) == hipSuccess ;
    if (ok && s_order && c == P->nchunks - 1 && P->vsrc_nz > 0)
    {
        hipLaunchKernelGGL (k_gather_values, dim3 ((unsigned) ((P->vsrc_nz + 255) / 256)), dim3 (256), 0, P->stream2,
            P->vsrc_nz, P->d_vsrc, P->d_vals, P->d_Sx) ;
        ok = hipGetLastError () == hipSuccess ;
    }
    if (!ok || hipEventRecord (P->chunk_ev [c], P->stream2) != hipSuccess)
    {
        (void) hipGetLastError () ;
        P->chunks_pushed.store (-1) ;
        return CHOLMOD_HIP_GPU_PROBLEM ;
    }
    P->chunks_pushed.store ((long) c + 1, std::memory_order_release) ;
    return CHOLMOD_HIP_OK ;
}

/* The values of the value map as sums of products of the caller's values (cholmod_hip.h): validated here, entry by
 * entry, so that k_product_values needs no bounds check of its own; then the lists go up once, with the entries sorted
 * by list length into the kernel's three classes (a counting sort: inside a class the entries keep their order). */
int cholmod_hip_set_product_map (cholmod_hip_plan *P, const int64_t *cp, const int64_t *ia, const int64_t *ib,
    int64_t nc, int64_t navalues)
{
    if (!P || P->host_only) return CHOLMOD_HIP_INVALID ;
    if (!cp) { drop_product_map (P) ; return CHOLMOD_HIP_OK ; }
    if (!ia || !ib || !P->d_vsrc || P->vsrc_nz != P->s_cur_nz || nc != P->vals_n || nc < 0 || navalues < 0 || cp [0] != 0)
        return CHOLMOD_HIP_INVALID ;
    for (i64 c = 0 ; c < nc ; c++) if (cp [c + 1] < cp [c]) return CHOLMOD_HIP_INVALID ;
    const i64 np = cp [nc] ;
    if (np > INT32_MAX || nc > INT32_MAX) return CHOLMOD_HIP_TOO_LARGE ;
    for (i64 p = 0 ; p < np ; p++) if (ia [p] < 0 || ia [p] >= navalues || ib [p] < 0 || ib [p] >= navalues) return CHOLMOD_HIP_INVALID ;
    drop_product_map (P) ;
    auto cls = [&] (i64 c) { const i64 len = cp [c + 1] - cp [c] ; return len <= PM_LEN1 ? 0 : len <= PM_LEN16 ? 1 : 2 ; } ;
    i64 first [4] = {0, 0, 0, 0} ;
    for (i64 c = 0 ; c < nc ; c++) first [cls (c) + 1]++ ;
    for (int k = 0 ; k < 3 ; k++) first [k + 1] += first [k] ;
    std::vector<i32> order ((size_t) nc) ;
    {
        i64 next [3] = {first [0], first [1], first [2]} ;
        for (i64 c = 0 ; c < nc ; c++) order [next [cls (c)]++] = (i32) c ;
    }
    const std::vector<i64> vcp (cp, cp + nc + 1), via (ia, ia + np), vib (ib, ib + np) ;
    hipError_t e = hipSuccess ;
    P->d_pm_cp = dupload (vcp, e) ;
    if (e == hipSuccess) P->d_pm_ia = dupload (via, e) ;
    if (e == hipSuccess) P->d_pm_ib = dupload (vib, e) ;
    if (e == hipSuccess) P->d_pm_order = dupload (order, e) ;
    if (e != hipSuccess)
    {
        const int rc = alloc_failure (e) ;
        drop_product_map (P) ;
        return rc ;
    }
    for (int k = 0 ; k < 4 ; k++) P->pm_class [k] = first [k] ;
    P->pm_na = navalues ;
    P->pm_set = true ;
    return CHOLMOD_HIP_OK ;
}

/* A values-only factorization whose values are in device memory already (cholmod_hip.h): the engine stream takes its
 * place behind the caller's, the values go from dvalues straight into the resident S -- through the product kernel and the
 * plan's d_vals first when they are to be computed -- and the factorization runs as on any resident S: the assembly
 * (k_assemble_mapped, one value of S per entry of L) is the first to read them.  No pinned buffer, no copy. */
int cholmod_hip_factorize_values_device (cholmod_hip_plan *P, const double *dvalues, int64_t nvalues,
    double beta, int quick_return_if_not_posdef, void *stream, int64_t *minor)
{
    if (!real_device_plan (P) || !dvalues || !minor) return CHOLMOD_HIP_INVALID ;
    if (!P->d_Sp || !P->d_vsrc || P->s_unpacked || P->vsrc_nz != P->s_cur_nz) return CHOLMOD_HIP_INVALID ;
    if (nvalues != (P->pm_set ? P->pm_na : P->vals_n)) return CHOLMOD_HIP_INVALID ;
    if (P->values_begun) return CHOLMOD_HIP_INVALID ;           // (a host upload is under way: its factorization comes first)
    hipStream_t user = (hipStream_t) stream, st = P->stream ;
    HIP_TRY (stream_enter (P, user)) ;
    const double *vals = dvalues ;
    if (P->pm_set)
    {
        const i64 *c = P->pm_class ;
#define PM_LAUNCH(G_, K_) if (c [K_ + 1] > c [K_]) \
            hipLaunchKernelGGL (k_product_values<G_>, dim3 ((unsigned) (((c [K_ + 1] - c [K_]) * G_ + 255) / 256)), dim3 (256), 0, st, \
                c [K_ + 1] - c [K_], P->d_pm_order + c [K_], P->d_pm_cp, P->d_pm_ia, P->d_pm_ib, dvalues, P->d_vals)
        PM_LAUNCH (1, 0) ; PM_LAUNCH (16, 1) ; PM_LAUNCH (64, 2) ;
#undef PM_LAUNCH
        vals = P->d_vals ;
    }
    if (P->vsrc_nz > 0)
        hipLaunchKernelGGL (k_gather_values, dim3 ((unsigned) ((P->vsrc_nz + 255) / 256)), dim3 (256), 0, st,
            P->vsrc_nz, P->d_vsrc, vals, P->d_Sx) ;
    HIPCHK (hipGetLastError ()) ;
    i64 m = P->n ;
    const int rc = run_factorize (P, beta, quick_return_if_not_posdef, &m) ;
    *minor = m ;
    if (rc < 0) return rc ;
    // (run_factorize has checked the launches and waited for the engine stream: what the caller enqueues next finds the
    // factor, and dvalues is free)
    HIP_TRY (stream_rejoin (P, user)) ;
    return rc ;
}

int cholmod_hip_download_matrix_values (cholmod_hip_plan *P, double *Sx_host)
{
    if (!P || P->host_only || !Sx_host || !P->d_Sp || !P->d_Sx) return CHOLMOD_HIP_INVALID ;
    HIPCHK (hipStreamSynchronize (P->stream)) ;
    if (P->s_cur_nz > 0) HIPCHK (hipMemcpy (Sx_host, P->d_Sx, (size_t) P->s_cur_nz * sizeof (double), hipMemcpyDeviceToHost)) ;
    return CHOLMOD_HIP_OK ;
}

} // extern "C"
