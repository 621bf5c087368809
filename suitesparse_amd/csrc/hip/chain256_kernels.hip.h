// chain256_kernels.hip.h -- gfx950 kernels of the panel chain in 256-column sub-blocks: k_diag + k_rowsolve, their
// one-launch form k_chainf, and ONE copy of every step the three share (engine.hip launches them, probes.hip times
// k_diag / k_rowsolve).  Uses find_group, pf_eliminate, trsm_diag_inverses and trsm_solve_rows of kernels.hip.h.
#pragma once
#include "kernels.hip.h"

namespace sship {

// ---- the panel chain in 256-column sub-blocks (opt-in: CHOLMOD_HIP_CHAIN256) ---------------
// The default chain walks a front's outer block column in 64-column steps: dpotrf of the
// diagonal block, dtrsm of ALL rows below, the K = 64 ... 256 doubling updates -- about fifteen
// dependent launches of 15-30 us per 512 columns.  This variant advances 256 columns per pair of
// launches (reference steps: dpotrf t_cholmod_super_numeric.c:864-867, dtrsm :997-1002, applied
// to a 256-column sub-block):
//   k_diag      ONE workgroup per front factors the w x w (w <= 256) diagonal sub-block, left-
//               looking over 64-column panels: the panel's 64 x 64 diagonal block is updated with
//               the sub-block's earlier columns on the matrix cores (operands straight from L2
//               in MFMA layout), eliminated in LDS (pf_eliminate), its rows inside the sub-block
//               solved as k_trsm_mfma does; the sixteen 16 x 16 diagonal-block inverses it needs
//               for that are published (dinv) for
//   k_rowsolve  every 64 rows below the sub-block, one workgroup: X = B inv(L)' for all w columns
//               at once -- per 64-column panel the rows of L it multiplies with are staged
//               k-major in LDS (negated), the solved 16 x 16 blocks of X stay in registers in
//               the A-operand layout (16 x d4 per wave) and feed the later panels' products; the
//               K < 256 "narrow updates" of the 64-column chain do not exist here, they are the
//               left-looking products inside these two kernels.
// Measured (round 3, MI355X): 2.3x fewer launches (nd24k stand-in 617 -> 273), same parity, but
// k_diag takes 126 us per full sub-block (four 64-column eliminations at ~11 us, whose column
// chain of ~250 cycles per column is what any variant waits for, plus the in-block solves) and
// k_rowsolve 39 us (544 MFMAs per wave, serial on its SIMD): 190 us per 256 columns against
// ~220 us for the 64-column chain's sixteen launches -- and slower where many fronts share a
// launch.  Poisson 100^3 156 against 150 ms, nd24k stand-in 32.9 against 29.4, 2D 1259^2 7.7
// against 5.3.  Kept as an option: a one-workgroup diagonal kernel is what a look-ahead on a
// CU-masked stream would need.
// Not-positive-definite protocol as everywhere: the first pivot <= 0 goes to info [front]
// (1-based, relative to the front), every later column of the front is written as zero.

// ---- the steps the three kernels share ----------------------------------------------------------------------------------
// Everywhere: lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4; a 16 x 64 slice in "accumulator layout" is
// d4 t [4], t [jb][r] = entry (this lane's row, column 16 jb + lk + 4 r).  COH: the access is one of k_chainf's hand-off
// accesses (relaxed agent-scope atomics, see there) instead of a plain one; which accesses are, the kernels decide.
__device__ __forceinline__ double ld_coh (const double *p) { return __hip_atomic_load (p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ; }
__device__ __forceinline__ void st_coh (double *p, double v) { __hip_atomic_store (p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ; }
template <bool COH> __device__ __forceinline__ double c256_ld (const double *p) { if constexpr (COH) return ld_coh (p) ; else return *p ; }
template <bool COH> __device__ __forceinline__ void c256_st (double *p, double v) { if constexpr (COH) st_coh (p, v) ; else *p = v ; }

// valid columns of the sub-block [col0, col0 + w) of a front whose info is inf (0, or 1 + its first failed column)
__device__ __forceinline__ int c256_valid_cols (int inf, int col0, int w)
{
    int nvt = w ;
    if (inf != 0) { nvt = inf - 1 - col0 ; if (nvt < 0) nvt = 0 ; if (nvt > w) nvt = w ; }
    return nvt ;
}

// t = the columns c0 .. c0 + 63 of this lane's row of L, clamped to the sub-block's last (w - 1: the same as clamping to the
// panel's last, c0 + pw - 1); p = the row's entry in the sub-block's column 0
__device__ __forceinline__ void c256_load_tile (d4 (&t) [4], const double *p, i64 lda, int c0, int w, int lk)
{
#pragma unroll
    for (int jb = 0 ; jb < 4 ; jb++)
#pragma unroll
        for (int r = 0 ; r < 4 ; r++)
        {
            int col = c0 + 16 * jb + lk + 4 * r ; if (col > w - 1) col = w - 1 ;
            t [jb][r] = p [(i64) col * lda] ;
        }
}

// a panel's updated pw x pw diagonal block from the accumulators into T (k-major): its lower triangle, identity-padded to 64
__device__ __forceinline__ void c256_acc_to_T (double *T, const d4 (&acc) [4], int pw, int wave, int lr, int lk)
{
#pragma unroll
    for (int jb = 0 ; jb < 4 ; jb++)
#pragma unroll
        for (int r = 0 ; r < 4 ; r++)
        {
            const int i = 16 * wave + lr, j = 16 * jb + lk + 4 * r ;
            T [j * PF2_LD + i] = (i < pw && j < pw) ? (i >= j ? acc [jb][r] : 0.0) : (i == j ? 1.0 : 0.0) ;
        }
}

// the factored block from T to L (A = entry (0, 0) of the sub-block, the block at (c0, c0); columns at / beyond a failed
// pivot: zero), and -L11 k-major (diagonal positive, identity-padded) into Ls for the inverses and the row solves
template <bool COH>
__device__ __forceinline__ void c256_factored_block (const double *T, double *Ls, double *A, i64 lda, int c0, int pw, int nvalid, int wave, int lane)
{
#pragma unroll
    for (int q = 0 ; q < 16 ; q++)
    {
        const int k = wave + 4 * q, i = lane ;
        if (k < pw && i >= k && i < pw) c256_st<COH> (&A [(c0 + i) + (i64) (c0 + k) * lda], (k < nvalid) ? T [k * PF2_LD + i] : 0.0) ;
        double v = (i == k) ? 1.0 : 0.0 ;
        if (i < nvalid && k < i) v = -T [k * PF2_LD + i] ;
        if (i < nvalid && k == i) v = T [k * PF2_LD + k] ;
        Ls [k * 64 + i] = v ;
    }
}

// stage the rows c0 .. c0 + 63 of L (L = entry (0, 0) of the sub-block), columns kb .. kb + 63, into Lst [k][c] k-major:
// -L (c0 + c, k) for k < c0 + c, the diagonal entry itself, identity elsewhere and in the rows c >= nvc (not valid);
// sixteen loads in flight per thread
template <bool COH>
__device__ __forceinline__ void c256_stage_batch (double *Lst, const double *L, i64 lda, int w, int c0, int kb, int nvc, int lane, int wave)
{
    const int c = lane ;
    const int rowL = (c0 + c < w) ? c0 + c : w - 1 ;
    double tmp [16] ;
#pragma unroll
    for (int q = 0 ; q < 16 ; q++)
    {
        int k = kb + wave + 4 * q ; if (k > w - 1) k = w - 1 ;
        tmp [q] = c256_ld<COH> (L + rowL + (i64) k * lda) ;
    }
#pragma unroll
    for (int q = 0 ; q < 16 ; q++)
    {
        const int k = kb + wave + 4 * q ;
        double v = (k == c0 + c) ? 1.0 : 0.0 ;
        if (c < nvc && k < c0 + c) v = -tmp [q] ;
        if (c < nvc && k == c0 + c) v = tmp [q] ;
        Lst [k * 64 + c] = v ;
    }
}

// acc - sum over k0 <= kb < k1 of X_kb L (16 jb .., 16 kb ..)' out of the staging.  k0, k1 and jb are constants once the
// caller's loops are unrolled: X [] is indexed by compile-time constants and stays in registers.
// (four partial sums: a dependent fp64 MFMA costs ~190 cycles, an independent one 64)
__device__ __forceinline__ d4 c256_products (d4 acc, const d4 (&X) [16], const double *Lst, int k0, int k1, int jb, int lr, int lk)
{
    d4 a1 = (d4) {0.0, 0.0, 0.0, 0.0}, a2 = a1, a3 = a1 ;
#pragma unroll
    for (int kb = 0 ; kb < 16 ; kb++)
    {
        if (kb >= k0 && kb < k1)
        {
            double b [4] ;
#pragma unroll
            for (int s4 = 0 ; s4 < 4 ; s4++) b [s4] = Lst [(16 * kb + 4 * s4 + lk) * 64 + 16 * jb + lr] ;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64 (b [0], X [kb][0], acc, 0, 0, 0) ;
            a1 = __builtin_amdgcn_mfma_f64_16x16x4f64 (b [1], X [kb][1], a1, 0, 0, 0) ;
            a2 = __builtin_amdgcn_mfma_f64_16x16x4f64 (b [2], X [kb][2], a2, 0, 0, 0) ;
            a3 = __builtin_amdgcn_mfma_f64_16x16x4f64 (b [3], X [kb][3], a3, 0, 0, 0) ;
        }
    }
    return (acc + a1) + (a2 + a3) ;
}

// the solved block: acc times the jb-th 16 x 16 inverse in Wd, its columns at / past a failed pivot (c >= nvj) zero
__device__ __forceinline__ d4 c256_apply_inverse (d4 acc, const double *Wd, int jb, int nvj, int lr, int lk)
{
    d4 x = (d4) {0.0, 0.0, 0.0, 0.0} ;
#pragma unroll
    for (int s4 = 0 ; s4 < 4 ; s4++)
    {
        double b = Wd [jb * 256 + (4 * s4 + lk) * 16 + lr] ;
        x = __builtin_amdgcn_mfma_f64_16x16x4f64 (b, acc [s4], x, 0, 0, 0) ;
    }
#pragma unroll
    for (int r = 0 ; r < 4 ; r++) x [r] = (16 * jb + lk + 4 * r < nvj) ? x [r] : 0.0 ;
    return x ;
}
// ... and into L: P = this lane's row of the panel's first column, ncol = the panel's width, 0 for a lane that must not store
// (no row of its own).  Nearly every lane stores: without the hint the stores are laid out as out-of-line branches (k_rowsolve 42.1 -> 43.2 us)
template <bool COH>
__device__ __forceinline__ void c256_store_block (d4 x, double *P, i64 lda, int jb, int ncol, int lk)
{
#pragma unroll
    for (int r = 0 ; r < 4 ; r++) if (__builtin_expect (16 * jb + lk + 4 * r < ncol, 1)) c256_st<COH> (P + (i64) (16 * jb + lk + 4 * r) * lda, x [r]) ;
}

template <typename Tick>
__device__ __forceinline__ void dg_left_looking (d4 (&acc) [4], const double *A, i64 lda, int rowc, int c0, int w, int lr, int lk, Tick)
{
    // acc [jb] -= L (rowc, 0 : c0) L (c0 + 16 jb + lr', 0 : c0)'   (rows of the wave in lanes lr, columns lk + 4 r)
    const double *pa = A + rowc + (i64) lk * lda ;
    const double *pb [4] ;
#pragma unroll
    for (int jb = 0 ; jb < 4 ; jb++)
    {
        int rb = c0 + 16 * jb + lr ; if (rb > w - 1) rb = w - 1 ;
        pb [jb] = A + rb + (i64) lk * lda ;
    }
    // (c0 is a multiple of 64: batches of 32 columns, all forty loads of a batch in flight before its MFMAs.
    // Fetching the next batch under this batch's MFMAs was tried: 160 more registers, spills, 130 -> 219 us.)
    for (int k0 = 0 ; k0 < c0 ; k0 += 32)
    {
        double af [8], bf [8][4] ;
#pragma unroll
        for (int u = 0 ; u < 8 ; u++)
        {
            af [u] = pa [(i64) (k0 + 4 * u) * lda] ;
#pragma unroll
            for (int jb = 0 ; jb < 4 ; jb++) bf [u][jb] = pb [jb][(i64) (k0 + 4 * u) * lda] ;
        }
#pragma unroll
        for (int u = 0 ; u < 8 ; u++)
#pragma unroll
            for (int jb = 0 ; jb < 4 ; jb++)
                acc [jb] = __builtin_amdgcn_mfma_f64_16x16x4f64 (-bf [u][jb], af [u], acc [jb], 0, 0, 0) ;
    }
}

template <bool TIMED>
__global__ void __launch_bounds__(256) k_diag (const DgGroup *g, double *Lx, i32 *info, double *dinv, long long *tim)
{
    long long tc [8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_prev = 0 ;
    auto stamp = [&] (int slot) { if constexpr (TIMED) { long long t = __builtin_readcyclecounter () ; tc [slot] += t - t_prev ; t_prev = t ; } } ;
    if constexpr (TIMED) t_prev = __builtin_readcyclecounter () ;
    __shared__ __attribute__((aligned(16))) double T [PF_NB * PF2_LD] ;     // the panel's 64 x 64 diagonal block, k-major
    __shared__ __attribute__((aligned(16))) double Ls [64 * 64] ;           // -L11 k-major (diagonal positive), identity-padded
    __shared__ __attribute__((aligned(16))) double Wd [4 * 256] ;           // inverses of its four 16 x 16 diagonal blocks
    __shared__ int s_fail ;
    __builtin_amdgcn_s_setprio (3) ;
    const DgGroup G = g [blockIdx.x] ;
    double *A = Lx + G.off ;
    const i64 lda = G.lda ;
    const int w = G.w ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    double *DI = dinv + (i64) G.slot * 4096 ;
    auto tick = [] (int) {} ;
    bool dead = info [G.front] != 0 ;        // an earlier pivot of this front failed
    for (int c0 = 0 ; c0 < w ; c0 += 64)
    {
        const int pw = (w - c0 < 64) ? w - c0 : 64 ;
        if (dead)
        {
            // the front's remaining columns are zero (:889-895, :926-931); identity "inverses" so
            // that nothing non-finite reaches k_rowsolve's (masked) products
            for (int k = wave ; k < pw ; k += 4)
                for (int i = c0 + k + lane ; i < w ; i += 64) A [i + (i64) (c0 + k) * lda] = 0.0 ;
            for (int e = tid ; e < 1024 ; e += 256) DI [(c0 >> 6) * 1024 + e] = ((e & 255) >> 4) == (e & 15) ? 1.0 : 0.0 ;
            continue ;
        }
        // ---- the panel's diagonal block: this wave's 16 rows, left-looking update, into T
        {
            const int rowg = c0 + 16 * wave + lr ;
            const int rowc = rowg < w ? rowg : w - 1 ;
            d4 acc [4] ;
            c256_load_tile (acc, A + rowc, lda, c0, w, lk) ;
            dg_left_looking (acc, A, lda, rowc, c0, w, lr, lk, tick) ;
            stamp (0) ;
            c256_acc_to_T (T, acc, pw, wave, lr, lk) ;
        }
        if (tid == 0) s_fail = -1 ;
        __syncthreads () ;
        stamp (1) ;
        pf_eliminate (T, (pw + 15) >> 4, &s_fail, tid, tick) ;
        stamp (2) ;
        const int fail = s_fail ;
        const int nvalid = fail >= 0 ? fail : pw ;
        if (fail >= 0 && tid == 0) info [G.front] = G.col0 + c0 + fail + 1 ;
        c256_factored_block<false> (T, Ls, A, lda, c0, pw, nvalid, wave, lane) ;
        __syncthreads () ;
        stamp (3) ;
        trsm_diag_inverses (Ls, 64, Wd, 4, lane, wave, tick) ;
        __syncthreads () ;
        for (int e = tid ; e < 1024 ; e += 256) DI [(c0 >> 6) * 1024 + e] = Wd [e] ;
        stamp (4) ;
        // ---- the rows of the sub-block below this panel (only behind a full panel)
        for (int rr = c0 + 64 ; rr < w ; rr += 64)
        {
            const int row = rr + 16 * wave + lr ;
            const bool rok = row < w ;
            const int rowc = rok ? row : w - 1 ;
            d4 bj [4], xr [4] ;
#pragma unroll
            for (int jb = 0 ; jb < 4 ; jb++)
#pragma unroll
                for (int r = 0 ; r < 4 ; r++) bj [jb][r] = A [rowc + (i64) (c0 + 16 * jb + lk + 4 * r) * lda] ;
            dg_left_looking (bj, A, lda, rowc, c0, w, lr, lk, tick) ;
            stamp (5) ;
            trsm_solve_rows<false> (bj, 4, Ls, 64, Wd, lane, nvalid, rok, 64, A + (i64) c0 * lda, rowc, lda, tick, xr) ;
            stamp (6) ;
        }
        if (fail >= 0) dead = true ;
        __syncthreads () ;          // this panel's columns are in Lx for the next panel's products (workgroup scope)
        stamp (7) ;
    }
    if constexpr (TIMED) { if (tid == 0) for (int q = 0 ; q < 8 ; q++) tim [q] = tc [q] ; }
}

__host__ __device__ inline size_t rowsolve_lds_bytes () { return (size_t) (DG_W * 64 + 4 * 256) * sizeof (double) ; }
__global__ void __launch_bounds__(256) k_rowsolve (const RsGroup *g, int ng, double *Lx, const i32 *info, const double *dinv)
{
    extern __shared__ __attribute__((aligned(16))) double rs_lds [] ;
    double *Lst = rs_lds ;                  // [k][c]: -L (c0 + c, k) for k < c0 + c (k-major, 64 columns wide), identity-padded
    double *Wd = Lst + DG_W * 64 ;          // the panel's four 16 x 16 diagonal-block inverses (from k_diag)
    const int gi = find_group (g, ng, (int) blockIdx.x, &RsGroup::blk_start) ;
    const RsGroup G = g [gi] ;
    const i64 lda = G.lda ;
    const int w = G.w ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const int row = ((int) blockIdx.x - G.blk_start) * RS_ROWS + wave * 16 + lr ;
    const bool rok = row < G.m ;
    double *B = Lx + G.b_off + (rok ? row : G.m - 1) ;       // this lane's row, first column of the sub-block
    const double *L = Lx + G.l_off ;                          // L (0, 0) of the sub-block
    const double *DI = dinv + (i64) G.slot * 4096 ;
    const int nvt = c256_valid_cols (info [G.front], G.col0, w) ;
    d4 X [16] ;
#pragma unroll
    for (int q = 0 ; q < 16 ; q++) X [q] = (d4) {0.0, 0.0, 0.0, 0.0} ;
    // one 64-column panel; j is a compile-time constant so that X [] stays in registers
    auto panel = [&] (auto jc)
    {
        constexpr int j = decltype (jc)::value ;
        constexpr int c0 = 64 * j ;
        if (c0 < w)
        {
            const int pw = (w - c0 < 64) ? w - c0 : 64 ;
            int nvj = nvt - c0 ; if (nvj < 0) nvj = 0 ; if (nvj > pw) nvj = pw ;
            d4 bj [4] ;
            c256_load_tile (bj, B, lda, c0, w, lk) ;
            __syncthreads () ;              // the previous panel's readers are done with Lst / Wd
            // stage the rows c0 .. c0 + 63 of L, columns 0 .. c0 + 63, and the panel's inverses (all j + 1 batches unrolled: 41.1 us
            // against 42.1 with the loop left to the compiler, which the written-out copy had at 41.6)
#pragma unroll
            for (int kb = 0 ; kb < c0 + 64 ; kb += 64) c256_stage_batch<false> (Lst, L, lda, w, c0, kb, nvj, lane, wave) ;
            for (int e = tid ; e < 1024 ; e += 256) Wd [e] = DI [j * 1024 + e] ;
            __syncthreads () ;
#pragma unroll
            for (int jb = 0 ; jb < 4 ; jb++)
            {
                const d4 x = c256_apply_inverse (c256_products (bj [jb], X, Lst, 0, 4 * j + jb, jb, lr, lk), Wd, jb, nvj, lr, lk) ;
                c256_store_block<false> (x, B + (i64) c0 * lda, lda, jb, rok ? pw : 0, lk) ;
                X [4 * j + jb] = x ;
            }
        }
    } ;
    panel (std::integral_constant<int, 0> {}) ;
    panel (std::integral_constant<int, 1> {}) ;
    panel (std::integral_constant<int, 2> {}) ;
    panel (std::integral_constant<int, 3> {}) ;
}

// ---- the 256-column chain in ONE launch (round 4): k_chainf -----------------------------------
// k_diag + k_rowsolve fused, with the diagonal sub-block's work spread over four workgroups instead
// of one.  Every workgroup owns 64 rows of a front's sub-block column [col0, col0 + w), w <= 256,
// for the whole launch:
//   * row block rb < nd = ceil (w / 64) lies INSIDE the w x w diagonal sub-block ("diagonal
//     workgroup"): it solves its rows against the panels j < rb exactly as a row workgroup does, then
//     subtracts its own X X' from its 64 x 64 diagonal block, eliminates it (pf_eliminate), inverts
//     the four 16 x 16 diagonal blocks and PUBLISHES row block rb of L (its solved blocks, L_rb,rb,
//     the inverses) -- the critical path per 64 columns is solve + syrk + elimination of ONE
//     workgroup (k_diag: one workgroup did all four row blocks' solves and products as well);
//   * the row blocks below the sub-block ("row workgroups") are k_rowsolve: per panel j they stage
//     row block j of L k-major in LDS and multiply out of registers -- but wait, per panel, for
//     diagonal workgroup j's flag instead of a kernel boundary.
// Hand-off without an L2 write-back: everything a diagonal workgroup publishes is written with
// relaxed agent-scope atomic stores (global_store ... sc1: write-through past the XCD's L2) and read
// with relaxed agent-scope atomic loads (sc1: served at the coherence point); the flag follows the
// data after an explicit s_waitcnt vmcnt(0) in every wave + the workgroup barrier (cf_drain_stores;
// checked in the gfx950 ISA: waitcnt, s_barrier, flag store) -- no buffer_wbl2 / buffer_inv, which
// is what made the cross-workgroup hand-off of round 2 cost 30 us.  A workgroup only ever waits for
// workgroups with a LOWER block index (all diagonal workgroups of a launch come first, in panel
// order per front), so in-order dispatch cannot deadlock; a wait that exceeds its budget raises
// *err (the host reports CHOLMOD_HIP_GPU_PROBLEM) instead of hanging the device.
// flags [4 slot + j]: low byte = stages of row block j published (s <= j: its solved blocks of the panels
// < s; j + 1: its diagonal block and the inverses as well), then bits 8.. = 1 + nvt, nvt = valid columns
// of the sub-block so far (w when no pivot has failed).
// rows below the sub-block: [w, w + m1) and, for a front shared between ranks (its block column dealt by row chunks), two
// more ranges [off2, off2 + m2) and [off3, off3 + m3) -- the rest of the 512-wide diagonal block on every rank, then this
// rank's chunk of the near rows (inside the outer block column) and its chunk of the far rows
// polls (s_sleep 4 + one coherent load, ~1.5 us each) before a hand-off counts as failed: ~6 s, far beyond any jitter
// hold or time slice another process of the device can cause (the host then reports CHOLMOD_HIP_GPU_PROBLEM on all ranks)
#define CF_SPIN_LIMIT (1 << 22)
// all of this wave's global stores (and loads) acknowledged; also a compiler barrier for memory operations
__device__ __forceinline__ void cf_drain_stores () { asm volatile ("s_waitcnt vmcnt(0)" ::: "memory") ; }
__host__ __device__ inline size_t chainf_lds_bytes () { return (size_t) (DG_W * 64 + 4 * 256 + 16) * sizeof (double) ; }
__global__ void __launch_bounds__(256) k_chainf (const CfGroup *g, int ng, int ndiag_total, double *Lx, i32 *info,
    double *dinv, int *flags, int *err)
{
    extern __shared__ __attribute__((aligned(16))) double cf_lds [] ;
    double *Lst = cf_lds ;                  // [k][c]: -L (c0 + c, k), k-major, 64 columns wide (row workgroup phase)
    double *Wd = Lst + DG_W * 64 ;          // four 16 x 16 diagonal-block inverses of the current panel
    int *s_int = (int *) (Wd + 4 * 256) ;   // [0] broadcast of a polled flag, [1] s_fail
    double *T = Lst ;                       // (diagonal phase, after the panels: the 64 x 64 block, k-major)
    double *Lsd = Lst + PF_NB * PF2_LD ;    // (diagonal phase: -L11 k-major for the inverses)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const bool isdiag = (int) blockIdx.x < ndiag_total ;
    int gi ;
    if (isdiag) gi = find_group (g, ng, (int) blockIdx.x, &CfGroup::dstart) ;
    else gi = find_group (g, ng, (int) blockIdx.x - ndiag_total, &CfGroup::bstart) ;
    const CfGroup G = g [gi] ;
    const i64 lda = G.lda ;
    const int w = G.w ;
    const int nd = (w + 63) >> 6 ;
    const int rb = isdiag ? (int) blockIdx.x - G.dstart : nd ;
    int row0 = 64 * rb, rowend = w ;
    if (!isdiag)
    {
        const int t = (int) blockIdx.x - ndiag_total - G.bstart, n1 = (G.m1 + 63) >> 6, n2 = (G.m2 + 63) >> 6 ;
        if (t < n1) { row0 = w + 64 * t ; rowend = w + G.m1 ; }
        else if (t < n1 + n2) { row0 = G.off2 + 64 * (t - n1) ; rowend = G.off2 + G.m2 ; }
        else { row0 = G.off3 + 64 * (t - n1 - n2) ; rowend = G.off3 + G.m3 ; }
    }
    const int row = row0 + 16 * wave + lr ;
    const bool rok = row < rowend ;
    double *Lb = Lx + G.l_off ;                               // L (0, 0) of the sub-block
    double *B = Lb + (rok ? row : rowend - 1) ;               // this lane's row, first column of the sub-block
    double *DI = dinv + (i64) G.slot * 4096 ;
    int *fl = flags + 4 * (i64) G.fslot ;
    if (isdiag) __builtin_amdgcn_s_setprio (3) ; else __builtin_amdgcn_s_setprio (1) ;
    bool dead = false ;                                       // a hand-off timed out (wait_stage): no store into L from here on
    if (tid == 0) s_int [2] = 0 ;                             // (read after wait_stage's barrier only)
    int nvt = c256_valid_cols (info [G.front], G.col0, w) ;   // valid columns of the sub-block (a pivot of an EARLIER launch failed)
    // Row block j of L is published in stages: flag j = s (1 <= s <= j) once its solved blocks of the panels < s are
    // written, and (j + 1) | (1 + nvt) << 8 once its diagonal block and the inverses are.  Thread 0 polls until the stage
    // exceeds `have`; the value travels through LDS.
    auto wait_stage = [&] (int j, int have) -> int
    {
        if (tid == 0)
        {
            int v = 0, n = 0 ;
            while (((v = __hip_atomic_load (fl + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xFF) <= have)
            {
                __builtin_amdgcn_s_sleep (4) ;
                // budget exceeded (or somebody else's was: no second full wait behind a dead workgroup): tell the host, go
                // on as "nothing valid" and DEAD -- a dead workgroup stores nothing into L any more, it only keeps
                // publishing its flags so that the workgroups behind it come to an end as well
                if (++n > CF_SPIN_LIMIT || ((n & 1023) == 0 && __hip_atomic_load (err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0))
                {
                    atomicExch (err, 1) ; v = (j + 1) | (1 << 8) ; s_int [2] = 1 ; break ;
                }
            }
            s_int [0] = v ;
        }
        __syncthreads () ;
        if (s_int [2]) dead = true ;
        return s_int [0] ;
    } ;
    d4 X [16] ;
#pragma unroll
    for (int q = 0 ; q < 16 ; q++) X [q] = (d4) {0.0, 0.0, 0.0, 0.0} ;
    // a diagonal workgroup: its 64 x 64 diagonal block in registers from the start (accumulator layout), updated panel by
    // panel; Xp = the LDS rows k >= 192 of Lst, which a diagonal workgroup (panels j <= 2: k < 192) never stages into
    double *Xp = Lst + 192 * 64 ;
    d4 dacc [4] ;
#pragma unroll
    for (int jb = 0 ; jb < 4 ; jb++) dacc [jb] = (d4) {0.0, 0.0, 0.0, 0.0} ;
    if (isdiag) c256_load_tile (dacc, B, lda, row0, w, lk) ;         // (here row0 = 64 rb and rowend = w: B is the clamped row)
    // one 64-column panel left of this workgroup's rows (k_rowsolve's panel; j is a compile-time constant so that X [] stays in registers)
    auto panel = [&] (auto jc)
    {
        constexpr int j = decltype (jc)::value ;
        constexpr int c0 = 64 * j ;
        if (j < rb && c0 < w)
        {
            const int pw = (w - c0 < 64) ? w - c0 : 64 ;
            d4 bj [4] ;
            c256_load_tile (bj, B, lda, c0, w, lk) ;
            // stage the rows c0 .. c0 + 63 of L, columns 0 .. c0 + 63, following diagonal workgroup j's stages: the
            // columns of the earlier panels while it is still busy with the later ones, so that only its diagonal
            // block (16 loads) and the inverses are left to fetch when its last flag arrives (coherent loads)
            int have = 0, nvj = 0 ;
            // (1) the columns of the EARLIER panels, as diagonal workgroup j publishes them (it is still busy with the later ones)
            while (have < j)
            {
                const int fv = wait_stage (j, have) ;      // (ends with a barrier: the previous panel's readers are done with Lst / Wd)
                int upto = fv & 0xFF ; if (upto > j) upto = j ;
                // (in these columns every row c0 + c counts as valid, nvc = 64 -- what it feeds are output columns that
                // are masked if it is not, see the note at the products)
                for (int p = have ; p < upto ; p++) c256_stage_batch<true> (Lst, Lb, lda, w, c0, 64 * p, 64, lane, wave) ;
                have = upto ;
            }
            // (2) ... and the products with them, BEFORE the last flag: pre [jb] = B_jb - sum_{kb < 4 j} X_kb L (16 jb .., 16 kb ..)'
            // (a row of L past a failed pivot enters only output columns at / past that pivot, which are written as zero)
            d4 pre [4] ;
            if (j > 0) __syncthreads () ;
#pragma unroll
            for (int jb = 0 ; jb < 4 ; jb++) pre [jb] = c256_products (bj [jb], X, Lst, 0, 4 * j, jb, lr, lk) ;
            // (3) the last stage: its diagonal block (16 loads) and the inverses
            {
                const int fv = wait_stage (j, j) ;
                const int pv = (fv >> 8) - 1 ;
                if (pv < nvt) nvt = pv ;
                nvj = nvt - c0 ; if (nvj < 0) nvj = 0 ; if (nvj > pw) nvj = pw ;
                c256_stage_batch<true> (Lst, Lb, lda, w, c0, c0, nvj, lane, wave) ;
                for (int e = tid ; e < 1024 ; e += 256) Wd [e] = ld_coh (DI + j * 1024 + e) ;
            }
            __syncthreads () ;
#pragma unroll
            for (int jb = 0 ; jb < 4 ; jb++)
            {
                const d4 x = c256_apply_inverse (c256_products (pre [jb], X, Lst, 4 * j, 4 * j + jb, jb, lr, lk), Wd, jb, nvj, lr, lk) ;
                // (a diagonal workgroup's solved blocks are row block rb of L for everybody after it)
                if (isdiag) c256_store_block<true> (x, B + (i64) c0 * lda, lda, jb, (rok && !dead) ? pw : 0, lk) ;
                else c256_store_block<false> (x, B + (i64) c0 * lda, lda, jb, (rok && !dead) ? pw : 0, lk) ;
                X [4 * j + jb] = x ;
            }
            if (isdiag)
            {
                // this row block's solved blocks through panel j are written (stage j + 1: the workgroups after it prefetch them)
                // ... and its own diagonal block takes their product right away, dacc -= X_j X_j' (K = 64: B operands
                // through LDS, A operands = the registers), so that only the LAST panel's is left when the last flag comes
#pragma unroll
                for (int kb2 = 0 ; kb2 < 4 ; kb2++)
#pragma unroll
                    for (int s4 = 0 ; s4 < 4 ; s4++) Xp [(16 * kb2 + lk + 4 * s4) * 64 + 16 * wave + lr] = X [4 * j + kb2][s4] ;
                __syncthreads () ;
#pragma unroll
                for (int kb2 = 0 ; kb2 < 4 ; kb2++)
#pragma unroll
                    for (int s4 = 0 ; s4 < 4 ; s4++)
#pragma unroll
                        for (int jb = 0 ; jb < 4 ; jb++)
                        {
                            const double bfv = Xp [(16 * kb2 + 4 * s4 + lk) * 64 + 16 * jb + lr] ;
                            dacc [jb] = __builtin_amdgcn_mfma_f64_16x16x4f64 (-bfv, X [4 * j + kb2][s4], dacc [jb], 0, 0, 0) ;
                        }
                // (the stage flag after the product: every wave drains ITS stores -- s_waitcnt vmcnt(0), stores count in
                // vmcnt on gfx9 -- before the barrier the flag store follows; a workgroup-scope release fence emits lgkmcnt only
                // and s_barrier waits for nothing.  By now the stores are acknowledged, so the wait is free.)
                cf_drain_stores () ;
                __syncthreads () ;
                if (tid == 0) __hip_atomic_store (fl + rb, j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ;
            }
        }
    } ;
    panel (std::integral_constant<int, 0> {}) ;
    panel (std::integral_constant<int, 1> {}) ;
    panel (std::integral_constant<int, 2> {}) ;
    panel (std::integral_constant<int, 3> {}) ;
    if (!isdiag) return ;
    // ---- diagonal workgroup rb: its own 64 x 64 diagonal block
    const int c0 = 64 * rb ;
    const int pw = (w - c0 < 64) ? w - c0 : 64 ;
    __syncthreads () ;                      // (the last panel's readers are done with Lst / Xp: T and Lsd overlay Lst)
    auto tick = [] (int) {} ;
    int nv_out = nvt ;
    if (dead) { }
    else if (nvt <= c0)
    {
        // an earlier pivot failed: this panel's columns are zero (:889-895, :926-931), identity "inverses"
        for (int k = wave ; k < pw ; k += 4)
            for (int i = c0 + k + lane ; i < c0 + pw ; i += 64) st_coh (Lb + i + (i64) (c0 + k) * lda, 0.0) ;
        for (int e = tid ; e < 1024 ; e += 256) st_coh (DI + rb * 1024 + e, ((e & 255) >> 4) == (e & 15) ? 1.0 : 0.0) ;
    }
    else
    {
        c256_acc_to_T (T, dacc, pw, wave, lr, lk) ;
        if (tid == 0) s_int [1] = -1 ;
        __syncthreads () ;
        pf_eliminate (T, (pw + 15) >> 4, &s_int [1], tid, tick) ;
        const int fail = s_int [1] ;
        const int nvalid = fail >= 0 ? fail : pw ;
        if (fail >= 0) { nv_out = c0 + fail ; if (tid == 0) info [G.front] = G.col0 + c0 + fail + 1 ; }
        c256_factored_block<true> (T, Lsd, Lb, lda, c0, pw, nvalid, wave, lane) ;
        __syncthreads () ;
        trsm_diag_inverses (Lsd, 64, Wd, 4, lane, wave, tick) ;
        __syncthreads () ;
        for (int e = tid ; e < 1024 ; e += 256) st_coh (DI + rb * 1024 + e, Wd [e]) ;
    }
    // publish: every wave waits for the acknowledgement of its own write-through stores (vmcnt(0)), the barrier collects the
    // four waves, then the flag goes out -- data before flag at the coherence point, still without buffer_wbl2 / buffer_inv
    cf_drain_stores () ;
    __syncthreads () ;
    if (tid == 0) __hip_atomic_store (fl + rb, (rb + 1) | ((1 + nv_out) << 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ;
}

} // namespace sship
