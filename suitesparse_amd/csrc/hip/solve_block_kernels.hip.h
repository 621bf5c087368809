// solve_block_kernels.hip.h -- triangular solves with a panel of 16 right-hand sides (cholmod_hip_solve_device).
//
// The kernels of kernels.hip.h sweep L once per right-hand side.  Here the right-hand sides travel 16 at a time
// in a panel workspace W [n][16], the right-hand side index fastest: row k of the permuted system is one 128-byte
// line, so a gather or scatter by Ls [i] touches one line per row, and every product with L is a sequence of
// v_mfma_f64_16x16x4 tiles -- L is read once per panel (the reference's dtrsm / dgemm branch,
// t_cholmod_super_solve.c:164-173, :368-379).  A panel narrower than 16 has zero columns: they stay zero.
//
// Lane maps of v_mfma_f64_16x16x4 (lr = lane & 15, lk = lane >> 4): first operand A [row lr][k lk], second operand
// B [k lk][column lr], result register r = D [row lk + 4 r][column lr].  The column is always the right-hand side,
// so the four result registers of a lane group are 16 lanes x 8 bytes of one row of W.
//
// The schedule is the plan's: the whole-supernode tasks of a level (SolveTask, one workgroup each) and the
// 256-column blocks of the big supernodes (SolveBlk, the launches of sb_launch) with their explicit 64 x 64
// inverses (k_diag_inv64).  Real factors only.
#pragma once
#include "kernels.hip.h"

namespace sship {

#define SD_NP 16        /* right-hand sides per panel */

__device__ __forceinline__ d4 sd_zero () { d4 z = {0.0, 0.0, 0.0, 0.0} ; return z ; }

// acc (rows i0 .. i0+15, 16 right-hand sides) += M [i0 .., 0 .. K) * Xs [0 .. K)[.]
// M: column-major, leading dimension ld (16 consecutive rows of a column per lane group: coalesced), rows >= ilim
// read as zero; Xs: LDS, [K][16].
__device__ __forceinline__ d4 sd_mul_nx (const double *M, int ld, int i0, int ilim, int K, const double *Xs,
    d4 acc, int lr, int lk)
{
    const int i = i0 + lr ;
    const bool rok = i < ilim ;
    const double *Mi = M + (rok ? i : 0) ;
    for (int k0 = 0 ; k0 < K ; k0 += 4)
    {
        const int k = k0 + lk ;
        const bool ok = k < K ;
        const double a = (rok && ok) ? Mi [(i64) k * ld] : 0.0 ;
        const double b = ok ? Xs [k * SD_NP + lr] : 0.0 ;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64 (a, b, acc, 0, 0, 0) ;
    }
    return acc ;
}

// acc (columns j0 .. j0+15 of M, 16 right-hand sides) += sum over rows i = ia, ia + 1, .. (16 at a time, then
// istep further on) below ib of M [i, j0 ..]' y (i)[.]
// A lane reads four consecutive rows of its column (lk-th quarter of the 16): a lane group covers 128 contiguous
// bytes of each of its 16 columns, and the four values feed four k-steps.  Columns >= jlim read as zero.
template <class YF>
__device__ __forceinline__ d4 sd_mul_ty (const double *M, int ld, int j0, int jlim, int ia, int ib, int istep,
    YF y, d4 acc, int lr, int lk)
{
    const int j = j0 + lr ;
    const bool cok = j < jlim ;
    const double *Mc = M + (i64) (cok ? j : j0) * ld ;
    for (int ibase = ia ; ibase < ib ; ibase += istep)
    {
        double a [4], b [4] ;
#pragma unroll
        for (int s = 0 ; s < 4 ; s++)
        {
            const int i = ibase + 4 * lk + s ;
            const bool ok = i < ib ;
            a [s] = (ok && cok) ? Mc [i] : 0.0 ;
            b [s] = ok ? y (i, lr) : 0.0 ;
        }
#pragma unroll
        for (int s = 0 ; s < 4 ; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64 (a [s], b [s], acc, 0, 0, 0) ;
    }
    return acc ;
}

// ---- pack / unpack: B (column-major, ldb) through Perm into W, W through Perm into X ------------------------------
// One workgroup = 256 rows of the permuted system, transposed through LDS: a right-hand side is read / written
// along its column, W along its lines.  pw = width of this panel (<= 16): the missing columns of W are zero and
// are never written to X.
__global__ void __launch_bounds__(256) k_sd_pack (i64 n, const i64 *perm, const double *B, i64 ldb, int pw, double *W)
{
    __shared__ double tile [256 * 17] ;
    const int tid = threadIdx.x ;
    const i64 k0 = blockIdx.x * (i64) 256, k = k0 + tid ;
    if (k < n)
    {
        const i64 src = perm ? perm [k] : k ;
        for (int r = 0 ; r < SD_NP ; r++) tile [tid * 17 + r] = (r < pw) ? B [src + (i64) r * ldb] : 0.0 ;
    }
    __syncthreads () ;
    for (int e = tid ; e < 256 * SD_NP ; e += 256)
        if (k0 + (e >> 4) < n) W [k0 * SD_NP + e] = tile [(e >> 4) * 17 + (e & 15)] ;
}

__global__ void __launch_bounds__(256) k_sd_unpack (i64 n, const i64 *perm, const double *W, int pw, double *X, i64 ldx)
{
    __shared__ double tile [256 * 17] ;
    const int tid = threadIdx.x ;
    const i64 k0 = blockIdx.x * (i64) 256, k = k0 + tid ;
    for (int e = tid ; e < 256 * SD_NP ; e += 256)
        if (k0 + (e >> 4) < n) tile [(e >> 4) * 17 + (e & 15)] = W [k0 * SD_NP + e] ;
    __syncthreads () ;
    if (k < n)
    {
        const i64 dst = perm ? perm [k] : k ;
        for (int r = 0 ; r < pw ; r++) X [dst + (i64) r * ldx] = tile [tid * 17 + r] ;
    }
}

// ---- whole supernodes (at most 256 columns, one workgroup each) ----------------------------------------------------
// the 16 x 16 diagonal block at column jb into LDS, identity-padded past the supernode's last column
__device__ __forceinline__ void sd_stage_diag (const double *L, int nsrow, int jb, int nb, double *Dl, int tid)
{
    const int i = tid & 15, j = tid >> 4 ;
    Dl [i * 17 + j] = (i < nb && j < nb && j <= i) ? L [jb + i + (i64) (jb + j) * nsrow] : (i == j ? 1.0 : 0.0) ;
}

// forward: x1 = L1 \ x1 by 16-column blocks (substitution on 16 right-hand sides at once, one lane each, then the
// rows below inside the supernode as tiles), W [Ls2] -= L2 x1 as tiles (siblings share ancestor rows: atomic)
__global__ void __launch_bounds__(256) k_sd_lsolve (const SolveTask *tasks, const FrontD *fr, const i64 *Ls,
    const double *Lx, double *W)
{
    __shared__ double x1 [256 * SD_NP] ;
    __shared__ double Dl [16 * 17] ;
    const SolveTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, tid = threadIdx.x ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    double *Wk = W + (i64) f.k1 * SD_NP ;
    for (int e = tid ; e < nscol * SD_NP ; e += 256) x1 [e] = Wk [e] ;
    __syncthreads () ;
    for (int jb = 0 ; jb < nscol ; jb += 16)
    {
        const int nb = nscol - jb < 16 ? nscol - jb : 16 ;
        sd_stage_diag (L, nsrow, jb, nb, Dl, tid) ;
        __syncthreads () ;
        if (tid < 16)
        {
            double v [16] ;
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) v [i] = (i < nb) ? x1 [(jb + i) * SD_NP + tid] : 0.0 ;
#pragma unroll
            for (int j = 0 ; j < 16 ; j++)
            {
                v [j] = v [j] / Dl [j * 17 + j] ;
#pragma unroll
                for (int i = j + 1 ; i < 16 ; i++) v [i] = __builtin_fma (-Dl [i * 17 + j], v [j], v [i]) ;
            }
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) if (i < nb) x1 [(jb + i) * SD_NP + tid] = v [i] ;
        }
        __syncthreads () ;
        for (int i0 = jb + 16 + 16 * wave ; i0 < nscol ; i0 += 64)
        {
            const d4 p = sd_mul_nx (L + (i64) jb * nsrow, nsrow, i0, nscol, nb, x1 + jb * SD_NP, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++)
            {
                const int i = i0 + lk + 4 * r ;
                if (i < nscol) x1 [i * SD_NP + lr] -= p [r] ;
            }
        }
        __syncthreads () ;
    }
    for (int e = tid ; e < nscol * SD_NP ; e += 256) Wk [e] = x1 [e] ;
    if (T.below)
        for (int i0 = nscol + 16 * wave ; i0 < nsrow ; i0 += 64)
        {
            const d4 p = sd_mul_nx (L, nsrow, i0, nsrow, nscol, x1, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++)
            {
                const int i = i0 + lk + 4 * r ;
                if (i < nsrow) atomicAdd (&W [rows [i] * SD_NP + lr], -p [r]) ;
            }
        }
}

// backward: x1 -= L2' W [Ls2] (the rows split over the four waves, their partial tiles summed in a fixed order: no
// atomics), then x1 = L1' \ x1 by 16-column blocks from the bottom
__global__ void __launch_bounds__(256) k_sd_ltsolve (const SolveTask *tasks, const FrontD *fr, const i64 *Ls,
    const double *Lx, double *W)
{
    __shared__ double x1 [256 * SD_NP] ;
    __shared__ double red [4][256] ;
    __shared__ double Dl [16 * 17] ;
    const SolveTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, tid = threadIdx.x ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    double *Wk = W + (i64) f.k1 * SD_NP ;
    for (int e = tid ; e < nscol * SD_NP ; e += 256) x1 [e] = Wk [e] ;
    __syncthreads () ;
    if (T.below && nsrow > nscol)
    {
        auto yg = [&] (int i, int c) { return W [rows [i] * SD_NP + c] ; } ;
        for (int j0 = 0 ; j0 < nscol ; j0 += 16)
        {
            const d4 p = sd_mul_ty (L, nsrow, j0, nscol, nscol + 16 * wave, nsrow, 64, yg, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++) red [wave][(lk + 4 * r) * SD_NP + lr] = p [r] ;
            __syncthreads () ;
            if (j0 + (tid >> 4) < nscol)
                x1 [j0 * SD_NP + tid] -= (red [0][tid] + red [1][tid]) + (red [2][tid] + red [3][tid]) ;
            __syncthreads () ;
        }
    }
    auto ys = [&] (int i, int c) { return x1 [i * SD_NP + c] ; } ;
    for (int jb = ((nscol - 1) / 16) * 16 ; jb >= 0 ; jb -= 16)
    {
        const int nb = nscol - jb < 16 ? nscol - jb : 16 ;
        sd_stage_diag (L, nsrow, jb, nb, Dl, tid) ;
        __syncthreads () ;
        if (tid < 16)
        {
            double v [16] ;
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) v [i] = (i < nb) ? x1 [(jb + i) * SD_NP + tid] : 0.0 ;
#pragma unroll
            for (int j = 15 ; j >= 0 ; j--)
            {
                v [j] = v [j] / Dl [j * 17 + j] ;
#pragma unroll
                for (int i = 0 ; i < j ; i++) v [i] = __builtin_fma (-Dl [j * 17 + i], v [j], v [i]) ;
            }
#pragma unroll
            for (int i = 0 ; i < 16 ; i++) if (i < nb) x1 [(jb + i) * SD_NP + tid] = v [i] ;
        }
        __syncthreads () ;
        // the columns before the block: x1 [0, jb) -= L [jb .. jb+nb, 0 .. jb)' x1 [jb .. jb+nb)
        for (int j0 = 16 * wave ; j0 < jb ; j0 += 64)
        {
            const d4 p = sd_mul_ty (L, nsrow, j0, jb, jb, jb + nb, 16, ys, sd_zero (), lr, lk) ;
#pragma unroll
            for (int r = 0 ; r < 4 ; r++) x1 [(j0 + lk + 4 * r) * SD_NP + lr] -= p [r] ;
        }
        __syncthreads () ;
    }
    for (int e = tid ; e < nscol * SD_NP ; e += 256) Wk [e] = x1 [e] ;
}

// ---- big supernodes: the walk in 256-column blocks of kernels.hip.h, 16 right-hand sides wide --------------------------
// forward, step 1 (one workgroup per task): x_b = inv (L_bb) x_b by 64-column sub-blocks, in place in W.  Wave =
// 16 rows of the sub-block: t = x_k - L [sub-block k, columns before it] x (solved), then x_k = W_k t with the
// explicit inverse, both as tiles.
__global__ void __launch_bounds__(256) k_sd_fwd_diag (const SolveBlk *tasks, const FrontD *fr, const double *Lx,
    const double *Winv, double *W)
{
    __shared__ double xs [SOLVE_SB * SD_NP] ;
    __shared__ double ts [64 * SD_NP] ;
    const SolveBlk T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nsrow = f.nsrow, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *Lbb = Lx + f.psx + jb + (i64) jb * nsrow ;
    double *Wk = W + (i64) (f.k1 + jb) * SD_NP ;
    for (int e = tid ; e < SOLVE_SB * SD_NP ; e += 256) xs [e] = (e < w * SD_NP) ? Wk [e] : 0.0 ;
    __syncthreads () ;
    for (int k = 0 ; k < nsub ; k++)
    {
        const int i0 = 64 * k + 16 * wave ;
        const d4 p = sd_mul_nx (Lbb, nsrow, i0, w, 64 * k, xs, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) ts [(16 * wave + lk + 4 * r) * SD_NP + lr] = xs [(i0 + lk + 4 * r) * SD_NP + lr] - p [r] ;
        __syncthreads () ;
        const d4 q = sd_mul_nx (Winv + (i64) (T.inv + k) * 8192, 64, 16 * wave, 64, 64, ts, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) xs [(i0 + lk + 4 * r) * SD_NP + lr] = q [r] ;
        __syncthreads () ;
    }
    for (int e = tid ; e < w * SD_NP ; e += 256) Wk [e] = xs [e] ;
}

// forward, step 2: W [rows below the block] -= L [rows, b] x_b ; workgroup = (256-row chunk) x (64-column
// sub-block), wave = 64 of the rows as four tiles that share the x_b operand
__global__ void __launch_bounds__(256) k_sd_fwd_apply (const SolveBlk *tasks, int ntasks, const FrontD *fr,
    const i64 *Ls, const double *Lx, double *W)
{
    __shared__ double xs [64 * SD_NP] ;
    const SolveBlk T = tasks [find_solve_task (tasks, ntasks, (int) blockIdx.x)] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const int wgl = (int) blockIdx.x - T.wg_start ;
    const int q = wgl % nsub, chunk = wgl / nsub ;
    const int c0 = 64 * q, cw = (w - c0 < 64) ? w - c0 : 64 ;
    const double *L = Lx + f.psx + (i64) (jb + c0) * nsrow ;
    const i64 *rows = Ls + f.psi ;
    const double *Wb = W + (i64) (k1 + jb + c0) * SD_NP ;
    for (int e = tid ; e < 64 * SD_NP ; e += 256) xs [e] = (e < cw * SD_NP) ? Wb [e] : 0.0 ;
    __syncthreads () ;
    const int rb = jb + w + chunk * 256 + 64 * wave ;
    if (rb >= nsrow) return ;
    d4 acc [4] = {sd_zero (), sd_zero (), sd_zero (), sd_zero ()} ;
    bool rok [4] ;
    const double *Li [4] ;
#pragma unroll
    for (int t = 0 ; t < 4 ; t++)
    {
        const int i = rb + 16 * t + lr ;
        rok [t] = i < nsrow ;
        Li [t] = L + (rok [t] ? i : rb) ;
    }
    for (int k0 = 0 ; k0 < cw ; k0 += 4)
    {
        const int k = k0 + lk ;
        const bool ok = k < cw ;
        const double b = ok ? xs [k * SD_NP + lr] : 0.0 ;
        double a [4] ;
#pragma unroll
        for (int t = 0 ; t < 4 ; t++) a [t] = (ok && rok [t]) ? Li [t][(i64) k * nsrow] : 0.0 ;
#pragma unroll
        for (int t = 0 ; t < 4 ; t++) acc [t] = __builtin_amdgcn_mfma_f64_16x16x4f64 (a [t], b, acc [t], 0, 0, 0) ;
    }
#pragma unroll
    for (int t = 0 ; t < 4 ; t++)
#pragma unroll
        for (int r = 0 ; r < 4 ; r++)
        {
            const int i = rb + 16 * t + lk + 4 * r ;
            // (several column sub-blocks, and siblings of the level, add into the same row)
            if (i < nsrow) atomicAdd (&W [(i < nscol ? (i64) k1 + i : rows [i]) * SD_NP + lr], -acc [t][r]) ;
        }
}

// backward, step 1: acc (task) += L [rows, b]' W [rows] ; workgroup = (256-row chunk) x (64-column sub-block);
// the gathered rows are staged in LDS once, wave = 16 of the columns, one atomic add per column, right-hand side
// and workgroup.  acc: [slot][256][16].
__global__ void __launch_bounds__(256) k_sd_bwd_apply (const SolveBlk *tasks, int ntasks, const FrontD *fr,
    const i64 *Ls, const double *Lx, const double *W, double *accbuf)
{
    __shared__ double ys [256 * SD_NP] ;
    const SolveBlk T = tasks [find_solve_task (tasks, ntasks, (int) blockIdx.x)] ;
    const FrontD &f = fr [T.front] ;
    const int nscol = f.nscol, nsrow = f.nsrow, k1 = f.k1, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const int wgl = (int) blockIdx.x - T.wg_start ;
    const int qsub = wgl % nsub, chunk = wgl / nsub ;
    const double *L = Lx + f.psx ;
    const i64 *rows = Ls + f.psi ;
    double *acc = accbuf + (i64) T.slot * SOLVE_SB * SD_NP ;
    const int r0 = jb + w + chunk * 256 ;
    const int nr = nsrow - r0 < 256 ? nsrow - r0 : 256 ;
    if (nr <= 0) return ;
    for (int e = tid ; e < 256 * SD_NP ; e += 256)
    {
        const int i = r0 + (e >> 4) ;
        ys [e] = (i < nsrow) ? W [(i < nscol ? (i64) k1 + i : rows [i]) * SD_NP + (e & 15)] : 0.0 ;
    }
    __syncthreads () ;
    const int c0 = 64 * qsub + 16 * wave ;
    if (c0 >= w) return ;
    auto yl = [&] (int i, int c) { return ys [(i - r0) * SD_NP + c] ; } ;
    const d4 p = sd_mul_ty (L, nsrow, jb + c0, jb + w, r0, r0 + nr, 16, yl, sd_zero (), lr, lk) ;
#pragma unroll
    for (int r = 0 ; r < 4 ; r++)
    {
        const int c = c0 + lk + 4 * r ;
        if (c < w) atomicAdd (&acc [c * SD_NP + lr], p [r]) ;
    }
}

// backward, step 2 (one workgroup per task): x_b = inv (L_bb)' (x_b - acc) by sub-blocks from the bottom; the
// accumulator is cleared for the next step
__global__ void __launch_bounds__(256) k_sd_bwd_diag (const SolveBlk *tasks, const FrontD *fr, const double *Lx,
    const double *Winv, double *W, double *accbuf)
{
    __shared__ double xs [SOLVE_SB * SD_NP] ;
    __shared__ double ts [64 * SD_NP] ;
    const SolveBlk T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nsrow = f.nsrow, tid = threadIdx.x ;
    const int jb = T.jb, w = T.w, nsub = (w + 63) >> 6 ;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    const double *Lbb = Lx + f.psx + jb + (i64) jb * nsrow ;
    double *acc = accbuf + (i64) T.slot * SOLVE_SB * SD_NP ;
    double *Wk = W + (i64) (f.k1 + jb) * SD_NP ;
    for (int e = tid ; e < SOLVE_SB * SD_NP ; e += 256)
    {
        xs [e] = (e < w * SD_NP) ? Wk [e] - acc [e] : 0.0 ;
        acc [e] = 0.0 ;
    }
    __syncthreads () ;
    auto yl = [&] (int i, int c) { return xs [i * SD_NP + c] ; } ;
    for (int k = nsub - 1 ; k >= 0 ; k--)
    {
        const int c0 = 64 * k + 16 * wave ;
        // t = x_k - sum over the solved rows below sub-block k (inside the block) of L (row, column)' x (row)
        const d4 p = sd_mul_ty (Lbb, nsrow, c0, w, 64 * (k + 1), w, 16, yl, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) ts [(16 * wave + lk + 4 * r) * SD_NP + lr] = xs [(c0 + lk + 4 * r) * SD_NP + lr] - p [r] ;
        __syncthreads () ;
        const d4 q = sd_mul_nx (Winv + (i64) (T.inv + k) * 8192 + 4096, 64, 16 * wave, 64, 64, ts, sd_zero (), lr, lk) ;
#pragma unroll
        for (int r = 0 ; r < 4 ; r++) xs [(c0 + lk + 4 * r) * SD_NP + lr] = q [r] ;
        __syncthreads () ;
    }
    for (int e = tid ; e < w * SD_NP ; e += 256) Wk [e] = xs [e] ;
}

} // namespace sship
