// schur_kernels.hip.h -- device code of the Schur complement on the resident factor (schur.hip).  With t = n - m the first
// trailing column and L22 = L [t:, t:], Sc = L22 L22'.  L22 lives in the panels of the supernodes s0 = supermap [t] ..
// nsuper - 1: of each its columns max (k1, t) .. k1 + nscol - 1 and, of those, the rows from the first such column down
// (the boundary may fall inside s0; every row below a panel's own columns is >= t by construction).  The strictly upper
// triangle of a diagonal block counts as zero whatever Lx holds there: an entry at local row r of local column c is read
// only if r >= c.
//
// k_schur_tile: one workgroup owns one 64 x 64 tile (I, J), I >= J, of the lower triangle of Sc and walks the trailing
// supernodes in ascending order.  In a panel, every lane looks up the five rows it feeds -- one of the tile's row range
// for the A operand of its wave's 16-row strip, four of its column range for the B operands -- by si_locate's search in
// the sorted row list, once per supernode; a row the list does not hold feeds zeros.  The operands then stream from the
// panel straight into v_mfma_f64_16x16x4 (the dense position of a row within the tile IS its lane), four columns of the
// panel per instruction; the sixteen accumulators of a lane stay in registers over all supernodes.  No LDS, no scratch,
// no atomics: one owner, one summation order (supernodes ascending, columns ascending), and the upper triangle of Sc is
// written from the same registers as the lower one.
#pragma once
#include "sweep_device.hip.h"

namespace sship {

// local row of global row r in the panel of t, -1: not in its row list (or r outside 0 .. n-1 of the tile's ragged edge)
__device__ __forceinline__ int sc_local_row (const FrontD &t, const i64 *Ls, i64 r)
{
    if (r < (i64) t.k1) return -1 ;
    if (r < (i64) t.k1 + t.nscol) return (int) (r - t.k1) ;
    const i64 *rows = Ls + t.psi ;
    int lo = t.nscol, hi = t.nsrow ;
    while (lo < hi) { const int mid = (lo + hi) >> 1 ; if (rows [mid] < r) lo = mid + 1 ; else hi = mid ; }
    return (lo < t.nsrow && rows [lo] == r) ? lo : -1 ;
}

// first local row of the panel of t whose global row is >= r
__device__ __forceinline__ int sc_lower_bound (const FrontD &t, const i64 *Ls, i64 r)
{
    const i64 *rows = Ls + t.psi ;
    int lo = 0, hi = t.nsrow ;
    while (lo < hi) { const int mid = (lo + hi) >> 1 ; if (rows [mid] < r) lo = mid + 1 ; else hi = mid ; }
    return lo ;
}

// tile b of the lower triangle, column by column: (I, J) with I >= J, nt tiles a side
__device__ __forceinline__ void sc_tile_of (int b, int nt, int &I, int &J)
{
    int j = 0, left = b ;
    while (left >= nt - j) { left -= nt - j ; j++ ; }
    J = j ; I = j + left ;
}

__global__ void __launch_bounds__(256) k_schur_tile (i64 n, i64 m, int nt, int s0, int nsuper, const FrontD *fr, const i64 *Ls,
    const double *Lx, double *S, i64 lds)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4 ;
    int I, J ;
    sc_tile_of (blockIdx.x, nt, I, J) ;
    const i64 t0 = n - m ;
    const i64 rI = t0 + 64 * (i64) I, rJ = t0 + 64 * (i64) J ;          // first global row of the tile's rows / columns
    const i64 gA = rI + 16 * wave + lr ;                                // the row this lane feeds as A
    si_d4 acc [4] ;
#pragma unroll
    for (int t = 0 ; t < 4 ; t++) acc [t] = (si_d4) {0.0, 0.0, 0.0, 0.0} ;
    for (int s = s0 ; s < nsuper ; s++)
    {
        const FrontD &f = fr [s] ;
        // a panel whose columns start after the tile's last column row holds none of the tile's column rows (its rows
        // are >= k1); one that has no row in either range contributes nothing (uniform over the workgroup)
        if ((i64) f.k1 >= rJ + 64) break ;
        const int c0 = (i64) f.k1 < t0 ? (int) (t0 - f.k1) : 0 ;        // first contributing column
        const int jlo = sc_lower_bound (f, Ls, rJ), jhi = sc_lower_bound (f, Ls, rJ + 64) ;
        if (jlo == jhi) continue ;
        const int ilo = sc_lower_bound (f, Ls, rI), ihi = sc_lower_bound (f, Ls, rI + 64) ;
        if (ilo == ihi) continue ;
        const int ia = gA < n ? sc_local_row (f, Ls, gA) : -1 ;
        int ib [4] ;
#pragma unroll
        for (int t = 0 ; t < 4 ; t++)
        {
            const i64 g = rJ + 16 * t + lr ;
            ib [t] = g < n ? sc_local_row (f, Ls, g) : -1 ;
        }
        const i64 ld = f.nsrow ;
        const double *P = Lx + f.psx ;
        // columns past the first row of the column range hold zeros in every row of it (masked upper triangle, or rows
        // above the column): the contraction ends at the last column any B row can reach
        const int cend = min ((int) f.nscol, jhi) ;
        for (int kc = c0 ; kc < cend ; kc += 4)
        {
            const int k = kc + lk ;
            const bool kin = k < cend ;
            const double *Pk = P + (i64) (kin ? k : c0) * ld ;
            const double a = (kin && ia >= k) ? Pk [ia] : 0.0 ;
            double b [4] ;
#pragma unroll
            for (int t = 0 ; t < 4 ; t++) b [t] = (kin && ib [t] >= k) ? Pk [ib [t]] : 0.0 ;
#pragma unroll
            for (int t = 0 ; t < 4 ; t++) acc [t] = __builtin_amdgcn_mfma_f64_16x16x4f64 (a, b [t], acc [t], 0, 0, 0) ;
        }
    }
    // acc [t][r] of lane (lr, lk) is C (row 16 wave + lk + 4 r, column 16 t + lr) of the tile
#pragma unroll
    for (int t = 0 ; t < 4 ; t++)
#pragma unroll
        for (int r = 0 ; r < 4 ; r++)
        {
            const i64 i = 64 * (i64) I + 16 * wave + lk + 4 * r, j = 64 * (i64) J + 16 * t + lr ;
            if (i >= m || j >= m || i < j) continue ;
            const double v = acc [t][r] ;
            S [i + j * lds] = v ;
            S [j + i * lds] = v ;
        }
}

// dense L22 into F (m x m, ldf): one workgroup per trailing column.  The column is cleared (+0.0: the strict upper
// triangle and the entries outside the pattern), then the panel's rows from the diagonal down are scattered.
__global__ void __launch_bounds__(256) k_schur_factor (i64 n, i64 m, const i32 *supermap, const FrontD *fr, const i64 *Ls,
    const double *Lx, double *F, i64 ldf)
{
    const i64 j = blockIdx.x, t0 = n - m, c = t0 + j ;
    const FrontD &f = fr [supermap [c]] ;
    const int cl = (int) (c - f.k1) ;
    double *Fc = F + j * ldf ;
    for (i64 i = threadIdx.x ; i < m ; i += 256) Fc [i] = 0.0 ;
    __syncthreads () ;
    const i64 *rows = Ls + f.psi ;
    const double *Pc = Lx + f.psx + (i64) cl * f.nsrow ;
    for (int r = cl + threadIdx.x ; r < f.nsrow ; r += 256) Fc [rows [r] - t0] = Pc [r] ;
}

// Out (j, q) = sum_{i >= j} L22 (i, j) V (i, q): one workgroup per trailing column j owns row j of Out for every
// right-hand side; the 256 partial sums (rows strided by 256, ascending) are added by a fixed tree: the same bits twice.
__global__ void __launch_bounds__(256) k_schur_mult_t (i64 n, i64 m, const i32 *supermap, const FrontD *fr, const i64 *Ls,
    const double *Lx, const double *V, i64 ldv, double *Out, i64 ldo, i64 nrhs)
{
    __shared__ double part [256] ;
    const int tid = threadIdx.x ;
    const i64 j = blockIdx.x, t0 = n - m, c = t0 + j ;
    const FrontD &f = fr [supermap [c]] ;
    const int cl = (int) (c - f.k1) ;
    const i64 *rows = Ls + f.psi ;
    const double *Pc = Lx + f.psx + (i64) cl * f.nsrow ;
    for (i64 q = 0 ; q < nrhs ; q++)
    {
        const double *Vq = V + q * ldv ;
        double s = 0 ;
        for (int r = cl + tid ; r < f.nsrow ; r += 256) s += Pc [r] * Vq [rows [r] - t0] ;
        part [tid] = s ;
        __syncthreads () ;
        for (int w = 128 ; w > 0 ; w >>= 1)
        {
            if (tid < w) part [tid] += part [tid + w] ;
            __syncthreads () ;
        }
        if (tid == 0) Out [j + q * ldo] = part [0] ;
        __syncthreads () ;
    }
}

__global__ void __launch_bounds__(256) k_schur_clear (i64 m, i64 nrhs, double *Out, i64 ldo)
{
    const i64 e = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (e < m * nrhs) Out [e % m + (e / m) * ldo] = 0.0 ;
}

// Out (i, q) += L22 (i, j) V (j, q) over the rows i of column j: one workgroup per trailing column, added atomically
// into the cleared Out, as the forward solves this product is composed with add into their right-hand sides.
__global__ void __launch_bounds__(256) k_schur_mult_n (i64 n, i64 m, const i32 *supermap, const FrontD *fr, const i64 *Ls,
    const double *Lx, const double *V, i64 ldv, double *Out, i64 ldo, i64 nrhs)
{
    const i64 j = blockIdx.x, t0 = n - m, c = t0 + j ;
    const FrontD &f = fr [supermap [c]] ;
    const int cl = (int) (c - f.k1) ;
    const i64 *rows = Ls + f.psi ;
    const double *Pc = Lx + f.psx + (i64) cl * f.nsrow ;
    for (i64 q = 0 ; q < nrhs ; q++)
    {
        const double v = V [j + q * ldv] ;
        double *Oq = Out + q * ldo ;
        for (int r = cl + threadIdx.x ; r < f.nsrow ; r += 256) atomicAdd (Oq + (rows [r] - t0), Pc [r] * v) ;
    }
}

} // namespace sship
