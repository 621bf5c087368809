// residual_kernels.hip.h -- gfx950 kernels of the device-resident residual R = B - (A + beta I) X (residual.hip launches
// them).  A is symmetric and only S = tril (P A P') is resident, by columns: row j of the product is
//     sum over the entries (i, j) of column j of S, i >= j, of S (i, j) X (i)         -- a walk down the column
//   + sum over the entries (j, k) of row j of S, k < j,   of S (j, k) X (k)           -- the transposed index T
// T (Tp [n + 1], Tj, Tq) lists, for every row, its entries left of the diagonal by ascending column, each with its
// POSITION in Sx: the values-only uploads rewrite Sx in place and T stays good.  Both parts skip what the assembly skips
// (k_assemble: entries above the diagonal, all but the last of equal neighbours in a column).
// Every entry of R has one owner that adds its terms in a fixed order -- first the column, top to bottom, then the row,
// left to right -- and there is no floating-point atomic: the same inputs give the same bits.
#pragma once
#include "device_util.hip.h"

namespace sship {

#define RS_NP 16        /* right-hand sides per panel: SD_NP of the solves */

// Panel form: X, B, R are [n][16], right-hand side fastest, so row k is one 128-byte line.  A 16-lane group owns a
// row (lane = right-hand side), a wave four consecutive rows, a workgroup sixteen: every gathered X (i) is one
// coalesced line per group, the index and the value are one broadcast load per group, and no cross-lane reduction is
// needed.  Rows of a wave have about the same length on the stencil matrices (7 on Poisson, some hundreds on the box
// stencils), so the four groups of a wave stay together; the loads of a row are independent of each other (the
// predicate is folded into the operands, not into control flow) and the unrolled loop keeps four in flight.
// R may be B.
__global__ void __launch_bounds__(256) k_rs_panel (i64 n, const i64 *Sp, const i64 *Snz, const i64 *Si, const double *Sx,
    const i64 *Tp, const i32 *Tj, const i64 *Tq, double beta, const double *X, const double *B, double *R)
{
    const int lr = threadIdx.x & 15 ;
    const i64 j = blockIdx.x * (i64) 16 + (threadIdx.x >> 4) ;
    if (j >= n) return ;
    double acc = 0.0 ;
    const i64 p0 = Sp [j], pend = Snz ? p0 + Snz [j] : Sp [j + 1] ;
#pragma unroll 4
    for (i64 p = p0 ; p < pend ; p++)
    {
        const i64 i = Si [p] ;
        const bool ok = i >= j && !(p + 1 < pend && Si [p + 1] == i) ;
        const double s = ok ? Sx [p] : 0.0 ;
        acc = __builtin_fma (s, X [(ok ? i : j) * RS_NP + lr], acc) ;
    }
    const i64 q1 = Tp [j + 1] ;
#pragma unroll 4
    for (i64 q = Tp [j] ; q < q1 ; q++) acc = __builtin_fma (Sx [Tq [q]], X [(i64) Tj [q] * RS_NP + lr], acc) ;
    R [j * RS_NP + lr] = (B [j * RS_NP + lr] - beta * X [j * RS_NP + lr]) - acc ;
}

// Column form (fewer than 8 right-hand sides): X, B, R are [nrhs][ld]; thread = row, blockIdx.y = right-hand side.
// The same terms in the same order.  R may be B.
__global__ void __launch_bounds__(256) k_rs_columns (i64 n, const i64 *Sp, const i64 *Snz, const i64 *Si, const double *Sx,
    const i64 *Tp, const i32 *Tj, const i64 *Tq, double beta, const double *X, i64 ldx, const double *B, i64 ldb,
    double *R, i64 ldr)
{
    const i64 j = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (j >= n) return ;
    const double *x = X + blockIdx.y * ldx ;
    double acc = 0.0 ;
    const i64 p0 = Sp [j], pend = Snz ? p0 + Snz [j] : Sp [j + 1] ;
#pragma unroll 4
    for (i64 p = p0 ; p < pend ; p++)
    {
        const i64 i = Si [p] ;
        const bool ok = i >= j && !(p + 1 < pend && Si [p + 1] == i) ;
        const double s = ok ? Sx [p] : 0.0 ;
        acc = __builtin_fma (s, x [ok ? i : j], acc) ;
    }
    const i64 q1 = Tp [j + 1] ;
#pragma unroll 4
    for (i64 q = Tp [j] ; q < q1 ; q++) acc = __builtin_fma (Sx [Tq [q]], x [Tj [q]], acc) ;
    R [blockIdx.y * ldr + j] = (B [blockIdx.y * ldb + j] - beta * x [j]) - acc ;
}

// x += w
__global__ void __launch_bounds__(256) k_rs_add (i64 count, double *x, const double *w)
{
    const i64 e = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (e < count) x [e] += w [e] ;
}

// ---- column max-norms: out [c] = max_i |R (i, c)| ---------------------------------------------------------------------
// |v| as a bit pattern orders like the number (non-negative doubles; a NaN sorts above infinity and so survives):
// a workgroup reduces its rows, then one integer atomicMax per column -- exact, and independent of the order.
// out is zero before the first launch.
#define RS_NORM_ROWS 1024       /* rows per workgroup of the norm kernels */

__device__ __forceinline__ unsigned long long rs_abs_bits (double v) { return (unsigned long long) __double_as_longlong (fabs (v)) ; }

// R [n][16]; nc columns (<= 16) are reported
__global__ void __launch_bounds__(256) k_rs_norm_panel (i64 n, const double *R, int nc, unsigned long long *out)
{
    __shared__ unsigned long long red [256] ;
    const int tid = threadIdx.x, c = tid & 15 ;
    const i64 j0 = blockIdx.x * (i64) RS_NORM_ROWS, j1 = (j0 + RS_NORM_ROWS < n) ? j0 + RS_NORM_ROWS : n ;
    unsigned long long m = 0 ;
    for (i64 j = j0 + (tid >> 4) ; j < j1 ; j += 16)
    {
        const unsigned long long v = rs_abs_bits (R [j * RS_NP + c]) ;
        m = v > m ? v : m ;
    }
    red [tid] = m ;
    __syncthreads () ;
    if (tid < 16)
    {
        for (int g = 1 ; g < 16 ; g++) { const unsigned long long v = red [16 * g + tid] ; m = v > m ? v : m ; }
        if (tid < nc) atomicMax (&out [tid], m) ;
    }
}

// R [nrhs][ld]; blockIdx.y = column
__global__ void __launch_bounds__(256) k_rs_norm_columns (i64 n, const double *R, i64 ld, unsigned long long *out)
{
    __shared__ unsigned long long red [256] ;
    const int tid = threadIdx.x ;
    const double *r = R + blockIdx.y * ld ;
    const i64 j0 = blockIdx.x * (i64) RS_NORM_ROWS, j1 = (j0 + RS_NORM_ROWS < n) ? j0 + RS_NORM_ROWS : n ;
    unsigned long long m = 0 ;
    for (i64 j = j0 + tid ; j < j1 ; j += 256)
    {
        const unsigned long long v = rs_abs_bits (r [j]) ;
        m = v > m ? v : m ;
    }
    red [tid] = m ;
    __syncthreads () ;
    for (int s = 128 ; s > 0 ; s >>= 1)
    {
        if (tid < s) { const unsigned long long v = red [tid + s] ; if (v > red [tid]) red [tid] = v ; }
        __syncthreads () ;
    }
    if (tid == 0) atomicMax (&out [blockIdx.y], red [0]) ;
}

} // namespace sship
