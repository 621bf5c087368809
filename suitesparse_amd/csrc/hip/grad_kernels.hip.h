// grad_kernels.hip.h -- device code of grad.hip: the gradient of a scalar with respect to the values of A, sampled on
// the pattern of the resident S (cholmod_hip_values_grad_device), the chain rule from there through a product map to the
// values of an unsymmetric A (k_product_grad: cholmod_hip_product_*_grad_device), and log det of the resident factor
// (cholmod_hip_logdet_device).
//
// The gradient is a sampled product: for entry p = (i, j) of S that the factorization reads (the rule of
// k_si_gather_values: on or below the diagonal, row < n, the last of equal neighbours)
//     G [src [p]] = alpha sum_r ( U [i, r] V [j, r] + [i != j] U [j, r] V [i, r] )
// A pure gather with no matrix structure per entry: nothing for the matrix cores, bound by latency and bandwidth.  Work
// is divided by ENTRIES of S, never by columns (arrow300 has columns of hundreds of entries next to columns of one); the
// column of an entry comes from an i32 column-of-entry array, built once per upload on the device by a binary search in
// Sp per entry (k_gr_column_index): 4 bytes of HBM per entry of S, read coalesced, where the search in every call cost
// log2 (n) dependent reads per entry (measured at Poisson 100^3, nrhs = 1: 0.45 ms per call with the search inside).
// Every entry of G has one owner and one summation order, no atomics: the same inputs give the same bits.
#pragma once
#include "descriptors.hip.h"

namespace sship {

#define GR_NP 16            /* right-hand sides per panel: the solve's (SD_NP) */

__global__ void __launch_bounds__(256) k_gr_zero_fill (i64 n, double *out)
{
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (k < n) out [k] = 0.0 ;
}

// the column of entry p of the packed S (0 <= p < Sp [n], n > 0): the last j with Sp [j] <= p (an empty column never wins:
// its successor starts at the same p)
__device__ __forceinline__ i64 gr_column_of (const i64 *Sp, i64 n, i64 p)
{
    i64 lo = 0, hi = n - 1 ;
    while (lo < hi)
    {
        const i64 mid = (lo + hi + 1) >> 1 ;
        if (Sp [mid] <= p) lo = mid ; else hi = mid - 1 ;
    }
    return lo ;
}

// colof [p] = the column of entry p, once per uploaded pattern
__global__ void __launch_bounds__(256) k_gr_column_index (i64 n, i64 nz, const i64 *Sp, i32 *colof)
{
    const i64 p = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (p < nz) colof [p] = (i32) gr_column_of (Sp, n, p) ;
}

// is entry p = (i, j) one the factorization reads?
__device__ __forceinline__ bool gr_reads (const i64 *Sp, const i64 *Si, i64 n, i64 p, i64 i, i64 j)
{
    return !(i < j || i >= n || (p + 1 < Sp [j + 1] && Si [p + 1] == i)) ;
}

// Fewer than SD_BLOCK_MIN_NRHS right-hand sides: U and V read in place through Perm, one thread per entry of S, the
// right-hand sides in index order.
__global__ void __launch_bounds__(256) k_gr_columns (i64 n, i64 nz, const i64 *Sp, const i64 *Si, const i32 *colof, const i64 *src, const i64 *perm,
    const double *U, i64 ldu, const double *V, i64 ldv, int nrhs, double alpha, double *G)
{
    const i64 p = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (p >= nz) return ;
    const i64 j = colof [p], i = Si [p] ;
    if (!gr_reads (Sp, Si, n, p, i, j)) return ;
    const i64 ri = perm ? perm [i] : i, rj = perm ? perm [j] : j ;
    double s = 0.0 ;
    for (int r = 0 ; r < nrhs ; r++)
    {
        s += U [ri + r * ldu] * V [rj + r * ldv] ;
        if (i != j) s += U [rj + r * ldu] * V [ri + r * ldv] ;
    }
    G [src [p]] = alpha * s ;
}

// One panel of 16 right-hand sides, Wu / Wv [n][16] packed through Perm by k_sd_pack (a row = one 128-byte line, the
// columns past the panel's width zero).  A group of 16 lanes owns 16 consecutive entries of S: lane l loads the column
// of entry l and finds whether it is read, then the group walks its entries -- four coalesced row
// loads, the lane's two products, a fixed xor tree over the 16 lanes -- and lane e keeps the sum of entry e.  An entry
// that is not read loads row 0 and contributes nothing.  At the end every lane owns one entry: one 8-byte store through
// src [].  first: G is written, else added to (the same owner, in panel order); last: the sum is scaled by alpha.
__global__ void __launch_bounds__(256) k_gr_panel (i64 n, i64 nz, const i64 *Sp, const i64 *Si, const i32 *colof, const i64 *src,
    const double *Wu, const double *Wv, int first, int last, double alpha, double *G)
{
    const int l = threadIdx.x & 15 ;
    const i64 p = (blockIdx.x * (i64) 16 + (threadIdx.x >> 4)) * 16 + l ;
    int i = 0, j = 0, rd = 0 ;                   // (n fits 32 bits: the engine's maps)
    if (p < nz)
    {
        const i64 jj = colof [p], ii = Si [p] ;
        if (gr_reads (Sp, Si, n, p, ii, jj)) { i = (int) ii ; j = (int) jj ; rd = 1 ; }
    }
    double mine = 0.0 ;
#pragma unroll 4
    for (int e = 0 ; e < 16 ; e++)
    {
        const int ie = __shfl (i, e, 16), je = __shfl (j, e, 16), re = __shfl (rd, e, 16) ;
        const double ui = Wu [(i64) ie * GR_NP + l], vj = Wv [(i64) je * GR_NP + l] ;
        const double uj = Wu [(i64) je * GR_NP + l], vi = Wv [(i64) ie * GR_NP + l] ;
        double t = ui * vj ;
        if (ie != je) t += uj * vi ;
        if (!re) t = 0.0 ;
        for (int o = 8 ; o > 0 ; o >>= 1) t += __shfl_xor (t, o, 16) ;
        if (l == e) mine = t ;
    }
    if (rd)
    {
        const i64 k = src [p] ;
        const double s = first ? mine : G [k] + mine ;
        G [k] = last ? alpha * s : s ;
    }
}

// ---- the chain rule through a product map: the transpose of k_product_values (values_kernels.hip.h) ------------------------
//
// vals [c] = sum over the pairs p of list c of a [ia [p]] a [ib [p]], and Gv [c] = d loss / d vals [c]; then
//     g [q] = sum_{p : ia [p] = q} Gv [c (p)] a [ib [p]]  +  sum_{p : ib [p] = q} Gv [c (p)] a [ia [p]]
// (a pair with ia [p] == ib [p] == q is in both sums: the 2 a_q of a square).  The transposed map stores, per value q, these
// half-pairs as (tc [h], tpart [h]), tp [q] <= h < tp [q + 1], in ascending p, the ia half of a pair before its ib half:
// 16 bytes per pair, as the forward map.  The values come sorted by list length into the classes of the forward kernel
// (order [g]: the value group g of this launch owns; PM_LEN1, PM_LEN16) and a group of G lanes owns one value: lane l adds
// the half-pairs l, l + G, ... in that order (fused multiply-add), the G partial sums meet in a butterfly of fixed shape and
// lane 0 stores -- one owner per g [q], the order a function of the map alone, no floating-point atomic: the same inputs give
// the same bits.  A value in no pair has an empty list and gets +0.0.  Two dependent gathers per half-pair (8-byte Gv and
// a, scattered) behind two coalesced 4-byte index loads: latency and bandwidth, nothing for the matrix cores.  Every index
// was checked on the host when the forward map was set: nothing outside Gv [0 .. nc) and a [0 .. navalues) is read.
template <int G>
__global__ void __launch_bounds__(256) k_product_grad (i64 ngroups, const i32 *order, const i64 *tp, const i32 *tc, const i32 *tpart,
    const double *Gv, const double *a, double *g)
{
    const i64 t = blockIdx.x * (i64) 256 + threadIdx.x ;
    const i64 grp = t / G ;
    const int l = (int) (t % G) ;
    // (a whole group leaves together: the shuffles below see the lanes of live groups only)
    if (grp >= ngroups) return ;
    const i64 q = order [grp] ;
    const i64 h1 = tp [q + 1] ;
    double acc = 0.0 ;
#pragma unroll 2
    for (i64 h = tp [q] + l ; h < h1 ; h += G) acc = __builtin_fma (Gv [tc [h]], a [tpart [h]], acc) ;
#pragma unroll
    for (int w = G / 2 ; w > 0 ; w >>= 1) acc += __shfl_xor (acc, w, 64) ;
    if (l == 0) g [q] = acc ;
}

// ---- log det of the resident factor: 2 sum_j log L_jj, two fixed-order stages, no atomics ---------------------------------

// the 256 values of a workgroup added in a fixed tree; the sum in red [0]
__device__ __forceinline__ void gr_block_sum (double *red, double v)
{
    red [threadIdx.x] = v ;
    __syncthreads () ;
    for (int o = 128 ; o > 0 ; o >>= 1)
    {
        if ((int) threadIdx.x < o) red [threadIdx.x] += red [threadIdx.x + o] ;
        __syncthreads () ;
    }
}

// part [b] = sum of log L_jj over the 256 columns of workgroup b, the diagonal addressed through the supernode map as
// k_diag_minmax does
__global__ void __launch_bounds__(256) k_gr_logdet_partial (i64 n, const i32 *supermap, const FrontD *fr, const double *Lx, double *part)
{
    __shared__ double red [256] ;
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    double v = 0.0 ;
    if (k < n)
    {
        const FrontD &f = fr [supermap [k]] ;
        const i64 jj = k - f.k1 ;
        v = log (Lx [f.psx + jj + jj * (i64) f.nsrow]) ;
    }
    gr_block_sum (red, v) ;
    if (threadIdx.x == 0) part [blockIdx.x] = red [0] ;
}

// out [0] = 2 sum of the partials: one workgroup, thread t adds the partials t, t + 256, ... in index order, then the tree
__global__ void __launch_bounds__(256) k_gr_logdet_final (i64 nparts, const double *part, double *out)
{
    __shared__ double red [256] ;
    double v = 0.0 ;
    for (i64 q = threadIdx.x ; q < nparts ; q += 256) v += part [q] ;
    gr_block_sum (red, v) ;
    if (threadIdx.x == 0) out [0] = 2.0 * red [0] ;
}

} // namespace sship
