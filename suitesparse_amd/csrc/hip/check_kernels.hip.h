// check_kernels.hip.h -- device kernels of the read-only passes over a finished factor (checks.hip): its extreme diagonal
// entries, its size-independent invariants, and its even columns (the complex factor of an embedded complex matrix).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "descriptors.hip.h"
#include "device_util.hip.h"

namespace sship {

// ---- extreme diagonal entries of L (cholmod_l_rcond on a device-resident factor) ---------------------
// out [0] = min L_jj, out [1] = max L_jj (as ordered bit patterns of NON-NEGATIVE doubles: the caller seeds them with
// +inf / 0), out [2] += number of NaN or negative diagonal entries; a diagonal entry -0.0 counts as +0.0 (a minimum of 0,
// not a negative entry).  One thread per column; CX: a complex factor in its own
// storage, the diagonal of the complex L is the (real) entry (2j, 2j) of the twin, kept in the even column 2j.
template <bool CX>
__global__ void __launch_bounds__(256) k_diag_minmax (i64 n, const i32 *supermap, const FrontD *fr, const double *Lx, unsigned long long *out)
{
    const i64 k = blockIdx.x * (i64) 256 + threadIdx.x ;
    double v = 0 ;
    bool have = false, bad = false ;
    if (k < n && !(CX && (k & 1)))
    {
        const FrontD f = fr [supermap [k]] ;
        const int jj = (int) (k - f.k1) ;
        v = Lx [f.psx + jj + colx<CX> (jj, f.nsrow)] ;
        have = true ;
        if (!(v >= 0.0)) { bad = true ; have = false ; }        // (NaN or negative: counted, kept out of the extremes)
        // a zero of either sign is the minimum +0.0: the bit pattern of -0.0 is above that of +inf as an unsigned integer,
        // so it would win the wave's comparisons and then lose the atomicMin, and the wave's minimum with it
        // (-0.0 + 0.0 = +0.0 in round-to-nearest, every other value unchanged; needs signed zeros, i.e. no fast-math build)
        v = v + 0.0 ;
    }
    double lo = have ? v : __builtin_inf (), hi = have ? v : 0.0 ;
    for (int o = 32 ; o > 0 ; o >>= 1)
    {
        const double l2 = __shfl_xor (lo, o), h2 = __shfl_xor (hi, o) ;
        lo = l2 < lo ? l2 : lo ; hi = h2 > hi ? h2 : hi ;
    }
    const unsigned long long nbad = __popcll (__ballot (bad)) ;
    if ((threadIdx.x & 63) == 0)
    {
        atomicMin (out, (unsigned long long) __double_as_longlong (lo)) ;
        atomicMax (out + 1, (unsigned long long) __double_as_longlong (hi)) ;
        if (nbad) atomicAdd (out + 2, nbad) ;
    }
}

// ---- even columns of the factor (complex input through the real embedding) ---------
// The engine factors the 2n x 2n embedding of a complex matrix (host/complex.c); the
// interleaved complex column j of a supernode is the even column 2j of the real one.
// out (packed: supernode s at px [s] / 2, i.e. 2 * nsrow_c * nscol_c doubles) receives
// them, the imaginary part of the diagonal as the exact zero zpotrf leaves.
__global__ void __launch_bounds__(256) k_even_columns (const CheckTask *tasks, const FrontD *fr,
    const double *Lx, double *out)
{
    const CheckTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    const int nsrow = f.nsrow, nscol = f.nscol ;
    const double *L = Lx + f.psx ;
    double *O = out + f.psx / 2 ;
    const int c1 = T.c0 + CHK_COLS < nscol ? T.c0 + CHK_COLS : nscol ;
    for (int c = T.c0 + (T.c0 & 1) ; c < c1 ; c += 2)
        for (int i = threadIdx.x ; i < nsrow ; i += 256)
            O [(i64) (c >> 1) * nsrow + i] = (i == c + 1) ? 0.0 : L [(i64) c * nsrow + i] ;
}

// ---- size-independent invariants of a device-resident factor ----------------
// One pass over Lx (parity checks at sizes the CPU oracle cannot reach):
//   out[0] += sum_j log L(j,j)          (= logdet(A)/2, analytic for Poisson grids)
//   out[1] += entries != 0 in the dead strictly-upper triangles of the diagonal
//             blocks (the reference never writes them);
//             a NaN counts, -0.0 does not
//   out[2] += non-finite entries of the lower trapezoids
//   out[3] += sum of squares of the finite entries of the lower trapezoids (||L||_F^2)
//   out[4] += diagonal entries that are not > 0 (zero of either sign, negative, NaN)
// A workgroup owns CHK_COLS columns of one supernode; wave w takes the columns
// == w (mod 4), lanes stride the rows (coalesced).
// (CX: the checks run on the twin the storage stands for -- ldx rebuilds the odd columns)
template <bool CX>
__global__ void __launch_bounds__(256) k_factor_checks (const CheckTask *tasks, const FrontD *fr,
    const double *Lx, double *out)
{
    CheckTask T = tasks [blockIdx.x] ;
    const FrontD &f = fr [T.front] ;
    int nsrow = f.nsrow, nscol = f.nscol ;
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6 ;
    const double *L = Lx + f.psx ;
    double slog = 0.0, sq = 0.0 ;
    double nup = 0.0, nbad = 0.0, nneg = 0.0 ;
    int c1 = T.c0 + CHK_COLS < nscol ? T.c0 + CHK_COLS : nscol ;
    for (int j = T.c0 + wave ; j < c1 ; j += 4)
    {
        for (int i = lane ; i < nsrow ; i += 64)
        {
            double v = ldcx<CX> (L, i, col_local (f, j), nsrow) ;      // (a distributed front: the tasks cover this rank's slabs)
            if (i < j) { if (v != 0.0) nup += 1.0 ; }
            else
            {
                if (!(v - v == 0.0)) nbad += 1.0 ; else sq = __builtin_fma (v, v, sq) ;
                if (i == j) { if (v > 0.0) slog += log (v) ; else nneg += 1.0 ; }
            }
        }
    }
    double acc [5] = {slog, nup, nbad, sq, nneg} ;
    __shared__ double red [4][5] ;
#pragma unroll
    for (int q = 0 ; q < 5 ; q++)
    {
        double v = acc [q] ;
        for (int o = 32 ; o > 0 ; o >>= 1) v += __shfl_down (v, o) ;
        if (lane == 0) red [wave][q] = v ;
    }
    __syncthreads () ;
    if (threadIdx.x < 5)
    {
        double v = (red [0][threadIdx.x] + red [1][threadIdx.x]) + (red [2][threadIdx.x] + red [3][threadIdx.x]) ;
        if (v != 0.0) atomicAdd (&out [threadIdx.x], v) ;
    }
}

} // namespace sship
