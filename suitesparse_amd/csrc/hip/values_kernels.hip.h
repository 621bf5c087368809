// values_kernels.hip.h -- device kernels of the matrix-values pipeline (values.hip): new values of the caller's matrix into
// the resident S, given or computed as sums of products.  (k_values_chunk, which applies a chunk of a value upload inside the
// launch loop of a factorization, is with the factorization kernels: kernels.hip.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "descriptors.hip.h"

namespace sship {

// Sx [q] = values [src [q]]: new values of the caller's matrix into the resident S
__global__ void __launch_bounds__(256) k_gather_values (i64 nz, const i64 *src, const double *values, double *Sx)
{
    i64 q = blockIdx.x * (i64) 256 + threadIdx.x ;
    if (q < nz) Sx [q] = values [src [q]] ;
}

// Values that are not given but computed (cholmod_hip_set_product_map): vals [c] = sum over the pairs p of list c,
// cp [c] <= p < cp [c + 1], of a [ia [p]] * a [ib [p]] -- the entries of tril (A A') from the values of A, a list per
// entry, its pairs by ascending column of A.  Lists are 1 pair long (two rows of A that share one column) up to a whole
// row of A (a diagonal entry of a dense row), so the entries come sorted into three classes by length (order [g]: the
// entry group g of this launch owns) and a group of G lanes owns one entry:
//     G = 1    lists of <= PM_LEN1 pairs: lane = entry, the lanes of a wave hold lists of about one length;
//     G = 16   up to PM_LEN16: four entries to a wave, a list is at most PM_LEN16 / 16 rounds;
//     G = 64   above: a wave walks one list 64 pairs a round, two independent gathers per lane in flight.
// Lane l of a group adds the pairs l, l + G, l + 2 G, ... in that order (fused multiply-add), then the G partial sums
// meet in a butterfly of fixed shape: one owner per entry, the order a function of the list alone, no floating-point
// atomic -- the same values give the same bits, as in residual_kernels.hip.h.  Every index was checked on the host when
// the map was set: nothing outside a [0 .. navalues) is read.  (PM_LEN1, PM_LEN16: descriptors.hip.h)
template <int G>
__global__ void __launch_bounds__(256) k_product_values (i64 ngroups, const i32 *order, const i64 *cp, const i64 *ia, const i64 *ib,
    const double *a, double *vals)
{
    const i64 t = blockIdx.x * (i64) 256 + threadIdx.x ;
    const i64 g = t / G ;
    const int l = (int) (t % G) ;
    // (a whole group leaves together: the shuffles below see the lanes of live groups only)
    if (g >= ngroups) return ;
    const i64 c = order [g] ;
    const i64 p1 = cp [c + 1] ;
    double acc = 0.0 ;
#pragma unroll 2
    for (i64 p = cp [c] + l ; p < p1 ; p += G) acc = __builtin_fma (a [ia [p]], a [ib [p]], acc) ;
#pragma unroll
    for (int w = G / 2 ; w > 0 ; w >>= 1) acc += __shfl_xor (acc, w, 64) ;
    if (l == 0) vals [c] = acc ;
}

} // namespace sship
