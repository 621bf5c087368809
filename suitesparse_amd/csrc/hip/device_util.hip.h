// device_util.hip.h -- the few device helpers the factorization kernels (kernels.hip.h), the solve kernels
// (solve_kernels.hip.h) and the check kernels (check_kernels.hip.h) share: the vector types, the access to a complex factor in its own storage, a binary search
// and two lane exchanges.  Inline code only, so that several objects of one library may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "descriptors.hip.h"

namespace sship {

typedef double d4 __attribute__((ext_vector_type(4))) ;
typedef double d2u __attribute__((ext_vector_type(2), aligned(8))) ;

// ---- complex factors in their own storage (CX) -----------------------------------------
// A complex factor is computed on the index space of its real twin (phi embedding: rows /
// columns 2i, 2i+1 = re, im of i; host/complex.c) but STORED as the reference stores it
// (t_cholmod_super_numeric.c:41-83: L complex, interleaved): of every front only the even twin
// columns exist -- column c of the twin lives at (c >> 1) * ld, ld = the twin's row count =
// twice the complex one -- i.e. the panel IS the interleaved complex panel (2 xsize doubles
// instead of the twin's 4 xsize).  The odd columns are the rotations of the even ones,
//     twin (2i, 2j+1) = -twin (2i+1, 2j)      twin (2i+1, 2j+1) = twin (2i, 2j),
// and are rebuilt on the way into LDS / registers by ldcx; stcx keeps the even columns only.
// `base` must address an element with an even row and an even column of the twin.
template <bool CX>
__device__ __forceinline__ double ldcx (const double *base, int r, int c, i64 ld)
{
    if constexpr (!CX) return base [r + (i64) c * ld] ;
    else
    {
        const double v = base [(r ^ (c & 1)) + (i64) (c >> 1) * ld] ;
        return ((c & 1) && !(r & 1)) ? -v : v ;
    }
}
template <bool CX>
__device__ __forceinline__ void stcx (double *base, int r, int c, i64 ld, double v)
{
    if constexpr (!CX) base [r + (i64) c * ld] = v ;
    else if (!(c & 1)) base [r + (i64) (c >> 1) * ld] = v ;
}
// offset of twin column c of a panel with leading dimension ld
template <bool CX> __host__ __device__ __forceinline__ i64 colx (int c, i64 ld) { return CX ? (i64) (c >> 1) * ld : (i64) c * ld ; }

__device__ __forceinline__ int lower_bound_i32 (const i32 *a, int n, int v)
{
    int lo = 0, hi = n ;
    while (lo < hi) { int mid = (lo + hi) >> 1 ; if (a [mid] < v) lo = mid + 1 ; else hi = mid ; }
    return lo ;
}

// v as lane l holds it (l uniform)
__device__ __forceinline__ double readlane_f64 (double v, int l)
{
    int lo = __double2loint (v), hi = __double2hiint (v) ;
    lo = __builtin_amdgcn_readlane (lo, l) ;
    hi = __builtin_amdgcn_readlane (hi, l) ;
    return __hiloint2double (hi, lo) ;
}
// v as the other lane of the pair (lane ^ 1) holds it
__device__ __forceinline__ double lane_xor1_f64 (double v)
{
    int lo = __double2loint (v), hi = __double2hiint (v) ;
    lo = __builtin_amdgcn_update_dpp (0, lo, 0xB1, 0xF, 0xF, true) ;       // quad_perm [1, 0, 3, 2]
    hi = __builtin_amdgcn_update_dpp (0, hi, 0xB1, 0xF, 0xF, true) ;
    return __hiloint2double (hi, lo) ;
}

} // namespace sship
