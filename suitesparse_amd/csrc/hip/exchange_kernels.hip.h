// exchange_kernels.hip.h -- gfx950 kernels of the exchange of a shared front's block column (exchange.hip launches
// them): the pack / unpack of its row chunks around the collectives (k_xchg_move; the geometry is descriptors.hip.h:
// XchgD, filled in by schedule_dense.hip) and the progress marker (k_mark).  The window kernels of a distributed front
// (k_win_move, k_extend_add) stay in kernels.hip.h: engine.hip launches them.
#pragma once
#include "device_util.hip.h"

namespace sship {

// ---- multi-GPU: packing of a shared front's block column for the row-split exchange ----
// A block column [b0, b0+w) of a front shared by g ranks holds per-rank partial sums in
// its live rows (>= b0).  It is summed with ONE reduce-scatter whose segment q carries
//     [ D : the w x w diagonal block (ld = w) | near chunk q : R x w (ld = R) | far chunk q : Rf x w (ld = Rf) ]
// NEAR rows = the rows below D inside the outer block column [b0 + w, o1): later block columns of the
// outer block need them as an operand; FAR rows = [o1, nsrow), cut into the SAME g chunks for every block
// column of the outer block (chunks zero-padded past their last row).  Every rank receives the summed
// diagonal block and the summed rows of ITS two chunks, runs the panel chain (dpotrf / dtrsm / K < 512
// updates, reference t_cholmod_super_numeric.c:864-867, :997-1002) on those rows only, and the solved
// chunks travel back with two all-gathers: a small one of the near chunks, in line, and a large one of the
// far chunks that nobody needs before the outer update (round 5: the updates between the block columns of
// an outer block are chunk-local on the far rows), so it runs on the exchange stream beside the chain of the
// following block columns.  Same volume as the all-reduce it replaces.
// mode 0: Lx -> stage (all g segments: this rank's partial sums, D repeated per segment)
// mode 1: segment r of stage -> Lx (summed D and own chunks)
// mode 2: own near chunk of Lx -> ag + r R w        mode 3: ag (all near chunks but r) -> Lx
// mode 4: own far chunk of Lx -> ag + r Rf w        mode 5: ag (all far chunks but r) -> Lx   (ag: the buffer of that gather)
// (round 4: one workgroup = one column of the block column x one part -- the diagonal block or one row chunk; rows
// stream contiguously, no division per element: the element-indexed first version moved ~1 TB/s, and a rank of 8 moves
// 67 GB through these copies per factorization of Poisson 200^3)
// grid: w * (2 g + 1) workgroups for mode 0 (part 2 g = the diagonal block), w * 3 for mode 1 (D, own chunks), w for
// modes 2 / 4, w * g for modes 3 / 5.
// progress marker (cholmod_hip_progress_enable): one word into host-visible memory, in stream order -- a watchdog
// thread of the host reads which exchange of the factorization a hung rank has entered and not left
__global__ void k_mark (volatile long long *p, long long v)
{
    *p = v ;
    __threadfence_system () ;
}

// n doubles from src to dst, those at index >= nr as zeros (pad) or not at all: four independent loads per thread in flight
// (the pack of a block column and the unpack of the gathered chunks are 48 GB each per rank of 8 and factorization)
__device__ __forceinline__ void xm_copy (double *dst, const double *src, int n, int nr, int tid, int nt, bool pad)
{
    int i = tid ;
    for ( ; i + 3 * nt < n ; i += 4 * nt)
    {
        double v [4] ;
#pragma unroll
        for (int u = 0 ; u < 4 ; u++) { const int e = i + u * nt ; v [u] = (e < nr) ? __builtin_nontemporal_load (src + e) : 0.0 ; }
#pragma unroll
        for (int u = 0 ; u < 4 ; u++) { const int e = i + u * nt ; if (pad || e < nr) dst [e] = v [u] ; }
    }
    for ( ; i < n ; i += nt) { if (i < nr) dst [i] = __builtin_nontemporal_load (src + i) ; else if (pad) dst [i] = 0.0 ; }
}

__global__ void __launch_bounds__(256) k_xchg_move (XchgD X, int mode, double *Lx, double *stage, double *ag)
{
    const i64 seg = (i64) X.w * X.w + ((i64) X.R + X.Rf) * X.w ;
    const int j = (int) blockIdx.x % X.w, part = (int) blockIdx.x / X.w ;
    double *S = Lx + X.slab + (i64) j * X.lda ;                   // column j of the block column, from the diagonal block's first row
    const int tid = threadIdx.x, nt = (int) blockDim.x ;
    // chunk q of the near (far = false) or far rows: where it starts in the column, its rows that exist, its place in a segment
    auto rows_of = [&] (bool far, int q, int &first, int &nr, int &R, i64 &sofs)
    {
        R = far ? X.Rf : X.R ;
        first = (far ? X.fo : X.w) + q * R ;
        nr = (far ? X.mf : X.mb) - q * R ;
        sofs = (i64) X.w * X.w + (far ? (i64) X.R * X.w : 0) + (i64) j * R ;
    } ;
    int first, nr, R ; i64 sofs ;
    if (mode == 0)
    {
        if (part == 2 * X.g)
        {
            // the diagonal block's column j (lower part, zero above) into every segment
            for (int i = tid ; i < X.w ; i += nt)
            {
                const double v = (i >= j) ? S [i] : 0.0 ;
                for (int q = 0 ; q < X.g ; q++) stage [(i64) q * seg + (i64) j * X.w + i] = v ;
            }
        }
        else
        {
            const int q = part % X.g ;
            rows_of (part >= X.g, q, first, nr, R, sofs) ;
            xm_copy (stage + (i64) q * seg + sofs, S + first, R, nr, tid, nt, true) ;
        }
    }
    else if (mode == 1)
    {
        const double *ps = stage + (i64) X.r * seg ;
        if (part == 0) { for (int i = j + tid ; i < X.w ; i += nt) S [i] = ps [(i64) j * X.w + i] ; }
        else
        {
            rows_of (part == 2, X.r, first, nr, R, sofs) ;
            const double *src = ps + sofs ;
            double *dst = S + first ;
            for (int i = tid ; i < R && i < nr ; i += nt) dst [i] = src [i] ;
        }
    }
    else if (mode == 2 || mode == 4)
    {
        rows_of (mode == 4, X.r, first, nr, R, sofs) ;
        const double *src = S + first ;
        double *dst = ag + (i64) X.r * R * X.w + (i64) j * R ;
        for (int i = tid ; i < R ; i += nt) dst [i] = (i < nr) ? src [i] : 0.0 ;
    }
    else
    {
        const int q = part ;
        if (q == X.r || q >= X.g) return ;
        rows_of (mode == 5, q, first, nr, R, sofs) ;
        const double *src = ag + (i64) q * R * X.w + (i64) j * R ;
        xm_copy (S + first, src, R < nr ? R : nr, nr, tid, nt, false) ;
    }
}

} // namespace sship
