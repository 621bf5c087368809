// update_launch.hip.h -- the one place that decides how a one-wave update launch (k_update3 / k_update3f / k_update3g,
// kernels.hip.h) goes to the device: which instantiation, which grid, which block.  The engine's runner (engine.hip) and
// the probe library (probes.hip) both launch through it, so the kernel-level tests run the dispatch that ships.
// Knows the kernels and nothing of the plan.
#pragma once
#include "kernels.hip.h"
#include "../../../include/cholmod_hip.h"
#include <cstdio>

namespace sship {

// The update kernels' TW by a run-time value -- 0 real, 1 twin (even-column contraction), 2 complex storage:
// f (std::integral_constant<int, TW>).
template <typename F>
inline void with_tw (int tw, F &&f)
{
    if (tw == 2) f (std::integral_constant<int, 2> ()) ;
    else if (tw == 1) f (std::integral_constant<int, 1> ()) ;
    else f (std::integral_constant<int, 0> ()) ;
}

// operand sets in flight: four for long contractions, two for short ones (tools/upd3.py); kmax = the longest K of the launch
inline int upd3_depth (int kmax) { return kmax >= 1024 ? 4 : 2 ; }

// Blocks of a launch of `tiles` tiles (the regions' nblk, summed):
//   one tile per one-wave workgroup: as many;
//   half: two waves per tile, blocks b and b + 8 share one -- twice the tiles, in whole groups of eight;
//   wg4:  four tiles per four-wave workgroup, eight workgroups (one per XCD) take a group of 32.
inline unsigned upd3_grid (int tiles, bool half, bool wg4)
{
    if (wg4) return (unsigned) (((tiles + 31) / 32) * 8) ;
    if (half) return 2u * (unsigned) ((tiles + 7) / 8 * 8) ;
    return (unsigned) tiles ;
}

// what a caller knows of the launch
struct Upd3Shape
{
    int tiles ;             // its tiles (Launch::grid)
    int kmax ;              // the longest contraction among its regions (Launch::aux)
    bool half ;             // two waves per tile (one GPU: launches of 512 .. 10 240 tiles, schedule_dense.hip)
    bool wg4 ;              // four tiles per workgroup (several ranks, see k_update3)
    int tw ;                // see with_tw
    int depth = 0 ;         // probes: operand sets in flight; 0 = by kmax
} ;

// side arrays of a launch with a carrier (k_update3f; gfz already at the launch's first region)
struct Upd3Fuse { const i32 *gfz ; const FuseD *fz ; const ChildD *cdesc ; const i32 *invmap ; } ;

namespace upd3_detail {

// What the schedule guarantees and the kernels are built for: four tiles per workgroup only for plain whole tiles; carriers
// and gathered regions only in real plans; a carrier has its side arrays.
inline bool valid (const Upd3Shape &s, int depth, bool side_arrays)
{
    if (s.wg4 && (s.half || side_arrays)) return false ;
    if (side_arrays && s.tw != 0) return false ;
#ifdef UPD3_PROBE_DEPTH3
    if (depth == 3) return !s.half && !s.wg4 && !side_arrays && s.tw == 0 ;
#endif
    return depth == 2 || depth == 4 ;
}

inline int invalid ()
{
    fprintf (stderr, "cholmod_hip: a fused update launch without its side arrays\n") ;
    return CHOLMOD_HIP_INVALID ;
}

// f (std::integral_constant<int, DEPTH>): 4 or 2
template <typename F>
inline void with_depth (int depth, F &&f)
{
    if (depth == 4) f (std::integral_constant<int, 4> ()) ; else f (std::integral_constant<int, 2> ()) ;
}

// f (std::integral_constant<int, DEPTH>, std::bool_constant<HALF>)
template <typename F>
inline void with_depth_half (int depth, bool half, F &&f)
{
    with_depth (depth, [&] (auto D) { if (half) f (D, std::true_type ()) ; else f (D, std::false_type ()) ; }) ;
}

}   // namespace upd3_detail

// regions g [0 .. ng): C -= A B' (or C = -A B') with one wave per 64 x 64 tile or per half of one
inline int launch_update3 (hipStream_t st, const GemmGroup *g, int ng, double *Lx, double *CB, const Upd3Shape &s,
    const Upd3Fuse *fuse = nullptr)
{
    using namespace upd3_detail ;
    const int depth = s.depth ? s.depth : upd3_depth (s.kmax) ;
    if (!valid (s, depth, fuse != nullptr) || (fuse && !(fuse->gfz && fuse->fz))) return invalid () ;
    const dim3 grid (upd3_grid (s.tiles, s.half, s.wg4)), block (s.wg4 ? 256 : 64) ;
#ifdef UPD3_PROBE_DEPTH3
    if (depth == 3) { hipLaunchKernelGGL ((k_update3<3>), grid, block, 0, st, g, ng, Lx, CB) ; return CHOLMOD_HIP_OK ; }
#endif
    if (fuse)
        with_depth_half (depth, s.half, [&] (auto D, auto H)
        {
            hipLaunchKernelGGL ((k_update3f<decltype (D)::value, decltype (H)::value>), grid, block, 0, st,
                g, ng, fuse->gfz, fuse->fz, fuse->cdesc, fuse->invmap, Lx, CB) ;
        }) ;
    else if (s.wg4)
        with_tw (s.tw, [&] (auto TW) { with_depth (depth, [&] (auto D)
        {
            hipLaunchKernelGGL ((k_update3<decltype (D)::value, decltype (TW)::value, 4>), grid, block, 0, st, g, ng, Lx, CB) ;
        }) ; }) ;
    else
        with_tw (s.tw, [&] (auto TW) { with_depth_half (depth, s.half, [&] (auto D, auto H)
        {
            hipLaunchKernelGGL ((k_update3<decltype (D)::value, decltype (TW)::value, 1, decltype (H)::value>), grid, block, 0, st,
                g, ng, Lx, CB) ;
        }) ; }) ;
    return CHOLMOD_HIP_OK ;
}

// gathered regions g [0 .. ng) (head updates over the rows their heads reach) and their row maps
inline int launch_update3g (hipStream_t st, const GatherGroup *g, int ng, const i32 *rmap, double *Lx, double *CB, const Upd3Shape &s)
{
    using namespace upd3_detail ;
    const int depth = s.depth ? s.depth : upd3_depth (s.kmax) ;
    if (!valid (s, depth, true)) return invalid () ;
    with_depth_half (depth, s.half, [&] (auto D, auto H)
    {
        hipLaunchKernelGGL ((k_update3g<decltype (D)::value, decltype (H)::value>), dim3 (upd3_grid (s.tiles, s.half, false)), dim3 (64), 0, st,
            g, ng, rmap, Lx, CB) ;
    }) ;
    return CHOLMOD_HIP_OK ;
}

}   // namespace sship
