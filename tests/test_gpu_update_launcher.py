"""Kernel-level GPU tests of the one-wave update kernel k_update3 as the engine's launcher starts it
(csrc/hip/update_launch.hip.h; run with -m gpu on an MI355X).  They go with
tests/test_gpu_parity.py::test_wave_tile_kernel_16x16_super_tile_walk_is_bit_identical, which covers the 16 x 16 walk."""
import pytest

from suitesparse_amd import cholmod as ch

pytestmark = pytest.mark.gpu

UPD3_D3, UPD3_D2, UPD3_D4, UPD3_HALF, UPD3_WG4 = 8192, 16384, 32768, 524288, 1048576
UPD3_VARIANTS = {"D2": UPD3_D2, "D3": UPD3_D3, "D4": UPD3_D4, "HALF|D2": UPD3_HALF | UPD3_D2, "HALF|D4": UPD3_HALF | UPD3_D4,
                 "WG4|D2": UPD3_WG4 | UPD3_D2, "WG4|D4": UPD3_WG4 | UPD3_D4}
# (m, n, k, tri, assign): the smallest regions that reach each branch of the block -> tile remaps (kernels.hip.h:
# upd3_virtual_block) and of the grids (update_launch.hip.h: upd3_grid)
UPD3_SHAPES = ((64, 64, 8, 0, 0),           # one tile: every other block of a group of 8 / 16 / 32 returns early
               (129, 33, 5, 0, 0),          # the right half of the last tile column is one column wide
               (129, 31, 7, 0, 1),          # ... is empty: the early return
               (200, 130, 67, 0, 0),        # 12 tiles, ragged in both directions, K no multiple of 4
               (577, 577, 9, 1, 0),         # 55 triangular tiles: more than one group of 32, no multiple of 8
               (1000, 700, 12, 1, 1),       # 121 tiles, trapezoid, assign, two groups of 64
               (3900, 3333, 9, 1, 0),       # 1855 tiles: the XCD walk is on, the remaps must keep block % 8
               (4096, 4096, 16, 0, 0))      # 4096 whole tiles, XCD walk on


@pytest.mark.parametrize("variant", list(UPD3_VARIANTS))
def test_wave_tile_kernel_variants_through_the_launcher_are_bit_identical(variant):
    """k_update3 as the engine's launcher (update_launch.hip.h) starts it -- 2 / 3 / 4 operand sets in flight, half tiles
    (two waves per tile), four tiles per workgroup (what every plan of several ranks runs) -- covers every tile exactly once
    and computes every entry in k_update2's order: bitwise the result of k_update2<64,64,16,2> on the same operands.  Zero is
    what the whole-tile and half-tile forms measured standalone (profiles/r03b_update_kernels_standalone.json,
    profiles/r05_upd3_half_tiles.json); four tiles per workgroup run the same tile code, only the block -> tile map differs
    (measured 0.0 on every shape when the flag was added)."""
    Pr = ch.probes()
    for (m, n, k, tri, asg) in UPD3_SHAPES:
        d = Pr.cholmod_hip_debug_update_diff(m, n, k, tri, asg, UPD3_VARIANTS[variant])
        print(f"k_update3 {variant} {m}x{n}x{k} tri={tri} assign={asg}: max|diff|/max|ref| = {d!r}")
        assert d == 0.0, (variant, m, n, k, tri, asg, d)


def test_wave_tile_probe_rejects_four_per_workgroup_with_half_tiles():
    """Half tiles run one to a workgroup: the probes refuse the two flags together before anything is launched."""
    Pr = ch.probes()
    assert Pr.cholmod_hip_debug_update_diff(64, 64, 8, 0, 0, UPD3_WG4 | UPD3_HALF | UPD3_D2) == ch.HIP_INVALID
    assert Pr.cholmod_hip_bench_update_kernel(64, 64, 8, 1, UPD3_WG4 | UPD3_HALF | UPD3_D2) == ch.HIP_INVALID
