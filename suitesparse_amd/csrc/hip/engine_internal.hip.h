// engine_internal.hip.h -- what engine.hip shares with values.hip: the two steps of a factorization that the matrix-values
// pipeline calls, and the release of the product map that the plan's destruction calls back.  The factorization kernels
// (kernels.hip.h, chain256_kernels.hip.h) stay in engine.hip's translation unit.  Internal to the library: not exported.
#pragma once
#include "plan.hip.h"

namespace sship {
#pragma GCC visibility push(hidden)

// engine.hip: what a factorization enqueues before it touches a value (start event, reallocation, clearing of L and counters)
int factorize_prologue (cholmod_hip_plan *P) ;
// engine.hip: the numeric factorization on the resident S; leaves Lx on the device, *minor as cholmod_l_factorize reports it
int run_factorize (cholmod_hip_plan *P, double beta, int quick, i64 *minor) ;
// values.hip: releases the product map of the value map and its transpose (free_device; a new matrix or value map)
void drop_product_map (cholmod_hip_plan *P) ;

#pragma GCC visibility pop
} // namespace sship
