// tinsel_baked.hip -- a BAKED instance's translation unit: the library's closed FIT kernel, tn::k_bounce<kBounceFitClosed, true, false>,
// compiled for the one scene whose generated header -DTN_BAKED_HEADER names (tn_scene.h, tn_baked.h).
// Not part of the library: tinsel_amd/build.py bake() compiles it on request, device code only, with the parity flags of tinsel_hip.hip,
// and tinsel_hip_install_baked loads the result.
#ifndef TN_BAKED_HEADER
#error "tinsel_baked.hip is compiled with -DTN_BAKED_HEADER=\"<generated header>\" (tinsel_amd/build.py bake())"
#endif

#include "tn_fused.h"

template __global__ void tn::k_bounce<tn::kBounceFitClosed, true, false>(tn::BounceKernargs);
