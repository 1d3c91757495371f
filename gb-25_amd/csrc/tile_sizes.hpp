// tile_sizes.hpp -- the tile sizes of the tendency kernels, each stated once: the kernels (kernels.hpp, tendency_kernels.hpp) index with
// them, the plans (tendency_plan.hpp) count blocks with them.  Plain C++, no HIP.
#pragma once
namespace {
constexpr int TX = 64, TY = 4;   // the direct-stencil kernels (option "kernels" = 1): tiles of 64 x 4 cells, one level
constexpr int V2_TX = 64;        // momentum: tile width = one wavefront; tile height (rows = waves per block) is a template parameter ...
constexpr int MOMENTUM_TY = 4;   // ... and this is the one instantiated: 4 blocks per CU cover each other's barriers
constexpr int V3_OUT = 63;       // tracers: outputs per wavefront
constexpr int V3_PAIR = 2 * V3_OUT;   // one tracer (CATKE's e), two columns per lane: outputs per wavefront
}  // namespace
