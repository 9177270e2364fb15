// rt_tiles.hip — the tile-list variants of the ahead-of-time path kernels (rt_kernel.h trace_body
// with TILES = true), launched by rt_render_tiles_device through render_device_rows
// (rt_device.hip). One instance per product kernel of rt_device.hip's tables; the op-counting
// kernels have no variant. A translation unit of its own: these 18 instances compile beside
// rt_device.hip's instead of after them.
#include <hip/hip_runtime.h>

#include "rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_layout.h"
#include "rt_scene_impl.hpp"

using namespace rtk;

namespace rts {
typedef void (*tile_kern_t)(TraceParams);
RTS_HIDDEN tile_kern_t tile_trace_kernel(int set, int idx);
}  // namespace rts

namespace {

// rt_device.hip's rt_trace with the variant switched on: same template arguments, launch bounds
// and walker as the plain kernel it stands in for
template <bool VOL, bool TEX, bool BVH, bool STAGED, bool VOLB = VOL, bool VOLI = true, int VN = 0>
__global__ __launch_bounds__(BlockOf<BVH>::value, (MinWaves<VOL, TEX, BVH>::value)) void
rt_trace_tiles(TraceParams P) {
  trace_body<false, VOL, TEX, BVH, STAGED, VOLB, VOLI, TravInterpN<VN>, true>(P);
}

}  // namespace

rts::tile_kern_t rts::tile_trace_kernel(int set, int idx) {
  // the product halves of rt_device.hip's tables, in their order
  static const tile_kern_t plain[8] = {
      rt_trace_tiles<false, false, false, false>, rt_trace_tiles<false, false, true, false>,
      rt_trace_tiles<false, true, false, false>,  rt_trace_tiles<false, true, true, false>,
      rt_trace_tiles<true, false, false, false>,  rt_trace_tiles<true, false, true, false>,
      rt_trace_tiles<true, true, false, false>,   rt_trace_tiles<true, true, true, false>};
  static const tile_kern_t staged[4] = {
      rt_trace_tiles<false, false, false, true>, rt_trace_tiles<false, true, false, true>,
      rt_trace_tiles<true, false, false, true>,  rt_trace_tiles<true, true, false, true>};
  static const tile_kern_t bvh_novolb[4] = {rt_trace_tiles<true, false, true, false, false>,
                                            rt_trace_tiles<true, true, true, false, false>,
                                            rt_trace_tiles<true, false, true, false, false, false>,
                                            rt_trace_tiles<true, true, true, false, false, false>};
  static const tile_kern_t nested[2] = {
      rt_trace_tiles<true, true, false, false, true, true, RTL_VOLUME_NEST>,
      rt_trace_tiles<true, true, true, false, true, true, RTL_VOLUME_NEST>};
  switch (set) {
    case 0: return idx >= 0 && idx < 8 ? plain[idx] : nullptr;
    case 1: return idx >= 0 && idx < 4 ? staged[idx] : nullptr;
    case 2: return idx >= 0 && idx < 4 ? bvh_novolb[idx] : nullptr;
    case 3: return idx >= 0 && idx < 2 ? nested[idx] : nullptr;
  }
  return nullptr;
}
