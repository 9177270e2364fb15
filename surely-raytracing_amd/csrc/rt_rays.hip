// rt_rays.hip — the ray variants of the ahead-of-time path kernels (rt_kernel.h trace_body with
// LK = kLaunchRays), launched by rt_render_rays_device through render_device_rows (rt_device.hip).
// One instance per row of RT_VARIANTS (rt_variant.h), looked up by the variant; the op-counting
// kernels have no ray variant. A translation unit of its own, as rt_tiles.hip: these 18 instances
// compile beside rt_device.hip's instead of after them.
#include <hip/hip_runtime.h>

#include "rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_layout.h"
#include "rt_scene_impl.hpp"
#include "rt_variant.h"

using namespace rtk;

namespace {

// rt_device.hip's rt_trace with the variant switched on: same template arguments, launch bounds
// and walker as the plain kernel it stands in for
template <bool VOL, bool TEX, bool BVH, bool STAGED, bool VOLB, bool VOLI, int VN>
__global__ __launch_bounds__(BlockOf<BVH>::value, (MinWaves<VOL, TEX, BVH>::value)) void
rt_trace_rays(TraceParams P) {
  trace_body<false, VOL, TEX, BVH, STAGED, VOLB, VOLI, TravInterpN<VN>, kLaunchRays>(P);
}

}  // namespace

rts::kern_t rts::ray_trace_kernel(const rtv::Variant& v) {
#define RT_VARIANT_ROW(vol, tex, bvh, staged, volb, voli, vn)  \
  if (v == rtv::Variant{vol, tex, bvh, staged, volb, voli, vn}) \
    return rt_trace_rays<vol, tex, bvh, staged, volb, voli, vn>;
  RT_VARIANTS(RT_VARIANT_ROW)
#undef RT_VARIANT_ROW
  return nullptr;
}
