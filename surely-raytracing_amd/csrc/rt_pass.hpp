// rt_pass.hpp — the launch of a pass that runs the interpreter's walker on the interpreter's LDS
// plan with one of five general kernel instances: the first-hit AOV pass (rt_aov.hip) and the ray
// queries (rt_query.hip). Host only; the steps themselves are rt_scene_impl.hpp's.
#pragma once
#include "rt_kernel.h"  // TraceParams
#include "rt_scene_impl.hpp"
#include "rt_variant.h"

// The body of a function that returns the instance of the kernel template
// KERN<BVH, STAGED, VN, trailing arguments...> for what the scene's variant `v` says of the
// walker's data path: BVH (per-lane walker, the plan's 768-thread workgroup), STAGED (table reads
// from the LDS copy), VN (nested volumes). A macro: a function template cannot be passed as a
// template argument.
#define RT_RETURN_INTERP_KERNEL(v, KERN, ...)                                 \
  if ((v).vn)                                                                 \
    return (v).bvh ? KERN<true, false, RTL_VOLUME_NEST, ##__VA_ARGS__>        \
                   : KERN<false, false, RTL_VOLUME_NEST, ##__VA_ARGS__>;      \
  if ((v).staged) return KERN<false, true, 0, ##__VA_ARGS__>;                 \
  return (v).bvh ? KERN<true, false, 0, ##__VA_ARGS__> : KERN<false, false, 0, ##__VA_ARGS__>

namespace rts {

struct InterpPass {
  LdsPlan LP;
  rtk::TraceParams P;
  rtv::Variant v;
};

// With sc->mu held through hold.lock: a slot on `stream` into `hold` (the pass needs no queue word
// and no workspace, but a slot gives it the scene's ordering and lifetime rules and the stats
// events, as any render has them), the interpreter's plan (the walker reads the staged tables, the
// compact BVHs and its per-lane stacks where plan_lds put them, at the workgroup size the plan
// assumes), the TraceParams of cam and opts on it, and the scene's variant.
inline int begin_interp_pass(rt_scene* sc, SlotHold& hold, hipStream_t stream, const rt_camera* cam,
                             const rt_render_opts* opts, InterpPass* ip) {
  HIP_TRY(hipSetDevice(sc->device));
  RT_TRY(acquire_slot(sc, hold.lock, stream, &hold.sl));
  ip->LP = plan_lds(sc->hdr, sc->o_perl, opts->flags, false, sc->lds_module_max);
  fill_trace_params(&ip->P, sc, cam, opts, ip->LP);
  ip->P.sphere_light0 = -1;
  ip->v = rtv::choose_variant(sc->hdr, opts->flags, ip->LP.stage_scene != 0);
  return RT_OK;
}

// The last steps before the launch of `kern` (`what` in error texts) on the pass's plan. From
// here on a failure still records the slot's `done` (SlotHold); timed: ev0 goes into the stream.
inline int arm_interp_launch(rt_scene* sc, SlotHold& hold, hipStream_t stream, const void* kern,
                             const LdsPlan& LP, const char* what, bool timed) {
  if (LP.lds_bytes > (64u << 10))
    HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)LP.lds_bytes));
  int resident = 0;  // only asked: these grids do not depend on it
  RT_TRY(resident_blocks(sc, kern, nullptr, LP.block, LP.lds_bytes, what, &resident));
  hold.stream = stream;
  hold.enqueued = true;
  if (timed) HIP_TRY(hipEventRecord(hold.sl->ev0, stream));
  return RT_OK;
}

}  // namespace rts
