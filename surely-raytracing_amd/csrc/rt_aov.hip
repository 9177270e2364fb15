// rt_aov.hip — the first-hit AOV pass of include/rt_mi355x.h: the rt_aov kernels (body in
// rt_aov.h) and rt_render_aov / rt_render_aov_device. Its own translation unit so that it builds
// beside rt_device.hip (every path-kernel instance); the scene and render-slot types come from
// rt_scene_impl.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>

#include "rt_mi355x.h"
#include "rt_aov.h"
#include "rt_pass.hpp"
#include "rt_stage.hpp"

using namespace rtk;
using namespace rts;

namespace {

// General instances only (every feature bit set: a bit set for a feature the scene lacks keeps
// code that never runs), over what changes the walker's data path (RT_RETURN_INTERP_KERNEL).
// The pass carries no path state, so the register budget is left to the workgroup size alone.
template <bool BVH, bool STAGED, int VN>
__global__ __launch_bounds__(BlockOf<BVH>::value) void rt_aov(TraceParams P,
                                                              float* __restrict__ aov) {
  aov_body<true, true, BVH, STAGED, TravInterpN<VN>>(P, aov);
}

typedef void (*aov_kern_t)(TraceParams, float*);
aov_kern_t aov_kernel(const rtv::Variant& v) { RT_RETURN_INTERP_KERNEL(v, rt_aov); }

int aov_device_rows(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts, float* aov,
                    void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  int sj0 = 0, n_sj = 0;
  RT_TRY(check_render_args(cam, opts, false, 1, &sj0, &n_sj));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)opts->n_rows * cam->image_width;
  if (n_px == 0) return RT_OK;
  std::unique_lock<std::mutex> lock(sc->mu);
  hipStream_t stream = (hipStream_t)stream_v;
  SlotHold hold{sc, lock};
  InterpPass ip;
  // RT_FLAG_INTERPRETER / RT_FLAG_SEMANTICS_REFERENCE change no first hit; the kernel reads
  // RT_FLAG_REFERENCE_BVH (the walker) and RT_FLAG_OVERWRITE
  RT_TRY(begin_interp_pass(sc, hold, stream, cam, opts, &ip));
  const LdsPlan& LP = ip.LP;
  TraceParams& P = ip.P;
  P.sj0 = sj0;
  P.n_sj = n_sj;
  const int n_tiles = P.tiles_x * ((opts->n_rows + kWaveTile - 1) / kWaveTile);
  const aov_kern_t kern = aov_kernel(ip.v);
  RT_TRY(arm_interp_launch(sc, hold, stream, (const void*)kern, LP, "AOV kernel",
                           stats != nullptr));
  const int tiles_per_block = LP.block / 64;
  const unsigned blocks = (unsigned)((n_tiles + tiles_per_block - 1) / tiles_per_block);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(LP.block), LP.lds_bytes, stream, P, aov);
  HIP_TRY(hipGetLastError());
  rt_stats counts{};
  counts.samples = (uint64_t)n_px * (uint64_t)n_sj * (uint64_t)cam->sqrt_spp;
  counts.out_bytes = (uint64_t)n_px * RT_AOV_CHANNELS * sizeof(float);
  counts.launches = 1;
  return complete_render(hold, stream, stats, counts, false, t0);
}

}  // namespace

extern "C" {

int rt_render_aov_device(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts,
                         float* aov, void* stream_v, rt_stats* stats) {
  if (!sc || !cam || !opts || !aov) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (opts->flags & RT_FLAG_COUNT_OPS)
    return set_err(RT_ERR_INVALID_ARG, "RT_FLAG_COUNT_OPS: the AOV pass counts no ops");
  if (opts->n_rows <= kRowsPerCall || cam->image_width <= 0)
    return aov_device_rows(sc, cam, opts, aov, stream_v, stats);
  // taller row ranges: consecutive sub-renders, as rt_render_device splits them
  const time_point t0 = std::chrono::steady_clock::now();
  rt_stats part{}, sum{};
  for (int k0 = 0; k0 < opts->n_rows; k0 += kRowsPerCall) {
    rt_render_opts o = *opts;
    o.row_begin = opts->row_begin + k0 * opts->row_step;
    o.n_rows = std::min(kRowsPerCall, opts->n_rows - k0);
    const int rc =
        aov_device_rows(sc, cam, &o, aov + (size_t)k0 * cam->image_width * RT_AOV_CHANNELS,
                        stream_v, stats ? &part : nullptr);
    if (rc != RT_OK) return rc;
    if (stats) {
      sum.ms_kernel += part.ms_kernel;
      sum.samples += part.samples;
      sum.out_bytes += part.out_bytes;
      sum.launches += part.launches;
    }
  }
  if (stats) {
    sum.ms_total = ms_since(t0);
    *stats = sum;
  }
  return RT_OK;
}

int rt_render_aov(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts, float* aov,
                  rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  if (!sc || !cam || !opts || !aov) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (opts->flags & RT_FLAG_COUNT_OPS)
    return set_err(RT_ERR_INVALID_ARG, "RT_FLAG_COUNT_OPS: the AOV pass counts no ops");
  if (opts->n_rows < 0 || cam->image_width <= 0) return set_err(RT_ERR_INVALID_ARG, "bad size");
  const size_t bytes =
      (size_t)opts->n_rows * cam->image_width * RT_AOV_CHANNELS * sizeof(float);
  if (bytes == 0) return RT_OK;
  Staging st;
  const int i_aov = st.add(bytes);
  RT_TRY(st.alloc(sc->device));
  if (!(opts->flags & RT_FLAG_OVERWRITE)) RT_TRY(st.upload(i_aov, aov));
  rt_stats local;
  RT_TRY(rt_render_aov_device(sc, cam, opts, st.ptr<float>(i_aov), nullptr,
                              stats ? stats : &local));
  RT_TRY(st.download(i_aov, aov));
  if (stats) stats->ms_total = ms_since(t0);
  return RT_OK;
}

}  // extern "C"
