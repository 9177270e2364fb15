// rt_aov.hip — the first-hit AOV pass of include/rt_mi355x.h: the rt_aov kernels (body in
// rt_aov.h) and rt_render_aov / rt_render_aov_device. Its own translation unit so that it builds
// beside rt_device.hip (every path-kernel instance); the scene and render-slot types come from
// rt_scene_impl.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>

#include "rt_mi355x.h"
#include "rt_aov.h"
#include "rt_scene_impl.hpp"
#include "rt_variant.h"

using namespace rtk;
using namespace rts;

namespace {

// General instances only (every feature bit set: a bit set for a feature the scene lacks keeps
// code that never runs), over what changes the walker's data path: BVH (per-lane walker, the
// plan's 768-thread workgroup), STAGED (table reads from the LDS copy), VN (nested volumes).
// The pass carries no path state, so the register budget is left to the workgroup size alone.
template <bool BVH, bool STAGED, int VN>
__global__ __launch_bounds__(BlockOf<BVH>::value) void rt_aov(TraceParams P,
                                                              float* __restrict__ aov) {
  aov_body<true, true, BVH, STAGED, TravInterpN<VN>>(P, aov);
}

typedef void (*aov_kern_t)(TraceParams, float*);
// the instance for what the scene's variant (rt_variant.h) says of the walker's data path
aov_kern_t aov_kernel(const rtv::Variant& v) {
  if (v.vn) return v.bvh ? rt_aov<true, false, RTL_VOLUME_NEST> : rt_aov<false, false, RTL_VOLUME_NEST>;
  if (v.staged) return rt_aov<false, true, 0>;
  return v.bvh ? rt_aov<true, false, 0> : rt_aov<false, false, 0>;
}

int aov_device_rows(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts, float* aov,
                    void* stream_v, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  int sj0 = 0, n_sj = 0;
  RT_TRY(check_render_args(cam, opts, false, 1, &sj0, &n_sj));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)opts->n_rows * cam->image_width;
  if (n_px == 0) return RT_OK;
  std::unique_lock<std::mutex> lock(sc->mu);
  hipStream_t stream = (hipStream_t)stream_v;
  HIP_TRY(hipSetDevice(sc->device));
  // the pass needs no queue word and no workspace, but a slot gives it the scene's ordering and
  // lifetime rules (and the stats events) as any render has them
  SlotHold hold{sc, lock};
  RT_TRY(acquire_slot(sc, lock, stream, &hold.sl));
  // the interpreter's plan: the walker reads the staged tables, the compact BVHs and its per-lane
  // stacks where plan_lds put them, at the workgroup size the plan assumes
  const LdsPlan LP = plan_lds(sc->hdr, sc->o_perl, opts->flags, false, sc->lds_module_max);
  // RT_FLAG_INTERPRETER / RT_FLAG_SEMANTICS_REFERENCE change no first hit; the kernel reads
  // RT_FLAG_REFERENCE_BVH (the walker) and RT_FLAG_OVERWRITE
  TraceParams P;
  fill_trace_params(&P, sc, cam, opts, LP);
  P.sphere_light0 = -1;
  P.sj0 = sj0;
  P.n_sj = n_sj;
  const int n_tiles = P.tiles_x * ((opts->n_rows + kWaveTile - 1) / kWaveTile);
  const aov_kern_t kern = aov_kernel(rtv::choose_variant(sc->hdr, opts->flags, LP.stage_scene != 0));
  if (LP.lds_bytes > (64u << 10))
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)LP.lds_bytes));
  int resident = 0;  // only asked: the grid is one workgroup per block / 64 tiles
  RT_TRY(resident_blocks(sc, (const void*)kern, nullptr, LP.block, LP.lds_bytes, "AOV kernel",
                         &resident));
  hold.stream = stream;
  hold.enqueued = true;  // from here on a failure still records `done` (SlotHold)
  if (stats) HIP_TRY(hipEventRecord(hold.sl->ev0, stream));
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
  auto t0 = std::chrono::steady_clock::now();
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
    sum.ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *stats = sum;
  }
  return RT_OK;
}

int rt_render_aov(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts, float* aov,
                  rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!sc || !cam || !opts || !aov) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (opts->flags & RT_FLAG_COUNT_OPS)
    return set_err(RT_ERR_INVALID_ARG, "RT_FLAG_COUNT_OPS: the AOV pass counts no ops");
  if (opts->n_rows < 0 || cam->image_width <= 0) return set_err(RT_ERR_INVALID_ARG, "bad size");
  const size_t bytes =
      (size_t)opts->n_rows * cam->image_width * RT_AOV_CHANNELS * sizeof(float);
  if (bytes == 0) return RT_OK;
  HIP_TRY(hipSetDevice(sc->device));
  float* d = nullptr;
  HIP_TRY(hipMalloc(&d, bytes));
  hipError_t e = (opts->flags & RT_FLAG_OVERWRITE) ? hipSuccess
                                                   : hipMemcpy(d, aov, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(RT_ERR_HIP, std::string("upload aov: ") + hipGetErrorString(e));
  }
  rt_stats local;
  int rc = rt_render_aov_device(sc, cam, opts, d, nullptr, stats ? stats : &local);
  if (rc == RT_OK) {
    e = hipMemcpy(aov, d, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
      rc = set_err(RT_ERR_HIP, std::string("download aov: ") + hipGetErrorString(e));
  }
  (void)hipFree(d);
  if (rc == RT_OK && stats)
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

}  // extern "C"
