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

int aov_device_rows(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts, float* aov,
                    void* stream_v, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  // the size and stratum limits of render_device_rows, with its status codes (cam->max_depth is
  // not read: AOVs exist at max_depth 0 too)
  const int W = cam->image_width, S = cam->sqrt_spp;
  if (W <= 0 || cam->image_height <= 0 || S <= 0 || opts->n_rows < 0 || opts->row_step <= 0 ||
      opts->row_begin < 0)
    return set_err(RT_ERR_INVALID_ARG, "bad camera or row range");
  if (opts->n_rows > 0 &&
      (int64_t)opts->row_begin + (int64_t)(opts->n_rows - 1) * opts->row_step >= cam->image_height)
    return set_err(RT_ERR_INVALID_ARG, "row range outside the image");
  if ((int64_t)W * cam->image_height >= (1ll << 32) || (int64_t)S * S >= (1ll << 32))
    return set_err(RT_ERR_UNSUPPORTED, "image or spp too large for 32-bit pixel/sample keys");
  if (W > 65535 || opts->n_rows > 32767)
    return set_err(RT_ERR_UNSUPPORTED, "image_width > 65535 or n_rows > 32767 in one call");
  if (S > 32768) return set_err(RT_ERR_UNSUPPORTED, "spp > 2^30 (sqrt_spp > 32768)");
  const int sj0 = opts->sj_count > 0 ? opts->sj_begin : 0;
  const int n_sj = opts->sj_count > 0 ? opts->sj_count : S;
  if (sj0 < 0 || sj0 + n_sj > S) return set_err(RT_ERR_INVALID_ARG, "bad stratum range");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)opts->n_rows * W;
  if (n_px == 0) return RT_OK;
  std::unique_lock<std::mutex> lock(sc->mu);
  hipStream_t stream = (hipStream_t)stream_v;
  HIP_TRY(hipSetDevice(sc->device));
  // the pass needs no queue word and no workspace, but a slot gives it the scene's ordering and
  // lifetime rules (and the stats events) as any render has them
  SlotHold hold{sc, lock};
  {
    const int rc = acquire_slot(sc, lock, stream, &hold.sl);
    if (rc != RT_OK) return rc;
  }
  RenderSlot* const sl = hold.sl;
  TraceParams P;
  std::memset(&P, 0, sizeof(P));
  P.nodes = sc->nodes;
  P.mats = sc->mats;
  P.texs = sc->texs;
  P.perlin = sc->perlin;
  P.lights = sc->lights;
  P.light_offs = sc->light_offs;
  P.texels = sc->texels;
  P.root = sc->hdr.root;
  P.sphere_light0 = -1;
  // RT_FLAG_INTERPRETER / RT_FLAG_SEMANTICS_REFERENCE change no first hit; the kernel reads
  // RT_FLAG_REFERENCE_BVH (the walker) and RT_FLAG_OVERWRITE
  P.flags = opts->flags;
  const bool bvh = sc->hdr.has_bvh != 0;
  // the interpreter's plan: the walker reads the staged tables, the compact BVHs and its per-lane
  // stacks where plan_lds put them, at the workgroup size the plan assumes
  const LdsPlan LP = plan_lds(sc->hdr, sc->o_perl, opts->flags, false, sc->lds_module_max);
  const int block = LP.block;
  P.stage_scene = LP.stage_scene;
  P.n_perlin_lds = LP.n_perlin_lds;
  P.stage_src = LP.stage_scene ? sc->dev : sc->perlin;
  P.stage_bytes = LP.stage_bytes;
  P.bvh_words = sc->hdr.bvh_words;
  P.cbvh_src = (const uint8_t*)(sc->nodes + sc->hdr.cbvh_word0);
  P.cbvh_bytes = LP.cbvh_bytes;
  P.cbvh_lds_off = LP.cbvh_lds_off;
  P.stack_lds_off = LP.stack_lds_off;
  P.bvh_lds_words = LP.bvh_lds_words;
  P.bvh_lds_off = LP.bvh_lds_off;
  P.row_lds_off = LP.row_lds_off;
  P.o_mats = sc->o_mats;
  P.o_texs = sc->o_texs;
  P.o_lights = sc->o_lights;
  P.o_loffs = sc->o_loffs;
  P.o_perl = sc->o_perl;
  const size_t lds_bytes = LP.lds_bytes;
  for (int k = 0; k < 3; ++k) {
    P.center[k] = cam->center[k];
    P.p00[k] = cam->pixel00_loc[k];
    P.du[k] = cam->pixel_delta_u[k];
    P.dv[k] = cam->pixel_delta_v[k];
    P.ddu[k] = cam->defocus_disk_u[k];
    P.ddv[k] = cam->defocus_disk_v[k];
    P.bg[k] = cam->background[k];
    P.bg_w[k] = (float)cam->background[k];  // the f32 weight the path kernel multiplies by
  }
  P.rs = cam->recip_sqrt_spp;
  P.defocus = cam->defocus_angle > 0.0;
  P.W = W;
  P.n_rows = opts->n_rows;
  P.row_begin = opts->row_begin;
  P.row_step = opts->row_step;
  P.sqrt_spp = S;
  P.sj0 = sj0;
  P.n_sj = n_sj;
  P.seed_lo = (uint32_t)opts->seed;
  P.seed_hi = (uint32_t)(opts->seed >> 32);
  P.tiles_x = (W + kWaveTile - 1) / kWaveTile;
  const int n_tiles = P.tiles_x * ((opts->n_rows + kWaveTile - 1) / kWaveTile);
  typedef void (*kern_t)(TraceParams, float*);
  // [bvh], [staged] (no BVH, the small tables in LDS), [nested volumes][bvh]
  static const kern_t table[5] = {rt_aov<false, false, 0>, rt_aov<true, false, 0>,
                                  rt_aov<false, true, 0>, rt_aov<false, false, RTL_VOLUME_NEST>,
                                  rt_aov<true, false, RTL_VOLUME_NEST>};
  const bool staged = !bvh && P.stage_scene && !sc->hdr.nested_volumes;
  const int kslot = sc->hdr.nested_volumes ? 3 + (bvh ? 1 : 0) : (staged ? 2 : (bvh ? 1 : 0));
  const kern_t kern = table[kslot];
  if (lds_bytes > (64u << 10))
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes));
  // a dispatch the hardware cannot place aborts the whole queue: ask first
  if (sc->aov_resident[kslot] == 0 || sc->aov_resident_lds[kslot] != lds_bytes) {
    int nb = 0;
    const hipError_t oe =
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)kern, block, lds_bytes);
    if (oe != hipSuccess || nb <= 0)
      return set_err(RT_ERR_HIP, std::string("occupancy query: the AOV kernel does not fit a CU (") +
                                     (oe != hipSuccess ? hipGetErrorString(oe) : "0 blocks") + ")");
    sc->aov_resident[kslot] = nb;
    sc->aov_resident_lds[kslot] = lds_bytes;
  }
  hold.stream = stream;
  hold.enqueued = true;  // from here on a failure still records `done` (SlotHold)
  if (stats) HIP_TRY(hipEventRecord(sl->ev0, stream));
  const int tiles_per_block = block / 64;
  const unsigned blocks = (unsigned)((n_tiles + tiles_per_block - 1) / tiles_per_block);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(block), lds_bytes, stream, P, aov);
  HIP_TRY(hipGetLastError());
  if (stats) HIP_TRY(hipEventRecord(sl->ev1, stream));
  HIP_TRY(hipEventRecord(sl->done, stream));
  sl->recorded = true;
  sl->last_stream = stream;
  hold.finished = true;
  if (stats) {
    lock.unlock();  // the slot stays held: other renders of the scene go on meanwhile
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, sl->ev0, sl->ev1));
    stats->ms_kernel = ms;
    stats->samples = (uint64_t)n_px * (uint64_t)n_sj * (uint64_t)S;
    stats->out_bytes = (uint64_t)n_px * RT_AOV_CHANNELS * sizeof(float);
    stats->launches = 1;
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return RT_OK;
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
