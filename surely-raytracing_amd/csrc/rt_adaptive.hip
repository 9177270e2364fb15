// rt_adaptive.hip — adaptive sampling over the sample moments (include/rt_mi355x.h): the pass
// schedule, the per-tile error and resolve kernels, the rt_adaptive handle and the driver that
// loops rt_render_tiles_device (rt_device.hip) over the tiles that have not converged. Its own
// translation unit; of scenes it knows only the C ABI.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "rt_mi355x.h"
#include "rt_stage.hpp"

using rts::set_err;
using rts::time_point;

// The workspace holds, per tile, rows_held (u32), the error (f32) and the invalid pixels (u32).
// The host copy of rows_held that an asynchronous resolve uploads from is rewritten only after
// `done`. Not timed: the driver's stats are the renders'.
struct rt_adaptive : rts::Stage {
  std::vector<uint32_t> rows_host;
  std::vector<uint32_t> back;  // the error and invalid counts as downloaded
};

namespace {

constexpr int kTile = 8;  // the path kernel's 8x8 wave tile (rt_kernel.h kWaveTile)

// One wave per tile, lane = pixel of the tile (rt_reduce's mapping). err[tile] and inv[tile] are
// written by lane 0 of the tile's wave alone; no atomics.
__global__ __launch_bounds__(256) void ad_tile_error(const float* __restrict__ accum,
                                                     const float* __restrict__ m2,
                                                     const uint32_t* __restrict__ rows,
                                                     float* __restrict__ err,
                                                     uint32_t* __restrict__ inv, int W, int H,
                                                     int tiles_x, int n_tiles, int S, double floor) {
  const int tile = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const int pv = threadIdx.x & 63;
  if (tile >= n_tiles) return;  // wave-uniform
  const uint32_t nr = rows[tile];
  if (nr < 2u) {
    if (pv == 0) err[tile] = __builtin_inff(), inv[tile] = 0u;
    return;
  }
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int tile_w = min(kTile, W - tx * kTile), tile_h = min(kTile, H - ty * kTile);
  const bool in = pv < tile_w * tile_h;
  float e32 = 0.f;
  bool bad = false;
  if (in) {
    const int x = tx * kTile + pv % tile_w, y = ty * kTile + pv / tile_w;
    const size_t i = ((size_t)y * W + x) * 3;
    const double n = (double)nr, B = n * (double)S;
    const double k = n / ((n - 1.0) * (B * B));
    double var = 0.0, mean = floor;
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double s = (double)accum[i + c], q = (double)m2[i + c];
      fin = fin && isfinite(s) && isfinite(q);
      var += fmax(0.0, q - s * s / n) * k;
      mean += fmax(s, 0.0) / B;
    }
    const double e = sqrt(var) / mean;
    bad = !fin || !isfinite(e);
    if (!bad) e32 = (float)e;
  }
  const unsigned long long bads = __ballot(bad);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) e32 = fmaxf(e32, __shfl_xor(e32, o, 64));
  if (pv == 0) err[tile] = e32, inv[tile] = (uint32_t)__popcll(bads);
}

// One lane per pixel. out may be accum: each lane reads its pixel before it writes it.
__global__ __launch_bounds__(256) void ad_resolve(const float* accum,
                                                  const uint32_t* __restrict__ rows, float* out,
                                                  float* __restrict__ samples, int W, int H,
                                                  int tiles_x, int S) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)W * H) return;
  const int x = (int)(p % W), y = (int)(p / W);
  const uint32_t nr = rows[(y / kTile) * tiles_x + x / kTile];
  const double B = (double)nr * (double)S;
  const float a0 = accum[3 * p], a1 = accum[3 * p + 1], a2 = accum[3 * p + 2];
  if (nr == (uint32_t)S) {  // every row held: the sums as they are, bit for bit
    out[3 * p] = a0, out[3 * p + 1] = a1, out[3 * p + 2] = a2;
  } else {
    const double f = ((double)S * (double)S) / B;
    out[3 * p] = (float)((double)a0 * f);
    out[3 * p + 1] = (float)((double)a1 * f);
    out[3 * p + 2] = (float)((double)a2 * f);
  }
  if (samples) samples[p] = (float)B;
}

int check_frame(int width, int height, int sqrt_spp) {
  if (width <= 0 || height < 0)
    return set_err(RT_ERR_INVALID_ARG, "bad frame size (width <= 0 or height < 0)");
  if ((int64_t)width * height >= (1ll << 31))
    return set_err(RT_ERR_INVALID_ARG, "frame too large (width * height >= 2^31)");
  if (sqrt_spp < 1 || sqrt_spp > 32768) return set_err(RT_ERR_INVALID_ARG, "bad sqrt_spp");
  return RT_OK;
}

int check_rows(const uint32_t* rows, size_t n_tiles, uint32_t lo, int sqrt_spp) {
  for (size_t t = 0; t < n_tiles; ++t)
    if (rows[t] < lo || rows[t] > (uint32_t)sqrt_spp)
      return set_err(RT_ERR_INVALID_ARG, "rows_held outside the stratum rows of sqrt_spp");
  return RT_OK;
}

size_t tile_count(int width, int height) {
  return (size_t)((width + kTile - 1) / kTile) * (size_t)((height + kTile - 1) / kTile);
}

// rows_held into the handle's host copy and workspace (ad->mu held): both may still be in use by
// the handle's previous call, which `done` follows. The wait for it is the host's, not the
// stream's (so the callers' Run needs no begin()): the host vector is reused.
int upload_rows(rt_adaptive* ad, const uint32_t* rows, size_t n_tiles, hipStream_t stream) {
  HIP_TRY(hipSetDevice(ad->device));
  if (ad->recorded) HIP_TRY(hipEventSynchronize(ad->done));
  RT_TRY(ad->reserve(n_tiles * 12));
  ad->rows_host.assign(rows, rows + n_tiles);
  HIP_TRY(hipMemcpyAsync(ad->work, ad->rows_host.data(), n_tiles * 4, hipMemcpyHostToDevice, stream));
  return RT_OK;
}

// rt_adaptive_tile_error with the arguments checked and ad->mu held
int tile_error_locked(rt_adaptive* ad, int W, int H, int S, double floor, const float* accum,
                      const float* m2, const uint32_t* rows, float* err_out, uint64_t* n_invalid,
                      hipStream_t stream) {
  const size_t n_tiles = tile_count(W, H);
  if (n_invalid) *n_invalid = 0;
  if (n_tiles == 0) return RT_OK;
  const int rc = upload_rows(ad, rows, n_tiles, stream);
  if (rc != RT_OK) return rc;
  {
    rts::Run run(*ad, stream);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(ad->work);
    float* d_err = reinterpret_cast<float*>(ad->work + n_tiles * 4);
    uint32_t* d_inv = reinterpret_cast<uint32_t*>(ad->work + n_tiles * 8);
    hipLaunchKernelGGL(ad_tile_error, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, stream,
                       accum, m2, d_rows, d_err, d_inv, W, H, (W + kTile - 1) / kTile, (int)n_tiles,
                       S, floor);
    HIP_TRY(hipGetLastError());
    ad->back.resize(2 * n_tiles);
    HIP_TRY(hipMemcpyAsync(ad->back.data(), d_err, n_tiles * 8, hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(err_out, ad->back.data(), n_tiles * 4);
  if (n_invalid)
    for (size_t t = 0; t < n_tiles; ++t) *n_invalid += ad->back[n_tiles + t];
  return RT_OK;
}

// rt_adaptive_resolve_device with the arguments checked and ad->mu held (out may be null when
// only the sample counts are wanted: the driver)
int resolve_locked(rt_adaptive* ad, int W, int H, int S, const uint32_t* rows, const float* accum,
                   float* out, float* samples, hipStream_t stream) {
  const size_t n_tiles = tile_count(W, H);
  if (n_tiles == 0) return RT_OK;
  const int rc = upload_rows(ad, rows, n_tiles, stream);
  if (rc != RT_OK) return rc;
  rts::Run run(*ad, stream);
  const size_t n_px = (size_t)W * H;
  hipLaunchKernelGGL(ad_resolve, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream, accum,
                     reinterpret_cast<const uint32_t*>(ad->work), out, samples, W, H,
                     (W + kTile - 1) / kTile, S);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_adaptive_schedule(int sqrt_spp, int passes, int pass, int* sj_begin, int* sj_step,
                         int* sj_count) {
  if (!sj_begin || !sj_step || !sj_count) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (sqrt_spp < 2 || passes < 1 || passes > sqrt_spp / 2 || pass < 0 || pass >= passes)
    return set_err(RT_ERR_INVALID_ARG, "schedule: 1 <= passes <= sqrt_spp / 2, 0 <= pass < passes");
  *sj_begin = pass;
  *sj_step = passes;
  *sj_count = (sqrt_spp - pass + passes - 1) / passes;  // rows pass, pass + P, ... below sqrt_spp
  return RT_OK;
}

int rt_adaptive_create(int device, rt_adaptive** out) {
  return rts::stage_create(device, false, out);
}

void rt_adaptive_destroy(rt_adaptive* ad) { rts::stage_destroy(ad); }

int rt_adaptive_tile_error(rt_adaptive* ad, int width, int height, int sqrt_spp, double floor,
                           const float* accum, const float* m2, const uint32_t* rows_held,
                           float* err_out, uint64_t* n_invalid_out, void* stream_v) {
  if (!ad || !accum || !m2 || !rows_held || !err_out)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  int rc = check_frame(width, height, sqrt_spp);
  if (rc != RT_OK) return rc;
  if (!std::isfinite(floor) || floor <= 0.0)
    return set_err(RT_ERR_INVALID_ARG, "floor must be finite and > 0");
  rc = check_rows(rows_held, tile_count(width, height), 0u, sqrt_spp);
  if (rc != RT_OK) return rc;
  std::lock_guard<std::mutex> lock(ad->mu);
  return tile_error_locked(ad, width, height, sqrt_spp, floor, accum, m2, rows_held, err_out,
                           n_invalid_out, (hipStream_t)stream_v);
}

int rt_adaptive_resolve_device(rt_adaptive* ad, int width, int height, int sqrt_spp,
                               const uint32_t* rows_held, const float* accum, float* out,
                               float* samples, void* stream_v) {
  if (!ad || !rows_held || !accum || !out) return set_err(RT_ERR_INVALID_ARG, "null argument");
  int rc = check_frame(width, height, sqrt_spp);
  if (rc != RT_OK) return rc;
  rc = check_rows(rows_held, tile_count(width, height), 1u, sqrt_spp);
  if (rc != RT_OK) return rc;
  std::lock_guard<std::mutex> lock(ad->mu);
  return resolve_locked(ad, width, height, sqrt_spp, rows_held, accum, out, samples,
                        (hipStream_t)stream_v);
}

int rt_render_adaptive_device(rt_adaptive* ad, rt_scene* sc, const rt_camera* cam,
                              const rt_render_opts* opts, const rt_adaptive_params* ap,
                              float* accum, float* m2, float* out, float* samples,
                              uint32_t* rows_held_out, uint32_t* tiles_per_pass, void* stream_v,
                              rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  if (!ad || !sc || !cam || !opts || !ap || !accum || !m2)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  const int W = cam->image_width, H = opts->n_rows, S = cam->sqrt_spp;
  int rc = check_frame(W, H, S);
  if (rc != RT_OK) return rc;
  if (ap->passes < 1 || ap->passes > S / 2 || ap->min_passes < 1 || ap->min_passes > ap->passes)
    return set_err(RT_ERR_INVALID_ARG, "adaptive: 1 <= min_passes <= passes <= sqrt_spp / 2");
  if (std::isnan(ap->threshold)) return set_err(RT_ERR_INVALID_ARG, "adaptive: NaN threshold");
  if (!std::isfinite(ap->floor) || ap->floor <= 0.0)
    return set_err(RT_ERR_INVALID_ARG, "floor must be finite and > 0");
  if (opts->sj_begin != 0 || opts->sj_count != 0)
    return set_err(RT_ERR_INVALID_ARG, "adaptive: sj_begin and sj_count must be 0 (the passes pick the rows)");
  if (!(opts->flags & RT_FLAG_OVERWRITE) || (opts->flags & RT_FLAG_COUNT_OPS))
    return set_err(RT_ERR_INVALID_ARG, "adaptive: RT_FLAG_OVERWRITE must be set, RT_FLAG_COUNT_OPS clear");
  if (H > rts::kRowsPerCall) return set_err(RT_ERR_UNSUPPORTED, "adaptive: n_rows > 32760");
  const int P = ap->passes;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (tiles_per_pass) std::memset(tiles_per_pass, 0, sizeof(uint32_t) * (size_t)P);
  const size_t n_tiles = tile_count(W, H);
  if (n_tiles == 0) return RT_OK;
  hipStream_t stream = (hipStream_t)stream_v;
  std::lock_guard<std::mutex> lock(ad->mu);
  std::vector<uint32_t> active(n_tiles), held(n_tiles, 0u), next;
  for (size_t t = 0; t < n_tiles; ++t) active[t] = (uint32_t)t;
  std::vector<float> err(n_tiles);
  rt_stats sum{}, part{};
  for (int p = 0; p < P && !active.empty(); ++p) {
    rt_render_opts o = *opts;
    int step = 1;
    rc = rt_adaptive_schedule(S, P, p, &o.sj_begin, &step, &o.sj_count);
    if (rc != RT_OK) return rc;
    if (p > 0) o.flags &= ~RT_FLAG_OVERWRITE;
    // with stats the call returns when the pass is complete: the error kernel reads its sums
    rc = rt_render_tiles_device(sc, cam, &o, active.data(), (uint32_t)active.size(), step, accum, m2,
                                stream_v, &part);
    if (rc != RT_OK) return rc;
    sum.ms_kernel += part.ms_kernel;
    sum.samples += part.samples;
    sum.out_bytes += part.out_bytes;
    sum.launches += part.launches;
    if (tiles_per_pass) tiles_per_pass[p] = (uint32_t)active.size();
    for (uint32_t t : active) held[t] += (uint32_t)o.sj_count;
    if (p + 1 >= ap->min_passes && p + 1 < P) {
      rc = tile_error_locked(ad, W, H, S, ap->floor, accum, m2, held.data(), err.data(), nullptr,
                             stream);
      if (rc != RT_OK) return rc;
      next.clear();
      for (uint32_t t : active)
        if (err[t] > ap->threshold) next.push_back(t);  // ascending as `active` is
      active.swap(next);
    }
  }
  if (out || samples) {
    // samples alone: the resolve kernel still writes an image, into the scaled sums' place
    if (!out) return set_err(RT_ERR_INVALID_ARG, "adaptive: samples_dev needs out_dev");
    rc = resolve_locked(ad, W, H, S, held.data(), accum, out, samples, stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
  }
  if (rows_held_out) std::memcpy(rows_held_out, held.data(), n_tiles * sizeof(uint32_t));
  if (stats) {
    sum.ms_total = rts::ms_since(t0);
    *stats = sum;
  }
  return RT_OK;
}

int rt_render_adaptive(rt_adaptive* ad, rt_scene* sc, const rt_camera* cam,
                       const rt_render_opts* opts, const rt_adaptive_params* ap, float* accum,
                       float* m2, float* out, float* samples, uint32_t* rows_held_out,
                       uint32_t* tiles_per_pass, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  if (!ad || !sc || !cam || !opts || !ap || !accum || !m2)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (cam->image_width <= 0 || opts->n_rows < 0) return set_err(RT_ERR_INVALID_ARG, "bad size");
  if (samples && !out) return set_err(RT_ERR_INVALID_ARG, "adaptive: samples needs out");
  const size_t n_px = (size_t)cam->image_width * (size_t)opts->n_rows;
  // the sums, the second moments, the resolved frame, the sample counts
  const size_t b3 = n_px * 3 * sizeof(float);
  rts::Staging st;
  const int i_acc = st.add(b3), i_m2 = st.add(b3), i_out = st.add_if(out != nullptr, b3);
  const int i_smp = st.add_if(samples != nullptr, n_px * sizeof(float));
  RT_TRY(st.alloc(ad->device));
  RT_TRY(rt_render_adaptive_device(ad, sc, cam, opts, ap, st.ptr<float>(i_acc), st.ptr<float>(i_m2),
                                   st.ptr<float>(i_out), st.ptr<float>(i_smp), rows_held_out,
                                   tiles_per_pass, nullptr, stats));
  RT_TRY(st.download(i_acc, accum));
  RT_TRY(st.download(i_m2, m2));
  RT_TRY(st.download(i_out, out));
  RT_TRY(st.download(i_smp, samples));
  if (stats) stats->ms_total = rts::ms_since(t0);
  return RT_OK;
}

}  // extern "C"
