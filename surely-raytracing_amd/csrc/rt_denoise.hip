// rt_denoise.hip — the edge-avoiding a-trous denoiser of include/rt_mi355x.h: the dn_prepare /
// dn_atrous kernels (body in rt_denoise.h) and the rt_denoise* entry points. Its own translation
// unit, built beside rt_device.hip and rt_aov.hip; it knows nothing of scenes.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>

#include "rt_mi355x.h"
#include "rt_denoise.h"
#include "rt_denoise_var.h"
#include "rt_scene_impl.hpp"  // set_err, HIP_TRY

using namespace rtd;
using rts::set_err;

// One workspace and one ordering event per handle. `mu` serialises the calls; every call's stream
// waits for `done` of the call before it (whatever stream that went to), so the workspace is never
// shared by two calls in flight.
struct rt_denoiser {
  int device = 0;
  uint8_t* work = nullptr;
  size_t work_bytes = 0;
  hipEvent_t done = nullptr, ev0 = nullptr, ev1 = nullptr;
  bool recorded = false;  // `done` has been recorded at least once
  std::mutex mu;
};

namespace {

__global__ __launch_bounds__(kBlock) void dn_prepare(DnParams P, const float* __restrict__ beauty,
                                                     const float* __restrict__ aov,
                                                     float4* __restrict__ G0,
                                                     float4* __restrict__ G1,
                                                     float4* __restrict__ X) {
  prepare_body(P, beauty, aov, G0, G1, X);
}

// FINAL: the last level, fused with the re-modulation and the store to the user's buffer (`out`
// may be `beauty`: each lane reads its own beauty pixel before it writes it)
template <bool FINAL>
__global__ __launch_bounds__(kBlock) void dn_atrous(DnParams P, const float4* __restrict__ G0,
                                                    const float4* __restrict__ G1,
                                                    const float4* __restrict__ Xin, float4* Xout,
                                                    const float* beauty,
                                                    const float* __restrict__ aov, float* out) {
  atrous_body<FINAL>(P, G0, G1, Xin, Xout, beauty, aov, out);
}

// the levels of step 1 and 2 with their records staged in LDS (atrous_tiled_body)
template <int STEP, bool FINAL>
__global__ __launch_bounds__(kBlock) void dn_atrous_tiled(DnParams P, const float4* __restrict__ G0,
                                                          const float4* __restrict__ G1,
                                                          const float4* __restrict__ Xin,
                                                          float4* Xout, const float* beauty,
                                                          const float* __restrict__ aov,
                                                          float* out) {
  __shared__ TileLds<STEP> L;
  atrous_tiled_body<STEP, FINAL>(P, L, G0, G1, Xin, Xout, beauty, aov, out);
}

// The variance-guided filter (rt_denoise_var.h): its own prepare, the 3x3 variance prefilter and
// the three level forms with the variance lane, beside the plain filter's kernels.
__global__ __launch_bounds__(kBlock) void dn_prepare_var(DnVarParams V,
                                                         const float* __restrict__ beauty,
                                                         const float* __restrict__ m2,
                                                         const float* __restrict__ aov,
                                                         float4* __restrict__ G0,
                                                         float4* __restrict__ G1,
                                                         float4* __restrict__ X) {
  prepare_var_body(V, beauty, m2, aov, G0, G1, X);
}

__global__ __launch_bounds__(kBlock) void dn_prefilter_var(DnParams P,
                                                           const float4* __restrict__ G1,
                                                           const float4* __restrict__ Xin,
                                                           float4* __restrict__ Xout) {
  prefilter_body(P, G1, Xin, Xout);
}

template <bool FINAL>
__global__ __launch_bounds__(kBlock) void dn_atrous_var(DnParams P, const float4* __restrict__ G0,
                                                        const float4* __restrict__ G1,
                                                        const float4* __restrict__ Xin,
                                                        float4* Xout, const float* beauty,
                                                        const float* __restrict__ aov, float* out,
                                                        float* var_out) {
  atrous_var_body<FINAL>(P, G0, G1, Xin, Xout, beauty, aov, out, var_out);
}

template <int STEP, bool FINAL>
__global__ __launch_bounds__(kBlock) void dn_atrous_var_tiled(
    DnParams P, const float4* __restrict__ G0, const float4* __restrict__ G1,
    const float4* __restrict__ Xin, float4* Xout, const float* beauty,
    const float* __restrict__ aov, float* out, float* var_out) {
  __shared__ TileLds<STEP> L;
  atrous_var_tiled_body<STEP, FINAL>(P, L, G0, G1, Xin, Xout, beauty, aov, out, var_out);
}

// bytes of workspace per pixel: G0, G1 and the two colour records the levels alternate between
// (a single level reads one and writes the user's buffer)
size_t work_per_pixel(int levels) { return levels > 1 ? 64 : 48; }

// Everything that can be refused without reading the handle or touching HIP.
int check_params(const rt_denoise_params* p) {
  if (p->width <= 0 || p->height < 0)
    return set_err(RT_ERR_INVALID_ARG, "bad frame size (width <= 0 or height < 0)");
  if ((int64_t)p->width * p->height >= (1ll << 31))
    return set_err(RT_ERR_INVALID_ARG, "frame too large (width * height >= 2^31)");
  if (p->levels < 1 || p->levels > RT_DENOISE_MAX_LEVELS)
    return set_err(RT_ERR_INVALID_ARG, "levels outside 1..RT_DENOISE_MAX_LEVELS");
  if (p->flags & ~RT_DENOISE_DEMODULATE)
    return set_err(RT_ERR_INVALID_ARG, "unknown RT_DENOISE_* flag bits");
  if (!std::isfinite(p->beauty_samples) || p->beauty_samples <= 0.0 ||
      !std::isfinite(p->aov_samples) || p->aov_samples <= 0.0)
    return set_err(RT_ERR_INVALID_ARG, "sample counts must be finite and > 0");
  if (!std::isfinite(p->sigma_color) || !std::isfinite(p->sigma_normal) ||
      !std::isfinite(p->sigma_depth) || !std::isfinite(p->sigma_albedo))
    return set_err(RT_ERR_INVALID_ARG, "non-finite sigma");
  return RT_OK;
}

int check_args(const rt_denoiser* dn, const rt_denoise_params* p, const float* beauty,
               const float* aov, const float* out) {
  if (!dn || !p || !beauty || !aov || !out) return set_err(RT_ERR_INVALID_ARG, "null argument");
  return check_params(p);
}

// rt_denoise_var*: the shared fields as rt_denoise's, then its own
int check_var_args(const rt_denoiser* dn, const rt_denoise_var_params* p, const float* beauty,
                   const float* m2, const float* aov, const float* out) {
  if (!dn || !p || !beauty || !m2 || !aov || !out)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  rt_denoise_params q;
  std::memset(&q, 0, sizeof(q));
  q.width = p->width;
  q.height = p->height;
  q.levels = p->levels;
  q.flags = p->flags;
  q.beauty_samples = p->beauty_samples;
  q.aov_samples = p->aov_samples;
  q.sigma_color = p->sigma_color;
  q.sigma_normal = p->sigma_normal;
  q.sigma_depth = p->sigma_depth;
  q.sigma_albedo = p->sigma_albedo;
  const int rc = check_params(&q);
  if (rc != RT_OK) return rc;
  if (p->beauty_rows < 2)
    return set_err(RT_ERR_INVALID_ARG, "beauty_rows < 2 (the between-row estimate needs two rows)");
  if (p->_pad0 != 0) return set_err(RT_ERR_INVALID_ARG, "_pad0 must be 0");
  return RT_OK;
}

// log2(e) / sigma^2 (the kernel evaluates exp2 of the summed exponent); 0 switches the term off
float term_scale(double sigma) {
  return sigma > 0.0 ? (float)(1.4426950408889634 / (sigma * sigma)) : 0.f;
}

// Records `done` after whatever a failing call has enqueued, so that the next call still waits
// for the kernels that may be using the workspace.
struct DoneGuard {
  rt_denoiser* dn;
  hipStream_t stream;
  bool enqueued = false, finished = false;
  ~DoneGuard() {
    if (!enqueued || finished) return;
    if (hipEventRecord(dn->done, stream) == hipSuccess)
      dn->recorded = true;
    else
      (void)hipStreamSynchronize(stream);
  }
};

}  // namespace

extern "C" {

int rt_denoise_default_params(int width, int height, double beauty_samples, double aov_samples,
                              rt_denoise_params* out) {
  if (!out) return set_err(RT_ERR_INVALID_ARG, "null out");
  rt_denoise_params p;
  std::memset(&p, 0, sizeof(p));
  p.width = width;
  p.height = height;
  p.levels = 5;
  p.flags = RT_DENOISE_DEMODULATE;
  p.beauty_samples = beauty_samples;
  p.aov_samples = aov_samples;
  p.sigma_color = 4.0f;
  p.sigma_normal = 0.3f;
  p.sigma_depth = 0.1f;
  p.sigma_albedo = 0.1f;
  const int rc = check_params(&p);
  if (rc != RT_OK) return rc;
  *out = p;
  return RT_OK;
}

int rt_denoiser_create(int device, rt_denoiser** out) {
  if (!out) return set_err(RT_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_err(RT_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return set_err(RT_ERR_INVALID_ARG, "bad device ordinal");
  HIP_TRY(hipSetDevice(device));
  rt_denoiser* dn = new rt_denoiser;
  dn->device = device;
  hipError_t e = hipEventCreateWithFlags(&dn->done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreate(&dn->ev0);
  if (e == hipSuccess) e = hipEventCreate(&dn->ev1);
  if (e != hipSuccess) {
    rt_denoiser_destroy(dn);
    return set_err(RT_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
  }
  *out = dn;
  return RT_OK;
}

void rt_denoiser_destroy(rt_denoiser* dn) {
  if (!dn) return;
  {
    std::lock_guard<std::mutex> lock(dn->mu);
    (void)hipSetDevice(dn->device);
    if (dn->recorded) (void)hipEventSynchronize(dn->done);
    if (dn->work) (void)hipFree(dn->work);
    if (dn->done) (void)hipEventDestroy(dn->done);
    if (dn->ev0) (void)hipEventDestroy(dn->ev0);
    if (dn->ev1) (void)hipEventDestroy(dn->ev1);
  }
  delete dn;
}

int rt_denoise_device(rt_denoiser* dn, const rt_denoise_params* p, const float* beauty,
                      const float* aov, float* out, void* stream_v, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  {
    const int rc = check_args(dn, p, beauty, aov, out);
    if (rc != RT_OK) return rc;
  }
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  if (n_px == 0) return RT_OK;
  hipStream_t stream = (hipStream_t)stream_v;
  // held to the end of the call, through the synchronisation a stats call asks for: the stats
  // events are the handle's
  std::lock_guard<std::mutex> lock(dn->mu);
  HIP_TRY(hipSetDevice(dn->device));
  const size_t need = n_px * work_per_pixel(p->levels);
  if (need > dn->work_bytes) {
    // the previous call may still be reading the old workspace
    if (dn->recorded) HIP_TRY(hipEventSynchronize(dn->done));
    if (dn->work) HIP_TRY(hipFree(dn->work));
    dn->work = nullptr;
    dn->work_bytes = 0;
    HIP_TRY(hipMalloc((void**)&dn->work, need));
    dn->work_bytes = need;
  }
  if (dn->recorded) HIP_TRY(hipStreamWaitEvent(stream, dn->done, 0));
  float4* const G0 = reinterpret_cast<float4*>(dn->work);
  float4* const G1 = G0 + n_px;
  float4* const Xa = G1 + n_px;
  float4* const Xb = Xa + n_px;  // touched only when levels > 1
  DnParams P;
  std::memset(&P, 0, sizeof(P));
  P.W = p->width;
  P.H = p->height;
  P.step = 1;
  P.flags = p->flags;
  P.B = (float)p->beauty_samples;
  P.A = (float)p->aov_samples;
  P.k_normal = term_scale(p->sigma_normal);
  P.k_depth = term_scale(p->sigma_depth);
  P.k_albedo = term_scale(p->sigma_albedo);
  const unsigned tiles_x = ((unsigned)P.W + kTileW - 1) / kTileW;
  const unsigned tiles_y = ((unsigned)P.H + kTileH - 1) / kTileH;
  const dim3 grid(tiles_x * tiles_y), block(kBlock);  // W * H < 2^31: fewer than 2^28 + W + H tiles
  DoneGuard guard{dn, stream};
  guard.enqueued = true;
  if (stats) HIP_TRY(hipEventRecord(dn->ev0, stream));
  hipLaunchKernelGGL(dn_prepare, grid, block, 0, stream, P, beauty, aov, G0, G1, Xa);
  HIP_TRY(hipGetLastError());
  float4 *xin = Xa, *xout = Xb;
  for (int k = 0; k < p->levels; ++k) {
    P.step = 1 << k;
    P.k_color = term_scale((double)p->sigma_color / (double)(1 << k));  // sigma_c * 2^-k
    typedef void (*kern_t)(DnParams, const float4*, const float4*, const float4*, float4*,
                           const float*, const float*, float*);
    const bool last = k + 1 == p->levels;
    kern_t kern = last ? dn_atrous<true> : dn_atrous<false>;
    // steps 1 and 2 from LDS tiles (measured faster than the direct kernel; at step 4 the halo
    // outgrows the tile and the tiled form measured no faster: DESIGN.md §4.2c)
    if (k == 0) kern = last ? dn_atrous_tiled<1, true> : dn_atrous_tiled<1, false>;
    if (k == 1) kern = last ? dn_atrous_tiled<2, true> : dn_atrous_tiled<2, false>;
    hipLaunchKernelGGL(kern, grid, block, 0, stream, P, G0, G1, xin, xout, beauty, aov, out);
    HIP_TRY(hipGetLastError());
    std::swap(xin, xout);
  }
  if (stats) HIP_TRY(hipEventRecord(dn->ev1, stream));
  HIP_TRY(hipEventRecord(dn->done, stream));
  dn->recorded = true;
  guard.finished = true;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, dn->ev0, dn->ev1));
    stats->ms_kernel = ms;
    stats->samples = n_px;
    stats->out_bytes = (uint64_t)n_px * 3 * sizeof(float);
    stats->launches = 1u + (uint32_t)p->levels;
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return RT_OK;
}

int rt_denoise(rt_denoiser* dn, const rt_denoise_params* p, const float* beauty, const float* aov,
               float* out, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  {
    const int rc = check_args(dn, p, beauty, aov, out);
    if (rc != RT_OK) return rc;
  }
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  if (n_px == 0) return RT_OK;
  const size_t b_bytes = n_px * 3 * sizeof(float), a_bytes = n_px * RT_AOV_CHANNELS * sizeof(float);
  HIP_TRY(hipSetDevice(dn->device));
  // one allocation: the beauty frame (denoised in place), then the AOVs
  uint8_t* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, b_bytes + a_bytes));
  float* const d_beauty = reinterpret_cast<float*>(d);
  float* const d_aov = reinterpret_cast<float*>(d + b_bytes);
  int rc = RT_OK;
  hipError_t e = hipMemcpy(d_beauty, beauty, b_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_aov, aov, a_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("upload: ") + hipGetErrorString(e));
  rt_stats local;
  if (rc == RT_OK)
    rc = rt_denoise_device(dn, p, d_beauty, d_aov, d_beauty, nullptr, stats ? stats : &local);
  if (rc == RT_OK) {
    e = hipMemcpy(out, d_beauty, b_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("download: ") + hipGetErrorString(e));
  }
  (void)hipFree(d);
  if (rc == RT_OK && stats)
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int rt_denoise_var_default_params(int width, int height, double beauty_samples, int beauty_rows,
                                  double aov_samples, rt_denoise_var_params* out) {
  if (!out) return set_err(RT_ERR_INVALID_ARG, "null out");
  rt_denoise_var_params p;
  std::memset(&p, 0, sizeof(p));
  p.width = width;
  p.height = height;
  p.levels = 5;
  p.flags = RT_DENOISE_DEMODULATE;
  p.beauty_samples = beauty_samples;
  p.aov_samples = aov_samples;
  p.beauty_rows = beauty_rows;
  p.sigma_color = 4.0f;  // measured: DESIGN.md §4.2d
  p.sigma_normal = 0.3f;
  p.sigma_depth = 0.1f;
  p.sigma_albedo = 0.1f;
  const float one = 1.f;  // any non-null pointers: only the params are looked at
  const int rc = check_var_args(reinterpret_cast<const rt_denoiser*>(&one), &p, &one, &one, &one, &one);
  if (rc != RT_OK) return rc;
  *out = p;
  return RT_OK;
}

int rt_denoise_var_device(rt_denoiser* dn, const rt_denoise_var_params* p, const float* beauty,
                          const float* m2, const float* aov, float* out, float* var_out,
                          void* stream_v, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  {
    const int rc = check_var_args(dn, p, beauty, m2, aov, out);
    if (rc != RT_OK) return rc;
  }
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  if (n_px == 0) return RT_OK;
  hipStream_t stream = (hipStream_t)stream_v;
  std::lock_guard<std::mutex> lock(dn->mu);
  HIP_TRY(hipSetDevice(dn->device));
  // G0, G1 and both colour records at every level count: the prefilter writes the second
  const size_t need = n_px * 64;
  if (need > dn->work_bytes) {
    if (dn->recorded) HIP_TRY(hipEventSynchronize(dn->done));
    if (dn->work) HIP_TRY(hipFree(dn->work));
    dn->work = nullptr;
    dn->work_bytes = 0;
    HIP_TRY(hipMalloc((void**)&dn->work, need));
    dn->work_bytes = need;
  }
  if (dn->recorded) HIP_TRY(hipStreamWaitEvent(stream, dn->done, 0));
  float4* const G0 = reinterpret_cast<float4*>(dn->work);
  float4* const G1 = G0 + n_px;
  float4* const Xa = G1 + n_px;
  float4* const Xb = Xa + n_px;
  DnVarParams V;
  std::memset(&V, 0, sizeof(V));
  DnParams& P = V.d;
  P.W = p->width;
  P.H = p->height;
  P.step = 1;
  P.flags = p->flags;
  P.B = (float)p->beauty_samples;
  P.A = (float)p->aov_samples;
  P.k_color = term_scale(p->sigma_color);  // every level: the propagated variance narrows it
  P.k_normal = term_scale(p->sigma_normal);
  P.k_depth = term_scale(p->sigma_depth);
  P.k_albedo = term_scale(p->sigma_albedo);
  V.n = (double)p->beauty_rows;
  V.vscale = V.n / ((V.n - 1.0) * p->beauty_samples * p->beauty_samples);
  const unsigned tiles_x = ((unsigned)P.W + kTileW - 1) / kTileW;
  const unsigned tiles_y = ((unsigned)P.H + kTileH - 1) / kTileH;
  const dim3 grid(tiles_x * tiles_y), block(kBlock);
  DoneGuard guard{dn, stream};
  guard.enqueued = true;
  if (stats) HIP_TRY(hipEventRecord(dn->ev0, stream));
  hipLaunchKernelGGL(dn_prepare_var, grid, block, 0, stream, V, beauty, m2, aov, G0, G1, Xa);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dn_prefilter_var, grid, block, 0, stream, P, G1, Xa, Xb);
  HIP_TRY(hipGetLastError());
  float4 *xin = Xb, *xout = Xa;
  for (int k = 0; k < p->levels; ++k) {
    P.step = 1 << k;
    typedef void (*kern_t)(DnParams, const float4*, const float4*, const float4*, float4*,
                           const float*, const float*, float*, float*);
    const bool last = k + 1 == p->levels;
    kern_t kern = last ? dn_atrous_var<true> : dn_atrous_var<false>;
    if (k == 0) kern = last ? dn_atrous_var_tiled<1, true> : dn_atrous_var_tiled<1, false>;
    if (k == 1) kern = last ? dn_atrous_var_tiled<2, true> : dn_atrous_var_tiled<2, false>;
    hipLaunchKernelGGL(kern, grid, block, 0, stream, P, G0, G1, xin, xout, beauty, aov, out,
                       var_out);
    HIP_TRY(hipGetLastError());
    std::swap(xin, xout);
  }
  if (stats) HIP_TRY(hipEventRecord(dn->ev1, stream));
  HIP_TRY(hipEventRecord(dn->done, stream));
  dn->recorded = true;
  guard.finished = true;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, dn->ev0, dn->ev1));
    stats->ms_kernel = ms;
    stats->samples = n_px;
    stats->out_bytes = (uint64_t)n_px * (var_out ? 4 : 3) * sizeof(float);
    stats->launches = 2u + (uint32_t)p->levels;
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return RT_OK;
}

int rt_denoise_var(rt_denoiser* dn, const rt_denoise_var_params* p, const float* beauty,
                   const float* m2, const float* aov, float* out, float* var_out,
                   rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  {
    const int rc = check_var_args(dn, p, beauty, m2, aov, out);
    if (rc != RT_OK) return rc;
  }
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  if (n_px == 0) return RT_OK;
  const size_t b_bytes = n_px * 3 * sizeof(float), a_bytes = n_px * RT_AOV_CHANNELS * sizeof(float);
  const size_t v_bytes = var_out ? n_px * sizeof(float) : 0;
  HIP_TRY(hipSetDevice(dn->device));
  // one allocation: the beauty frame (denoised in place), the moments, the AOVs, the variance
  uint8_t* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 2 * b_bytes + a_bytes + v_bytes));
  float* const d_beauty = reinterpret_cast<float*>(d);
  float* const d_m2 = reinterpret_cast<float*>(d + b_bytes);
  float* const d_aov = reinterpret_cast<float*>(d + 2 * b_bytes);
  float* const d_var = var_out ? reinterpret_cast<float*>(d + 2 * b_bytes + a_bytes) : nullptr;
  int rc = RT_OK;
  hipError_t e = hipMemcpy(d_beauty, beauty, b_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_m2, m2, b_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_aov, aov, a_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("upload: ") + hipGetErrorString(e));
  rt_stats local;
  if (rc == RT_OK)
    rc = rt_denoise_var_device(dn, p, d_beauty, d_m2, d_aov, d_beauty, d_var, nullptr,
                               stats ? stats : &local);
  if (rc == RT_OK) {
    e = hipMemcpy(out, d_beauty, b_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && var_out) e = hipMemcpy(var_out, d_var, v_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("download: ") + hipGetErrorString(e));
  }
  (void)hipFree(d);
  if (rc == RT_OK && stats)
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

}  // extern "C"
