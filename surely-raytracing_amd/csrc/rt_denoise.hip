// rt_denoise.hip — the two edge-avoiding a-trous denoisers of include/rt_mi355x.h: the dn_prepare*,
// dn_prefilter_var and dn_level kernels (bodies in rt_denoise.h) and the rt_denoise* entry points.
// Its own translation unit, built beside rt_device.hip and rt_aov.hip; it knows nothing of scenes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <utility>

#include "rt_mi355x.h"
#include "rt_denoise.h"
#include "rt_stage.hpp"

using namespace rtd;
using rts::set_err;
using rts::time_point;

struct rt_denoiser : rts::Stage {};

namespace {

__global__ __launch_bounds__(kBlock) void dn_prepare(DnParams P, const float* __restrict__ beauty,
                                                     const float* __restrict__ aov,
                                                     float4* __restrict__ G0,
                                                     float4* __restrict__ G1,
                                                     float4* __restrict__ X) {
  prepare_body(P, beauty, aov, G0, G1, X);
}

// The variance-guided filter's own prepare and its 3x3 variance prefilter.
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

// One level of either filter (atrous_level). VAR: with the variance lane; the plain filter passes
// a null var_out. STEP 0: the direct form, its step in P.step; STEP 1, 2: the records staged in
// LDS. FINAL: the last level, fused with the re-modulation and the store to the user's buffer
// (`out` may be `beauty`: each lane reads its own beauty pixel before it writes it).
template <bool VAR, int STEP, bool FINAL>
__global__ __launch_bounds__(kBlock) void dn_level(DnParams P, const float4* __restrict__ G0,
                                                   const float4* __restrict__ G1,
                                                   const float4* __restrict__ Xin, float4* Xout,
                                                   const float* beauty,
                                                   const float* __restrict__ aov, float* out,
                                                   float* var_out) {
  __shared__ TileLds<STEP> L;
  atrous_level<VAR, STEP, FINAL>(P, L, G0, G1, Xin, Xout, beauty, aov, out, var_out);
}

typedef void (*level_kern_t)(DnParams, const float4*, const float4*, const float4*, float4*,
                             const float*, const float*, float*, float*);

// the kernel of level k: steps 1 and 2 from LDS tiles (measured faster than the direct kernel; at
// step 4 the halo outgrows the tile and the tiled form measured no faster: DESIGN.md §4.2c)
template <bool VAR>
level_kern_t level_kernel(int k, bool last) {
  if (k == 0) return last ? dn_level<VAR, 1, true> : dn_level<VAR, 1, false>;
  if (k == 1) return last ? dn_level<VAR, 2, true> : dn_level<VAR, 2, false>;
  return last ? dn_level<VAR, 0, true> : dn_level<VAR, 0, false>;
}

// what rt_denoise_params and rt_denoise_var_params share
struct Fields {
  int32_t width, height, levels;
  uint32_t flags;
  double beauty_samples, aov_samples;
  float sigma_color, sigma_normal, sigma_depth, sigma_albedo;
};
template <class PARAMS>
Fields fields(const PARAMS& p) {
  return Fields{p.width,       p.height,      p.levels,       p.flags,       p.beauty_samples,
                p.aov_samples, p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo};
}

// Everything that can be refused without reading the handle or touching HIP.
int check_fields(const Fields& f) {
  if (f.width <= 0 || f.height < 0)
    return set_err(RT_ERR_INVALID_ARG, "bad frame size (width <= 0 or height < 0)");
  if ((int64_t)f.width * f.height >= (1ll << 31))
    return set_err(RT_ERR_INVALID_ARG, "frame too large (width * height >= 2^31)");
  if (f.levels < 1 || f.levels > RT_DENOISE_MAX_LEVELS)
    return set_err(RT_ERR_INVALID_ARG, "levels outside 1..RT_DENOISE_MAX_LEVELS");
  if (f.flags & ~RT_DENOISE_DEMODULATE)
    return set_err(RT_ERR_INVALID_ARG, "unknown RT_DENOISE_* flag bits");
  if (!std::isfinite(f.beauty_samples) || f.beauty_samples <= 0.0 ||
      !std::isfinite(f.aov_samples) || f.aov_samples <= 0.0)
    return set_err(RT_ERR_INVALID_ARG, "sample counts must be finite and > 0");
  if (!std::isfinite(f.sigma_color) || !std::isfinite(f.sigma_normal) ||
      !std::isfinite(f.sigma_depth) || !std::isfinite(f.sigma_albedo))
    return set_err(RT_ERR_INVALID_ARG, "non-finite sigma");
  return RT_OK;
}

// rt_denoise_var*: the shared fields as rt_denoise's, then its own
int check_var_fields(const rt_denoise_var_params& p) {
  const int rc = check_fields(fields(p));
  if (rc != RT_OK) return rc;
  if (p.beauty_rows < 2)
    return set_err(RT_ERR_INVALID_ARG, "beauty_rows < 2 (the between-row estimate needs two rows)");
  if (p._pad0 != 0) return set_err(RT_ERR_INVALID_ARG, "_pad0 must be 0");
  return RT_OK;
}

// log2(e) / sigma^2 (the kernel evaluates exp2 of the summed exponent); 0 switches the term off
float term_scale(double sigma) {
  return sigma > 0.0 ? (float)(1.4426950408889634 / (sigma * sigma)) : 0.f;
}

// Both filters on device buffers, the arguments already checked. A null m2 is the plain filter
// (var_out null, beauty_rows unused); otherwise the variance-guided one.
int denoise_device(rt_denoiser* dn, const Fields& f, int beauty_rows, const float* beauty,
                   const float* m2, const float* aov, float* out, float* var_out,
                   hipStream_t stream, rt_stats* stats, time_point t0) {
  const bool var = m2 != nullptr;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)f.width * (size_t)f.height;
  if (n_px == 0) return RT_OK;
  // held to the end of the call, through the synchronisation a stats call asks for: the stats
  // events are the handle's
  std::lock_guard<std::mutex> lock(dn->mu);
  HIP_TRY(hipSetDevice(dn->device));
  // bytes of workspace per pixel: G0, G1 and the two colour records the levels alternate between
  // (a single plain level reads one and writes the user's buffer; the prefilter always writes the
  // second)
  RT_TRY(dn->reserve(n_px * (var || f.levels > 1 ? 64 : 48)));
  float4* const G0 = reinterpret_cast<float4*>(dn->work);
  float4* const G1 = G0 + n_px;
  float4 *xin = G1 + n_px, *xout = xin + n_px;  // xout: touched only at 64 B per pixel
  DnVarParams V;
  std::memset(&V, 0, sizeof(V));
  DnParams& P = V.d;
  P.W = f.width;
  P.H = f.height;
  P.step = 1;
  P.flags = f.flags;
  P.B = (float)f.beauty_samples;
  P.A = (float)f.aov_samples;
  P.k_normal = term_scale(f.sigma_normal);
  P.k_depth = term_scale(f.sigma_depth);
  P.k_albedo = term_scale(f.sigma_albedo);
  const unsigned tiles_x = ((unsigned)P.W + kTileW - 1) / kTileW;
  const unsigned tiles_y = ((unsigned)P.H + kTileH - 1) / kTileH;
  const dim3 grid(tiles_x * tiles_y), block(kBlock);  // W * H < 2^31: fewer than 2^28 + W + H tiles
  {
    rts::Run run(*dn, stream);
    RT_TRY(run.begin(stats != nullptr));
    if (var) {
      P.k_color = term_scale(f.sigma_color);  // every level: the propagated variance narrows it
      V.n = (double)beauty_rows;
      V.vscale = V.n / ((V.n - 1.0) * f.beauty_samples * f.beauty_samples);
      hipLaunchKernelGGL(dn_prepare_var, grid, block, 0, stream, V, beauty, m2, aov, G0, G1, xin);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(dn_prefilter_var, grid, block, 0, stream, P, G1, xin, xout);
      HIP_TRY(hipGetLastError());
      std::swap(xin, xout);
    } else {
      hipLaunchKernelGGL(dn_prepare, grid, block, 0, stream, P, beauty, aov, G0, G1, xin);
      HIP_TRY(hipGetLastError());
    }
    for (int k = 0; k < f.levels; ++k) {
      P.step = 1 << k;
      if (!var) P.k_color = term_scale((double)f.sigma_color / (double)(1 << k));  // sigma_c * 2^-k
      const bool last = k + 1 == f.levels;
      const level_kern_t kern = var ? level_kernel<true>(k, last) : level_kernel<false>(k, last);
      hipLaunchKernelGGL(kern, grid, block, 0, stream, P, G0, G1, xin, xout, beauty, aov, out,
                         var_out);
      HIP_TRY(hipGetLastError());
      std::swap(xin, xout);
    }
    if (stats) HIP_TRY(hipEventRecord(dn->ev1, stream));
  }
  if (stats) {
    const uint64_t out_bytes = (uint64_t)n_px * (var_out ? 4 : 3) * sizeof(float);
    RT_TRY(dn->finish_stats(stream, stats, n_px, out_bytes, (var ? 2u : 1u) + (uint32_t)f.levels,
                            t0));
  }
  return RT_OK;
}

// The same on host buffers: staged through one allocation, denoised in place, synchronous.
int denoise_host(rt_denoiser* dn, const Fields& f, int beauty_rows, const float* beauty,
                 const float* m2, const float* aov, float* out, float* var_out, rt_stats* stats,
                 time_point t0) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = (size_t)f.width * (size_t)f.height;
  if (n_px == 0) return RT_OK;
  const size_t b_bytes = n_px * 3 * sizeof(float), a_bytes = n_px * RT_AOV_CHANNELS * sizeof(float);
  // the beauty frame (denoised in place), the moments, the AOVs, the variance
  rts::Staging st;
  const int i_beauty = st.add(b_bytes), i_m2 = st.add_if(m2 != nullptr, b_bytes);
  const int i_aov = st.add(a_bytes), i_var = st.add_if(var_out != nullptr, n_px * sizeof(float));
  RT_TRY(st.alloc(dn->device));
  RT_TRY(st.upload(i_beauty, beauty));
  RT_TRY(st.upload(i_m2, m2));
  RT_TRY(st.upload(i_aov, aov));
  float* const d_beauty = st.ptr<float>(i_beauty);
  rt_stats local;
  RT_TRY(denoise_device(dn, f, beauty_rows, d_beauty, st.ptr<float>(i_m2), st.ptr<float>(i_aov),
                        d_beauty, st.ptr<float>(i_var), nullptr, stats ? stats : &local, t0));
  RT_TRY(st.download(i_beauty, out));
  RT_TRY(st.download(i_var, var_out));
  if (stats) stats->ms_total = rts::ms_since(t0);
  return RT_OK;
}

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
  const int rc = check_fields(fields(p));
  if (rc != RT_OK) return rc;
  *out = p;
  return RT_OK;
}

int rt_denoiser_create(int device, rt_denoiser** out) {
  return rts::stage_create(device, true, out);
}

void rt_denoiser_destroy(rt_denoiser* dn) { rts::stage_destroy(dn); }

int rt_denoise_device(rt_denoiser* dn, const rt_denoise_params* p, const float* beauty,
                      const float* aov, float* out, void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  if (!dn || !p || !beauty || !aov || !out) return set_err(RT_ERR_INVALID_ARG, "null argument");
  const int rc = check_fields(fields(*p));
  if (rc != RT_OK) return rc;
  return denoise_device(dn, fields(*p), 0, beauty, nullptr, aov, out, nullptr,
                        (hipStream_t)stream_v, stats, t0);
}

int rt_denoise(rt_denoiser* dn, const rt_denoise_params* p, const float* beauty, const float* aov,
               float* out, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  if (!dn || !p || !beauty || !aov || !out) return set_err(RT_ERR_INVALID_ARG, "null argument");
  const int rc = check_fields(fields(*p));
  if (rc != RT_OK) return rc;
  return denoise_host(dn, fields(*p), 0, beauty, nullptr, aov, out, nullptr, stats, t0);
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
  const int rc = check_var_fields(p);
  if (rc != RT_OK) return rc;
  *out = p;
  return RT_OK;
}

int rt_denoise_var_device(rt_denoiser* dn, const rt_denoise_var_params* p, const float* beauty,
                          const float* m2, const float* aov, float* out, float* var_out,
                          void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  if (!dn || !p || !beauty || !m2 || !aov || !out)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  const int rc = check_var_fields(*p);
  if (rc != RT_OK) return rc;
  return denoise_device(dn, fields(*p), p->beauty_rows, beauty, m2, aov, out, var_out,
                        (hipStream_t)stream_v, stats, t0);
}

int rt_denoise_var(rt_denoiser* dn, const rt_denoise_var_params* p, const float* beauty,
                   const float* m2, const float* aov, float* out, float* var_out,
                   rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  if (!dn || !p || !beauty || !m2 || !aov || !out)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  const int rc = check_var_fields(*p);
  if (rc != RT_OK) return rc;
  return denoise_host(dn, fields(*p), p->beauty_rows, beauty, m2, aov, out, var_out, stats, t0);
}

}  // extern "C"
