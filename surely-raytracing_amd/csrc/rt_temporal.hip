// rt_temporal.hip — temporal accumulation with reprojection of the frame history
// (include/rt_mi355x.h): the tp_accumulate kernel (body in rt_temporal.h), the rt_temporal handle
// with its two alternating history sets, and the rt_temporal_* entry points. Its own translation
// unit, built beside rt_denoise.hip; of scenes it knows nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>

#include "rt_mi355x.h"
#include "rt_temporal.h"
#include "rt_stage.hpp"

using namespace rtt;
using rts::set_err;
using rts::time_point;

// The workspace holds two history sets of 48 B per pixel; a call reads set `cur` and writes the
// other.
struct rt_temporal : rts::Stage {
  int cur = 0;
  int hist_w = 0, hist_h = 0;  // 0 x 0: no history
  bool hist_m2 = false;
  uint64_t frames = 0;
  double center[3] = {0, 0, 0};  // of the camera that wrote the history
  double minv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // the inverse of its M
};

namespace {

template <bool M2>
__global__ __launch_bounds__(kBlock) void tp_accumulate(TpParams P, const float* beauty,
                                                        const float* m2,
                                                        const float* __restrict__ aov,
                                                        const float4* __restrict__ hin,
                                                        float4* __restrict__ hout, float* out_b,
                                                        float* out_q,
                                                        float* __restrict__ hist_len) {
  accumulate_body<M2>(P, beauty, m2, aov, hin, hout, out_b, out_q, hist_len);
}

constexpr uint32_t kKnownFlags = RT_TEMPORAL_RESET | RT_TEMPORAL_VARIANCE_OF_MEAN;
constexpr size_t kSetBytesPerPixel = 48;  // three float4 records

// The inverse of M = [pixel00_loc - center | pixel_delta_u | pixel_delta_v] (columns), row-major,
// as adjugate over determinant in f64. False for a singular or non-finite M.
bool invert_camera(const rt_camera* cam, double inv[9]) {
  double m[3][3];  // m[r][c]
  for (int r = 0; r < 3; ++r) {
    m[r][0] = cam->pixel00_loc[r] - cam->center[r];
    m[r][1] = cam->pixel_delta_u[r];
    m[r][2] = cam->pixel_delta_v[r];
  }
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
  const double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
  const double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
  if (!std::isfinite(det) || det == 0.0) return false;
  inv[0] = c00 / det;
  inv[1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
  inv[2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
  inv[3] = c01 / det;
  inv[4] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
  inv[5] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
  inv[6] = c02 / det;
  inv[7] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
  inv[8] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(inv[k])) return false;
  return true;
}

int check_params(const rt_temporal_params& p) {
  if (p.width <= 0 || p.height < 0)
    return set_err(RT_ERR_INVALID_ARG, "bad frame size (width <= 0 or height < 0)");
  if ((int64_t)p.width * p.height >= (1ll << 31))
    return set_err(RT_ERR_INVALID_ARG, "frame too large (width * height >= 2^31)");
  if (p.flags & ~kKnownFlags)
    return set_err(RT_ERR_INVALID_ARG, "unknown RT_TEMPORAL_* flag bits");
  if (p.beauty_rows < 0) return set_err(RT_ERR_INVALID_ARG, "beauty_rows < 0");
  if ((p.flags & RT_TEMPORAL_VARIANCE_OF_MEAN) && p.beauty_rows < 2)
    return set_err(RT_ERR_INVALID_ARG, "RT_TEMPORAL_VARIANCE_OF_MEAN needs beauty_rows >= 2");
  if (!std::isfinite(p.max_history) || p.max_history < 1.f)
    return set_err(RT_ERR_INVALID_ARG, "max_history must be finite and >= 1");
  if (!std::isfinite(p.depth_tol) || !std::isfinite(p.normal_tol))
    return set_err(RT_ERR_INVALID_ARG, "non-finite tolerance");
  if (!std::isfinite(p.min_weight) || p.min_weight < 0.f || p.min_weight >= 1.f)
    return set_err(RT_ERR_INVALID_ARG, "min_weight must be finite and in [0, 1)");
  return RT_OK;
}

// everything that can be judged without the handle and without HIP; inv: the inverse of cam's M
int check_args(const rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam,
               const float* beauty, const float* m2, const float* aov, const float* out_beauty,
               const float* out_m2, double inv[9]) {
  if (!t || !p || !cam || !beauty || !aov || !out_beauty)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  const int rc = check_params(*p);
  if (rc != RT_OK) return rc;
  if ((m2 != nullptr) != (out_m2 != nullptr))
    return set_err(RT_ERR_INVALID_ARG, "m2 and out_m2 must be given together or not at all");
  if ((p->flags & RT_TEMPORAL_VARIANCE_OF_MEAN) && !m2)
    return set_err(RT_ERR_INVALID_ARG, "RT_TEMPORAL_VARIANCE_OF_MEAN needs m2");
  if (cam->image_width != p->width || cam->image_height != p->height)
    return set_err(RT_ERR_INVALID_ARG, "the camera's image size differs from the params'");
  if (!invert_camera(cam, inv) || !std::isfinite(cam->center[0]) ||
      !std::isfinite(cam->center[1]) || !std::isfinite(cam->center[2]))
    return set_err(RT_ERR_INVALID_ARG, "singular or non-finite camera");
  return RT_OK;
}

// the arguments checked, at least one pixel; inv: the inverse of cam's M
int accumulate_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam,
                      const double inv[9], const float* beauty, const float* m2, const float* aov,
                      float* out_beauty, float* out_m2, float* hist_len, hipStream_t stream,
                      rt_stats* stats, time_point t0) {
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  // held to the end of the call, through the synchronisation a stats call asks for: the stats
  // events are the handle's
  std::lock_guard<std::mutex> lock(t->mu);
  const bool has_history = !(p->flags & RT_TEMPORAL_RESET) && t->hist_w == p->width &&
                           t->hist_h == p->height;
  if (has_history && t->hist_m2 != (m2 != nullptr))
    return set_err(RT_ERR_INVALID_ARG, m2 ? "m2 given, but the history carries no moments"
                                          : "the history carries moments, but m2 is null");
  HIP_TRY(hipSetDevice(t->device));
  const size_t need = 2 * kSetBytesPerPixel * n_px;
  // a larger frame: the history is void, whether or not the new workspace can be had
  if (need > t->work_bytes) t->hist_w = t->hist_h = 0;
  RT_TRY(t->reserve(need));
  // the sets lie n_px * 48 B apart, for this frame size: a size change voids the history anyway
  const float4* hin = reinterpret_cast<const float4*>(t->work + (size_t)t->cur * kSetBytesPerPixel * n_px);
  float4* hout = reinterpret_cast<float4*>(t->work + (size_t)(1 - t->cur) * kSetBytesPerPixel * n_px);
  TpParams P;
  std::memset(&P, 0, sizeof(P));
  P.W = p->width;
  P.H = p->height;
  P.mode = (has_history ? kHasHistory : 0u) |
           ((p->flags & RT_TEMPORAL_VARIANCE_OF_MEAN) ? kVarianceOfMean : 0u);
  P.max_history = p->max_history;
  P.normal_tol2 = p->normal_tol > 0.f ? (float)((double)p->normal_tol * (double)p->normal_tol) : 0.f;
  P.min_weight = p->min_weight;
  P.depth_tol = p->depth_tol > 0.f ? (double)p->depth_tol : 0.0;
  P.rows = (double)p->beauty_rows;
  for (int k = 0; k < 3; ++k) {
    P.p00c[k] = cam->pixel00_loc[k] - cam->center[k];
    P.du[k] = cam->pixel_delta_u[k];
    P.dv[k] = cam->pixel_delta_v[k];
    P.cdiff[k] = has_history ? cam->center[k] - t->center[k] : 0.0;
  }
  if (has_history) std::memcpy(P.minv, t->minv, sizeof(P.minv));
  const unsigned tiles_x = ((unsigned)P.W + kTileW - 1) / kTileW;
  const unsigned tiles_y = ((unsigned)P.H + kTileH - 1) / kTileH;
  const dim3 grid(tiles_x * tiles_y), block(kBlock);  // W * H < 2^31: fewer than 2^28 + W + H tiles
  {
    rts::Run run(*t, stream);
    RT_TRY(run.begin(stats != nullptr));
    if (m2)
      hipLaunchKernelGGL(tp_accumulate<true>, grid, block, 0, stream, P, beauty, m2, aov, hin, hout,
                         out_beauty, out_m2, hist_len);
    else
      hipLaunchKernelGGL(tp_accumulate<false>, grid, block, 0, stream, P, beauty, m2, aov, hin,
                         hout, out_beauty, out_m2, hist_len);
    HIP_TRY(hipGetLastError());
    // the launch is in the stream: from here the other set is the history
    t->cur = 1 - t->cur;
    t->frames = has_history ? t->frames + 1 : 1;
    t->hist_w = p->width;
    t->hist_h = p->height;
    t->hist_m2 = m2 != nullptr;
    std::memcpy(t->center, cam->center, sizeof(t->center));
    std::memcpy(t->minv, inv, sizeof(t->minv));
    if (stats) HIP_TRY(hipEventRecord(t->ev1, stream));
  }
  if (stats) {
    const uint64_t out_bytes = (uint64_t)n_px * ((m2 ? 6 : 3) + (hist_len ? 1 : 0)) * sizeof(float);
    RT_TRY(t->finish_stats(stream, stats, n_px, out_bytes, 1u, t0));
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_temporal_default_params(int width, int height, rt_temporal_params* out) {
  if (!out) return set_err(RT_ERR_INVALID_ARG, "null out");
  rt_temporal_params p;
  std::memset(&p, 0, sizeof(p));
  p.width = width;
  p.height = height;
  p.max_history = 4.f;  // measured: DESIGN.md §4.2h
  p.depth_tol = 0.1f;
  p.normal_tol = 0.3f;
  p.min_weight = 0.01f;
  const int rc = check_params(p);
  if (rc != RT_OK) return rc;
  *out = p;
  return RT_OK;
}

int rt_temporal_create(int device, rt_temporal** out) {
  return rts::stage_create(device, true, out);
}

void rt_temporal_destroy(rt_temporal* t) { rts::stage_destroy(t); }

int rt_temporal_info(rt_temporal* t, uint64_t* out, int n) {
  if (!t || !out || n < 0) return set_err(RT_ERR_INVALID_ARG, "null argument");
  std::lock_guard<std::mutex> lock(t->mu);
  const bool held = t->hist_w > 0 && t->hist_h > 0;
  const uint64_t v[4] = {held ? t->frames : 0, (uint64_t)t->hist_w, (uint64_t)t->hist_h,
                         held && t->hist_m2 ? 1u : 0u};
  for (int k = 0; k < n && k < 4; ++k) out[k] = v[k];
  return RT_OK;
}

int rt_temporal_accumulate_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam,
                                  const float* beauty, const float* m2, const float* aov,
                                  float* out_beauty, float* out_m2, float* hist_len, void* stream_v,
                                  rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  double inv[9];
  const int rc = check_args(t, p, cam, beauty, m2, aov, out_beauty, out_m2, inv);
  if (rc != RT_OK) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (p->height == 0) return RT_OK;
  return accumulate_device(t, p, cam, inv, beauty, m2, aov, out_beauty, out_m2, hist_len,
                           (hipStream_t)stream_v, stats, t0);
}

int rt_temporal_accumulate(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam,
                           const float* beauty, const float* m2, const float* aov,
                           float* out_beauty, float* out_m2, float* hist_len, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  double inv[9];
  const int rc = check_args(t, p, cam, beauty, m2, aov, out_beauty, out_m2, inv);
  if (rc != RT_OK) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (p->height == 0) return RT_OK;
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  const size_t b_bytes = n_px * 3 * sizeof(float), a_bytes = n_px * RT_AOV_CHANNELS * sizeof(float);
  // the beauty frame and the moments (both accumulated in place), the AOVs, the history lengths
  rts::Staging st;
  const int i_beauty = st.add(b_bytes), i_m2 = st.add_if(m2 != nullptr, b_bytes);
  const int i_aov = st.add(a_bytes), i_len = st.add_if(hist_len != nullptr, n_px * sizeof(float));
  RT_TRY(st.alloc(t->device));
  RT_TRY(st.upload(i_beauty, beauty));
  RT_TRY(st.upload(i_m2, m2));
  RT_TRY(st.upload(i_aov, aov));
  float *const d_beauty = st.ptr<float>(i_beauty), *const d_m2 = st.ptr<float>(i_m2);
  rt_stats local;
  RT_TRY(accumulate_device(t, p, cam, inv, d_beauty, d_m2, st.ptr<float>(i_aov), d_beauty, d_m2,
                           st.ptr<float>(i_len), nullptr, stats ? stats : &local, t0));
  RT_TRY(st.download(i_beauty, out_beauty));
  RT_TRY(st.download(i_m2, out_m2));
  RT_TRY(st.download(i_len, hist_len));
  if (stats) stats->ms_total = rts::ms_since(t0);
  return RT_OK;
}

}  // extern "C"
