// rt_raygen.hip — the ray generators on the device (include/rt_mi355x.h): rth_projection_rays and
// rth_ao_rays (host/capi.cpp) restated one lane per ray, the count of unoccluded directions, the
// rt_raygen handle and the ambient-occlusion driver over rt_query_rays_device. The host's
// functions are the definition; the expressions below are theirs, in their order, fma where they
// write std::fma and nowhere else (the build has -ffp-contract=off). Its own translation unit; of
// scenes it knows the device ordinal alone.
//
// One lane per ray, 64 consecutive rays per wave, as query_body (rt_query.h): an 80-byte record
// is five 16-byte stores (the AO generator reads the two 16-byte words of the primary and the four
// of the record it needs the same way); lanes past the end of a ragged last wave store nothing.
// No LDS, no atomics: a ray depends on its index and the arguments alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "rt_mi355x.h"
#include "rt_frame3.h"
#include "rt_rng.h"
#include "rt_stage.hpp"

using rts::set_err;
using rts::time_point;

static_assert(sizeof(rt_projection) == 96 && sizeof(rt_ao_params) == 32 &&
                  sizeof(rt_ao_frame_params) == 40,
              "rt_projection, rt_ao_params, rt_ao_frame_params: no padding");

// The workspace is rt_ambient_occlusion_device's: per chunk the records (unless the caller takes
// them), the AO rays and the occlusion bytes.
struct rt_raygen : rts::Stage {};

namespace {

constexpr int kBlock = 256;
constexpr uint64_t kDefaultChunk = 1ull << 22;
constexpr double kPi = 3.14159265358979323846;  // M_PI

__device__ __forceinline__ uint4 pack2(double a, double b) {
  const unsigned long long x = (unsigned long long)__double_as_longlong(a);
  const unsigned long long y = (unsigned long long)__double_as_longlong(b);
  return make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
}
__device__ __forceinline__ double lo_f64(const uint4& v) {
  return __longlong_as_double((long long)(((unsigned long long)v.y << 32) | v.x));
}
__device__ __forceinline__ double hi_f64(const uint4& v) {
  return __longlong_as_double((long long)(((unsigned long long)v.w << 32) | v.z));
}
__device__ __forceinline__ void store_ray(uint4* R, const double* o, const double* d, double time,
                                          double tmin, double tmax, uint32_t pixel,
                                          uint32_t sample) {
  R[0] = pack2(o[0], o[1]);
  R[1] = pack2(o[2], d[0]);
  R[2] = pack2(d[1], d[2]);
  R[3] = pack2(time, tmin);
  const uint4 t = pack2(tmax, 0.0);
  R[4] = make_uint4(t.x, t.y, pixel, sample);
}

// what the projection kernels take: the frame, the view frame formed on the host, the stratum
struct ProjArgs {
  double f[3], r[3], u[3], origin[3];
  double fov, rs;
  int32_t W, H, S, s_i, s_j;
  uint32_t first_pixel;  // row_begin * W
  uint32_t n;            // n_rows * W
  uint32_t seed_lo, seed_hi;
};
// the pinhole's camera fields (get_ray without the defocus disk)
struct PinArgs {
  double center[3], p00[3], du[3], dv[3];
};

// rth_projection_rays' loop body for ray `idx` of the band
template <int KIND>
__global__ __launch_bounds__(kBlock) void raygen_projection(ProjArgs A, PinArgs C,
                                                            uint4* __restrict__ rays) {
  const uint32_t idx = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (idx >= A.n) return;
  const uint32_t pixel = A.first_pixel + idx;
  const uint32_t sample = (uint32_t)(A.s_j * A.S + A.s_i);
  const int i = (int)(pixel % (uint32_t)A.W), j = (int)(pixel / (uint32_t)A.W);
  rtd::Rng g = rtd::rng_seed(A.seed_lo, A.seed_hi, pixel, sample);
  const double px = fma(A.rs, (double)A.s_i + rtd::rnd(g), -0.5);
  const double py = fma(A.rs, (double)A.s_j + rtd::rnd(g), -0.5);
  const double time = rtd::rnd(g);
  double o[3], d[3];
  if (KIND == RT_PROJ_PINHOLE) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double pc = fma((double)j, C.dv[k], fma((double)i, C.du[k], C.p00[k]));
      const double ps = pc + fma(px, C.du[k], C.dv[k] * py);
      o[k] = C.center[k];
      d[k] = ps - C.center[k];
    }
  } else {
    const double x = ((double)i + 0.5 + px) / (double)A.W, y = ((double)j + 0.5 + py) / (double)A.H;
    double a = 0.0, b = 0.0, c = 0.0;  // dir = a r + b u + c f
    double oa = 0.0, ob = 0.0;         // origin offset along r and u
    if (KIND == RT_PROJ_ORTHO) {
      c = 1.0;
      oa = (x - 0.5) * A.fov * (double)A.W / (double)A.H;
      ob = (0.5 - y) * A.fov;
    } else if (KIND == RT_PROJ_PANORAMA) {
      const double lon = (x - 0.5) * 2.0 * kPi, lat = (0.5 - y) * kPi;
      a = cos(lat) * sin(lon);
      b = sin(lat);
      c = cos(lat) * cos(lon);
    } else {
      const double m = (double)(A.W < A.H ? A.W : A.H);
      const double nx = (2.0 * x - 1.0) * (double)A.W / m, ny = (1.0 - 2.0 * y) * (double)A.H / m;
      const double th = hypot(nx, ny) * (A.fov * kPi / 180.0) * 0.5;
      if (th <= kPi) {
        const double ph = atan2(ny, nx);
        a = sin(th) * cos(ph);
        b = sin(th) * sin(ph);
        c = cos(th);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k] = A.origin[k] + oa * A.r[k] + ob * A.u[k];
      d[k] = a * A.r[k] + b * A.u[k] + c * A.f[k];
    }
  }
  store_ray(rays + (size_t)idx * 5u, o, d, time, 1e-4, (double)INFINITY, pixel, sample);
}

typedef void (*proj_kern_t)(ProjArgs, PinArgs, uint4*);
proj_kern_t projection_kernel(int kind) {
  switch (kind) {
    case RT_PROJ_PINHOLE: return raygen_projection<RT_PROJ_PINHOLE>;
    case RT_PROJ_ORTHO: return raygen_projection<RT_PROJ_ORTHO>;
    case RT_PROJ_PANORAMA: return raygen_projection<RT_PROJ_PANORAMA>;
    default: return raygen_projection<RT_PROJ_FISHEYE>;
  }
}

// rth_ao_rays' loop body for ray i. primary and out may be the same buffer (no __restrict__): a
// lane reads its own records before it writes its own ray, and no lane reads another's.
__global__ __launch_bounds__(kBlock) void raygen_ao(const uint4* primary, const uint4* hits,
                                                    uint4* out, uint32_t n, uint32_t seed_lo,
                                                    uint32_t seed_hi, double tmin, double radius,
                                                    uint32_t dir_index) {
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (i >= n) return;
  const uint4* P = primary + (size_t)i * 5u;
  const uint4* H = hits + (size_t)i * 5u;
  const uint4 p3 = P[3], p4 = P[4];  // time, tmin | tmax, pixel, sample
  const uint4 h1 = H[1], h2 = H[2], h3 = H[3], h4 = H[4];  // p.xy | p.z, n.x | n.yz | hit ..
  const double time = lo_f64(p3);
  const uint32_t pixel = p4.z;
  double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
  if ((int32_t)h4.x == 1) {
    const double nrm[3] = {hi_f64(h2), lo_f64(h3), hi_f64(h3)};
    rtd::Rng g = rtd::rng_seed(seed_lo, seed_hi, pixel, dir_index);
    const double r1 = rtd::rnd(g), r2 = rtd::rnd(g);
    // random_cosine_direction (vec3.rs:240-250)
    const double phi = 2. * kPi * r1;
    const double x = cos(phi) * sqrt(r2), y = sin(phi) * sqrt(r2);
    const double z = sqrt(1. - r2);
    // Onb::build_from_w (onb.rs:32-47)
    double w[3], a[3] = {1., 0., 0.}, wa[3], v[3], u[3];
    const double wl = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = nrm[k] / wl;
    if (fabs(w[0]) > 0.9) a[0] = 0., a[1] = 1.;
    wa[0] = w[1] * a[2] - w[2] * a[1];
    wa[1] = w[2] * a[0] - w[0] * a[2];
    wa[2] = w[0] * a[1] - w[1] * a[0];
    const double vl = sqrt(wa[0] * wa[0] + wa[1] * wa[1] + wa[2] * wa[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = wa[k] / vl;
    u[0] = w[1] * v[2] - w[2] * v[1];
    u[1] = w[2] * v[0] - w[0] * v[2];
    u[2] = w[0] * v[1] - w[1] * v[0];
    o[0] = lo_f64(h1), o[1] = hi_f64(h1), o[2] = lo_f64(h2);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = x * u[k] + y * v[k] + z * w[k];  // Onb::local (onb.rs:24-26)
  }
  store_ray(out + (size_t)i * 5u, o, d, time, tmin, radius, pixel, dir_index);
}

// the count of unoccluded directions: 1 byte read, CH floats read-modify-written per lane
template <int CH, bool OVERWRITE>
__global__ __launch_bounds__(kBlock) void raygen_accumulate(const uint8_t* __restrict__ occ,
                                                            float* __restrict__ sums, uint32_t n) {
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (i >= n) return;
  const float add = occ[i] == 0 ? 1.0f : 0.0f;
  float* s = sums + (size_t)i * CH;
#pragma unroll
  for (int c = 0; c < CH; ++c) s[c] = (OVERWRITE ? 0.0f : s[c]) + add;
}

typedef void (*acc_kern_t)(const uint8_t*, float*, uint32_t);
acc_kern_t accumulate_kernel(uint32_t channels, bool overwrite) {
  if (channels == 3) return overwrite ? raygen_accumulate<3, true> : raygen_accumulate<3, false>;
  return overwrite ? raygen_accumulate<1, true> : raygen_accumulate<1, false>;
}

unsigned blocks_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// ---- the argument checks: everything that can be judged without the handle and without HIP

bool aligned16(const void* p) { return (uintptr_t)p % 16u == 0; }

int check_interval(double tmin, double radius) {
  if (!(std::isfinite(tmin) && tmin >= 0.0))
    return set_err(RT_ERR_INVALID_ARG, "tmin must be finite and >= 0");
  if (!(radius > tmin))
    return set_err(RT_ERR_INVALID_ARG, "radius must be > tmin (NaN is invalid)");
  return RT_OK;
}

// rth_projection_rays' checks and the row range; fills the kernels' arguments
int check_projection(const rt_raygen* g, const rt_projection* pr, const rt_camera* cam,
                     uint64_t seed, int32_t s_i, int32_t s_j, int32_t row_begin, int32_t n_rows,
                     const rt_ray* rays, ProjArgs* A, PinArgs* C) {
  using rtframe::cross3;
  using rtframe::unit3;
  if (!g || !pr || !rays) return set_err(RT_ERR_INVALID_ARG, "null argument");
  const bool pin = pr->kind == RT_PROJ_PINHOLE;
  if (pr->kind < RT_PROJ_PINHOLE || pr->kind > RT_PROJ_FISHEYE)
    return set_err(RT_ERR_INVALID_ARG, "unknown projection kind");
  if (pin && !cam) return set_err(RT_ERR_INVALID_ARG, "the pinhole projection needs a camera");
  const int W = pin ? cam->image_width : pr->width, H = pin ? cam->image_height : pr->height;
  const int S = pin ? cam->sqrt_spp : pr->sqrt_spp;
  if (W < 1 || H < 1 || S < 1 || (int64_t)W * H >= (1ll << 31))
    return set_err(RT_ERR_INVALID_ARG,
                   "width, height and sqrt_spp must be >= 1 (and width * height < 2^31)");
  if (s_i < 0 || s_i >= S || s_j < 0 || s_j >= S)
    return set_err(RT_ERR_INVALID_ARG, "stratum outside sqrt_spp");
  if (row_begin < 0 || n_rows < 0 || (int64_t)row_begin + n_rows > H)
    return set_err(RT_ERR_INVALID_ARG,
                   "rows outside the frame (row_begin < 0, n_rows < 0 or past the height)");
  if (!aligned16(rays)) return set_err(RT_ERR_INVALID_ARG, "rays not 16-byte aligned");
  std::memset(A, 0, sizeof(*A));
  std::memset(C, 0, sizeof(*C));
  if (!pin) {
    double fxu[3];
    if (!unit3(pr->forward, A->f))
      return set_err(RT_ERR_INVALID_ARG, "forward is zero or not finite");
    cross3(A->f, pr->up, fxu);
    if (!unit3(fxu, A->r))
      return set_err(RT_ERR_INVALID_ARG, "up is zero, not finite or parallel to forward");
    cross3(A->r, A->f, A->u);
    for (int k = 0; k < 3; ++k) {
      if (!std::isfinite(pr->origin[k])) return set_err(RT_ERR_INVALID_ARG, "origin is not finite");
      A->origin[k] = pr->origin[k];
    }
    if (pr->kind != RT_PROJ_PANORAMA && !(pr->fov > 0.0 && std::isfinite(pr->fov)))
      return set_err(RT_ERR_INVALID_ARG, "fov must be positive and finite");
    A->fov = pr->fov;
  } else {
    for (int k = 0; k < 3; ++k) {
      C->center[k] = cam->center[k];
      C->p00[k] = cam->pixel00_loc[k];
      C->du[k] = cam->pixel_delta_u[k];
      C->dv[k] = cam->pixel_delta_v[k];
    }
  }
  // recip_sqrt_spp as Camera::new forms it (render.rs:76); the pinhole takes the camera's own
  A->rs = pin ? cam->recip_sqrt_spp : 1.0 / (double)S;
  A->W = W, A->H = H, A->S = S, A->s_i = s_i, A->s_j = s_j;
  A->first_pixel = (uint32_t)((int64_t)row_begin * W);
  A->n = (uint32_t)((int64_t)n_rows * W);
  A->seed_lo = (uint32_t)seed, A->seed_hi = (uint32_t)(seed >> 32);
  return RT_OK;
}

int check_ao_rays(const rt_raygen* g, const rt_ao_params* p, const rt_ray* primary,
                  const rt_hit* hits, uint64_t n, const rt_ray* out) {
  if (!g || !p || !primary || !hits || !out) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (n >= (1ull << 31)) return set_err(RT_ERR_INVALID_ARG, "n >= 2^31");
  if (!aligned16(primary) || !aligned16(hits) || !aligned16(out))
    return set_err(RT_ERR_INVALID_ARG, "primary, hits or out not 16-byte aligned");
  if (p->_pad0 != 0u) return set_err(RT_ERR_INVALID_ARG, "_pad0 must be 0");
  return check_interval(p->tmin, p->radius);
}

int check_accumulate(const rt_raygen* g, const uint8_t* occ, uint64_t n, uint32_t channels,
                     uint32_t flags, const float* sums) {
  if (!g || !occ || !sums) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (n >= (1ull << 31)) return set_err(RT_ERR_INVALID_ARG, "n >= 2^31");
  if (channels != 1u && channels != 3u)
    return set_err(RT_ERR_INVALID_ARG, "channels must be 1 or 3");
  if (flags & ~RT_FLAG_OVERWRITE)
    return set_err(RT_ERR_INVALID_ARG, "the accumulation takes RT_FLAG_OVERWRITE only");
  return RT_OK;
}

int check_ao_frame(const rt_raygen* g, const rt_scene* sc, const rt_ao_frame_params* p,
                   const rt_ray* primary, uint64_t n, const float* sums, const rt_hit* hits_out) {
  if (!g || !sc || !p || !primary || !sums) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (n >= (1ull << 31)) return set_err(RT_ERR_INVALID_ARG, "n >= 2^31");
  if (!aligned16(primary) || !aligned16(hits_out))
    return set_err(RT_ERR_INVALID_ARG, "primary or hits_out not 16-byte aligned");
  if (p->directions == 0u) return set_err(RT_ERR_INVALID_ARG, "directions must be >= 1");
  if (p->channels != 1u && p->channels != 3u)
    return set_err(RT_ERR_INVALID_ARG, "channels must be 1 or 3");
  if (p->flags & ~(RT_FLAG_OVERWRITE | RT_FLAG_REFERENCE_BVH))
    return set_err(RT_ERR_INVALID_ARG,
                   "the AO frame takes RT_FLAG_OVERWRITE and RT_FLAG_REFERENCE_BVH only");
  return check_interval(p->tmin, p->radius);
}

// ---- launches (the handle's mutex held, its device set, the arguments checked)

int launch_projection(int kind, const ProjArgs& A, const PinArgs& C, rt_ray* rays,
                      hipStream_t stream) {
  hipLaunchKernelGGL(projection_kernel(kind), dim3(blocks_of(A.n)), dim3(kBlock), 0, stream, A, C,
                     reinterpret_cast<uint4*>(rays));
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int launch_ao_rays(uint64_t seed, double tmin, double radius, uint32_t dir_index,
                   const rt_ray* primary, const rt_hit* hits, uint64_t n, rt_ray* out,
                   hipStream_t stream) {
  hipLaunchKernelGGL(raygen_ao, dim3(blocks_of(n)), dim3(kBlock), 0, stream,
                     reinterpret_cast<const uint4*>(primary), reinterpret_cast<const uint4*>(hits),
                     reinterpret_cast<uint4*>(out), (uint32_t)n, (uint32_t)seed,
                     (uint32_t)(seed >> 32), tmin, radius, dir_index);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int launch_accumulate(const uint8_t* occ, uint64_t n, uint32_t channels, bool overwrite,
                      float* sums, hipStream_t stream) {
  hipLaunchKernelGGL(accumulate_kernel(channels, overwrite), dim3(blocks_of(n)), dim3(kBlock), 0,
                     stream, occ, sums, (uint32_t)n);
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

// One of the three single-launch calls: the run guard around `launch`, then the stats.
template <class Launch>
int run_one(rt_raygen* g, hipStream_t stream, rt_stats* stats, uint64_t samples,
            uint64_t out_bytes, time_point t0, Launch launch) {
  std::lock_guard<std::mutex> lock(g->mu);  // to the end: the stats events are the handle's
  HIP_TRY(hipSetDevice(g->device));
  {
    rts::Run run(*g, stream);
    RT_TRY(run.begin(stats != nullptr));
    RT_TRY(launch());
    if (stats) HIP_TRY(hipEventRecord(g->ev1, stream));
  }
  if (stats) RT_TRY(g->finish_stats(stream, stats, samples, out_bytes, 1u, t0));
  return RT_OK;
}

// The driver's own launches under stats != NULL: each between the handle's two events, waited
// for and added to *ms (the queries bring their own rt_stats). Without stats, the launch alone.
template <class Launch>
int timed(rt_raygen* g, hipStream_t stream, bool want, double* ms, Launch launch) {
  if (want) HIP_TRY(hipEventRecord(g->ev0, stream));
  RT_TRY(launch());
  if (!want) return RT_OK;
  HIP_TRY(hipEventRecord(g->ev1, stream));
  HIP_TRY(hipEventSynchronize(g->ev1));
  float one = 0.f;
  HIP_TRY(hipEventElapsedTime(&one, g->ev0, g->ev1));
  *ms += one;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_raygen_create(int device, rt_raygen** out) { return rts::stage_create(device, true, out); }

void rt_raygen_destroy(rt_raygen* g) { rts::stage_destroy(g); }

int rt_projection_rays_device(rt_raygen* g, const rt_projection* proj, const rt_camera* cam,
                              uint64_t seed, int32_t s_i, int32_t s_j, int32_t row_begin,
                              int32_t n_rows, rt_ray* rays, void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  ProjArgs A;
  PinArgs C;
  RT_TRY(check_projection(g, proj, cam, seed, s_i, s_j, row_begin, n_rows, rays, &A, &C));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (A.n == 0) return RT_OK;
  const hipStream_t stream = (hipStream_t)stream_v;
  const int kind = proj->kind;
  return run_one(g, stream, stats, A.n, (uint64_t)A.n * sizeof(rt_ray), t0,
                 [&] { return launch_projection(kind, A, C, rays, stream); });
}

int rt_ao_rays_device(rt_raygen* g, const rt_ao_params* p, const rt_ray* primary,
                      const rt_hit* hits, uint64_t n, rt_ray* out, void* stream_v,
                      rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  RT_TRY(check_ao_rays(g, p, primary, hits, n, out));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return RT_OK;
  const hipStream_t stream = (hipStream_t)stream_v;
  return run_one(g, stream, stats, n, n * sizeof(rt_ray), t0, [&] {
    return launch_ao_rays(p->seed, p->tmin, p->radius, p->dir_index, primary, hits, n, out, stream);
  });
}

int rt_ao_accumulate_device(rt_raygen* g, const uint8_t* occ, uint64_t n, uint32_t channels,
                            uint32_t flags, float* sums, void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  RT_TRY(check_accumulate(g, occ, n, channels, flags, sums));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return RT_OK;
  const hipStream_t stream = (hipStream_t)stream_v;
  return run_one(g, stream, stats, n, n * channels * sizeof(float), t0, [&] {
    return launch_accumulate(occ, n, channels, (flags & RT_FLAG_OVERWRITE) != 0, sums, stream);
  });
}

int rt_ambient_occlusion_device(rt_raygen* g, rt_scene* sc, const rt_ao_frame_params* p,
                                const rt_ray* primary, uint64_t n, float* sums, rt_hit* hits_out,
                                void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  RT_TRY(check_ao_frame(g, sc, p, primary, n, sums, hits_out));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return RT_OK;
  const hipStream_t stream = (hipStream_t)stream_v;
  const uint64_t chunk = std::min<uint64_t>(p->chunk_rays ? p->chunk_rays : kDefaultChunk, n);
  const uint32_t K = p->directions, ch = p->channels;
  const bool want = stats != nullptr;
  rt_query_params rec{}, any{};
  rec.seed = any.seed = p->seed;
  rec.flags = any.flags = p->flags & RT_FLAG_REFERENCE_BVH;
  any.mode = RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT;
  double ms = 0.0;
  uint32_t launches = 0;
  std::lock_guard<std::mutex> lock(g->mu);
  if (sc->device != g->device)
    return set_err(RT_ERR_INVALID_ARG, "the scene lives on another device than the handle");
  HIP_TRY(hipSetDevice(g->device));
  // [records, unless the caller takes them][AO rays][occlusion bytes]: 80 + 80 + 1 per ray
  const size_t rec_bytes = hits_out ? 0 : (size_t)chunk * sizeof(rt_hit);
  RT_TRY(g->reserve(rec_bytes + (size_t)chunk * (sizeof(rt_ray) + 1)));
  rt_ray* const ao = reinterpret_cast<rt_ray*>(g->work + rec_bytes);
  uint8_t* const occ = g->work + rec_bytes + (size_t)chunk * sizeof(rt_ray);
  {
    rts::Run run(*g, stream);
    RT_TRY(run.begin(false));
    rt_stats qs;
    for (uint64_t at = 0; at < n; at += chunk) {
      const uint64_t m = std::min(chunk, n - at);
      const rt_ray* prim = primary + at;
      rt_hit* hits = hits_out ? hits_out + at : reinterpret_cast<rt_hit*>(g->work);
      float* out = sums + at * ch;
      RT_TRY(rt_query_rays_device(sc, &rec, prim, m, hits, stream_v, want ? &qs : nullptr));
      if (want) ms += qs.ms_kernel;
      for (uint32_t k = 0; k < K; ++k) {
        RT_TRY(timed(g, stream, want, &ms, [&] {
          return launch_ao_rays(p->seed, p->tmin, p->radius, k, prim, hits, m, ao, stream);
        }));
        RT_TRY(rt_query_rays_device(sc, &any, ao, m, occ, stream_v, want ? &qs : nullptr));
        if (want) ms += qs.ms_kernel;
        const bool overwrite = k == 0 && (p->flags & RT_FLAG_OVERWRITE) != 0;
        RT_TRY(timed(g, stream, want, &ms,
                     [&] { return launch_accumulate(occ, m, ch, overwrite, out, stream); }));
      }
      launches += 1u + 3u * K;
    }
  }
  if (!want) return RT_OK;
  HIP_TRY(hipStreamSynchronize(stream));
  stats->ms_kernel = ms;
  stats->samples = n * K;
  stats->out_bytes = n * ch * sizeof(float) + (hits_out ? n * sizeof(rt_hit) : 0);
  stats->launches = launches;
  stats->ms_total = rts::ms_since(t0);
  return RT_OK;
}

}  // extern "C"
