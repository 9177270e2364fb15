// rt_output.hip — the output stage on the device (include/rt_mi355x.h): auto_expose
// (render.rs:325-339) as a fixed-order f64 reduction, write_color (color.rs:8-59) one lane per
// pixel, and the rt_output_stage handle. The host's rth_auto_expose and rth_write_color
// (host/capi.cpp) are the definition; the expressions below are theirs, in their order. Its own
// translation unit; of scenes it knows nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>

#include "rt_mi355x.h"
#include "rt_stage.hpp"

using rts::set_err;
using rts::time_point;

// The workspace holds doubles: [0] the exposure, [1 ..] one partial sum per reduction block.
struct rt_output_stage : rts::Stage {};

namespace {

constexpr int kBlock = 256;
constexpr int kPerLane = 8;  // pixels a lane of out_expose_partial adds serially
constexpr uint32_t kKnownFlags = RT_OUTPUT_EXPOSURE | RT_OUTPUT_AUTO_EXPOSE | RT_OUTPUT_RGBA;

// the block's sum over its lanes in a fixed tree: lane t += lane t + s for s = 128, 64, .. 1
__device__ double block_tree(double v, double* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (t < s) lds[t] = lds[t] + lds[t + s];
    __syncthreads();
  }
  return lds[0];
}

// Block b owns pixels [b * 2048, (b + 1) * 2048); lane t adds pixels b * 2048 + k * 256 + t,
// k = 0 .. 7 in that order, each term weight * lum^2 as rth_auto_expose forms it.
__global__ __launch_bounds__(kBlock) void out_expose_partial(const float* __restrict__ sums,
                                                             double* __restrict__ partial,
                                                             size_t n_px, double weight) {
  __shared__ double lds[kBlock];
  const size_t base = (size_t)blockIdx.x * (kBlock * kPerLane) + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const size_t p = base + (size_t)k * kBlock;
    if (p < n_px) {
      const double lum = 0.2126 * (double)sums[3 * p] + 0.71516 * (double)sums[3 * p + 1] +
                         0.072169 * (double)sums[3 * p + 2];
      acc = acc + weight * (lum * lum);
    }
  }
  const double total = block_tree(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// One block. Lane t adds partials t, t + 256, .. in ascending block order, then the same tree;
// lane 0 forms the exposure. neg_ln06 is the host's -ln(0.6): the device takes no logarithm.
__global__ __launch_bounds__(kBlock) void out_expose_final(const double* __restrict__ partial,
                                                           double* __restrict__ ev_out,
                                                           uint32_t n_blocks, double spp2,
                                                           double neg_ln06) {
  __shared__ double lds[kBlock];
  double acc = 0.0;
  for (uint32_t b = threadIdx.x; b < n_blocks; b += kBlock) acc = acc + partial[b];
  const double total = block_tree(acc, lds);
  if (threadIdx.x == 0) {
    const double m = total / spp2;
    *ev_out = m > 0.001 ? neg_ln06 / sqrt(m) : 1.0;  // NaN fails the test: 1
  }
}

__device__ double linear_to_gamma(double linear) {  // color.rs:53-59
  if (linear <= 0.0031308) return 12.92 * linear;
  return 1.055 * pow(linear, 1. / 2.4) - 0.055;
}

// one value of write_color: scale, exposure, gamma, clamp, Rust's saturating `as u8`
template <bool EXPOSE>
__device__ uint32_t to_u8(float sum, double scale, double ev) {
  double x = (double)sum * scale;
  if (EXPOSE) x = 1. - pow(2.718281828459045, -ev * x);  // color.rs:37-39
  x = linear_to_gamma(x);
  if (x < 0.) x = 0.;             // Interval{0, 0.999}.clamp
  else if (x > 0.999) x = 0.999;  // NaN falls through both tests
  const double y = 256. * x;
  if (!(y == y) || y <= 0.) return 0u;
  if (y >= 255.) return 255u;
  return (uint32_t)y;
}

// One lane per pixel. STRIDE 3: three byte stores; STRIDE 4: alpha 255, one 32-bit store where
// the buffer is 4-byte aligned (uniform over the launch), four byte stores where it is not.
// ev_dev != null: the exposure out_expose_final left in the workspace.
template <int STRIDE, bool EXPOSE>
__global__ __launch_bounds__(kBlock) void out_write(const float* __restrict__ sums,
                                                    uint8_t* __restrict__ out, size_t n_px,
                                                    double scale, double ev_arg,
                                                    const double* __restrict__ ev_dev) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n_px) return;
  const double ev = EXPOSE && ev_dev ? *ev_dev : ev_arg;
  const uint32_t r = to_u8<EXPOSE>(sums[3 * p], scale, ev);
  const uint32_t g = to_u8<EXPOSE>(sums[3 * p + 1], scale, ev);
  const uint32_t b = to_u8<EXPOSE>(sums[3 * p + 2], scale, ev);
  uint8_t* o = out + STRIDE * p;
  if (STRIDE == 4 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(o) = r | (g << 8) | (b << 16) | 0xff000000u;
    return;
  }
  o[0] = (uint8_t)r, o[1] = (uint8_t)g, o[2] = (uint8_t)b;
  if (STRIDE == 4) o[3] = 255;
}

typedef void (*write_kern_t)(const float*, uint8_t*, size_t, double, double, const double*);
write_kern_t write_kernel(bool rgba, bool expose) {
  if (rgba) return expose ? out_write<4, true> : out_write<4, false>;
  return expose ? out_write<3, true> : out_write<3, false>;
}

// everything that can be judged without the handle and without HIP
int check_args(const rt_output_stage* o, const rt_output_params* p, const float* sums,
               const uint8_t* rgb8) {
  if (!o || !p || !sums || !rgb8) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (p->width <= 0 || p->height < 0)
    return set_err(RT_ERR_INVALID_ARG, "bad frame size (width <= 0 or height < 0)");
  if ((int64_t)p->width * p->height >= (1ll << 31))
    return set_err(RT_ERR_INVALID_ARG, "frame too large (width * height >= 2^31)");
  if (p->flags & ~kKnownFlags) return set_err(RT_ERR_INVALID_ARG, "unknown RT_OUTPUT_* flag bits");
  if (p->_pad0 != 0) return set_err(RT_ERR_INVALID_ARG, "_pad0 must be 0");
  if (!std::isfinite(p->samples_per_pixel) || p->samples_per_pixel <= 0.0)
    return set_err(RT_ERR_INVALID_ARG, "samples_per_pixel must be finite and > 0");
  if ((p->flags & (RT_OUTPUT_EXPOSURE | RT_OUTPUT_AUTO_EXPOSE)) == RT_OUTPUT_EXPOSURE &&
      !std::isfinite(p->exposure))
    return set_err(RT_ERR_INVALID_ARG, "exposure must be finite");
  return RT_OK;
}

// the arguments checked, at least one pixel
int output_device(rt_output_stage* o, const rt_output_params* p, const float* sums, uint8_t* rgb8,
                  double* exposure_out, hipStream_t stream, rt_stats* stats, time_point t0) {
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  const bool autoexp = (p->flags & RT_OUTPUT_AUTO_EXPOSE) != 0;
  const bool expose = autoexp || (p->flags & RT_OUTPUT_EXPOSURE) != 0;
  const bool rgba = (p->flags & RT_OUTPUT_RGBA) != 0;
  // held to the end of the call, through the synchronisation that stats or exposure_out ask
  // for: the stats events are the handle's
  std::lock_guard<std::mutex> lock(o->mu);
  HIP_TRY(hipSetDevice(o->device));
  const size_t n_blocks = (n_px + kBlock * kPerLane - 1) / (kBlock * kPerLane);  // < 2^20
  if (autoexp) RT_TRY(o->reserve((n_blocks + 1) * sizeof(double)));
  double* const work = reinterpret_cast<double*>(o->work);
  double ev_host = expose && !autoexp ? p->exposure : 0.0;
  {
    rts::Run run(*o, stream);
    RT_TRY(run.begin(stats != nullptr));
    if (autoexp) {
      hipLaunchKernelGGL(out_expose_partial, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream,
                         sums, work + 1, n_px, 1. / (double)n_px);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(out_expose_final, dim3(1), dim3(kBlock), 0, stream, work + 1, work,
                         (uint32_t)n_blocks, p->samples_per_pixel * p->samples_per_pixel,
                         -std::log(0.6));
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(write_kernel(rgba, expose), dim3((unsigned)((n_px + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, stream, sums, rgb8, n_px, 1.0 / p->samples_per_pixel,
                       ev_host, autoexp ? work : nullptr);
    HIP_TRY(hipGetLastError());
    if (stats) HIP_TRY(hipEventRecord(o->ev1, stream));
    if (autoexp && exposure_out)
      HIP_TRY(hipMemcpyAsync(&ev_host, work, sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  if (stats)
    RT_TRY(o->finish_stats(stream, stats, n_px, (uint64_t)n_px * (rgba ? 4 : 3), autoexp ? 3u : 1u,
                           t0));
  else if (exposure_out)
    HIP_TRY(hipStreamSynchronize(stream));
  if (exposure_out) *exposure_out = ev_host;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_output_create(int device, rt_output_stage** out) {
  return rts::stage_create(device, true, out);
}

void rt_output_destroy(rt_output_stage* o) { rts::stage_destroy(o); }

int rt_output_device(rt_output_stage* o, const rt_output_params* p, const float* sums, uint8_t* rgb8,
                     double* exposure_out, void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  const int rc = check_args(o, p, sums, rgb8);
  if (rc != RT_OK) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (p->height == 0) return RT_OK;
  return output_device(o, p, sums, rgb8, exposure_out, (hipStream_t)stream_v, stats, t0);
}

int rt_output(rt_output_stage* o, const rt_output_params* p, const float* sums, uint8_t* rgb8,
              double* exposure_out, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  const int rc = check_args(o, p, sums, rgb8);
  if (rc != RT_OK) return rc;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (p->height == 0) return RT_OK;
  const size_t n_px = (size_t)p->width * (size_t)p->height;
  const size_t in_bytes = n_px * 3 * sizeof(float);
  const size_t out_bytes = n_px * ((p->flags & RT_OUTPUT_RGBA) ? 4 : 3);
  rts::Staging st;
  const int i_sums = st.add(in_bytes), i_rgb = st.add(out_bytes);
  RT_TRY(st.alloc(o->device));
  RT_TRY(st.upload(i_sums, sums));
  rt_stats local;
  RT_TRY(output_device(o, p, st.ptr<const float>(i_sums), st.ptr<uint8_t>(i_rgb), exposure_out,
                       nullptr, stats ? stats : &local, t0));
  RT_TRY(st.download(i_rgb, rgb8));
  if (stats) stats->ms_total = rts::ms_since(t0);
  return RT_OK;
}

}  // extern "C"
