// rt_temporal.h — device body of the temporal accumulation of include/rt_mi355x.h: one lane per
// pixel reprojects its first-hit point into the previous camera, gathers the history there with a
// bilinear footprint whose taps on another surface are rejected, blends and writes the next
// history. f64 for the projection, the four weights and the depth test, f32 for the rest; no
// atomics, taps in a fixed order: the same calls give the same bits. Ahead-of-time only
// (rt_temporal.hip); not one of the headers embedded for the scene-specialised kernels.
//
// History records, 16 B each, one array per kind (a wave's tap is three runs of consecutive 16-B
// loads, as in rt_denoise.h):
//   R0 = {Sr, Sg, Sb, L}   R1 = {nx, ny, nz, z}   R2 = {Qr, Qg, Qb, id}   (Q = 0 without moments)
// The four taps of neighbouring lanes overlap almost entirely, so they are plain global loads
// served by L1/L2; nothing is staged in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_mi355x.h"

namespace rtt {

constexpr int kTileW = 32, kTileH = 8, kBlock = kTileW * kTileH;  // 4 waves of 64, the denoiser's

constexpr uint32_t kHasHistory = 0x1u;      // TpParams::mode: the handle holds a frame of this size
constexpr uint32_t kVarianceOfMean = 0x2u;  // RT_TEMPORAL_VARIANCE_OF_MEAN

// Uniform over the launch: kernel arguments, so they stay in SGPRs.
struct TpParams {
  int W, H;
  uint32_t mode;
  float max_history;
  float normal_tol2;  // normal_tol^2, <= 0: test off
  float min_weight;
  double depth_tol;   // <= 0: test off
  double rows;        // beauty_rows (RT_TEMPORAL_VARIANCE_OF_MEAN)
  double p00c[3];     // pixel00_loc - center, this call's camera
  double du[3], dv[3];
  double cdiff[3];    // center - center'
  double minv[9];     // inverse of M', row-major: rows give s, a, b
};

__device__ __forceinline__ bool finite3(float a, float b, float c) {
  return isfinite(a) && isfinite(b) && isfinite(c);
}

// pixel of this lane: 32x8 tiles, row-major over the frame, on a one-dimensional grid
__device__ __forceinline__ bool lane_pixel(const TpParams& P, int* x, int* y) {
  const unsigned tiles_x = ((unsigned)P.W + kTileW - 1) / kTileW;
  const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  *x = (int)(tx * kTileW + (threadIdx.x & (kTileW - 1)));
  *y = (int)(ty * kTileH + (threadIdx.x >> 5));
  return *x < P.W && *y < P.H;
}

// The running sums of a pixel's gather, and one tap added to them. `in`: the tap lies in the
// frame (the caller passes an index it may read either way). A rejected tap is skipped by
// selection on the values, never by a product with 0: an invalid pixel's record may hold NaN.
struct Gather {
  float w = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, q0 = 0.f, q1 = 0.f, q2 = 0.f, len = 0.f;
};

template <bool M2>
__device__ __forceinline__ void add_tap(const TpParams& P, Gather& g, bool in, float w, float4 r0,
                                        float4 r1, float4 r2, float4 guide, float id, double s) {
  bool ok = in && r0.w >= 1.f && r1.w > 0.f && r2.w == id;
  if (P.normal_tol2 > 0.f) {
    const float d0 = r1.x - guide.x, d1 = r1.y - guide.y, d2 = r1.z - guide.z;
    ok = ok && fmaf(d2, d2, fmaf(d1, d1, d0 * d0)) <= P.normal_tol2;
  }
  if (P.depth_tol > 0.0) ok = ok && fabs((double)r1.w - s) <= P.depth_tol * s;
  if (!ok) return;
  g.w = g.w + w;
  g.s0 = fmaf(w, r0.x, g.s0);
  g.s1 = fmaf(w, r0.y, g.s1);
  g.s2 = fmaf(w, r0.z, g.s2);
  g.len = fmaf(w, r0.w, g.len);
  if (M2) {
    g.q0 = fmaf(w, r2.x, g.q0);
    g.q1 = fmaf(w, r2.y, g.q1);
    g.q2 = fmaf(w, r2.z, g.q2);
  }
}

// RT_TEMPORAL_VARIANCE_OF_MEAN for one channel: S^2 / n + max(0, Q - S^2 / n) / L
__device__ __forceinline__ float variance_of_mean(float S, float Q, float L, double rows) {
  const double m = ((double)S * (double)S) / rows;
  const double d = (double)Q - m;
  return (float)(m + (d > 0.0 ? d : 0.0) / (double)L);
}

// hin: the previous call's records (read only where P.mode has kHasHistory), hout: this call's;
// n_px apart per kind. out_b may be beauty and out_q may be m2: the lane reads its own pixel
// before it writes it, and no lane reads another's.
template <bool M2>
__device__ __forceinline__ void accumulate_body(const TpParams& P, const float* beauty,
                                                const float* m2, const float* __restrict__ aov,
                                                const float4* __restrict__ hin,
                                                float4* __restrict__ hout, float* out_b,
                                                float* out_q, float* __restrict__ hist_len) {
  int x, y;
  if (!lane_pixel(P, &x, &y)) return;
  const size_t n_px = (size_t)P.W * (size_t)P.H;
  const uint32_t p = (uint32_t)y * (uint32_t)P.W + (uint32_t)x;  // W * H < 2^31
  const float* b = beauty + (size_t)p * 3;
  const float* a = aov + (size_t)p * RT_AOV_CHANNELS;
  const float S0 = b[0], S1 = b[1], S2 = b[2];
  float Q0 = 0.f, Q1 = 0.f, Q2 = 0.f;
  if (M2) {
    const float* q = m2 + (size_t)p * 3;
    Q0 = q[0], Q1 = q[1], Q2 = q[2];
  }
  const float hits = a[RT_AOV_HITS], id = a[RT_AOV_MATID];
  float4 guide = make_float4(0.f, 0.f, 0.f, 0.f);  // {n, z}
  if (hits > 0.f) {
    guide.x = a[RT_AOV_NORMAL] / hits;
    guide.y = a[RT_AOV_NORMAL + 1] / hits;
    guide.z = a[RT_AOV_NORMAL + 2] / hits;
    guide.w = a[RT_AOV_T] / hits;
  }
  const bool valid = finite3(S0, S1, S2) && (!M2 || finite3(Q0, Q1, Q2));
  float o0 = S0, o1 = S1, o2 = S2, oq0 = Q0, oq1 = Q1, oq2 = Q2;  // the blended sums
  float v0 = Q0, v1 = Q1, v2 = Q2;                                // what out_m2 receives
  float L = valid ? 1.f : 0.f;
  if (valid && (P.mode & kHasHistory) && hits > 0.f) {
    const double di = (double)x, dj = (double)y, z = (double)guide.w;
    const double D0 = fma(dj, P.dv[0], fma(di, P.du[0], P.p00c[0]));
    const double D1 = fma(dj, P.dv[1], fma(di, P.du[1], P.p00c[1]));
    const double D2 = fma(dj, P.dv[2], fma(di, P.du[2], P.p00c[2]));
    const double V0 = fma(z, D0, P.cdiff[0]), V1 = fma(z, D1, P.cdiff[1]),
                 V2 = fma(z, D2, P.cdiff[2]);
    const double s = fma(P.minv[2], V2, fma(P.minv[1], V1, P.minv[0] * V0));
    const double ta = fma(P.minv[5], V2, fma(P.minv[4], V1, P.minv[3] * V0));
    const double tb = fma(P.minv[8], V2, fma(P.minv[7], V1, P.minv[6] * V0));
    const double xp = ta / s, yp = tb / s;
    const double fx0 = floor(xp), fy0 = floor(yp);
    // the comparisons are false for NaN; they keep i0, j0 in [-1, W) x [-1, H) before the
    // conversion to int: outside it no tap lies in the frame
    if (isfinite(s) && s > 0.0 && isfinite(xp) && isfinite(yp) && fx0 >= -1.0 &&
        fx0 < (double)P.W && fy0 >= -1.0 && fy0 < (double)P.H) {
      const int i0 = (int)fx0, j0 = (int)fy0;
      const double fx = xp - fx0, fy = yp - fy0;
      const float w[4] = {(float)((1.0 - fx) * (1.0 - fy)), (float)(fx * (1.0 - fy)),
                          (float)((1.0 - fx) * fy), (float)(fx * fy)};
      Gather g;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int qi = i0 + (t & 1), qj = j0 + (t >> 1);
        const bool in = qi >= 0 && qi < P.W && qj >= 0 && qj < P.H;
        const uint32_t q = in ? (uint32_t)qj * (uint32_t)P.W + (uint32_t)qi : p;
        add_tap<M2>(P, g, in, w[t], hin[q], hin[n_px + q], hin[2 * n_px + q], guide, id, s);
      }
      if (g.w > P.min_weight) {
        const float Lh = g.len / g.w;
        L = fminf(Lh + 1.f, P.max_history);
        const float alpha = 1.f / L, keep = 1.f - alpha;
        o0 = fmaf(alpha, S0, keep * (g.s0 / g.w));
        o1 = fmaf(alpha, S1, keep * (g.s1 / g.w));
        o2 = fmaf(alpha, S2, keep * (g.s2 / g.w));
        if (M2) {
          oq0 = fmaf(alpha, Q0, keep * (g.q0 / g.w));
          oq1 = fmaf(alpha, Q1, keep * (g.q1 / g.w));
          oq2 = fmaf(alpha, Q2, keep * (g.q2 / g.w));
          v0 = oq0, v1 = oq1, v2 = oq2;
          if (P.mode & kVarianceOfMean) {
            v0 = variance_of_mean(o0, oq0, L, P.rows);
            v1 = variance_of_mean(o1, oq1, L, P.rows);
            v2 = variance_of_mean(o2, oq2, L, P.rows);
          }
        }
      }
    }
  }
  hout[p] = make_float4(o0, o1, o2, L);
  hout[n_px + p] = guide;
  hout[2 * n_px + p] = make_float4(oq0, oq1, oq2, id);
  float* ob = out_b + (size_t)p * 3;
  ob[0] = o0, ob[1] = o1, ob[2] = o2;
  if (M2) {
    float* oq = out_q + (size_t)p * 3;
    oq[0] = v0, oq[1] = v1, oq[2] = v2;
  }
  if (hist_len) hist_len[p] = L;
}

}  // namespace rtt
