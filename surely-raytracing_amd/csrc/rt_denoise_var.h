// rt_denoise_var.h — device body of the variance-guided a-trous denoiser (include/rt_mi355x.h,
// "variance-guided a-trous denoiser"): the filter of rt_denoise.h with the colour distance
// normalised by a per-pixel variance that the levels propagate (SVGF, Schied et al. 2017). Same
// discipline: f32 (the variance estimate alone is formed in f64, once per pixel), no atomics,
// weight 0 by selection, taps in a fixed order, the same bits on every call. The records are those
// of rt_denoise.h with the colour record's fourth lane in use:
//   G0 = {nx, ny, nz, z}   G1 = {ax, ay, az, valid}   X = {xr, xg, xb, v}
// so a tap loads nothing more than the plain filter's. Ahead-of-time only (rt_denoise.hip).
#pragma once
#include "rt_denoise.h"

namespace rtd {

constexpr float kVarEps = 1e-10f;  // v_p + v_q + 1e-10

struct DnVarParams {
  DnParams d;     // k_color: log2(e) / sigma_color^2, the same at every level
  double n;       // beauty_rows
  double vscale;  // n / ((n - 1) B^2)
};

// prepare_body plus the pixel's raw variance in X.w:
//   var_c = max(0, Q_c - S_c^2 / n) * n / ((n - 1) B^2)   in f64 (the difference cancels)
//   v_raw = sum_c var_c / m_c^2 (demodulating) or sum_c var_c, rounded once to f32
__device__ __forceinline__ void prepare_var_body(const DnVarParams& V,
                                                 const float* __restrict__ beauty,
                                                 const float* __restrict__ m2,
                                                 const float* __restrict__ aov,
                                                 float4* __restrict__ G0, float4* __restrict__ G1,
                                                 float4* __restrict__ X) {
  const DnParams& P = V.d;
  int x, y;
  if (!lane_pixel(P, &x, &y)) return;
  const size_t p = (size_t)y * P.W + x;
  const float* b = beauty + p * 3;
  const float* qq = m2 + p * 3;
  const float* g = aov + p * RT_AOV_CHANNELS;
  const float s0 = b[0], s1 = b[1], s2 = b[2];
  const float q0 = qq[0], q1 = qq[1], q2 = qq[2];
  const float c0 = s0 / P.B, c1 = s1 / P.B, c2 = s2 / P.B;
  const float hits = g[RT_AOV_HITS];
  float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (hits > 0.f) {
    g0.x = g[RT_AOV_NORMAL] / hits;
    g0.y = g[RT_AOV_NORMAL + 1] / hits;
    g0.z = g[RT_AOV_NORMAL + 2] / hits;
    g0.w = g[RT_AOV_T] / hits;
  }
  const float a0 = g[RT_AOV_ALBEDO] / P.A, a1 = g[RT_AOV_ALBEDO + 1] / P.A,
              a2 = g[RT_AOV_ALBEDO + 2] / P.A;
  float x0 = c0, x1 = c1, x2 = c2;
  double v0 = fmax(0.0, (double)q0 - (double)s0 * (double)s0 / V.n) * V.vscale;
  double v1 = fmax(0.0, (double)q1 - (double)s1 * (double)s1 / V.n) * V.vscale;
  double v2 = fmax(0.0, (double)q2 - (double)s2 * (double)s2 / V.n) * V.vscale;
  if (P.flags & RT_DENOISE_DEMODULATE) {
    const float m0 = fmaxf(a0, kAlbedoFloor), m1 = fmaxf(a1, kAlbedoFloor),
                mm2 = fmaxf(a2, kAlbedoFloor);
    x0 = (c0 - g[RT_AOV_EMISSION] / P.A) / m0;
    x1 = (c1 - g[RT_AOV_EMISSION + 1] / P.A) / m1;
    x2 = (c2 - g[RT_AOV_EMISSION + 2] / P.A) / mm2;
    v0 = v0 / ((double)m0 * (double)m0);
    v1 = v1 / ((double)m1 * (double)m1);
    v2 = v2 / ((double)mm2 * (double)mm2);
  }
  const float v = (float)((v0 + v1) + v2);
  // fmax drops a NaN operand, so a non-finite Q is asked for by itself
  const bool valid = finite3(x0, x1, x2) && finite3(q0, q1, q2) && isfinite(v);
  G0[p] = g0;
  G1[p] = make_float4(a0, a1, a2, valid ? 1.f : 0.f);
  X[p] = valid ? make_float4(x0, x1, x2, v) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ constexpr float g3(int i) { return i == 0 ? 1.f / 2.f : 1.f / 4.f; }

// SVGF's 3x3 prefilter of the raw variance over the valid in-frame neighbours (j outer, i inner);
// the colour passes through. Nine 16-B loads of each of two records per lane, through L1: a
// fraction of one level's traffic.
__device__ __forceinline__ void prefilter_body(const DnParams& P, const float4* __restrict__ G1,
                                               const float4* __restrict__ Xin,
                                               float4* __restrict__ Xout) {
  int x, y;
  if (!lane_pixel(P, &x, &y)) return;
  const uint32_t p = (uint32_t)y * (uint32_t)P.W + (uint32_t)x;
  float4 xp = Xin[p];
  if (G1[p].w == 0.f) {
    Xout[p] = xp;  // all zero
    return;
  }
  float sv = 0.f, sg = 0.f;
#pragma unroll
  for (int j = -1; j <= 1; ++j) {
    const bool in_y = tap_inside(y, P.H, j);
    const uint32_t row = p + (uint32_t)j * (uint32_t)P.W;
#pragma unroll
    for (int i = -1; i <= 1; ++i) {
      const bool ok = in_y && tap_inside(x, P.W, i);
      const uint32_t q = ok ? row + (uint32_t)i : p;
      float w = g3(i) * g3(j);
      w = (ok && G1[q].w != 0.f) ? w : 0.f;
      sv = fmaf(w, Xin[q].w, sv);
      sg += w;
    }
  }
  xp.w = sv / sg;  // the centre alone gives sg = 1/4
  Xout[p] = xp;
}

// TapSums plus the variance sum: sv = sum w^2 v_q
struct TapSumsVar {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, sw = 0.f, sv = 0.f;
};
// tap_add of rt_denoise.h with the colour term divided by v_p + v_q + 1e-10 (a second v_rcp_f32,
// 1 ulp; still one v_exp_f32 per tap) and w^2 v_q accumulated
__device__ __forceinline__ void tap_add_var(const DnParams& P, const float4& g0p,
                                            const float4& g1p, const float4& xp, float zp2,
                                            const float4& g0q, const float4& g1q,
                                            const float4& xq, float hw, bool ok, TapSumsVar& S) {
  const float dx0 = xp.x - xq.x, dx1 = xp.y - xq.y, dx2 = xp.z - xq.z;
  const float dn0 = g0p.x - g0q.x, dn1 = g0p.y - g0q.y, dn2 = g0p.z - g0q.z;
  const float da0 = g1p.x - g1q.x, da1 = g1p.y - g1q.y, da2 = g1p.z - g1q.z;
  const float dz = g0p.w - g0q.w;
  const float zz = fmaxf(fmaxf(zp2, g0q.w * g0q.w), kDepthFloor);
  const float vv = (xp.w + xq.w) + kVarEps;
  float E = fmaf(dx2, dx2, fmaf(dx1, dx1, dx0 * dx0)) * P.k_color * __builtin_amdgcn_rcpf(vv);
  E = fmaf(fmaf(dn2, dn2, fmaf(dn1, dn1, dn0 * dn0)), P.k_normal, E);
  E = fmaf(fmaf(da2, da2, fmaf(da1, da1, da0 * da0)), P.k_albedo, E);
  E = fmaf(dz * dz * P.k_depth, __builtin_amdgcn_rcpf(zz), E);
  float w = hw * __builtin_amdgcn_exp2f(-E);
  w = (ok && g1q.w != 0.f) ? w : 0.f;
  S.s0 = fmaf(w, xq.x, S.s0);
  S.s1 = fmaf(w, xq.y, S.s1);
  S.s2 = fmaf(w, xq.z, S.s2);
  S.sv = fmaf(w * w, xq.w, S.sv);
  S.sw += w;
}

// the end of a level for a valid pixel: x_{k+1} and v_{k+1} = sv / sw^2
template <bool FINAL>
__device__ __forceinline__ void level_store_var(const DnParams& P, const float4& g1p,
                                                const TapSumsVar& S, uint32_t p, float4* Xout,
                                                const float* __restrict__ aov, float* out,
                                                float* var_out) {
  const float r0 = S.s0 / S.sw, r1 = S.s1 / S.sw, r2 = S.s2 / S.sw;
  const float v = S.sv / (S.sw * S.sw);
  if (FINAL) {
    final_store(P, g1p, r0, r1, r2, p, aov, out);
    if (var_out) var_out[p] = v;
  } else {
    Xout[p] = make_float4(r0, r1, r2, v);
  }
}

template <bool FINAL>
__device__ __forceinline__ void invalid_pass_var(uint32_t p, const float4* __restrict__ Xin,
                                                 float4* Xout, const float* beauty, float* out,
                                                 float* var_out) {
  invalid_pass<FINAL>(p, Xin, Xout, beauty, out);
  if (FINAL && var_out) var_out[p] = 0.f;
}

// atrous_body with the variance lane
template <bool FINAL>
__device__ __forceinline__ void atrous_var_body(const DnParams& P, const float4* __restrict__ G0,
                                                const float4* __restrict__ G1,
                                                const float4* __restrict__ Xin, float4* Xout,
                                                const float* beauty,
                                                const float* __restrict__ aov, float* out,
                                                float* var_out) {
  int x, y;
  if (!lane_pixel(P, &x, &y)) return;
  const uint32_t p = (uint32_t)y * (uint32_t)P.W + (uint32_t)x;
  const float4 g1p = G1[p];
  if (g1p.w == 0.f) {
    invalid_pass_var<FINAL>(p, Xin, Xout, beauty, out, var_out);
    return;
  }
  const float4 g0p = G0[p];
  const float4 xp = Xin[p];
  const float zp2 = g0p.w * g0p.w;
  TapSumsVar S;
#pragma unroll
  for (int j = -2; j <= 2; ++j) {
    const bool in_y = tap_inside(y, P.H, j * P.step);
    const uint32_t row = p + (uint32_t)(j * P.step) * (uint32_t)P.W;
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
      const bool ok = in_y && tap_inside(x, P.W, i * P.step);
      const uint32_t q = ok ? row + (uint32_t)(i * P.step) : p;
      tap_add_var(P, g0p, g1p, xp, zp2, G0[q], G1[q], Xin[q], b3(i) * b3(j), ok, S);
    }
  }
  level_store_var<FINAL>(P, g1p, S, p, Xout, aov, out, var_out);
}

// atrous_tiled_body with the variance lane: the same TileLds (the colour record already has the
// lane), the same staging, so the same 30 KB at STEP 2
template <int STEP, bool FINAL>
__device__ __forceinline__ void atrous_var_tiled_body(const DnParams& P, TileLds<STEP>& L,
                                                      const float4* __restrict__ G0,
                                                      const float4* __restrict__ G1,
                                                      const float4* __restrict__ Xin,
                                                      float4* Xout, const float* beauty,
                                                      const float* __restrict__ aov, float* out,
                                                      float* var_out) {
  constexpr int RW = TileLds<STEP>::RW, N = TileLds<STEP>::N, HALO = 2 * STEP;
  int x, y;
  const bool inside = lane_pixel(P, &x, &y);
  const int lx = (int)(threadIdx.x & (kTileW - 1)), ly = (int)(threadIdx.x >> 5);
  const int x0 = x - lx - HALO, y0 = y - ly - HALO;  // the region's first pixel (may be < 0)
  for (int r = (int)threadIdx.x; r < N; r += kBlock) {
    const int ry = r / RW, rx = r - ry * RW;
    const int gx = x0 + rx, gy = y0 + ry;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
    if (gx >= 0 && gx < P.W && gy >= 0 && gy < P.H) {
      const uint32_t q = (uint32_t)gy * (uint32_t)P.W + (uint32_t)gx;
      a = G0[q];
      b = G1[q];
      c = Xin[q];
    }
    L.g0[r] = a;
    L.g1[r] = b;
    L.x[r] = c;
  }
  __syncthreads();
  if (!inside) return;
  const uint32_t p = (uint32_t)y * (uint32_t)P.W + (uint32_t)x;
  const int c = (ly + HALO) * RW + lx + HALO;
  const float4 g1p = L.g1[c];
  if (g1p.w == 0.f) {
    invalid_pass_var<FINAL>(p, Xin, Xout, beauty, out, var_out);
    return;
  }
  const float4 g0p = L.g0[c];
  const float4 xp = L.x[c];
  const float zp2 = g0p.w * g0p.w;
  TapSumsVar S;
#pragma unroll
  for (int j = -2; j <= 2; ++j) {
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
      const int q = c + j * STEP * RW + i * STEP;
      tap_add_var(P, g0p, g1p, xp, zp2, L.g0[q], L.g1[q], L.x[q], b3(i) * b3(j), true, S);
    }
  }
  level_store_var<FINAL>(P, g1p, S, p, Xout, aov, out, var_out);
}

}  // namespace rtd
