// rt_denoise.h — device body of the two edge-avoiding a-trous denoisers of include/rt_mi355x.h:
// the plain one (Dammertz et al. 2010) and, with VAR, the variance-guided one, whose colour distance
// is normalised by a per-pixel variance that the levels propagate (SVGF, Schied et al. 2017). f32
// throughout (the variance estimate alone is formed in f64, once per pixel), no atomics, taps in a
// fixed order (j outer, i inner): the same inputs give the same bits on every call. Ahead-of-time
// only (rt_denoise.hip); not one of the headers embedded for the scene-specialised kernels.
//
// Workspace records, 16 B each, one array per kind so that a wave's tap is three runs of
// consecutive 16-B loads (a wave covers two 32-pixel row segments of its 32x8 tile):
//   G0 = {nx, ny, nz, z}   G1 = {ax, ay, az, valid}   X = {xr, xg, xb, v}   (v = 0 without VAR)
// so a tap of the variance-guided filter loads nothing more than the plain filter's.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rt_mi355x.h"

namespace rtd {

constexpr int kTileW = 32, kTileH = 8, kBlock = kTileW * kTileH;  // 4 waves of 64
constexpr float kAlbedoFloor = 1e-3f;   // m = max(a, 1e-3)
constexpr float kDepthFloor = 1e-30f;   // max(z_p^2, z_q^2, 1e-30)
constexpr float kVarEps = 1e-10f;       // v_p + v_q + 1e-10

struct DnParams {
  int W, H;
  int step;           // 2^k of this level
  uint32_t flags;     // RT_DENOISE_*
  float B;            // beauty_samples
  float A;            // aov_samples
  // log2(e) / sigma^2 per term, 0 = term off; the colour term is sigma_c * 2^-k at level k of the
  // plain filter, sigma_c at every level with VAR
  float k_color, k_normal, k_depth, k_albedo;
};

struct DnVarParams {
  DnParams d;
  double n;       // beauty_rows
  double vscale;  // n / ((n - 1) B^2)
};

__device__ __forceinline__ bool finite3(float a, float b, float c) {
  return isfinite(a) && isfinite(b) && isfinite(c);
}

// pixel of this lane: 32x8 tiles, row-major over the frame; the grid is one-dimensional so that
// no frame height meets a grid limit
__device__ __forceinline__ bool lane_pixel(const DnParams& P, int* x, int* y) {
  const unsigned tiles_x = ((unsigned)P.W + kTileW - 1) / kTileW;
  const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  *x = (int)(tx * kTileW + (threadIdx.x & (kTileW - 1)));
  *y = (int)(ty * kTileH + (threadIdx.x >> 5));
  return *x < P.W && *y < P.H;
}

// one lane per pixel: the user buffers (dword loads: they need no more than 4-byte alignment)
// -> the three records
__device__ __forceinline__ void prepare_body(const DnParams& P, const float* __restrict__ beauty,
                                             const float* __restrict__ aov,
                                             float4* __restrict__ G0, float4* __restrict__ G1,
                                             float4* __restrict__ X) {
  int x, y;
  if (!lane_pixel(P, &x, &y)) return;
  const size_t p = (size_t)y * P.W + x;
  const float* b = beauty + p * 3;
  const float* g = aov + p * RT_AOV_CHANNELS;
  const float c0 = b[0] / P.B, c1 = b[1] / P.B, c2 = b[2] / P.B;
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
  if (P.flags & RT_DENOISE_DEMODULATE) {
    x0 = (c0 - g[RT_AOV_EMISSION] / P.A) / fmaxf(a0, kAlbedoFloor);
    x1 = (c1 - g[RT_AOV_EMISSION + 1] / P.A) / fmaxf(a1, kAlbedoFloor);
    x2 = (c2 - g[RT_AOV_EMISSION + 2] / P.A) / fmaxf(a2, kAlbedoFloor);
  }
  const bool valid = finite3(x0, x1, x2);
  G0[p] = g0;
  G1[p] = make_float4(a0, a1, a2, valid ? 1.f : 0.f);
  // an invalid pixel's colour is never read for a sum (its weight is selected to 0, and 0 * 0
  // keeps the sums finite)
  X[p] = valid ? make_float4(x0, x1, x2, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

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

// is x + d inside [0, n)? (no x + d: it may not fit an int for the widest frames)
__device__ __forceinline__ bool tap_inside(int x, int n, int d) {
  return d >= 0 ? d < n - x : -d <= x;
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

// The running sums of one pixel's level, and one tap added to them. `hw` = h[i] h[j]; `ok` =
// the tap is inside the frame (the caller then passes the records of a pixel it may read, the
// centre's for instance). A tap that is outside or on an invalid pixel gets weight 0 by selection,
// not by a branch, so that a wave's 75 loads can be in flight together; an invalid pixel's colour
// record is 0, so 0 * x adds nothing. fma is written out (the build has contraction off).
// VAR: the colour term is divided by v_p + v_q + 1e-10 (a second v_rcp_f32, 1 ulp; still one
// v_exp_f32 per tap) and sv = sum w^2 v_q is accumulated.
struct TapSums {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, sw = 0.f, sv = 0.f;  // sv: VAR only
};
template <bool VAR>
__device__ __forceinline__ void tap_add(const DnParams& P, const float4& g0p, const float4& g1p,
                                        const float4& xp, float zp2, const float4& g0q,
                                        const float4& g1q, const float4& xq, float hw, bool ok,
                                        TapSums& S) {
  const float dx0 = xp.x - xq.x, dx1 = xp.y - xq.y, dx2 = xp.z - xq.z;
  const float dn0 = g0p.x - g0q.x, dn1 = g0p.y - g0q.y, dn2 = g0p.z - g0q.z;
  const float da0 = g1p.x - g1q.x, da1 = g1p.y - g1q.y, da2 = g1p.z - g1q.z;
  const float dz = g0p.w - g0q.w;
  const float zz = fmaxf(fmaxf(zp2, g0q.w * g0q.w), kDepthFloor);
  float E = fmaf(dx2, dx2, fmaf(dx1, dx1, dx0 * dx0)) * P.k_color;
  if (VAR) E = E * __builtin_amdgcn_rcpf((xp.w + xq.w) + kVarEps);
  E = fmaf(fmaf(dn2, dn2, fmaf(dn1, dn1, dn0 * dn0)), P.k_normal, E);
  E = fmaf(fmaf(da2, da2, fmaf(da1, da1, da0 * da0)), P.k_albedo, E);
  E = fmaf(dz * dz * P.k_depth, __builtin_amdgcn_rcpf(zz), E);  // v_rcp_f32: 1 ulp
  // v_exp_f32 (1 ulp); a result below the normal range may be flushed: a weight < 2^-126
  float w = hw * __builtin_amdgcn_exp2f(-E);
  w = (ok && g1q.w != 0.f) ? w : 0.f;
  S.s0 = fmaf(w, xq.x, S.s0);
  S.s1 = fmaf(w, xq.y, S.s1);
  S.s2 = fmaf(w, xq.z, S.s2);
  if (VAR) S.sv = fmaf(w * w, xq.w, S.sv);
  S.sw += w;
}

__device__ __forceinline__ constexpr float b3(int i) {
  return i == 0 ? 3.f / 8.f : (i == 1 || i == -1) ? 1.f / 4.f : 1.f / 16.f;
}

// The end of the last level for a valid pixel: re-modulate, scale to sums, store.
__device__ __forceinline__ void final_store(const DnParams& P, const float4& g1p, float r0,
                                            float r1, float r2, uint32_t p,
                                            const float* __restrict__ aov, float* out) {
  if (P.flags & RT_DENOISE_DEMODULATE) {
    const float* g = aov + (size_t)p * RT_AOV_CHANNELS;
    r0 = fmaf(r0, fmaxf(g1p.x, kAlbedoFloor), g[RT_AOV_EMISSION] / P.A);
    r1 = fmaf(r1, fmaxf(g1p.y, kAlbedoFloor), g[RT_AOV_EMISSION + 1] / P.A);
    r2 = fmaf(r2, fmaxf(g1p.z, kAlbedoFloor), g[RT_AOV_EMISSION + 2] / P.A);
  }
  float* o = out + (size_t)p * 3;
  o[0] = r0 * P.B;
  o[1] = r1 * P.B;
  o[2] = r2 * P.B;
}

// The end of a level for a valid pixel: x_{k+1} and, with VAR, v_{k+1} = sv / sw^2. The centre
// tap alone gives sw = 9/64. FINAL: the last level re-modulates and writes the user's output
// (and var_out, where given) instead of the next colour record.
template <bool VAR, bool FINAL>
__device__ __forceinline__ void level_store(const DnParams& P, const float4& g1p, const TapSums& S,
                                            uint32_t p, float4* Xout,
                                            const float* __restrict__ aov, float* out,
                                            float* var_out) {
  const float r0 = S.s0 / S.sw, r1 = S.s1 / S.sw, r2 = S.s2 / S.sw;
  const float v = VAR ? S.sv / (S.sw * S.sw) : 0.f;
  if (FINAL) {
    final_store(P, g1p, r0, r1, r2, p, aov, out);
    if (VAR && var_out) var_out[p] = v;
  } else {
    Xout[p] = make_float4(r0, r1, r2, v);
  }
}

// An invalid pixel passes through every level untouched; the last level copies the bits of its
// beauty sums (`out` may be `beauty`) and, with VAR, reports a variance of 0.
template <bool VAR, bool FINAL>
__device__ __forceinline__ void invalid_pass(uint32_t p, const float4* __restrict__ Xin,
                                             float4* Xout, const float* beauty, float* out,
                                             float* var_out) {
  if (FINAL) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(beauty) + (size_t)p * 3;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out) + (size_t)p * 3;
    const uint32_t u0 = src[0], u1 = src[1], u2 = src[2];
    dst[0] = u0;
    dst[1] = u1;
    dst[2] = u2;
    if (VAR && var_out) var_out[p] = 0.f;
  } else {
    Xout[p] = Xin[p];
  }
}

// The LDS form of a level, for a step STEP of 1 or 2: the tile's records and their halo of 2 STEP
// pixels, (32 + 4 STEP) x (8 + 4 STEP) records of 48 B (30 KB at STEP 2), each read from memory
// once instead of up to 25 times through L1. One array per record kind: a half-wave's tap is 32
// consecutive 16-B slots, which ds_read_b128 serves without a bank conflict, at offsets that are
// constants of the instruction. STEP 0 is the direct form and stages nothing.
template <int STEP>
struct TileLds {
  static constexpr int RW = kTileW + 4 * STEP, RH = kTileH + 4 * STEP, N = RW * RH;
  float4 g0[N], g1[N], x[N];
};
template <>
struct TileLds<0> {};

// One level for the lane's pixel. STEP 0: the step is P.step and every record is read from memory
// (through L1). STEP 1, 2: the records come from the tile staged in L; a record outside the frame
// is staged as an invalid pixel (all zero), so the tap arithmetic, its order and hence every bit
// match the direct form. Pixel indices are 32-bit (W * H < 2^31); a tap's index is formed modulo
// 2^32 and used only inside.
template <bool VAR, int STEP, bool FINAL>
__device__ __forceinline__ void atrous_level(const DnParams& P, TileLds<STEP>& L,
                                             const float4* __restrict__ G0,
                                             const float4* __restrict__ G1,
                                             const float4* __restrict__ Xin, float4* Xout,
                                             const float* beauty, const float* __restrict__ aov,
                                             float* out, float* var_out) {
  int x, y;
  const bool inside = lane_pixel(P, &x, &y);
  [[maybe_unused]] int c = 0;  // the lane's slot in the tile
  if constexpr (STEP != 0) {
    constexpr int RW = TileLds<STEP>::RW, N = TileLds<STEP>::N, HALO = 2 * STEP;
    const int lx = (int)(threadIdx.x & (kTileW - 1)), ly = (int)(threadIdx.x >> 5);
    const int x0 = x - lx - HALO, y0 = y - ly - HALO;  // the region's first pixel (may be < 0)
    for (int r = (int)threadIdx.x; r < N; r += kBlock) {
      const int ry = r / RW, rx = r - ry * RW;
      const int gx = x0 + rx, gy = y0 + ry;  // tile origin < W, H: no overflow
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, d = a;
      if (gx >= 0 && gx < P.W && gy >= 0 && gy < P.H) {
        const uint32_t q = (uint32_t)gy * (uint32_t)P.W + (uint32_t)gx;
        a = G0[q];
        b = G1[q];
        d = Xin[q];
      }
      L.g0[r] = a;
      L.g1[r] = b;
      L.x[r] = d;
    }
    __syncthreads();
    c = (ly + HALO) * RW + lx + HALO;
  }
  if (!inside) return;
  const uint32_t p = (uint32_t)y * (uint32_t)P.W + (uint32_t)x;
  float4 g0p, g1p, xp;
  if constexpr (STEP != 0)
    g1p = L.g1[c];
  else
    g1p = G1[p];
  if (g1p.w == 0.f) {
    invalid_pass<VAR, FINAL>(p, Xin, Xout, beauty, out, var_out);
    return;
  }
  if constexpr (STEP != 0)
    g0p = L.g0[c], xp = L.x[c];
  else
    g0p = G0[p], xp = Xin[p];
  const float zp2 = g0p.w * g0p.w;
  TapSums S;
#pragma unroll
  for (int j = -2; j <= 2; ++j) {
    if constexpr (STEP != 0) {
#pragma unroll
      for (int i = -2; i <= 2; ++i) {
        const int q = c + j * STEP * TileLds<STEP>::RW + i * STEP;
        tap_add<VAR>(P, g0p, g1p, xp, zp2, L.g0[q], L.g1[q], L.x[q], b3(i) * b3(j), true, S);
      }
    } else {
      const bool in_y = tap_inside(y, P.H, j * P.step);
      const uint32_t row = p + (uint32_t)(j * P.step) * (uint32_t)P.W;
#pragma unroll
      for (int i = -2; i <= 2; ++i) {
        const bool ok = in_y && tap_inside(x, P.W, i * P.step);
        const uint32_t q = ok ? row + (uint32_t)(i * P.step) : p;
        tap_add<VAR>(P, g0p, g1p, xp, zp2, G0[q], G1[q], Xin[q], b3(i) * b3(j), ok, S);
      }
    }
  }
  level_store<VAR, FINAL>(P, g1p, S, p, Xout, aov, out, var_out);
}

}  // namespace rtd
