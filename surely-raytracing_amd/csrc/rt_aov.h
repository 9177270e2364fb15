// rt_aov.h — the first-hit AOV pass (include/rt_mi355x.h, rt_render_aov): the body of the rt_aov
// kernels (rt_aov.hip). Ahead-of-time only: this header is NOT part of the hiprtc embedded set.
//
// One wave per 8x8 pixel tile (kWaveTile, as rt_reduce maps them), lane = pixel. The lane loops
// over the call's n_sj x sqrt_spp samples in the reference's order (s_j outer, s_i inner,
// render.rs:185-189); per sample it seeds the sample's own stream, forms the camera ray exactly as
// trace_body's camera-ray block does (two jitter draws, the defocus-disk rejection loop, the time
// draw), runs ONE world query over [1e-4, inf) through the interpreter walker with that generator
// (a ConstantMedium free-flight draw is then the one the beauty pass makes) and forms the hit
// record as trace_body does. Eleven f64 sums and the first sample's material id stay in
// registers; the lane writes its RT_AOV_CHANNELS floats once. No pool queue, no workspace, no
// reduction kernel, no atomics: the output is bitwise reproducible.
//
// The walker depends on the launch's LDS plan (rt_scene_impl.hpp plan_lds: staged tables, Perlin
// tables, compact BVHs, the per-lane walk stacks at stack_lds_off) and on the workgroup size the
// plan assumes (BlockOf<BVH>), so the prologue is the one trace_body runs (rt_kernel.h stage_lds
// and make_tabs) and the launch uses the plan's block size; a workgroup holds blockDim / 64 tiles.
#pragma once
#include "rt_kernel.h"

namespace rtk {

template <bool VOL, bool TEX, bool BVH, bool STAGED, class Trav>
__device__ __forceinline__ void aov_body(const TraceParams& P, float* __restrict__ aov) {
  constexpr bool COUNT = false;
  typedef typename cond<STAGED, lptr, gptr>::type TP;
  stage_lds<BVH, BVH>(P);  // the product build's prologue: no COUNT here
  TabsT<TP> T;
  make_tabs<STAGED>(P, T);
  Ctr<COUNT> C;

  // ---- tile and pixel of this lane (rt_reduce's mapping). A wave past the last tile leaves (no
  // barrier follows); the lanes a ragged tile masks trace the tile's first pixel and write nothing,
  // so the walker always runs with the whole wave, as it does in the path kernel.
  const int n_tiles = P.tiles_x * ((P.n_rows + kWaveTile - 1) / kWaveTile);
  const int tile_id = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (tile_id >= n_tiles) return;
  const int lane = threadIdx.x & 63;
  const int tx = tile_id % P.tiles_x, ty = tile_id / P.tiles_x;
  const int tile_w = imin(kWaveTile, P.W - tx * kWaveTile);
  const int tile_h = imin(kWaveTile, P.n_rows - ty * kWaveTile);
  const bool live = lane < tile_w * tile_h;
  const int pv = live ? lane : 0;
  const int x = tx * kWaveTile + pv % tile_w, kr = ty * kWaveTile + pv / tile_w;
  const int y = P.row_begin + kr * P.row_step;

  double s_hits = 0.0, s_t = 0.0;
  d3 s_n = mk(0., 0., 0.), s_alb = s_n, s_em = s_n;
  float matid = -1.0f;
  for (int s_j = P.sj0; s_j < P.sj0 + P.n_sj; ++s_j) {
    for (int s_i = 0; s_i < P.sqrt_spp; ++s_i) {
      const kparams_t Q = kparams();
      // get_ray render.rs:218-249, as trace_body's camera-ray block: the same draws in the same
      // order, the same arithmetic
      Rng g = rng_seed(Q->seed_lo, Q->seed_hi, (uint32_t)(y * Q->W + x),
                       (uint32_t)(s_j * Q->sqrt_spp + s_i));
      d3 pc = vfma((double)y, karr3(Q->dv), vfma((double)x, karr3(Q->du), karr3(Q->p00)));
      double px = fma(Q->rs, (double)s_i + rnd(g), -0.5);
      double py = fma(Q->rs, (double)s_j + rnd(g), -0.5);
      d3 ps = pc + vfma(px, karr3(Q->du), karr3(Q->dv) * py);
      d3 origin = karr3(Q->center);
      if (Q->defocus) {
        for (;;) {
          double dx = rnd_pm1(g);
          double dy = rnd_pm1(g);
          if (fma(dx, dx, dy * dy) < 1.0) {
            const kparams_t R = kparams();
            origin = vfma(dy, karr3(R->ddv), vfma(dx, karr3(R->ddu), karr3(R->center)));
            break;
          }
        }
      }
      d3 ro = origin, rd = ps - origin;
      const double tm = rnd(g);  // the ray's time (render.rs:246), drawn for every scene
      // ---- the one world query (render.rs:267)
      double t;
      uint32_t hn = 0;
      int hf = -1;
      const bool hit_w =
          Trav::template world<COUNT, VOL, BVH, VOL, true>(P, ro, rd, tm, t, hn, hf, g, C);
      const bool first = s_j == P.sj0 && s_i == 0;
      if (!hit_w) {  // background (render.rs:298-309): ray_color at depth 1
        s_em = s_em + karr3(kparams()->bg);
        if (first) matid = -1.0f;
      } else {
        // ---- hit record of the winning primitive, recomputed in its own frame. A second copy of
        // trace_body's hit-record block (rt_kernel.h, "hit record of the winning primitive"): the
        // two are pinned together by tests/test_aov_gpu.py (the depth-1 oracle render and the
        // depth-1 beauty render against the emission channels, the textured albedo against the
        // oracle). Change one, change the other.
        const TP X = T.nodes + hn;
        const uint32_t type = X[0] & 0xffu;
        d3 o, d;
        Trav::frame_in(T.nodes, hf, ro, rd, o, d);
        d3 p = vfma(t, d, o);
        double u = 0., v = 0.;
        const uint32_t mat = X[2];
        const TP M = T.mats + (size_t)mat * RTL_MAT_WORDS;
        const uint4 mh = ld4u(M);
        const bool needs_uv = TEX && (mh.x & RTL_MATF_NEEDS_UV) != 0u;
        d3 outward;
        if (type == RTL_QUAD) {
          const TP XG = X + RTL_QUAD_GEN;
          outward = ld3(XG, 0);
          if (needs_uv) {
            d3 pq = p - ld3(XG, 4);
            u = dot(pq, ld3(XG, 8));
            v = dot(pq, ld3(XG, 12));
          }
        } else if (type == RTL_SPHERE) {
          d3 c = ld3(X, 0);
          if (X[0] & RTL_SPHERE_MOVING) c = vfma(tm, ld3(X, 4), c);
          // (p - c) / radius (object.rs:169): the correctly rounded quotient, as trace_body
          const d3 pcn = p - c;
          const double ir = ldd(X, 7), rad = ldd(X, 3);
          const d3 q0 = pcn * ir;
          outward = mk(fma(fma(-q0.x, rad, pcn.x), ir, q0.x), fma(fma(-q0.y, rad, pcn.y), ir, q0.y),
                       fma(fma(-q0.z, rad, pcn.z), ir, q0.z));
          if (needs_uv) sphere_uv(outward, u, v);
        } else {  // ConstantMedium: normal (1, 0, 0), front_face true (constant_medium.rs:82-90)
          outward = mk(1., 0., 0.);
        }
        const bool front = (type != RTL_QUAD && type != RTL_SPHERE) | (dot(d, outward) < 0.0);
        d3 normal = front ? outward : -outward;
        Trav::frame_out(T.nodes, hf, p, normal);  // back to world space
        const uint32_t kind = mh.x & 0xffu;
        // ---- what the first bounce would multiply by / what the hit emits
        d3 alb = mk(0., 0., 0.), em = alb;
        if (kind == RT_MAT_DIFFUSE_LIGHT) {  // material.rs:210-222
          if (front) em = tex_value<COUNT, TEX>(P, T, mh.y, u, v, p, C);
        } else if (kind == RT_MAT_METAL || kind == RT_MAT_DIELECTRIC) {
          alb = ld3(M, 0);  // Metal's albedo, Dielectric's tint
        } else {  // Lambertian, Isotropic: tex.value(u, v, p)
          alb = tex_value<COUNT, TEX>(P, T, mh.y, u, v, p, C);
        }
        s_hits += 1.0;
        s_t += t;
        s_n = s_n + normal;
        s_alb = s_alb + alb;
        s_em = s_em + em;
        if (first) matid = (float)mat;
      }
    }
  }
  if (!live) return;
  float* a = aov + ((size_t)kr * P.W + x) * RT_AOV_CHANNELS;
  const double s[11] = {s_hits, s_t,     s_n.x,   s_n.y,  s_n.z, s_alb.x,
                        s_alb.y, s_alb.z, s_em.x, s_em.y, s_em.z};
  if (P.flags & RT_FLAG_OVERWRITE) {
#pragma unroll
    for (int k = 0; k < 11; ++k) a[k] = (float)s[k];
  } else {  // as rt_reduce adds into the caller's accumulator
#pragma unroll
    for (int k = 0; k < 11; ++k) a[k] = (float)((double)a[k] + s[k]);
  }
  a[RT_AOV_MATID] = matid;
}

}  // namespace rtk
