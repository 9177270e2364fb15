// rt_query.h — ray queries (include/rt_mi355x.h, rt_query_rays): the body of the rt_query kernels
// (rt_query.hip). Ahead-of-time only: this header is NOT part of the hiprtc embedded set.
//
// One lane per caller-supplied ray, 64 consecutive rays per wave. The lane reads its 80-byte
// rt_ray with five 16-byte loads, seeds the ray's own stream from (seed, pixel, sample), runs ONE
// world query over the ray's own [tmin, tmax] through the interpreter walker (as rt_aov.h runs its
// query over [1e-4, inf)), forms the hit record as aov_body does and writes its 80-byte rt_hit
// with five 16-byte stores, or one byte in occlusion mode. No pool queue, no workspace, no
// atomics: a record depends on its ray and the params alone.
//
// The walker ballots and keeps per-lane LDS stacks, so a wave enters it whole: a lane past the end
// of the batch and a lane whose ray is invalid (rt_mi355x.h) walk a fixed ray, origin 0, direction
// +z, [1e-4, inf), with their wave and never hand their own values to the walker. Only whole waves
// past the end leave early (no barrier follows the prologue's).
//
// The launch runs on the AOV pass's LDS plan at the plan's workgroup size (rt_aov.h): the same
// prologue, the same five instances.
//
// ANY (mode RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT): five more instances whose world query is the
// walker's ANY form (rt_kernel.h traverse): it leaves at the first accept and returns the closest-
// hit walk's flag. A tail lane and a lane with an invalid ray enter it with the empty interval
// [1, 0], so they are done from the start: their fixed ray misses most scenes and would hold every
// ragged or partly invalid wave to the full walk.
#pragma once
#include "rt_kernel.h"

namespace rtk {

__device__ __forceinline__ uint4 pack2(double a, double b) {
  const unsigned long long x = (unsigned long long)__double_as_longlong(a);
  const unsigned long long y = (unsigned long long)__double_as_longlong(b);
  return make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
}

// prim_tab: n_prim record word offsets, ascending, then their n_prim prims (rt_scene::prim_dev)
__device__ __forceinline__ int prim_of(const uint32_t* __restrict__ prim_tab, uint32_t n_prim,
                                       uint32_t hn) {
  uint32_t lo = 0u, hi = n_prim;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (prim_tab[mid] < hn) lo = mid + 1u; else hi = mid;
  }
  return lo < n_prim && prim_tab[lo] == hn ? (int)prim_tab[n_prim + lo] : -1;
}

template <bool BVH, bool STAGED, int VN, bool ANY = false>
__device__ __forceinline__ void query_body(const TraceParams& P, const uint4* __restrict__ rays,
                                           void* __restrict__ out, uint32_t n_rays, uint32_t mode,
                                           const uint32_t* __restrict__ prim_tab, uint32_t n_prim) {
  constexpr bool COUNT = false;
  typedef typename cond<STAGED, lptr, gptr>::type TP;
  typedef TravInterpN<VN> Trav;
  stage_lds<BVH, BVH>(P);  // the product build's prologue, as aov_body
  TabsT<TP> T;
  make_tabs<STAGED>(P, T);
  Ctr<COUNT> C;

  const uint32_t wave0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u);
  if (wave0 >= n_rays) return;  // a whole wave past the end
  const uint32_t i = wave0 + (threadIdx.x & 63u);
  const bool live = i < n_rays;
  // a tail lane reads the wave's first ray (memory that exists) and discards it
  const uint4* R = rays + (size_t)(live ? i : wave0) * 5u;
  const uint4 r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3], r4 = R[4];
  const bool dir0 = ((r1.z | r2.x | r2.z) == 0u) & (((r1.w | r2.y | r2.w) & 0x7fffffffu) == 0u);
  const bool valid = finite_hi(r0.y) && finite_hi(r0.w) && finite_hi(r1.y) && finite_hi(r1.w) &&
                     finite_hi(r2.y) && finite_hi(r2.w) && finite_hi(r3.y) &&  // origin, dir, time
                     finite_hi(r3.w) &&  // tmin: neither NaN nor infinite
                     !dir0;
  const double tmax_in = hilo(r4.x, r4.y);
  const bool ok = live && valid && tmax_in == tmax_in;
  d3 ro = mk(0., 0., 0.), rd = mk(0., 0., 1.);
  double tm = 0.0, tmin = 0.0001, tmax = kInf;
  if constexpr (ANY) tmin = 1.0, tmax = 0.0;  // done at entry unless the lane has a ray
  uint32_t pixel = 0u, sample = 0u;
  if (ok) {
    ro = mk(hilo(r0.x, r0.y), hilo(r0.z, r0.w), hilo(r1.x, r1.y));
    rd = mk(hilo(r1.z, r1.w), hilo(r2.x, r2.y), hilo(r2.z, r2.w));
    tm = hilo(r3.x, r3.y), tmin = hilo(r3.z, r3.w), tmax = tmax_in;
    pixel = r4.z, sample = r4.w;
  }
  Rng g = rng_seed(P.seed_lo, P.seed_hi, pixel, sample);
  // ---- the one world query: Trav::world's call (rt_kernel.h TravInterpN) with the ray's interval.
  // PK = true in every instance, not only the nested-volume ones: the walker then reads its launch
  // constants from P and nowhere through kparams(), which is null in a called function. The
  // compiler left this kernel's top-level walk of the BVH instance as one (the AOV pass's is
  // inlined), and under RT_FLAG_REFERENCE_BVH every lane's per-lane walk read bvh_words at
  // address 0x98. No code of this header calls kparams() either.
  double t;
  uint32_t hn = 0;
  int hf = -1;
  const bool hit_w = traverse<true, COUNT, true, true, BVH, true, true, VN, true, ANY>(
      P, P.root, ~0u, ro, rd, tm, ro, rd, -1, tmin, tmax, t, hn, hf, g, C);
  if (!live) return;
  if (ANY || (mode & RT_QUERY_OCCLUSION)) {  // ANY has no record to fill (the host checks mode)
    reinterpret_cast<uint8_t*>(out)[i] = ok ? (hit_w ? (uint8_t)1 : (uint8_t)0) : (uint8_t)255;
    return;
  }
  uint4* H = reinterpret_cast<uint4*>(out) + (size_t)i * 5u;
  if (!ok) {  // hit = -1, every other field 0
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    H[0] = z, H[1] = z, H[2] = z, H[3] = z;
    H[4] = make_uint4(0xffffffffu, 0u, 0u, 0u);
    return;
  }
  if (!hit_w) {  // t: the ray's own tmax (traverse leaves `closest` there)
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    H[0] = pack2(t, 0.0), H[1] = z, H[2] = z, H[3] = z;
    H[4] = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
    return;
  }
  // ---- hit record of the winning primitive, recomputed in its own frame. A third copy of
  // trace_body's hit-record block (rt_kernel.h, "hit record of the winning primitive") after
  // aov_body's (rt_aov.h): frame_in, the per-type outward normal, set_face_normal, frame_out.
  // tests/test_query_gpu.py pins this one to the f64 oracle and to the AOV channels. Change one,
  // change the others.
  const TP X = T.nodes + hn;
  const uint32_t type = X[0] & 0xffu;
  d3 o, d;
  Trav::frame_in(T.nodes, hf, ro, rd, o, d);
  d3 p = vfma(t, d, o);
  d3 outward;
  if (type == RTL_QUAD) {
    outward = ld3(X + RTL_QUAD_GEN, 0);
  } else if (type == RTL_SPHERE) {
    d3 c = ld3(X, 0);
    if (X[0] & RTL_SPHERE_MOVING) c = vfma(tm, ld3(X, 4), c);
    // (p - c) / radius (object.rs:169): the correctly rounded quotient, as trace_body
    const d3 pcn = p - c;
    const double ir = ldd(X, 7), rad = ldd(X, 3);
    const d3 q0 = pcn * ir;
    outward = mk(fma(fma(-q0.x, rad, pcn.x), ir, q0.x), fma(fma(-q0.y, rad, pcn.y), ir, q0.y),
                 fma(fma(-q0.z, rad, pcn.z), ir, q0.z));
  } else {  // ConstantMedium: normal (1, 0, 0), front_face true (constant_medium.rs:82-90)
    outward = mk(1., 0., 0.);
  }
  const bool front = (type != RTL_QUAD && type != RTL_SPHERE) | (dot(d, outward) < 0.0);
  d3 normal = front ? outward : -outward;
  Trav::frame_out(T.nodes, hf, p, normal);  // back to world space
  const double dist = t * sqrt_nr(dot(rd, rd));
  H[0] = pack2(t, dist);
  H[1] = pack2(p.x, p.y);
  H[2] = pack2(p.z, normal.x);
  H[3] = pack2(normal.y, normal.z);
  H[4] = make_uint4(1u, front ? 1u : 0u, X[2], (uint32_t)prim_of(prim_tab, n_prim, hn));
}

}  // namespace rtk
