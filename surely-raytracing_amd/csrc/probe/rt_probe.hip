// rt_probe.hip — TEST INFRASTRUCTURE ONLY (build/librtprobe.so, tests/probe_lib.py).
//
// One C function per device primitive of rt_kernel.h / rt_rng.h, so a test can run the product's
// own inline functions on the GPU one by one and compare them with a high-precision reference
// (tests/test_device_primitives_gpu.py). Compiled with the product's HIPFLAGS (contraction off),
// so a primitive computes here the bits it computes inside the path kernel. No product code links
// this library and librtmi355x.so does not change.
//
// Every function has the shape  int rtp_<name>(const double* in, double* out, int n)  (the Perlin
// probe also takes the table bytes): `in` holds n records of IN doubles, `out` n records of OUT
// doubles; integers, booleans and f32 values cross as f64, which is exact. A call copies its inputs
// to the device, launches one bounds-checked kernel with one thread per record, copies back and
// returns 0 or the HIP error code. Synchronous HIP calls only; no state is kept between calls.
//
// The kernels call the product's functions and nothing else: no formula is restated here.
#include "../rt_kernel.h"

namespace {
using namespace rtk;

constexpr int kProbeBlock = 64;

template <class P>
__global__ void __launch_bounds__(kProbeBlock) probe_kernel(const double* __restrict__ in,
                                                            double* __restrict__ out, int n,
                                                            const uint8_t* __restrict__ aux) {
  const int i = (int)(blockIdx.x * (unsigned)kProbeBlock + threadIdx.x);
  if (i >= n) return;
  P::apply(in + (size_t)i * P::IN, out + (size_t)i * P::OUT, aux);
}

template <class P>
int probe_run(const double* in, double* out, int n, const void* aux, size_t aux_bytes) {
  if (n < 0 || (n > 0 && (!in || !out)) || (aux_bytes && !aux)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t ib = (size_t)n * P::IN * sizeof(double), ob = (size_t)n * P::OUT * sizeof(double);
  double *din = nullptr, *dout = nullptr;
  uint8_t* daux = nullptr;
  hipError_t e = hipMalloc((void**)&din, ib);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, ob);
  if (e == hipSuccess && aux_bytes) e = hipMalloc((void**)&daux, aux_bytes);
  if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess && aux_bytes) e = hipMemcpy(daux, aux, aux_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, ob);
  if (e == hipSuccess) {
    const unsigned blocks = ((unsigned)n + kProbeBlock - 1u) / kProbeBlock;
    probe_kernel<P><<<dim3(blocks), dim3(kProbeBlock), 0, 0>>>(din, dout, n, daux);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  // the buffers are released on every path; the first error is the one reported
  const hipError_t f0 = din ? hipFree(din) : hipSuccess;
  const hipError_t f1 = dout ? hipFree(dout) : hipSuccess;
  const hipError_t f2 = daux ? hipFree(daux) : hipSuccess;
  if (e == hipSuccess) e = f0 != hipSuccess ? f0 : (f1 != hipSuccess ? f1 : f2);
  return (int)e;
}

__device__ __forceinline__ d3 in3(const double* p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ void out3(double* p, d3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }
__device__ __forceinline__ Rng seeded(const double* in) {  // seed_lo, seed_hi, pixel, sample
  return rng_seed((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3]);
}
}  // namespace

// PROBE(name, IN, OUT) { body }: the body sees `in` (IN doubles), `out` (OUT doubles) and `aux`.
#define PROBE_DECL(name, NIN, NOUT)                                                       \
  namespace {                                                                             \
  struct P_##name {                                                                       \
    static constexpr int IN = NIN, OUT = NOUT;                                            \
    static __device__ __forceinline__ void apply(const double* in, double* out,           \
                                                 const uint8_t* aux);                     \
  };                                                                                      \
  }
#define PROBE(name, NIN, NOUT)                                                            \
  PROBE_DECL(name, NIN, NOUT)                                                             \
  extern "C" __attribute__((visibility("default"))) int rtp_##name(const double* in,      \
                                                                   double* out, int n) {  \
    return probe_run<P_##name>(in, out, n, nullptr, 0);                                   \
  }                                                                                       \
  __device__ __forceinline__ void P_##name::apply(const double* in, double* out,          \
                                                  const uint8_t* aux)

// ---------------------------------------------------------------- reciprocals and roots
PROBE(rcp_nr, 1, 1) { out[0] = rcp_nr(in[0]); }
PROBE(rcp_nr1, 1, 1) { out[0] = rcp_nr1(in[0]); }
PROBE(div_nr, 2, 1) { out[0] = div_nr(in[0], in[1]); }
PROBE(rsq_nr, 1, 1) { out[0] = rsq_nr(in[0]); }
PROBE(sqrt_nr, 1, 1) { out[0] = sqrt_nr(in[0]); }
PROBE(rcp_w, 1, 1) { out[0] = rcp_w(in[0]); }
PROBE(rcp_wt, 1, 1) { out[0] = (double)rcp_wt((wt)in[0]); }
PROBE(rsq_wt, 1, 1) { out[0] = (double)rsq_wt((wt)in[0]); }

// ---------------------------------------------------------------- transcendentals
PROBE(sincos2pi, 1, 2) { sincos2pi(in[0], &out[0], &out[1]); }
PROBE(log_u01, 1, 1) { out[0] = log_u01(in[0]); }
PROBE(pow5_cr, 1, 1) { out[0] = pow5_cr(in[0]); }
PROBE(f2i_sat, 1, 1) { out[0] = (double)f2i_sat(in[0]); }
PROBE(f2u_sat, 1, 1) { out[0] = (double)f2u_sat(in[0]); }

// ---------------------------------------------------------------- RNG
// in: seed_lo, seed_hi, pixel, sample. out: the state of rng_seed, of the split key, of the split
// key advanced from sample - 1 by rng_key_next, then the first 16 outputs of rng_u32.
PROBE(rng_stream, 4, 22) {
  const uint32_t lo = (uint32_t)in[0], hi = (uint32_t)in[1], px = (uint32_t)in[2],
                 sm = (uint32_t)in[3];
  Rng g = rng_seed(lo, hi, px, sm);
  const Rng a = rng_key_mix(rng_key_pixel(lo, px), rng_key_sample(lo, hi, sm));
  const Rng b = rng_key_mix(rng_key_pixel(lo, px), rng_key_next(rng_key_sample(lo, hi, sm - 1u)));
  out[0] = (double)g.s0, out[1] = (double)g.s1;
  out[2] = (double)a.s0, out[3] = (double)a.s1;
  out[4] = (double)b.s0, out[5] = (double)b.s1;
  for (int k = 0; k < 16; ++k) out[6 + k] = (double)rng_u32(g);
}
// in: seed_lo, seed_hi, pixel, sample, n. out: rnd, rnd_pm1, rnd_index(g, n) of the stream's
// first three draws, in this order.
PROBE(rng_draws, 5, 3) {
  Rng g = seeded(in);
  out[0] = rnd(g);
  out[1] = rnd_pm1(g);
  out[2] = (double)rnd_index(g, (uint32_t)in[4]);
}
// in: seed_lo, seed_hi, pixel, sample. out: the vector, then the generator's state after it (the
// stream position: how many draws were consumed).
PROBE(random_cosine_direction, 4, 5) {
  Rng g = seeded(in);
  out3(out, random_cosine_direction(g));
  out[3] = (double)g.s0, out[4] = (double)g.s1;
}
PROBE(random_unit_vector, 4, 5) {
  Rng g = seeded(in);
  out3(out, random_unit_vector(g));
  out[3] = (double)g.s0, out[4] = (double)g.s1;
}

// ---------------------------------------------------------------- hit tests
// in: center3, radius, o3, d3, tmin, tmax, t_out's sentinel. out: hit, t_out, a, half_b, disc.
PROBE(sphere_test_v, 13, 5) {
  Ctr<false> C;
  double t = in[12], a, hb, disc;
  const bool h = sphere_test_v<false>(in3(in), in[3], in3(in + 4), in3(in + 7), in[10], in[11], t, C,
                                      a, hb, disc);
  out[0] = h ? 1.0 : 0.0, out[1] = t, out[2] = a, out[3] = hb, out[4] = disc;
}
// in: K, h0, qk, lo0, lo1, hi0, hi1, o3, d3, tmin, tmax, sentinel. out: hit, t_out, t_plane,
// plane_inr. Two forms, by the reciprocal handed over per component: aquad_test_nr1 with
// r = rcp_nr1(d), which is what every caller passes (traverse, volume_two_hits, the BVH walkers,
// light_leaf_pdf, the generated walkers), and aquad_test with the two-step r = rcp_nr(d).
namespace {
template <bool NR1>
__device__ __forceinline__ void aquad_probe(const double* in, double* out) {
  Ctr<false> C;
  const AQuad q = {(uint32_t)in[1], in[2], in[3], in[4], in[5], in[6]};
  const d3 o = in3(in + 7), d = in3(in + 10);
  const d3 r = NR1 ? mk(rcp_nr1(d.x), rcp_nr1(d.y), rcp_nr1(d.z))
                   : mk(rcp_nr(d.x), rcp_nr(d.y), rcp_nr(d.z));
  double t = in[15], tp = 0.0;
  bool inr = false, h;
  const int K = (int)in[0];
  if (K == 0)
    h = aquad_test<false, 0>(q, o, d, r, in[13], in[14], t, C, tp, inr);
  else if (K == 1)
    h = aquad_test<false, 1>(q, o, d, r, in[13], in[14], t, C, tp, inr);
  else
    h = aquad_test<false, 2>(q, o, d, r, in[13], in[14], t, C, tp, inr);
  out[0] = h ? 1.0 : 0.0, out[1] = t, out[2] = tp, out[3] = inr ? 1.0 : 0.0;
}
}  // namespace
PROBE(aquad_test, 16, 4) { aquad_probe<false>(in, out); }
PROBE(aquad_test_nr1, 16, 4) { aquad_probe<true>(in, out); }
// in: two doubles in the place of a record's four header words, the general payload d0-15
// (rt_layout.h QUAD), o3, d3, tmin, tmax, sentinel, one pad (records stay 16-byte aligned for
// ld3's paired loads). out: hit, t_out.
PROBE(quad_test, 28, 2) {
  Ctr<false> C;
  double t = in[26];
  const bool h = quad_test<false>(reinterpret_cast<gptr>(in), in3(in + 18), in3(in + 21), in[24],
                                  in[25], t, C);
  out[0] = h ? 1.0 : 0.0, out[1] = t;
}
// in: mn3, mx3, o3, inv3, tmin, tmax. out: aabb_hit, aabb_hit_bf.
PROBE(aabb_hit, 14, 2) {
  const double mn[3] = {in[0], in[1], in[2]}, mx[3] = {in[3], in[4], in[5]};
  out[0] = aabb_hit(mn, mx, in3(in + 6), in3(in + 9), in[12], in[13]) ? 1.0 : 0.0;
  out[1] = aabb_hit_bf(mn, mx, in3(in + 6), in3(in + 9), in[12], in[13]) ? 1.0 : 0.0;
}

// ---------------------------------------------------------------- transforms and vector helpers
// in: sin, cos, then two vectors (o, d for _in; p, n for _out). out: both, transformed.
PROBE(rotate_y_in, 8, 6) {
  d3 o = in3(in + 2), d = in3(in + 5);
  rotate_y_in(in[0], in[1], o, d);
  out3(out, o), out3(out + 3, d);
}
PROBE(rotate_y_out, 8, 6) {
  d3 p = in3(in + 2), n = in3(in + 5);
  rotate_y_out(in[0], in[1], p, n);
  out3(out, p), out3(out + 3, n);
}
PROBE(reflect, 6, 3) { out3(out, reflect(in3(in), in3(in + 3))); }
PROBE(refract, 7, 3) { out3(out, refract(in3(in), in3(in + 3), in[6])); }
PROBE(unit_vector, 3, 3) { out3(out, unit_vector(in3(in))); }
// in: the basis u3, v3, w3, then a3.
PROBE(onb_local, 12, 3) {
  const Onb b = {in3(in), in3(in + 3), in3(in + 6)};
  out3(out, onb_local(b, in3(in + 9)));
}

// ---------------------------------------------------------------- textures and light weights
PROBE(sphere_uv_f, 3, 2) {
  const UV r = sphere_uv_f(in3(in));
  out[0] = r.u, out[1] = r.v;
}
PROBE(quad_light_w, 8, 1) { out[0] = (double)quad_light_w(in3(in), in[3], in3(in + 4), in[7]); }
PROBE(sphere_light_w, 1, 1) { out[0] = (double)sphere_light_w(in[0]); }

// table: one Perlin table in the RTL_PERLIN_BYTES layout (rt_layout.h). in: p3. out: turb.
PROBE_DECL(perlin_turb, 3, 1)
extern "C" __attribute__((visibility("default"))) int rtp_perlin_turb(const uint8_t* table,
                                                                      const double* in, double* out,
                                                                      int n) {
  return probe_run<P_perlin_turb>(in, out, n, table, RTL_PERLIN_BYTES);
}
__device__ __forceinline__ void P_perlin_turb::apply(const double* in, double* out,
                                                     const uint8_t* aux) {
  out[0] = (double)perlin_turb(aux, in3(in));
}

// ---------------------------------------------------------------- f32 weight constants
// in: a double. out: the bits of to_w3's component for it, as an integer. The flattener stores the
// host's (float) cast of a weight constant (rt_layout.h RTL_MATF_SOLID_W) in place of this
// conversion; tests/test_weight_mirror_gpu.py holds the two together. (Written out, not through
// PROBE: tests/probe_lib.py lists the probes that take and return plain values.)
namespace {
struct P_to_w3_bits {
  static constexpr int IN = 1, OUT = 1;
  static __device__ __forceinline__ void apply(const double* in, double* out, const uint8_t*) {
    const w3 w = to_w3(mk(in[0], in[0], in[0]));
    out[0] = (double)__builtin_bit_cast(uint32_t, (float)w.x);
  }
};
}  // namespace
extern "C" __attribute__((visibility("default"))) int rtp_to_w3_bits(const double* in, double* out,
                                                                     int n) {
  if (n > 4096) return (int)hipErrorInvalidValue;
  return probe_run<P_to_w3_bits>(in, out, n, nullptr, 0);
}
