// rt_probe_scene.hip — TEST INFRASTRUCTURE ONLY (build/librtprobe.so, tests/probe_lib.py).
//
// The scene-level device functions of rt_kernel.h behind a C ABI: the ones that read the flattened
// scene tables (rt_layout.h) and call the primitives rt_probe.hip exposes one by one — traverse,
// frame_ray / frame_out, volume_two_hits, light_pdf, tex_value. A test hands over an rt_scene_blob
// and records; a call flattens the blob (rtf::flatten, the product's flattener), packs and uploads
// the tables the way rt_scene_create does (the node array keeps its 256 bytes of padding), fills
// the table fields of a TraceParams (everything else zero), launches one bounds-checked kernel with
// one thread per record, the TraceParams by value as its first argument, copies back and frees
// every buffer on every path. The two BVH entries (bvh_walks, world_hit_bvh) also set up what the
// BVH kernels' launch sets up (rt_device.hip plan_lds, rt_kernel.h trace_body): kBlockBvh threads,
// the compact trees copied to LDS offset 0 by the kernel before any walk, the per-lane walk
// stacks after them. Synchronous HIP calls only; no state is kept between calls. Compiled
// with the product's HIPFLAGS; no product code links this library.
//
// Return value: 0, a positive HIP error code, or a negative refusal that never reaches a kernel:
// the flattener's status (include/rt_mi355x.h RT_ERR_*), or
//   RTP_ERR_BVH     the scene has a BvhNode and the entry is not one of the BVH entries (with
//                   BVH = false, traverse steps over RTL_BVH records: a silent miss must not pass
//                   for an answer)
//   RTP_ERR_NESTED  a ConstantMedium inside another one's boundary (not instantiated here)
//   RTP_ERR_RECORD  a record carries an index that is not what the kernel would read it as: a
//                   texture id outside the table, a node that is no top-level one-walk VOLUME
//                   record, a frame that is neither -1 nor a transform record; for the BVH
//                   entries: a scene without a BvhNode, a node that is no top-level subtree root
//                   with an ordered BVH and a compact copy, compact trees that fail the
//                   flattener's host checks, an LDS need above 64 KB
//   RTP_ERR_ARG     null pointers, a negative count
//
// The kernels call the product's functions and nothing else: no formula is restated here.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../rt_kernel.h"
#include "../rt_flatten.hpp"
#include "../rt_variant.h"

#define RTP_ERR_ARG (-100)
#define RTP_ERR_BVH (-101)
#define RTP_ERR_NESTED (-102)
#define RTP_ERR_RECORD (-103)

namespace {
using namespace rtk;

constexpr int kSceneBlock = 64;

// one record of the flattened world sequence, as the host scan sees it
struct Rec {
  uint32_t word, type, flags, w2;
  int frame;  // the transform record enclosing it, -1 at top level
};

struct DevScene {
  rtf::FlatScene F;
  std::vector<Rec> recs;
  uint8_t* dev = nullptr;
  TraceParams P;
  ~DevScene() {
    if (dev) (void)hipFree(dev);
  }
};

// The frame of every BVH record the top-level walk hands to the per-lane walker (traverse<UNI>'s
// order: the world sequence, instances entered and left), by record word. BVH records sit in the
// BVH region in front of the node array, so the memory-order scan below cannot tell their frame.
std::vector<std::pair<uint32_t, int>> bvh_root_frames(const rtf::FlatScene& F) {
  std::vector<std::pair<uint32_t, int>> roots;
  const std::vector<uint32_t>& w = F.nodes;
  uint32_t x = F.hdr.root;
  int frame = -1;
  for (size_t guard = 0; x + 4 <= F.hdr.n_rec_words && guard < w.size(); ++guard) {
    const uint32_t ty = w[x] & 0xffu;
    if (ty == RTL_END) break;
    if (ty == RTL_BVH) roots.push_back({x, frame});
    if (ty == RTL_TRANSLATE || ty == RTL_ROTATE_Y) frame = (int)x;
    if (ty == RTL_EXIT) frame = (int)w[x + 2];
    const bool next = ty == RTL_QUAD || ty == RTL_SPHERE || ty == RTL_TRANSLATE ||
                      ty == RTL_ROTATE_Y || ty == RTL_EXIT;
    x = next ? w[x + 3] : w[x + 1];
  }
  return roots;
}

// blob -> flattened tables + the record list; no HIP call. A BVH record is listed with its word 3
// (its ordered BVH, 0 = none) in w2 and, as its frame, the one the top-level walk reaches it in,
// -2 when that walk does not reach it (a node inside a subtree or inside a boundary).
int scene_flatten(const rt_scene_blob* blob, DevScene& S, bool allow_bvh = false) {
  if (!blob) return RTP_ERR_ARG;
  std::string err;
  const int rc = rtf::flatten(blob, &S.F, &err);
  if (rc != RT_OK) return rc;
  const rtf::FlatScene& F = S.F;
  if (F.hdr.has_bvh && !allow_bvh) return RTP_ERR_BVH;
  if (F.hdr.nested_volumes) return RTP_ERR_NESTED;
  const std::vector<std::pair<uint32_t, int>> roots = bvh_root_frames(F);
  int frame = -1;
  for (size_t p = 0; p < F.hdr.n_rec_words; p += rtf::record_words(F.nodes[p])) {
    const uint32_t h = F.nodes[p], ty = h & 0xffu;
    if ((ty == RTL_BVH || ty == RTL_DUP) && !allow_bvh) return RTP_ERR_BVH;
    if (ty == RTL_BVH) {
      int bf = -2;
      for (const auto& r : roots)
        if (r.first == p) bf = r.second;
      S.recs.push_back({(uint32_t)p, ty, h >> 8, F.nodes[p + 3], bf});
      continue;
    }
    S.recs.push_back({(uint32_t)p, ty, h >> 8, p + 2 < F.nodes.size() ? F.nodes[p + 2] : 0u, frame});
    if (ty == RTL_TRANSLATE || ty == RTL_ROTATE_Y) frame = (int)p;
    if (ty == RTL_EXIT) frame = (int)F.nodes[p + 2];
  }
  // the tables the texture walk trusts: children, Perlin indices and texel ranges inside them
  const size_t n_tex = F.texs.size() / RTL_TEX_WORDS;
  for (size_t i = 0; i < n_tex; ++i) {
    const uint32_t* t = &F.texs[i * RTL_TEX_WORDS];
    if (t[0] == RT_TEX_CHECKER && (t[1] >= n_tex || t[2] >= n_tex)) return RTP_ERR_RECORD;
    if (t[0] == RT_TEX_NOISE && (size_t)(t[1] + 1) * RTL_PERLIN_BYTES > F.perlin.size())
      return RTP_ERR_RECORD;
    if (t[0] == RT_TEX_IMAGE && (int)t[1] > 0 && (int)t[2] > 0 &&
        (size_t)t[3] + (size_t)t[1] * t[2] * 3 > F.texels.size())
      return RTP_ERR_RECORD;
  }
  return 0;
}

// pack and upload as rt_scene_create does (rt_device.hip table_layout), then the table fields of P
hipError_t scene_upload(DevScene& S) {
  const rtf::FlatScene& F = S.F;
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t o_nodes = 0;
  const size_t o_mats = al(o_nodes + F.nodes.size() * 4 + 256);  // the walkers' 64-byte fetches
  const size_t o_texs = al(o_mats + F.mats.size() * 4);
  const size_t o_lig = al(o_texs + F.texs.size() * 4);
  const size_t o_loff = al(o_lig + F.lights.size() * 4);
  const size_t o_perl = al(o_loff + F.light_offs.size() * 4);
  const size_t o_tx = al(o_perl + F.perlin.size());
  const size_t total = al(o_tx + F.texels.size()) + 256;
  std::vector<uint8_t> host(total, 0);
  auto cp = [&](size_t off, const void* src, size_t n) {
    if (n) std::memcpy(host.data() + off, src, n);
  };
  cp(o_nodes, F.nodes.data(), F.nodes.size() * 4);
  cp(o_mats, F.mats.data(), F.mats.size() * 4);
  cp(o_texs, F.texs.data(), F.texs.size() * 4);
  cp(o_lig, F.lights.data(), F.lights.size() * 4);
  cp(o_loff, F.light_offs.data(), F.light_offs.size() * 4);
  cp(o_perl, F.perlin.data(), F.perlin.size());
  cp(o_tx, F.texels.data(), F.texels.size());
  hipError_t e = hipMalloc((void**)&S.dev, total);
  if (e == hipSuccess) e = hipMemcpy(S.dev, host.data(), total, hipMemcpyHostToDevice);
  if (e != hipSuccess) return e;
  TraceParams& P = S.P;
  std::memset(&P, 0, sizeof(P));
  P.nodes = (const uint32_t*)(S.dev + o_nodes);
  P.mats = (const uint32_t*)(S.dev + o_mats);
  P.texs = (const uint32_t*)(S.dev + o_texs);
  P.perlin = S.dev + o_perl;
  P.lights = (const uint32_t*)(S.dev + o_lig);
  P.light_offs = (const uint32_t*)(S.dev + o_loff);
  P.texels = S.dev + o_tx;
  P.root = F.hdr.root;
  P.n_lights = F.hdr.n_lights;
  P.lights_is_list = F.hdr.lights_is_list;
  P.lights_nested = F.hdr.lights_nested;
  P.inv_n_lights = F.hdr.n_lights ? 1.0 / (double)F.hdr.n_lights : 0.0;
  P.sphere_light0 = -1;
  for (size_t i = 0; i < F.light_offs.size(); ++i)
    if ((F.lights[F.light_offs[i]] & 0xffu) == RTL_SPHERE) {
      P.sphere_light0 = (int)i;
      break;
    }
  P.n_perlin_lds = 0;
  P.o_mats = (uint32_t)o_mats;
  P.o_texs = (uint32_t)o_texs;
  P.o_lights = (uint32_t)o_lig;
  P.o_loffs = (uint32_t)o_loff;
  P.o_perl = (uint32_t)o_perl;
  // the BVH region stays in global memory (bvh_lds_words = 0), the compact trees go to LDS
  // offset 0 with the walk stacks after them (bvh_lds_need checked the size)
  P.bvh_words = F.hdr.bvh_words;
  P.cbvh_lds_off = ~0u;
  if (F.hdr.has_bvh && F.hdr.cbvh_words) {
    P.cbvh_src = (const uint8_t*)(P.nodes + F.hdr.cbvh_word0);
    P.cbvh_bytes = 4u * F.hdr.cbvh_words;
    P.cbvh_lds_off = 0u;
    P.stack_lds_off = P.cbvh_bytes;
  }
  return hipSuccess;
}

// dynamic LDS of a BVH launch: the compact trees, then one stack per lane (stride blockDim.x)
size_t bvh_lds_need(const rtf::FlatScene& F) {
  return F.hdr.cbvh_words ? 4u * (size_t)F.hdr.cbvh_words + (size_t)F.hdr.cbvh_stack * kBlockBvh : 0u;
}
constexpr size_t kLdsDefault = 64u << 10;  // what a kernel gets without asking for more

// what rt_scene_create checks before it uploads a BVH scene, and the launch's LDS need
int bvh_host_checks(const rtf::FlatScene& F) {
  if (!F.hdr.has_bvh) return RTP_ERR_RECORD;
  if (F.hdr.cbvh_words && (F.hdr.cbvh_word0 % 4u || F.hdr.cbvh_words % 4u ||
                           (size_t)F.hdr.cbvh_word0 + F.hdr.cbvh_words > F.nodes.size()))
    return RTP_ERR_RECORD;
  if (rtf::check_compact_trees(F.nodes, F.hdr, 0, 0).errors) return RTP_ERR_RECORD;
  return bvh_lds_need(F) <= kLdsDefault ? 0 : RTP_ERR_RECORD;
}

template <class K>
__global__ void __launch_bounds__(kSceneBlock) scene_kernel(TraceParams P,
                                                            const double* __restrict__ in,
                                                            double* __restrict__ out, int n,
                                                            uint32_t arg) {
  const int i = (int)(blockIdx.x * (unsigned)kSceneBlock + threadIdx.x);
  if (i >= n) return;
  K::apply(P, in + (size_t)i * K::IN, out + (size_t)i * K::OUT, arg);
}

// The BVH entries' kernel: the BVH kernels' block size, and their prologue's copy of the compact
// trees into LDS (rt_kernel.h stage_lds; scene_upload stages nothing else) before any lane walks
template <class K>
__global__ void __launch_bounds__(kBlockBvh) scene_kernel_bvh(TraceParams P,
                                                              const double* __restrict__ in,
                                                              double* __restrict__ out, int n,
                                                              uint32_t arg) {
  stage_lds<true, true>(P);
  const int i = (int)(blockIdx.x * (unsigned)kBlockBvh + threadIdx.x);
  if (i >= n) return;
  K::apply(P, in + (size_t)i * K::IN, out + (size_t)i * K::OUT, arg);
}

// check(S, record) -> 0 or a refusal, on the host, for every record before anything is launched;
// arg: a call-wide index (wave-uniform in the kernel), checked by the caller
template <class K, bool BVH = false, class Check>
int scene_run(const rt_scene_blob* blob, const double* in, double* out, int n, uint32_t arg,
              Check check) {
  if (n < 0 || (n > 0 && (!in || !out))) return RTP_ERR_ARG;
  DevScene S;
  int rc = scene_flatten(blob, S, BVH);
  if (rc) return rc;
  if (BVH) rc = bvh_host_checks(S.F);
  if (rc) return rc;
  rc = check(S, (const double*)nullptr);  // the call-wide argument
  for (int i = 0; i < n && !rc; ++i) rc = check(S, in + (size_t)i * K::IN);
  if (rc) return rc;
  if (n == 0) return 0;
  const size_t ib = (size_t)n * K::IN * sizeof(double), ob = (size_t)n * K::OUT * sizeof(double);
  double *din = nullptr, *dout = nullptr;
  hipError_t e = scene_upload(S);
  if (e == hipSuccess) e = hipMalloc((void**)&din, ib);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, ob);
  if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, ob);
  if (e == hipSuccess) {
    if constexpr (BVH) {
      const unsigned blocks = ((unsigned)n + kBlockBvh - 1u) / kBlockBvh;
      scene_kernel_bvh<K><<<dim3(blocks), dim3(kBlockBvh), bvh_lds_need(S.F), 0>>>(S.P, din, dout,
                                                                                   n, arg);
    } else {
      const unsigned blocks = ((unsigned)n + kSceneBlock - 1u) / kSceneBlock;
      scene_kernel<K><<<dim3(blocks), dim3(kSceneBlock), 0, 0>>>(S.P, din, dout, n, arg);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  // the buffers are released on every path (the tables by ~DevScene); the first error is reported
  const hipError_t f0 = din ? hipFree(din) : hipSuccess;
  const hipError_t f1 = dout ? hipFree(dout) : hipSuccess;
  if (e == hipSuccess) e = f0 != hipSuccess ? f0 : f1;
  return (int)e;
}

__device__ __forceinline__ d3 in3(const double* p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ void out3(double* p, d3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }

// a double that is an integer in [lo, hi]
bool int_in(double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); }

const Rec* find_rec(const DevScene& S, double word) {
  if (!int_in(word, 0.0, 4294967295.0)) return nullptr;
  for (const Rec& r : S.recs)
    if (r.word == (uint32_t)word) return &r;
  return nullptr;
}

// ---------------------------------------------------------------- the world query
// in: o3, d3, time, tmin, tmax, seed_lo, seed_hi, pixel, sample. out, once per COUNT value (the
// product build first): hit, t, hit node, hit frame, the hit record's material word, the
// generator's state afterwards.
template <bool VOL>
struct K_world_hit_t {
  static constexpr int IN = 13, OUT = 14;
  template <bool COUNT>
  static __device__ __forceinline__ void one(const TraceParams& P, const double* in, double* out) {
    Ctr<COUNT> C;
    Rng g = rng_seed((uint32_t)in[9], (uint32_t)in[10], (uint32_t)in[11], (uint32_t)in[12]);
    const d3 o = in3(in), d = in3(in + 3);
    double t = 0.0;
    uint32_t hn = 0u;
    int hf = -1;
    const bool h = traverse<true, COUNT, VOL, true, false, false, true, 0>(
        P, P.root, ~0u, o, d, in[6], o, d, -1, in[7], in[8], t, hn, hf, g, C);
    out[0] = h ? 1.0 : 0.0, out[1] = t;
    out[2] = h ? (double)hn : -1.0, out[3] = h ? (double)hf : -1.0;
    out[4] = h ? (double)P.nodes[hn + 2] : -1.0;
    out[5] = (double)g.s0, out[6] = (double)g.s1;
  }
  static __device__ __forceinline__ void apply(const TraceParams& P, const double* in, double* out,
                                               uint32_t) {
    one<false>(P, in, out);
    one<true>(P, in, out + 7);
  }
};

// The same query through the BVH kernels' walker (traverse<..., UNI, BVH = true, VOLB, VOLI>):
// bvh_subtree's ordered walk from LDS, its ballot and the flagged lanes' re-walk in the product
// build, the reference tree in the COUNT build (which always carries the two-walk interpreter).
template <bool VOL, bool VOLB, bool VOLI>
struct K_world_hit_bvh_t {
  static constexpr int IN = 13, OUT = 14;
  template <bool COUNT>
  static __device__ __forceinline__ void one(const TraceParams& P, const double* in, double* out) {
    Ctr<COUNT> C;
    Rng g = rng_seed((uint32_t)in[9], (uint32_t)in[10], (uint32_t)in[11], (uint32_t)in[12]);
    const d3 o = in3(in), d = in3(in + 3);
    double t = 0.0;
    uint32_t hn = 0u;
    int hf = -1;
    const bool h = traverse<true, COUNT, VOL, true, true, VOLB, (COUNT || VOLI)>(
        P, P.root, ~0u, o, d, in[6], o, d, -1, in[7], in[8], t, hn, hf, g, C);
    out[0] = h ? 1.0 : 0.0, out[1] = t;
    out[2] = h ? (double)hn : -1.0, out[3] = h ? (double)hf : -1.0;
    out[4] = h ? (double)P.nodes[hn + 2] : -1.0;
    out[5] = (double)g.s0, out[6] = (double)g.s1;
  }
  static __device__ __forceinline__ void apply(const TraceParams& P, const double* in, double* out,
                                               uint32_t) {
    one<false>(P, in, out);
    one<true>(P, in, out + 7);
  }
};

// ---------------------------------------------------------------- the BVH walkers, ray by ray
// arg: a top-level BVH subtree root (frame -1) with an ordered BVH and a compact copy. in: o3, d3,
// time, tmin, tmax. One thread runs the ray through cbvh_walk (the compact tree in LDS), obvh_walk
// (the octant streams in global memory) and the reference-order traverse over [node, skip). out,
// once with MAIN = true and once with MAIN = false (the ConstantMedium boundary's instantiation;
// hit node -1): per walk hit, t (tmax on a miss), hit node, and the ordered walks' tie flag:
// [cbvh 4][obvh 4][reference 3].
struct K_bvh_walks {
  static constexpr int IN = 9, OUT = 22;
  template <bool MAIN>
  static __device__ __forceinline__ void pass(const TraceParams& P, uint32_t node, uint4 h, uint4 hd,
                                              const double* in, double* out) {
    const d3 o = in3(in), d = in3(in + 3);
    const double tm = in[6], tmin = in[7], tmax = in[8];
    auto put = [&](double* p, bool hit, double t, uint32_t hn) {
      p[0] = hit ? 1.0 : 0.0, p[1] = hit ? t : tmax, p[2] = hit && MAIN ? (double)hn : -1.0;
    };
    double t = tmax;
    uint32_t hn = 0u;
    int hf = -1;
    bool fl = false;
    bool hit = cbvh_walk<MAIN>(P, hd, o, d, tm, -1, tmin, tmax, t, hn, hf, fl);
    put(out, hit, t, hn);
    out[3] = fl ? 1.0 : 0.0;
    t = tmax, hn = 0u, fl = false;
    hit = obvh_walk<MAIN>(P, h.w, o, d, tm, -1, tmin, tmax, t, hn, hf, fl);
    put(out + 4, hit, t, hn);
    out[7] = fl ? 1.0 : 0.0;
    Ctr<false> C;
    Rng g = rng_seed(0u, 0u, 0u, 0u);
    t = tmax, hn = 0u;
    hit = traverse<MAIN, false, false, false, true>(P, node, h.y, o, d, tm, o, d, -1, tmin, tmax, t,
                                                    hn, hf, g, C);
    put(out + 8, hit, t, hn);
  }
  static __device__ __forceinline__ void apply(const TraceParams& P, const double* in, double* out,
                                               uint32_t node) {
    const uint4 h = ld4u((kptr)P.nodes + node);     // [hdr][skip][first child][ordered BVH]
    const uint4 hd = ld4u((gptr)P.nodes + h.w);     // [n_entries][cbvh block][root ref][streams]
    pass<true>(P, node, h, hd, in, out);
    pass<false>(P, node, h, hd, in, out + 11);
  }
};

// ---------------------------------------------------------------- frames
// in: frame, world o3, d3, local p3, n3. out: the local ray o3, d3, the world p3, n3.
struct K_frame {
  static constexpr int IN = 13, OUT = 12;
  static __device__ __forceinline__ void apply(const TraceParams& P, const double* in, double* out,
                                               uint32_t) {
    const gptr N = P.nodes;
    const int frame = (int)in[0];
    d3 o, d, p = in3(in + 7), n = in3(in + 10);
    frame_ray(N, frame, in3(in + 1), in3(in + 4), o, d);
    frame_out(N, frame, p, n);
    out3(out, o), out3(out + 3, d), out3(out + 6, p), out3(out + 9, n);
  }
};

// ---------------------------------------------------------------- ConstantMedium boundaries
// arg: a top-level one-walk VOLUME record. in: o3, d3, time. out: both, t1, t2, fallback of
// volume_two_hits, then the two boundary passes volume_hit falls back to: the first pass's hit,
// both, t1, t2.
struct K_volume_bounds {
  static constexpr int IN = 7, OUT = 8;
  static __device__ __forceinline__ void apply(const TraceParams& P, const double* in, double* out,
                                               uint32_t node) {
    const uint4 h = ld4u((kptr)P.nodes + node);
    const uint32_t kind = h.x & (RTL_VOLF_SPHERE | RTL_VOLF_QUADS);
    const d3 o = in3(in), d = in3(in + 3);
    const double tm = in[6];
    double t1 = 0.0, t2 = 0.0;
    bool fb = false;
    const bool both = volume_two_hits(P, h.w, kind, o, d, tm, t1, t2, fb);
    out[0] = both ? 1.0 : 0.0, out[1] = t1, out[2] = t2, out[3] = fb ? 1.0 : 0.0;
    Ctr<false> C;
    Rng g = rng_seed(0u, 0u, 0u, 0u);
    double p1 = 0.0, p2 = 0.0;
    uint32_t dn;
    int df;
    bool b2 = traverse<false, false, false, true, false>(P, h.w, ~0u, o, d, tm, o, d, -1, -kInf,
                                                         kInf, p1, dn, df, g, C);
    out[4] = b2 ? 1.0 : 0.0;
    if (b2)
      b2 = traverse<false, false, false, true, false>(P, h.w, ~0u, o, d, tm, o, d, -1,
                                                      p1 + 0.0001, kInf, p2, dn, df, g, C);
    out[5] = b2 ? 1.0 : 0.0, out[6] = p1, out[7] = p2;
  }
};

// ---------------------------------------------------------------- the light-list PDF
// in: origin3, dir3, cos_sl0. out: light_pdf<true> (the root test), light_pdf<false> (the root-free
// sphere predicate).
struct K_light_pdf {
  static constexpr int IN = 7, OUT = 2;
  static __device__ __forceinline__ void apply(const TraceParams& P, const double* in, double* out,
                                               uint32_t) {
    Ctr<true> C1;
    Ctr<false> C0;
    out[0] = (double)light_pdf<true>(P, in3(in), in3(in + 3), in[6], C1);
    out[1] = (double)light_pdf<false>(P, in3(in), in3(in + 3), in[6], C0);
  }
};

// ---------------------------------------------------------------- textures
// in: texture id, u, v, p3. out: RGB with no Perlin table counted as local (perlin_turb_global),
// then RGB with every table counted as local (T.perlin = the same global tables).
struct K_tex_value {
  static constexpr int IN = 6, OUT = 6;
  static __device__ __forceinline__ void apply(const TraceParams& P, const double* in, double* out,
                                               uint32_t) {
    TabsT<gptr> T;
    T.nodes = P.nodes, T.mats = P.mats, T.texs = P.texs, T.lights = P.lights;
    T.loffs = P.light_offs, T.perlin = P.perlin;
    Ctr<false> C;
    const uint32_t id = (uint32_t)in[0];
    out3(out, tex_value<false, true>(P, T, id, in[1], in[2], in3(in + 3), C));
    TraceParams Q = P;
    Q.n_perlin_lds = ~0u;
    out3(out + 3, tex_value<false, true>(Q, T, id, in[1], in[2], in3(in + 3), C));
  }
};

int no_check(const DevScene&, const double*) { return 0; }
}  // namespace

#define RTP_API extern "C" __attribute__((visibility("default")))

// SCENE_PROBE(name, IN, OUT): records of IN doubles in, OUT doubles out (tests/probe_lib.py)
#define SCENE_PROBE(name, NIN, NOUT) \
  static_assert(K_##name::IN == NIN && K_##name::OUT == NOUT, "record sizes of " #name);

namespace {
typedef K_world_hit_t<false> K_world_hit;
SCENE_PROBE(world_hit, 13, 14)
SCENE_PROBE(frame, 13, 12)
SCENE_PROBE(volume_bounds, 7, 8)
SCENE_PROBE(light_pdf, 7, 2)
SCENE_PROBE(tex_value, 6, 6)
typedef K_world_hit_bvh_t<false, false, true> K_world_hit_bvh;
SCENE_PROBE(world_hit_bvh, 13, 14)
SCENE_PROBE(bvh_walks, 9, 22)
}  // namespace

RTP_API int rtp_world_hit(const rt_scene_blob* blob, const double* in, double* out, int n) {
  DevScene S;  // only to choose the instance: VOL as rt_render_device chooses it
  const int rc = scene_flatten(blob, S);
  if (rc) return rc;
  if (S.F.hdr.has_volume) return scene_run<K_world_hit_t<true>>(blob, in, out, n, 0u, no_check);
  return scene_run<K_world_hit_t<false>>(blob, in, out, n, 0u, no_check);
}

// The VOL, VOLB and VOLI of the product kernel's variant for the scene (rt_variant.h)
RTP_API int rtp_world_hit_bvh(const rt_scene_blob* blob, const double* in, double* out, int n) {
  DevScene S;
  const int rc = scene_flatten(blob, S, true);
  if (rc) return rc;
  if (!S.F.hdr.has_bvh) return RTP_ERR_RECORD;
  const rtv::Variant v = rtv::choose_variant(S.F.hdr, 0u, false);
  if (!v.vol) return scene_run<K_world_hit_bvh_t<false, false, true>, true>(blob, in, out, n, 0u, no_check);
  if (v.volb) return scene_run<K_world_hit_bvh_t<true, true, true>, true>(blob, in, out, n, 0u, no_check);
  if (!v.voli)
    return scene_run<K_world_hit_bvh_t<true, false, false>, true>(blob, in, out, n, 0u, no_check);
  return scene_run<K_world_hit_bvh_t<true, false, true>, true>(blob, in, out, n, 0u, no_check);
}

RTP_API int rtp_bvh_walks(const rt_scene_blob* blob, int node, const double* in, double* out,
                          int n) {
  return scene_run<K_bvh_walks, true>(blob, in, out, n, (uint32_t)node,
                                      [node](const DevScene& S, const double* r) {
    if (r) return 0;
    const Rec* x = find_rec(S, (double)node);
    if (!x || x->type != RTL_BVH || x->frame != -1 || x->w2 == 0u) return RTP_ERR_RECORD;
    // the ordered BVH's header and streams inside the node array, a compact block staged
    const std::vector<uint32_t>& w = S.F.nodes;
    const size_t ob = x->w2;
    if (ob < S.F.hdr.n_rec_words || ob + 8 > w.size() || w[ob + 1] == ~0u) return RTP_ERR_RECORD;
    if (w[ob + 1] >= 4u * S.F.hdr.cbvh_words) return RTP_ERR_RECORD;
    return ob + w[ob + 3] + (size_t)64 * w[ob] <= w.size() ? 0 : RTP_ERR_RECORD;
  });
}

RTP_API int rtp_frame(const rt_scene_blob* blob, const double* in, double* out, int n) {
  return scene_run<K_frame>(blob, in, out, n, 0u, [](const DevScene& S, const double* r) {
    if (!r || r[0] == -1.0) return 0;
    const Rec* x = find_rec(S, r[0]);
    return x && (x->type == RTL_TRANSLATE || x->type == RTL_ROTATE_Y) ? 0 : RTP_ERR_RECORD;
  });
}

RTP_API int rtp_volume_bounds(const rt_scene_blob* blob, int node, const double* in, double* out,
                              int n) {
  return scene_run<K_volume_bounds>(blob, in, out, n, (uint32_t)node,
                                    [node](const DevScene& S, const double* r) {
    if (r) return 0;
    const Rec* x = find_rec(S, (double)node);
    const uint32_t fuse = (RTL_VOLF_SPHERE | RTL_VOLF_QUADS) >> 8;
    return x && x->type == RTL_VOLUME && x->frame == -1 && (x->flags & fuse) ? 0 : RTP_ERR_RECORD;
  });
}

RTP_API int rtp_light_pdf(const rt_scene_blob* blob, const double* in, double* out, int n) {
  return scene_run<K_light_pdf>(blob, in, out, n, 0u, no_check);
}

RTP_API int rtp_tex_value(const rt_scene_blob* blob, const double* in, double* out, int n) {
  return scene_run<K_tex_value>(blob, in, out, n, 0u, [](const DevScene& S, const double* r) {
    if (!r) return 0;
    const size_t n_tex = S.F.texs.size() / RTL_TEX_WORDS;
    return n_tex > 0 && int_in(r[0], 0.0, (double)(n_tex - 1)) ? 0 : RTP_ERR_RECORD;
  });
}

// The records of the flattened world sequence in memory order, so a test can name a frame or a
// VOLUME record and tell which primitive a hit node is: rows of [word, type, header word 0 >> 8,
// word 2 (material, chain length or parent frame), enclosing frame]. A scene with a BvhNode is
// listed too (this entry launches nothing): a BVH record's fourth column is its ordered BVH's word
// offset (0 = none, the reference tree is walked) and its frame is the one the top-level walk
// reaches it in, -2 for a node that walk does not reach. Returns the number of records (at most
// `cap` rows are written) or a refusal. No GPU is touched.
RTP_API int rtp_scene_records(const rt_scene_blob* blob, double* out, int cap) {
  if (cap < 0 || (cap > 0 && !out)) return RTP_ERR_ARG;
  DevScene S;
  const int rc = scene_flatten(blob, S, true);
  if (rc) return rc;
  for (size_t i = 0; i < S.recs.size() && i < (size_t)cap; ++i) {
    const Rec& r = S.recs[i];
    double* o = out + 5 * i;
    o[0] = r.word, o[1] = r.type, o[2] = r.flags, o[3] = r.w2, o[4] = r.frame;
  }
  return (int)S.recs.size();
}

// The rtl_scene_header of rtf::flatten, word by word in the struct's order (rt_layout.h), for any
// scene the flattener takes (nested volumes and BVHs included: nothing is launched, no HIP call):
// the bits rtv::choose_variant reads, for tests/test_variant_matrix.py. Copies at most `cap`
// words; returns the header's size in words, or a refusal.
RTP_API int rtp_scene_header(const rt_scene_blob* blob, uint32_t* out, int cap) {
  static_assert(sizeof(rtl_scene_header) % sizeof(uint32_t) == 0, "rtl_scene_header: 32-bit words");
  constexpr int kWords = (int)(sizeof(rtl_scene_header) / sizeof(uint32_t));
  if (!blob || cap < 0 || (cap > 0 && !out)) return RTP_ERR_ARG;
  rtf::FlatScene F;
  std::string err;
  const int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return rc;
  if (cap > 0) std::memcpy(out, &F.hdr, (size_t)(cap < kWords ? cap : kWords) * sizeof(uint32_t));
  return kWords;
}

// The flattened material and texture tables of a scene (any scene: nothing is launched), for the
// host test of the f32 weight mirrors (tests/test_weight_mirror.py). Copies at most *_cap words
// each; returns the flattener's status, the table sizes in words through n_mats / n_texs.
RTP_API int rtp_flat_tables(const rt_scene_blob* blob, uint32_t* mats, int mats_cap, uint32_t* texs,
                            int texs_cap, int* n_mats, int* n_texs) {
  if (!blob || !n_mats || !n_texs || mats_cap < 0 || texs_cap < 0 || (mats_cap > 0 && !mats) ||
      (texs_cap > 0 && !texs))
    return RTP_ERR_ARG;
  rtf::FlatScene F;
  std::string err;
  const int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return rc;
  *n_mats = (int)F.mats.size();
  *n_texs = (int)F.texs.size();
  const size_t nm = F.mats.size() < (size_t)mats_cap ? F.mats.size() : (size_t)mats_cap;
  const size_t nt = F.texs.size() < (size_t)texs_cap ? F.texs.size() : (size_t)texs_cap;
  if (nm) std::memcpy(mats, F.mats.data(), nm * 4);
  if (nt) std::memcpy(texs, F.texs.data(), nt * 4);
  return 0;
}
