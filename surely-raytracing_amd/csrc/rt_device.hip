// rt_device.hip — gfx950 path-tracing kernels + the C ABI of include/rt_mi355x.h.
//
// Replaces the reference's per-pixel render loop (render.rs:144-216) and everything it calls:
// get_ray (render.rs:218-249), ray_color (render.rs:251-311), HittableList/BvhNode::hit
// (hittable.rs:88-109, 216-236), Quad/Sphere/Aabb::hit (object.rs:145-184, 340-370, 453-490),
// Translate/RotateY::hit (transform.rs:57-135), ConstantMedium::hit (constant_medium.rs:41-95),
// Material scatter (material.rs:92-248), PDFs (pdf.rs:44-127), Onb (onb.rs:24-47), textures
// and Perlin noise (texture.rs:17-131, perlin.rs:30-96), vec3 math (vec3.rs).
//
// Work decomposition: persistent waves claim POOLS from a global queue; a pool
// is one 8x8 pixel tile x one stratum row s_j (x one block of kPoolSi stratum columns s_i for
// segment and tail pools). Each lane traces one path at a time (ray_color's recursion -> an
// iterative bounce loop with beta/L) and takes a row item (all of one pixel's samples of the
// row, summed per block and then per row in f64 in LDS), a segment item (one block) or, for the
// launch's last pools, one sample; when its item ends it writes the f64 value and claims the
// next item with a wave ballot + mbcnt, so lanes stay busy whatever the per-pixel path cost.
// rt_reduce forms each row's total from block partials where a lane did not, and adds the rows
// in the reference's sample order (s_i inside s_j, render.rs:185-189; the association differs
// from its single running sum only between blocks and between rows) into the caller's
// accumulator, so no atomics touch the framebuffer and results are bitwise reproducible and
// identical across 1..8 GPUs and any split of the work (the RNG is keyed by global pixel and
// sample).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rt_mi355x.h"
#include "rt_flatten.hpp"
#include "rt_jit.hpp"
#include "rt_kernel.h"
#include "rt_layout.h"
#include "rt_scene_impl.hpp"
#include "rt_variant.h"

using namespace rtk;
using namespace rts;

namespace {

// Ahead-of-time kernels: the interpreter traversal, one per row of RT_VARIANTS (rt_variant.h) and,
// for the rows that keep the two-walk interpreter, one more that counts ops.
template <bool COUNT, bool VOL, bool TEX, bool BVH, bool STAGED, bool VOLB, bool VOLI, int VN>
__global__ __launch_bounds__(BlockOf<BVH>::value, (MinWaves<VOL, TEX, BVH>::value)) void rt_trace(
    TraceParams P) {
  trace_body<COUNT, VOL, TEX, BVH, STAGED, VOLB, VOLI, TravInterpN<VN>>(P);
}
template <bool VOL, bool TEX, bool BVH, bool STAGED, bool VOLB, bool VOLI, int VN>
constexpr kern_t count_kernel() {
  if constexpr (VOLI)
    return rt_trace<true, VOL, TEX, BVH, STAGED, VOLB, VOLI, VN>;
  else
    return nullptr;  // choose_variant keeps voli under RT_FLAG_COUNT_OPS
}
kern_t trace_kernel(const rtv::Variant& v, bool count) {
#define RT_VARIANT_ROW(vol, tex, bvh, staged, volb, voli, vn)                    \
  if (v == rtv::Variant{vol, tex, bvh, staged, volb, voli, vn})                  \
    return count ? count_kernel<vol, tex, bvh, staged, volb, voli, vn>()         \
                 : rt_trace<false, vol, tex, bvh, staged, volb, voli, vn>;
  RT_VARIANTS(RT_VARIANT_ROW)
#undef RT_VARIANT_ROW
  return nullptr;
}

// Per pixel, in the reference's sample order (s_j, then s_i: render.rs:185-189): for each
// stratum row s_j its total R = ((p_0 + p_1) + p_2) + ... over the block partials p_b (a row
// item's R as the lane formed it; a segment pair's from its block partials; a tail pair's from
// the sequential sums of its blocks' samples: the same running sums, bit for bit), added into
// one running total. The reference adds every sample into that total; here a block's samples are
// summed first and a row's blocks next, so the association differs from the reference's only
// between blocks and between rows, and it does not depend on how the launch split its pairs into
// row, segment and tail items. One wave per 8x8 tile, lane = pixel of the tile: each load
// instruction reads 64 * 8 contiguous bytes. Chunked calls carry the running total in `tot`.
// mode: bit0 first chunk, bit1 last chunk (write accum), bit2 overwrite.
//
// M2 (rt_render_moments*): beside the running total, q = fma(R, R, q) per channel over the same
// row totals R in the same order: the pixel's second moment over the call's stratum rows, carried
// between chunks in `mo.tot2` and written to `mo.m2` exactly as the total is to `accum`. The plain
// instantiation (MomentsOut<false>, an empty argument) names none of it.
constexpr int kRedU = 8;  // values loaded ahead per step of rt_reduce
template <bool M2>
struct MomentsOut {};  // the plain reduction: no further kernel argument
template <>
struct MomentsOut<true> {
  double* tot2;  // the chunks' carry of q
  float* m2;     // the caller's second buffer
};
// TILES (rt_render_tiles_device): one wave per entry of the launch's tile list; n_tiles is the
// list's length, the pixel position comes from the listed tile, and the pairs (q0 = entry * n_sj)
// and the chunks' carries (64 pixels per entry) stay compact, indexed by the position in the list.
// The plain instantiation (TileIn<false>, an empty argument) names none of it.
// RAYS (rt_render_rays_device): the launch's "image" is the batch, 8 rays wide, so tile t is rays
// 64 t .. 64 t + 63 and the pixel index is the ray index; lanes past n_rays leave, and an invalid
// ray's three outputs become quiet NaN whatever the mode (the validity test of trace_body's ray
// block, on the same words).
template <int LK>
struct TileIn {};
template <>
struct TileIn<kLaunchTiles> {
  const uint32_t* list;
};
template <>
struct TileIn<kLaunchRays> {
  const uint4* rays;
  uint32_t n_rays;
};
template <bool M2, int LK = kLaunchPlain>
__global__ __launch_bounds__(256) void rt_reduce(const double* __restrict__ part,
                                                 double* __restrict__ tot,
                                                 float* __restrict__ accum, int W, int n_rows,
                                                 int tiles_x, int n_tiles, int n_sj, int S,
                                                 int n_pairs_r, int n_pairs_a, int mode,
                                                 MomentsOut<M2> mo, TileIn<LK> ti = {}) {
  constexpr bool TILES = LK == kLaunchTiles, RAYS = LK == kLaunchRays;
  const int tile_id = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const int pv = threadIdx.x & 63;
  if (tile_id >= n_tiles) return;
  int tile_px = tile_id;  // the tile of the call's grid whose pixels this wave sums
  if constexpr (TILES) tile_px = (int)ti.list[tile_id];
  const int tx = tile_px % tiles_x, ty = tile_px / tiles_x;
  const int tile_w = min(kWaveTile, W - tx * kWaveTile);
  const int tile_h = min(kWaveTile, n_rows - ty * kWaveTile);
  if (pv >= tile_w * tile_h) return;
  if constexpr (RAYS) {
    if ((uint32_t)tile_id * 64u + (uint32_t)pv >= ti.n_rays) return;
  }
  const int x = tx * kWaveTile + pv % tile_w, kr = ty * kWaveTile + pv / tile_w;
  const size_t i = (size_t)kr * W + x;
  const size_t ic = TILES ? (size_t)tile_id * 64 + pv : i;  // the pixel's carry between chunks
  const int n_blk = (S + kPoolSi - 1) / kPoolSi;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  if (!(mode & 1)) {
    t0 = tot[3 * ic];
    t1 = tot[3 * ic + 1];
    t2 = tot[3 * ic + 2];
  }
  double m0 = 0.0, m1 = 0.0, m2c = 0.0;  // M2: sum of R^2
  if constexpr (M2) {
    if (!(mode & 1)) {
      m0 = mo.tot2[3 * ic];
      m1 = mo.tot2[3 * ic + 1];
      m2c = mo.tot2[3 * ic + 2];
    }
  }
  const int q0 = tile_id * n_sj;  // this tile's pairs q0 .. q0 + n_sj - 1 (s_j order)
  const int k_r = max(0, min(n_sj, n_pairs_r - q0)), k_a = max(0, min(n_sj, n_pairs_a - q0));
  int k = 0;
  // row pairs: one total each, 64 values apart; loads first, then the in-order adds (a share's
  // few waves are otherwise bound by one load's latency per value)
  {
    const double* r = part + ((size_t)q0 * 64 + pv) * 3;
    for (; k + kRedU <= k_r; k += kRedU) {
      double v[kRedU][3];
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const double* e = r + (size_t)(k + u) * 192;
        v[u][0] = e[0], v[u][1] = e[1], v[u][2] = e[2];
      }
#pragma unroll
      for (int u = 0; u < kRedU; ++u) t0 += v[u][0], t1 += v[u][1], t2 += v[u][2];
      if (M2) {
#pragma unroll
        for (int u = 0; u < kRedU; ++u) {
          m0 = fma(v[u][0], v[u][0], m0);
          m1 = fma(v[u][1], v[u][1], m1);
          m2c = fma(v[u][2], v[u][2], m2c);
        }
      }
    }
    for (; k < k_r; ++k) {
      const double* e = r + (size_t)k * 192;
      t0 += e[0], t1 += e[1], t2 += e[2];
      if (M2) m0 = fma(e[0], e[0], m0), m1 = fma(e[1], e[1], m1), m2c = fma(e[2], e[2], m2c);
    }
  }
  // segment pairs: the row total of n_blk block partials
  for (; k < k_a; ++k) {
    const int q = q0 + k;
    const double* r =
        part + (((size_t)n_pairs_r + (size_t)(q - n_pairs_r) * n_blk) * 64 + pv) * 3;
    double r0 = r[0], r1 = r[1], r2 = r[2];
    int b = 1;
    for (; b + kRedU <= n_blk; b += kRedU) {
      double v[kRedU][3];
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const double* e = r + (size_t)(b + u) * 192;
        v[u][0] = e[0], v[u][1] = e[1], v[u][2] = e[2];
      }
#pragma unroll
      for (int u = 0; u < kRedU; ++u) r0 += v[u][0], r1 += v[u][1], r2 += v[u][2];
    }
    for (; b < n_blk; ++b) {
      const double* e = r + (size_t)b * 192;
      r0 += e[0], r1 += e[1], r2 += e[2];
    }
    t0 += r0, t1 += r1, t2 += r2;
    if (M2) m0 = fma(r0, r0, m0), m1 = fma(r1, r1, m1), m2c = fma(r2, r2, m2c);
  }
  // tail pairs: per-sample values, summed per block of kPoolSi samples, then the blocks
  const size_t tail0 = (size_t)n_pairs_r + (size_t)(n_pairs_a - n_pairs_r) * n_blk;
  for (; k < n_sj; ++k) {
    const int q = q0 + k;
    const double* rt = part + ((tail0 + (size_t)(q - n_pairs_a) * S) * 64 + pv) * 3;
    double R0 = 0.0, R1 = 0.0, R2 = 0.0;
    for (int s0 = 0; s0 < S; s0 += kPoolSi) {
      const int n = min(kPoolSi, S - s0);
      double v[kPoolSi][3];
#pragma unroll
      for (int u = 0; u < kPoolSi; ++u) {
        if (u < n) {
          const double* e = rt + (size_t)(s0 + u) * 192;
          v[u][0] = e[0], v[u][1] = e[1], v[u][2] = e[2];
        }
      }
      double r0 = 0.0, r1 = 0.0, r2 = 0.0;
#pragma unroll
      for (int u = 0; u < kPoolSi; ++u)
        if (u < n) r0 += v[u][0], r1 += v[u][1], r2 += v[u][2];
      if (s0 == 0) {
        R0 = r0, R1 = r1, R2 = r2;
      } else {
        R0 += r0, R1 += r1, R2 += r2;
      }
    }
    t0 += R0, t1 += R1, t2 += R2;
    if (M2) m0 = fma(R0, R0, m0), m1 = fma(R1, R1, m1), m2c = fma(R2, R2, m2c);
  }
  float* a = accum + 3 * i;
  if constexpr (RAYS) {
    if (mode & 2) {
      const uint4* R = ti.rays + i * 5u;
      const uint4 r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3];
      const bool dir0 = ((r1.z | r2.x | r2.z) == 0u) & (((r1.w | r2.y | r2.w) & 0x7fffffffu) == 0u);
      const bool valid = finite_hi(r0.y) && finite_hi(r0.w) && finite_hi(r1.y) && finite_hi(r1.w) &&
                         finite_hi(r2.y) && finite_hi(r2.w) && finite_hi(r3.y) && !dir0;
      if (!valid) {
        a[0] = a[1] = a[2] = __uint_as_float(0x7fc00000u);
        return;
      }
    }
  }
  if (mode & 2) {
    if (mode & 4) {
      a[0] = (float)t0, a[1] = (float)t1, a[2] = (float)t2;
    } else {
      a[0] = (float)((double)a[0] + t0), a[1] = (float)((double)a[1] + t1);
      a[2] = (float)((double)a[2] + t2);
    }
  } else {
    tot[3 * ic] = t0, tot[3 * ic + 1] = t1, tot[3 * ic + 2] = t2;
  }
  if constexpr (M2) {
    float* b = mo.m2 + 3 * i;
    if (mode & 2) {
      if (mode & 4) {
        b[0] = (float)m0, b[1] = (float)m1, b[2] = (float)m2c;
      } else {
        b[0] = (float)((double)b[0] + m0), b[1] = (float)((double)b[1] + m1);
        b[2] = (float)((double)b[2] + m2c);
      }
    } else {
      mo.tot2[3 * ic] = m0, mo.tot2[3 * ic + 1] = m1, mo.tot2[3 * ic + 2] = m2c;
    }
  }
}

// rt_multi_render's gather on the first device: device k's compact rows (its cyclic share of
// the call's rows, k, k + G, ...) arrive in `stage` at row offset row0[k]; each row goes to row
// k + j * G of the frame, overwritten or added (the caller's accumulator, render.rs:189).
// to_frame = 0: the reverse (the caller's accumulator rows into the staging area, so that every
// device accumulates into its own rows exactly as rt_render_device does, render.rs:189).
__global__ __launch_bounds__(256) void rt_deinterleave(float* __restrict__ stage,
                                                       float* __restrict__ frame, int row_floats,
                                                       int n_rows, int G, int to_frame) {
  // kr: row of the frame (a grid's y extent ends at 65535 blocks, so taller frames loop; the
  // same shape as rt_gather_deinterleave_k)
  for (int kr = blockIdx.y; kr < n_rows; kr += gridDim.y) {
    const int k = kr % G, j = kr / G;
    // device k's rows start at sum_{k' < k} rows(k'), rows(k') = ceil((n_rows - k') / G)
    int row0 = 0;
    for (int q = 0; q < k; ++q) row0 += (n_rows - q + G - 1) / G;
    float* st = stage + (size_t)(row0 + j) * row_floats;
    float* fr = frame + (size_t)kr * row_floats;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < row_floats;
         i += gridDim.x * blockDim.x) {
      if (to_frame)
        fr[i] = st[i];
      else
        st[i] = fr[i];
    }
  }
}

// ---------------------------------------------------------------- host side
thread_local std::string g_err;

}  // namespace

int rts::set_err(int code, const std::string& m) {
  g_err = m;
  return code;
}

// The launch's LDS plan (LdsPlan, rt_scene_impl.hpp)
LdsPlan rts::plan_lds(const rtl_scene_header& hdr, uint32_t o_perl, uint32_t flags, bool want_jit,
                      size_t lds_module_max) {
  LdsPlan L;
  const bool count = (flags & RT_FLAG_COUNT_OPS) != 0;
  const bool bvh = hdr.has_bvh != 0;
  L.block = bvh ? kBlockBvh : kBlock;
  // static LDS of the path kernel: the per-lane f64 running sums (trace_body sh_acc; non-BVH
  // kernels also the row totals sh_row, the bounce's throughput factor and ending radiance,
  // sh_f / sh_le, and the item's stream key sh_key: 80 of the 96 bytes per lane), the op
  // counters, slack for the profiling build
  L.static_lds = (size_t)L.block * (bvh ? 24 : 96) + 512 + (count ? 128 : 0);
#ifdef RT_PROF
  L.static_lds += 4096;  // the profiling build's counters (tools_gpu/prof_*.py)
#endif
  // a scene whose tables up to the Perlin block fit kStageScene bytes is copied whole (per-lane
  // reads then never leave the CU); otherwise only its first Perlin tables
  const uint32_t used_perlins = hdr.has_textures ? hdr.n_perlins : 0u;
  const size_t scene_prefix = o_perl + (size_t)used_perlins * RTL_PERLIN_BYTES;
  L.stage_scene = scene_prefix <= kStageScene ? 1u : 0u;
  if (L.stage_scene) {
    L.n_perlin_lds = used_perlins;
    L.stage_bytes = (uint32_t)((scene_prefix + 15) & ~(size_t)15);
  } else {
    L.n_perlin_lds = std::min<uint32_t>(used_perlins, kPerlinLds);
    L.stage_bytes = L.n_perlin_lds * RTL_PERLIN_BYTES;
  }
  const size_t cap = (want_jit ? lds_module_max : kLdsTotal) - L.static_lds;
  L.cbvh_bytes = hdr.cbvh_words * 4u;
  const size_t need = (size_t)L.stage_bytes + L.cbvh_bytes + (size_t)hdr.cbvh_stack * L.block;
  if (bvh && !count && L.cbvh_bytes && !(flags & RT_FLAG_REFERENCE_BVH) &&
      !std::getenv("RT_NO_CBVH_LDS") && need <= cap) {
    L.cbvh_lds_off = L.stage_bytes;
    L.stack_lds_off = L.stage_bytes + L.cbvh_bytes;
    L.cbvh_lds = need - L.stage_bytes;
  }
  if (L.stage_scene) {
    L.bvh_lds_words = hdr.bvh_words;
  } else if (bvh && L.cbvh_lds_off == ~0u) {
    const size_t room = cap > L.stage_bytes ? cap - L.stage_bytes : 0;
    L.bvh_lds_words = (uint32_t)std::min<size_t>(hdr.bvh_words, room / 64 * 16);
    L.bvh_lds_off = L.stage_bytes;
  }
  L.lds_bytes = L.stage_bytes + (L.stage_scene ? 0u : (size_t)L.bvh_lds_words * 4u) + L.cbvh_lds;
  // BVH product kernels with the compact trees in LDS: the row items' per-lane row totals after
  // them when they fit (C4: 124 + 18 KB dynamic, 18 KB static), so that a whole frame keeps one
  // f64 value per (pixel, s_j) instead of one per block of kPoolSi samples
  const size_t row_bytes = (size_t)L.block * 3 * sizeof(double);
  if (bvh && L.cbvh_lds_off != ~0u && !std::getenv("RT_NO_BVH_ROWS") &&
      L.lds_bytes + row_bytes <= cap) {
    L.row_lds_off = (uint32_t)L.lds_bytes;
    L.lds_bytes += row_bytes;
  }
  return L;
}

namespace {

// Byte offsets of the scene's tables in its one device allocation (rt_scene_create): nodes,
// materials, textures, lights, light offsets, Perlin tables, 16-byte aligned; texels last.
struct TableLayout {
  size_t o_nodes = 0, o_mats = 0, o_texs = 0, o_lig = 0, o_loff = 0, o_perl = 0, o_tx = 0, total = 0;
};
TableLayout table_layout(const rtf::FlatScene& F) {
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  TableLayout T;
  // +256 B: the LANE walker fetches 64 bytes of every node it visits (END, 16 B, included) and
  // prefetches one quad record past a batch
  T.o_mats = al(T.o_nodes + F.nodes.size() * 4 + 256);
  T.o_texs = al(T.o_mats + F.mats.size() * 4);
  T.o_lig = al(T.o_texs + F.texs.size() * 4);
  T.o_loff = al(T.o_lig + F.lights.size() * 4);
  T.o_perl = al(T.o_loff + F.light_offs.size() * 4);
  T.o_tx = al(T.o_perl + F.perlin.size());
  T.total = al(T.o_tx + F.texels.size()) + 256;
  return T;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_error(void) { return g_err.c_str(); }

int rt_device_count(int* count) {
  if (!count) return set_err(RT_ERR_INVALID_ARG, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *count = n;
  return RT_OK;
}

int rt_scene_validate(const rt_scene_blob* blob) {
  rtf::FlatScene F;
  std::string err;
  int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return set_err(rc, err);
  return RT_OK;
}

int rt_scene_layout_stats(const rt_scene_blob* blob, uint32_t* out, int n) {
  if (!out || n < 0) return set_err(RT_ERR_INVALID_ARG, "null out");
  rtf::FlatScene F;
  std::string err;
  int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return set_err(rc, err);
  uint32_t v[RT_LAYOUT_STATS] = {(uint32_t)F.nodes.size(), F.hdr.bvh_words, 0, 0, 0, 0, 0,
                                 F.hdr.n_lights, 0, 0, F.hdr.cbvh_words * 4u};
  for (size_t p = 0; p < F.hdr.n_rec_words; p += rtf::record_words(F.nodes[p])) {
    const uint32_t h = F.nodes[p], ty = h & 0xffu;
    if (ty == RTL_BVH) ++v[2];
    if (ty == RTL_BVH && F.nodes[p + 3] != 0u) {
      ++v[8];
      if (F.nodes[F.nodes[p + 3] + 1] != 0xffffffffu) ++v[9];
    }
    if (ty == RTL_DUP) ++v[3];
    if (ty == RTL_VOLUME) {
      ++v[4];
      if (h & RTL_VOLF_SPHERE) ++v[5];
      if (h & RTL_VOLF_QUADS) ++v[6];
    }
  }
  for (int k = 0; k < n && k < RT_LAYOUT_STATS; ++k) out[k] = v[k];
  return RT_OK;
}

int rt_scene_lds_check(const rt_scene_blob* blob, uint32_t flags, uint32_t n_rays, uint64_t seed,
                       uint64_t* out, int n, char* msg, uint32_t msg_len) {
  if (!out || n < 0) return set_err(RT_ERR_INVALID_ARG, "null out");
  rtf::FlatScene F;
  std::string err;
  const int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return set_err(rc, err);
  const TableLayout TL = table_layout(F);
  // the product kernel's plan on a device whose workgroups may take the CU's whole LDS
  const LdsPlan L = plan_lds(F.hdr, (uint32_t)TL.o_perl, flags, true, kLdsTotal);
  const rtf::WalkCheck W = rtf::check_compact_trees(F.nodes, F.hdr, n_rays, seed);
  const uint64_t v[RT_LDS_CHECK] = {
      (uint64_t)L.block, L.static_lds, L.stage_bytes, L.cbvh_lds_off, L.cbvh_bytes, L.stack_lds_off,
      F.hdr.cbvh_stack, L.lds_bytes, L.static_lds + L.lds_bytes, kLdsTotal, W.trees, W.max_depth,
      W.errors, W.max_store_slot, W.max_live, W.rays, W.steps, W.max_read, L.row_lds_off};
  for (int k = 0; k < n && k < RT_LDS_CHECK; ++k) out[k] = v[k];
  if (msg && msg_len) {
    std::strncpy(msg, W.first_error.c_str(), msg_len - 1);
    msg[msg_len - 1] = '\0';
  }
  return RT_OK;
}

int rt_scene_create(const rt_scene_blob* blob, int device, rt_scene** out) {
  if (!out) return set_err(RT_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  rtf::FlatScene F;
  std::string err;
  int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return set_err(rc, err);
  {
    // The LDS walk (rt_kernel.h cbvh_walk_t) trusts the compact trees: its only global loads are
    // the leaf records it reaches through their references, and its stack stores are bounded by
    // the header's cbvh_stack. Every tree is checked before upload (structure, references, leaf
    // records, depth; no ray walks): a malformed tree is refused here, not met on the device.
    const rtf::WalkCheck W = rtf::check_compact_trees(F.nodes, F.hdr, 0, 0);
    if (W.errors) return set_err(RT_ERR_BAD_BLOB, "compact BVH check: " + W.first_error);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_err(RT_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return set_err(RT_ERR_INVALID_ARG, "bad device ordinal");
  HIP_TRY(hipSetDevice(device));
  // Pack the tables into one allocation, in the order the kernel stages them into LDS (a
  // prefix of it: nodes, materials, textures, lights, light offsets, Perlin tables), 16-byte
  // aligned; texels last (never staged).
  const TableLayout TL = table_layout(F);
  const size_t o_nodes = TL.o_nodes, s_nodes = F.nodes.size() * 4;
  const size_t o_mats = TL.o_mats, s_mats = F.mats.size() * 4;
  const size_t o_texs = TL.o_texs, s_texs = F.texs.size() * 4;
  const size_t o_lig = TL.o_lig, s_lig = F.lights.size() * 4;
  const size_t o_loff = TL.o_loff, s_loff = F.light_offs.size() * 4;
  const size_t o_perl = TL.o_perl, s_perl = F.perlin.size();
  const size_t o_tx = TL.o_tx, s_tx = F.texels.size();
  const size_t total = TL.total;
  std::vector<uint8_t> host(total, 0);
  auto cp = [&](size_t off, const void* src, size_t n) {
    if (n) std::memcpy(host.data() + off, src, n);
  };
  cp(o_nodes, F.nodes.data(), s_nodes);
  cp(o_mats, F.mats.data(), s_mats);
  cp(o_texs, F.texs.data(), s_texs);
  cp(o_perl, F.perlin.data(), s_perl);
  cp(o_lig, F.lights.data(), s_lig);
  cp(o_loff, F.light_offs.data(), s_loff);
  cp(o_tx, F.texels.data(), s_tx);
  rt_scene* sc = new rt_scene();
  sc->device = device;
  sc->hdr = F.hdr;
  hipError_t e = hipMalloc(&sc->dev, total);
  if (e == hipSuccess) e = hipMemcpy(sc->dev, host.data(), total, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&sc->n_cu, hipDeviceAttributeMultiprocessorCount,
                                                 device);
  int lds_block = 0;
  if (e == hipSuccess)
    e = hipDeviceGetAttribute(&lds_block, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
  if (e == hipSuccess && lds_block > 0)
    sc->lds_module_max = std::min<size_t>((size_t)lds_block, kLdsTotal);
  if (e == hipSuccess) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot > 0) sc->mem_total = tot;
  }
  for (int k = 0; k < rt_scene::kTraceRing && e == hipSuccess; ++k) {
    e = hipEventCreate(&sc->tev[k][0]);
    if (e == hipSuccess) e = hipEventCreate(&sc->tev[k][1]);
  }
  if (e != hipSuccess) {
    rt_scene_destroy(sc);
    return set_err(RT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
  }
  sc->dev_bytes = total;
  sc->nodes = (const uint32_t*)(sc->dev + o_nodes);
  sc->mats = (const uint32_t*)(sc->dev + o_mats);
  sc->texs = (const uint32_t*)(sc->dev + o_texs);
  sc->perlin = sc->dev + o_perl;
  sc->lights = (const uint32_t*)(sc->dev + o_lig);
  sc->light_offs = (const uint32_t*)(sc->dev + o_loff);
  sc->texels = sc->dev + o_tx;
  sc->o_mats = (uint32_t)o_mats;
  sc->o_texs = (uint32_t)o_texs;
  sc->o_lights = (uint32_t)o_lig;
  sc->o_loffs = (uint32_t)o_loff;
  sc->o_perl = (uint32_t)o_perl;
  const char* jit_env = std::getenv("RT_JIT");
  if (jit_env && std::strcmp(jit_env, "0") == 0) {
    sc->jit_msg = "disabled by RT_JIT=0";
  } else {
    sc->jit_walker = rtj::generate(F, &sc->jit_msg);
    sc->jit_state = sc->jit_walker.empty() ? -1 : 0;
  }
  sc->prim_word = F.prim_word;  // the ray query's prim table (rt_query.hip uploads it on first use)
  sc->prim_id = F.prim_id;
  sc->sphere_light0 = -1;
  for (size_t i = 0; i < F.light_offs.size(); ++i)
    if ((F.lights[F.light_offs[i]] & 0xffu) == RTL_SPHERE) {
      sc->sphere_light0 = (int)i;
      break;
    }
  *out = sc;
  return RT_OK;
}

void rt_scene_destroy(rt_scene* sc) {
  if (!sc) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(sc->device);
  // renders are asynchronous on the caller's streams (rt_render_device): wait for them before
  // the module cache may unload this scene's kernel code object (release_kernel evicts idle
  // modules) and before the tables and workspace are freed
  (void)hipDeviceSynchronize();
  for (const rtj::Kernel& k : sc->jit_k) rtj::release_kernel(k);  // the module cache's holds
  if (sc->dev) (void)hipFree(sc->dev);
  if (sc->prim_dev) (void)hipFree(sc->prim_dev);
  for (const auto& sl : sc->slots) {
    if (sl->work) (void)hipFree(sl->work);
    if (sl->work2) (void)hipFree(sl->work2);
    if (sl->tiles) (void)hipFree(sl->tiles);
    if (sl->ops) (void)hipFree(sl->ops);
    if (sl->done) (void)hipEventDestroy(sl->done);
    if (sl->ev0) (void)hipEventDestroy(sl->ev0);
    if (sl->ev1) (void)hipEventDestroy(sl->ev1);
  }
  for (int k = 0; k < rt_scene::kTraceRing; ++k)
    for (int j = 0; j < 2; ++j)
      if (sc->tev[k][j]) (void)hipEventDestroy(sc->tev[k][j]);
  delete sc;
  if (prev >= 0) (void)hipSetDevice(prev);
}

uint64_t rt_scene_device_bytes(const rt_scene* sc) { return sc ? sc->dev_bytes : 0; }

int rt_jit_check(const rt_scene_blob* blob, const char* arch, int* state, char* msg,
                 uint32_t msg_len) {
  if (!blob || !arch || !state) return set_err(RT_ERR_INVALID_ARG, "null argument");
  rtf::FlatScene F;
  std::string err;
  int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return set_err(rc, err);
  std::string why, out;
  const std::string walker = rtj::generate(F, &why);
  *state = walker.empty() ? -1 : 1;
  out = walker.empty() ? why : walker;
  if (!walker.empty()) {
    std::vector<char> code;
    std::string log;
    // the variant of a product render whose plan stages the scene's tables
    const rtv::Variant v = rtv::choose_variant(F.hdr, 0u, true);
    rc = rtj::compile(rtj::kernel_source(walker, v, kLaunchPlain), arch, &code, &log);
    if (rc != 0) {
      *state = -2;
      out = log;
    }
    // RT_JIT_CHECK_TILES=1 (tools/jit_cache_fill.py): the tile-list variant of the same kernel
    // too, so that the code-object cache holds both; the returned source is the plain walker's
    const char* tv = std::getenv("RT_JIT_CHECK_TILES");
    if (rc == 0 && tv && std::strcmp(tv, "1") == 0) {
      rc = rtj::compile(rtj::kernel_source(walker, v, kLaunchTiles), arch, &code, &log);
      if (rc != 0) {
        *state = -2;
        out = log;
      }
    }
    // RT_JIT_CHECK_RAYS=1: the ray variant (rt_render_rays_device) as well; the returned source is
    // then that kernel's whole translation unit, the walker and the wrapper that names the instance
    const char* rv = std::getenv("RT_JIT_CHECK_RAYS");
    if (rc == 0 && rv && std::strcmp(rv, "1") == 0) {
      const std::string src = rtj::kernel_source(walker, v, kLaunchRays);
      rc = rtj::compile(src, arch, &code, &log);
      if (rc != 0) {
        *state = -2;
        out = log;
      } else {
        out = src;
      }
    }
  }
  if (msg && msg_len) {
    std::strncpy(msg, out.c_str(), msg_len - 1);
    msg[msg_len - 1] = '\0';
  }
  return *state == -2 ? set_err(RT_ERR_HIP, out) : RT_OK;
}

int rt_scene_jit_info(rt_scene* sc, int* state, char* msg, uint32_t msg_len) {
  if (!sc || !state) return set_err(RT_ERR_INVALID_ARG, "null argument");
  std::lock_guard<std::mutex> lock(sc->mu);
  *state = sc->jit_state;
  if (msg && msg_len) {
    std::strncpy(msg, sc->jit_msg.c_str(), msg_len - 1);
    msg[msg_len - 1] = '\0';
  }
  return RT_OK;
}

}  // extern "C"

// A slot for a render on `stream` (rt_scene_impl.hpp)
int rts::acquire_slot(rt_scene* sc, std::unique_lock<std::mutex>& lock, hipStream_t stream,
                      RenderSlot** out) {
  for (;;) {
    RenderSlot* pick = nullptr;
    for (const auto& sl : sc->slots) {
      if (sl->held) continue;
      if (sl->recorded && sl->last_stream == stream) {  // stream order: no wait needed
        pick = sl.get();
        break;
      }
      if (!pick) {
        const hipError_t q = sl->recorded ? hipEventQuery(sl->done) : hipSuccess;
        if (q == hipSuccess) pick = sl.get();
        else if (q != hipErrorNotReady) return set_err(RT_ERR_HIP, std::string("slot event: ") + hipGetErrorString(q));
      }
    }
    if (!pick && (int)sc->slots.size() < rt_scene::kMaxSlots) {
      std::unique_ptr<RenderSlot> sl(new RenderSlot());
      hipError_t e = hipMalloc(&sl->ops, sizeof(unsigned long long) * 64 + 256);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&sl->done, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreate(&sl->ev0);
      if (e == hipSuccess) e = hipEventCreate(&sl->ev1);
      if (e != hipSuccess) {
        if (sl->ops) (void)hipFree(sl->ops);
        if (sl->done) (void)hipEventDestroy(sl->done);
        if (sl->ev0) (void)hipEventDestroy(sl->ev0);
        if (sl->ev1) (void)hipEventDestroy(sl->ev1);
        return set_err(RT_ERR_HIP, std::string("render slot: ") + hipGetErrorString(e));
      }
      sl->queue = (unsigned int*)(sl->ops + 32);
      sc->slots.push_back(std::move(sl));
      pick = sc->slots.back().get();
    }
    if (!pick) {  // every slot busy: wait for the oldest unheld one, or for a release
      for (const auto& sl : sc->slots)
        if (!sl->held) {
          pick = sl.get();
          break;
        }
      if (pick) {
        HIP_TRY(hipEventSynchronize(pick->done));
      } else {
        sc->slot_cv.wait(lock);
        continue;
      }
    }
    if (pick->recorded) HIP_TRY(hipStreamWaitEvent(stream, pick->done, 0));
    pick->held = true;
    sc->last_slot = (int)(std::find_if(sc->slots.begin(), sc->slots.end(),
                                       [&](const std::unique_ptr<RenderSlot>& u) {
                                         return u.get() == pick;
                                       }) - sc->slots.begin());
    *out = pick;
    return RT_OK;
  }
}

int rts::check_render_args(const rt_camera* cam, const rt_render_opts* opts, bool path_depth,
                           int sj_step, int* sj0_out, int* n_sj_out) {
  const int W = cam->image_width, S = cam->sqrt_spp;
  if (W <= 0 || cam->image_height <= 0 || S <= 0 ||
      (path_depth && (cam->max_depth < 0 || cam->max_depth > 0xffffff)) || opts->n_rows < 0 ||
      opts->row_step <= 0 || opts->row_begin < 0)
    return set_err(RT_ERR_INVALID_ARG, "bad camera or row range");
  if (opts->n_rows > 0 &&
      (int64_t)opts->row_begin + (int64_t)(opts->n_rows - 1) * opts->row_step >= cam->image_height)
    return set_err(RT_ERR_INVALID_ARG, "row range outside the image");
  if ((int64_t)W * cam->image_height >= (1ll << 32) || (int64_t)S * S >= (1ll << 32))
    return set_err(RT_ERR_UNSUPPORTED, "image or spp too large for 32-bit pixel/sample keys");
  // lane item keys pack x (16 bits), the call's row index (15 bits), s_j (15 bits, beside the
  // row-item bit) and s_i (16 bits)
  if (W > 65535 || opts->n_rows > 32767)
    return set_err(RT_ERR_UNSUPPORTED, "image_width > 65535 or n_rows > 32767 in one call");
  if (S > 32768) return set_err(RT_ERR_UNSUPPORTED, "spp > 2^30 (sqrt_spp > 32768)");
  const int sj0 = opts->sj_count > 0 ? opts->sj_begin : 0;
  const int n_sj = opts->sj_count > 0 ? opts->sj_count : S;
  if (sj0 < 0 || (int64_t)sj0 + (int64_t)(n_sj - 1) * sj_step + 1 > S)
    return set_err(RT_ERR_INVALID_ARG, "bad stratum range");
  *sj0_out = sj0;
  *n_sj_out = n_sj;
  return RT_OK;
}

void rts::fill_trace_params(TraceParams* Pp, const rt_scene* sc, const rt_camera* cam,
                            const rt_render_opts* opts, const LdsPlan& LP) {
  TraceParams& P = *Pp;
  std::memset(&P, 0, sizeof(P));
  P.nodes = sc->nodes;
  P.mats = sc->mats;
  P.texs = sc->texs;
  P.perlin = sc->perlin;
  P.lights = sc->lights;
  P.light_offs = sc->light_offs;
  P.texels = sc->texels;
  P.root = sc->hdr.root;
  P.n_lights = sc->hdr.n_lights;
  P.lights_is_list = sc->hdr.lights_is_list;
  P.lights_nested = sc->hdr.lights_nested;
  P.inv_n_lights = sc->hdr.n_lights ? 1.0 / (double)sc->hdr.n_lights : 0.0;
  P.sphere_light0 = sc->sphere_light0;
  P.flags = opts->flags;
  // LDS: staged tables, then the compact ordered BVHs (rt_layout.h CBVH) with the walk's
  // per-lane stacks, or as much of the reference BVH region as fits (plan_lds); with the compact
  // trees in LDS the reference BVH region stays in global memory (only lanes flagged for the
  // reference-order re-walk read it)
  P.stage_scene = LP.stage_scene;
  P.n_perlin_lds = LP.n_perlin_lds;
  P.stage_src = LP.stage_scene ? sc->dev : sc->perlin;
  P.stage_bytes = LP.stage_bytes;
  P.bvh_words = sc->hdr.bvh_words;
  P.cbvh_src = (const uint8_t*)(sc->nodes + sc->hdr.cbvh_word0);
  P.cbvh_bytes = LP.cbvh_bytes;
  P.cbvh_lds_off = LP.cbvh_lds_off;
  P.stack_lds_off = LP.stack_lds_off;
  P.bvh_lds_words = LP.bvh_lds_words;
  P.bvh_lds_off = LP.bvh_lds_off;
  P.row_lds_off = LP.row_lds_off;
  P.o_mats = sc->o_mats;
  P.o_texs = sc->o_texs;
  P.o_lights = sc->o_lights;
  P.o_loffs = sc->o_loffs;
  P.o_perl = sc->o_perl;
  for (int k = 0; k < 3; ++k) {
    P.center[k] = cam->center[k];
    P.p00[k] = cam->pixel00_loc[k];
    P.du[k] = cam->pixel_delta_u[k];
    P.dv[k] = cam->pixel_delta_v[k];
    P.ddu[k] = cam->defocus_disk_u[k];
    P.ddv[k] = cam->defocus_disk_v[k];
    P.bg[k] = cam->background[k];
    P.bg_w[k] = (float)cam->background[k];  // the f32 weight the path kernel multiplies by
  }
  P.rs = cam->recip_sqrt_spp;
  P.defocus = cam->defocus_angle > 0.0;
  P.W = cam->image_width;
  P.n_rows = opts->n_rows;
  P.row_begin = opts->row_begin;
  P.row_step = opts->row_step;
  P.sqrt_spp = cam->sqrt_spp;
  P.max_depth = cam->max_depth;
  P.seed_lo = (uint32_t)opts->seed;
  P.seed_hi = (uint32_t)(opts->seed >> 32);
  P.tiles_x = (cam->image_width + kWaveTile - 1) / kWaveTile;
  P.sj_step = 1;
  P.n_blk = (cam->sqrt_spp + kPoolSi - 1) / kPoolSi;
}

int rts::resident_blocks(rt_scene* sc, const void* kernel, hipFunction_t module, int block,
                         size_t lds_bytes, const char* what, int* out) {
  const void* key = module ? (const void*)module : kernel;
  auto it = std::find_if(sc->resident.begin(), sc->resident.end(),
                         [&](const rt_scene::Resident& r) { return r.kernel == key; });
  if (it == sc->resident.end() || it->lds != lds_bytes) {
    int nb = 0;
    const hipError_t oe =
        module ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, module, block, lds_bytes)
               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, lds_bytes);
    if (oe != hipSuccess || nb <= 0)
      return set_err(RT_ERR_HIP, std::string("occupancy query: the ") + what +
                                     " does not fit a CU (" +
                                     (oe != hipSuccess ? hipGetErrorString(oe) : "0 blocks") + ")");
    if (it == sc->resident.end()) it = sc->resident.insert(it, rt_scene::Resident{key, 0, 0});
    it->lds = lds_bytes;
    it->blocks = nb;
  }
  *out = it->blocks;
  return RT_OK;
}

int rts::complete_render(SlotHold& hold, hipStream_t stream, rt_stats* stats,
                         const rt_stats& counts, bool read_ops,
                         std::chrono::steady_clock::time_point t0) {
  RenderSlot* const sl = hold.sl;
  if (stats) HIP_TRY(hipEventRecord(sl->ev1, stream));
  HIP_TRY(hipEventRecord(sl->done, stream));
  sl->recorded = true;
  sl->last_stream = stream;
  hold.finished = true;
  if (stats) {
    hold.lock.unlock();  // the slot stays held: other renders of the scene go on meanwhile
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, sl->ev0, sl->ev1));
    stats->ms_kernel = ms;
    stats->samples = counts.samples;
    stats->out_bytes = counts.out_bytes;
    stats->launches = counts.launches;
    if (read_ops) {
      unsigned long long h[32];
      HIP_TRY(hipMemcpy(h, sl->ops, sizeof(h), hipMemcpyDeviceToHost));
      for (int k = 0; k < 32; ++k) stats->ops[k] = h[k];
    }
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return RT_OK;
}

// A tile-list render's list (rt_render_tiles_device), validated by the entry point: strictly
// ascending indices of the call's tile grid. n_px: the pixels of the listed tiles.
struct TileJob {
  const uint32_t* tiles;
  uint32_t n_list;
  int sj_step;
  uint64_t n_px;
};
// A ray render's batch (rt_render_rays_device), its arguments checked by the entry point
struct RayJob {
  const rt_ray* rays;  // device
  uint64_t n_rays;
  uint32_t skip, mode;
};

namespace {

// The kernel of a render: the ahead-of-time instance of the scene's variant (rt_variant.h), and
// for product renders of a generated scene its scene-specialised kernel (same template arguments
// and launch bounds, top-level walk unrolled; rt_jit.cpp), compiled on the first such render.
struct PathKernel {
  kern_t kern = nullptr;
  hipFunction_t jfn = nullptr;  // runs instead of kern when set
};
int select_kernel(rt_scene* sc, uint32_t flags, const LdsPlan& LP, int launch, bool want_jit,
                  PathKernel* out) {
  const rtv::Variant v = rtv::choose_variant(sc->hdr, flags, LP.stage_scene != 0);
  out->kern = launch == kLaunchTiles  ? tile_trace_kernel(v)
              : launch == kLaunchRays ? ray_trace_kernel(v)
                                      : trace_kernel(v, (flags & RT_FLAG_COUNT_OPS) != 0);
  if (!out->kern)
    return set_err(RT_ERR_INVALID_ARG, launch == kLaunchTiles  ? "no tile-list variant of this kernel"
                                       : launch == kLaunchRays ? "no ray variant of this kernel"
                                                               : "no ahead-of-time kernel of this variant");
  if (!want_jit || LP.lds_bytes + LP.static_lds > sc->lds_module_max) return RT_OK;
  rtj::Kernel& jk = sc->jit_k[launch];
  if (!jk.fn) {
    std::string log;
    if (rtj::get_kernel(sc->jit_walker, sc->device, v, launch, &jk, &log) != 0) {
      sc->jit_state = -2;
      sc->jit_msg = log;
    } else {
      // a dispatch the hardware cannot place aborts the whole queue (the CP's register or
      // LDS check), so the code object's resources are checked against this launch first:
      // workgroup size, VGPRs x waves per SIMD within the 512-entry file, LDS within the CU
      const int waves_per_simd = (LP.block / 64 + 3) / 4;
      const int regs = (jk.regs + 7) & ~7;
      char why[256];
      std::snprintf(why, sizeof(why),
                    "scene-specialised kernel%s: %d regs, max %d threads, %d B static LDS, "
                    "%d B scratch/lane; launch %d threads, %zu B dynamic LDS",
                    jk.cached ? " (code-object cache)" : "", jk.regs, jk.max_threads,
                    jk.static_lds, jk.scratch, LP.block, LP.lds_bytes);
      if (jk.max_threads < LP.block || regs * waves_per_simd > 512 ||
          (size_t)jk.static_lds + LP.lds_bytes > sc->lds_module_max ||
          (size_t)jk.static_lds > LP.static_lds) {
        sc->jit_state = -2;
        sc->jit_msg = std::string("not launched: ") + why;
        rtj::release_kernel(jk);
        jk = rtj::Kernel{};
      } else {
        sc->jit_msg = why;
      }
    }
  }
  if (jk.fn) {
    sc->jit_state = 1;
    out->jfn = jk.fn;
  }
  return RT_OK;
}

// Outputs (TraceParams::part): one f64 RGB value per (pixel, s_j) of the row pairs, one per
// (pixel, s_j, block) of the segment pairs and one per sample of the tail pairs.
//  * A launch of many pairs per resident wave (a whole frame on one GPU: C2 has 60) renders
//    row items, then a band of segment items about four pairs per resident wave long, then a
//    tail of single samples an eighth of a pair per wave long. When the row pools run out, the
//    lanes still finishing a row have up to sqrt_spp paths left (rows through glass take
//    several times the mean), and the band keeps the other lanes busy meanwhile; the tail
//    does the same for the segments' last ~kPoolSi / 2 samples. The workspace is then about
//    one value per (pixel, s_j): C2 0.59 GB instead of 2.1.
//  * Smaller launches (an N-way share, chunks) balance better without rows (C2 over 8 GPUs:
//    0.940 of ideal with segments, 0.894 with half the pairs as rows, profiles/
//    r03_scaling_probe_*.log): segment items, then a tail of one pair per resident wave.
//  * BVH kernels render rows when their plan fits the row totals beside the compact trees.
// RT_SEG_PAIRS (rows with that band) and RT_TAIL_PAIRS override the sizes (tests: the image
// does not depend on the split).
struct WorkIn {
  int n_tiles, n_sj, S, n_blk;  // the launch's tiles, the call's stratum rows, sqrt_spp, its blocks
  int64_t res_waves;            // waves the device holds at once
  bool rows_ok;                 // the kernel renders row items
  size_t n_carry;               // pixels (or pixel slots of the list) carried between chunks
  size_t mem_total;             // device memory
  const char *seg_pairs, *tail_pairs, *workspace_mb;  // RT_SEG_PAIRS, RT_TAIL_PAIRS, RT_WORKSPACE_MB
};
struct Split {
  int64_t pairs, r, a, values;  // row pairs [0, r), segment pairs [r, a), tail [a, pairs)
};
Split split_pairs(const WorkIn& in, int cn) {
  Split sp;
  sp.pairs = (int64_t)in.n_tiles * cn;
  const bool rows = in.rows_ok && (in.seg_pairs ? true : sp.pairs >= 24 * in.res_waves);
  int64_t tail = rows ? std::max<int64_t>(1, in.res_waves / 8) : in.res_waves;
  if (in.tail_pairs) tail = std::strtoll(in.tail_pairs, nullptr, 10);
  const int64_t band = in.seg_pairs ? std::strtoll(in.seg_pairs, nullptr, 10) : 4 * in.res_waves;
  const int64_t tb = std::min<int64_t>(sp.pairs, std::max<int64_t>(0, tail));
  sp.a = sp.pairs - tb;
  sp.r = rows ? std::max<int64_t>(0, sp.a - std::max<int64_t>(0, band)) : 0;
  sp.values = sp.r + (sp.a - sp.r) * in.n_blk + tb * in.S;  // 64-value slots
  return sp;
}
constexpr size_t kValBytes = (size_t)64 * 3 * sizeof(double);  // one f64 RGB value per pixel
size_t part_bytes(const WorkIn& in, int cn) { return (size_t)split_pairs(in, cn).values * kValBytes; }
// The workspace of a render: the chunks' carries (one f64 RGB value per pixel of the call, or per
// pixel slot of the list), then the largest chunk's outputs. Chunks of stratum rows keep it under
// RT_WORKSPACE_MB (default 40 GiB, at most a quarter of the device's memory): the whole C5 frame
// (3840 x 2160, 10000 spp, ~19 GB of row totals) renders in one launch; 800x800 x 961 spp takes
// one (~0.59 GB). A pure function of `in`.
struct WorkPlan {
  int chunk;          // stratum rows per launch
  size_t tot_bytes;   // the carries
  size_t need;        // the whole workspace
  bool indexable;     // the chunk's outputs and pools fit their 32- and 31-bit indices
};
WorkPlan plan_workspace(const WorkIn& in) {
  WorkPlan wp;
  wp.tot_bytes = (in.n_carry * 3 * sizeof(double) + 255) & ~(size_t)255;
  // a launch's f64 RGB outputs are indexed in 32 bits (end_sample) and its pools in 31
  auto indexable = [&](int cn) {
    const Split sp = split_pairs(in, cn);
    return sp.values * 64 < (1ll << 32) && sp.r + (sp.pairs - sp.r) * in.n_blk <= 0x7fffffff;
  };
  size_t cap = std::min<size_t>((size_t)40960 << 20, in.mem_total / 4);
  if (in.workspace_mb) cap = (size_t)std::strtoull(in.workspace_mb, nullptr, 10) << 20;
  wp.chunk = in.n_sj;
  while (wp.chunk > 1 && (wp.tot_bytes + part_bytes(in, wp.chunk) > cap || !indexable(wp.chunk)))
    wp.chunk = (wp.chunk + 1) / 2;
  wp.need = wp.tot_bytes + part_bytes(in, wp.chunk);
  wp.indexable = indexable(wp.chunk);
  return wp;
}

// The slot's buffers for this render: the workspace, a moments render's second carry when it runs
// in several chunks, a tile-list render's list. Each is touched only after the slot's previous
// render (another stream's, or this one's) has finished with it.
int grow_slot(RenderSlot* sl, const WorkPlan& wp, bool m2_chunked, const TileJob* tj) {
  if (wp.need > sl->work_bytes) {
    if (sl->recorded) HIP_TRY(hipEventSynchronize(sl->done));
    if (sl->work) HIP_TRY(hipFree(sl->work));
    sl->work = nullptr;
    sl->work_bytes = 0;
    HIP_TRY(hipMalloc(&sl->work, wp.need));
    sl->work_bytes = wp.need;
  }
  // a moments render in several chunks carries its second moments in a buffer of the slot's own,
  // allocated by the first such render (plain renders never pay for it)
  if (m2_chunked && wp.tot_bytes > sl->work2_bytes) {
    if (sl->recorded) HIP_TRY(hipEventSynchronize(sl->done));
    if (sl->work2) HIP_TRY(hipFree(sl->work2));
    sl->work2 = nullptr;
    sl->work2_bytes = 0;
    HIP_TRY(hipMalloc(&sl->work2, wp.tot_bytes));
    sl->work2_bytes = wp.tot_bytes;
  }
  if (tj) {
    // the list travels through the slot: a host copy (the caller may free its list on return) and
    // a device buffer, both touched only after the slot's previous render has finished (its
    // kernels read the device buffer, its upload the host copy)
    if (sl->recorded && (sl->tiles_busy || tj->n_list > sl->tiles_cap))
      HIP_TRY(hipEventSynchronize(sl->done));
    sl->tiles_busy = false;
    if (tj->n_list > sl->tiles_cap) {
      if (sl->tiles) HIP_TRY(hipFree(sl->tiles));
      sl->tiles = nullptr;
      sl->tiles_cap = 0;
      HIP_TRY(hipMalloc(&sl->tiles, (size_t)tj->n_list * sizeof(uint32_t)));
      sl->tiles_cap = tj->n_list;
    }
    sl->tiles_host.assign(tj->tiles, tj->tiles + tj->n_list);
  }
  return RT_OK;
}

// One rt_reduce launch over (M2, launch kind), with the instance's own MomentsOut / TileIn
// arguments, of the chunk P describes; the carries live in the slot (tot2: only between chunks)
template <bool M2, int LK>
void launch_reduce(const TraceParams& P, RenderSlot* sl, float* accum, float* m2, int n_tiles,
                   int mode, hipStream_t stream) {
  MomentsOut<M2> mo;
  if constexpr (M2) mo = {(double*)sl->work2, m2};
  TileIn<LK> ti;
  if constexpr (LK == kLaunchTiles) ti = {sl->tiles};
  if constexpr (LK == kLaunchRays) ti = {P.rays, P.n_rays};
  hipLaunchKernelGGL((rt_reduce<M2, LK>), dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0,
                     stream, P.part, (double*)sl->work, accum, P.W, P.n_rows, P.tiles_x, n_tiles,
                     P.n_sj, P.sqrt_spp, P.n_pairs_r, P.n_pairs_a, mode, mo, ti);
}

// The launches of a render: per chunk of stratum rows sj0 + (k0 .. k0 + cn - 1) * sj_step one path
// kernel over the chunk's pools and one rt_reduce into the carries or, last, the accumulator.
int launch_chunks(rt_scene* sc, RenderSlot* sl, const PathKernel& K, TraceParams& P,
                  const LdsPlan& LP, const WorkIn& in, const WorkPlan& wp, int64_t max_blocks,
                  int sj0, uint32_t flags, float* accum, float* m2, int launch,
                  hipStream_t stream, rt_stats* counts) {
  // (ray renders have no moments: the entry point passes no second buffer)
  static void (*const reduce[2][3])(const TraceParams&, RenderSlot*, float*, float*, int, int,
                                    hipStream_t) = {
      {launch_reduce<false, kLaunchPlain>, launch_reduce<false, kLaunchTiles>,
       launch_reduce<false, kLaunchRays>},
      {launch_reduce<true, kLaunchPlain>, launch_reduce<true, kLaunchTiles>, nullptr}};
  const int block = LP.block;
  for (int k0 = 0; k0 < in.n_sj; k0 += wp.chunk) {
    const int cn = std::min(wp.chunk, in.n_sj - k0);
    counts->out_bytes += part_bytes(in, cn);
    ++counts->launches;
    const Split sp = split_pairs(in, cn);
    P.sj0 = sj0 + k0 * P.sj_step;
    P.n_sj = cn;
    P.n_pairs_r = (int)sp.r;
    P.n_pairs_a = (int)sp.a;
    P.n_pools = (int)(sp.r + (sp.pairs - sp.r) * P.n_blk);
    // persistent grid: as many waves as the device holds at once (never more than pools)
    const int64_t blocks = std::min(max_blocks, ((int64_t)P.n_pools + (block / 64) - 1) / (block / 64));
    HIP_TRY(hipMemsetAsync(sl->queue, 0, sizeof(unsigned int), stream));
    const int ring = (int)(sc->n_tev % rt_scene::kTraceRing);
    HIP_TRY(hipEventRecord(sc->tev[ring][0], stream));
    if (K.jfn) {
      void* args[] = {&P};
      HIP_TRY(hipModuleLaunchKernel(K.jfn, (unsigned)blocks, 1, 1, (unsigned)block, 1, 1,
                                    (unsigned)LP.lds_bytes, stream, args, nullptr));
    } else {
      hipLaunchKernelGGL(K.kern, dim3((unsigned)blocks), dim3(block), LP.lds_bytes, stream, P);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc->tev[ring][1], stream));
    sc->tev_render[ring] = sc->n_render;
    ++sc->n_tev;
    const int mode =
        (k0 == 0 ? 1 : 0) | (k0 + cn == in.n_sj ? 2 : 0) | ((flags & RT_FLAG_OVERWRITE) ? 4 : 0);
    reduce[m2 != nullptr][launch](P, sl, accum, m2, in.n_tiles, mode, stream);
    HIP_TRY(hipGetLastError());
  }
  return RT_OK;
}

}  // namespace

// m2 != nullptr: a moments render (rt_render_moments_device), which also writes the second
// moments of the row totals; every other step is the plain render's. tj != nullptr: a tile-list
// render (rt_render_tiles_device): the launch's pairs run over the list's entries and the strided
// stratum rows sj_begin + k * sj_step, through the TILES variants of the same kernels; LDS plan,
// kernel choice, slot, chunking and stats are shared. rj != nullptr: a ray render
// (rt_render_rays_device): cam and opts describe the batch as an image 8 pixels wide and
// ceil(n_rays / 8) rows tall (no 32760-row sub-calls: a ray item's key is the ray index, not x and
// row), every stratum row of it, through the RAYS variants; accum is the caller's n_rays * 3 floats.
static int render_device_rows(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts,
                              float* accum, float* m2, const TileJob* tj, void* stream_v,
                              rt_stats* stats, const RayJob* rj = nullptr) {
  auto t0 = std::chrono::steady_clock::now();
  const int launch = rj ? kLaunchRays : tj ? kLaunchTiles : kLaunchPlain;
  int sj0 = 0, n_sj = cam->sqrt_spp;
  if (!rj) RT_TRY(check_render_args(cam, opts, true, tj ? tj->sj_step : 1, &sj0, &n_sj));
  if (sc->hdr.n_lights == 0 && (opts->flags & RT_FLAG_SEMANTICS_REFERENCE) && sc->hdr.pdf_materials)
    return set_err(RT_ERR_EMPTY_LIGHTS,
                   "empty light list with a diffuse/volume material: the reference panics "
                   "(hittable.rs:115-129)");
  std::unique_lock<std::mutex> lock(sc->mu);
  hipStream_t stream = (hipStream_t)stream_v;
  HIP_TRY(hipSetDevice(sc->device));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const size_t n_px = rj ? (size_t)rj->n_rays : (size_t)opts->n_rows * cam->image_width;
  if (n_px == 0) return RT_OK;
  SlotHold hold{sc, lock};
  RT_TRY(acquire_slot(sc, lock, stream, &hold.sl));
  RenderSlot* const sl = hold.sl;
  const bool count = (opts->flags & RT_FLAG_COUNT_OPS) != 0;
#ifdef RT_PROF  // profiling build: the product kernels also fill the ops buffer (section cycles)
  const bool ops_buf = true;
#else
  const bool ops_buf = count;
#endif
  const bool want_jit = !count && !(opts->flags & RT_FLAG_INTERPRETER) && sc->jit_state >= 0;
  const LdsPlan LP = plan_lds(sc->hdr, sc->o_perl, opts->flags, want_jit, sc->lds_module_max);
  TraceParams P;
  fill_trace_params(&P, sc, cam, opts, LP);
  P.ops = sl->ops;
  P.queue = sl->queue;
  if (tj) P.sj_step = tj->sj_step;
  if (rj) {
    P.rays = reinterpret_cast<const uint4*>(rj->rays);
    P.n_rays = (uint32_t)rj->n_rays;
    P.rays_skip = rj->skip;
    P.rays_mode = rj->mode;
  }
  PathKernel K;
  RT_TRY(select_kernel(sc, opts->flags, LP, launch, want_jit, &K));
  // (module kernels take their dynamic LDS size at launch)
  if (!K.jfn && LP.lds_bytes > (64u << 10))
    HIP_TRY(hipFuncSetAttribute((const void*)K.kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)LP.lds_bytes));
  int resident = 0;
  RT_TRY(resident_blocks(sc, (const void*)K.kern, K.jfn, LP.block, LP.lds_bytes, "path kernel",
                         &resident));
  const int64_t max_blocks = (int64_t)resident * std::max(1, sc->n_cu);
  // the launch's tiles: the call's whole grid, or the entries of the list
  const int n_tiles = tj ? (int)tj->n_list : P.tiles_x * ((opts->n_rows + kWaveTile - 1) / kWaveTile);
  // (a ray batch: tiles_x = 1, so ceil(n_rays / 64) tiles, carried as whole tiles)
  const WorkIn in{n_tiles, n_sj, cam->sqrt_spp, P.n_blk, max_blocks * (LP.block / 64),
                  !sc->hdr.has_bvh || LP.row_lds_off != ~0u, tj || rj ? (size_t)n_tiles * 64 : n_px,
                  sc->mem_total, std::getenv("RT_SEG_PAIRS"), std::getenv("RT_TAIL_PAIRS"),
                  std::getenv("RT_WORKSPACE_MB")};
  const WorkPlan wp = plan_workspace(in);
  if (!wp.indexable) return set_err(RT_ERR_UNSUPPORTED, "grid too large");
  RT_TRY(grow_slot(sl, wp, m2 && wp.chunk < n_sj, tj));
  if (tj) P.tile_list = sl->tiles;
  P.part = (double*)(sl->work + wp.tot_bytes);
  hold.stream = stream;
  hold.enqueued = true;  // from here on a failure still records `done` (SlotHold)
  if (ops_buf) HIP_TRY(hipMemsetAsync(sl->ops, 0, sizeof(unsigned long long) * 32, stream));
  if (tj) {
    sl->tiles_busy = true;
    HIP_TRY(hipMemcpyAsync(sl->tiles, sl->tiles_host.data(), (size_t)tj->n_list * sizeof(uint32_t),
                           hipMemcpyHostToDevice, stream));
  }
#ifdef RT_PROF
  HIP_TRY(hipMemsetAsync(sl->ops + 40, 0, sizeof(unsigned long long) * 21, stream));
#endif
  if (stats) HIP_TRY(hipEventRecord(sl->ev0, stream));
  rt_stats counts{};
  counts.samples = (uint64_t)(tj ? tj->n_px : n_px) * (uint64_t)n_sj * (uint64_t)cam->sqrt_spp;
  RT_TRY(launch_chunks(sc, sl, K, P, LP, in, wp, max_blocks, sj0, opts->flags, accum, m2,
                       launch, stream, &counts));
  ++sc->n_render;
  return complete_render(hold, stream, stats, counts, ops_buf, t0);
}

// rt_render_device and rt_render_moments_device (m2 != nullptr): tall row ranges as sub-calls
static int render_device_split(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts,
                               float* accum, float* m2, void* stream_v, rt_stats* stats) {
  if (opts->n_rows <= kRowsPerCall || cam->image_width <= 0)
    return render_device_rows(sc, cam, opts, accum, m2, nullptr, stream_v, stats);
  auto t0 = std::chrono::steady_clock::now();
  rt_stats part{}, sum{};
  for (int k0 = 0; k0 < opts->n_rows; k0 += kRowsPerCall) {
    rt_render_opts o = *opts;
    o.row_begin = opts->row_begin + k0 * opts->row_step;
    o.n_rows = std::min(kRowsPerCall, opts->n_rows - k0);
    const size_t off = (size_t)k0 * cam->image_width * 3;
    const int rc = render_device_rows(sc, cam, &o, accum + off, m2 ? m2 + off : nullptr, nullptr,
                                      stream_v, stats ? &part : nullptr);
    if (rc != RT_OK) return rc;
    if (stats) {
      sum.ms_kernel += part.ms_kernel;
      sum.samples += part.samples;
      sum.out_bytes += part.out_bytes;
      sum.launches += part.launches;
      for (int k = 0; k < 32; ++k) sum.ops[k] += part.ops[k];
    }
  }
  if (stats) {
    sum.ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *stats = sum;
  }
  return RT_OK;
}

extern "C" {

int rt_render_device(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts,
                     float* accum, void* stream_v, rt_stats* stats) {
  if (!sc || !cam || !opts || !accum) return set_err(RT_ERR_INVALID_ARG, "null argument");
  return render_device_split(sc, cam, opts, accum, nullptr, stream_v, stats);
}

int rt_render_moments_device(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts,
                             float* accum, float* m2, void* stream_v, rt_stats* stats) {
  if (!sc || !cam || !opts || !accum || !m2) return set_err(RT_ERR_INVALID_ARG, "null argument");
  return render_device_split(sc, cam, opts, accum, m2, stream_v, stats);
}

int rt_render_tiles_device(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts,
                           const uint32_t* tiles, uint32_t n_list, int32_t sj_step, float* accum,
                           float* m2, void* stream_v, rt_stats* stats) {
  if (!sc || !cam || !opts || !accum || (!tiles && n_list))
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (opts->flags & RT_FLAG_COUNT_OPS)
    return set_err(RT_ERR_INVALID_ARG, "RT_FLAG_COUNT_OPS: no tile-list variant of the counting kernels");
  if (cam->image_width <= 0 || opts->n_rows < 0) return set_err(RT_ERR_INVALID_ARG, "bad size");
  if (sj_step < 1 || opts->sj_count < 1 || opts->sj_begin < 0)
    return set_err(RT_ERR_INVALID_ARG, "tile render: sj_step >= 1, sj_count >= 1, sj_begin >= 0");
  if (opts->n_rows > kRowsPerCall)
    return set_err(RT_ERR_UNSUPPORTED, "tile render: n_rows > 32760 in one call");
  // the device never sees an unvalidated tile index: strictly ascending, inside the call's grid
  const int64_t W = cam->image_width, H = opts->n_rows;
  const int64_t tiles_x = (W + kWaveTile - 1) / kWaveTile, tiles_y = (H + kWaveTile - 1) / kWaveTile;
  uint64_t n_px = 0;
  for (uint32_t k = 0; k < n_list; ++k) {
    const int64_t t = tiles[k];
    if (t >= tiles_x * tiles_y || (k && tiles[k] <= tiles[k - 1]))
      return set_err(RT_ERR_INVALID_ARG, "tile list: entries must be strictly ascending and inside the grid");
    const int64_t tx = t % tiles_x, ty = t / tiles_x;
    n_px += (uint64_t)(std::min<int64_t>(kWaveTile, W - tx * kWaveTile) *
                       std::min<int64_t>(kWaveTile, H - ty * kWaveTile));
  }
  if (n_list == 0 || opts->n_rows == 0) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return RT_OK;
  }
  const TileJob tj{tiles, n_list, (int)sj_step, n_px};
  return render_device_rows(sc, cam, opts, accum, m2, &tj, stream_v, stats);
}

// made before the scene is read and before any HIP call
static int check_rays_args(const rt_scene* sc, const rt_rays_params* rp, const rt_ray* rays,
                           uint64_t n_rays, const float* rgb) {
  if (!sc || !rp || !rays || !rgb) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (n_rays >= (1ull << 31)) return set_err(RT_ERR_INVALID_ARG, "n_rays >= 2^31");
  if (rp->flags & ~(RT_FLAG_OVERWRITE | RT_FLAG_INTERPRETER | RT_FLAG_REFERENCE_BVH |
                    RT_FLAG_SEMANTICS_REFERENCE))
    return set_err(RT_ERR_INVALID_ARG,
                   "ray renders take RT_FLAG_OVERWRITE, INTERPRETER, REFERENCE_BVH and "
                   "SEMANTICS_REFERENCE only (the counting kernels have no ray variant)");
  if (rp->mode & ~RT_RAYS_STREAM_TIME) return set_err(RT_ERR_INVALID_ARG, "unknown ray-render mode bits");
  if (rp->_pad0 != 0u) return set_err(RT_ERR_INVALID_ARG, "rt_rays_params._pad0 must be 0");
  if (rp->sqrt_paths < 1 || rp->max_depth < 0)
    return set_err(RT_ERR_INVALID_ARG, "sqrt_paths < 1 or max_depth < 0");
  if (rp->stream_skip > RT_RAYS_MAX_SKIP)
    return set_err(RT_ERR_INVALID_ARG, "stream_skip > RT_RAYS_MAX_SKIP");
  if ((rp->mode & RT_RAYS_STREAM_TIME) && rp->stream_skip == 0u)
    return set_err(RT_ERR_INVALID_ARG, "RT_RAYS_STREAM_TIME needs stream_skip >= 1");
  if ((uintptr_t)rays % 16u) return set_err(RT_ERR_INVALID_ARG, "rays not 16-byte aligned");
  if (rp->sqrt_paths > 32768 || rp->max_depth > 0xffffff)
    return set_err(RT_ERR_UNSUPPORTED, "sqrt_paths > 32768 or max_depth > 0xffffff");
  return RT_OK;
}

int rt_render_rays_device(rt_scene* sc, const rt_rays_params* rp, const rt_ray* rays,
                          uint64_t n_rays, float* rgb, void* stream_v, rt_stats* stats) {
  RT_TRY(check_rays_args(sc, rp, rays, n_rays, rgb));
  if (n_rays == 0) return RT_OK;
  // the batch as an image 8 pixels wide (render_device_rows): no camera geometry is read
  rt_camera cam{};
  cam.image_width = kWaveTile;
  cam.image_height = (int32_t)((n_rays + kWaveTile - 1) / kWaveTile);
  cam.sqrt_spp = rp->sqrt_paths;
  cam.samples_per_pixel = rp->sqrt_paths * rp->sqrt_paths;
  cam.recip_sqrt_spp = 1.0 / (double)rp->sqrt_paths;
  cam.max_depth = rp->max_depth;
  for (int k = 0; k < 3; ++k) cam.background[k] = rp->background[k];
  rt_render_opts opts{};
  opts.seed = rp->seed;
  opts.flags = rp->flags;
  opts.row_step = 1;
  opts.n_rows = cam.image_height;
  const RayJob rj{rays, n_rays, rp->stream_skip, rp->mode};
  return render_device_rows(sc, &cam, &opts, rgb, nullptr, nullptr, stream_v, stats, &rj);
}

int rt_render_rays(rt_scene* sc, const rt_rays_params* rp, const rt_ray* rays, uint64_t n_rays,
                   float* rgb, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  RT_TRY(check_rays_args(sc, rp, rays, n_rays, rgb));
  if (n_rays == 0) return RT_OK;
  const size_t in_bytes = (size_t)n_rays * sizeof(rt_ray), ob = (size_t)n_rays * 3 * sizeof(float);
  HIP_TRY(hipSetDevice(sc->device));
  uint8_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, ob);
  if (e == hipSuccess) e = hipMemcpy(d_in, rays, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && !(rp->flags & RT_FLAG_OVERWRITE))
    e = hipMemcpy(d_out, rgb, ob, hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? RT_OK
                           : set_err(RT_ERR_HIP, std::string("upload rays: ") + hipGetErrorString(e));
  rt_stats local;
  if (rc == RT_OK)
    rc = rt_render_rays_device(sc, rp, (const rt_ray*)d_in, n_rays, (float*)d_out, nullptr,
                               stats ? stats : &local);
  if (rc == RT_OK) {
    e = hipMemcpy(rgb, d_out, ob, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("download rgb: ") + hipGetErrorString(e));
  }
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (rc == RT_OK && stats)
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// Profiling builds (-DRT_PROF, not shipped): the ordered-BVH walk counters of the last render
// (rt_kernel.h obvh_walk). Other builds return zeros.
int rt_scene_prof_counters(rt_scene* sc, uint64_t* out, int n) {
  if (!sc || !out || n < 0) return set_err(RT_ERR_INVALID_ARG, "null argument");
  std::lock_guard<std::mutex> lock(sc->mu);
  HIP_TRY(hipSetDevice(sc->device));
  unsigned long long h[24] = {};
#ifdef RT_PROF
  if (sc->last_slot >= 0) {
    RenderSlot* sl = sc->slots[sc->last_slot].get();
    HIP_TRY(hipEventSynchronize(sl->done));
    HIP_TRY(hipMemcpy(h, sl->ops + 40, sizeof(h), hipMemcpyDeviceToHost));
  }
#endif
  for (int k = 0; k < n && k < 24; ++k) out[k] = h[k];
  return RT_OK;
}

int rt_scene_trace_ms(rt_scene* sc, float* ms_out, int max_n, int* n_out) {
  if (!sc || !ms_out || !n_out || max_n < 0) return set_err(RT_ERR_INVALID_ARG, "null argument");
  std::lock_guard<std::mutex> lock(sc->mu);
  HIP_TRY(hipSetDevice(sc->device));
  const uint64_t R = rt_scene::kTraceRing;
  const uint64_t first = sc->n_tev > R ? sc->n_tev - R : 0;
  // a render whose first launches fell out of the ring is incomplete: skip it
  const uint64_t skip_render = sc->n_tev > R ? sc->tev_render[first % R] : UINT64_MAX;
  std::vector<std::pair<uint64_t, double>> per;  // (render id, ms), oldest first
  for (uint64_t i = first; i < sc->n_tev; ++i) {
    const int k = (int)(i % R);
    const uint64_t id = sc->tev_render[k];
    if (id == skip_render) continue;
    HIP_TRY(hipEventSynchronize(sc->tev[k][1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, sc->tev[k][0], sc->tev[k][1]));
    if (per.empty() || per.back().first != id) per.push_back({id, 0.0});
    per.back().second += ms;
  }
  const int n = (int)std::min<size_t>((size_t)max_n, per.size());
  for (int i = 0; i < n; ++i) ms_out[i] = (float)per[per.size() - n + i].second;
  *n_out = n;
  return RT_OK;
}

int rt_render(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts, float* accum,
              rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!sc || !cam || !opts || !accum) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (opts->n_rows < 0 || cam->image_width <= 0) return set_err(RT_ERR_INVALID_ARG, "bad size");
  HIP_TRY(hipSetDevice(sc->device));
  size_t bytes = (size_t)opts->n_rows * cam->image_width * 3 * sizeof(float);
  if (bytes == 0) return RT_OK;
  float* d = nullptr;
  HIP_TRY(hipMalloc(&d, bytes));
  hipError_t e = (opts->flags & RT_FLAG_OVERWRITE) ? hipSuccess
                                                   : hipMemcpy(d, accum, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(RT_ERR_HIP, std::string("upload accum: ") + hipGetErrorString(e));
  }
  rt_stats local;
  int rc = rt_render_device(sc, cam, opts, d, nullptr, stats ? stats : &local);
  if (rc == RT_OK) {
    e = hipMemcpy(accum, d, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("download accum: ") + hipGetErrorString(e));
  }
  (void)hipFree(d);
  if (rc == RT_OK && stats)
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int rt_render_moments(rt_scene* sc, const rt_camera* cam, const rt_render_opts* opts, float* accum,
                      float* m2, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!sc || !cam || !opts || !accum || !m2) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (opts->n_rows < 0 || cam->image_width <= 0) return set_err(RT_ERR_INVALID_ARG, "bad size");
  HIP_TRY(hipSetDevice(sc->device));
  const size_t bytes = (size_t)opts->n_rows * cam->image_width * 3 * sizeof(float);
  if (bytes == 0) return RT_OK;
  // one allocation: the beauty sums, then the second moments
  uint8_t* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 2 * bytes));
  float* const d_acc = reinterpret_cast<float*>(d);
  float* const d_m2 = reinterpret_cast<float*>(d + bytes);
  hipError_t e = hipSuccess;
  if (!(opts->flags & RT_FLAG_OVERWRITE)) {
    e = hipMemcpy(d_acc, accum, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_m2, m2, bytes, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(RT_ERR_HIP, std::string("upload accum: ") + hipGetErrorString(e));
  }
  rt_stats local;
  int rc = rt_render_moments_device(sc, cam, opts, d_acc, d_m2, nullptr, stats ? stats : &local);
  if (rc == RT_OK) {
    e = hipMemcpy(accum, d_acc, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(m2, d_m2, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("download accum: ") + hipGetErrorString(e));
  }
  (void)hipFree(d);
  if (rc == RT_OK && stats)
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int rt_render_multi(const rt_scene_blob* blob, const rt_camera* cam, const rt_render_opts* opts,
                    const int* devices, int n_devices, float* accum, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!blob || !cam || !opts || !devices || !accum || n_devices <= 0)
    return set_err(RT_ERR_INVALID_ARG, "null argument or no devices");
  if (opts->n_rows < 0 || opts->row_step <= 0 || cam->image_width <= 0)
    return set_err(RT_ERR_INVALID_ARG, "bad row range");
  const int W = cam->image_width, G = n_devices;
  const size_t row_floats = (size_t)W * 3;
  int prev_device = -1;  // the caller's current device, restored on return
  (void)hipGetDevice(&prev_device);
  struct Part {
    rt_scene* sc = nullptr;
    hipStream_t stream = nullptr;
    float* dbuf = nullptr;
    std::vector<float> host;
    rt_render_opts o{};
  };
  std::vector<Part> parts(G);
  int rc = RT_OK;
  auto cleanup = [&]() {
    for (Part& p : parts) {
      if (p.sc) (void)hipSetDevice(p.sc->device);
      if (p.stream) (void)hipStreamSynchronize(p.stream);
      if (p.dbuf) (void)hipFree(p.dbuf);
      if (p.stream) (void)hipStreamDestroy(p.stream);
      rt_scene_destroy(p.sc);
    }
  };
  // device k renders rows k, k + G, ... of the call's rows (cyclic), each on its
  // own stream; all devices run concurrently, the host only waits at the end
  for (int k = 0; k < G && rc == RT_OK; ++k) {
    Part& p = parts[k];
    p.o = *opts;
    p.o.row_begin = opts->row_begin + k * opts->row_step;
    p.o.row_step = opts->row_step * G;
    p.o.n_rows = k < opts->n_rows ? (opts->n_rows - k + G - 1) / G : 0;
    p.o.device = devices[k];
    if (p.o.n_rows == 0) continue;
    rc = rt_scene_create(blob, devices[k], &p.sc);
    if (rc != RT_OK) break;
    hipError_t e = hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking);
    const size_t n = (size_t)p.o.n_rows * row_floats;
    if (e == hipSuccess) e = hipMalloc(&p.dbuf, n * sizeof(float));
    if (e == hipSuccess && !(opts->flags & RT_FLAG_OVERWRITE)) {
      p.host.resize(n);  // this device's rows of the caller's accumulator, accumulated on device
      for (int j = 0; j < p.o.n_rows; ++j)
        std::memcpy(&p.host[(size_t)j * row_floats],
                    accum + (size_t)(k + (size_t)j * G) * row_floats, row_floats * sizeof(float));
      e = hipMemcpyAsync(p.dbuf, p.host.data(), n * sizeof(float), hipMemcpyHostToDevice, p.stream);
    }
    if (e != hipSuccess) {
      rc = set_err(RT_ERR_HIP, std::string("rt_render_multi setup: ") + hipGetErrorString(e));
      break;
    }
    rc = rt_render_device(p.sc, cam, &p.o, p.dbuf, p.stream, nullptr);
  }
  for (int k = 0; k < G && rc == RT_OK; ++k) {
    Part& p = parts[k];
    if (!p.sc) continue;
    const size_t n = (size_t)p.o.n_rows * row_floats;
    p.host.resize(n);
    hipError_t e = hipSetDevice(p.sc->device);
    if (e == hipSuccess)
      e = hipMemcpyAsync(p.host.data(), p.dbuf, n * sizeof(float), hipMemcpyDeviceToHost, p.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p.stream);
    if (e != hipSuccess) {
      rc = set_err(RT_ERR_HIP, std::string("rt_render_multi gather: ") + hipGetErrorString(e));
      break;
    }
    for (int j = 0; j < p.o.n_rows; ++j)  // de-interleave into the caller's rows
      std::memcpy(accum + (size_t)(k + (size_t)j * G) * row_floats, &p.host[(size_t)j * row_floats],
                  row_floats * sizeof(float));
  }
  if (rc == RT_OK && stats) {
    std::memset(stats, 0, sizeof(*stats));
    const int S = cam->sqrt_spp, n_sj = opts->sj_count > 0 ? opts->sj_count : S;
    stats->samples = (uint64_t)opts->n_rows * W * (uint64_t)n_sj * S;
    stats->ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->ms_kernel = stats->ms_total;
    stats->launches = (uint32_t)G;
  }
  const std::string err = rc == RT_OK ? std::string() : g_err;
  cleanup();
  if (rc != RT_OK) g_err = err;
  if (prev_device >= 0) (void)hipSetDevice(prev_device);
  return rc;
}

// ---------------------------------------------------------------- persistent multi-GPU handle
// rt_multi_create uploads the scene to every listed device once; each device keeps its scene,
// its workspace, its stream, its compact row buffer and (after the first frame) its compiled
// scene-specialised kernel across rt_multi_render calls. A frame: every device renders its
// cyclic rows into its own buffer on its own stream, the buffers are copied peer-to-peer
// (hipMemcpyPeerAsync: xGMI between MI355X devices) into a staging area on the first device,
// and one kernel there de-interleaves the rows into the caller's frame.
struct rt_multi {
  struct Dev {
    rt_scene* sc = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    float* rows = nullptr;  // compact rows of this device's share
    size_t rows_bytes = 0;
  };
  std::vector<int> devices;
  std::vector<Dev> dev;
  float* stage = nullptr;  // on devices[0]: every device's rows, device after device
  size_t stage_bytes = 0;
  hipEvent_t start = nullptr;  // on devices[0]: the frame's start on the caller's stream
  // on devices[0]: the previous frame's end (its gather out of `stage`); a frame rendered on
  // another caller stream waits for it before reusing the staging area and the device rows
  hipEvent_t frame_done = nullptr;
  bool frame_recorded = false;
  uint64_t frames = 0, uploads = 0, stage_allocs = 0;
  std::mutex mu;
};

int rt_multi_create(const rt_scene_blob* blob, const int* devices, int n_devices,
                    rt_multi** out) {
  if (!blob || !devices || n_devices <= 0 || !out)
    return set_err(RT_ERR_INVALID_ARG, "null argument or no devices");
  *out = nullptr;
  int prev = -1;
  (void)hipGetDevice(&prev);
  rt_multi* m = new rt_multi();
  m->devices.assign(devices, devices + n_devices);
  m->dev.resize(n_devices);
  int rc = RT_OK;
  for (int k = 0; k < n_devices && rc == RT_OK; ++k) {
    rc = rt_scene_create(blob, devices[k], &m->dev[k].sc);
    if (rc != RT_OK) break;
    ++m->uploads;
    hipError_t e = hipStreamCreateWithFlags(&m->dev[k].stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->dev[k].done, hipEventDisableTiming);
    // direct peer copies into the first device (already enabled / same device: not an error)
    if (e == hipSuccess && devices[k] != devices[0]) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[k], devices[0]) == hipSuccess && can) {
        const hipError_t pe = hipDeviceEnablePeerAccess(devices[0], 0);
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) e = pe;
        (void)hipGetLastError();
      }
    }
    if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("rt_multi_create: ") + hipGetErrorString(e));
  }
  if (rc == RT_OK) {
    hipError_t e = hipSetDevice(devices[0]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->start, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->frame_done, hipEventDisableTiming);
    if (e != hipSuccess) rc = set_err(RT_ERR_HIP, std::string("rt_multi_create: ") + hipGetErrorString(e));
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  if (rc != RT_OK) {
    const std::string err = g_err;
    rt_multi_destroy(m);
    g_err = err;
    return rc;
  }
  *out = m;
  return RT_OK;
}

void rt_multi_destroy(rt_multi* m) {
  if (!m) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (size_t k = 0; k < m->dev.size(); ++k) {
    rt_multi::Dev& d = m->dev[k];
    (void)hipSetDevice(m->devices[k]);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    if (d.rows) (void)hipFree(d.rows);
    if (d.done) (void)hipEventDestroy(d.done);
    if (d.stream) (void)hipStreamDestroy(d.stream);
    rt_scene_destroy(d.sc);
  }
  (void)hipSetDevice(m->devices[0]);
  if (m->stage) (void)hipFree(m->stage);
  if (m->start) (void)hipEventDestroy(m->start);
  if (m->frame_done) (void)hipEventDestroy(m->frame_done);
  delete m;
  if (prev >= 0) (void)hipSetDevice(prev);
}

int rt_multi_render(rt_multi* m, const rt_camera* cam, const rt_render_opts* opts,
                    float* accum_rgb_device0, void* hip_stream, rt_stats* stats) {
  auto t0 = std::chrono::steady_clock::now();
  if (!m || !cam || !opts || !accum_rgb_device0)
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (opts->n_rows < 0 || opts->row_step <= 0 || cam->image_width <= 0)
    return set_err(RT_ERR_INVALID_ARG, "bad row range");
  if (opts->n_rows > 0 &&
      (int64_t)opts->row_begin + (int64_t)(opts->n_rows - 1) * opts->row_step >= cam->image_height)
    return set_err(RT_ERR_INVALID_ARG, "row range outside the image");
  std::lock_guard<std::mutex> lock(m->mu);
  int prev = -1;
  (void)hipGetDevice(&prev);
  const int G = (int)m->devices.size(), d0 = m->devices[0];
  const size_t row_floats = (size_t)cam->image_width * 3;
  const size_t frame_bytes = (size_t)opts->n_rows * row_floats * sizeof(float);
  hipStream_t out_stream = (hipStream_t)hip_stream;
  auto fail = [&](hipError_t e, const char* what) {
    if (prev >= 0) (void)hipSetDevice(prev);
    return set_err(RT_ERR_HIP, std::string("rt_multi_render ") + what + ": " + hipGetErrorString(e));
  };
  if (opts->n_rows == 0) return RT_OK;
  hipError_t e = hipSetDevice(d0);
  if (e == hipSuccess && m->frame_recorded) e = hipStreamWaitEvent(out_stream, m->frame_done, 0);
  if (e == hipSuccess && m->stage_bytes < frame_bytes) {
    // the previous frame's gather reads the staging buffer: it must have finished (a failed
    // wait leaves the buffer in use, so it is reported, not freed)
    if (m->frame_recorded) e = hipEventSynchronize(m->frame_done);
    if (e != hipSuccess) return fail(e, "staging buffer (waiting for the previous frame)");
    if (m->stage) (void)hipFree(m->stage);
    m->stage = nullptr;
    m->stage_bytes = 0;
    e = hipMalloc(&m->stage, frame_bytes);
    if (e == hipSuccess) m->stage_bytes = frame_bytes, ++m->stage_allocs;
  }
  if (e != hipSuccess) return fail(e, "staging buffer");
  const bool accumulate = !(opts->flags & RT_FLAG_OVERWRITE);
  const int gx = (int)std::min<size_t>(64, (row_floats + 255) / 256);
  const int gy = std::min(opts->n_rows, 65535);  // rt_deinterleave loops over the rest
  if (accumulate) {  // the caller's rows to the staging area: each device accumulates its own
    hipLaunchKernelGGL(rt_deinterleave, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0,
                       out_stream, m->stage, accum_rgb_device0, (int)row_floats, opts->n_rows, G, 0);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(e, "scatter");
  }
  // the caller's stream on the first device orders the frame: every device starts after it
  e = hipEventRecord(m->start, out_stream);
  if (e != hipSuccess) return fail(e, "start event");
  std::vector<char> used(G, 0);
  uint64_t samples = 0;
  size_t row0 = 0;
  int rc = RT_OK;
  for (int k = 0; k < G && rc == RT_OK; ++k) {
    rt_multi::Dev& d = m->dev[k];
    rt_render_opts o = *opts;
    o.row_begin = opts->row_begin + k * opts->row_step;
    o.row_step = opts->row_step * G;
    o.n_rows = k < opts->n_rows ? (opts->n_rows - k + G - 1) / G : 0;
    o.device = m->devices[k];
    // compact rows: overwritten, or the caller's rows (scattered above) accumulated into
    if (o.n_rows == 0) continue;
    const size_t bytes = (size_t)o.n_rows * row_floats * sizeof(float);
    e = hipSetDevice(m->devices[k]);
    if (e == hipSuccess && d.rows_bytes < bytes) {
      if (d.rows) (void)hipFree(d.rows);
      d.rows = nullptr;
      d.rows_bytes = 0;
      e = hipMalloc(&d.rows, bytes);
      if (e == hipSuccess) d.rows_bytes = bytes;
    }
    if (e == hipSuccess) e = hipStreamWaitEvent(d.stream, m->start, 0);
    if (e == hipSuccess && accumulate)
      e = hipMemcpyPeerAsync(d.rows, m->devices[k], m->stage + row0 * row_floats, d0, bytes, d.stream);
    if (e != hipSuccess) {
      rc = fail(e, "device setup");
      break;
    }
    rc = rt_render_device(d.sc, cam, &o, d.rows, d.stream, nullptr);
    if (rc != RT_OK) break;
    // the rows travel to the first device's staging area (xGMI peer copy, or a local copy)
    e = hipMemcpyPeerAsync(m->stage + row0 * row_floats, d0, d.rows, m->devices[k], bytes, d.stream);
    if (e == hipSuccess) e = hipEventRecord(d.done, d.stream);
    if (e != hipSuccess) {
      rc = fail(e, "peer copy");
      break;
    }
    used[k] = 1;
    samples += (uint64_t)o.n_rows * cam->image_width *
               (uint64_t)(opts->sj_count > 0 ? opts->sj_count : cam->sqrt_spp) * cam->sqrt_spp;
    row0 += (size_t)o.n_rows;
  }
  if (rc == RT_OK) {
    e = hipSetDevice(d0);
    for (int k = 0; k < G && e == hipSuccess; ++k)
      if (used[k]) e = hipStreamWaitEvent(out_stream, m->dev[k].done, 0);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(rt_deinterleave, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0,
                         out_stream, m->stage, accum_rgb_device0, (int)row_floats, opts->n_rows, G, 1);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(m->frame_done, out_stream);
    if (e == hipSuccess) m->frame_recorded = true;
    if (e == hipSuccess && stats) e = hipStreamSynchronize(out_stream);
    if (e != hipSuccess) rc = fail(e, "gather");
  }
  if (rc == RT_OK) {
    ++m->frames;
    if (stats) {
      std::memset(stats, 0, sizeof(*stats));
      stats->samples = samples;
      stats->launches = (uint32_t)G;
      stats->ms_total =
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      stats->ms_kernel = stats->ms_total;
    }
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  return rc;
}

int rt_multi_info(rt_multi* m, uint64_t* out, int n) {
  if (!m || !out || n < 0) return set_err(RT_ERR_INVALID_ARG, "null argument");
  std::lock_guard<std::mutex> lock(m->mu);
  const uint64_t v[4] = {m->frames, m->uploads, m->stage_allocs, (uint64_t)m->devices.size()};
  for (int k = 0; k < n && k < 4; ++k) out[k] = v[k];
  return RT_OK;
}

int rt_render_blob(const rt_scene_blob* blob, const rt_camera* cam, const rt_render_opts* opts,
                   float* accum, rt_stats* stats) {
  if (!opts) return set_err(RT_ERR_INVALID_ARG, "null opts");
  rt_scene* sc = nullptr;
  int rc = rt_scene_create(blob, opts->device, &sc);
  if (rc != RT_OK) return rc;
  rc = rt_render(sc, cam, opts, accum, stats);
  rt_scene_destroy(sc);
  return rc;
}

}  // extern "C"
