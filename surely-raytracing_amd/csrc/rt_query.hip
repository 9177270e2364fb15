// rt_query.hip — ray queries of include/rt_mi355x.h: the rt_query kernels (body in rt_query.h),
// rt_query_rays / rt_query_rays_device and the host-only rt_scene_prim_map. A sibling of
// rt_aov.hip: its own translation unit beside rt_device.hip, the scene and render-slot types from
// rt_scene_impl.hpp, the AOV pass's LDS plan, workgroup and slot path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "rt_mi355x.h"
#include "rt_query.h"
#include "rt_flatten.hpp"
#include "rt_pass.hpp"
#include "rt_stage.hpp"

using namespace rtk;
using namespace rts;

static_assert(sizeof(rt_ray) == 80 && sizeof(rt_hit) == 80 && sizeof(rt_query_params) == 16,
              "rt_ray, rt_hit, rt_query_params: no padding");

namespace {

// The AOV pass's five instances (rt_aov.hip, RT_RETURN_INTERP_KERNEL); every feature bit set.
// TraceParams stays the first argument, as in every kernel on this plan; the query's walker is
// instantiated with PK and reads nothing through kparams() (rt_query.h). ANY: the five any-hit
// instances, the same plan, workgroup and prologue.
template <bool BVH, bool STAGED, int VN, bool ANY = false>
__global__ __launch_bounds__(BlockOf<BVH>::value) void rt_query(
    TraceParams P, const uint4* __restrict__ rays, void* __restrict__ out, uint32_t n_rays,
    uint32_t mode, const uint32_t* __restrict__ prim_tab, uint32_t n_prim) {
  query_body<BVH, STAGED, VN, ANY>(P, rays, out, n_rays, mode, prim_tab, n_prim);
}

typedef void (*query_kern_t)(TraceParams, const uint4*, void*, uint32_t, uint32_t, const uint32_t*,
                             uint32_t);
template <bool ANY>
query_kern_t query_kernel_of(const rtv::Variant& v) {
  RT_RETURN_INTERP_KERNEL(v, rt_query, ANY);
}
query_kern_t query_kernel(const rtv::Variant& v, uint32_t mode) {
  return (mode & RT_QUERY_ANY_HIT) ? query_kernel_of<true>(v) : query_kernel_of<false>(v);
}

// made before the scene is read and before any HIP call
int check_query_args(const rt_scene* sc, const rt_query_params* qp, const void* rays,
                     uint64_t n_rays, const void* out) {
  if (!sc || !qp || !rays || !out) return set_err(RT_ERR_INVALID_ARG, "null argument");
  if (n_rays >= (1ull << 31)) return set_err(RT_ERR_INVALID_ARG, "n_rays >= 2^31");
  if (qp->flags & ~RT_FLAG_REFERENCE_BVH)
    return set_err(RT_ERR_INVALID_ARG, "ray queries take RT_FLAG_REFERENCE_BVH only");
  if (qp->mode & ~(RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT))
    return set_err(RT_ERR_INVALID_ARG, "unknown query mode bits");
  if ((qp->mode & RT_QUERY_ANY_HIT) && !(qp->mode & RT_QUERY_OCCLUSION))
    return set_err(RT_ERR_INVALID_ARG, "RT_QUERY_ANY_HIT needs RT_QUERY_OCCLUSION");
  if ((uintptr_t)rays % 16u) return set_err(RT_ERR_INVALID_ARG, "rays not 16-byte aligned");
  if (!(qp->mode & RT_QUERY_OCCLUSION) && (uintptr_t)out % 16u)
    return set_err(RT_ERR_INVALID_ARG, "out not 16-byte aligned");
  return RT_OK;
}

uint64_t out_bytes_of(const rt_query_params* qp, uint64_t n_rays) {
  return (qp->mode & RT_QUERY_OCCLUSION) ? n_rays : n_rays * sizeof(rt_hit);
}

// the scene's first query (sc->mu held, the device set): the prim table, n words then n prims
int upload_prim_table(rt_scene* sc) {
  std::vector<uint32_t> tab(sc->prim_word);
  tab.insert(tab.end(), sc->prim_id.begin(), sc->prim_id.end());
  tab.resize(tab.size() + 4, 0u);
  uint32_t* d = nullptr;
  HIP_TRY(hipMalloc(&d, tab.size() * 4));
  const hipError_t e = hipMemcpy(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(RT_ERR_HIP, std::string("upload prim table: ") + hipGetErrorString(e));
  }
  sc->prim_dev = d;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_query_rays_device(rt_scene* sc, const rt_query_params* qp, const rt_ray* rays,
                         uint64_t n_rays, void* out, void* stream_v, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  RT_TRY(check_query_args(sc, qp, rays, n_rays, out));
  if (n_rays == 0) return RT_OK;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  std::unique_lock<std::mutex> lock(sc->mu);
  hipStream_t stream = (hipStream_t)stream_v;
  // no camera: the kernel reads the tables, the plan's LDS regions, flags and seed
  rt_camera cam{};
  cam.image_width = cam.image_height = cam.sqrt_spp = cam.samples_per_pixel = 1;
  rt_render_opts opts{};
  opts.seed = qp->seed;
  opts.flags = qp->flags;
  opts.row_step = 1;
  SlotHold hold{sc, lock};
  InterpPass ip;
  RT_TRY(begin_interp_pass(sc, hold, stream, &cam, &opts, &ip));
  const LdsPlan& LP = ip.LP;
  if (!sc->prim_dev) RT_TRY(upload_prim_table(sc));
  const query_kern_t kern = query_kernel(ip.v, qp->mode);
  RT_TRY(arm_interp_launch(sc, hold, stream, (const void*)kern, LP, "query kernel",
                           stats != nullptr));
  const unsigned blocks = (unsigned)((n_rays + (uint64_t)LP.block - 1) / (uint64_t)LP.block);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(LP.block), LP.lds_bytes, stream, ip.P,
                     reinterpret_cast<const uint4*>(rays), out, (uint32_t)n_rays, qp->mode,
                     (const uint32_t*)sc->prim_dev, (uint32_t)sc->prim_word.size());
  HIP_TRY(hipGetLastError());
  rt_stats counts{};
  counts.samples = n_rays;
  counts.out_bytes = out_bytes_of(qp, n_rays);
  counts.launches = 1;
  return complete_render(hold, stream, stats, counts, false, t0);
}

int rt_query_rays(rt_scene* sc, const rt_query_params* qp, const rt_ray* rays, uint64_t n_rays,
                  void* out, rt_stats* stats) {
  const time_point t0 = std::chrono::steady_clock::now();
  RT_TRY(check_query_args(sc, qp, rays, n_rays, out));
  if (n_rays == 0) return RT_OK;
  Staging st;
  const int i_rays = st.add((size_t)n_rays * sizeof(rt_ray));
  const int i_out = st.add((size_t)out_bytes_of(qp, n_rays));
  RT_TRY(st.alloc(sc->device));
  RT_TRY(st.upload(i_rays, rays));
  rt_stats local;
  RT_TRY(rt_query_rays_device(sc, qp, st.ptr<const rt_ray>(i_rays), n_rays, st.ptr<void>(i_out),
                              nullptr, stats ? stats : &local));
  RT_TRY(st.download(i_out, out));
  if (stats) stats->ms_total = ms_since(t0);
  return RT_OK;
}

int rt_scene_prim_map(const rt_scene_blob* blob, uint32_t* node_word, uint32_t* prim, uint32_t cap,
                      uint32_t* n_out) {
  if (!blob || !n_out || (cap > 0 && (!node_word || !prim)))
    return set_err(RT_ERR_INVALID_ARG, "null argument");
  rtf::FlatScene F;
  std::string err;
  const int rc = rtf::flatten(blob, &F, &err);
  if (rc != RT_OK) return set_err(rc, err);
  const size_t n = F.prim_word.size(), m = std::min<size_t>(n, cap);
  if (m) {
    std::memcpy(node_word, F.prim_word.data(), m * 4);
    std::memcpy(prim, F.prim_id.data(), m * 4);
  }
  *n_out = (uint32_t)n;
  return RT_OK;
}

}  // extern "C"
