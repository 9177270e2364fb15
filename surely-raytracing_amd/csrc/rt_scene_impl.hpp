// rt_scene_impl.hpp — the host-side scene and render-slot types shared by the translation units of
// librtmi355x.so that launch kernels on a scene, and the steps every such launch takes (argument
// checks, LDS plan, TraceParams fill, occupancy query, completion): rt_device.hip (the path kernels
// and the C ABI's scene functions, where everything declared here is defined), rt_tiles.hip and
// rt_rays.hip (the tile-list and ray instances of the path kernels), rt_aov.hip (the first-hit AOV
// pass) and rt_query.hip (the ray queries). The two passes on the interpreter's plan string these
// steps together in rt_pass.hpp. The stage handles' translation units (rt_denoise.hip,
// rt_temporal.hip, rt_adaptive.hip, rt_output.hip; rt_raygen.hip, whose driver also reads a
// scene's device ordinal) know nothing of scenes and take only set_err, HIP_TRY and RT_TRY from
// here, through rt_stage.hpp, which holds the handle lifecycle and the host-buffer staging of
// every pass. Internal: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rt_mi355x.h"
#include "rt_jit.hpp"
#include "rt_layout.h"

#define RTS_HIDDEN __attribute__((visibility("hidden")))

namespace rtk {
struct TraceParams;  // rt_kernel.h
}

namespace rts {

// status code + the thread's rt_last_error() message
RTS_HIDDEN int set_err(int code, const std::string& m);

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return rts::set_err(RT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

// a step of a call that returns an rt status: leave with it unless RT_OK
#define RT_TRY(expr)                    \
  do {                                  \
    const int rc_ = (expr);             \
    if (rc_ != RT_OK) return rc_;       \
  } while (0)

// The path kernel's LDS for one render (rt_trace's prologue stages these regions, in this order,
// from byte 0 of the dynamic LDS): the small tables or the Perlin tables (stage), then either the
// compact ordered BVHs and the LDS walk's per-lane stacks (cbvh_walk_t: lane l's slot k at
// stack_off + 4 (l + k block), header cbvh_stack = 4 x the deepest tree's depth bytes per lane),
// or as much of the reference BVH region as fits. One function for the render, for the AOV pass
// (whose kernel runs the same walker on the same plan) and for the host check of the plan
// (rt_scene_lds_check), so they cannot drift apart.
struct LdsPlan {
  int block = 0;
  size_t static_lds = 0;  // the kernel's static LDS (per-lane f64 sums, ...), an upper bound
  uint32_t stage_scene = 0, stage_bytes = 0, n_perlin_lds = 0;
  uint32_t cbvh_lds_off = ~0u, stack_lds_off = 0, cbvh_bytes = 0;
  size_t cbvh_lds = 0;  // bytes of the trees and stacks
  uint32_t bvh_lds_words = 0, bvh_lds_off = 0;
  uint32_t row_lds_off = ~0u;  // BVH kernels: the row items' row totals (~0u: no row items)
  size_t lds_bytes = 0;  // dynamic LDS of the launch
};
RTS_HIDDEN LdsPlan plan_lds(const rtl_scene_header& hdr, uint32_t o_perl, uint32_t flags,
                            bool want_jit, size_t lds_module_max);

}  // namespace rts

// The per-render state of a scene: the f64 workspace, the pool-queue word and op counters, the
// stats events and a completion event. A render takes a slot that no render still uses (its done
// event has fired) or one whose last render went to the same stream (stream order then protects
// it); otherwise a new slot is made (up to kMaxSlots), so renders of one scene on different
// streams or host threads run concurrently on their own queue words and workspaces.
struct RenderSlot {
  uint8_t* work = nullptr;  // row totals / segment partials / tail samples + f64 running sums
  size_t work_bytes = 0;
  uint8_t* work2 = nullptr;  // moments renders in several chunks: the f64 running sums of R^2
  size_t work2_bytes = 0;
  // tile-list renders: the list on the device and the host copy it is uploaded from; both are
  // rewritten, freed or regrown only after `done` (tiles_busy: the last render here used them)
  uint32_t* tiles = nullptr;
  size_t tiles_cap = 0;  // entries
  std::vector<uint32_t> tiles_host;
  bool tiles_busy = false;
  unsigned long long* ops = nullptr;  // 32 op counters, the pool-queue word (32), profiling (40..)
  unsigned int* queue = nullptr;
  hipEvent_t done = nullptr;  // recorded after the render's last kernel
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // rt_stats::ms_kernel
  hipStream_t last_stream = nullptr;
  bool recorded = false;  // `done` has been recorded at least once
  bool held = false;      // a render call is between acquire and release
};

struct rt_scene {
  int device = 0;
  rtl_scene_header hdr{};
  uint8_t* dev = nullptr;  // one allocation for all tables
  uint64_t dev_bytes = 0;
  const uint32_t *nodes = nullptr, *mats = nullptr, *texs = nullptr, *lights = nullptr,
                 *light_offs = nullptr;
  const uint8_t *perlin = nullptr, *texels = nullptr;
  uint32_t o_mats = 0, o_texs = 0, o_lights = 0, o_loffs = 0, o_perl = 0;  // byte offsets in dev
  int sphere_light0 = -1;  // first SPHERE light record (TraceParams::sphere_light0)
  // the table behind rt_hit.prim (rtf::FlatScene prim_word / prim_id), kept from the flattener;
  // prim_dev: its device copy, n words then n prims, uploaded by the scene's first ray query
  // (rt_query.hip, under mu) and freed by rt_scene_destroy
  std::vector<uint32_t> prim_word, prim_id;
  uint32_t* prim_dev = nullptr;
  static constexpr int kMaxSlots = 8;
  std::vector<std::unique_ptr<RenderSlot>> slots;  // grown on demand (RenderSlot)
  int last_slot = -1;                              // the slot of the latest render
  std::condition_variable slot_cv;                 // a held slot was released
  int n_cu = 0;                 // compute units of the device
  size_t mem_total = (size_t)8 << 30;  // device memory (hipMemGetInfo at creation)
  size_t lds_module_max = 64u << 10;  // LDS a module (hiprtc) launch may take (device limit)
  // per kernel launched on the scene, keyed by the kernel itself (the ahead-of-time kernel's
  // address or the module's function handle): blocks resident per CU at this dynamic LDS size
  // (rts::resident_blocks)
  struct Resident {
    const void* kernel;
    size_t lds;
    int blocks;
  };
  std::vector<Resident> resident;
  // scene-specialised product kernel (rt_jit.cpp): the generated world walker, compiled on the
  // first product render. jit_state: 0 = not compiled yet, 1 = compiled, -1 = scene not
  // generated (jit_msg says why), -2 = compile failed (jit_msg = log; the interpreter runs)
  std::string jit_walker, jit_msg;
  int jit_state = -1;
  rtj::Kernel jit_k[3];  // [launch kind: plain, tile list, rays] of the scene's one variant (rt_variant.h)
  // rt_trace launch timing: one event pair per launch, ring of kTraceRing, tagged by render id
  static constexpr int kTraceRing = 4 * RT_TRACE_HISTORY;
  hipEvent_t tev[kTraceRing][2] = {};
  uint64_t tev_render[kTraceRing] = {};
  uint64_t n_tev = 0, n_render = 0;
  std::mutex mu;
};

namespace rts {

// A slot for a render on `stream` (RenderSlot), with sc->mu held through `lock`: a free one (its
// last render has finished, or went to the same stream handle), else a new one, else wait for a
// release. A reused slot's `done` event is always waited for on `stream` (hipStreamWaitEvent):
// equal handles are not the same stream everywhere (hipStreamPerThread, the per-thread default
// stream), so stream order alone cannot be trusted; on the same stream the wait costs nothing.
RTS_HIDDEN int acquire_slot(rt_scene* sc, std::unique_lock<std::mutex>& lock, hipStream_t stream,
                            RenderSlot** out);

// Releases a held slot on every exit path of a render call. Once the call has enqueued work on
// `stream` (enqueued), a call that fails half way still records the slot's `done` event after
// that work: the next render to take the slot then waits for the kernels that may still use its
// workspace and queue word, instead of for the previous render's event.
struct SlotHold {
  rt_scene* sc;
  std::unique_lock<std::mutex>& lock;
  RenderSlot* sl = nullptr;
  hipStream_t stream = nullptr;
  bool enqueued = false;   // work of this call is on `stream`
  bool finished = false;   // `done` was recorded after all of it
  ~SlotHold() {
    if (!sl) return;
    if (!lock.owns_lock()) lock.lock();
    if (enqueued && !finished) {
      if (hipEventRecord(sl->done, stream) == hipSuccess) {
        sl->recorded = true;
        sl->last_stream = stream;
      } else {
        (void)hipStreamSynchronize(stream);  // no event: drain the stream before the slot is reused
      }
    }
    sl->held = false;
    sc->slot_cv.notify_all();
  }
};

// The tile-list variant (trace_body's TILES) of the ahead-of-time product kernel of variant `v`
// (rt_tiles.hip: its 18 instances compile beside rt_device.hip's); nullptr: RT_VARIANTS has no such row.
typedef void (*kern_t)(rtk::TraceParams);
RTS_HIDDEN kern_t tile_trace_kernel(const rtv::Variant& v);
// The ray variant (trace_body's kLaunchRays; rt_rays.hip, 18 more instances in their own object)
RTS_HIDDEN kern_t ray_trace_kernel(const rtv::Variant& v);

// What every pass that launches on a scene checks of its camera and row range, with the status
// codes and rt_last_error() texts; *sj0 / *n_sj: the call's stratum rows sj0 + k * sj_step,
// k < n_sj (sj_step: 1, or a tile-list render's stride). path_depth: cam->max_depth is checked
// (the AOV pass does not read it: AOVs exist at max_depth 0 too).
RTS_HIDDEN int check_render_args(const rt_camera* cam, const rt_render_opts* opts, bool path_depth,
                                 int sj_step, int* sj0, int* n_sj);

// TraceParams of a launch on `sc` with plan LP: the scene's tables and light list, the plan's LDS
// regions, the camera, the call's rows, seed and flags. The caller adds what only it knows: the
// slot's queue and op counters, the chunk's stratum rows and pairs, the outputs.
RTS_HIDDEN void fill_trace_params(rtk::TraceParams* P, const rt_scene* sc, const rt_camera* cam,
                                  const rt_render_opts* opts, const LdsPlan& LP);

// Blocks of `kernel` (module != nullptr: that module function instead) resident per CU, asked once
// per kernel and LDS size (rt_scene::resident). A dispatch the hardware cannot place aborts the
// whole queue, so every launch asks first; `what` names the kernel in the error text.
RTS_HIDDEN int resident_blocks(rt_scene* sc, const void* kernel, hipFunction_t module, int block,
                               size_t lds_bytes, const char* what, int* out);

// The end of a render call that enqueued its work on `stream`: the slot's events, and with `stats`
// the wait for the stream and the read-back. counts: samples, out_bytes and launches as the caller
// counted them; read_ops: the launch filled the slot's op counters; t0: the call's start.
RTS_HIDDEN int complete_render(SlotHold& hold, hipStream_t stream, rt_stats* stats,
                               const rt_stats& counts, bool read_ops,
                               std::chrono::steady_clock::time_point t0);

// Lane item keys hold the call's row index in 15 bits (render_device_rows): taller row ranges
// are rendered as consecutive sub-calls of kRowsPerCall rows into the matching rows of accum.
// The RNG is keyed by the global pixel and sample, so the image does not depend on the split.
constexpr int kRowsPerCall = 32760;

}  // namespace rts
