// rt_stage.hpp — what the stage handles (rt_denoiser, rt_temporal, rt_adaptive, rt_output_stage,
// rt_raygen) share, and the host-buffer path of every pass: the handle's fields, creation and
// destruction, the workspace growth, the run guard that orders a handle's calls, the stats
// read-back (rts::Stage, rts::Run), one device allocation made of parts with its uploads and
// downloads (rts::Staging), and the calls' clock (rts::ms_since). Host only; DESIGN.md §4.2c.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "rt_mi355x.h"
#include "rt_scene_impl.hpp"  // set_err, HIP_TRY, RT_TRY

namespace rts {

typedef std::chrono::steady_clock::time_point time_point;
inline double ms_since(time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// One workspace and one ordering event per handle. `mu` serialises the handle's calls; every
// call's stream waits for `done` of the call before it (whatever stream that went to), so the
// workspace is never shared by two calls in flight: the previous call may still be using it on
// another stream, even when it failed half way (Run).
struct Stage {
  int device = 0;
  uint8_t* work = nullptr;
  size_t work_bytes = 0;
  hipEvent_t done = nullptr;                // after the last work of the latest call
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // rt_stats::ms_kernel (timed handles)
  bool recorded = false;                    // `done` has been recorded at least once
  std::mutex mu;

  // At least `bytes` of workspace (mu held, the device set). Growth waits for the previous call,
  // which may still be using the old workspace; a failed allocation leaves none.
  int reserve(size_t bytes) {
    if (bytes <= work_bytes) return RT_OK;
    if (recorded) HIP_TRY(hipEventSynchronize(done));
    if (work) HIP_TRY(hipFree(work));
    work = nullptr;
    work_bytes = 0;
    HIP_TRY(hipMalloc((void**)&work, bytes));
    work_bytes = bytes;
    return RT_OK;
  }

  // The end of a timed call whose Run has ended: waits for `stream`, then fills *stats with the
  // device time between ev0 and ev1, the caller's counts and the wall time since t0.
  int finish_stats(hipStream_t stream, rt_stats* stats, uint64_t samples, uint64_t out_bytes,
                   uint32_t launches, time_point t0) {
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    stats->ms_kernel = ms;
    stats->samples = samples;
    stats->out_bytes = out_bytes;
    stats->launches = launches;
    stats->ms_total = ms_since(t0);
    return RT_OK;
  }
};

// Waits for the handle's last call, then frees what the Stage owns and the handle itself.
template <class H>
void stage_destroy(H* h) {
  if (!h) return;
  {
    std::lock_guard<std::mutex> lock(h->mu);
    (void)hipSetDevice(h->device);
    if (h->recorded) (void)hipEventSynchronize(h->done);
    if (h->work) (void)hipFree(h->work);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
  }
  delete h;
}

// The handle of type H (a Stage) on `device`; timed: with the two stats events.
template <class H>
int stage_create(int device, bool timed, H** out) {
  if (!out) return set_err(RT_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_err(RT_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return set_err(RT_ERR_INVALID_ARG, "bad device ordinal");
  HIP_TRY(hipSetDevice(device));
  H* h = new H;
  h->device = device;
  hipError_t e = hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
  if (e == hipSuccess && timed) e = hipEventCreate(&h->ev0);
  if (e == hipSuccess && timed) e = hipEventCreate(&h->ev1);
  if (e != hipSuccess) {
    stage_destroy(h);
    return set_err(RT_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
  }
  *out = h;
  return RT_OK;
}

// One call's use of the workspace on `stream` (mu held). begin() makes the stream wait for the
// handle's previous call; the destructor records `done` after whatever the call has enqueued, on
// every exit path, so that the next call still waits for the kernels of a call that failed half
// way. A caller that must read the stream's results ends the Run's scope first.
struct Run {
  Stage& s;
  hipStream_t stream;
  Run(Stage& stage, hipStream_t st) : s(stage), stream(st) {}
  Run(const Run&) = delete;
  // timed: ev0 goes into the stream after the wait (the caller records ev1 after its kernels)
  int begin(bool timed) {
    if (s.recorded) HIP_TRY(hipStreamWaitEvent(stream, s.done, 0));
    if (timed) HIP_TRY(hipEventRecord(s.ev0, stream));
    return RT_OK;
  }
  ~Run() {
    if (hipEventRecord(s.done, stream) == hipSuccess)
      s.recorded = true;
    else
      (void)hipStreamSynchronize(stream);  // no event: drain the stream before the next call
  }
};

// The host-buffer entry points' device memory: one allocation made of parts, each 256-byte
// aligned (rt_ray and rt_hit ask for 16), freed on every exit path. add() the parts, alloc()
// once, then upload / ptr / download by the part's id. An optional buffer the caller did not give
// is no part: its id is `none`, its pointer null, its copies are skipped.
// rt_device.hip's three wrappers (rt_render, rt_render_moments, rt_render_rays) still stage by
// hand: that file is hashed into the committed PMC profiles (roofline.KERNEL_SOURCES), so they
// move here with the change that next collects those profiles again.
class Staging {
 public:
  static constexpr int none = -1;
  Staging() = default;
  Staging(const Staging&) = delete;
  ~Staging() {
    if (base_) (void)hipFree(base_);
  }
  int add(size_t bytes) {
    parts_.push_back(Part{total_, bytes});
    total_ += (bytes + 255) & ~(size_t)255;
    return (int)parts_.size() - 1;
  }
  int add_if(bool wanted, size_t bytes) { return wanted ? add(bytes) : none; }
  // on `device`; parts of no bytes still get a pointer that is not null
  int alloc(int device) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc((void**)&base_, total_ ? total_ : 256));
    return RT_OK;
  }
  template <class T>
  T* ptr(int part) const {
    return part == none ? nullptr : reinterpret_cast<T*>(base_ + parts_[part].off);
  }
  int upload(int part, const void* host) { return copy(part, const_cast<void*>(host), true); }
  int download(int part, void* host) { return copy(part, host, false); }

 private:
  struct Part {
    size_t off, bytes;
  };
  int copy(int part, void* host, bool up) {
    if (part == none || parts_[part].bytes == 0) return RT_OK;
    uint8_t* dev = base_ + parts_[part].off;
    const hipError_t e = up ? hipMemcpy(dev, host, parts_[part].bytes, hipMemcpyHostToDevice)
                            : hipMemcpy(host, dev, parts_[part].bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) return RT_OK;
    return set_err(RT_ERR_HIP, std::string(up ? "upload: " : "download: ") + hipGetErrorString(e));
  }
  uint8_t* base_ = nullptr;
  size_t total_ = 0;
  std::vector<Part> parts_;
};

}  // namespace rts
