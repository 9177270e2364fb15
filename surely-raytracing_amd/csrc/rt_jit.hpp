// rt_jit.hpp — scene-specialised path kernels: the world walker generated from the flattened
// scene and compiled at run time by hiprtc (rt_jit.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rt_flatten.hpp"
#include "rt_variant.h"

namespace rtj {

// Source of `struct TravGen` (the world query of ray_color, render.rs:264-267) for this scene:
// the wave-uniform node sequence that the interpreter (rt_kernel.h traverse<UNI>) walks at run
// time, unrolled, with every record's constants as literals; a BVH subtree record becomes a call
// of the interpreter's per-lane walker. Empty when the scene has records the generator does not
// emit or is too large; *why says which.
std::string generate(const rtf::FlatScene& F, std::string* why);

// The generated walker runs in the path kernel (rt_kernel.h trace_body) with the scene's variant
// (rt_variant.h choose_variant): the template arguments and launch bounds of the ahead-of-time
// interpreter kernel the scene would otherwise launch. generate() refuses scenes with nested
// volumes, so a variant's vn never reaches the source. launch: trace_body's LK, 0 the plain kernel, 1 the
// tile-list variant (rt_render_tiles_device), 2 the ray variant (rt_render_rays_device).

// Kernel for (generated walker, variant, launch kind) on `device`, compiled on first use and cached for
// the process. Returns 0 or a negative rt status with *log filled.
struct Kernel {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  // code-object resources as the runtime reports them (hipFuncGetAttribute), checked against
  // the launch before every first use (rt_device.hip)
  int regs = 0, max_threads = 0, static_lds = 0, scratch = 0;
  bool cached = false;  // loaded from the code-object cache (rt_jit.cpp cache_path), not compiled
};
int get_kernel(const std::string& walker, int device, const rtv::Variant& v, int launch,
               Kernel* out, std::string* log);
// A scene's hold on a kernel from get_kernel ends (rt_scene_destroy). The process-wide cache keeps
// every kernel some scene holds, plus up to kIdleModules unheld ones for scenes created again
// with the same geometry; older unheld modules are unloaded (hipModuleUnload).
constexpr int kIdleModules = 8;
void release_kernel(const Kernel& k);

// The hiprtc translation unit (embedded headers + walker + rt_trace_jit wrapper) and its
// compilation for `arch` (e.g. "gfx950") into a code object; host-only, no device needed.
// use_cache = false bypasses the code-object cache (a cached entry that failed to load).
std::string kernel_source(const std::string& walker, const rtv::Variant& v, int launch);
int compile(const std::string& src, const std::string& arch, std::vector<char>* code,
            std::string* log, bool use_cache = true);

}  // namespace rtj
