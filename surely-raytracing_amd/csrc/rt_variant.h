// rt_variant.h — which instance of the path kernel (rt_kernel.h trace_body) a scene runs: the
// template arguments the scene determines, the one function that chooses them, and the one list of
// the instances that exist. Host only, plain C++ (no HIP; build/variant_check compiles it alone).
//
// The launch decides COUNT (RT_FLAG_COUNT_OPS) and the launch kind (plain, rt_render_tiles_device's
// tile list, rt_render_rays_device's rays), the kernel's
// origin the walker (the interpreter ahead of time, TravGen in a scene-specialised kernel).
// Everything that needs the choice calls choose_variant: the render's kernel lookup, the
// scene-specialised kernel's template arguments and the occupancy cache (rt_device.hip), the
// tile-list and ray kernels (rt_tiles.hip, rt_rays.hip), the AOV pass (rt_aov.hip: bvh, staged, vn) and the probe
// (probe/rt_probe_scene.hip).
#pragma once
#include <stdint.h>

#include "rt_layout.h"
#include "rt_mi355x.h"

namespace rtv {

struct Variant {
  bool vol;     // ConstantMedium nodes or an Isotropic material (also usable outside one)
  bool tex;     // some material reads a non-solid texture
  bool bvh;     // BVH records: the per-lane walker, the 768-thread workgroup
  bool staged;  // no BVH and the small tables staged in LDS: LDS-typed table reads
  bool volb;    // the per-lane BVH walker keeps its volume branch
  bool voli;    // the top-level walker keeps the two-walk volume interpreter
  int vn;       // ConstantMedium records nested in volume boundaries, that deep (0: none)
};
inline bool operator==(const Variant& a, const Variant& b) {
  return a.vol == b.vol && a.tex == b.tex && a.bvh == b.bvh && a.staged == b.staged &&
         a.volb == b.volb && a.voli == b.voli && a.vn == b.vn;
}

// stage_scene: the launch's LDS plan copies the scene's small tables whole (LdsPlan::stage_scene).
inline Variant choose_variant(const rtl_scene_header& hdr, uint32_t flags, bool stage_scene) {
  Variant v;
  v.vol = (hdr.has_volume | hdr.has_isotropic) != 0;
  v.tex = hdr.has_textures != 0;
  v.bvh = hdr.has_bvh != 0;
  // a scene without a BVH whose tables are staged in LDS runs the STAGED variant, BVH kernels read
  // the tables from global memory
  v.staged = !v.bvh && stage_scene && !hdr.nested_volumes;
  // BVH scenes whose volumes all sit outside BVH subtrees (final_scene) run the variant whose
  // per-lane walker has no volume branch; when those volumes are all one-walk spheres, the
  // top-level walker carries no two-walk interpreter either (the op-counting build always walks
  // twice, so only product kernels drop it)
  const bool novolb = v.bvh && v.vol && !hdr.volume_in_bvh;
  v.volb = novolb ? false : v.vol;
  v.voli = !(novolb && hdr.volumes_one_walk_spheres && !(flags & RT_FLAG_COUNT_OPS));
  v.vn = 0;
  // ConstantMedium nested in volume boundaries (rt_flatten.cpp: at most RTL_VOLUME_NEST deep):
  // the generic texture/volume kernels that walk them
  if (hdr.nested_volumes) {
    v.vol = v.tex = v.volb = v.voli = true;
    v.vn = RTL_VOLUME_NEST;
  }
  return v;
}

}  // namespace rtv

// The instances that exist: X(vol, tex, bvh, staged, volb, voli, vn), every Variant that
// choose_variant can return. rt_device.hip, rt_tiles.hip and rt_rays.hip instantiate their kernels from these
// rows and build their lookup (by equality on the Variant) from the same tokens. The op-counting
// kernels exist for the rows with voli (choose_variant never clears it under RT_FLAG_COUNT_OPS).
#define RT_VARIANTS(X)                                                               \
  /* [vol][tex][bvh], tables in global memory */                                     \
  X(false, false, false, false, false, true, 0)                                      \
  X(false, false, true, false, false, true, 0)                                       \
  X(false, true, false, false, false, true, 0)                                       \
  X(false, true, true, false, false, true, 0)                                        \
  X(true, false, false, false, true, true, 0)                                        \
  X(true, false, true, false, true, true, 0)                                         \
  X(true, true, false, false, true, true, 0)                                         \
  X(true, true, true, false, true, true, 0)                                          \
  /* [vol][tex], no BVH, staged */                                                   \
  X(false, false, false, true, false, true, 0)                                       \
  X(false, true, false, true, false, true, 0)                                        \
  X(true, false, false, true, true, true, 0)                                         \
  X(true, true, false, true, true, true, 0)                                          \
  /* BVH, every volume outside the subtrees: [two-walk interpreter][tex] */          \
  X(true, false, true, false, false, true, 0)                                        \
  X(true, true, true, false, false, true, 0)                                         \
  X(true, false, true, false, false, false, 0)                                       \
  X(true, true, true, false, false, false, 0)                                        \
  /* nested volumes: [bvh] */                                                        \
  X(true, true, false, false, true, true, RTL_VOLUME_NEST)                           \
  X(true, true, true, false, true, true, RTL_VOLUME_NEST)
