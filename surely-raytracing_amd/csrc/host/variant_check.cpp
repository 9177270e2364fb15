// variant_check — host print-out of the path-kernel variant choice (rt_variant.h choose_variant).
// Without arguments: one line per input over the full product of the seven scene-header bits the
// choice reads x RT_FLAG_COUNT_OPS x the plan's stage_scene (512 lines),
//   has_volume has_isotropic has_textures has_bvh volume_in_bvh volumes_one_walk_spheres
//   nested_volumes count_ops stage_scene -> vol tex bvh staged volb voli vn
// With those nine inputs as arguments: that one line. Exits 1 when a chosen variant is not a row of
// RT_VARIANTS (no kernel instance would exist for it). Built by the Makefile with the host
// compiler alone (build/variant_check), run by tests/test_variant_choice.py.
#include <cstdio>
#include <cstdlib>

#include "../rt_variant.h"

namespace {

bool listed(const rtv::Variant& v) {
#define RT_VARIANT_ROW(vol, tex, bvh, staged, volb, voli, vn) \
  if (v == rtv::Variant{vol, tex, bvh, staged, volb, voli, vn}) return true;
  RT_VARIANTS(RT_VARIANT_ROW)
#undef RT_VARIANT_ROW
  return false;
}

bool line(const int in[9]) {
  rtl_scene_header h{};
  h.has_volume = in[0], h.has_isotropic = in[1], h.has_textures = in[2], h.has_bvh = in[3];
  h.volume_in_bvh = in[4], h.volumes_one_walk_spheres = in[5], h.nested_volumes = in[6];
  const rtv::Variant v = rtv::choose_variant(h, in[7] ? RT_FLAG_COUNT_OPS : 0u, in[8] != 0);
  std::printf("%d %d %d %d %d %d %d %d %d -> %d %d %d %d %d %d %d\n", in[0], in[1], in[2], in[3],
              in[4], in[5], in[6], in[7], in[8], v.vol, v.tex, v.bvh, v.staged, v.volb, v.voli,
              v.vn);
  return listed(v);
}

}  // namespace

int main(int argc, char** argv) {
  int in[9];
  bool ok = true;
  if (argc == 10) {
    for (int k = 0; k < 9; ++k) in[k] = std::atoi(argv[k + 1]) != 0;
    ok = line(in);
  } else {
    for (int x = 0; x < 512; ++x) {
      for (int k = 0; k < 9; ++k) in[k] = (x >> (8 - k)) & 1;
      ok = line(in) && ok;
    }
  }
  if (!ok) std::fprintf(stderr, "variant_check: a chosen variant is not in RT_VARIANTS\n");
  return ok ? 0 : 1;
}
