"""The path-kernel variant of a scene (csrc/rt_variant.h choose_variant: the template arguments
vol, tex, bvh, staged, volb, voli, vn of trace_body) is chosen in one place. The stand-alone host
program build/variant_check (csrc/host/variant_check.cpp, built by the Makefile with the host
compiler alone) prints the choice for every input: the seven scene-header bits it reads x
RT_FLAG_COUNT_OPS x the LDS plan's stage_scene. Each line is compared with the rules restated here,
and the presets' variants with the ones DESIGN.md §4.2f lists."""
import itertools
import subprocess
from pathlib import Path

import pytest

import surely_rt as rt

REPO = Path(__file__).resolve().parent.parent
EXE = REPO / "build" / "variant_check"
VOLUME_NEST = 2  # csrc/rt_layout.h RTL_VOLUME_NEST
PERLIN_BYTES = 4096 + 768  # csrc/rt_layout.h RTL_PERLIN_BYTES


def rules(has_volume, has_isotropic, has_textures, has_bvh, volume_in_bvh, one_walk_spheres,
          nested_volumes, count_ops, stage_scene):
    """(vol, tex, bvh, staged, volb, voli, vn) by the rules of the variant choice"""
    vol = bool(has_volume or has_isotropic)
    tex = bool(has_textures)
    bvh = bool(has_bvh)
    staged = (not bvh) and bool(stage_scene) and not nested_volumes
    novolb = bvh and vol and not volume_in_bvh
    volb = False if novolb else vol
    voli = not (novolb and one_walk_spheres and not count_ops)
    vn = 0
    if nested_volumes:
        vol = tex = volb = voli = True
        vn = VOLUME_NEST
    return tuple(int(x) for x in (vol, tex, bvh, staged, volb, voli, vn))


def run(*args):
    assert EXE.exists(), "build/variant_check is missing: run make (or __graft_entry__.build())"
    out = subprocess.run([str(EXE), *map(str, args)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = []
    for ln in out.stdout.splitlines():
        lhs, rhs = ln.split("->")
        lines.append((tuple(map(int, lhs.split())), tuple(map(int, rhs.split()))))
    return lines


def test_every_input_gets_the_variant_of_the_rules():
    lines = run()
    assert [i for i, _ in lines] == list(itertools.product((0, 1), repeat=9))  # 512, each once
    for inp, got in lines:
        assert got == rules(*inp), inp


# preset -> (has_textures, volume_in_bvh as the scene is built, the variant DESIGN.md lists):
# cornell_smoke's two media are boxes in the world list; final_scene's two media are spheres added to
# the world list beside its BVHs, and it has noise and image textures
PRESETS = {
    "cornell_box": (0, 0, (0, 0, 0, 1, 0, 1, 0)),
    "cornell_smoke": (0, 0, (1, 0, 0, 1, 1, 1, 0)),
    "final_scene": (1, 0, (1, 1, 1, 0, 0, 0, 0)),
    "two_perlin_spheres": (1, 0, (0, 1, 0, 1, 0, 1, 0)),
    "earth": (1, 0, (0, 1, 0, 1, 0, 1, 0)),
}


@pytest.mark.parametrize("name", list(PRESETS))
def test_presets_run_the_variant_the_design_lists(name):
    tex, vol_in_bvh, want = PRESETS[name]
    blob, _ = rt.preset_blob(name, width=16, spp=4)
    ls, plan = rt.layout_stats(blob), rt.lds_check(blob, n_rays=0)
    has_volume = int(ls["volumes"] > 0)
    one_walk = int(ls["volumes"] > 0 and ls["volumes_one_walk_sphere"] == ls["volumes"])
    # the plan stages the whole small-table prefix (more than the Perlin tables alone) or not
    perlins = blob.header()["n_perlin"] if tex else 0
    stage_scene = int(plan["stage_bytes"] > perlins * PERLIN_BYTES)
    (_, got), = run(has_volume, has_volume, tex, int(ls["bvh_records"] > 0), vol_in_bvh, one_walk,
                    0, 0, stage_scene)
    assert got == want
