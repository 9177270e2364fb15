"""One smallest scene per row of RT_VARIANTS (csrc/rt_variant.h): the path kernel's 18 instances,
keyed by the row's template arguments (vol, tex, bvh, staged, volb, voli, vn). TEST INFRASTRUCTURE
ONLY. tests/test_variant_matrix.py checks on the CPU that the 18 scenes select the 18 rows, each
once, and that the oracle reaches each row's feature; tests/test_variant_matrix_gpu.py renders
every row's kernels against the f64 oracle.

Every scene, through the public rt.Scene API: a Lambertian floor and ball, a metal and a glass
ball in view, one light quad in the world and in the light list, a sky-coloured background.
  tex   a noise_texture ball and a checker floor (otherwise solid colours only)
  vol   a ConstantMedium: over a box where the row keeps the two-walk interpreter (voli), over a
        sphere for the two rows that drop it (every boundary a one-walk sphere)
  bvh   the balls (and two small ones: 5 leaves, a span-1 node) in a create_bvh list; with volb
        the medium is one of that list's items, without it the medium sits beside the BVH in the
        world list
  vn    a ConstantMedium inside another one's boundary (test_nested_constant_medium_parity), in
        the world list; the BVH row has a plain fog ball among its leaves as well
  staged = 0 without a BVH: a flat world list whose table prefix (nodes, materials, textures,
        lights, light offsets, used Perlin tables; rt_device.hip plan_lds) just exceeds kStageScene
        = 24 KiB: a mosaic back wall of small quads, each with its own Lambertian material and
        solid texture (a record, a material and a texture per tile). UNSTAGED_TILES states the
        smallest tile count for which the LDS plan no longer stages the scene
        (stage_scene(blob), the derivation of test_variant_choice.py); with one tile fewer the
        scene is staged (test_variant_matrix.py asserts both).

Cameras: 20 x 12 pixels (ragged 8 x 8 tiles on both edges), 4 spp, depth 6, a thin lens on every
other row of RT_VARIANTS.
"""
import re
from pathlib import Path

import surely_rt as rt

REPO = Path(__file__).resolve().parent.parent
VARIANT_H = REPO / "surely-raytracing_amd" / "csrc" / "rt_variant.h"
VOLUME_NEST = 2  # csrc/rt_layout.h RTL_VOLUME_NEST
PERLIN_BYTES = 4096 + 768  # csrc/rt_layout.h RTL_PERLIN_BYTES
STAGE_SCENE = 24 << 10  # csrc/rt_kernel.h kStageScene

WIDTH, HEIGHT, SPP, DEPTH = 20, 12, 4, 6
BACKGROUND = (0.35, 0.45, 0.6)
# the oracle's op counts for these two seeds are those of the fused-dot oracle
# (liboracle_f64fma.so) in every scene (test_variant_matrix.py asserts it): no path decision
# hangs on the last bit of a dot product, so the device's counts must be the oracle's exactly
SEEDS = (1, 2)

# (vol, tex) of a flat unstaged scene -> its mosaic's tile count, the smallest that is not staged
UNSTAGED_TILES = {(0, 0): 72, (0, 1): 56, (1, 0): 67, (1, 1): 52}
MOSAIC_COLUMNS = 12


def parse_rows(text=None):
    """The X(...) rows of RT_VARIANTS as 7-tuples of ints, in the header's order."""
    text = VARIANT_H.read_text() if text is None else text
    body = text[text.index("#define RT_VARIANTS(X)"):]
    rows = []
    for m in re.finditer(r"^\s*X\(([^)]*)\)", body, re.M):
        f = [t.strip() for t in m.group(1).split(",")]
        assert len(f) == 7, m.group(0)
        val = {"true": 1, "false": 0, "RTL_VOLUME_NEST": VOLUME_NEST}
        rows.append(tuple(val[t] if t in val else int(t) for t in f))
    return rows


def stage_scene(blob, tex):
    """Whether the launch's LDS plan stages the scene's small tables whole: it then stages more
    than the used Perlin tables alone (test_variant_choice.py's derivation)."""
    plan = rt.lds_check(blob, n_rays=0)
    perlins = blob.header()["n_perlin"] if tex else 0
    return int(plan["stage_bytes"] > perlins * PERLIN_BYTES), plan["stage_bytes"]


def camera(key, rows=None):
    rows = parse_rows() if rows is None else rows
    lens = (1.5, 9.0) if rows.index(key) % 2 else (0.0, 0.0)
    vol, tex, bvh, staged = key[:4]
    # the unstaged flat scenes look a little narrower, at the balls and the mosaic behind them
    vfov = 24.0 if not bvh and not staged and not key[6] else 27.0
    cam = rt.camera_new(5.0 / 3.0, WIDTH, SPP, DEPTH, vfov, (0.3, 2.0, 9.0), (0.0, 0.8, 0.0),
                        (0, 1, 0), *lens, BACKGROUND)
    assert (cam.image_width, cam.image_height, cam.sqrt_spp) == (WIDTH, HEIGHT, 2)
    return cam


def _medium(sc, white, kind):
    """A ConstantMedium behind the balls: over a box, over a sphere, or a nest of two."""
    if kind == "box":
        return sc.constant_medium(sc.make_box((-0.9, -0.3, -2.0), (0.9, 1.9, -0.6), white), 0.9,
                                  (0.85, 0.85, 0.9))
    if kind == "sphere":
        return sc.constant_medium(sc.sphere((0.0, 0.9, -1.2), 1.1, white), 0.9, (0.85, 0.85, 0.9))
    assert kind == "nest"
    inner = sc.constant_medium(sc.sphere((0.0, 0.9, -1.2), 0.6, white), 3.0, (0.9, 0.3, 0.2))
    return sc.constant_medium(sc.hittable_list(sc.sphere((0.0, 0.9, -1.2), 1.1, white), inner),
                              0.7, (0.3, 0.5, 0.9))


def build(key, tiles=None):
    """The scene of the row `key` -> Blob. tiles: the mosaic's tile count of an unstaged flat scene
    (default: UNSTAGED_TILES)."""
    vol, tex, bvh, staged, volb, voli, vn = key
    sc = rt.Scene(100 + 64 * vol + 32 * tex + 16 * bvh + 8 * staged + 4 * volb + 2 * voli + vn)
    white = sc.lambertian((0.73, 0.73, 0.73))
    light = sc.diffuse_light((9, 9, 9))
    # the floor below the checker's own discontinuity plane y = 0 (test_gpu_parity.py)
    ground = (sc.lambertian(tex=sc.checker_from_color(0.8, (0.85, 0.2, 0.15), (0.15, 0.3, 0.85)))
              if tex else sc.lambertian((0.5, 0.6, 0.4)))
    floor = sc.quad((-6, -0.3, -6), (12, 0, 0), (0, 0, 12), ground)
    lamp = sc.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), light)
    balls = [sc.sphere((-1.7, 0.5, 0.6), 0.8, sc.metal((0.8, 0.7, 0.5), 0.15)),
             sc.sphere((1.7, 0.5, 0.9), 0.8, sc.dielectric(1.5)),
             sc.sphere((0.0, 0.35, 2.2), 0.65,
                       sc.lambertian(tex=sc.noise_texture(3.0)) if tex
                       else sc.lambertian((0.65, 0.1, 0.1)))]
    medium = None
    if vol:
        medium = _medium(sc, white, "nest" if vn else "box" if voli else "sphere")
    items = [floor, lamp]
    if bvh:
        leaves = balls + [sc.sphere((-0.9, -0.05, 3.0), 0.25, white),
                          sc.sphere((1.0, -0.05, 3.2), 0.25, sc.lambertian((0.1, 0.6, 0.3)))]
        # the flattener takes no nest inside a BVH: the nest stays in the world list, and the
        # per-lane walker's volume branch, which the nested kernel keeps, gets a plain fog ball
        in_bvh = medium is not None and volb and not vn
        if in_bvh:
            leaves.append(medium)
        if vn:
            leaves.append(sc.constant_medium(sc.sphere((-2.6, 0.3, 2.0), 0.6, white), 1.2,
                                             (0.8, 0.8, 0.8)))
        items.append(sc.create_bvh(sc.hittable_list(*leaves)))
        if medium is not None and not in_bvh:
            items.append(medium)
    else:
        items += balls
        if medium is not None:
            items.append(medium)
        if not staged and not vn:
            n = UNSTAGED_TILES[vol, tex] if tiles is None else tiles
            for k in range(n):  # the mosaic: 0.5 x 0.5 tiles, columns left to right, rows upwards
                i, j = k % MOSAIC_COLUMNS, k // MOSAIC_COLUMNS
                col = (0.15 + 0.07 * (k % 11), 0.2 + 0.06 * (k % 13), 0.25 + 0.1 * (k % 7))
                items.append(sc.quad((-3.0 + 0.5 * i, -0.3 + 0.5 * j, -2.5), (0.5, 0, 0),
                                     (0, 0.5, 0), sc.lambertian(col)))
    world = sc.hittable_list(*items)
    lights = sc.hittable_list(sc.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), light))
    return sc.serialize(world, lights)


def scenes():
    """{row: (blob, camera)} for the 18 rows, in the header's order."""
    rows = parse_rows()
    return {key: (build(key), camera(key, rows)) for key in rows}
