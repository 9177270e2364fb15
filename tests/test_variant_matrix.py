"""Every row of RT_VARIANTS (csrc/rt_variant.h: the 18 instances of the path kernel) has one
smallest scene in tests/variant_scenes.py that selects it. Checked here without a GPU: each scene's
header bits (the probe library's rtp_scene_header, the product's flattener) and LDS plan
(rt.lds_check) go through build/variant_check, and the variant it prints is the scene's key; the
18 keys are the 18 parsed rows, each once; the f64 oracle renders every scene finite and its op
counts show that the row's feature is reached; the two render seeds give the fused-dot oracle the
same op counts; the scene-specialised walker of every non-nested scene is generated and compiled.
tests/test_variant_matrix_gpu.py then renders every row's kernels.

The four flat scenes that are not staged (no BVH, tables read from global memory):
  (vol, tex)   tiles   primitives   stage_bytes with one tile fewer (staged, <= 24576)
  (0, 0)       72      77           24464
  (0, 1)       56      61           24304 (of which one Perlin table, 4864)
  (1, 0)       67      78           24336
  (1, 1)       52      63           24496 (of which one Perlin table, 4864)
(primitives: the tiles, the floor, the lamp and three balls, plus the medium's six box faces;
test_unstaged_scenes_are_the_smallest_that_are_not_staged asserts the tile counts and these
stage_bytes, and prints the plans.)"""
import time

import numpy as np
import pytest

import oracle_lib as O
import probe_lib as P
import surely_rt as rt
import variant_scenes as V
from test_variant_choice import run, rules

BITS = ("has_volume", "has_isotropic", "has_textures", "has_bvh", "volume_in_bvh",
        "volumes_one_walk_spheres", "nested_volumes")
ROWS = V.parse_rows()
IDS = ["".join(map(str, k)) for k in ROWS]
FLAT_UNSTAGED = [k for k in ROWS if not k[2] and not k[3] and not k[6]]


@pytest.fixture(scope="module")
def scenes():
    return V.scenes()


@pytest.fixture(scope="module")
def oracle(scenes):
    """{row: {seed: (frame, op counts)}} of the f64 oracle, rendered once"""
    return {k: {s: O.render(b, c, rt.make_opts(c, seed=s), precision=64) for s in V.SEEDS}
            for k, (b, c) in scenes.items()}


def chosen(blob, tex, count_ops):
    """the variant build/variant_check prints for the scene's header bits and LDS plan"""
    h = P.scene_header(blob)
    stage, _ = V.stage_scene(blob, tex)
    inp = tuple(int(h[b] != 0) for b in BITS) + (count_ops, stage)
    (got_in, got), = run(*inp)
    assert got_in == inp and got == rules(*inp)
    return got


def test_the_header_lists_18_rows_each_once():
    assert len(ROWS) == 18 and len(set(ROWS)) == 18
    assert V.parse_rows("#define RT_VARIANTS(X) \\\n  /* c */ \\\n  X(true, false, true, false, "
                        "false, true, RTL_VOLUME_NEST)\n") == [(1, 0, 1, 0, 0, 1, V.VOLUME_NEST)]
    # the op-counting kernels exist for the rows with voli: all but two
    assert sum(1 for r in ROWS if r[5]) == 16


def test_18_scenes_cover_the_18_rows_exactly(scenes):
    assert list(scenes) == ROWS
    got = [chosen(blob, key[1], 0) for key, (blob, _) in scenes.items()]
    for key, g in zip(ROWS, got):
        assert g == key, (key, g)
    assert sorted(got) == sorted(ROWS) and len(set(got)) == 18


def test_counting_renders_land_on_a_row_that_keeps_the_interpreter(scenes):
    """RT_FLAG_COUNT_OPS: the variant is again a row (variant_check exits 1 otherwise), one with
    voli = 1, and only the two rows without voli move (to their voli = 1 neighbours)."""
    with_voli = {r for r in ROWS if r[5]}
    landed = {}
    for key, (blob, _) in scenes.items():
        got = chosen(blob, key[1], 1)
        assert got in with_voli, (key, got)
        landed[key] = got
        print(f"{key} -> counting build {got}")
    moved = {k: g for k, g in landed.items() if g != k}
    assert moved == {(1, 0, 1, 0, 0, 0, 0): (1, 0, 1, 0, 0, 1, 0),
                     (1, 1, 1, 0, 0, 0, 0): (1, 1, 1, 0, 0, 1, 0)}


def test_cameras(scenes):
    for n, (key, (_, cam)) in enumerate(scenes.items()):
        assert (cam.image_width, cam.image_height) == (20, 12) == (V.WIDTH, V.HEIGHT)
        assert rt.tile_grid(20, 12) == (3, 2)  # ragged on both edges
        assert cam.samples_per_pixel == 4 and cam.max_depth == 6
        assert (cam.defocus_angle > 0) == bool(n % 2)
        assert tuple(cam.background[:]) == V.BACKGROUND and min(V.BACKGROUND) > 0


def test_unstaged_scenes_are_the_smallest_that_are_not_staged():
    assert len(FLAT_UNSTAGED) == 4
    assert V.UNSTAGED_TILES == {(0, 0): 72, (0, 1): 56, (1, 0): 67, (1, 1): 52}
    one_fewer = {(0, 0): 24464, (0, 1): 24304, (1, 0): 24336, (1, 1): 24496}  # the docstring's
    for key in FLAT_UNSTAGED:
        vol, tex = key[:2]
        n = V.UNSTAGED_TILES[vol, tex]
        assert n < 100
        perl = V.PERLIN_BYTES if tex else 0
        stage, nbytes = V.stage_scene(V.build(key), tex)
        assert stage == 0 and nbytes == perl  # only the Perlin table is staged, if any
        stage1, nbytes1 = V.stage_scene(V.build(key, tiles=n - 1), tex)
        assert stage1 == 1 and perl < nbytes1 <= V.STAGE_SCENE and nbytes1 == one_fewer[vol, tex]
        prims = n + 5 + (6 if vol else 0)
        print(f"(vol, tex) = {(vol, tex)}: {n} tiles, {prims} primitives: stage_bytes {nbytes}, "
              f"not staged; {n - 1} tiles: stage_bytes {nbytes1} <= {V.STAGE_SCENE}, staged")
        assert nbytes1 + 2 * 320 > V.STAGE_SCENE  # about 320 B per tile: n is the threshold


@pytest.mark.parametrize("key", ROWS, ids=IDS)
def test_oracle_reaches_the_rows_feature(oracle, key):
    vol, tex, bvh = key[:3]
    for seed in V.SEEDS:
        frame, ops = oracle[key][seed]
        assert frame.shape == (12, 20, 3) and np.isfinite(frame).all() and frame.min() >= 0.0
        assert ops["samples"] == 20 * 12 * 4
        for k in ("metal", "dielectric", "lambertian", "light_gen", "cosine_gen", "misses"):
            assert ops[k] > 0, (key, seed, k)
        assert (ops["noise_evals"] > 0) == bool(tex)
        assert (ops["volume_draws"] > 0) == bool(vol) and (ops["isotropic"] > 0) == bool(vol)
        assert (ops["aabb_tests"] > 0) == bool(bvh)


@pytest.mark.parametrize("key", ROWS, ids=IDS)
def test_fused_dot_oracle_counts_the_same_ops(scenes, oracle, key):
    """No path of the two seeds hangs on the last bit of a dot product: the oracle with fused dot
    products (liboracle_f64fma.so, tools/flip_study.py) takes the same decisions, so the device's
    op counts must be the oracle's exactly (ops_rtol = 0 in the GPU test)."""
    blob, cam = scenes[key]
    for seed in V.SEEDS:
        _, ops = O.render(blob, cam, rt.make_opts(cam, seed=seed), precision="64fma")
        assert ops == oracle[key][seed][1], (key, seed)


def test_scene_specialised_walkers_compile(scenes):
    """rt.jit_check generates and compiles the walker of every scene but the two nested ones
    (rtj::generate refuses them). The compile times are printed beside cornell_smoke's."""
    t0 = time.perf_counter()
    state, _ = rt.jit_check(rt.preset_blob("cornell_smoke", width=16, spp=4)[0])
    smoke = time.perf_counter() - t0
    assert state == 1
    print(f"cornell_smoke: {smoke:.2f} s")
    for key, (blob, _) in scenes.items():
        t0 = time.perf_counter()
        state, msg = rt.jit_check(blob)
        dt = time.perf_counter() - t0
        print(f"{key}: state {state}, {dt:.2f} s" + (f" ({msg})" if state != 1 else ""))
        assert state == (-1 if key[6] else 1), (key, msg)
