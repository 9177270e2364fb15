"""Every row of RT_VARIANTS (csrc/rt_variant.h) on the device, each with its scene of
tests/variant_scenes.py (tests/test_variant_matrix.py shows on the CPU that the 18 scenes select
the 18 rows). Per row, for two seeds whose op counts do not depend on the rounding of a dot
product: the product kernel, the op-counting kernel and the interpreter's product kernel give the
same image bit for bit; the image has the f64 oracle's NaN / inf masks and lies within TOL of it
per sample; the op counts are the oracle's exactly. The first seed goes through
test_gpu_parity._compare (a DeviceScene per render), the second through the same checks on one
DeviceScene, on which the first seed's product render is repeated: the scene-specialised kernel of
the row (hiprtc, same template arguments) really ran, for the plain and for the tile-list render,
in every scene but the two nested ones; the tile-list kernels (plain and interpreter) over the
full tile list give the plain render bit for bit.

The row "nested volumes, BVH" is the one whose product kernel faulted when this test first
launched it: kparams() is null in a called function, and only this row's kernels are large enough
for the inliner to leave the per-lane BVH walker in one (rt_kernel.h kparams, traverse's PK)."""
import time

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
import variant_scenes as V
from adaptive_cases import bits
from hip_buf import DevBuf
from test_gpu_parity import TOL, _check_values, _compare

pytestmark = pytest.mark.gpu

OW = rt.RT_FLAG_OVERWRITE
ROWS = V.parse_rows()
IDS = ["".join(map(str, k)) for k in ROWS]


def same(a, b):
    """bit for bit, which includes equal NaN / inf masks"""
    return np.array_equal(bits(a), bits(b))


def tiles_all(ds, cam, seed, flags):
    """rt_render_tiles_device over the full tile list at stride 1 (test_zero_throughput_gpu.py
    Scene.tiles_all)"""
    tx, ty = rt.tile_grid(cam.image_width, cam.image_height)
    b = DevBuf((cam.image_height, cam.image_width, 3))
    try:
        o = rt.make_opts(cam, seed=seed, flags=flags, sj_count=cam.sqrt_spp)
        ds.render_tiles_device(cam, o, np.arange(tx * ty), 1, b.ptr, 0)
        return b.download()
    finally:
        b.free()


@pytest.mark.parametrize("key", ROWS, ids=IDS)
def test_row_against_the_oracle(gpu_available, key):
    t0 = time.perf_counter()
    blob, cam = V.build(key), V.camera(key, ROWS)
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (20, 12, 4)
    spp = cam.samples_per_pixel
    # product vs counting vs interpreter, oracle masks, TOL, op counts with ops_rtol = 0
    acc_g, acc_o, st = _compare(blob, cam, seed=V.SEEDS[0])
    worst = np.abs(acc_g.astype(np.float64) - acc_o.astype(np.float64)).max() / spp
    print(f"{key} seed {V.SEEDS[0]}: max |gpu - oracle| / spp {worst:.3e} (TOL {TOL})")
    want = -1 if key[6] else 1

    def ran_specialised(ds, what):
        """the scene-specialised kernel of the render just made was the one that ran"""
        state, msg = ds.jit_info()
        print(f"{key}: {what}: jit state {state}: {msg[:240]}")
        if "not launched:" in msg:
            # the code object's resources do not fit this launch (rt_device.hip select_kernel):
            # the row then stands on its ahead-of-time kernels
            print(f"{key}: {what}: {msg}")
        else:
            assert state == want, (key, what, state, msg[:2000])

    ds = rt.DeviceScene(blob)
    try:
        # the first seed again, on the one handle: the kernels that ran, the tile-list renders
        s0 = V.SEEDS[0]
        prod, _ = ds.render(cam, rt.make_opts(cam, seed=s0, flags=OW))
        ran_specialised(ds, "render")
        assert same(prod, acc_g), "one DeviceScene vs _compare's product render"
        assert same(prod, tiles_all(ds, cam, s0, OW)), "plain vs tile-list render"
        ran_specialised(ds, "tile-list render")  # its own kernel and slot (select_kernel)
        assert same(prod, tiles_all(ds, cam, s0, OW | rt.RT_FLAG_INTERPRETER)), \
            "plain vs interpreter tile-list render"
        # the second seed: every check of _compare, and the tile-list renders
        seed = V.SEEDS[1]
        acc_o, ops_o = O.render(blob, cam, rt.make_opts(cam, seed=seed), precision=64)
        assert np.isfinite(acc_o).all()
        prod, _ = ds.render(cam, rt.make_opts(cam, seed=seed, flags=OW))
        cnt, st = ds.render(cam, rt.make_opts(cam, seed=seed, flags=OW | rt.RT_FLAG_COUNT_OPS))
        assert same(prod, cnt), "product vs counting build"
        interp, _ = ds.render(cam, rt.make_opts(cam, seed=seed, flags=OW | rt.RT_FLAG_INTERPRETER))
        assert same(prod, interp), "scene-specialised vs interpreter kernel"
        _check_values(prod, acc_o, cam)
        ops_g = st.op_counts()
        bad = {k: (ops_g[k], ops_o[k]) for k in ops_o if ops_g[k] != ops_o[k]}
        assert not bad, (seed, bad)
        assert st.samples == 20 * 12 * spp
        assert same(prod, tiles_all(ds, cam, seed, OW)), "plain vs tile-list render"
        assert same(prod, tiles_all(ds, cam, seed, OW | rt.RT_FLAG_INTERPRETER)), \
            "plain vs interpreter tile-list render"
        d = np.abs(prod.astype(np.float64) - acc_o.astype(np.float64)).max() / spp
        worst = max(worst, d)
        print(f"{key} seed {seed}: max |gpu - oracle| / spp {d:.3e} (TOL {TOL})")
    finally:
        ds.close()
    print(f"{key}: max |gpu - oracle| / spp over both seeds {worst:.3e}; "
          f"test wall time {time.perf_counter() - t0:.2f} s")
