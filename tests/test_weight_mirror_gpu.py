"""GPU: the f32 weight mirrors (rt_layout.h RTL_MATF_SOLID_W) against the conversion they replace,
and small renders through every kernel that reads them.

1. The device's to_w3 (v_cvt_f32_f64 in the kernels' mode) gives the bits of the host's (float)
   cast, which is what the flattener stores: on the edge values of tests/weight_mirror_lib.py
   (f32 subnormals, the overflow threshold, NaN, -0.0, ties) and on random doubles of every
   exponent range a colour can have.
2. 20 x 12 pixels (a right-edge partial 8 x 8 tile and a partial bottom tile), 16 spp, depth 8:
   the scene-specialised product kernel, the op-counting build and the interpreter's product
   kernel give the same image bit for bit, and the image is the f64 oracle's within the tolerance
   of tests/test_gpu_parity.py (1e-4 on the per-sample average, equal NaN / inf masks, equal op
   counts); that file's _compare is the comparison, unchanged.
"""
import numpy as np
import pytest

import surely_rt as rt
import test_gpu_parity as G
import weight_mirror_lib as W

pytestmark = pytest.mark.gpu


def test_device_to_w3_is_the_host_cast(gpu_available):
    rng = np.random.default_rng(11)
    n = 4096 - W.EDGE.size
    # random bit patterns (every exponent, NaN payloads and both infinities included), colours in
    # [0, 16), and doubles around the f32 subnormal range and the overflow threshold
    bits = rng.integers(0, 1 << 64, size=n // 4, dtype=np.uint64).view(np.float64)
    unit = rng.random(n // 4) * 16.0
    tiny = np.ldexp(rng.random(n // 4) + 0.5, rng.integers(-160, -120, n // 4)) * rng.choice([-1.0, 1.0], n // 4)
    huge = np.ldexp(rng.random(n - 3 * (n // 4)) + 0.5, rng.integers(120, 132, n - 3 * (n // 4)))
    x = np.concatenate([W.EDGE, bits, unit, tiny, huge])
    assert x.size == 4096
    got, want = W.to_w3_bits(x), W.f32_bits(x)
    nan = np.isnan(x)
    # Every NaN stays a NaN. IEEE 754 leaves the payload of a narrowed NaN to the implementation,
    # and nothing downstream reads it (frames are compared by NaN mask), so the random NaN
    # patterns are held to that alone; the NaN of the edge list (the default quiet NaN, what a
    # scene description can produce) and every non-NaN value are held to the host cast's bits.
    assert ((got[nan] & 0x7f800000) == 0x7f800000).all() and ((got[nan] & 0x7fffff) != 0).all()
    print("random NaN payloads that differ from the host's:", int((got != want)[W.EDGE.size:].sum()))
    held = ~nan
    held[:W.EDGE.size] = True
    bad = np.flatnonzero((got != want) & held)
    assert bad.size == 0, [(float(x[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    sub = (want & 0x7f800000 == 0) & (want & 0x7fffffff != 0)
    assert sub.sum() > 100 and np.isinf(want.view(np.float32)).sum() > 100  # the classes occurred


def _mixed_scene():
    """Tinted glass, fuzzy metal and a solid emitter (their colours come from the material record's
    mirror), a solid Lambertian floor (the flagged path), one checker and one noise Lambertian (the
    unflagged path, TEX kernels), under a non-black background (TraceParams::bg_w)."""
    sc = rt.Scene(23)
    white = sc.lambertian((0.73, 0.73, 0.73))
    chk = sc.lambertian(tex=sc.checker_from_color(0.9, (0.9, 0.2, 0.1), (0.1, 0.3, 0.9)))
    marble = sc.lambertian(tex=sc.noise_texture(4.0))
    glass = sc.dielectric(1.5, (0.9, 0.6, 0.95))
    metal = sc.metal((0.8, 0.7, 0.3), 0.3)
    light = sc.diffuse_light((7, 6, 5))
    lq = sc.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), light)
    world = sc.hittable_list(sc.quad((-5, -0.3, -5), (10, 0, 0), (0, 0, 10), white),
                             sc.quad((-5, -0.3, -3), (10, 0, 0), (0, 6, 0), chk),
                             sc.sphere((-1.6, 0.5, 0.5), 0.8, marble),
                             sc.sphere((0.2, 0.6, 1.0), 0.9, glass),
                             sc.sphere((2.0, 0.5, 0.2), 0.8, metal), lq)
    lights = sc.hittable_list(sc.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), light),
                              sc.sphere((0.2, 0.6, 1.0), 0.9, glass))
    blob = sc.serialize(world, lights)
    cam = rt.camera_new(20.0 / 12.0, 20, 16, 8, 45, (0, 2.0, 7), (0, 0.6, 0), (0, 1, 0), 0, 0,
                        (0.2, 0.3, 0.45))
    return blob, cam, {}


def _cornell_box():
    blob, cam = rt.preset_blob("cornell_box", width=20, spp=16, depth=8, aspect=20.0 / 12.0)
    return blob, cam, {}


def _cornell_smoke_crop():
    # rows 4..15 of the 20 x 20 frame
    blob, cam = rt.preset_blob("cornell_smoke", width=20, spp=16, depth=8)
    return blob, cam, dict(row_begin=4, n_rows=12)


@pytest.mark.parametrize("make", [_cornell_box, _mixed_scene, _cornell_smoke_crop])
def test_small_renders_bitwise_across_kernels_and_against_the_oracle(gpu_available, make):
    blob, cam, kw = make()
    assert cam.image_width == 20 and kw.get("n_rows", cam.image_height) == 12
    assert cam.samples_per_pixel == 16 and cam.max_depth == 8
    state, msg = G._jit_state(blob, cam)
    assert state == 1, msg  # the product render below is the scene-specialised kernel's
    acc, _, st = G._compare(blob, cam, **kw)
    assert acc.shape == (12, 20, 3) and st.samples == 20 * 12 * 16
    assert np.isfinite(acc).all() and acc.mean() > 0.0
    if make is _mixed_scene:
        mats, _ = W.flat_tables(blob)
        flagged = {bool(r[0] & W.MATF_SOLID_W) for r in mats if int(r[0]) & 0xff == W.LAMBERTIAN}
        assert flagged == {True, False}
        ops = st.op_counts()
        assert ops["metal"] > 0 and ops["dielectric"] > 0 and ops["emissive_hits"] > 0
        assert ops["noise_evals"] > 0 and ops["misses"] > 0
