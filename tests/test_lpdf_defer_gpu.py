"""The deferred light-list PDF on the GPU (rt_kernel.h trace_body DEFER, rt_jit.cpp kLpdfDefer).

The product build of a qualifying scene leaves a bounce's light-list PDF to the next world query;
the counting build, the interpreter kernel and the f64 oracle do not. test_gpu_parity._compare
requires product = counting = interpreter bit for bit, the oracle within 1e-4 per sample, equal
NaN / inf masks and equal op counts: any difference the deferral made would show there."""
import numpy as np
import pytest

import lpdf_scenes as S
import surely_rt as rt
import test_gpu_parity as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("depth", [3, 2])
def test_cornell_box_shallow_depths(gpu_available, depth):
    """Depth 3: a deferred bounce, another, then the last bounce's immediate path; depth 2: every
    first bounce deferred, every second immediate (50, 1 and 0 are test_turnover_gpu.py's)."""
    blob, cam = rt.preset_blob("cornell_box", width=40, spp=100, depth=depth, aspect=40 / 24)
    assert (cam.image_width, cam.image_height) == (40, 24)
    P._compare(blob, cam)


def test_one_quad_light_list(gpu_available):
    blob, cam = rt.preset_blob("cornell_box", variant="mixed_pdf", width=40, spp=16, depth=50,
                               aspect=40 / 24)
    P._compare(blob, cam)


@pytest.mark.parametrize("depth,sphere_light", [(10, False), (2, False), (1, False),
                                                (10, True), (1, True)])
def test_zero_pdf_under_deferral(gpu_available, depth, sphere_light):
    """_zero_pdf_scene with the low quad in the world too, so every entry matches and pdf_val = 0
    is found one iteration later (or at once, on a last bounce). The f64 oracle's NaN shares:
    0.576 / 0.575 / 0.553 at depth 10 / 2 / 1, and 0.595 / 0.527 at depth 10 / 1 with the glass
    sphere also a light entry; finite pixels exist and there is no inf."""
    blob, cam = S.zero_pdf_matched(depth, sphere_light)
    acc_g, _, _ = P._compare(blob, cam)
    assert np.isnan(acc_g).mean() > 0.2 and np.isfinite(acc_g).any()


def test_checker_floor_attenuation(gpu_available):
    """atten varies per bounce and is parked across the iteration."""
    blob, cam = S.room("checker", 32, 16)
    P._compare(blob, cam)


@pytest.mark.parametrize("flags", [rt.RT_FLAG_OVERWRITE,
                                   rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_SEMANTICS_REFERENCE])
def test_lights_and_volume(gpu_available, flags):
    """Isotropic lanes take the same finalisation; under reference semantics their s_pdf is 0."""
    blob, cam = S.room("volume", 32, 16, depth=8)
    _, _, st = P._compare(blob, cam, flags=flags)
    assert st.op_counts()["isotropic"] > 0


def test_switch_gives_the_same_image(gpu_available):
    """-DRT_LPDF_NOW (immediate evaluation in the same kernel source) against the default."""
    blob, cam = rt.preset_blob("cornell_box", width=64, spp=16)
    now = P._render_env(blob, cam, {"RT_JIT_OPTS": "-DRT_LPDF_NOW"})
    deferred = P._render_env(blob, cam, {})
    assert np.array_equal(now, deferred, equal_nan=True)
