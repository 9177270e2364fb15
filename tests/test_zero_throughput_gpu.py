"""Zero-throughput paths end at once (rt_kernel.h trace_body, ZCUT).

A path whose throughput is exactly zero in all channels, with no special value pending, gathers
0 * X = +0 from then on; the product kernels end it with radiance 0, the counting build runs it on
for the oracle's op counts and forces the same 0. Where the f64 oracle's frame is finite the rule
changes no bit (a zero or NaN pdf under such a prefix would have made the oracle's sample NaN), so
on Cornell the default render must equal the render under RT_FLAG_SEMANTICS_REFERENCE, which
keeps the reference's behaviour, bit for bit, in every kernel instance. The one deviation, 0 where
the reference returns NaN, is pinned on a scene built to have it.

Oracle figures (f64, seed 1) of the deviation scene: 1,531 of 2,304 pixels hold a NaN, and 1,727
zero-pdf bounces lie under a zero-throughput prefix."""
import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
from adaptive_cases import bits
from hip_buf import DevBuf
from test_gpu_parity import C23_TOL

pytestmark = pytest.mark.gpu

OW = rt.RT_FLAG_OVERWRITE
REF = OW | rt.RT_FLAG_SEMANTICS_REFERENCE


class Scene:
    """One device scene, its renders and the oracle's frames, each made once."""

    def __init__(self, blob, cam):
        self.blob, self.cam = blob, cam
        self.ds = rt.DeviceScene(blob)
        self._gpu, self._cpu = {}, {}

    def gpu(self, flags=OW, seed=1):
        """(frame, stats) of rt_render"""
        if (flags, seed) not in self._gpu:
            self._gpu[flags, seed] = self.ds.render(self.cam, rt.make_opts(self.cam, seed=seed,
                                                                           flags=flags))
        return self._gpu[flags, seed]

    def oracle(self, flags=OW, seed=1):
        if (flags, seed) not in self._cpu:
            self._cpu[flags, seed] = O.render(self.blob, self.cam,
                                              rt.make_opts(self.cam, seed=seed, flags=flags),
                                              precision=64)
        return self._cpu[flags, seed]

    def tiles_all(self, seed=1):
        """rt_render_tiles_device over the full tile list"""
        shape = (self.cam.image_height, self.cam.image_width, 3)
        tx, ty = rt.tile_grid(self.cam.image_width, self.cam.image_height)
        b = DevBuf(shape)
        try:
            o = rt.make_opts(self.cam, seed=seed, flags=OW, sj_count=self.cam.sqrt_spp)
            self.ds.render_tiles_device(self.cam, o, np.arange(tx * ty), 1, b.ptr, 0)
            return b.download()
        finally:
            b.free()


def same(a, b):
    """bit for bit, which includes equal NaN / inf masks"""
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def cornell(gpu_available):
    s = Scene(*rt.preset_blob("cornell_box", width=64, spp=64, depth=50))
    yield s
    s.ds.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_cornell_is_exact_in_every_kernel(cornell, seed, monkeypatch):
    c = cornell
    assert (c.cam.image_width, c.cam.image_height, c.cam.samples_per_pixel) == (64, 64, 64)
    acc_o, ops_o = c.oracle(OW, seed)
    assert np.isfinite(acc_o).all()  # the precondition: no zero or NaN pdf anywhere, S9 is exact
    prod, _ = c.gpu(OW, seed)
    assert np.isfinite(prod).all()
    ref, _ = c.gpu(REF, seed)
    assert same(prod, ref), "default vs RT_FLAG_SEMANTICS_REFERENCE"
    cnt, st = c.gpu(OW | rt.RT_FLAG_COUNT_OPS, seed)
    assert same(prod, cnt), "product vs counting build"
    assert st.op_counts() == ops_o
    interp, _ = c.gpu(OW | rt.RT_FLAG_INTERPRETER, seed)
    assert same(prod, interp), "scene-specialised vs interpreter kernel"
    assert same(prod, c.tiles_all(seed)), "plain vs tile-list render"
    # two chunks of four stratum rows: the 512 (tile, s_j) pairs are tail pairs, 6.3 MB of f64
    # values in one launch and 3.1 MB in each of two (rt_device.hip split / part_bytes)
    monkeypatch.setenv("RT_WORKSPACE_MB", "4")
    two, st2 = c.ds.render(c.cam, rt.make_opts(c.cam, seed=seed, flags=OW))
    monkeypatch.delenv("RT_WORKSPACE_MB")
    assert st2.launches == 2
    assert same(prod, two), "one launch vs two chunks"
    d = np.abs(prod.astype(np.float64) - acc_o.astype(np.float64)) / c.cam.samples_per_pixel
    print(f"seed {seed}: max |d| per sample {d.max():.3e} (bound {C23_TOL})")
    assert d.max() <= C23_TOL


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_short_paths(gpu_available, depth):
    """Depth 1: every bounce is a last bounce (the deferral's immediate path); 2 and 3: a cut falls
    on the iteration a depth cutoff also fires."""
    s = Scene(*rt.preset_blob("cornell_box", width=32, spp=16, depth=depth))
    try:
        assert s.cam.max_depth == depth and s.cam.image_width == 32
        prod, _ = s.gpu(OW)
        ref, _ = s.gpu(REF)
        assert same(prod, ref)
    finally:
        s.ds.close()


def deviation_scene():
    """A plate over a floor; the light list's first quad lies 1e-9 under the floor and is not in the
    world (an immediate-path kernel: no deferral). A direction sampled towards it from the plate's
    top points below the plate (scattering pdf 0, throughput 0) and reaches the floor, where a
    direction sampled towards it again has pdf_val = 0: the reference's sample is NaN, S9's is 0."""
    sc = rt.Scene(9)
    white = sc.lambertian((0.73, 0.73, 0.73))
    light = sc.diffuse_light((6, 6, 6))
    floor = sc.quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), white)
    plate = sc.quad((-2, 2, -2), (4, 0, 0), (0, 0, 4), white)
    top = sc.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2), light)
    walls = [sc.quad((6, -1, -6), (0, 7, 0), (0, 0, 12), light),
             sc.quad((-6, -1, -6), (0, 0, 12), (0, 7, 0), light),
             sc.quad((-6, -1, 6), (0, 7, 0), (12, 0, 0), light),
             sc.quad((-6, -1, -6), (12, 0, 0), (0, 7, 0), light)]
    world = sc.hittable_list(floor, plate, top, *walls)
    lights = sc.hittable_list(sc.quad((-1, -1e-9, -1), (2, 0, 0), (0, 0, 2), light),
                              sc.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2), light))
    blob = sc.serialize(world, lights)
    cam = rt.camera_new(1.0, 48, 16, 10, 40, (0, 5.5, 5), (0, 1.5, 0), (0, 1, 0), 0, 0, (0, 0, 0))
    return blob, cam


def test_documented_deviation(gpu_available):
    s = Scene(*deviation_scene())
    try:
        acc_o, ops_o = s.oracle()
        nan_o = np.isnan(acc_o)
        assert nan_o.any(axis=2).sum() == 1531 and acc_o.shape == (48, 48, 3)
        ref, _ = s.gpu(REF)
        assert np.array_equal(np.isnan(ref), nan_o)
        prod, _ = s.gpu(OW)
        nan_p = np.isnan(prod)
        print(f"NaN pixels: oracle {nan_o.any(axis=2).sum()}, default {nan_p.any(axis=2).sum()}")
        assert not (nan_p & ~nan_o).any() and nan_p.sum() < nan_o.sum()  # a strict subset
        fin = np.isfinite(prod) & np.isfinite(ref)
        assert np.array_equal(bits(prod)[fin], bits(ref)[fin])
        cnt, st = s.gpu(OW | rt.RT_FLAG_COUNT_OPS)
        assert same(prod, cnt)
        assert st.op_counts() == ops_o
    finally:
        s.ds.close()


def test_switch_compiles_the_rule_out(gpu_available, monkeypatch):
    """-DRT_NO_ZERO_CUT (the A/B handle, scene-specialised kernels): the deviation scene then
    renders the reference-flag frame, NaNs and all; Cornell renders what it renders by default."""
    s = Scene(*deviation_scene())
    c = Scene(*rt.preset_blob("cornell_box", width=32, spp=16, depth=50))
    try:
        ref, _ = s.gpu(REF)
        prod, _ = c.gpu(OW)
        monkeypatch.setenv("RT_JIT_OPTS", "-DRT_NO_ZERO_CUT")
        s2, c2 = Scene(s.blob, s.cam), Scene(c.blob, c.cam)
        try:
            off, _ = s2.gpu(OW)
            assert s2.ds.jit_info()[0] == 1
            assert same(off, ref)
            assert same(c2.gpu(OW)[0], prod)
        finally:
            s2.ds.close()
            c2.ds.close()
    finally:
        s.ds.close()
        c.ds.close()


def test_a_cut_lane_leaves_no_state_behind(gpu_available, monkeypatch):
    """8 x 8 at 9 spp: one tile, and with row items only (a launch this small renders none by
    itself) one wave holds the three row items of each pixel, cuts among their samples; the
    samples that follow a cut in an item are those of the render that cuts nothing."""
    s = Scene(*rt.preset_blob("cornell_box", width=8, spp=9, depth=50))
    try:
        assert rt.tile_grid(s.cam.image_width, s.cam.image_height) == (1, 1)
        acc_o, ops_o = s.oracle()
        assert np.isfinite(acc_o).all()
        prod, _ = s.gpu(OW)
        cnt, st = s.gpu(OW | rt.RT_FLAG_COUNT_OPS)
        assert same(prod, cnt) and st.op_counts() == ops_o
        monkeypatch.setenv("RT_SEG_PAIRS", "0")
        monkeypatch.setenv("RT_TAIL_PAIRS", "0")
        rows, _ = s.ds.render(s.cam, rt.make_opts(s.cam, seed=1, flags=OW))
        rows_ref, _ = s.ds.render(s.cam, rt.make_opts(s.cam, seed=1, flags=REF))
        assert same(rows, rows_ref) and same(rows, prod)
    finally:
        s.ds.close()
