"""The first-hit AOV pass (rt_render_aov, include/rt_mi355x.h) against the CPU oracle.

Two references:
 * scenes without volumes: the oracle's per-sample hooks, oracle_camera_ray + oracle_world_hit
   (the sample's own stream forms the ray; the hook's world query seeds its own generator, so it
   is no reference for ConstantMedium draws), with materials and solid textures read from the
   blob, summed per pixel in f64 in (s_j, s_i) order and rounded once to f32;
 * volumes, BVHs, Perlin, motion blur, textures: the oracle's depth-1 render, whose frame is the
   first hit's emission (or the background) and whose op counts are the frame's material-kind
   histogram, each with the right per-sample streams.

Tolerance of every float channel: 1e-6 * max(1, |ref|) per pixel sum. The values are f64 results
rounded once to f32 (albedo and emission may pass the f32 weight type: one more rounding), so the
expected error is about 1.2e-7 relative; 1e-6 is the project's per-sample constant (C23_TOL,
test_gpu_parity.py). hits and matid are exact."""
import numpy as np
import pytest

import oracle_lib as O
import probe_lib as P
import surely_rt as rt
import variant_scenes as V
from hip_buf import DevBuf

pytestmark = pytest.mark.gpu

TOL = 1e-6
BG = (0.25, 0.5, 1.0)
F = slice(1, 11)  # the float sum channels t .. emission


def _close(got, ref):
    """(ok, max of |got - ref| / max(1, |ref|))."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    m = float(e.max()) if e.size else 0.0
    return m <= TOL, m


def _copy(cam, **kw):
    c = rt.RtCamera.from_buffer_copy(cam)
    for k, v in kw.items():
        if k == "background":
            c.background[:] = v
        else:
            setattr(c, k, v)
    return c


def _tables(blob):
    """(material kinds, material records, texture records) of the blob, 8 slots each."""
    s = blob.slots
    nt, to, nm, mo = int(s[3]), int(s[4]), int(s[5]), int(s[6])
    mats = s[mo:mo + 8 * nm].reshape(nm, 8)  # RT_MAT_SLOTS = RT_TEX_SLOTS = 8
    texs = s[to:to + 8 * nt].reshape(nt, 8)
    return mats[:, 0].astype(np.int64), mats, texs


def _solid(texs, t):
    assert int(texs[t, 0]) == 1, "the hook reference reads solid textures only"
    return texs[t, 1:4].view(np.float64)


def hook_reference(blob, cam, seed):
    """AOVs of the whole frame from the oracle's per-sample hooks (scenes without volumes and
    with solid textures). Returns (aov float32 [H, W, 12], per-kind sample counts)."""
    kinds, mats, texs = _tables(blob)
    W, H, S = cam.image_width, cam.image_height, cam.sqrt_spp
    bg = np.array(cam.background[:], np.float64)
    acc = np.zeros((H, W, 11), np.float64)
    matid = np.zeros((H, W), np.float64)
    count = {k: 0 for k in (0, 1, 2, 3, 4, 5)}  # 0 = miss
    for j in range(H):
        for i in range(W):
            a = acc[j, i]
            for s_j in range(S):
                for s_i in range(S):
                    h = O.world_hit(blob, O.camera_ray(cam, seed, i, j, s_i, s_j))
                    first = s_j == 0 and s_i == 0
                    if h is None:
                        a[8:11] += bg
                        count[0] += 1
                        if first:
                            matid[j, i] = -1
                        continue
                    m = int(h[8])
                    k = int(kinds[m])
                    count[k] += 1
                    alb = np.zeros(3)
                    em = np.zeros(3)
                    if k in (1, 5):
                        alb = _solid(texs, int(mats[m, 1]))
                    elif k == 2:
                        alb = mats[m, 1:4].view(np.float64)
                    elif k == 3:
                        alb = mats[m, 2:5].view(np.float64)
                    elif k == 4 and h[7] != 0.0:
                        em = _solid(texs, int(mats[m, 1]))
                    a[0] += 1.0
                    a[1] += h[0]
                    a[2:5] += h[4:7]
                    a[5:8] += alb
                    a[8:11] += em
                    if first:
                        matid[j, i] = m
    out = np.zeros((H, W, rt.AOV_CHANNELS), np.float32)
    out[..., :11] = acc
    out[..., 11] = matid
    return out, count


def _check_all_channels(got, ref, what):
    assert np.array_equal(got[..., 0], ref[..., 0]), f"{what}: hits differ"
    assert np.array_equal(got[..., 11], ref[..., 11]), f"{what}: matid differs"
    ok, m = _close(got[..., F], ref[..., F])
    print(f"{what}: max |d| / max(1, |ref|) over channels 1-10 = {m:.3e}")
    assert ok, (what, m)


@pytest.fixture(scope="module")
def cornell(gpu_available):
    blob, cam = rt.preset_blob("cornell_box", width=16, spp=4)
    ds = rt.DeviceScene(blob)
    yield blob, cam, ds
    ds.close()


# ---------------------------------------------------------------- 1. Cornell, all channels
def test_cornell_all_channels_against_the_hooks(cornell):
    blob, cam, ds = cornell
    ref, count = hook_reference(blob, cam, 1)
    # the oracle's frame: 1024 samples of every kind the scene has, and pixels that mix normals
    assert sum(count.values()) == 1024 and count[0] == 94 and count[1] == 875
    assert count[3] == 51 and count[4] == 4
    got, st = ds.render_aov(cam, rt.make_opts(cam, seed=1))
    _check_all_channels(got, ref, "cornell_box 16x16x4")
    assert st.samples == 1024 and st.launches == 1 and st.out_bytes == got.nbytes
    assert not any(st.ops[:]) and st.ms_kernel > 0.0


# ---------------------------------------------------------------- 2. thin lens, ragged tiles
@pytest.mark.parametrize("width,aspect", [(16, 1.0), (13, 13 / 11), (1, 1.0)])
def test_thin_lens_and_ragged_tiles(cornell, width, aspect):
    blob, _, ds = cornell
    cam = rt.camera_new(aspect, width, 4, 50, 40, (278, 278, -800), (278, 278, 0), (0, 1, 0),
                        2.0, 800.0, (0, 0, 0))
    assert cam.sqrt_spp == 2 and cam.defocus_angle > 0
    if width == 13:
        assert cam.image_height == 11  # ragged on both edges
    ref, _ = hook_reference(blob, cam, 1)
    got, _ = ds.render_aov(cam, rt.make_opts(cam, seed=1))
    _check_all_channels(got, ref, f"thin lens {width}x{cam.image_height}x4")


# ---------------------------------------------------------------- 3. depth-1 oracle render
NESTED_BVH = (1, 1, 1, 0, 1, 1, 2)  # the row "nested volumes, BVH"
UNSTAGED_FLAT = (1, 1, 0, 0, 1, 1, 0)  # the rt_variant.h row "vol, tex, no BVH, tables in global memory"


def _depth1_scene(name):
    """A preset at 24 x 24 x 1, or one of two scenes of variant_scenes.py with a camera of their
    own: the flat scene with a medium and a noise texture whose tables the LDS plan does not stage
    (the AOV pass's "no BVH, unstaged" instance), and the nest of media beside a BVH (its "BVH,
    nested volumes" instance)."""
    if name not in ("unstaged_flat", "nested_bvh"):
        return rt.preset_blob(name, width=24, spp=1, aspect=1.0)
    if name == "nested_bvh":  # the AOV pass's "BVH, nested volumes" instance
        blob = V.build(NESTED_BVH)
        h = P.scene_header(blob)
        assert h["has_bvh"] == 1 and h["nested_volumes"] == 1
    else:
        blob = V.build(UNSTAGED_FLAT)
        assert V.stage_scene(blob, 1)[0] == 0 and P.scene_header(blob)["has_bvh"] == 0
    # wide enough for the lamp: every material kind is a first hit somewhere
    cam = rt.camera_new(1.0, 24, 1, 6, 45.0, (0.3, 2.0, 9.0), (0.0, 1.6, 0.0), (0, 1, 0), 0, 0, BG)
    return blob, cam


@pytest.mark.parametrize("name", ["cornell_smoke", "final_scene", "unstaged_flat", "nested_bvh"])
def test_volumes_bvh_perlin_motion_against_depth1_oracle(gpu_available, name):
    blob, cam0 = _depth1_scene(name)
    cam = _copy(cam0, background=BG)
    cam1 = _copy(cam, max_depth=1)
    W, H = cam.image_width, cam.image_height
    assert (W, H, cam.sqrt_spp) == (24, 24, 1)
    opts = rt.make_opts(cam, seed=1)
    frame, ops = O.render(blob, cam1, opts, precision=64)
    per_kind = ("lambertian", "metal", "dielectric", "emissive_hits", "isotropic")
    # at depth 1 every sample ends as exactly one of these; a future oracle change must not turn
    # the histogram check vacuous
    assert ops["samples"] == W * H == ops["misses"] + sum(ops[k] for k in per_kind)
    ds = rt.DeviceScene(blob)
    try:
        aov, _ = ds.render_aov(cam, opts)
        beauty1, _ = ds.render(cam1, opts)
    finally:
        ds.close()
    kinds, _, _ = _tables(blob)
    matid = aov[..., 11].astype(np.int64)
    assert np.array_equal(matid.astype(np.float32), aov[..., 11])
    assert matid.min() >= -1 and matid.max() < len(kinds)
    hit = matid >= 0
    hist = np.bincount(kinds[matid[hit]], minlength=6)
    got = dict(lambertian=int(hist[1]), metal=int(hist[2]), dielectric=int(hist[3]),
               emissive_hits=int(hist[4]), isotropic=int(hist[5]))
    print(name, "kinds", got, "misses", int((~hit).sum()))
    assert got == {k: ops[k] for k in per_kind}
    assert int((~hit).sum()) == ops["misses"] == W * H - int(aov[..., 0].sum())
    if name in ("cornell_smoke", "unstaged_flat", "nested_bvh"):
        assert ops["isotropic"] > 0  # the volumes are seen
    if name == "unstaged_flat":
        assert all(ops[k] > 0 for k in per_kind) and ops["noise_evals"] > 0
    ok, m = _close(aov[..., 8:11], frame)
    print(f"{name}: emission vs depth-1 oracle frame {m:.3e}")
    assert ok, m
    ok, m = _close(beauty1, aov[..., 8:11])
    print(f"{name}: depth-1 beauty vs emission {m:.3e}")
    assert ok, m


# ---------------------------------------------------------------- 4. textured albedo
def _textured_scene(light_materials):
    sc = rt.Scene(1)
    mk = (lambda t: sc.diffuse_light(tex=t)) if light_materials else (lambda t: sc.lambertian(tex=t))
    img = np.random.default_rng(7).integers(0, 256, (4, 8, 3), dtype=np.uint8)  # 8 wide, 4 high
    floor = sc.quad((-3, -1, -3), (0, 0, 6), (6, 0, 0),
                    mk(sc.checker_from_color(0.8, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    noise = sc.sphere((-1.2, 0, 0), 1.0, mk(sc.noise_texture(4)))
    image = sc.sphere((1.2, 0, 0), 1.0, mk(sc.image_texture(img)))
    light = sc.quad((-0.5, 6, -0.5), (1, 0, 0), (0, 0, 1), mk(sc.solid_color((4, 4, 4))))
    return sc.serialize(sc.hittable_list(floor, noise, image, light), sc.hittable_list(light))


def test_textured_albedo_against_emissive_twin(gpu_available):
    cam = rt.camera_new(1.0, 24, 1, 1, 40, (0, 2.5, 7), (0, 0, 0), (0, 1, 0), 0, 10, (0, 0, 0))
    opts = rt.make_opts(cam, seed=1)
    blob_a, blob_b = _textured_scene(False), _textured_scene(True)
    frame_b, ops = O.render(blob_b, cam, opts, precision=64)
    # every hit is front-facing, so B's depth-1 frame IS the texture value at every hit
    lit = frame_b.any(axis=-1)
    assert ops["samples"] == 576 and ops["emissive_hits"] == 342 == int(lit.sum())
    out = {}
    for key, blob in (("a", blob_a), ("b", blob_b)):
        ds = rt.DeviceScene(blob)
        try:
            out[key], _ = ds.render_aov(cam, opts)
        finally:
            ds.close()
    for key in out:
        assert np.array_equal(out[key][..., 0] != 0, lit), key
    ok, m = _close(out["a"][..., 5:8], frame_b)
    print(f"textured albedo vs emissive twin's oracle frame {m:.3e}")
    assert ok, m
    ok, m = _close(out["b"][..., 8:11], frame_b)
    print(f"textured emission vs oracle frame {m:.3e}")
    assert ok, m
    assert not out["a"][..., 8:11].any()  # Lambertian: no emission, black background
    assert not out["b"][..., 5:8].any()   # DiffuseLight: no albedo


# ---------------------------------------------------------------- 5. invariances
def test_repeatable_and_cyclic_rows_bitwise(cornell):
    blob, cam, ds = cornell
    one, _ = ds.render_aov(cam, rt.make_opts(cam, seed=5))
    two, _ = ds.render_aov(cam, rt.make_opts(cam, seed=5))
    assert np.array_equal(one, two)
    tiled = np.zeros_like(one)
    for r in range(3):  # the multi-GPU tiling contract: rows r, r + 3, ...
        part, _ = ds.render_aov(cam, rt.make_opts(cam, seed=5, row_begin=r, row_step=3))
        tiled[r::3] = part
    assert np.array_equal(tiled, one)


def test_reference_bvh_flag_bitwise(gpu_available):
    blob, cam = rt.preset_blob("final_scene", width=24, spp=1, aspect=1.0)
    ds = rt.DeviceScene(blob)
    try:
        a, _ = ds.render_aov(cam, rt.make_opts(cam, seed=1))
        b, _ = ds.render_aov(cam, rt.make_opts(
            cam, seed=1, flags=rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_REFERENCE_BVH))
        c, _ = ds.render_aov(cam, rt.make_opts(
            cam, seed=1, flags=rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_INTERPRETER |
            rt.RT_FLAG_SEMANTICS_REFERENCE))
    finally:
        ds.close()
    assert a[..., 0].any() and np.array_equal(a, b) and np.array_equal(a, c)


def test_stratum_halves_accumulate(gpu_available):
    blob, cam = rt.preset_blob("cornell_box", width=16, spp=16)
    assert cam.sqrt_spp == 4
    ds = rt.DeviceScene(blob)
    try:
        one, _ = ds.render_aov(cam, rt.make_opts(cam, seed=2))
        acc, st = ds.render_aov(cam, rt.make_opts(cam, seed=2, sj_begin=0, sj_count=2))
        assert st.samples == 16 * 16 * 8
        second, _ = ds.render_aov(cam, rt.make_opts(cam, seed=2, sj_begin=2, sj_count=2))
        acc, _ = ds.render_aov(cam, rt.make_opts(cam, seed=2, flags=0, sj_begin=2, sj_count=2),
                               aov=acc)
    finally:
        ds.close()
    assert np.array_equal(acc[..., 0], one[..., 0])
    ok, m = _close(acc[..., F], one[..., F])
    print(f"two stratum halves vs one call {m:.3e}")
    assert ok, m
    assert np.array_equal(acc[..., 11], second[..., 11])  # the second call's first sample


def test_max_depth_ignored_and_no_state_left(cornell):
    blob, cam, ds = cornell
    opts = rt.make_opts(cam, seed=9)
    before, _ = ds.render(cam, opts)
    aov, _ = ds.render_aov(cam, opts)
    aov0, _ = ds.render_aov(_copy(cam, max_depth=0), opts)
    assert np.array_equal(aov, aov0)
    after, _ = ds.render(cam, opts)
    assert np.array_equal(before, after)  # the pass leaves nothing behind


# ---------------------------------------------------------------- 6. error paths
def test_error_paths_start_no_kernel(cornell):
    blob, cam, ds = cornell
    H, W, S = cam.image_height, cam.image_width, cam.sqrt_spp
    sentinel = np.full((H, W, rt.AOV_CHANNELS), 7.25, np.float32)
    buf = DevBuf(sentinel.shape, init=sentinel)
    try:
        def code(o):
            with pytest.raises(rt.RtError) as e:
                ds.render_aov_device(cam, o, buf.ptr, stats=True)
            return e.value.code

        assert code(rt.make_opts(cam, flags=rt.RT_FLAG_OVERWRITE | rt.RT_FLAG_COUNT_OPS)) == \
            rt.RT_ERR_INVALID_ARG
        assert code(rt.make_opts(cam, row_begin=H - 2, row_step=2, n_rows=2)) == \
            rt.RT_ERR_INVALID_ARG
        assert code(rt.make_opts(cam, sj_begin=1, sj_count=S)) == rt.RT_ERR_INVALID_ARG
        assert np.array_equal(buf.download(), sentinel)  # nothing ran
        # n_rows == 0: RT_OK, nothing touched
        st = ds.render_aov_device(cam, rt.make_opts(cam, n_rows=0), buf.ptr, stats=True)
        assert st.samples == 0 and st.launches == 0
        assert np.array_equal(buf.download(), sentinel)
        # the device entry point, and the scene still renders after the refusals
        ds.render_aov_device(cam, rt.make_opts(cam, seed=1), buf.ptr)
        host, _ = ds.render_aov(cam, rt.make_opts(cam, seed=1))
        assert np.array_equal(buf.download(), host)
    finally:
        buf.free()
