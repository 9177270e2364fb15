"""The a-trous denoiser, host side (no GPU): the Python mirror of the header, the argument checks
that run before the handle is read or a device is touched, and the quality of the specified filter
itself (denoise_ref, the f64 restatement) on oracle renders of cornell_box."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
from denoise_ref import clipped_rmse, denoise_ref

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "rt_mi355x.h").read_text()


# ---------------------------------------------------------------- 1. the mirror
def test_python_constants_mirror_the_header():
    d = dict(re.findall(r"^#define (RT_DENOISE_\w+) ((?:0x)?[0-9a-fA-F]+)u?\b", HEADER, re.M))
    assert set(d) == {"RT_DENOISE_MAX_LEVELS", "RT_DENOISE_DEMODULATE"}
    assert rt.DENOISE_MAX_LEVELS == int(d["RT_DENOISE_MAX_LEVELS"], 0) == 8
    assert rt.DENOISE_DEMODULATE == int(d["RT_DENOISE_DEMODULATE"], 0) == 1


def test_params_struct_mirrors_the_header():
    body = re.search(r"typedef struct rt_denoise_params \{(.*?)\} rt_denoise_params;",
                     re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), re.S).group(1)
    sizes = {"int32_t": 4, "uint32_t": 4, "double": 8, "float": 4}
    c_fields, off = [], 0
    for decl in filter(None, (s.strip() for s in body.split(";"))):
        ty, name = decl.split()
        assert off % sizes[ty] == 0, f"{name}: padding before it"
        c_fields.append((name, off, sizes[ty]))
        off += sizes[ty]
    assert off == 48 == C.sizeof(rt.RtDenoiseParams)
    py = [(n, getattr(rt.RtDenoiseParams, n).offset, getattr(rt.RtDenoiseParams, n).size)
          for n, _ in rt.RtDenoiseParams._fields_]
    assert py == c_fields
    assert [n for n, _, _ in py] == ["width", "height", "levels", "flags", "beauty_samples",
                                     "aov_samples", "sigma_color", "sigma_normal", "sigma_depth",
                                     "sigma_albedo"]


def test_default_params():
    p = rt.denoise_default_params(800, 600, 16.0, 4.0)
    assert (p.width, p.height, p.levels, p.flags) == (800, 600, 5, rt.DENOISE_DEMODULATE)
    assert (p.beauty_samples, p.aov_samples) == (16.0, 4.0)
    f = np.float32
    assert (p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo) == \
        (f(4.0), f(0.3), f(0.1), f(0.1))
    assert rt.denoise_default_params(3, 0, 1.0).aov_samples == 1.0  # an empty frame is a frame
    lib = rt.device_lib()
    out = rt.RtDenoiseParams()
    out.levels = 77
    for w, h, b, a in [(0, 4, 1.0, 1.0), (-1, 4, 1.0, 1.0), (4, -1, 1.0, 1.0),
                       (65536, 32768, 1.0, 1.0), (4, 4, 0.0, 1.0), (4, 4, 1.0, -2.0),
                       (4, 4, float("nan"), 1.0), (4, 4, 1.0, float("inf"))]:
        assert lib.rt_denoise_default_params(w, h, b, a, C.byref(out)) == rt.RT_ERR_INVALID_ARG
        assert lib.rt_last_error()
    assert out.levels == 77  # a refusal writes nothing
    assert lib.rt_denoise_default_params(4, 4, 1.0, 1.0, None) == rt.RT_ERR_INVALID_ARG
    assert lib.rt_denoise_default_params(65535, 32768, 1.0, 1.0, C.byref(out)) == rt.RT_OK


# ---------------------------------------------------------------- 2. refusals without a device
def test_bad_arguments_are_rejected_without_a_device():
    lib = rt.device_lib()
    sentinel = np.full((4, 4, 3), 7.25, np.float32)
    out = sentinel.copy()
    beauty = np.ones((4, 4, 3), np.float32)
    aov = np.ones((4, 4, rt.AOV_CHANNELS), np.float32)
    fake = C.c_void_p(16)  # a non-null handle that must never be dereferenced
    good = rt.denoise_default_params(4, 4, 1.0)
    bp, ap, op = beauty.ctypes.data, aov.ctypes.data, out.ctypes.data

    def both(dn, p, b, a, o):
        r1 = lib.rt_denoise(dn, p, b, a, o, None)
        m1 = lib.rt_last_error()
        r2 = lib.rt_denoise_device(dn, p, b, a, o, None, None)
        assert r1 == r2
        return r1, m1

    for args in [(None, C.byref(good), bp, ap, op), (fake, None, bp, ap, op),
                 (fake, C.byref(good), None, ap, op), (fake, C.byref(good), bp, None, op),
                 (fake, C.byref(good), bp, ap, None)]:
        rc, msg = both(*args)
        assert rc == rt.RT_ERR_INVALID_ARG and b"null" in msg

    def variant(**kw):
        p = rt.RtDenoiseParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [variant(levels=0), variant(levels=9), variant(flags=rt.DENOISE_DEMODULATE | 0x2),
           variant(flags=0x80000000), variant(sigma_normal=float("nan")),
           variant(sigma_color=float("inf")), variant(beauty_samples=0.0),
           variant(aov_samples=float("nan")), variant(width=0), variant(height=-1),
           variant(width=65536, height=32768)]
    for p in bad:
        rc, msg = both(fake, C.byref(p), bp, ap, op)
        assert rc == rt.RT_ERR_INVALID_ARG and msg and b"null" not in msg
    # height == 0: RT_OK, nothing touched, the handle still not read
    st = rt.RtStats()
    st.samples = 5
    p0 = variant(height=0)
    assert lib.rt_denoise(fake, C.byref(p0), bp, ap, op, C.byref(st)) == rt.RT_OK
    assert st.samples == 0 and st.launches == 0
    assert lib.rt_denoise_device(fake, C.byref(p0), bp, ap, op, None, None) == rt.RT_OK
    assert np.array_equal(out, sentinel)
    assert lib.rt_denoiser_create(0, None) == rt.RT_ERR_INVALID_ARG
    lib.rt_denoiser_destroy(None)  # a no-op


# ---------------------------------------------------------------- 3. the reference on itself
def test_reference_blurs_and_stops_at_edges():
    """The f64 restatement alone: a constant frame is a fixed point, all sigmas off is the plain
    B3 blur (interior weights sum to 1), and two half-planes do not bleed."""
    H = W = 12
    aov = np.zeros((H, W, rt.AOV_CHANNELS), np.float32)
    aov[..., rt.AOV_HITS] = 2.0
    aov[..., rt.AOV_T] = 6.0
    aov[..., rt.AOV_NORMAL + 2] = 2.0
    aov[..., rt.AOV_ALBEDO:rt.AOV_ALBEDO + 3] = 1.0
    p = rt.denoise_default_params(W, H, 4.0, 2.0)
    p.levels = 2
    const = np.full((H, W, 3), 3.0, np.float32)
    out, valid = denoise_ref(const, aov, p)
    assert valid.all() and np.allclose(out, 3.0, rtol=0, atol=1e-12)
    p.flags = 0
    p.levels = 1
    p.sigma_color = p.sigma_normal = p.sigma_depth = p.sigma_albedo = 0.0
    imp = np.zeros((H, W, 3), np.float32)
    imp[6, 6] = 64.0 * 64.0
    out, _ = denoise_ref(imp, aov, p)
    k = np.array([1, 4, 6, 4, 1], np.float64) * 4  # 16 * 64 * h
    assert np.allclose(out[4:9, 4:9, 0], np.outer(k, k), rtol=0, atol=1e-9)
    assert out[..., 0].sum() == pytest.approx(64.0 * 64.0)


def oracle_aov(blob, cam, seed):
    """The AOV sums of the whole frame from the oracle's per-sample hooks (cornell_box: no volumes,
    solid textures), as test_aov_gpu.hook_reference forms them: f64 per pixel in (s_j, s_i)
    order, rounded once to f32."""
    s = blob.slots
    nt, to, nm, mo = int(s[3]), int(s[4]), int(s[5]), int(s[6])
    mats = s[mo:mo + 8 * nm].reshape(nm, 8)
    texs = s[to:to + 8 * nt].reshape(nt, 8)
    kinds = mats[:, 0].astype(np.int64)

    def solid(t):
        assert int(texs[t, 0]) == 1
        return texs[t, 1:4].view(np.float64)

    W, H, S = cam.image_width, cam.image_height, cam.sqrt_spp
    bg = np.array(cam.background[:], np.float64)
    acc = np.zeros((H, W, 11), np.float64)
    matid = np.zeros((H, W), np.float64)
    for j in range(H):
        for i in range(W):
            a = acc[j, i]
            for s_j in range(S):
                for s_i in range(S):
                    h = O.world_hit(blob, O.camera_ray(cam, seed, i, j, s_i, s_j))
                    first = s_j == 0 and s_i == 0
                    if h is None:
                        a[8:11] += bg
                        if first:
                            matid[j, i] = -1
                        continue
                    m = int(h[8])
                    k = int(kinds[m])
                    a[0] += 1.0
                    a[1] += h[0]
                    a[2:5] += h[4:7]
                    if k in (1, 5):
                        a[5:8] += solid(int(mats[m, 1]))
                    elif k == 2:
                        a[5:8] += mats[m, 1:4].view(np.float64)
                    elif k == 3:
                        a[5:8] += mats[m, 2:5].view(np.float64)
                    elif k == 4 and h[7] != 0.0:
                        a[8:11] += solid(int(mats[m, 1]))
                    if first:
                        matid[j, i] = m
    out = np.zeros((H, W, rt.AOV_CHANNELS), np.float32)
    out[..., :11] = acc
    out[..., 11] = matid
    return out


@pytest.fixture(scope="module")
def truth():
    blob, cam = rt.preset_blob("cornell_box", width=32, spp=4096)
    acc, _ = O.render(blob, cam, rt.make_opts(cam, seed=7), precision=64)
    return np.asarray(acc, np.float64) / cam.samples_per_pixel


@pytest.mark.parametrize("spp", [4, 16])
def test_the_specified_filter_denoises_cornell_box(truth, spp):
    """cornell_box 32x32, seed 1, against 4096 spp at seed 7: 3 levels, default sigmas,
    demodulation. The filter's clipped RMSE must be <= 0.75 x the noisy frame's (the numpy
    prototype of the specification gave 0.57 at 4 spp and 0.45 at 16 spp)."""
    blob, cam = rt.preset_blob("cornell_box", width=32, spp=spp)
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (32, 32, spp)
    beauty, _ = O.render(blob, cam, rt.make_opts(cam, seed=1), precision=64)
    beauty = np.asarray(beauty, np.float32)
    aov = oracle_aov(blob, cam, 1)
    p = rt.denoise_default_params(32, 32, spp)
    p.levels = 3
    out, valid = denoise_ref(beauty, aov, p)
    noisy = clipped_rmse(beauty.astype(np.float64) / spp, truth)
    den = clipped_rmse(out / spp, truth)
    print(f"cornell_box 32x32x{spp}: clipped RMSE noisy {noisy:.4f}, denoised {den:.4f}, "
          f"ratio {den / noisy:.3f}, invalid pixels {int((~valid).sum())}")
    assert den <= 0.75 * noisy
