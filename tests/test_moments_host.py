"""The variance-guided denoiser and the moments render, host side (no GPU): the Python mirror of
rt_denoise_var_params, its defaults, the argument checks that run before the handle is read or a
device is touched, and the specified filter itself (denoise_var_ref, the f64 restatement) on the
property the feature exists for: it smooths where the row totals say the pixel is noisy and keeps
what they say is converged."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import surely_rt as rt
from denoise_ref import denoise_ref
from denoise_var_ref import denoise_var_ref, moments_from_rows

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "rt_mi355x.h").read_text()


def test_var_params_struct_mirrors_the_header():
    body = re.search(r"typedef struct rt_denoise_var_params \{(.*?)\} rt_denoise_var_params;",
                     re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), re.S).group(1)
    sizes = {"int32_t": 4, "uint32_t": 4, "double": 8, "float": 4}
    c_fields, off = [], 0
    for decl in filter(None, (s.strip() for s in body.split(";"))):
        ty, name = decl.split()
        assert off % sizes[ty] == 0, f"{name}: padding before it"
        c_fields.append((name, off, sizes[ty]))
        off += sizes[ty]
    assert off == 56 == C.sizeof(rt.RtDenoiseVarParams)
    py = [(n, getattr(rt.RtDenoiseVarParams, n).offset, getattr(rt.RtDenoiseVarParams, n).size)
          for n, _ in rt.RtDenoiseVarParams._fields_]
    assert py == c_fields
    assert [(n, o) for n, o, _ in py] == [
        ("width", 0), ("height", 4), ("levels", 8), ("flags", 12), ("beauty_samples", 16),
        ("aov_samples", 24), ("beauty_rows", 32), ("_pad0", 36), ("sigma_color", 40),
        ("sigma_normal", 44), ("sigma_depth", 48), ("sigma_albedo", 52)]


def test_new_entry_points_are_declared_after_the_denoiser_block():
    """Appended at the end of the header: nothing above moved."""
    at = {n: HEADER.index(n + "(") for n in
          ("rt_denoise", "rt_render_moments_device", "rt_render_moments",
           "rt_denoise_var_default_params", "rt_denoise_var_device", "rt_denoise_var")}
    assert all(at[n] > at["rt_denoise"] for n in at if n != "rt_denoise")
    assert rt.device_lib().rt_abi_version() == 3


def test_var_default_params():
    p = rt.denoise_var_default_params(800, 600, 16.0, 4, 8.0)
    assert (p.width, p.height, p.levels, p.flags) == (800, 600, 5, rt.DENOISE_DEMODULATE)
    assert (p.beauty_samples, p.aov_samples, p.beauty_rows, p._pad0) == (16.0, 8.0, 4, 0)
    f = np.float32
    assert (p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo) == \
        (f(4.0), f(0.3), f(0.1), f(0.1))
    assert rt.denoise_var_default_params(3, 0, 4.0, 2).aov_samples == 4.0
    lib = rt.device_lib()
    out = rt.RtDenoiseVarParams()
    out.levels = 77
    for w, h, b, n, a in [(0, 4, 1.0, 2, 1.0), (4, -1, 1.0, 2, 1.0), (65536, 32768, 1.0, 2, 1.0),
                          (4, 4, 0.0, 2, 1.0), (4, 4, 1.0, 2, float("inf")), (4, 4, 1.0, 1, 1.0),
                          (4, 4, 1.0, 0, 1.0), (4, 4, 1.0, -3, 1.0)]:
        assert lib.rt_denoise_var_default_params(w, h, b, n, a, C.byref(out)) == \
            rt.RT_ERR_INVALID_ARG
        assert lib.rt_last_error()
    assert out.levels == 77  # a refusal writes nothing
    assert lib.rt_denoise_var_default_params(4, 4, 1.0, 2, 1.0, None) == rt.RT_ERR_INVALID_ARG


def test_bad_arguments_are_rejected_without_a_device():
    lib = rt.device_lib()
    sentinel = np.full((4, 4, 3), 7.25, np.float32)
    out = sentinel.copy()
    var = np.full((4, 4), 7.25, np.float32)
    beauty = np.ones((4, 4, 3), np.float32)
    m2 = np.ones((4, 4, 3), np.float32)
    aov = np.ones((4, 4, rt.AOV_CHANNELS), np.float32)
    fake = C.c_void_p(16)  # a non-null handle that must never be dereferenced
    good = rt.denoise_var_default_params(4, 4, 4.0, 2)
    bp, qp, ap, op, vp = (x.ctypes.data for x in (beauty, m2, aov, out, var))

    def both(dn, p, b, q, a, o):
        r1 = lib.rt_denoise_var(dn, p, b, q, a, o, vp, None)
        m1 = lib.rt_last_error()
        r2 = lib.rt_denoise_var_device(dn, p, b, q, a, o, vp, None, None)
        assert r1 == r2
        return r1, m1

    g = C.byref(good)
    for args in [(None, g, bp, qp, ap, op), (fake, None, bp, qp, ap, op),
                 (fake, g, None, qp, ap, op), (fake, g, bp, None, ap, op),
                 (fake, g, bp, qp, None, op), (fake, g, bp, qp, ap, None)]:
        rc, msg = both(*args)
        assert rc == rt.RT_ERR_INVALID_ARG and b"null" in msg

    def variant(**kw):
        p = rt.RtDenoiseVarParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [variant(levels=0), variant(levels=9), variant(flags=rt.DENOISE_DEMODULATE | 0x2),
           variant(flags=0x80000000), variant(sigma_normal=float("nan")),
           variant(sigma_color=float("inf")), variant(beauty_samples=0.0),
           variant(aov_samples=float("nan")), variant(width=0), variant(height=-1),
           variant(width=65536, height=32768),
           variant(beauty_rows=1), variant(beauty_rows=0), variant(beauty_rows=-2),
           variant(_pad0=1), variant(_pad0=-1)]
    for p in bad:
        rc, msg = both(fake, C.byref(p), bp, qp, ap, op)
        assert rc == rt.RT_ERR_INVALID_ARG and msg and b"null" not in msg
    # height == 0: RT_OK, nothing touched, the handle still not read
    st = rt.RtStats()
    st.samples = 5
    p0 = variant(height=0)
    assert lib.rt_denoise_var(fake, C.byref(p0), bp, qp, ap, op, vp, C.byref(st)) == rt.RT_OK
    assert st.samples == 0 and st.launches == 0
    assert lib.rt_denoise_var_device(fake, C.byref(p0), bp, qp, ap, op, vp, None, None) == rt.RT_OK
    assert lib.rt_denoise_var_device(fake, C.byref(p0), bp, qp, ap, op, None, None, None) == rt.RT_OK
    assert np.array_equal(out, sentinel) and (var == 7.25).all()


def test_moments_null_arguments_are_rejected_without_a_device():
    lib = rt.device_lib()
    cam, opts = rt.RtCamera(), rt.RtRenderOpts()
    buf = np.zeros(3, np.float32)
    fake = C.c_void_p(16)
    bp = buf.ctypes.data
    for sc, c, o, a, m in [(None, C.byref(cam), C.byref(opts), bp, bp),
                           (fake, None, C.byref(opts), bp, bp), (fake, C.byref(cam), None, bp, bp),
                           (fake, C.byref(cam), C.byref(opts), None, bp),
                           (fake, C.byref(cam), C.byref(opts), bp, None)]:
        assert lib.rt_render_moments(sc, c, o, a, m, None) == rt.RT_ERR_INVALID_ARG
        assert b"null" in lib.rt_last_error()
        assert lib.rt_render_moments_device(sc, c, o, a, m, None, None) == rt.RT_ERR_INVALID_ARG


# ---------------------------------------------------------------- the property, on the reference
LEFT = 8.0


def property_frame():
    """48x32, one surface. Left half: the constant LEFT plus strong noise (sd 0.6 per row mean, 0.3
    per pixel), as n = 4 row totals that differ, so the estimate sees the noise. Right half: a fine
    stripe texture around 0.5 of contrast 1/64 whose four row totals are identical and exact in
    f32, so Q == S^2 / n and its variance is 0. The left half's last column carries the constant
    without noise, so that the 3x3 prefilter leaves the stripes' variance at exactly 0; the two
    levels are 25 pixel standard deviations apart, so a stripe pixel's weight for a noisy one is
    exp(-|dx|^2 / (4 v)) ~ exp(-150)."""
    H, W, n, per_row = 32, 48, 4, 4.0
    B = A = n * per_row
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:H, 0:W]
    rows = np.zeros((n, H, W, 3))
    rows[:, :, :24] = LEFT * per_row
    rows[:, :, :23] += rng.normal(0.0, 0.6, (n, H, 23, 3)) * per_row
    stripe = 0.5 + (xx[:, 24:] % 2) / 64.0          # 0.5 and 0.515625: exact, and so is x4, ^2
    rows[:, :, 24:] = (stripe * per_row)[None, ..., None]
    beauty, m2 = moments_from_rows(rows)
    aov = np.zeros((H, W, rt.AOV_CHANNELS), np.float32)
    aov[..., rt.AOV_HITS] = A
    aov[..., rt.AOV_T] = (5.0 + 0.01 * yy) * A
    aov[..., rt.AOV_NORMAL + 1] = A
    aov[..., rt.AOV_ALBEDO:rt.AOV_ALBEDO + 3] = A     # albedo 1: filter space = colour
    pv = rt.denoise_var_default_params(W, H, B, n, A)
    pd = rt.denoise_default_params(W, H, B, A)
    return beauty, m2, aov, pv, pd


def property_figures(out_var, out_plain, beauty, B):
    """(change of the right half under the variance-guided filter, left-half deviation from the
    constant after / before it, change of the right half under the plain filter), as mean
    radiance."""
    x = np.asarray(beauty, np.float64) / B
    v = np.asarray(out_var, np.float64) / B
    d = np.asarray(out_plain, np.float64) / B
    keep = float(np.abs(v[:, 24:] - x[:, 24:]).max())
    before = float(np.sqrt(np.mean((x[:, :24] - LEFT) ** 2)))
    after = float(np.sqrt(np.mean((v[:, :24] - LEFT) ** 2)))
    plain = float(np.abs(d[:, 24:] - x[:, 24:]).max())
    return keep, after / before, plain


PROPERTY_BOUND = 6e-6  # tests/test_denoise_var_gpu.py's BOUND; the reference itself must do better


def test_the_specified_filter_smooths_noise_and_keeps_converged_texture():
    beauty, m2, aov, pv, pd = property_frame()
    assert np.array_equal(m2[:, 24:], beauty[:, 24:] ** 2 / np.float32(4))  # variance exactly 0
    out, var, valid = denoise_var_ref(beauty, m2, aov, pv)
    plain, _ = denoise_ref(beauty, aov, pd)
    assert valid.all()
    keep, ratio, moved = property_figures(out, plain, beauty, pv.beauty_samples)
    print(f"reference: right half moved {keep:.3e} (variance-guided) vs {moved:.3e} (plain); "
          f"left-half deviation x{ratio:.3f}")
    assert keep <= PROPERTY_BOUND
    assert ratio <= 0.5
    assert moved > 100 * PROPERTY_BOUND
    assert (var[:, 24:] <= 1e-12).all() and (var[:, :22] > 0).all()
