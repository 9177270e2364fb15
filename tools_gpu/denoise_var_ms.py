"""Device time and quality of the variance-guided a-trous denoiser (rt_denoise_var_device) next to
the plain one (rt_denoise_device), and of the moments render (rt_render_moments_device) next to
rt_render_device: each warmed up, then alternated in one process; the median (and minimum)
ms_kernel over the rounds. With PARENT_LIB (the device library of the parent commit, e.g. built by
tools_gpu/build_rev.sh) its rt_render_device of the same frame is alternated with them too.
With TRUTH_SPP: the clipped-[0,1] RMSE against a TRUTH_SPP render at seed 7 of the noisy frame and
of both filters at 1 .. LEVELS levels (the table of DESIGN.md §4.2c: same scene, seeds, spp and
measure), and a sigma_color sweep of the variance-guided filter over {0.5, 1, 2, 4}.
Usage: python tools_gpu/denoise_var_ms.py SCENE WIDTH SPP [LEVELS [ASPECT [TRUTH_SPP [ROUNDS
       [PARENT_LIB]]]]]"""
import ctypes as C
import sys

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402
import surely_rt as rt  # noqa: E402
from hip_buf import DevBuf  # noqa: E402

scene, W, SPP = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
LEVELS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
ASPECT = float(sys.argv[5]) if len(sys.argv) > 5 else 0.0
TRUTH = int(sys.argv[6]) if len(sys.argv) > 6 else 0
ROUNDS = int(sys.argv[7]) if len(sys.argv) > 7 else 9
PARENT = sys.argv[8] if len(sys.argv) > 8 else ""
SIGMAS = (0.5, 1.0, 2.0, 4.0)

blob, cam = rt.preset_blob(scene, width=W, spp=SPP, aspect=ASPECT)
H, spp, n_rows = cam.image_height, cam.samples_per_pixel, cam.sqrt_spp
ds, dn = rt.DeviceScene(blob), rt.Denoiser(0)
beauty, m2, aov, out = DevBuf((H, W, 3)), DevBuf((H, W, 3)), DevBuf((H, W, rt.AOV_CHANNELS)), \
    DevBuf((H, W, 3))
var = DevBuf((H, W))
scratch = DevBuf((H, W, 3))  # the timed plain renders write here: `beauty` stays the moments render's
opts = rt.make_opts(cam, seed=1)


def plain_params(levels):
    p = rt.denoise_default_params(W, H, spp)
    p.levels = levels
    return p


def var_params(levels, sigma=None):
    p = rt.denoise_var_default_params(W, H, spp, n_rows)
    p.levels = levels
    if sigma is not None:
        p.sigma_color = sigma
    return p


run = {"beauty": lambda: ds.render_device(cam, opts, scratch.ptr, stats=True),
       "moments": lambda: ds.render_moments_device(cam, opts, beauty.ptr, m2.ptr, stats=True),
       "aov": lambda: ds.render_aov_device(cam, opts, aov.ptr, stats=True)}
parent = None
if PARENT:
    plib = C.CDLL(PARENT)  # not load_device_lib: the parent has none of the new entry points
    plib.rt_last_error.restype = C.c_char_p
    plib.rt_scene_create.argtypes = [C.POINTER(rt.RtSceneBlob), C.c_int, C.POINTER(C.c_void_p)]
    plib.rt_scene_destroy.argtypes = [C.c_void_p]
    plib.rt_render_device.argtypes = [C.c_void_p, C.POINTER(rt.RtCamera),
                                      C.POINTER(rt.RtRenderOpts), C.c_void_p, C.c_void_p,
                                      C.POINTER(rt.RtStats)]
    ph = C.c_void_p()
    assert plib.rt_scene_create(blob.ref(), 0, C.byref(ph)) == rt.RT_OK
    parent = (plib, ph)

    def parent_render():
        st = rt.RtStats()
        rc = plib.rt_render_device(ph, C.byref(cam), C.byref(opts), C.c_void_p(scratch.ptr), None,
                                   C.byref(st))
        assert rc == rt.RT_OK, plib.rt_last_error()
        return st

    run["parent"] = parent_render
pl, pv = plain_params(LEVELS), var_params(LEVELS)
run["dn"] = lambda: dn.denoise_device(pl, beauty.ptr, aov.ptr, out.ptr, stats=True)
run["dn_var"] = lambda: dn.denoise_var_device(pv, beauty.ptr, m2.ptr, aov.ptr, out.ptr, 0,
                                              stats=True)
run["dn_var+v"] = lambda: dn.denoise_var_device(pv, beauty.ptr, m2.ptr, aov.ptr, out.ptr, var.ptr,
                                                stats=True)
for f in run.values():  # warm-up: code objects loaded, the scene's kernel compiled or fetched
    f()
ms = {k: [] for k in run}
for r in range(ROUNDS):
    for k, f in run.items():
        ms[k].append(f().ms_kernel)
med = {k: float(np.median(v)) for k, v in ms.items()}
print(f"{scene} {W}x{H} x {spp} spp ({n_rows} stratum rows), {LEVELS} levels, {ROUNDS} rounds")
for k, v in ms.items():
    print(f"  {k:9s} ms_kernel median {med[k]:8.4f} min {min(v):8.4f}")
print(f"  moments / beauty {med['moments'] / med['beauty']:.4f}"
      + (f", moments / parent's beauty {med['moments'] / med['parent']:.4f}, beauty / parent's "
         f"{med['beauty'] / med['parent']:.4f}" if parent else ""))
print(f"  dn_var / dn {med['dn_var'] / med['dn']:.3f}, with var_out {med['dn_var+v'] / med['dn']:.3f}; "
      f"dn_var / moments render {med['dn_var'] / med['moments']:.3f}")
if parent:
    a, b = scratch.download(), beauty.download()
    plib.rt_render_device(ph, C.byref(cam), C.byref(opts), C.c_void_p(scratch.ptr), None, None)
    print(f"  moments accum == parent's rt_render_device bits: "
          f"{np.array_equal(scratch.download().view(np.uint32), b.view(np.uint32))}")
    plib.rt_scene_destroy(ph)
if TRUTH:
    from denoise_ref import clipped_rmse  # noqa: E402

    _, cam_t = rt.preset_blob(scene, width=W, spp=TRUTH, aspect=ASPECT)
    truth, _ = ds.render(cam_t, rt.make_opts(cam_t, seed=7))
    truth = truth.astype(np.float64) / cam_t.samples_per_pixel

    def rmse():
        return clipped_rmse(out.download().astype(np.float64) / spp, truth)

    noisy = clipped_rmse(beauty.download().astype(np.float64) / spp, truth)
    print(f"  clipped RMSE against {cam_t.samples_per_pixel} spp (seed 7): noisy {noisy:.4f}")
    print("    levels   rt_denoise   rt_denoise_var  " + "  ".join(f"s={s:g}" for s in SIGMAS))
    for L in range(1, LEVELS + 1):
        dn.denoise_device(plain_params(L), beauty.ptr, aov.ptr, out.ptr)
        a = rmse()
        dn.denoise_var_device(var_params(L), beauty.ptr, m2.ptr, aov.ptr, out.ptr)
        b = rmse()
        sweep = []
        for s in SIGMAS:
            dn.denoise_var_device(var_params(L, s), beauty.ptr, m2.ptr, aov.ptr, out.ptr)
            sweep.append(rmse())
        print(f"    {L}        {a:.4f}       {b:.4f}          "
              + "  ".join(f"{x:.4f}" for x in sweep))
for b in (beauty, m2, aov, out, var, scratch):
    b.free()
dn.close()
ds.close()
