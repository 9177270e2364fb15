"""Device time of the a-trous denoiser (rt_denoise_device) next to the beauty render and the AOV
pass of the same frame: each warmed up, then alternated in one process; the median (and minimum)
ms_kernel over the rounds. The denoise is also timed at 1 .. LEVELS levels: the increments are the
cost of each further level (one dn_level<0, STEP, FINAL> launch: STEP 1 and 2 from LDS tiles, then
the direct form), and level 0's figure carries dn_prepare. The traffic floor of a level is
48 B read + 16 B written per pixel at 8 TB/s; dn_prepare (60 B read, 48 B written) is left out of it.
With TRUTH_SPP the clipped-[0,1] RMSE of the noisy and of the denoised frame against a TRUTH_SPP
render at seed 7 is printed too.
Usage: python tools_gpu/denoise_ms.py SCENE WIDTH SPP [LEVELS [ASPECT [TRUTH_SPP [ROUNDS]]]]"""
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
HBM_BPS = 8e12

blob, cam = rt.preset_blob(scene, width=W, spp=SPP, aspect=ASPECT)
H, spp = cam.image_height, cam.samples_per_pixel
ds, dn = rt.DeviceScene(blob), rt.Denoiser(0)
beauty, aov, out = DevBuf((H, W, 3)), DevBuf((H, W, rt.AOV_CHANNELS)), DevBuf((H, W, 3))
opts = rt.make_opts(cam, seed=1)


def params(levels):
    p = rt.denoise_default_params(W, H, spp)
    p.levels = levels
    return p


run = {"beauty": lambda: ds.render_device(cam, opts, beauty.ptr, stats=True),
       "aov": lambda: ds.render_aov_device(cam, opts, aov.ptr, stats=True)}
for L in range(1, LEVELS + 1):
    run[f"dn L{L}"] = (lambda p: lambda: dn.denoise_device(p, beauty.ptr, aov.ptr, out.ptr,
                                                           stats=True))(params(L))
for f in run.values():  # warm-up: code objects loaded, the scene's kernel compiled or fetched
    f()
ms = {k: [] for k in run}
for r in range(ROUNDS):
    for k, f in run.items():
        ms[k].append(f().ms_kernel)
print(f"{scene} {W}x{H} x {spp} spp, {LEVELS} levels, {ROUNDS} rounds")
for k, v in ms.items():
    print(f"  {k:6s} ms_kernel median {np.median(v):8.4f} min {min(v):8.4f}")
med = [float(np.median(ms[f"dn L{L}"])) for L in range(1, LEVELS + 1)]
floor_ms = W * H * 64 / HBM_BPS * 1e3
print("  denoise per level (median increments, level 0 with dn_prepare): "
      + " ".join(f"{a - b:.4f}" for a, b in zip(med, [0.0] + med[:-1])) + " ms")
print(f"  traffic floor {floor_ms * 1e3:.1f} us per level, {LEVELS * floor_ms * 1e3:.1f} us for "
      f"{LEVELS}; denoise / floor {med[-1] / (LEVELS * floor_ms):.2f}")
print(f"  denoise / beauty {med[-1] / np.median(ms['beauty']):.3f}, denoise / aov "
      f"{med[-1] / np.median(ms['aov']):.3f}")
if TRUTH:
    from denoise_ref import clipped_rmse  # noqa: E402

    _, cam_t = rt.preset_blob(scene, width=W, spp=TRUTH, aspect=ASPECT)
    truth, _ = ds.render(cam_t, rt.make_opts(cam_t, seed=7))
    truth = truth.astype(np.float64) / cam_t.samples_per_pixel
    noisy = clipped_rmse(beauty.download().astype(np.float64) / spp, truth)
    print(f"  clipped RMSE against {cam_t.samples_per_pixel} spp (seed 7): noisy {noisy:.4f}")
    for L in range(1, LEVELS + 1):
        dn.denoise_device(params(L), beauty.ptr, aov.ptr, out.ptr)
        den = clipped_rmse(out.download().astype(np.float64) / spp, truth)
        print(f"    {L} levels: denoised {den:.4f}, ratio {den / noisy:.3f}")
for b in (beauty, aov, out):
    b.free()
dn.close()
ds.close()
