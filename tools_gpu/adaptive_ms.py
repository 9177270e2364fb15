"""What adaptive sampling buys and what its machinery costs.

For a ladder of thresholds: the fraction of the frame's samples the driver
(rt_render_adaptive_device) traced, its kernel and wall time, and the clipped-[0,1] RMSE of its
resolved frame against the full rt_render_moments_device frame of the same seed (0 when every
tile takes every pass up to f32 accumulation order). Then the variant's overhead: a full-list,
stride-1 rt_render_tiles_device next to rt_render_moments_device for the same frame, alternated,
median and minimum ms_kernel; and the driver at threshold -1 (every pass on every tile: the tile
lists' uploads, the P launches and the per-pass synchronisations on top).
Usage: python tools_gpu/adaptive_ms.py SCENE WIDTH SPP [PASSES [ROUNDS [FLOOR]]]"""
import sys

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402
import surely_rt as rt  # noqa: E402
from hip_buf import DevBuf  # noqa: E402

scene, W, SPP = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
blob, cam = rt.preset_blob(scene, width=W, spp=SPP)
H, spp, S = cam.image_height, cam.samples_per_pixel, cam.sqrt_spp
P = int(sys.argv[4]) if len(sys.argv) > 4 and int(sys.argv[4]) > 0 else max(1, min(8, S // 2))
ROUNDS = int(sys.argv[5]) if len(sys.argv) > 5 else 3
FLOOR = float(sys.argv[6]) if len(sys.argv) > 6 else 1e-2
LADDER = (float("inf"), 0.5, 0.2, 0.1, 0.05, 0.02, 0.01, -1.0)

ds, ad = rt.DeviceScene(blob), rt.Adaptive(0)
full, full2 = DevBuf((H, W, 3)), DevBuf((H, W, 3))
acc, m2, out = DevBuf((H, W, 3)), DevBuf((H, W, 3)), DevBuf((H, W, 3))
opts = rt.make_opts(cam, seed=1)
tiles = np.arange(np.prod(rt.tile_grid(W, H)), dtype=np.uint32)
topts = rt.make_opts(cam, seed=1, sj_begin=0, sj_count=S)


def moments():
    return ds.render_moments_device(cam, opts, full.ptr, full2.ptr, stats=True)


def tile_render():
    return ds.render_tiles_device(cam, topts, tiles, 1, acc.ptr, m2.ptr, stats=True)


moments(), tile_render()  # warm-up: code objects loaded, the scene's kernels compiled or fetched
ms = {"moments": [], "tiles": []}
for _ in range(ROUNDS):
    ms["moments"].append(moments().ms_kernel)
    ms["tiles"].append(tile_render().ms_kernel)
same = np.array_equal(acc.download().view(np.uint32), full.download().view(np.uint32))
print(f"{scene} {W}x{H} x {spp} spp ({S} stratum rows), {P} passes, floor {FLOOR:g}, {ROUNDS} rounds")
for k, v in ms.items():
    print(f"  {k:8s} ms_kernel median {np.median(v):10.3f} min {min(v):10.3f}")
print(f"  full-list stride-1 tile render / moments render {np.median(ms['tiles']) / np.median(ms['moments']):.4f}"
      f" (same bits: {same})")
ref = np.clip(full.download().astype(np.float64) / spp, 0.0, 1.0)
total = W * H * spp
print("  threshold   traced   ms_kernel    ms_total   / moments   passes run   clipped RMSE")
for thr in LADDER:
    p = rt.RtAdaptiveParams()
    p.passes, p.min_passes, p.threshold, p.floor = P, 1, thr, FLOOR
    rows, per, st = ad.render_device(ds, cam, opts, p, acc.ptr, m2.ptr, out.ptr)
    img = np.clip(out.download().astype(np.float64) / spp, 0.0, 1.0)
    with np.errstate(invalid="ignore"):
        d = (img - ref)[np.isfinite(img) & np.isfinite(ref)]
    print(f"  {thr:9g}   {st.samples / total:6.3f}  {st.ms_kernel:10.3f}  {st.ms_total:10.3f}   "
          f"{st.ms_kernel / np.median(ms['moments']):8.4f}   {int((per > 0).sum()):10d}   "
          f"{np.sqrt((d * d).mean()):.6f}")
for b in (full, full2, acc, m2, out):
    b.free()
ad.close()
ds.close()
