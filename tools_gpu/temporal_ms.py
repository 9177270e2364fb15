"""Temporal accumulation over an orbit: what the kernel costs and what it buys. FRAMES frames of
SCENE at WIDTH and SPP, the camera turned DEG degrees per frame about the vertical axis through the
centre of the world's bounding box, frame f rendered with seed 1 + f (rt_render_moments_device and
rt_render_aov_device, once; every run below reads the same frames). For each max_history of the
ladder 4, 8, 16, 32 the frames go through a fresh rt_temporal handle on device buffers, with m2,
hist_len and RT_TEMPORAL_VARIANCE_OF_MEAN. Printed:
  * the kernel's ms per frame (events around its launch; median and minimum over the frames that
    have a history) next to the bytes it must move: 72 B of input, 48 B of history read, 48 B of
    history written and 28 B of output per pixel, and the fraction of the 8 TB/s HBM peak that is;
  * the share of the last frame's pixels with L > 1;
  * the clipped RMSE (tests/denoise_ref.clipped_rmse) of the last frame against a TRUTH_SPP render
    of that camera for: raw, accumulated, accumulated + rt_denoise_var, rt_denoise_var alone.
Usage: python tools_gpu/temporal_ms.py SCENE WIDTH SPP FRAMES DEG [TRUTH_SPP]"""
import sys

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402
import surely_rt as rt  # noqa: E402
from denoise_ref import clipped_rmse  # noqa: E402
from hip_buf import DevBuf  # noqa: E402

SCENE, W, SPP, FRAMES, DEG = (sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]),
                              float(sys.argv[5]))
TRUTH_SPP = int(sys.argv[6]) if len(sys.argv) > 6 else 1024
LADDER = (4.0, 8.0, 16.0, 32.0)
BYTES_PER_PIXEL = 72 + 48 + 48 + 28

sc = rt.Scene(1)
world, lights, cam0 = sc.preset(SCENE, "", W, SPP)
_, _, truth_cam0 = rt.Scene(1).preset(SCENE, "", W, TRUTH_SPP)
box = sc.bbox(world)
pivot = [(box[0] + box[1]) / 2, (box[2] + box[3]) / 2, (box[4] + box[5]) / 2]
ds = rt.DeviceScene(sc.serialize(world, lights))
H, spp, rows = cam0.image_height, cam0.samples_per_pixel, cam0.sqrt_spp
n_px = W * H
shape = (H, W, 3)
b_dev, q_dev, a_dev = DevBuf(shape), DevBuf(shape), DevBuf((H, W, rt.AOV_CHANNELS))
ob_dev, oq_dev, len_dev = DevBuf(shape), DevBuf(shape), DevBuf((H, W))
print(f"{SCENE} {W}x{H} x {spp} spp ({rows} stratum rows), {FRAMES} frames, {DEG} degrees per "
      f"frame about {pivot}")

cams = [rt.camera_orbit_y(cam0, pivot, DEG * f) for f in range(FRAMES)]
frames = []
for f, cam in enumerate(cams):
    st = ds.render_moments_device(cam, rt.make_opts(cam, seed=1 + f), b_dev.ptr, q_dev.ptr,
                                  stats=True)
    ds.render_aov_device(cam, rt.make_opts(cam, seed=1 + f), a_dev.ptr)
    frames.append((b_dev.download(), q_dev.download(), a_dev.download()))
print(f"  render of one frame: {st.ms_kernel:.3f} ms kernel")
truth_cam = rt.camera_orbit_y(truth_cam0, pivot, DEG * (FRAMES - 1))
ds.render_device(truth_cam, rt.make_opts(truth_cam, seed=12345), b_dev.ptr)
truth = b_dev.download().astype(np.float64) / truth_cam.samples_per_pixel
print(f"  truth: {truth_cam.samples_per_pixel} spp of the last camera")

dn = rt.Denoiser(0)
dvp = rt.denoise_var_default_params(W, H, spp, rows)
last_b, last_q, last_a = frames[-1]
raw = clipped_rmse(last_b.astype(np.float64) / spp, truth)
alone = clipped_rmse(dn.denoise_var(last_b, last_q, last_a, dvp).astype(np.float64) / spp, truth)
print(f"  clipped RMSE of the last frame: raw {raw:.5f}   rt_denoise_var alone {alone:.5f}")
print("  max_history   ms/frame median (min)   GB/s    of 8 TB/s   L>1 share   "
      "accumulated   accumulated + rt_denoise_var")
for max_history in LADDER:
    t = rt.Temporal(0)
    p = rt.temporal_default_params(W, H)
    p.max_history, p.beauty_rows, p.flags = max_history, rows, rt.RT_TEMPORAL_VARIANCE_OF_MEAN
    ms = []
    for f, (b, q, a) in enumerate(frames):
        b_dev.upload(b), q_dev.upload(q), a_dev.upload(a)
        st = t.accumulate_device(p, cams[f], b_dev.ptr, a_dev.ptr, ob_dev.ptr, q_dev.ptr,
                                 oq_dev.ptr, len_dev.ptr, stats=True)
        if f:
            ms.append(st.ms_kernel)
    acc_b, acc_q, L = ob_dev.download(), oq_dev.download(), len_dev.download()
    t.close()
    acc = clipped_rmse(acc_b.astype(np.float64) / spp, truth)
    both = clipped_rmse(dn.denoise_var(acc_b, acc_q, last_a, dvp).astype(np.float64) / spp, truth)
    med, best = (float(np.median(ms)), min(ms)) if ms else (float("nan"),) * 2
    rate = n_px * BYTES_PER_PIXEL / (med * 1e-3) / 1e9
    print(f"  {max_history:11.0f}   {med:8.4f} ({best:.4f})      {rate:7.1f}  {rate / 8000:9.3f}   "
          f"{np.mean(L > 1):9.3f}   {acc:11.5f}   {both:11.5f}")
print(f"  compulsory bytes: {BYTES_PER_PIXEL} B per pixel, {n_px * BYTES_PER_PIXEL / 1e6:.2f} MB "
      f"per frame ({n_px * BYTES_PER_PIXEL / 8e12 * 1e3:.4f} ms at 8 TB/s)")
dn.close()
for x in (b_dev, q_dev, a_dev, ob_dev, oq_dev, len_dev):
    x.free()
ds.close()
