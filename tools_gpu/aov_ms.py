"""Device time of the first-hit AOV pass (rt_render_aov_device) next to the beauty render
(rt_render_device) of the same frame, alternated in one process after a warm-up of each; the
minimum and median ms_kernel over the rounds.
Usage: python tools_gpu/aov_ms.py [scene width spp depth rounds]"""
import sys

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402
import surely_rt as rt  # noqa: E402
from hip_buf import DevBuf  # noqa: E402

scene = sys.argv[1] if len(sys.argv) > 1 else "cornell_box"
W = int(sys.argv[2]) if len(sys.argv) > 2 else 800
SPP = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
DEPTH = int(sys.argv[4]) if len(sys.argv) > 4 else 50
ROUNDS = int(sys.argv[5]) if len(sys.argv) > 5 else 5
blob, cam = rt.preset_blob(scene, width=W, spp=SPP, depth=DEPTH)
H = cam.image_height
ds = rt.DeviceScene(blob)
beauty, aov = DevBuf((H, W, 3)), DevBuf((H, W, rt.AOV_CHANNELS))
opts = rt.make_opts(cam, seed=1)
run = {"beauty": lambda: ds.render_device(cam, opts, beauty.ptr, stats=True),
       "aov": lambda: ds.render_aov_device(cam, opts, aov.ptr, stats=True)}
for f in run.values():  # warm-up: code objects loaded, the scene's kernel compiled or fetched
    f()
ms = {k: [] for k in run}
for r in range(ROUNDS):
    for k, f in run.items():
        st = f()
        ms[k].append(st.ms_kernel)
print(f"{scene} {W}x{H} x {cam.samples_per_pixel} spp, depth {cam.max_depth}, {ROUNDS} rounds, "
      f"jit_info {ds.jit_info()[0]}")
for k, v in ms.items():
    print(f"  {k:6s} ms_kernel min {min(v):9.3f} median {np.median(v):9.3f} "
          f"Msamples/s {st.samples / min(v) / 1e3:9.1f}   all {[round(x, 3) for x in v]}")
print(f"  aov / beauty (min) {min(ms['aov']) / min(ms['beauty']):.3f}; "
      f"hit pixels {int((aov.download()[..., 0] > 0).sum())} of {W * H}")
beauty.free()
aov.free()
ds.close()
