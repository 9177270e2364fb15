"""Device time of a ray render (rt_render_rays_device) next to the pinhole render it restates
(rt_render_device): the frame's W x H x SPP camera rays, made by the host generator
(rth_projection_rays, pinhole mode: the preset's camera without a lens) one frame per stratum, as
ONE batch of W * H * SPP rays at one path per ray with stream_skip = 3 and RT_RAYS_STREAM_TIME, so
both steps trace the same paths, sample for sample. The ray step also checks that: the per-ray
values summed over the strata in f64 against the frame's sums (printed as the largest difference
per sample), and bit for bit at SPP = 1. A third step, `paths`, renders W * H rays (stratum (0, 0)
of the same generator) at sqrt_paths = S, i.e. as many paths in the frame's own item shape (a
lane's item is a ray's 8 consecutive paths of a stratum row, not one path): other paths than the
frame's, the same count, and the figure that separates the ray block's cost from the cost of
one-path items (a claim, a 24-byte output value and a reduction read per path).
Per step: one warm-up, then the median (and minimum) ms_kernel over ROUNDS calls, Msamples/s; the
last line gives the ratios rays / frame and paths / frame of the medians.

Every step runs in a process of its own under its own `timeout`, chained with `&&`: a step that
fails or hangs ends the chain.
Usage: python tools_gpu/rays_ms.py SCENE WIDTH SPP [ROUNDS [STEP_SECONDS]]"""
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")

STEPS = ("frame", "rays", "paths", "ratio")
# the steps are processes of their own: the medians travel through this file to the last one
STATE = os.path.join(tempfile.gettempdir(), "rays_ms_state.json")


def load():
    try:
        return json.load(open(STATE))
    except OSError:
        return {}


def step(name, scene, W, SPP, rounds):
    import numpy as np
    import surely_rt as rt
    from hip_buf import DevBuf

    key = f"{scene} {W} {SPP}"
    state = load()
    if name == "ratio":
        f, r, q = state[key]["frame"], state[key]["rays"], state[key]["paths"]
        print(f"{scene} {W} x {SPP} spp: rays / frame = {r:.4f} / {f:.4f} ms = {r / f:.3f}; "
              f"paths / frame = {q:.4f} / {f:.4f} ms = {q / f:.3f}", flush=True)
        return
    blob, cam = rt.preset_blob(scene, width=W, spp=SPP)
    assert cam.defocus_angle <= 0.0, "the comparison needs a camera without a lens"
    H, S = cam.image_height, cam.sqrt_spp
    n = W * H * S * S
    ds = rt.DeviceScene(blob)
    frame = DevBuf((H, W, 3))
    bufs = [frame]
    opts = rt.make_opts(cam, seed=1)
    if name == "frame":
        run = lambda: ds.render_device(cam, opts, frame.ptr, stats=True)  # noqa: E731
    elif name == "paths":
        cam1 = cam.copy()
        cam1.sqrt_spp, cam1.samples_per_pixel, cam1.recip_sqrt_spp = 1, 1, 1.0
        rays = rt.projection_rays("pinhole", seed=1, cam=cam1)
        d_in = DevBuf((W * H, 20), init=rays.view(np.uint8).reshape(W * H, 80).view(np.float32))
        out = DevBuf((W * H, 3))
        bufs += [d_in, out]
        rp = rt.make_rays_params(seed=1, sqrt_paths=S, max_depth=cam.max_depth,
                                 background=cam.background[:], stream_skip=3, stream_time=True)
        run = lambda: ds.render_rays_device(d_in.ptr, W * H, out.ptr, rp, stats=True)  # noqa: E731
    else:
        ds.render_device(cam, opts, frame.ptr)
        rays = np.concatenate([rt.projection_rays("pinhole", seed=1, s_i=s_i, s_j=s_j, cam=cam)
                               for s_j in range(S) for s_i in range(S)])
        assert len(rays) == n
        d_in = DevBuf((n, 20), init=rays.view(np.uint8).reshape(n, 80).view(np.float32))
        out = DevBuf((n, 3))
        bufs += [d_in, out]
        rp = rt.make_rays_params(seed=1, sqrt_paths=1, max_depth=cam.max_depth,
                                 background=cam.background[:], stream_skip=3, stream_time=True)
        run = lambda: ds.render_rays_device(d_in.ptr, n, out.ptr, rp, stats=True)  # noqa: E731
    run()
    ms = [run().ms_kernel for _ in range(rounds)]
    med = float(np.median(ms))
    line = (f"{scene} {W}x{H} x {S * S} spp = {n} paths, {name:5s}: ms_kernel median {med:9.4f} "
            f"min {min(ms):9.4f} max {max(ms):9.4f}  {n / med / 1e3:8.1f} Msamples/s")
    if name == "rays":
        got = out.download().astype(np.float64).reshape(S * S, H, W, 3).sum(axis=0)
        want = frame.download().astype(np.float64)
        fin = np.isfinite(want) & np.isfinite(got)
        line += f"  (max |sum of rays - frame| per sample {np.abs(got - want)[fin].max() / (S * S):.3e}"
        if S == 1:
            same = np.array_equal(out.download().view(np.uint32).ravel(),
                                  frame.download().view(np.uint32).ravel())
            line += f", bit for bit: {same}"
        line += ")"
    print(line, flush=True)
    state.setdefault(key, {})[name] = med
    json.dump(state, open(STATE, "w"))
    for b in bufs:
        b.free()
    ds.close()


if __name__ == "__main__":
    if sys.argv[1] == "--step":
        step(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    else:
        scene, W, SPP = sys.argv[1], sys.argv[2], sys.argv[3]
        rounds = sys.argv[4] if len(sys.argv) > 4 else "7"
        limit = sys.argv[5] if len(sys.argv) > 5 else "150"
        chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {sys.argv[0]} --step {s} {scene} {W} "
                            f"{SPP} {rounds}" for s in STEPS)
        sys.exit(subprocess.run(chain, shell=True).returncode)
