"""Device time of the ray query (rt_query_rays_device) in record, occlusion and any-hit mode, next to the
first-hit AOV pass (rt_render_aov_device) for the same count of rays: the frame's W x H x SPP
camera rays, built on the host from the preset's camera at fixed stratum centres (no random jitter,
no defocus, time 0; the AOV pass jitters its own, so the two trace the same pixels' cones, not the
same rays), ordered as the AOV pass maps them: 8 x 8 tile by tile, a tile's samples one after
another, 64 consecutive rays per tile and sample (or, with `sample`, a whole frame per sample).
Per step: one warm-up, then the median (and minimum) ms_kernel over ROUNDS calls; Grays/s; bytes
moved over kernel time (160 B per ray in record mode, 81 B in occlusion mode) and their share of
the HBM peak (surely_rt.roofline.PEAK_HBM_GBPS).

Any-hit (RT_QUERY_ANY_HIT): step `anyhit` runs the camera rays of `occlusion`; the ray set `ao` has
its origins at those camera rays' first hits (one record query) and one cosine-distributed direction
each (surely_rt.ao_rays, every ray its own stream), once with radius = inf and once with a finite
radius of a tenth of the scene's bounding-box diagonal, each timed in occlusion and in any-hit
mode (steps ao_inf_occlusion, ao_inf_anyhit, ao_r_occlusion, ao_r_anyhit). Rays that saw no
surface are invalid rays there (byte 255); the line gives the counts of 1, 0 and 255 bytes.

Every step runs in a process of its own under its own `timeout`, chained with `&&`: a step that
fails or hangs ends the chain.
Usage: python tools_gpu/query_ms.py SCENE WIDTH SPP [ROUNDS [STEP_SECONDS [tile|sample]]]"""
import subprocess
import sys

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")

STEPS = ("record", "occlusion", "anyhit", "aov", "ao_inf_occlusion", "ao_inf_anyhit",
         "ao_r_occlusion", "ao_r_anyhit")


def camera_rays(rt, np, cam, order="tile"):
    """RAY_DTYPE [S*S * tiles * 64 clipped to the frame]. order "tile": tile, then (s_j, s_i), then
    the tile's pixels row by row, so that a tile's samples are consecutive 64-ray waves, as one
    wave of the AOV pass runs through them; "sample": (s_j, s_i) outermost, a frame per sample."""
    W, H, S = cam.image_width, cam.image_height, cam.sqrt_spp
    c, p00 = np.array(cam.center[:]), np.array(cam.pixel00_loc[:])
    du, dv = np.array(cam.pixel_delta_u[:]), np.array(cam.pixel_delta_v[:])
    ty, tx, ly, lx = np.meshgrid(np.arange((H + 7) // 8), np.arange((W + 7) // 8), np.arange(8),
                                 np.arange(8), indexing="ij")
    x, y = (tx * 8 + lx).ravel(), (ty * 8 + ly).ravel()
    keep = (x < W) & (y < H)
    x, y = x[keep], y[keep]
    parts = []
    for s_j in range(S):
        for s_i in range(S):
            px = cam.recip_sqrt_spp * (s_i + 0.5) - 0.5
            py = cam.recip_sqrt_spp * (s_j + 0.5) - 0.5
            d = p00 + np.outer(x + px, du) + np.outer(y + py, dv) - c
            parts.append(rt.make_rays(np.broadcast_to(c, d.shape), d,
                                      pixel=(y * W + x).astype(np.uint32), sample=s_j * S + s_i))
    if order == "sample":
        return np.concatenate(parts)
    assert W % 8 == 0 and H % 8 == 0, "tile order: whole 8 x 8 tiles"
    return np.stack([p.reshape(-1, 64) for p in parts], 1).reshape(-1)


def step(name, scene, W, SPP, rounds, order):
    import numpy as np
    import surely_rt as rt
    from hip_buf import DevBuf
    from surely_rt.roofline import PEAK_HBM_GBPS

    host = rt.Scene(1)
    world, lights, cam = host.preset(scene, width=W, spp=SPP)
    blob = host.serialize(world, lights)
    H = cam.image_height
    ds = rt.DeviceScene(blob)
    n = W * H * cam.samples_per_pixel
    bufs = []
    if name == "aov":
        out = DevBuf((H, W, rt.AOV_CHANNELS))
        bufs = [out]
        opts = rt.make_opts(cam, seed=1)
        run = lambda: ds.render_aov_device(cam, opts, out.ptr, stats=True)  # noqa: E731
        per_ray = None
    else:
        rays = camera_rays(rt, np, cam, order)
        assert len(rays) == n
        occ = name != "record"
        any_hit = name.endswith("anyhit")
        if name.startswith("ao_"):
            hits = ds.query(rays, seed=1)
            bb = host.bbox(world)  # x, y, z (min, max) pairs
            radius = float("inf") if name.startswith("ao_inf") else 0.1 * float(np.linalg.norm(bb[1::2] - bb[0::2]))
            rays["pixel"] = np.arange(n, dtype=np.uint32)  # every ray its own stream
            rays = rt.ao_rays(rays, hits, 0, seed=1, radius=radius)
            del hits
        d_in = DevBuf((n, 20), init=rays.view(np.uint8).reshape(n, 80).view(np.float32))
        out = DevBuf((n, 20) if not occ else ((n + 3) // 4,))
        bufs = [d_in, out]
        run = lambda: ds.query_device(d_in.ptr, n, out.ptr, seed=1, occlusion=occ, any_hit=any_hit,  # noqa: E731
                                      stats=True)
        per_ray = 81 if occ else 160
    run()
    ms = [run().ms_kernel for _ in range(rounds)]
    med = float(np.median(ms))
    what = name if name == "aov" else f"{name} ({order} order)"
    line = (f"{scene} {W}x{H} x {cam.samples_per_pixel} spp = {n} rays, {what:24s}: ms_kernel median "
            f"{med:8.4f} min {min(ms):8.4f}  {n / med / 1e6:7.3f} Grays/s")
    if per_ray:
        gbs = n * per_ray / med / 1e6
        line += f"  {gbs:7.1f} GB/s at {per_ray} B/ray = {100 * gbs / PEAK_HBM_GBPS:.1f} % of the HBM peak"
        if not occ:
            h = out.download().view(np.uint8).reshape(n, 80).view(rt.HIT_DTYPE).ravel()
            line += f"  ({int((h['hit'] == 1).sum())} hits)"
        else:
            b = out.download().view(np.uint8).ravel()[:n]
            line += f"  (bytes 1/0/255: {int((b == 1).sum())}/{int((b == 0).sum())}/{int((b == 255).sum())})"
            if name.startswith("ao_r"):
                line += f"  radius {radius:.4g}"
    print(line, flush=True)
    for b in bufs:
        b.free()
    ds.close()


if __name__ == "__main__":
    if sys.argv[1] == "--step":
        step(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]),
             sys.argv[7])
    else:
        scene, W, SPP = sys.argv[1], sys.argv[2], sys.argv[3]
        rounds = sys.argv[4] if len(sys.argv) > 4 else "7"
        limit = sys.argv[5] if len(sys.argv) > 5 else "150"
        order = sys.argv[6] if len(sys.argv) > 6 else "tile"
        chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {sys.argv[0]} --step {s} {scene} {W} "
                            f"{SPP} {rounds} {order}" for s in STEPS)
        sys.exit(subprocess.run(chain, shell=True).returncode)
