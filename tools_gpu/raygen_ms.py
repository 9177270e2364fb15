"""Wall and kernel time of the ray generators on the device next to today's host paths, in one
process, for the preset's W x H frame:

AO frame, K directions per pixel, the pixel-centre rays of the preset's camera (rt_render_cli --ao):
  (a) host path: rt_query_rays (records), then K x (rth_ao_rays, rt_query_rays any-hit) over host
      buffers and a numpy count: what rt_render_cli --ao runs without --device-rays;
  (b) rt_ambient_occlusion_device: primaries resident on the device, sums left there.
One panorama stratum of the same frame (sqrt_spp 1):
  (a) rth_projection_rays and the upload of the rays;
  (b) rt_projection_rays_device.
Per path one warm-up, then the median (and minimum) over ROUNDS calls of the wall time (the call
to the end of its device work) and of the summed ms_kernel of its launches, and the bytes that
cross the bus per call. The device paths are timed twice: wall time from calls without stats
(asynchronous, one synchronisation at the end), kernel time from calls with stats. The baseline
is the host path of this build in this process; nothing is asserted.
Usage: python tools_gpu/raygen_ms.py SCENE WIDTH K [ROUNDS]"""
import sys
import time

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")


def pixel_centre_rays(rt, np, cam):
    W, H = cam.image_width, cam.image_height
    c, p00 = np.array(cam.center[:]), np.array(cam.pixel00_loc[:])
    du, dv = np.array(cam.pixel_delta_u[:]), np.array(cam.pixel_delta_v[:])
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    d = p00 + x.reshape(-1, 1) * du + y.reshape(-1, 1) * dv - c
    return rt.make_rays(np.broadcast_to(c, d.shape), d, pixel=np.arange(W * H, dtype=np.uint32))


def main(scene, W, K, rounds):
    import numpy as np
    import surely_rt as rt
    from hip_buf import DevBuf, hip

    host = rt.Scene(1)
    world, lights, cam = host.preset(scene, width=W, spp=1)
    blob = host.serialize(world, lights)
    H = cam.image_height
    n = W * H
    ds, gen = rt.DeviceScene(blob), rt.RayGen()
    sync = hip().hipDeviceSynchronize
    primary = pixel_centre_rays(rt, np, cam)
    seed, radius = 1, float("inf")

    def report(what, wall, kern, note):
        print(f"{scene} {W}x{H} {what:44s}: wall median {np.median(wall):9.3f} ms min "
              f"{min(wall):9.3f}; kernels median {np.median(kern):8.4f} ms min {min(kern):8.4f}; "
              f"{note}", flush=True)

    def timed(fn):
        """wall ms and the call's result, after the device has drained"""
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    # ---- AO frame (a): host generators, host-buffer queries, numpy count
    def ao_host():
        ms = 0.0
        hits, st = ds.query(primary, seed=seed, stats=True)
        ms += st.ms_kernel
        count = np.zeros(n, np.float32)
        for k in range(K):
            batch = rt.ao_rays(primary, hits, k, seed=seed, radius=radius)
            occ, st = ds.query(batch, seed=seed, occlusion=True, any_hit=True, stats=True)
            ms += st.ms_kernel
            count += occ == 0
        return ms, count

    ao_host()
    runs = [timed(ao_host) for _ in range(rounds)]
    count_host = runs[-1][1][1]
    up, down = n * 80 * (1 + K), n * 80 + n * K
    report(f"AO K={K} (a) host path", [w for w, _ in runs], [r[0] for _, r in runs],
           f"{up} B up, {down} B down per frame")

    # ---- AO frame (b): the driver, everything resident
    d_prim = DevBuf((n, 20), init=primary.view(np.uint8).reshape(n, 80).view(np.float32))
    sums = DevBuf((n, 3))
    fp = rt.make_ao_frame_params(K, seed=seed, radius=radius, channels=3)
    gen.ambient_occlusion_device(ds, fp, d_prim.ptr, n, sums.ptr)
    wall = [timed(lambda: gen.ambient_occlusion_device(ds, fp, d_prim.ptr, n, sums.ptr))[0]
            for _ in range(rounds)]
    stats = [gen.ambient_occlusion_device(ds, fp, d_prim.ptr, n, sums.ptr, stats=True)
             for _ in range(rounds)]
    report(f"AO K={K} (b) rt_ambient_occlusion_device", wall, [s.ms_kernel for s in stats],
           f"0 B cross the bus; {stats[-1].out_bytes} B of sums on the device, "
           f"{stats[-1].launches} launches")
    count_dev = sums.download()[:, 0]
    surface = int((count_host > 0).sum() + 0)
    print(f"{scene} {W}x{H} AO K={K}: {int((count_dev != count_host).sum())} of {n} pixels differ "
          f"between the two paths (largest difference {np.abs(count_dev - count_host).max():.0f}); "
          f"{surface} pixels with an open direction, mean unoccluded share "
          f"{count_host.sum() / max(1, K * surface):.3f} over them", flush=True)
    sums.free()

    # ---- one panorama stratum (a): the host generator and the upload
    view = dict(origin=tuple(cam.center), up=tuple(-v for v in cam.pixel_delta_v),
                forward=tuple(cam.pixel00_loc[k] + 0.5 * (W - 1) * cam.pixel_delta_u[k] +
                              0.5 * (H - 1) * cam.pixel_delta_v[k] - cam.center[k] for k in range(3)))
    d_rays = DevBuf((n, 20))

    def pano_host():
        rays = rt.projection_rays("panorama", seed=seed, width=W, height=H, sqrt_spp=1, **view)
        d_rays.upload(rays.view(np.uint8).reshape(n, 80).view(np.float32))

    pano_host()
    wall = [timed(pano_host)[0] for _ in range(rounds)]
    report("panorama stratum (a) rth_projection_rays + upload", wall, [0.0] * rounds,
           f"{n * 80} B up per stratum")
    want = d_rays.download().view(np.uint8).reshape(n, 80).copy()

    # ---- (b): the device generator into the same buffer
    pr = rt.make_projection("panorama", width=W, height=H, sqrt_spp=1, **view)
    gen.projection_rays_device(pr, d_rays.ptr, seed=seed)
    wall = [timed(lambda: gen.projection_rays_device(pr, d_rays.ptr, seed=seed))[0]
            for _ in range(rounds)]
    stats = [gen.projection_rays_device(pr, d_rays.ptr, seed=seed, stats=True)
             for _ in range(rounds)]
    report("panorama stratum (b) rt_projection_rays_device", wall, [s.ms_kernel for s in stats],
           f"0 B cross the bus; {stats[-1].out_bytes} B of rays on the device")
    got = d_rays.download().view(np.uint8).reshape(n, 80)
    a, b = want.view(rt.RAY_DTYPE).ravel(), got.view(rt.RAY_DTYPE).ravel()
    print(f"{scene} {W}x{H} panorama: max |dir_dev - dir_host| = {np.abs(a['dir'] - b['dir']).max():.3e}, "
          f"{int((want != got).any(1).sum())} of {n} records differ in some bit", flush=True)
    for buf in (d_prim, d_rays):
        buf.free()
    gen.close()
    ds.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 7)
