"""The output stage of a frame that lies in device memory, two ways: (a) download the f32 sums and
run rth_auto_expose and rth_write_color on the host; (b) rt_output_device on the render's stream
and download the bytes. cornell_box is rendered once into a device buffer; both paths are warmed
up, then alternated in one process, with and without auto-exposure; wall time from the host clock
around work that ends in a synchronous download, median (and minimum) over the rounds. The
device stage's ms_kernel (events around its launches) is taken in rounds of its own, and the
conversion kernel's rate is printed over the 15 B per pixel it moves (12 read, 3 written). The
exposure of both sides and the number of bytes in which the two frames differ are printed too.
Usage: python tools_gpu/output_ms.py WIDTH SPP [ASPECT [ROUNDS]]"""
import sys
import time

sys.path.insert(0, "surely-raytracing_amd")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402
import surely_rt as rt  # noqa: E402
from hip_buf import DevBuf, Stream  # noqa: E402

W, SPP = int(sys.argv[1]), int(sys.argv[2])
ASPECT = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 7

blob, cam = rt.preset_blob("cornell_box", width=W, spp=SPP, aspect=ASPECT)
H, spp = cam.image_height, cam.samples_per_pixel
n_px = W * H
ds, out, stream = rt.DeviceScene(blob), rt.Output(0), Stream()
sums_dev = DevBuf((H, W, 3))
bytes_dev = DevBuf(((n_px * 3 + 3) // 4 + 2,))
st = ds.render_device(cam, rt.make_opts(cam, seed=1), sums_dev.ptr, stream=stream.handle,
                      stats=True)
print(f"cornell_box {W}x{H} x {spp} spp: render {st.ms_kernel:.3f} ms kernel; {ROUNDS} rounds")


def host_path(auto):
    sums = sums_dev.download()
    ev = rt.auto_expose(sums, spp) if auto else None
    return rt.write_color(sums, spp, ev), ev


def device_path(auto):
    p = rt.output_params(W, H, spp, auto=auto)
    out.output_device(p, sums_dev.ptr, bytes_dev.ptr, stream=stream.handle)
    rgb = bytes_dev.download().view(np.uint8)[:n_px * 3].reshape(H, W, 3)  # synchronises
    return rgb, None


def device_kernel_ms(auto):
    p = rt.output_params(W, H, spp, auto=auto)
    return out.output_device(p, sums_dev.ptr, bytes_dev.ptr, stream=stream.handle, stats=True)


run = {(name, auto): (lambda f, a: lambda: f(a))(f, auto)
       for auto in (False, True) for name, f in (("host", host_path), ("device", device_path))}
frames = {k: f()[0] for k, f in run.items()}  # warm-up; the frames are compared below
wall = {k: [] for k in run}
for r in range(ROUNDS):
    for k, f in run.items():
        t0 = time.perf_counter()
        f()
        wall[k].append((time.perf_counter() - t0) * 1e3)
kern = {auto: [] for auto in (False, True)}
for auto in kern:
    device_kernel_ms(auto)
for r in range(ROUNDS):
    for auto in kern:
        kern[auto].append(device_kernel_ms(auto).ms_kernel)

for auto in (False, True):
    label = "with auto-exposure" if auto else "no exposure"
    h, d = wall[("host", auto)], wall[("device", auto)]
    print(f"  {label}:")
    print(f"    (a) download sums + host stage   median {np.median(h):10.3f} ms  min {min(h):10.3f} ms")
    print(f"    (b) rt_output_device + download  median {np.median(d):10.3f} ms  min {min(d):10.3f} ms"
          f"   (a) / (b) = {np.median(h) / np.median(d):.1f}")
    k = kern[auto]
    print(f"    device stage ms_kernel           median {np.median(k):10.4f} ms  min {min(k):10.4f} ms")
    differ = int((frames[("host", auto)] != frames[("device", auto)]).sum())
    print(f"    bytes that differ between (a) and (b): {differ} of {n_px * 3}")
k = float(np.median(kern[False]))
print(f"  out_write alone: {n_px * 15 / (k * 1e-3) / 1e9:.1f} GB/s over {n_px * 15 / 1e6:.2f} MB "
      f"(15 B per pixel)")
ev_host = rt.auto_expose(sums_dev.download(), spp)
ev_dev = out.output_device(rt.output_params(W, H, spp, auto=True), sums_dev.ptr, bytes_dev.ptr,
                           stream=stream.handle, want_exposure=True)
print(f"  ev host {ev_host!r}  device {ev_dev!r}  relative difference "
      f"{abs(ev_dev - ev_host) / ev_host:.3e}")
stream.destroy()
for b in (sums_dev, bytes_dev):
    b.free()
out.close()
ds.close()
