"""The C-ABI framebuffer gather (include/rt_gather.h, librtgather.so): RCCL over xGMI for one
process per GPU, the C counterpart of bench.py's torch.distributed gather.

On the one-GPU test box: the de-interleave of three ranks' cyclic shares (rendered one after the
other with rt_render_device) must give the single-render frame bit for bit, and an RCCL
communicator of one rank must gather a frame through ncclGather unchanged."""
import os

import numpy as np
import pytest

import surely_rt as rt

pytestmark = pytest.mark.gpu


def test_deinterleave_of_three_shares_is_the_frame(gpu_available):
    from hip_buf import DevBuf
    from surely_rt.parallel import cyclic_rows, gather_lib, max_rows

    blob, cam = rt.preset_blob("cornell_box", width=61, spp=16)
    H, W, N = cam.image_height, cam.image_width, 3
    ds = rt.DeviceScene(blob)
    full, _ = ds.render(cam, rt.make_opts(cam, seed=5))
    m = max_rows(H, N)
    gathered = DevBuf((N, m, W, 3))
    frame = DevBuf((H, W, 3))
    try:
        for r in range(N):
            b, s, n = cyclic_rows(H, r, N)
            part, _ = ds.render(cam, rt.make_opts(cam, seed=5, row_begin=b, row_step=s, n_rows=n))
            host = gathered.download()
            host[r, :n] = part
            gathered.upload(host)
        assert gather_lib().rt_gather_deinterleave(gathered.ptr, N, W, H, frame.ptr, None) == 0
        assert np.array_equal(frame.download(), full)
    finally:
        gathered.free()
        frame.free()
        ds.close()


@pytest.mark.timeout(180)
def test_rccl_gather_of_one_rank(gpu_available):
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    from hip_buf import DevBuf
    from surely_rt.parallel import RcclFrameGather

    blob, cam = rt.preset_blob("cornell_box", width=48, spp=9)
    H, W = cam.image_height, cam.image_width
    ds = rt.DeviceScene(blob)
    local = DevBuf((H, W, 3))
    scratch = DevBuf((H, W, 3))
    frame = DevBuf((H, W, 3))
    comm = RcclFrameGather(RcclFrameGather.unique_id(), world=1, rank=0, device=0)
    try:
        ds.render_device(cam, rt.make_opts(cam, seed=2), local.ptr)
        comm.gather(local.ptr, W, H, scratch.ptr, frame.ptr)
        ref, _ = ds.render(cam, rt.make_opts(cam, seed=2))
        assert np.array_equal(frame.download(), ref)
    finally:
        comm.close()
        for b in (local, scratch, frame):
            b.free()
        ds.close()


# rt_gather_deinterleave is a pure permutation: frame[y] = gathered[y % world, y // world]. Synthetic
# bit patterns (NaN payloads, +-inf, -0.0, subnormals among them) compared as uint32; the padding
# rows past a rank's share hold a sentinel that must not reach the frame, and the frame lies
# between guard words that must not change. The shapes: one row of one rank; more ranks than rows;
# ragged shares; an even and an uneven deal over 8 ranks; rows wide enough for a second pass of the
# kernel's x stride loop (3 W > 64 * 256); and heights past the 65535 blocks of the grid's y extent,
# where the kernel's row loop iterates (one and two extra rows per block).
SENTINEL, GUARD, N_GUARD = 0xDEADBEEF, 0xA5A5A5A5, 64
PERM_SHAPES = [(1, 1, 1), (5, 1, 2), (3, 7, 61), (8, 3, 8), (8, 3, 9), (3, 5500, 5),
               (4, 1, 65536), (3, 1, 70001)]


@pytest.mark.parametrize("world,W,H", PERM_SHAPES)
def test_deinterleave_is_the_row_permutation(gpu_available, world, W, H):
    from hip_buf import DevBuf, Stream
    from surely_rt.parallel import gather_lib

    lib = gather_lib()
    m = lib.rt_gather_max_rows(H, world)
    assert m == -(-H // world)
    rng = np.random.default_rng(1000 * world + H)
    g = rng.integers(0, 2**32, (world, m, W * 3), dtype=np.uint64).astype(np.uint32)
    g.ravel()[:8] = [0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001,
                     0x807FFFFF, 0x7F812345][:min(8, g.size)]
    g[(g == SENTINEL) | (g == GUARD)] ^= 1
    y = np.arange(H)
    want = g[y % world, y // world]
    for r in range(world):
        g[r, lib.rt_gather_rows(H, world, r):] = SENTINEL
    assert (g == SENTINEL).sum() == (world * m - H) * W * 3
    n = H * W * 3
    gathered = DevBuf(g.shape, init=g.view(np.float32))
    framed = DevBuf((N_GUARD + n + N_GUARD,),
                    init=np.full(N_GUARD + n + N_GUARD, GUARD, np.uint32).view(np.float32))
    stream = Stream() if (world, W, H) == (3, 7, 61) else None  # one case on a non-null stream
    try:
        assert lib.rt_gather_deinterleave(gathered.ptr, world, W, H, framed.ptr + 4 * N_GUARD,
                                          stream.handle if stream else None) == 0
        if stream:
            stream.sync()
        got = framed.download().view(np.uint32)
        assert (got[:N_GUARD] == GUARD).all() and (got[N_GUARD + n:] == GUARD).all()
        frame = got[N_GUARD:N_GUARD + n].reshape(H, W * 3)
        assert not (frame == SENTINEL).any() and not (frame == GUARD).any()
        bad = np.unique(np.argwhere(frame != want)[:, 0])
        assert bad.size == 0, f"{bad.size} rows differ, first {bad[:8].tolist()}"
        assert np.array_equal(gathered.download().view(np.uint32), g)  # the source is only read
    finally:
        gathered.free()
        framed.free()
        if stream:
            stream.destroy()
