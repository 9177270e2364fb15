"""The sample turnover of the path loop (rt_kernel.h trace_body: end_sample, the pool claim, the
camera-ray block) at the small shapes that reach its corner cases. Non-BVH kernels form the first
round of a sample's stream key once per pool item (rt_rng.h rng_key_*, a per-lane LDS slot written
at the claim) and advance it by one add per sample, so every way an item starts and continues is
covered: ragged right-edge tiles, a block remainder, every lane ending in the same iteration
(depth 1), the depth cut-off, depth 0, fewer items than lanes with a drained queue, segment and
tail pools only (a cyclic row share, whose row numbers enter the pixel term), a stratum subset
(whose first row enters the sample term), the volume kernel, and the BVH kernel, which keeps the
per-sample hash.

Every case renders with the product (scene-specialised), the counting and the interpreter kernels,
which must agree bit for bit, and compares image and op counts with the f64 oracle
(test_gpu_parity._compare: |d| <= 1e-4 per sample, identical op counts)."""
import pytest

import surely_rt as rt
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu
W, H = 40, 24


def _cornell(spp, depth):
    blob, cam = rt.preset_blob("cornell_box", width=W, spp=spp, depth=max(depth, 1), aspect=W / H)
    cam.max_depth = depth
    assert (cam.image_width, cam.image_height) == (W, H)
    return blob, cam


@pytest.mark.parametrize("spp,depth", [
    (16, 50),   # ragged right-edge tiles (40 = 5 tiles of 8; 24 rows; the last pools are ragged in s_i)
    (100, 50),  # sqrt_spp 10: a full block of 8 plus a remainder of 2
    (100, 1),   # every lane ends its sample in the same iteration
    (100, 2),   # depth cut-off
    (100, 0),   # no bounce at all: the camera-ray block ends every sample
])
def test_cornell_small_frames(gpu_available, spp, depth):
    blob, cam = _cornell(spp, depth)
    acc_g, acc_o, st = _compare(blob, cam)
    assert st.samples == W * H * spp
    if depth == 0:
        assert not acc_g.any()


@pytest.mark.parametrize("width,spp", [(1, 1), (3, 4)])
def test_fewer_items_than_lanes(gpu_available, width, spp):
    """1x1 at 1 spp, 3x3 at 4 spp: most lanes never get an item and the queue is drained at once;
    the few lanes with an item finish it and the wave leaves."""
    blob, cam = rt.preset_blob("cornell_box", width=width, spp=spp, depth=50, aspect=1.0)
    assert (cam.image_width, cam.image_height) == (width, width)
    acc_g, acc_o, st = _compare(blob, cam)
    assert st.samples == width * width * spp


@pytest.mark.parametrize("rank", range(4))
def test_four_way_cyclic_row_share(gpu_available, rank):
    """One rank's rows of a 4-way cyclic share (rows rank, rank + 4, ...: 6 of 24): a launch too
    small for row pools, so segment and tail pools only."""
    blob, cam = _cornell(100, 50)
    n = len(range(rank, H, 4))
    acc_g, acc_o, st = _compare(blob, cam, row_begin=rank, row_step=4, n_rows=n)
    assert st.samples == n * W * 100


def test_stratum_subset(gpu_available):
    """Stratum rows s_j 3..6 of 10: the sample term of the split stream key starts at
    s_j * sqrt_spp + s_i with s_j from the subset."""
    blob, cam = _cornell(100, 50)
    acc_g, acc_o, st = _compare(blob, cam, sj_begin=3, sj_count=4)
    assert st.samples == W * H * 40


def test_volume_kernel(gpu_available):
    blob, cam = rt.preset_blob("cornell_smoke", width=32, spp=16, depth=10)
    assert (cam.image_width, cam.image_height) == (32, 32)
    _compare(blob, cam)


def test_bvh_kernel(gpu_available):
    """final_scene: the BVH kernel (row totals in dynamic LDS, the stream key hashed per sample)."""
    blob, cam = rt.preset_blob("final_scene", width=32, spp=16, depth=8)
    assert (cam.image_width, cam.image_height) == (32, 32)
    _compare(blob, cam)
