"""Any-hit ray queries (mode RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT, include/rt_mi355x.h) on the
GPU. The contract is one line: for every ray the any-hit byte equals the byte occlusion mode
writes for the same ray and params (1, 0, 255 for an invalid ray), with and without
RT_FLAG_REFERENCE_BVH and on scenes with ConstantMedium records. Every comparison here is
therefore bit for bit; there is no tolerance.

Rays and references are the ones tests/test_query_gpu.py and tests/test_scene_functions_gpu.py
already build (_camera_set, CAMERA_SCENES, RANDOM_SETS, _world_reference: the same (name, seed)
pairs, so the cached references are shared)."""
import math

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt
from hip_buf import DevBuf, Stream
from test_device_primitives_gpu import INF
from test_query_gpu import CAM_SEED, CAMERA_SCENES, RANDOM_SETS, _camera_set, _rays, _seed
from test_scene_functions_gpu import _keys, _mats, _oracle_world, _world_reference, _world_scene

pytestmark = pytest.mark.gpu


def _both(ds, rays, seed, flags=0):
    """(any-hit bytes, occlusion bytes) of one scene handle."""
    return (ds.query(rays, seed=seed, flags=flags, occlusion=True, any_hit=True),
            ds.query(rays, seed=seed, flags=flags, occlusion=True))


# ---------------------------------------------------------------- 1. every instance
@pytest.mark.parametrize("name", CAMERA_SCENES)
def test_every_any_hit_instance(gpu_available, name):
    blob, rays, ora = _camera_set(name)
    assert len(rays) == 576
    ds = rt.DeviceScene(blob)
    try:
        got, occ = _both(ds, rays, CAM_SEED)
        got_r, occ_r = _both(ds, rays, CAM_SEED, rt.RT_FLAG_REFERENCE_BVH)
    finally:
        ds.close()
    want = (ora[:, 0] > 0).astype(np.uint8)
    print(f"any-hit[{name}]: {int(want.sum())} hits of {len(want)}")
    assert 50 < want.sum() <= len(want)
    if name == "final_scene":  # its camera sees past the scene
        assert want.sum() < len(want)
    for what, a in (("any", got), ("occlusion", occ), ("any, reference BVH", got_r),
                    ("occlusion, reference BVH", occ_r)):
        bad = np.nonzero(a != want)[0]
        assert len(bad) == 0, (name, what, bad[:8], a[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------- 2. per-ray intervals
@pytest.mark.parametrize("name,seed", RANDOM_SETS, ids=[n for n, _ in RANDOM_SETS])
def test_per_ray_intervals(gpu_available, name, seed):
    blob, _ = _world_scene(name)
    rays9, keys, exact, _, _, share, hits = _world_reference(name, seed)
    rays = _rays(rays9, keys)
    assert len(rays) == 1024
    ds = rt.DeviceScene(blob)
    try:
        got, occ = _both(ds, rays, _seed(keys))
        got_r, _ = _both(ds, rays, _seed(keys), rt.RT_FLAG_REFERENCE_BVH)
    finally:
        ds.close()
    assert np.array_equal(got, occ), (name, np.nonzero(got != occ)[0][:8])
    assert np.array_equal(got_r, occ), (name, np.nonzero(got_r != occ)[0][:8])
    clear = np.array([not guard for _, guard, _ in exact])
    want = np.array([h is not None for h, _, _ in exact], np.uint8)
    bad = np.nonzero((got != want) & clear)[0]
    print(f"any-hit[{name}]: {len(rays)} rays, {int(got.sum())} accepted, {hits} exact hits, "
          f"guard band leaves out {100 * share:.2f} %")
    assert len(bad) == 0, (name, bad[:8])
    assert 0 < got.sum() < len(got)


# ---------------------------------------------------------------- 3. interval ends
def _ends_scene(bvh):
    """The dyadic five-object scene of test_query_gpu.test_interval_ends, as a list or with the
    same objects under one BVH node."""
    sc = rt.Scene(2)
    m = _mats(sc, 5)
    objs = [sc.quad((-1, -1, 3), (2, 0, 0), (0, 2, 0), m[0]),      # z = 3, [-1, 1]^2
            sc.quad((0, 0, 3), (2, 0, 0), (0, 2, 0), m[1]),        # the same plane, [0, 2]^2
            sc.sphere((0.5, 0.5, 4), 1.0, m[2]),                   # z in [3, 5] at (0.5, 0.5)
            sc.sphere((-6, 0, 5), 1.0, m[3]),                      # z in [4, 6] at (-6, 0)
            sc.quad((-7, -1, 4), (2, 0, 0), (0, 2, 0), m[4])]      # z = 4 over it
    world = sc.hittable_list(*objs)
    if bvh:
        world = sc.hittable_list(sc.create_bvh(world))
    return sc.serialize(world, None)


def _ends_cases():
    up, dn = (lambda x: math.nextafter(x, INF)), (lambda x: math.nextafter(x, -INF))
    z, nz = (0, 0, 1), (0, 0, -1)
    a, b, s = (-0.5, -0.5, 0), (-6, 0, 0), (-6, 0, 8)
    # o, d, tmin, tmax -> accepted; a pair where the list and the BVH differ: an Aabb rejects a
    # degenerate interval (Aabb::hit leaves when tmax <= tmin, object.rs:364), a quad's own test takes it
    return [
        # quad 0 alone at t = 3: inclusive at both ends, one ulp either side
        (a, z, 1e-4, INF, 1), (a, z, 3.0, INF, 1), (a, z, up(3.0), INF, 0), (a, z, dn(3.0), INF, 1),
        (a, z, 1e-4, 3.0, 1), (a, z, 1e-4, dn(3.0), 0), (a, z, 1e-4, up(3.0), 1),
        (a, z, 3.0, 3.0, (1, 0)), (a, z, up(3.0), 3.0, 0), (a, z, 3.0, dn(3.0), 0),
        ((-1.0, 0.0, 0), z, 1e-4, INF, 1), ((dn(-1.0), 0.0, 0), z, 1e-4, INF, 0),
        # from z = 0 at (-6, 0): sphere 3's roots 4 and 6, quad 4 at 4
        (b, z, 1e-4, INF, 1), (b, z, 4.0, 4.0, (1, 0)),         # the quad: inclusive
        (b, z, up(4.0), INF, 1),                                # the sphere's far root 6
        (b, z, up(4.0), 6.0, 0),                                # ... == tmax: strict
        (b, z, up(4.0), up(6.0), 1), (b, z, up(4.0), dn(6.0), 0),
        (b, z, 6.0, INF, 0), (b, z, dn(6.0), INF, 1), (b, z, up(6.0), INF, 0),
        (b, z, 1e-4, dn(4.0), 0),
        # from z = 8 downwards: the sphere's roots 2 and 4, the quad at 4
        (s, nz, 1e-4, 2.0, 0),                                  # near root == tmax: strict
        (s, nz, 1e-4, up(2.0), 1), (s, nz, 1e-4, dn(2.0), 0),
        (s, nz, 2.0, 3.0, 0),                                   # near root == tmin: strict
        (s, nz, dn(2.0), 3.0, 1), (s, nz, up(2.0), 3.0, 0),
        (s, nz, up(2.0), 4.0, 1),                               # far root strict, the quad inclusive
        (s, nz, up(2.0), dn(4.0), 0), (s, nz, 4.0, INF, 1), (s, nz, up(4.0), INF, 0),
        # sphere 2 and both quads at (0.5, 0.5): d = (0, 0, -2) from z = 8: roots 1.5, 2.5, quads 2.5
        ((0.5, 0.5, 8), (0, 0, -2), 1e-4, 1.5, 0), ((0.5, 0.5, 8), (0, 0, -2), 1e-4, up(1.5), 1),
        ((0.5, 0.5, 8), (0, 0, -2), 1.5, dn(2.5), 0), ((0.5, 0.5, 8), (0, 0, -2), 1.5, 2.5, 1),
        ((0.5, 0.5, 8), (0, 0, -2), up(2.5), INF, 0),
        # an empty interval accepts nothing
        (a, z, 4.0, 2.0, 0), (b, z, 7.0, 1.0, 0),
    ]


@pytest.mark.parametrize("bvh", [False, True], ids=["list", "bvh"])
def test_interval_ends(gpu_available, bvh):
    blob = _ends_scene(bvh)
    cases = _ends_cases()
    recs = np.array([list(o) + list(d) + [0.0, lo, hi] for o, d, lo, hi, _ in cases], float)
    keys = _keys(len(cases))
    want = np.array([w[bvh] if isinstance(w, tuple) else w for *_, w in cases], np.uint8)
    ora = _oracle_world(blob, recs, keys)
    assert np.array_equal(ora[:, 0].astype(np.uint8), want), np.nonzero(ora[:, 0] != want)[0]
    ds = rt.DeviceScene(blob)
    try:
        got, occ = _both(ds, _rays(recs, keys), _seed(keys))
        got_r, occ_r = _both(ds, _rays(recs, keys), _seed(keys), rt.RT_FLAG_REFERENCE_BVH)
    finally:
        ds.close()
    for what, a in (("any", got), ("occlusion", occ), ("any, reference BVH", got_r),
                    ("occlusion, reference BVH", occ_r)):
        bad = np.nonzero(a != want)[0]
        assert len(bad) == 0, (what, [(cases[k], int(a[k])) for k in bad[:6]])


# ---------------------------------------------------------------- 4. waves of mixed fate
def _mixed_batch(name):
    """769+ rays in whole 64-lane waves. Each of the first waves holds, interleaved, lanes that hit
    (camera rays the oracle reports as hits), lanes aimed away from the scene (from the camera,
    backwards and up: a miss after a full walk) and invalid rays; then one all-invalid wave, one
    wave whose only valid lane misses, and a last ragged piece."""
    _, rays, ora = _camera_set(name)
    hit = rays[ora[:, 0] > 0]
    away = rays.copy()
    away["dir"] = -away["dir"]
    away["dir"][:, 1] = np.abs(away["dir"][:, 1]) + 0.5 * np.abs(away["dir"][:, 2])
    # final_scene's fog fills a sphere of radius 5000 about everything: of the rays that leave the
    # scene, those whose free-flight draw ends inside it are hits; the oracle says which miss
    r7 = np.concatenate([away["origin"], away["dir"], away["time"][:, None]], 1)
    keys = np.stack([np.full(len(away), CAM_SEED), away["pixel"], away["sample"]], 1).astype(np.uint64)
    away = away[O.world_hit_batch(_camera_set(name)[0], r7, keys, 1e-4, INF)[:, 0] == 0]
    assert len(away) > 300
    bad = rays.copy()
    bad["dir"][0::3] = 0.0
    bad["origin"][1::3, 0] = np.nan
    bad["tmax"][2::3] = np.nan
    kind = np.zeros(13 * 64, np.uint8)  # 0 hit, 1 away, 2 invalid
    lane = np.arange(64)
    for w in range(11):
        kind[64 * w:64 * w + 64] = (lane * (w + 3) // 5 + w) % 3 if w else lane % 3
    kind[64 * 3:64 * 3 + 64] = np.where(lane == 17, 1, 0)     # one missing lane holds the wave
    kind[64 * 4:64 * 4 + 64] = np.where(lane % 8 == 0, 2, 0)  # hits and invalid rays only
    kind[64 * 11:64 * 12] = 2                                  # an all-invalid wave
    kind[64 * 12:64 * 13] = np.where(lane == 40, 1, 2)         # its only valid lane misses
    idx = np.arange(len(kind))
    batch = hit[idx % len(hit)].copy()
    batch[kind == 1] = away[idx[kind == 1] % len(away)]
    batch[kind == 2] = bad[idx[kind == 2] % len(bad)]
    return batch, kind


@pytest.mark.parametrize("name", ["final_scene", "cornell_smoke"])
def test_waves_of_mixed_fate(gpu_available, name):
    blob = _camera_set(name)[0]
    batch, kind = _mixed_batch(name)
    assert len(batch) >= 769
    perm = np.random.default_rng(5).permutation(len(batch))
    ds = rt.DeviceScene(blob)
    try:
        whole, occ = _both(ds, batch, CAM_SEED)
        parts = {n: _both(ds, batch[:n], CAM_SEED) for n in (1, 63, 64, 65, 767, 769)}
        shuffled = ds.query(batch[perm], seed=CAM_SEED, occlusion=True, any_hit=True)
        ref_order, _ = _both(ds, batch, CAM_SEED, rt.RT_FLAG_REFERENCE_BVH)
    finally:
        ds.close()
    # the batch is what it claims to be: hit lanes 1, lanes aimed away 0, invalid rays 255
    assert np.array_equal(occ, np.array([1, 0, 255], np.uint8)[kind]), np.nonzero(
        occ != np.array([1, 0, 255], np.uint8)[kind])[0][:8]
    assert np.array_equal(whole, occ), np.nonzero(whole != occ)[0][:8]
    assert np.array_equal(ref_order, occ)
    for n, (a, o) in parts.items():
        assert np.array_equal(a, occ[:n]) and np.array_equal(o, occ[:n]), n
    assert np.array_equal(shuffled, whole[perm])


# ---------------------------------------------------------------- 5. more rays than the device holds
def test_a_batch_larger_than_the_device(gpu_available):
    blob, rays, _ = _camera_set("final_scene")
    n = 600003
    ds = rt.DeviceScene(blob)
    try:
        small, small_occ = _both(ds, rays, CAM_SEED)
        big, st = ds.query(np.resize(rays, n), seed=CAM_SEED, occlusion=True, any_hit=True, stats=True)
    finally:
        ds.close()
    assert np.array_equal(small, small_occ) and 0 < (small == 1).sum() < len(small)
    assert np.array_equal(big, np.resize(small, n))
    assert (st.samples, st.launches, st.out_bytes) == (n, 1, n)


# ---------------------------------------------------------------- 6. stream
def test_any_hit_on_a_stream(gpu_available):
    blob, rays, _ = _camera_set("cornell_smoke")
    n = len(rays)
    ds = rt.DeviceScene(blob)
    d_in = DevBuf((n, 20), init=np.ascontiguousarray(rays).view(np.uint8).reshape(n, 80).view(np.float32))
    d_out = DevBuf((n // 4,))  # n bytes
    stream = Stream()
    try:
        want = ds.query(rays, seed=CAM_SEED, occlusion=True, any_hit=True)
        assert ds.query_device(d_in.ptr, n, d_out.ptr, seed=CAM_SEED, occlusion=True, any_hit=True,
                               stream=stream.handle) is None
        st = ds.query_device(d_in.ptr, n, d_out.ptr, seed=CAM_SEED, occlusion=True, any_hit=True,
                             stream=stream.handle, stats=True)
        stream.sync()
        assert np.array_equal(d_out.download().view(np.uint8).ravel()[:n], want)
        assert (st.samples, st.launches, st.out_bytes) == (n, 1, n)
    finally:
        stream.destroy()
        d_in.free()
        d_out.free()
        ds.close()


# ---------------------------------------------------------------- 7. ambient occlusion end to end
def test_ambient_occlusion_end_to_end(gpu_available):
    blob, cam = rt.preset_blob("cornell_box", width=16, spp=1)
    W, H = cam.image_width, cam.image_height
    assert (W, H, cam.sqrt_spp) == (16, 16, 1)
    rays7 = np.array([O.camera_ray(cam, 1, i, j, 0, 0) for j in range(H) for i in range(W)])
    primary = rt.make_rays(rays7[:, 0:3], rays7[:, 3:6], rays7[:, 6],
                           pixel=np.arange(W * H, dtype=np.uint32))
    K, radius, tmin, seed = 4, 150.0, 1e-4, 9
    ds = rt.DeviceScene(blob)
    try:
        hits = ds.query(primary, seed=seed)
        batches = [rt.ao_rays(primary, hits, k, seed=seed, radius=radius, tmin=tmin) for k in range(K)]
        res = [_both(ds, b, seed) for b in batches]
    finally:
        ds.close()
    h = hits["hit"] == 1
    assert 0 < h.sum() < W * H
    open_ = np.zeros(W * H)
    for k, (b, (got, occ)) in enumerate(zip(batches, res)):
        assert np.array_equal(got, occ), (k, np.nonzero(got != occ)[0][:8])
        assert np.all(got[~h] == 255)
        keys = np.stack([np.full(h.sum(), seed), b["pixel"][h], b["sample"][h]], 1).astype(np.uint64)
        r7 = np.concatenate([b["origin"][h], b["dir"][h], b["time"][h][:, None]], 1)
        ora = O.world_hit_batch(blob, r7, keys, tmin, radius)
        assert np.array_equal(got[h], ora[:, 0].astype(np.uint8)), (k, np.nonzero(got[h] != ora[:, 0])[0][:8])
        open_ += got == 0
    ao = open_[h] / K
    print(f"AO 16 x 16 cornell_box, K = {K}, radius {radius}: {int(h.sum())} hit pixels, "
          f"mean unoccluded {ao.mean():.3f}, fully open {int((ao == 1).sum())}, closed {int((ao == 0).sum())}")
    assert 0.0 < ao.mean() < 1.0  # a finite radius inside a closed box: some of both
