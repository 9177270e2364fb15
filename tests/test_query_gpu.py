"""Ray queries (rt_query_rays, include/rt_mi355x.h) against exact arithmetic, the f64 oracle and
the AOV pass.

The references are the ones tests/test_scene_functions_gpu.py and tests/test_aov_gpu.py already
build: the seeded ray sets with their exact-arithmetic answers and guard bands (_world_reference,
the same (name, seed) pairs, so the cached reference is shared), the dyadic interval-end cases,
the oracle's per-ray hooks (oracle_world_hit for p and normal, oracle_world_hit_batch with the
device's own keys for media) and the 24 x 24 camera rays of the AOV tests' scenes.

Bounds.
  * hit, prim, material, front_face: exact (outside the guard band on the random sets; on every
    ray of the camera sets, where test_aov_gpu.py demands the same of the same walker).
  * t on the random sets: the vector-operation rule, at most twice the oracle's own worst error
    against the exact t. On the camera sets: 1e-10 relative against the oracle's t.
  * p: the residual |p - (o + t d)| with the record's own t, relative to |o| + |t d|, at most
    twice the same residual of the oracle's (t, p), floor 4 ulp.
  * normal: max |n - n_oracle| <= 1e-9; distance: relative 1e-14 against t * |d| in numpy.
  * independence, invalid rays, RT_FLAG_REFERENCE_BVH, occlusion against record mode, a beauty
    render before and after: bit for bit.
Every test prints its figures.

Measured on an MI355X: see DESIGN.md section 4.2i.
"""
import ctypes as C
import functools
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import oracle_lib as O
import probe_lib as P
import surely_rt as rt
import variant_scenes as V
from hip_buf import DevBuf, Stream
from test_aov_gpu import NESTED_BVH, TOL, UNSTAGED_FLAT, _depth1_scene
from test_device_primitives_gpu import INF, M, _rule
from test_scene_functions_gpu import (WORLD_SCENES, _keys, _mats, _oracle_world, _rel, _world_reference,
                                      _world_scene)

pytestmark = pytest.mark.gpu

NESTED_FLAT = (1, 1, 0, 0, 1, 1, 2)  # rt_variant.h: nested volumes, no BVH (the fifth instance)
ULP = 2.0 ** -52


def _rays(rays9, keys):
    """[n, 9] (o3, d3, time, tmin, tmax) and [n, 3] (seed, pixel, sample) -> RAY_DTYPE."""
    rays9 = np.asarray(rays9, np.float64).reshape(-1, 9)
    return rt.make_rays(rays9[:, 0:3], rays9[:, 3:6], rays9[:, 6], rays9[:, 7], rays9[:, 8],
                        np.asarray(keys)[:, 1].astype(np.uint32),
                        np.asarray(keys)[:, 2].astype(np.uint32))


def _seed(keys):
    s = set(int(k) for k in np.asarray(keys)[:, 0])
    assert len(s) == 1
    return s.pop()


def _query(blob, rays, seed, **kw):
    ds = rt.DeviceScene(blob)
    try:
        return ds.query(rays, seed=seed, **kw)
    finally:
        ds.close()


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


# ---------------------------------------------------------------- 1. random rays, exact decisions
RANDOM_SETS = [(n, 200 + k) for k, n in enumerate(WORLD_SCENES)] + [("fog_sphere", 300), ("fog_box", 301)]


@pytest.mark.parametrize("name,seed", RANDOM_SETS, ids=[n for n, _ in RANDOM_SETS])
def test_random_rays_exact_decisions(gpu_available, name, seed):
    blob, _ = _world_scene(name)
    rays9, keys, exact, ora, ora_w, share, hits = _world_reference(name, seed)
    rays = _rays(rays9, keys)
    ds = rt.DeviceScene(blob)
    try:
        got = ds.query(rays, seed=_seed(keys))
        occ = ds.query(rays, seed=_seed(keys), occlusion=True)
    finally:
        ds.close()
    dev_w, worst = M(0), None
    for k, (g, (h, guard, _), o) in enumerate(zip(got, exact, ora)):
        if guard:
            continue
        assert int(g["hit"]) == (h is not None) == int(o[0]), (name, k, g, h)
        if h is None:
            assert (g["prim"], g["material"], g["front_face"]) == (-1, -1, 0), (name, k, g)
            assert g["t"] == rays9[k, 8] and g["distance"] == 0 and not g["p"].any()
            continue
        assert (g["prim"], g["material"]) == (h[1], h[2]) == (o[4], o[2]), (name, k, g, h, o)
        assert g["front_face"] == o[3], (name, k, g, o)
        if _rel(g["t"], h[0]) > dev_w:
            dev_w, worst = _rel(g["t"], h[0]), k
    print(f"query[{name}]: {len(rays)} rays, {hits} hits, guard band leaves out {100 * share:.2f} %, "
          f"worst ray {worst}")
    assert share <= 0.01
    _rule(f"query[{name}] t", float(dev_w), ora_w)
    assert np.array_equal(occ, got["hit"].astype(np.uint8))


# ---------------------------------------------------------------- 2. interval ends
def test_interval_ends(gpu_available):
    """The dyadic scene of test_world_hit_exact_cases through the public call: a quad is inclusive
    at both ends, a sphere's root strict, a later quad takes a tie; t, prim and hit are exact."""
    sc = rt.Scene(2)
    m = _mats(sc, 5)
    objs = [sc.quad((-1, -1, 3), (2, 0, 0), (0, 2, 0), m[0]),      # z = 3, [-1, 1]^2
            sc.quad((0, 0, 3), (2, 0, 0), (0, 2, 0), m[1]),        # the same plane, [0, 2]^2, later
            sc.sphere((0.5, 0.5, 4), 1.0, m[2]),                   # near root on z = 3 at (0.5, 0.5)
            sc.sphere((-6, 0, 5), 1.0, m[3]),
            sc.quad((-7, -1, 4), (2, 0, 0), (0, 2, 0), m[4])]      # the same t as sphere 3, later
    blob = sc.serialize(sc.hittable_list(*objs), None)
    up, dn = (lambda x: math.nextafter(x, INF)), (lambda x: math.nextafter(x, -INF))
    z = (0, 0, 1)
    cases = [  # o, d, tmin, tmax -> (t, prim) or None
        ((-0.5, -0.5, 0), z, 1e-4, INF, (3.0, 0)),
        ((0.5, 0.5, 0), z, 1e-4, INF, (3.0, 1)),        # both quads and the sphere at t = 3: quad 1
        ((0.25, 0.25, 0), z, 1e-4, INF, (3.0, 1)),      # both quads: the later one takes the tie
        ((-0.5, -0.5, 0), z, 3.0, INF, (3.0, 0)),       # t == tmin: inclusive
        ((-0.5, -0.5, 0), z, 1e-4, 3.0, (3.0, 0)),      # t == tmax: inclusive
        ((-0.5, -0.5, 0), z, up(3.0), INF, None),
        ((-0.5, -0.5, 0), z, 1e-4, dn(3.0), None),
        ((-1.0, 0.0, 0), z, 1e-4, INF, (3.0, 0)),       # on quad 0's edge
        ((-1.0, -1.0, 0), z, 1e-4, INF, (3.0, 0)),      # on its corner
        ((dn(-1.0), 0.0, 0), z, 1e-4, INF, None),
        ((2.0, 2.0, 0), z, 1e-4, INF, (3.0, 1)),        # quad 1's far corner
        ((-6, 0, 0), z, 1e-4, INF, (4.0, 4)),           # sphere 3 at t = 4, then quad 4 at t = 4: the quad
        ((-6, 0, 0), z, 4.0, INF, (4.0, 4)),            # the sphere's near root == tmin is not its hit
        ((-6, 0, 0), z, 1e-4, 4.0, (4.0, 4)),
        ((-6, 0, 0), z, up(4.0), INF, (6.0, 3)),        # the sphere's far root
        ((-6, 0, 0), z, up(4.0), 6.0, None),            # ... at tmax: strict
        ((-6, 0, 8), (0, 0, -1), 1e-4, INF, (2.0, 3)),  # from the other side: the sphere first
        ((0.5, 0.5, 8), (0, 0, -2), 1e-4, INF, (1.5, 2)),
        ((0.5, 0.5, 0), (0, 0, 0.5), 1e-4, 6.0, (6.0, 1)),
    ]
    recs = np.array([list(o) + list(d) + [0.0, a, b] for o, d, a, b, _ in cases], float)
    keys = _keys(len(cases))
    ora = _oracle_world(blob, recs, keys)
    got = _query(blob, _rays(recs, keys), _seed(keys))
    for (o, d, a, b, want), g, r in zip(cases, got, ora):
        if want is None:
            assert r[0] == 0 and g["hit"] == 0 and g["prim"] == -1 and g["t"] == b, (o, d, a, b, g)
            continue
        assert (r[0], r[1], r[4]) == (1, want[0], want[1]), ("oracle", o, d, a, b, r.tolist())
        assert (g["hit"], g["t"], g["prim"], g["material"]) == (1, want[0], want[1], r[2]), (o, d, a, b, g)
        assert g["distance"] == want[0] * math.sqrt(sum(x * x for x in d))


# ---------------------------------------------------------------- 3. p, normal, distance
def _residual(o, d, t, p):
    """max |p - (o + t d)| / (|o| + |t d|), infinity norms, the difference in exact arithmetic."""
    o, d, t, p = [Fr(x) for x in o], [Fr(x) for x in d], Fr(float(t)), [Fr(float(x)) for x in p]
    err = max(abs(pp - (oo + t * dd)) for pp, oo, dd in zip(p, o, d))
    return float(err / (max(abs(x) for x in o) + max(abs(t * x) for x in d)))


@pytest.mark.parametrize("name", ["quads", "spheres", "chain6", "instances"])
def test_p_normal_distance(gpu_available, name):
    blob, _ = _world_scene(name)
    rays9, keys, exact, _, _, _, _ = _world_reference(name, 200 + WORLD_SCENES.index(name))
    got = _query(blob, _rays(rays9, keys), _seed(keys))
    dev_p = ora_p = n_w = d_w = 0.0
    n = 0
    for k, (g, (h, guard, _)) in enumerate(zip(got, exact)):
        if guard or h is None:
            continue
        r = rays9[k]
        rec = O.world_hit(blob, r[:7], r[7], r[8])  # t, p3, normal3, front, mat
        assert rec is not None and g["hit"] == 1
        n += 1
        dev_p = max(dev_p, _residual(r[0:3], r[3:6], g["t"], g["p"]))
        ora_p = max(ora_p, _residual(r[0:3], r[3:6], rec[0], rec[1:4]))
        n_w = max(n_w, float(np.abs(g["normal"] - rec[4:7]).max()))
        want = g["t"] * np.linalg.norm(r[3:6])
        d_w = max(d_w, abs(g["distance"] - want) / want)
        assert g["front_face"] == rec[7] and g["material"] == rec[8]
    assert n > 200
    print(f"query[{name}]: {n} hits, normal max |n - n_oracle| {n_w:.3e}, distance rel {d_w:.3e}")
    print(f"query[{name}] p residual: device worst {dev_p:.3e}, reference worst {ora_p:.3e}")
    assert dev_p <= max(2.0 * ora_p, 4 * ULP), (name, dev_p, ora_p)
    assert n_w <= 1e-9, (name, n_w)
    assert d_w <= 1e-14, (name, d_w)


# ---------------------------------------------------------------- 4. every kernel instance
CAMERA_SCENES = ["cornell_smoke", "final_scene", "unstaged_flat", "nested_bvh", "nested_flat"]
CAM_SEED = 1


@functools.lru_cache(maxsize=None)
def _camera_set(name):
    """No GPU: the 24 x 24 camera rays of test_aov_gpu's scene, their keys and the oracle's answer."""
    if name == "nested_flat":
        blob, cam = V.build(NESTED_FLAT), _depth1_scene("nested_bvh")[1]
    else:
        blob, cam = _depth1_scene(name)
    W, H = cam.image_width, cam.image_height
    assert (W, H, cam.sqrt_spp) == (24, 24, 1)
    rays7 = np.array([O.camera_ray(cam, CAM_SEED, i, j, 0, 0) for j in range(H) for i in range(W)])
    keys = np.array([[CAM_SEED, j * W + i, 0] for j in range(H) for i in range(W)], np.uint64)
    rays9 = np.concatenate([rays7, np.full((len(rays7), 1), 1e-4), np.full((len(rays7), 1), INF)], 1)
    ora = O.world_hit_batch(blob, rays7, keys, 1e-4, INF)
    return blob, _rays(rays9, keys), ora


def _instance(blob):
    """(bvh, staged, nested) as rt_query.hip's kernel choice reads them."""
    h = P.scene_header(blob)
    staged = bool(V.stage_scene(blob, h["has_textures"])[0]) and not h["has_bvh"] and not h["nested_volumes"]
    return bool(h["has_bvh"]), staged, bool(h["nested_volumes"])


def test_camera_scenes_reach_every_instance():
    got = {n: _instance(_camera_set(n)[0]) for n in CAMERA_SCENES}
    assert got == {"cornell_smoke": (False, True, False), "final_scene": (True, False, False),
                   "unstaged_flat": (False, False, False), "nested_bvh": (True, False, True),
                   "nested_flat": (False, False, True)}, got


@pytest.mark.parametrize("name", CAMERA_SCENES)
def test_every_kernel_instance(gpu_available, name):
    blob, rays, ora = _camera_set(name)
    ds = rt.DeviceScene(blob)
    try:
        got = ds.query(rays, seed=CAM_SEED)
        ref_bvh = ds.query(rays, seed=CAM_SEED, flags=rt.RT_FLAG_REFERENCE_BVH)
        occ = ds.query(rays, seed=CAM_SEED, occlusion=True)
    finally:
        ds.close()
    hit = ora[:, 0] > 0
    assert 50 < hit.sum() <= len(hit)
    for f, col in (("hit", 0), ("material", 2), ("front_face", 3), ("prim", 4)):
        bad = np.nonzero(got[f] != ora[:, col])[0]
        assert len(bad) == 0, (name, f, bad[:8], got[bad[:8]], ora[bad[:8]])
    rel = np.abs(got["t"][hit] - ora[hit, 1]) / np.abs(ora[hit, 1])
    print(f"query[{name}]: {int(hit.sum())} hits of {len(hit)}, t worst rel {rel.max():.3e}, "
          f"{len(set(got['prim'][hit].tolist()))} prims, {len(set(got['material'][hit].tolist()))} materials")
    assert rel.max() <= 1e-10, (name, rel.max())
    assert np.all(np.isinf(got["t"][~hit]))
    assert np.array_equal(_raw(got), _raw(ref_bvh))
    assert np.array_equal(occ, got["hit"].astype(np.uint8))


# ---------------------------------------------------------------- 5. against the AOV pass
def test_against_the_aov_pass(gpu_available):
    blob, cam = rt.preset_blob("cornell_box", width=16, spp=1)
    W, H = cam.image_width, cam.image_height
    assert (W, H, cam.sqrt_spp) == (16, 16, 1)
    rays7 = np.array([O.camera_ray(cam, 1, i, j, 0, 0) for j in range(H) for i in range(W)])
    rays = rt.make_rays(rays7[:, 0:3], rays7[:, 3:6], rays7[:, 6],
                        pixel=np.arange(W * H, dtype=np.uint32))
    ds = rt.DeviceScene(blob)
    try:
        aov, _ = ds.render_aov(cam, rt.make_opts(cam, seed=1))
        got = ds.query(rays, seed=1)
    finally:
        ds.close()
    aov = aov.reshape(W * H, rt.AOV_CHANNELS)
    assert np.array_equal(got["hit"], aov[:, rt.AOV_HITS]) and 0 < got["hit"].sum() < W * H
    assert np.array_equal(got["material"], aov[:, rt.AOV_MATID])
    h = got["hit"] == 1
    t32 = np.where(h, got["t"], 0.0).astype(np.float32)
    n32 = got["normal"].astype(np.float32)
    for what, a, b in (("t", t32, aov[:, rt.AOV_T]), ("normal", n32, aov[:, 2:5])):
        e = np.abs(a.astype(np.float64) - b) / np.maximum(1.0, np.abs(b))
        print(f"query vs AOV {what}: max |d| / max(1, |ref|) = {e.max():.3e}")
        assert e.max() <= TOL, (what, e.max())


# ---------------------------------------------------------------- 6. independence, ragged sizes
def test_independence_and_ragged_sizes(gpu_available):
    blob, rays, _ = _camera_set("final_scene")
    big = np.resize(rays, 2000)
    perm = np.random.default_rng(7).permutation(len(big))
    ds = rt.DeviceScene(blob)
    try:
        whole = ds.query(big, seed=CAM_SEED)
        parts = {n: ds.query(big[:n], seed=CAM_SEED) for n in (1, 63, 65, 767, 769)}
        shuffled = ds.query(big[perm], seed=CAM_SEED)
    finally:
        ds.close()
    assert 0 < (whole["hit"] == 1).sum() < len(big)
    assert np.array_equal(_raw(whole[:576]), _raw(whole[576:1152]))  # recycled rays, other lanes
    for n, part in parts.items():
        assert np.array_equal(_raw(part), _raw(whole[:n])), n
    assert np.array_equal(_raw(shuffled), _raw(whole[perm]))


@pytest.mark.parametrize("name", ["final_scene", "cornell_smoke"])
def test_a_batch_larger_than_the_device(gpu_available, name):
    """More rays than the device holds lanes at once (at most 256 CUs x 16 waves x 64 lanes =
    262,144): workgroups start as others end, the last one ragged. The recycled rays give the
    records of the small batch, wherever and whenever they ran."""
    blob, rays, _ = _camera_set(name)
    n = 600003
    ds = rt.DeviceScene(blob)
    try:
        small = ds.query(rays, seed=CAM_SEED)
        big, st = ds.query(np.resize(rays, n), seed=CAM_SEED, stats=True)
        occ = ds.query(np.resize(rays, n), seed=CAM_SEED, occlusion=True)
    finally:
        ds.close()
    assert np.array_equal(_raw(big), _raw(np.resize(small, n)))
    assert np.array_equal(occ, np.resize(small["hit"], n).astype(np.uint8))
    assert (st.samples, st.launches, st.out_bytes) == (n, 1, 80 * n)


# ---------------------------------------------------------------- 7. invalid rays
def test_invalid_rays(gpu_available):
    """The handled path: such a ray never reaches the walker and its record is hit = -1, zeros."""
    blob, rays, _ = _camera_set("cornell_smoke")
    good = rays[:200].copy()
    nan, inf = float("nan"), float("inf")
    edits = [("origin", 0, nan), ("origin", 2, inf), ("origin", 1, -inf), ("dir", 0, nan),
             ("dir", 2, -inf), ("dir", 1, inf), ("time", None, nan), ("time", None, inf),
             ("tmin", None, nan), ("tmax", None, nan), ("tmin", None, inf), ("tmin", None, -inf),
             ("dir", "zero", 0.0), ("dir", "zero", -0.0)]
    at = [3 + 13 * k for k in range(len(edits))]  # spread over the first three waves, one wave whole
    at += list(range(64, 128))
    mixed = good.copy()
    for n, k in enumerate(at):
        f, c, v = edits[n % len(edits)]
        if c is None:
            mixed[f][k] = v
        elif c == "zero":
            mixed[f][k] = (v, v, -v)
        else:
            mixed[f][k, c] = v
    bad = np.zeros(len(good), bool)
    bad[at] = True
    ds = rt.DeviceScene(blob)
    try:
        want = ds.query(good, seed=CAM_SEED)
        got, st = ds.query(mixed, seed=CAM_SEED, stats=True)  # raises unless RT_OK
        occ = ds.query(mixed, seed=CAM_SEED, occlusion=True)
    finally:
        ds.close()
    zero = np.zeros(1, rt.HIT_DTYPE)
    zero["hit"] = -1
    assert np.array_equal(_raw(got[bad]), np.repeat(_raw(zero), bad.sum(), 0))
    assert np.array_equal(_raw(got[~bad]), _raw(want[~bad]))
    assert np.array_equal(occ[bad], np.full(bad.sum(), 255, np.uint8))
    assert np.array_equal(occ[~bad], want["hit"][~bad].astype(np.uint8))
    assert st.samples == len(mixed) and st.launches == 1
    # +inf tmax and a negative finite tmin are valid intervals
    edge = good[:4].copy()
    edge["tmin"] = -1.0
    assert (_query(blob, edge, CAM_SEED)["hit"] >= 0).all()


# ---------------------------------------------------------------- 8. stats, no state, error paths
def test_stats_no_state_and_error_paths(gpu_available):
    blob, cam = rt.preset_blob("cornell_box", width=16, spp=4)
    rays7 = np.array([O.camera_ray(cam, 1, i, 8, 0, 0) for i in range(16)])
    rays = rt.make_rays(rays7[:, 0:3], rays7[:, 3:6], rays7[:, 6])
    opts = rt.make_opts(cam, seed=3)
    ds = rt.DeviceScene(blob)
    try:
        before, _ = ds.render(cam, opts)
        got, st = ds.query(rays, seed=1, stats=True)
        occ, st_o = ds.query(rays, seed=1, occlusion=True, stats=True)
        after, _ = ds.render(cam, opts)
        assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
        assert (st.samples, st.launches, st.out_bytes) == (16, 1, 16 * 80)
        assert (st_o.samples, st_o.launches, st_o.out_bytes) == (16, 1, 16)
        for s in (st, st_o):
            assert not any(s.ops[:]) and s.ms_kernel > 0.0 and s.ms_total >= s.ms_kernel
        assert np.array_equal(occ, got["hit"].astype(np.uint8)) and got["hit"].sum() > 0
        # the argument errors start no kernel and leave the out buffer alone
        lib = rt.device_lib()
        out = np.full(16, 0xAB, np.uint8).repeat(80)
        base = out.copy()
        for qp in (rt.RtQueryParams(1, rt.RT_FLAG_OVERWRITE, 0), rt.RtQueryParams(1, 0, 4)):
            s = rt.RtStats()
            rc = lib.rt_query_rays(ds._h, C.byref(qp), rays.ctypes.data, len(rays), out.ctypes.data,
                                   C.byref(s))
            assert rc == rt.RT_ERR_INVALID_ARG and s.launches == 0 and np.array_equal(out, base)
        s = rt.RtStats()
        ok = rt.RtQueryParams(1, 0, 0)
        assert lib.rt_query_rays(ds._h, C.byref(ok), rays.ctypes.data, 0, out.ctypes.data,
                                 C.byref(s)) == rt.RT_OK
        assert s.launches == 0 and np.array_equal(out, base)
    finally:
        ds.close()


def test_query_device_on_a_stream(gpu_available):
    """query_device with device buffers on a stream of the caller's: the bytes of query()."""
    blob, rays, _ = _camera_set("cornell_smoke")
    n = len(rays)
    ds = rt.DeviceScene(blob)
    d_in = DevBuf((n, 20), init=_raw(rays).view(np.float32))  # 80 bytes a record
    d_out = DevBuf((n, 20))
    stream = Stream()
    try:
        want = ds.query(rays, seed=CAM_SEED)
        assert ds.query_device(d_in.ptr, n, d_out.ptr, seed=CAM_SEED, stream=stream.handle) is None
        st = ds.query_device(d_in.ptr, n, d_out.ptr, seed=CAM_SEED, stream=stream.handle, stats=True)
        stream.sync()
        assert np.array_equal(d_out.download().view(np.uint8), _raw(want))
        assert (st.samples, st.launches, st.out_bytes) == (n, 1, 80 * n)
    finally:
        stream.destroy()
        d_in.free()
        d_out.free()
        ds.close()
