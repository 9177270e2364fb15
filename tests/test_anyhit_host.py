"""Any-hit ray queries (RT_QUERY_ANY_HIT, include/rt_mi355x.h) and the ambient-occlusion ray
generator (rth_ao_rays, include/rt_host.h), the part that needs no GPU: the constant against the
header text and the bindings, the argument checks of both entry points (made before the scene is
read: the scene handle is a dummy pointer, as in tests/test_query_host.py) and rth_ao_rays against
a numpy restatement of vec3.rs:240-250 and onb.rs:32-47 on the oracle's draws.

Bounds of the restatement. origin, time, tmin, tmax, pixel, sample: bitwise. dir: 1e-14 absolute;
a component is a sum of three products of numbers at most 1 in size, each a few ulps off between
two libms (cos, sin, sqrt of the same arguments): about 10 ulps = 2.2e-15, with a factor four of
margin. |dir| = 1 within 1e-14, dot(dir, normal) >= -1e-15. The mean of dot(dir, normal) over
4,096 hits is 2/3 (a cosine-weighted hemisphere; a uniform one gives 1/2) within four standard
errors, 4 * sqrt((1/18) / 4096) = 0.0147."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
import surely_rt as rt

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "rt_mi355x.h").read_text()
HOST_HEADER = (REPO / "include" / "rt_host.h").read_text()
INF = float("inf")


def test_constant_mirrors_the_header():
    assert re.search(r"#define RT_QUERY_ANY_HIT 0x2u", HEADER)
    assert rt.RT_QUERY_ANY_HIT == 2 and rt.RT_QUERY_OCCLUSION == 1
    assert "#define RT_ABI_VERSION 3" in HEADER
    ffi = (REPO / "rust" / "rt_mi355x" / "src" / "ffi.rs").read_text()
    assert "pub const RT_QUERY_ANY_HIT: u32 = 0x2;" in ffi
    # any-hit is described, no longer listed as missing
    assert "Not covered: an any-hit early exit" not in HEADER


def test_ao_params_mirror_the_header():
    body = re.search(r"typedef struct rth_ao_params \{(.*?)\} rth_ao_params;", HOST_HEADER, re.S)
    text = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = [d.split() for d in text.split(";") if d.strip()]
    sizes = {"uint64_t": 8, "double": 8, "uint32_t": 4}
    assert [(n, sizes[t]) for t, n in fields] == \
        [(f, getattr(rt.RthAoParams, f).size) for f, _ in rt.RthAoParams._fields_]
    assert C.sizeof(rt.RthAoParams) == 32 == sum(sizes[t] for t, _ in fields)  # no padding


def _call(fn, scene, qp, rays, n, out, device):
    lib = rt.device_lib()
    st = rt.RtStats()
    args = [C.c_void_p(scene), C.byref(qp), C.c_void_p(rays), n, C.c_void_p(out)]
    if device:
        args.append(None)
    return getattr(lib, fn)(*args, C.byref(st)), st


@pytest.mark.parametrize("fn,device", [("rt_query_rays_device", True), ("rt_query_rays", False)])
def test_argument_checks_run_before_the_scene_is_read(fn, device):
    """A dummy non-null scene pointer: a check that read the scene would fault the test."""
    dummy = 0x10
    rays = np.zeros(5, rt.RAY_DTYPE)
    raw = np.zeros(1024, np.uint8)
    op = raw.ctypes.data + (-raw.ctypes.data) % 16
    rp = rays.ctypes.data
    assert rp % 16 == 0
    ANY = rt.RT_QUERY_OCCLUSION | rt.RT_QUERY_ANY_HIT
    assert ANY == 3
    # mode == 3 with n_rays == 0: RT_OK, nothing touched, with and without RT_FLAG_REFERENCE_BVH;
    # the byte output needs no alignment (checked with n = 0: a real call would read the scene)
    for flags in (0, rt.RT_FLAG_REFERENCE_BVH):
        for o in (op, op + 3):
            rc, st = _call(fn, dummy, rt.RtQueryParams(1, flags, ANY), rp, 0, o, device)
            assert rc == rt.RT_OK and st.launches == 0 and st.samples == 0, (flags, o - op)
    # the any-hit bit alone, unknown bits beside it
    for mode in (2, 4, 7, 0x80000003):
        for n in (0, 4):
            rc, st = _call(fn, dummy, rt.RtQueryParams(1, 0, mode), rp, n, op, device)
            assert rc == rt.RT_ERR_INVALID_ARG and st.launches == 0, (mode, n)
    # mode == 3 takes RT_FLAG_REFERENCE_BVH only
    for flags in (rt.RT_FLAG_OVERWRITE, rt.RT_FLAG_COUNT_OPS, 0x20,
                  rt.RT_FLAG_INTERPRETER | rt.RT_FLAG_REFERENCE_BVH):
        rc, st = _call(fn, dummy, rt.RtQueryParams(1, flags, ANY), rp, 4, op, device)
        assert rc == rt.RT_ERR_INVALID_ARG and st.launches == 0, flags
    # the other checks of occlusion mode hold in any-hit mode
    ok = rt.RtQueryParams(1, 0, ANY)
    for scene, r, n, o in ((0, rp, 4, op), (dummy, 0, 4, op), (dummy, rp, 4, 0),
                           (dummy, rp, 1 << 31, op), (dummy, rp + 4, 4, op)):
        rc, st = _call(fn, scene, ok, r, n, o, device)
        assert rc == rt.RT_ERR_INVALID_ARG and st.launches == 0
    assert not raw.any()


# ---------------------------------------------------------------- rth_ao_rays
def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _restate(primary, hits, k, seed, radius, tmin):
    """vec3.rs:240-250 and onb.rs:32-47 in numpy on the oracle's draws."""
    out = np.zeros(len(primary), rt.RAY_DTYPE)
    out["time"], out["pixel"] = primary["time"], primary["pixel"]
    out["tmin"], out["tmax"], out["sample"] = tmin, radius, k
    h = hits["hit"] == 1
    r = np.array([O.rng_draws(seed, int(p), k, 2) for p in primary["pixel"][h]]).reshape(-1, 2)
    phi = 2.0 * np.pi * r[:, 0]
    x, y, z = np.cos(phi) * np.sqrt(r[:, 1]), np.sin(phi) * np.sqrt(r[:, 1]), np.sqrt(1.0 - r[:, 1])
    w = _unit(hits["normal"][h])
    a = np.where((np.abs(w[:, 0]) > 0.9)[:, None], [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    v = _unit(np.cross(w, a))
    u = np.cross(w, v)
    out["dir"][h] = x[:, None] * u + y[:, None] * v + z[:, None] * w
    out["origin"][h] = hits["p"][h]
    return out


@pytest.fixture(scope="module")
def ao_case():
    g = np.random.default_rng(11)
    n_rand = 4096
    axis = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    # |x| just above and just below build_from_w's 0.9: 1e-9 away, far more than the ulp by which
    # two normalisations of the same vector can differ
    hi, lo = 0.9 + 1e-9, 0.9 - 1e-9
    edge = [[hi, np.sqrt(1 - hi * hi), 0.0], [lo, np.sqrt(1 - lo * lo), 0.0],
            [-hi, 0.0, np.sqrt(1 - hi * hi)], [-lo, 0.0, np.sqrt(1 - lo * lo)]]
    normals = np.concatenate([_unit(g.normal(size=(n_rand, 3))), np.array(axis, float),
                              np.array(edge, float), _unit(g.normal(size=(7, 3)))])
    n = len(normals)
    hits = np.zeros(n, rt.HIT_DTYPE)
    hits["normal"] = normals
    hits["p"] = g.uniform(-50, 50, (n, 3))
    hits["t"] = g.uniform(1, 9, n)
    hits["hit"] = 1
    hits["hit"][-7:] = [0, -1, 0, -1, 0, 2, -7]  # anything but 1 is "no surface"
    primary = rt.make_rays(g.normal(size=(n, 3)), g.normal(size=(n, 3)), time=g.uniform(0, 1, n),
                           pixel=g.permutation(1 << 20)[:n].astype(np.uint32), sample=5)
    return primary, hits, n_rand


@pytest.mark.parametrize("k,seed,radius,tmin", [(0, 1, INF, 1e-4), (3, 0xDEADBEEF12345678, 2.5, 0.0)])
def test_ao_rays_against_the_restatement(ao_case, k, seed, radius, tmin):
    primary, hits, n_rand = ao_case
    got = rt.ao_rays(primary, hits, k, seed=seed, radius=radius, tmin=tmin)
    want = _restate(primary, hits, k, seed, radius, tmin)
    assert got.dtype == rt.RAY_DTYPE and len(got) == len(primary)
    for f in ("origin", "time", "tmin", "tmax", "pixel", "sample"):
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes(), f
    h = hits["hit"] == 1
    assert (~h).sum() == 7
    assert not got["dir"][~h].any() and not got["origin"][~h].any()
    err = np.abs(got["dir"] - want["dir"]).max()
    length = np.abs(np.sqrt((got["dir"][h] ** 2).sum(1)) - 1.0).max()
    cosn = (got["dir"][h] * hits["normal"][h]).sum(1)
    mean = cosn[:n_rand].mean()
    print(f"ao_rays k={k}: dir max |d| {err:.3e}, | |dir| - 1 | {length:.3e}, min dir.n {cosn.min():.3e}, "
          f"mean dir.n over {n_rand} {mean:.4f}")
    assert err <= 1e-14
    assert length <= 1e-14
    assert cosn.min() >= -1e-15
    assert abs(mean - 2.0 / 3.0) <= 0.0147
    # the threshold of build_from_w: |x| just above 0.9 takes the y axis, just below the x axis
    e0 = 4096 + 6
    for row, above in ((e0, True), (e0 + 1, False), (e0 + 2, True), (e0 + 3, False)):
        w = hits["normal"][row] / np.linalg.norm(hits["normal"][row])
        assert (abs(w[0]) > 0.9) == above, row
        # the direction in the frame that side of the threshold builds is the cosine sample
        a = np.array([0.0, 1.0, 0.0] if above else [1.0, 0.0, 0.0])
        fv = _unit(np.cross(w, a))
        fu = np.cross(w, fv)
        r1, r2 = O.rng_draws(seed, int(primary["pixel"][row]), k, 2)
        assert abs(got["dir"][row] @ fu - np.cos(2 * np.pi * r1) * np.sqrt(r2)) <= 1e-14, row
        assert abs(got["dir"][row] @ fv - np.sin(2 * np.pi * r1) * np.sqrt(r2)) <= 1e-14, row
    # another k is another direction; the same k the same
    other = rt.ao_rays(primary, hits, k + 1, seed=seed, radius=radius, tmin=tmin)
    assert np.abs(other["dir"][h] - got["dir"][h]).max(1).min() > 0
    again = rt.ao_rays(primary, hits, k, seed=seed, radius=radius, tmin=tmin)
    assert again.tobytes() == got.tobytes()


def test_ao_rays_error_returns(ao_case):
    primary, hits, _ = ao_case
    primary, hits = primary[:4].copy(), hits[:4].copy()
    lib = rt.host_lib()
    out = np.zeros(4, rt.RAY_DTYPE)
    guard = out.copy()
    nan = float("nan")

    def call(p=primary.ctypes.data, h=hits.ctypes.data, ap=None, o=out.ctypes.data, null_params=False):
        ap = ap if ap is not None else rt.RthAoParams(1, INF, 1e-4, 0, 0)
        return lib.rth_ao_rays(p, h, 4, None if null_params else C.byref(ap), o)

    assert call() == 0
    out[:] = guard
    assert call(p=None) == -1 and b"null" in lib.rth_last_error()
    assert call(h=None) == -1 and call(o=None) == -1 and call(null_params=True) == -1
    bad = [rt.RthAoParams(1, nan, 1e-4, 0, 0),      # radius NaN
           rt.RthAoParams(1, 1e-4, 1e-4, 0, 0),     # radius == tmin
           rt.RthAoParams(1, 0.5, 1.0, 0, 0),       # radius < tmin
           rt.RthAoParams(1, -INF, 0.0, 0, 0),
           rt.RthAoParams(1, INF, nan, 0, 0),       # tmin NaN
           rt.RthAoParams(1, INF, INF, 0, 0),       # tmin infinite
           rt.RthAoParams(1, INF, -1e-9, 0, 0),     # tmin < 0
           rt.RthAoParams(1, INF, 1e-4, 0, 1)]      # _pad0
    for ap in bad:
        assert call(ap=ap) == -1, (ap.radius, ap.tmin, ap._pad0)
        assert len(lib.rth_last_error()) > 0
    assert out.tobytes() == guard.tobytes()  # an error writes nothing
    with pytest.raises(rt.RtError):
        rt.ao_rays(primary, hits, 0, radius=nan)
    with pytest.raises(ValueError):
        rt.ao_rays(primary, hits[:3], 0)
    assert len(rt.ao_rays(primary[:0], hits[:0], 0)) == 0
    # the good edge values: tmin == 0, an infinite radius, a radius one ulp above tmin
    for ap in (rt.RthAoParams(1, INF, 0.0, 7, 0), rt.RthAoParams(1, np.nextafter(1e-4, 1.0), 1e-4, 0, 0)):
        assert call(ap=ap) == 0
