"""Ray queries (rt_query_rays*, rt_scene_prim_map; include/rt_mi355x.h), the part that needs no
GPU: the three structs against the header text, the exported symbols, the argument checks (made
before the scene is read: the scene handle here is a dummy pointer) and the prim table of every
preset and of the 18 variant scenes against a pre-order walk of the blob."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import surely_rt as rt
import variant_scenes as V
from test_scene_functions_gpu import OBJ_BVH, _number, _parse

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "rt_mi355x.h").read_text()
C_SIZES = {"int32_t": 4, "uint32_t": 4, "uint64_t": 8, "double": 8}
PRESETS = ["cornell_box", "cornell_smoke", "final_scene", "quads", "simple_light", "two_spheres",
           "two_perlin_spheres", "random_balls", "three_spheres", "earth"]


def _c_fields(name):
    """[(field, bytes)] of a struct of the header, in order (one declaration may name several)."""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", text, re.S)
    assert body, name
    out = []
    for decl in body.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for f in rest.split(","):
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", f.strip())
            assert m, decl
            out.append((m.group(1), C_SIZES[ty] * int(m.group(2) or 1)))
    return out


@pytest.mark.parametrize("name,cls,dtype,size", [
    ("rt_ray", "RtRay", "RAY_DTYPE", 80), ("rt_hit", "RtHit", "HIT_DTYPE", 80),
    ("rt_query_params", "RtQueryParams", None, 16)])
def test_structs_mirror_the_header(name, cls, dtype, size):
    fields = _c_fields(name)
    assert sum(n for _, n in fields) == size  # no padding: the fields alone fill it
    st = getattr(rt, cls)
    assert C.sizeof(st) == size
    assert [(f, getattr(st, f).size) for f, _ in st._fields_] == fields
    assert [getattr(st, f).offset for f, _ in st._fields_] == \
        list(np.cumsum([0] + [n for _, n in fields])[:-1])
    if dtype:
        dt = getattr(rt, dtype)
        assert dt.itemsize == size and list(dt.names) == [f for f, _ in fields]
        assert [dt.fields[f][1] for f in dt.names] == [getattr(st, f).offset for f in dt.names]
    assert re.search(r"#define RT_QUERY_OCCLUSION 0x1u", HEADER) and rt.RT_QUERY_OCCLUSION == 1
    assert "#define RT_ABI_VERSION 3" in HEADER


def test_symbols_are_exported():
    so = C.CDLL(str(REPO / "build" / "librtmi355x.so"))
    for n in ("rt_query_rays_device", "rt_query_rays", "rt_scene_prim_map"):
        assert hasattr(so, n), n


def test_make_rays():
    r = rt.make_rays([[0, 0, 0], [1, 2, 3]], [[0, 0, 1], [0, 1, 0]], time=0.5, tmax=7.0)
    assert r.dtype == rt.RAY_DTYPE and r.shape == (2,)
    assert r["pixel"].tolist() == [0, 1] and r["sample"].tolist() == [0, 0]
    assert r["tmin"].tolist() == [1e-4, 1e-4] and r["tmax"].tolist() == [7.0, 7.0]
    assert r["origin"][1].tolist() == [1, 2, 3] and r["time"].tolist() == [0.5, 0.5]
    assert np.isinf(rt.make_rays([[0, 0, 0]], [[1, 0, 0]], pixel=9)["tmax"][0])


def _call(fn, scene, qp, rays, n, out, device):
    lib = rt.device_lib()
    st = rt.RtStats()
    args = [C.c_void_p(scene), C.byref(qp) if qp is not None else None, C.c_void_p(rays), n,
            C.c_void_p(out)]
    if device:
        args.append(None)
    return getattr(lib, fn)(*args, C.byref(st)), st


@pytest.mark.parametrize("fn,device", [("rt_query_rays_device", True), ("rt_query_rays", False)])
def test_argument_checks_run_before_the_scene_is_read(fn, device):
    """A dummy non-null scene pointer: a check that read the scene would fault the test."""
    dummy = 0x10
    rays = np.zeros(5, rt.RAY_DTYPE)  # 80-byte records: rays[k] stays 16-byte aligned
    raw = np.zeros(1024, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16  # a 16-byte aligned address inside raw
    rp, op = rays.ctypes.data, base
    assert rp % 16 == 0
    ok = rt.RtQueryParams(1, 0, 0)
    occ = rt.RtQueryParams(1, rt.RT_FLAG_REFERENCE_BVH, rt.RT_QUERY_OCCLUSION)
    bad = [
        (0, ok, rp, 4, op), (dummy, None, rp, 4, op), (dummy, ok, 0, 4, op), (dummy, ok, rp, 4, 0),
        (dummy, ok, rp, 1 << 31, op), (dummy, ok, rp, 1 << 40, op),
        (dummy, rt.RtQueryParams(1, rt.RT_FLAG_OVERWRITE, 0), rp, 4, op),
        (dummy, rt.RtQueryParams(1, rt.RT_FLAG_COUNT_OPS, 0), rp, 4, op),
        (dummy, rt.RtQueryParams(1, rt.RT_FLAG_INTERPRETER | rt.RT_FLAG_REFERENCE_BVH, 0), rp, 4, op),
        (dummy, rt.RtQueryParams(1, 0x20, 0), rp, 4, op),
        (dummy, rt.RtQueryParams(1, 0, 2), rp, 4, op),
        (dummy, rt.RtQueryParams(1, 0, 0x80000001), rp, 4, op),
        (dummy, ok, rp + 8, 4, op), (dummy, occ, rp + 4, 4, op),
        (dummy, ok, rp, 4, op + 8), (dummy, ok, rp, 4, op + 1),
    ]
    for scene, qp, r, n, o in bad:
        rc, st = _call(fn, scene, qp, r, n, o, device)
        assert rc == rt.RT_ERR_INVALID_ARG, (scene, r - rp, n, o - op)
        assert st.launches == 0 and st.samples == 0
    assert not raw.any()
    # n_rays == 0 returns RT_OK and touches nothing, the scene included; an occlusion buffer
    # needs no alignment (checked with n = 0: a real call would read the dummy scene)
    for qp, o in ((ok, op), (occ, op + 3)):
        rc, st = _call(fn, dummy, qp, rp, 0, o, device)
        assert rc == rt.RT_OK and st.launches == 0
    assert not raw.any()


def _scenes():
    out = [(n, lambda n=n: rt.preset_blob(n, width=32, spp=4)[0]) for n in PRESETS]
    out += [("variant-" + "".join(map(str, k)), lambda k=k: V.build(k)) for k in V.parse_rows()]
    return out


def _has_bvh(node):
    return node["tag"] == OBJ_BVH or any(_has_bvh(k) for k in node.get("kids", []))


@pytest.mark.parametrize("name,make", _scenes(), ids=[n for n, _ in _scenes()])
def test_prim_map(name, make):
    blob = make()
    world, _ = _parse(blob.slots, blob.header()["world_off"])
    K = _number(world)
    word, prim = rt.prim_map(blob)
    assert len(word) == len(prim) == K > 0
    assert np.all(np.diff(word.astype(np.int64)) > 0)  # ascending: the kernel's binary search
    assert sorted(prim.tolist()) == list(range(K))
    if not _has_bvh(world):
        assert prim.tolist() == list(range(K))  # memory order is the blob's order
    # cap = 0 reports the count and writes nothing; a short cap writes a prefix
    n = C.c_uint32(0)
    lib = rt.device_lib()
    assert lib.rt_scene_prim_map(blob.ref(), None, None, 0, C.byref(n)) == rt.RT_OK and n.value == K
    w2, p2 = np.full(3, 0xFFFFFFFF, np.uint32), np.full(3, 0xFFFFFFFF, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.rt_scene_prim_map(blob.ref(), w2.ctypes.data_as(u32p), p2.ctypes.data_as(u32p), 2,
                                 C.byref(n)) == rt.RT_OK and n.value == K
    m = min(2, K)
    assert w2[:m].tolist() == word[:m].tolist() and p2[:m].tolist() == prim[:m].tolist()
    assert w2[2] == 0xFFFFFFFF and p2[2] == 0xFFFFFFFF
    assert lib.rt_scene_prim_map(None, None, None, 0, C.byref(n)) == rt.RT_ERR_INVALID_ARG
    assert lib.rt_scene_prim_map(blob.ref(), None, None, 2, C.byref(n)) == rt.RT_ERR_INVALID_ARG


def test_prim_map_of_a_duplicated_span_one_leaf():
    """A BvhNode over three leaves holds one of them twice (hittable.rs:161-162). The reference's
    record for a duplicated quad comes from the second copy (its inclusive interval accepts the
    re-test over [tmin, rec.t]), for a duplicated sphere from the first (strict): the first copy's
    record, the one the walker reports, carries that prim. Checked against the oracle's own prim
    for one ray per leaf."""
    import oracle_lib as O

    for kind in ("quad", "sphere"):
        sc = rt.Scene(5)
        m = sc.lambertian((0.5, 0.5, 0.5))
        xs = (-4.0, 0.0, 4.0)
        if kind == "quad":
            leaves = [sc.quad((x - 1, -1, 0), (2, 0, 0), (0, 2, 0), m) for x in xs]
        else:
            leaves = [sc.sphere((x, 0, 0), 1.0, m) for x in xs]
        blob = sc.serialize(sc.hittable_list(sc.create_bvh(sc.hittable_list(*leaves))), None)
        world, _ = _parse(blob.slots, blob.header()["world_off"])
        K = _number(world)
        assert K == 4  # three leaves, one of them twice
        word, prim = rt.prim_map(blob)
        assert sorted(prim.tolist()) == [0, 1, 2, 3]
        rays = np.array([[x, 0, 5, 0, 0, -1, 0] for x in xs], float)
        keys = np.array([[1, k, 0] for k in range(3)], np.uint64)
        ora = O.world_hit_batch(blob, rays, keys, 1e-4, float("inf"))
        assert ora[:, 0].tolist() == [1, 1, 1]
        want = sorted(int(p) for p in ora[:, 4])
        # the records a product walk reports: every leaf's first copy, i.e. all but the record
        # right after the first copy of the duplicated leaf
        dup = [k for k in range(K - 1) if _leaf(world, k) == _leaf(world, k + 1)]
        assert len(dup) == 1
        first = [int(prim[k]) for k in range(K) if k != dup[0] + 1]
        assert sorted(first) == want, (kind, prim.tolist(), want)
        assert (prim.tolist() == [0, 1, 2, 3]) == (kind == "sphere")


def _leaf(node, k):
    """The k-th primitive of the tree in pre-order, without its number."""
    out = []

    def walk(nd):
        if "prim" in nd:
            out.append({a: b for a, b in nd.items() if a != "prim"})
        for c in nd.get("kids", []):
            walk(c)
    walk(node)
    return out[k]
