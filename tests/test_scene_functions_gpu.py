"""The scene-level device functions of rt_kernel.h, probed one by one on the GPU.

tests/test_device_primitives_gpu.py runs each small inline function alone; the render tests
compare whole images at 1e-4 per pixel. Between the two sit the functions that read the flattened
scene tables and call the primitives: traverse, world_quad_test / sphere_test, xform_in / xform_out,
frame_ray / frame_out (and the long-chain table), volume_two_hits / volume_hit, light_pdf and
tex_value. A camera and a path tracer never hand them an origin on a surface, a direction with a
zero component, a ray from 1e13 away, u == 1.0 on a one-pixel image or a checker on its own
discontinuity plane; these tests do, through the scene probe (csrc/probe/rt_probe_scene.hip,
tests/probe_lib.py: kernels that call the product's functions on the product's flattened tables
and restate nothing), against the f64 oracle's batch hooks (oracle_world_hit_batch,
oracle_light_pdf_batch, oracle_tex_value_batch) and exact rational arithmetic on the blob's own
constants.

Bounds: the ones tests/test_device_primitives_gpu.py states, with its helpers.
  * Decisions (hit or miss, which primitive, a zero PDF, a texel, a checker cell) are exact outside
    the guard band: a relative 1e-9 around each decision boundary, evaluated in exact arithmetic
    (roots through mpmath at 200 bits on the exact discriminant). At most 1 % of a set may be left
    out; on the rest the f64 oracle and the device must both take the exact decision.
  * Vector-operation rule for t, frame_ray and frame_out: the device's worst error against the
    exact value may be at most twice the oracle's own worst error (for the frames: Python floats
    in the oracle's operation order).
  * f32 weights (light_pdf, the noise texture): twice the worst error of a plain numpy float32
    restatement on the same inputs.
  * One walk against two passes (volume_two_hits), COUNT against the product build (traverse) and
    the two Perlin-table paths: bit for bit on every ray, no guard band.
Every test prints its figures. Every generator was also run without a GPU for the oracle alone
(the exact arithmetic and the oracle need none): every guard share there is the one printed here.

volume_two_hits under `fallback`: the function's contract is that the caller reruns the second
query, so its own `both` only says that a first hit exists. The tests assert exactly that (both
== the first pass's hit, t1 bit for bit) and take the two passes' both and t2 as the answer; an
edge-clipping ray on a box whose entry and exit lie within 1e-4 has no third candidate, so the
two passes miss where the one walk's provisional `both` is set.

Measured on an MI355X (the same table stands in DESIGN.md §2):
  rcp_nr1 (2406 inputs m 2^e, e = -200..200): at most 9 ulp from the correctly rounded reciprocal,
    0.206 ulp on average (rcp_nr: 0 ulp); aquad_test's t is within an ulp of the IEEE quotient
    with r = rcp_nr1(d) as with r = rcp_nr(d) (worst error 1.7-2.1e-16 in both forms)
  device worst / reference worst (vector-operation rule, bound: a factor 2); 1024 rays per scene
    world_hit t  quads 1.40e-15 / 1.23e-15   box 1.36e-16 / 1.36e-16      spheres 3.02e-14 / 2.58e-14
                 chain1 3.43e-14 / 3.74e-14  chain2 2.45e-14 / 4.09e-14   chain4 2.38e-14 / 2.40e-14
                 chain6 1.27e-14 / 1.83e-14  instances 1.46e-14 / 8.23e-15
                 fog_sphere 1.70e-14 / 1.80e-14 (513 draws)  fog_box 1.08e-14 / 9.66e-15 (513 draws)
    frame_ray o, d and frame_out p, n, the worst of the four, by depth
                 1: 1.86e-16 / 1.86e-16   2: 1.76e-16 / 1.76e-16   4: 2.17e-16 / 3.14e-16
                 6: 2.98e-16 / 3.11e-16
  device worst / float32 restatement worst (bound: a factor 2)
    light_pdf    aquad 2.96e-07 / 3.95e-07   gquad 3.77e-07 / 3.09e-07   sphere 7.71e-08 / 4.25e-06
                 spheres2 9.85e-08 / 6.13e-06  quad_sphere 3.32e-07 / 4.25e-06  single 3.20e-07 / 3.04e-07
                 nested 3.02e-07 / 6.13e-06  other 3.20e-07 / 2.96e-07  far_sphere 1.20e-07 / 4.25e-06
    noise        scale 4: 4.83e-07 / 6.63e-04   scale 0.35: 5.27e-07 / 4.78e-05
  volume_two_hits, 1024 rays per boundary, fallback lanes (of them without a third candidate):
    sphere 0, moving sphere 0, box 128 (128), box with a duplicated face 365 (128), one quad 0
  guard band: 0.00 % of the rays left out in every set, on the GPU and for the oracle alone.
  Flipping one decision in a scratch copy of rt_kernel.h: `<=` for `<` in volume_two_hits' tmin2
  test of the near root fails test_volume_two_hits_is_the_two_passes[sphere, moving]; rcp_nr1 without
  its Newton step fails the aquad_test_nr1 cases and test_world_hit_random_rays[box]; the
  checker's parity inverted fails test_tex_value_solid_and_checkers_are_exact.
"""
import functools
import math
from fractions import Fraction as Fr

import mpmath as mp
import numpy as np
import pytest

import oracle_lib as O
import probe_lib as P
import surely_rt as rt
from test_device_primitives_gpu import (AXIS_QUADS, GENERAL_QUAD, INF, M, _bits, _fr, _dot, _ord,
                                        _rng_py, _rule, _scaled, _vec_err)

pytestmark = pytest.mark.gpu

EPS = Fr(1, 10 ** 9)
OBJ_LIST, OBJ_BVH, OBJ_SPHERE, OBJ_QUAD, OBJ_TRANSLATE, OBJ_ROTATE_Y, OBJ_VOLUME = 1, 2, 3, 4, 5, 6, 7
SEED = (0x5EED << 32) | 0x1234


# ---------------------------------------------------------------- the blob, read back
def _parse(s, pos):
    """The object at slot `pos` of a blob (include/rt_mi355x.h) -> (node, next slot). Constants are
    the f64 values the host builder serialised: what the flattener and the oracle both read."""
    f = lambda i: float(s[i:i + 1].view(np.float64)[0])  # noqa: E731
    v3 = lambda i: [f(i), f(i + 1), f(i + 2)]  # noqa: E731
    tag = int(s[pos])
    if tag == OBJ_LIST:
        n, pos = int(s[pos + 1]), pos + 8
        kids = []
        for _ in range(n):
            k, pos = _parse(s, pos)
            kids.append(k)
        return dict(tag=tag, kids=kids), pos
    if tag == OBJ_BVH:  # [tag, bbox6], then left and right
        left, pos = _parse(s, pos + 7)
        right, pos = _parse(s, pos)
        # a span of one leaf is a BvhNode of that leaf twice (hittable.rs:161-162): one candidate
        return dict(tag=tag, kids=[left, right], dup=left == right), pos
    if tag == OBJ_SPHERE:
        return dict(tag=tag, mat=int(s[pos + 1]), moving=int(s[pos + 2]), c=v3(pos + 3), r=f(pos + 6),
                    cv=v3(pos + 7)), pos + 16
    if tag == OBJ_QUAD:
        return dict(tag=tag, mat=int(s[pos + 1]), q=v3(pos + 2), u=v3(pos + 5), v=v3(pos + 8),
                    n=v3(pos + 11), w=v3(pos + 14), D=f(pos + 17), area=f(pos + 18)), pos + 25
    if tag == OBJ_TRANSLATE:
        k, nxt = _parse(s, pos + 10)
        return dict(tag=tag, off=v3(pos + 1), kids=[k]), nxt
    if tag == OBJ_ROTATE_Y:
        k, nxt = _parse(s, pos + 9)
        return dict(tag=tag, sin=f(pos + 1), cos=f(pos + 2), kids=[k]), nxt
    if tag == OBJ_VOLUME:
        k, nxt = _parse(s, pos + 9)
        return dict(tag=tag, mat=int(s[pos + 1]), nid=f(pos + 2), kids=[k]), nxt
    raise AssertionError(f"tag {tag}")


def _number(node, k=0):
    """prim = the node's place among the spheres, quads and volumes in pre-order."""
    if node["tag"] in (OBJ_SPHERE, OBJ_QUAD, OBJ_VOLUME):
        node["prim"] = k
        k += 1
    for c in node.get("kids", []):
        k = _number(c, k)
    return k


def _world(blob):
    node, _ = _parse(blob.slots, blob.header()["world_off"])
    _number(node)
    return node


def _lights(blob):
    node, _ = _parse(blob.slots, blob.header()["lights_off"])
    return node


# ---------------------------------------------------------------- exact arithmetic
def _m(x):
    return M(x.numerator) / M(x.denominator) if isinstance(x, Fr) else M(x)


def _lt(a, b):
    if isinstance(a, mp.mpf) or isinstance(b, mp.mpf):
        return _m(a) < _m(b)
    return a < b


def _close(a, b):
    """a within a relative 1e-9 of the boundary b (exact for rationals)."""
    if isinstance(a, float) and math.isinf(a) or isinstance(b, float) and math.isinf(b):
        return False
    if isinstance(a, mp.mpf) or isinstance(b, mp.mpf):
        a, b = _m(a), _m(b)
        return abs(a - b) <= M(10) ** -9 * max(abs(a), abs(b))
    a, b = Fr(a), Fr(b)
    return abs(a - b) <= EPS * max(abs(a), abs(b))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


class _Ctx:
    """One ray's exact evaluation: `guard` collects every decision within the band; `u` is the
    ray's first draw (or the list of its first draws, for a world with several mediums), `draws` how
    many ConstantMedium draws the walk takes."""

    def __init__(self, tm, u=None):
        self.tm, self.u, self.guard, self.draws = Fr(tm), u, False, 0

    def near(self, a, b):
        if _close(a, b):
            self.guard = True


def _quad_x(cx, nd, o, d, tmin, tmax):
    """Quad::hit (object.rs:453-490) exactly; the interval is inclusive."""
    n, q, u, v, w = (_fr(nd[k]) for k in ("n", "q", "u", "v", "w"))
    den = _dot(n, d)
    cx.near(abs(den), 1e-8)
    if abs(den) < Fr(1e-8):
        return None
    t = (Fr(nd["D"]) - _dot(n, o)) / den
    cx.near(t, tmin), cx.near(t, tmax)
    if _lt(t, tmin) or _lt(tmax, t):
        return None
    pq = [oo + t * dd - qq for oo, dd, qq in zip(o, d, q)]
    a, b = _dot(w, _cross(pq, v)), _dot(w, _cross(u, pq))
    if any(abs(x) <= EPS or abs(x - 1) <= EPS for x in (a, b)):
        cx.guard = True
    return t if 0 <= a <= 1 and 0 <= b <= 1 else None


def _sphere_roots(cx, nd, o, d):
    c = [p + cx.tm * q for p, q in zip(_fr(nd["c"]), _fr(nd["cv"]))] if nd["moving"] else _fr(nd["c"])
    oc = [p - q for p, q in zip(o, c)]
    a, hb = _dot(d, d), _dot(oc, d)
    cc = _dot(oc, oc) - Fr(nd["r"]) ** 2
    disc = hb * hb - a * cc
    if abs(disc) <= EPS * max(hb * hb, abs(a * cc)):
        cx.guard = True
    if disc < 0:
        return None
    sq = mp.sqrt(_m(disc))
    return [(-_m(hb) - sq) / _m(a), (sq - _m(hb)) / _m(a)]


def _sphere_x(cx, nd, o, d, tmin, tmax):
    """Sphere::hit (object.rs:145-184) exactly; the interval is strict."""
    roots = _sphere_roots(cx, nd, o, d)
    for t in roots or []:
        cx.near(t, tmin), cx.near(t, tmax)
        if _lt(tmin, t) and _lt(t, tmax):
            return t
    return None


def _bvh_leaves(nd):
    """The leaves of a BvhNode in blob order, a duplicated span-1 leaf once."""
    if nd["tag"] != OBJ_BVH:
        return [nd]
    return _bvh_leaves(nd["kids"][0]) + ([] if nd["dup"] else _bvh_leaves(nd["kids"][1]))


def _hit_x(cx, nd, o, d, tmin, tmax):
    """Object::hit exactly -> (t, the primitive's node) or None (hittable.rs, transform.rs,
    constant_medium.rs in the reference's order)."""
    tag = nd["tag"]
    if tag == OBJ_LIST:
        best, closest = None, tmax
        for k in nd["kids"]:
            h = _hit_x(cx, k, o, d, tmin, closest)
            if h:
                best, closest = h, h[0]
        return best
    if tag == OBJ_BVH:
        # In exact arithmetic a BvhNode is the list of its leaves: the closest candidate. The
        # reference walks them in its tree's order, not the list's, which decides only between
        # candidates that tie: the guard band, whenever the two smallest lie within it.
        cands = [h for h in (_hit_x(cx, k, o, d, tmin, tmax) for k in _bvh_leaves(nd)) if h]
        cands.sort(key=lambda h: _m(h[0]))
        if len(cands) > 1:
            cx.near(cands[0][0], cands[1][0])
        return cands[0] if cands else None
    if tag == OBJ_QUAD:
        t = _quad_x(cx, nd, o, d, tmin, tmax)
        return None if t is None else (t, nd)
    if tag == OBJ_SPHERE:
        t = _sphere_x(cx, nd, o, d, tmin, tmax)
        return None if t is None else (t, nd)
    if tag == OBJ_TRANSLATE:
        return _hit_x(cx, nd["kids"][0], [p - q for p, q in zip(o, _fr(nd["off"]))], d, tmin, tmax)
    if tag == OBJ_ROTATE_Y:
        s, c = Fr(nd["sin"]), Fr(nd["cos"])
        rot = lambda v: [c * v[0] - s * v[2], v[1], s * v[0] + c * v[2]]  # noqa: E731
        return _hit_x(cx, nd["kids"][0], rot(o), rot(d), tmin, tmax)
    if tag == OBJ_VOLUME:
        b = nd["kids"][0]
        h1 = _hit_x(cx, b, o, d, -INF, INF)
        if not h1:
            return None
        t1 = h1[0]
        h2 = _hit_x(cx, b, o, d, t1 + Fr(0.0001), INF)
        if not h2:
            return None
        t2 = h2[0]
        cx.near(t1, tmin), cx.near(t2, tmax)
        if _lt(t1, tmin):
            t1 = tmin
        if _lt(tmax, t2):
            t2 = tmax
        cx.near(t1, t2)
        if not _lt(t1, t2):
            return None
        if _lt(t1, 0):
            t1 = Fr(0)
        ln = mp.sqrt(_m(_dot(d, d)))
        inside = (_m(t2) - _m(t1)) * ln
        u = cx.u[cx.draws] if isinstance(cx.u, (list, tuple)) else cx.u  # one draw per medium reached
        cx.draws += 1
        dist = M(nd["nid"]) * mp.log(M(u))
        cx.near(dist, inside)
        if dist > inside:
            return None
        return _m(t1) + dist / ln, nd
    raise AssertionError(tag)


def _rel(got, t):
    return abs(_m(Fr(float(got))) - _m(t)) / abs(_m(t))


# ---------------------------------------------------------------- world scenes and rays
def _mats(sc, n):
    return [sc.lambertian((0.05 + 0.9 * k / n, 0.5, 0.5)) for k in range(n)]


def _chain(sc, obj, depth):
    """Translate(RotateY(...)) nests, `depth` transforms deep, and what they do to a local point."""
    ops = []
    for k in range(depth):
        if k % 2 == 0:
            ang = (25.0, -40.0, 70.0)[(k // 2) % 3]
            obj = sc.rotate_y(obj, ang)
            ops.append(("r", math.radians(ang)))
        else:
            off = ((1.5, 0.25, -0.5), (-0.75, 0.5, 1.0), (0.5, -0.25, 0.75))[(k // 2) % 3]
            obj = sc.translate(obj, off)
            ops.append(("t", off))
    return obj, ops


def _to_world(ops, p):
    p = np.array(p, float)
    for kind, a in ops:  # innermost first
        if kind == "r":
            s, c = math.sin(a), math.cos(a)
            p = np.array([c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2]])
        else:
            p = p + np.array(a)
    return p


@functools.lru_cache(maxsize=None)
def _world_scene(name):
    """-> (blob, targets): world-space (centre, radius) of the regions rays are aimed at."""
    sc = rt.Scene(31)
    if name == "quads":
        m = _mats(sc, 4)
        objs = [sc.quad(*AXIS_QUADS[k], m[k]) for k in range(3)] + [sc.quad(*GENERAL_QUAD, m[3])]
        tg = [((3, 0, 0), 1.6), ((0, 3, 0), 1.6), ((0, 0, 3), 1.6), ((1.0, 0.0, 2.6), 1.6)]
    elif name == "box":
        m = _mats(sc, 2)
        objs = [sc.make_box((-1, -0.5, -0.75), (1, 0.5, 0.75), m[0]),
                sc.quad((-3, -1, -3), (6, 0, 0), (0, 0, 6), m[1])]
        tg = [((0, 0, 0), 1.5), ((0, -1, 0), 3.0)]
    elif name == "spheres":
        m = _mats(sc, 3)
        objs = [sc.sphere((0, 0, 0), 1.0, m[0]), sc.sphere((2.5, 0.5, 0), 0.25, m[1]),
                sc.sphere_moving((-2, 0, 1), (-2, 1.5, 1), 0.75, m[2])]
        tg = [((0, 0, 0), 1.3), ((2.5, 0.5, 0), 0.4), ((-2, 0.75, 1), 1.6)]
    elif name.startswith("chain"):
        depth = int(name[5:])
        m = _mats(sc, 3)
        inner = sc.hittable_list(sc.quad((-1, -1, 0.5), (2, 0, 0), (0, 2, 0), m[0]),
                                 sc.sphere((0, 0, -1), 0.75, m[1]))
        inst, ops = _chain(sc, inner, depth)
        objs = [inst, sc.sphere((0, 3, 0), 0.75, m[2])]  # the second runs after the EXIT record
        tg = [(_to_world(ops, (0, 0, 0.5)), 1.5), (_to_world(ops, (0, 0, -1)), 1.0), ((0, 3, 0), 1.0)]
    elif name == "instances":
        m = _mats(sc, 3)
        a, ops_a = _chain(sc, sc.make_box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), m[0]), 2)
        b = sc.translate(sc.rotate_y(sc.sphere((0, 0, 0), 0.75, m[1]), -30.0), (-2, 0.5, 0))
        objs = [a, b, sc.quad((-4, -1, -4), (8, 0, 0), (0, 0, 8), m[2])]
        tg = [(_to_world(ops_a, (0, 0, 0)), 0.9), ((-2, 0.5, 0), 1.0), ((0, -1, 0), 4.0)]
    elif name in ("fog_sphere", "fog_box"):
        m = _mats(sc, 3)
        if name == "fog_sphere":
            fog = sc.constant_medium(sc.sphere((0, 0, 0), 1.0, m[0]), 0.8, (0.9, 0.9, 0.9))
        else:
            box = sc.translate(sc.rotate_y(sc.make_box((-1, -0.5, -0.75), (1, 0.5, 0.75), m[0]), 20.0),
                               (0.25, 0, 0))
            fog = sc.constant_medium(box, 1.2, (0.9, 0.9, 0.9))
        objs = [sc.quad((-3, -1.5, 1.25), (6, 0, 0), (0, 3, 0), m[1]), fog, sc.sphere((0.5, 0, -0.5), 0.4, m[2])]
        tg = [((0, 0, 0), 1.3), ((0, 0, 1.25), 2.0), ((0.5, 0, -0.5), 0.6)]
    else:
        raise AssertionError(name)
    blob = sc.serialize(sc.hittable_list(*objs), None)
    return blob, [(np.array(c, float), r) for c, r in tg]


WORLD_SCENES = ["quads", "box", "spheres", "chain1", "chain2", "chain4", "chain6", "instances"]
N_RAYS = 1024


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _world_rays(name, seed, n=N_RAYS):
    """Seeded rays [n, 9] (o3, d3, time, tmin, tmax): aimed inside and just outside the primitives,
    bounce rays from a surface (tmin 1e-4), directions with one or two exact zeros of either sign,
    lengths 1e-3 and 1e3, a finite tmax around the hits."""
    blob, tg = _world_scene(name)
    rng = np.random.default_rng(seed)
    rays = []
    for k in range(n):
        c, r = tg[rng.integers(len(tg))]
        target = c + _unit(rng) * r * rng.random() ** (1 / 3)
        o = c + _unit(rng) * rng.uniform(2.0, 9.0) * max(r, 1.0) if k % 8 else target + _unit(rng) * 0.3 * r
        d = (target - o) * rng.uniform(0.5, 2.0)
        cls = k % 16
        if cls in (3, 11):  # one or two components exactly +-0: an axis-parallel ray through the target
            ax = rng.integers(3)
            keep = [ax] if cls == 3 else [ax, (ax + 1) % 3]
            o2 = target.copy()
            for a in keep:
                o2[a] = o[a]
            o, d = o2, np.array([(target - o2)[a] if a in keep else rng.choice([0.0, -0.0]) for a in range(3)])
            if not np.any(d):
                d[keep[0]] = 1.0
        if cls == 5:
            d = d / np.linalg.norm(d) * 1e-3
        if cls == 13:
            d = d / np.linalg.norm(d) * 1e3
        tm = (0.0, 1.0, float(rng.random()))[k % 3]
        tmax = INF
        if cls in (6, 14):  # a finite tmax around the hits
            tmax = float(np.linalg.norm(target - o) / np.linalg.norm(d) * rng.uniform(0.5, 1.5))
        rays.append(list(o) + list(d) + [tm, 1e-4, tmax])
    rays = np.array(rays)
    # bounce rays: the oracle's own hit point of an earlier ray becomes an origin on that surface
    first = O.world_hit_batch(blob, rays[:, :7], None, 1e-4, INF)
    src = np.nonzero(first[:, 0] > 0)[0]
    # They leave at |n . d| >= 0.2 |d| (the cut test_quad_light_w makes for the same reason): the
    # origin sits on the surface to a few ulps, so oc . oc - r^2 cancels to a few ulps of r^2 and a
    # root t carries that error times (r / (|d| t / 2))^2 = 1 / cos^2, whoever computes it. At a
    # grazing exit the worst t error of a set is then one ray's cancellation luck, device or
    # oracle, and the factor-2 rule would compare two draws of it, not two evaluations.
    for k in range(1, n, 8):
        if len(src) == 0:
            break
        while True:  # a surface hit (the one-ray hook draws a medium's distance from its own stream)
            j = src[rng.integers(len(src))]
            rec = O.world_hit(blob, rays[j, :7], 1e-4, INF)
            if rec is not None and rec[0] == first[j, 1]:
                break
        rays[k, 0:3] = rec[1:4]
        while True:
            u = _unit(rng)
            if abs(float(np.dot(u, rec[4:7]))) >= 0.2:
                break
        rays[k, 3:6] = u * rng.uniform(0.5, 2.0)
        rays[k, 6] = rays[j, 6]  # the same time: the origin lies on the moving sphere as well
        rays[k, 8] = INF
    return np.ascontiguousarray(rays)


def _oracle_world(blob, rays, keys):
    """oracle_world_hit_batch per (tmin, tmax) group of the records."""
    out = np.zeros((len(rays), 8))
    for lim in {(a, b) for a, b in rays[:, 7:9].tolist()}:
        sel = np.nonzero((rays[:, 7] == lim[0]) & (rays[:, 8] == lim[1]))[0]
        out[sel] = O.world_hit_batch(blob, rays[sel, :7], keys[sel], lim[0], lim[1])
    return out


def _keys(n, seed=SEED):
    return np.array([[seed, 977 * k + 5, 3 * k + 1] for k in range(n)], np.uint64)


@functools.lru_cache(maxsize=None)
def _world_reference(name, seed):
    """No GPU: rays, keys, the exact answers [(t, prim, mat) or None, guard, draws] and the
    oracle's; asserts the oracle's decisions and the set's shape."""
    blob, _ = _world_scene(name)
    rays, keys = _world_rays(name, seed), _keys(N_RAYS)
    world = _world(blob)
    ora = _oracle_world(blob, rays, keys)
    exact, left, hits, ora_w = [], 0, 0, M(0)
    for r, k, g in zip(rays.tolist(), keys.tolist(), ora):
        cx = _Ctx(r[6], O.rng_draws(k[0], k[1], k[2], 1)[0])
        tmax = INF if math.isinf(r[8]) else Fr(r[8])
        h = _hit_x(cx, world, _fr(r[0:3]), _fr(r[3:6]), Fr(r[7]), tmax)
        exact.append((None if h is None else (h[0], h[1]["prim"], h[1]["mat"]), cx.guard, cx.draws))
        if cx.guard:
            left += 1
            continue
        assert bool(g[0]) == (h is not None), ("oracle", name, r)
        if h:
            hits += 1
            assert (g[4], g[2]) == (h[1]["prim"], h[1]["mat"]), ("oracle", name, r, g.tolist())
            ora_w = max(ora_w, _rel(g[1], h[0]))
    share = left / len(rays)
    assert share <= 0.01, (name, share)
    assert 0.2 * len(rays) <= hits <= 0.8 * len(rays), (name, hits)
    return rays, keys, exact, ora, float(ora_w), share, hits


def _prims(blob):
    """word offset of a leaf record -> its place among the leaf records (memory order = blob order
    when there is no BVH)."""
    recs = P.scene_records(blob)
    leaf = recs[np.isin(recs[:, 1], (P.RTL_QUAD, P.RTL_SPHERE, P.RTL_VOLUME))]
    return {int(w): k for k, w in enumerate(leaf[:, 0].tolist())}, recs


def _world_records(rays, keys):
    k = keys.astype(np.float64)
    lo, hi = np.floor(k[:, 0] % 2.0 ** 32), np.floor(k[:, 0] / 2.0 ** 32)
    return np.concatenate([rays, lo[:, None], hi[:, None], k[:, 1:3]], 1)


def _check_world(name, seed):
    blob, _ = _world_scene(name)
    rays, keys, exact, ora, ora_w, share, hits = _world_reference(name, seed)
    got = P.scene_run("world_hit", blob, _world_records(rays, keys))
    prim_of, _ = _prims(blob)
    # the op-counting build and the product build: bit for bit, hit record and generator included
    assert np.array_equal(_bits(got[:, 0:7]), _bits(got[:, 7:14])), name
    dev_w, worst = M(0), None
    for r, k, (h, guard, draws), g in zip(rays.tolist(), keys.tolist(), exact, got):
        _, state, first = _rng_py(k[0], k[1], k[2], draws)
        if guard:
            continue
        assert bool(g[0]) == (h is not None), ("device", name, r, g.tolist())
        assert g[5:7].tolist() == [float(state[0]), float(state[1])], ("draws", name, r, draws)
        if h is None:
            assert g[2] == -1
            continue
        assert prim_of[int(g[2])] == h[1] and g[4] == h[2], ("device", name, r, g.tolist(), h[1:])
        if _rel(g[1], h[0]) > dev_w:
            dev_w, worst = _rel(g[1], h[0]), (r, h[1], float(g[1]))
    print(f"world_hit[{name}]: {len(rays)} rays, {hits} hits, guard band leaves out {100 * share:.2f} %")
    print(f"world_hit[{name}]: the device's worst ray {worst}")
    _rule(f"world_hit[{name}] t", float(dev_w), ora_w)
    return got, exact


@pytest.mark.parametrize("name", WORLD_SCENES)
def test_world_hit_random_rays(gpu_available, name):
    got, _ = _check_world(name, 200 + WORLD_SCENES.index(name))
    _, recs = _prims(_world_scene(name)[0])
    if name.startswith("chain"):
        depth = int(name[5:])
        xf = recs[np.isin(recs[:, 1], (P.RTL_TRANSLATE, P.RTL_ROTATE_Y))]
        assert len(xf) == depth and bool((xf[:, 2] & P.RTL_XFORM_LONG).any()) == (depth > 4)
        frames = set(got[got[:, 0] > 0, 3].astype(int).tolist())
        assert frames == {-1, int(xf[-1, 0])}, frames  # hits inside the chain and after its EXIT
    if name == "instances":
        assert len(set(got[got[:, 0] > 0, 3].astype(int).tolist())) == 3


@pytest.mark.parametrize("name", ["fog_sphere", "fog_box"])
def test_world_hit_with_a_constant_medium(gpu_available, name):
    """One ConstantMedium between opaque primitives, against the keyed oracle hook: the device's
    free-flight draw is the oracle's, the guard band also covers hit_distance against
    dist_inside, and the generator's state afterwards shows one draw when t1 < t2, else none."""
    got, exact = _check_world(name, 300 + (name == "fog_box"))
    blob, _ = _world_scene(name)
    vol = [k for k, nd in enumerate(_world(blob)["kids"]) if nd["tag"] == OBJ_VOLUME]
    assert len(vol) == 1
    draws = np.array([e[2] for e in exact])
    fog_hits = sum(1 for e in exact if e[0] is not None and not e[1] and e[0][1] == 1)
    print(f"world_hit[{name}]: {int(draws.sum())} draws, {fog_hits} hits in the medium")
    assert 0.2 * N_RAYS < draws.sum() < N_RAYS and fog_hits > 50


def test_world_hit_exact_cases(gpu_available):
    """Dyadic coordinates, so every t is exact: t equal to tmin and to tmax through the walker
    (inclusive for a quad, strict for a sphere), a hit point on a quad's edge and corner, and two
    primitives at the same t, where the list order decides (a later quad takes a tie, t <=
    closest; a later sphere does not, t < closest)."""
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
    got = P.scene_run("world_hit", blob, _world_records(recs, keys))
    prim_of, _ = _prims(blob)
    assert np.array_equal(_bits(got[:, 0:7]), _bits(got[:, 7:14]))
    for (o, d, a, b, want), g, r in zip(cases, got, ora):
        if want is None:
            assert r[0] == 0 and g[0] == 0, (o, d, a, b, g.tolist(), r.tolist())
            continue
        assert (r[0], r[1], r[4]) == (1, want[0], want[1]), ("oracle", o, d, a, b, r.tolist())
        assert (g[0], g[1], prim_of[int(g[2])], g[4]) == (1, want[0], want[1], r[2]), \
            ("device", o, d, a, b, g.tolist())


# ---------------------------------------------------------------- rcp_nr1
def test_rcp_nr1_distance_from_the_correctly_rounded_reciprocal(gpu_available):
    """rcp_nr1 (one Newton step) is what every caller of aquad_test passes. No bound on it is
    promised (the test's quotient is corrected once more, which is what bounds t), so its distance
    from the correctly rounded reciprocal is printed and recorded; it must be finite and no better
    input for aquad_test than a few ulps."""
    x = _scaled(np.random.default_rng(171), True)
    got = P.run("rcp_nr1", x)[:, 0]
    want = np.array([float(1 / Fr(v)) for v in x.tolist()])
    d = np.abs(_ord(got) - _ord(want))
    two = np.abs(_ord(P.run("rcp_nr", x)[:, 0]) - _ord(want))
    print(f"rcp_nr1: {len(x)} inputs, worst distance from the correctly rounded reciprocal "
          f"{d.max()} ulp (mean {d.mean():.3f}); rcp_nr {two.max()} ulp")
    assert np.isfinite(got).all() and (np.sign(got) == np.sign(x)).all()
    assert two.max() <= 1


# ---------------------------------------------------------------- frames
def _blob_chain(blob):
    """The transform nest in front of the world's first object, root first."""
    node, chain = _world(blob)["kids"][0], []
    while node["tag"] in (OBJ_TRANSLATE, OBJ_ROTATE_Y):
        chain.append(node)
        node = node["kids"][0]
    return chain


def _frame_refs(chain, rec, num):
    """frame_ray (root first) and frame_out (innermost first) of one record in the number type
    `num`: Fractions for the exact value, floats in the oracle's operation order."""
    o, d, p, n = ([num(x) for x in rec[a:a + 3]] for a in (1, 4, 7, 10))
    for tr in chain:
        if tr["tag"] == OBJ_TRANSLATE:
            o = [a - num(b) for a, b in zip(o, tr["off"])]
        else:
            s, c = num(tr["sin"]), num(tr["cos"])
            o = [c * o[0] + -(s * o[2]), o[1], s * o[0] + c * o[2]]
            d = [c * d[0] + -(s * d[2]), d[1], s * d[0] + c * d[2]]
    for tr in reversed(chain):
        if tr["tag"] == OBJ_TRANSLATE:
            p = [a + num(b) for a, b in zip(p, tr["off"])]
        else:
            s, c = num(tr["sin"]), num(tr["cos"])
            p = [c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2]]
            n = [c * n[0] + s * n[2], n[1], -s * n[0] + c * n[2]]
    return o, d, p, n


@pytest.mark.parametrize("depth", [1, 2, 4, 6])
def test_frame_ray_and_frame_out(gpu_available, depth):
    """Every prefix of a Translate(RotateY(...)) nest is a frame: frame_ray and frame_out against
    the transform sequence applied exactly to the sin, cos and offsets the blob holds. Depth 6
    reads its chain from the RTL_XFORM_LONG table."""
    blob, _ = _world_scene(f"chain{depth}")
    chain = _blob_chain(blob)
    recs = P.scene_records(blob)
    xf = recs[np.isin(recs[:, 1], (P.RTL_TRANSLATE, P.RTL_ROTATE_Y))]
    assert len(chain) == depth == len(xf) and xf[:, 3].tolist() == list(range(1, depth + 1))
    rng = np.random.default_rng(400 + depth)
    n = 128
    rows = []
    for k in range(depth):
        unit = lambda: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3)))  # noqa: E731
        rows.append(np.concatenate([np.full((n, 1), float(xf[k, 0])), rng.uniform(-600, 600, (n, 3)),
                                    unit() * rng.uniform(0.5, 2.0, (n, 1)), rng.uniform(-600, 600, (n, 3)),
                                    unit()], 1))
    rows = np.concatenate(rows)
    got = P.scene_run("frame", blob, rows)
    exact, ref = [], []
    for r in rows.tolist():
        pre = chain[:int(xf[:, 0].tolist().index(int(r[0]))) + 1]
        exact.append(_frame_refs(pre, r, Fr))
        ref.append(_frame_refs(pre, r, float))
    for col, name in enumerate(("frame_ray o", "frame_ray d", "frame_out p", "frame_out n")):
        ex = [[_m(x) for x in e[col]] for e in exact]
        _rule(f"{name}, depth {depth}", _vec_err(got[:, 3 * col:3 * col + 3], ex),
              _vec_err([e[col] for e in ref], ex))
    # frame -1: the inputs come back bit for bit
    world = rows.copy()
    world[:, 0] = -1.0
    back = P.scene_run("frame", blob, world)
    assert np.array_equal(_bits(back), _bits(world[:, 1:]))


# ---------------------------------------------------------------- ConstantMedium boundaries
DUP_BOX = ((-1.0, 0.0, -1.0), (1.0, 1.5, 1.0))


@functools.lru_cache(maxsize=None)
def _boundary_scene(name):
    """-> (blob, ops to world space, the boundary's local (lo, hi) box)."""
    sc = rt.Scene(41)
    w = sc.lambertian((0.7, 0.7, 0.7))
    ops, lo, hi = [], (-1, -1, -1), (1, 1, 1)
    if name == "sphere":
        b = sc.sphere((0, 0, 0), 1.0, w)
    elif name == "moving":
        b = sc.sphere_moving((0, 0, 0), (0, 0.5, 0), 1.0, w)
    elif name == "box":
        lo, hi = (-1, -0.5, -0.75), (1, 0.5, 0.75)
        b, ops = _chain(sc, sc.make_box(lo, hi, w), 2)
    elif name == "dupbox":  # the box of test_volume_boundary_one_walk: its top face twice
        a, c = DUP_BOX
        lo, hi = a, c
        faces = [sc.quad((a[0], a[1], c[2]), (2, 0, 0), (0, 1.5, 0), w),
                 sc.quad((c[0], a[1], c[2]), (0, 0, -2), (0, 1.5, 0), w),
                 sc.quad((c[0], a[1], a[2]), (-2, 0, 0), (0, 1.5, 0), w),
                 sc.quad((a[0], a[1], a[2]), (0, 0, 2), (0, 1.5, 0), w),
                 sc.quad((a[0], c[1], c[2]), (2, 0, 0), (0, 0, -2), w),
                 sc.quad((a[0], c[1], c[2]), (2, 0, 0), (0, 0, -2), w),
                 sc.quad((a[0], a[1], a[2]), (2, 0, 0), (0, 0, 2), w)]
        b = sc.rotate_y(sc.hittable_list(*faces), 25.0)
        ops = [("r", math.radians(25.0))]
    elif name == "quad":
        lo, hi = (-1, -1, 0), (1, 1, 0)
        b = sc.quad((-1, -1, 0), (2, 0, 0), (0, 2, 0), w)
    else:
        raise AssertionError(name)
    fog = sc.constant_medium(b, 0.9, (0.9, 0.9, 0.9))
    blob = sc.serialize(sc.hittable_list(sc.quad((-9, -3, -9), (18, 0, 0), (0, 0, 18), w), fog), None)
    return blob, ops, (np.array(lo, float), np.array(hi, float))


def _dir_world(ops, v):
    return _to_world(ops, v) - _to_world(ops, (0, 0, 0))


def _boundary_rays(name, seed, n=1024):
    """(rays [n, 7], class labels): through the body, from inside, clipping an edge or the rim
    (entry and exit within 1e-4), through the duplicated face, from 1e13 away, parallel to a
    face, missing."""
    _, ops, (lo, hi) = _boundary_scene(name)
    rng = np.random.default_rng(seed)
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    round_ = name in ("sphere", "moving")
    rays, labels = [], []
    for k in range(n):
        cls = ("through", "inside", "clip", "dup", "far", "parallel", "miss", "through")[k % 8]
        tm = float(rng.random())
        c = ctr + (np.array([0, 0.5 * tm, 0]) if name == "moving" else 0)
        u = _unit(rng)
        if cls == "through":
            target = c + half * rng.uniform(-0.9, 0.9, 3)
            o = target - u * rng.uniform(3, 9)
        elif cls == "inside":
            o = c + half * rng.uniform(-0.5, 0.5, 3)
        elif cls == "clip":
            if round_:  # the rim: impact parameter r (1 - 1e-10 x), a chord below 1e-4
                wv = np.cross(u, _unit(rng))
                wv /= np.linalg.norm(wv)
                o = c + wv * (1.0 - 1e-10 * rng.random()) - u * rng.uniform(3, 9)
            else:  # across an edge, 1e-6 inside it (for the single quad: across its border)
                ax = rng.integers(3)
                e1, e2 = (ax + 1) % 3, (ax + 2) % 3
                p = c + half * rng.uniform(-0.8, 0.8, 3)
                s1, s2 = rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])
                p[e1] = c[e1] + s1 * (half[e1] - 1e-6)
                p[e2] = c[e2] + s2 * (half[e2] - 1e-6)
                u = np.zeros(3)
                u[e1], u[e2] = s1, -s2
                u /= np.linalg.norm(u)
                o = p - u * rng.uniform(3, 9)
        elif cls == "dup":  # down through the top face
            target = c + half * rng.uniform(-0.8, 0.8, 3)
            u = np.array([rng.uniform(-0.3, 0.3), -1.0, rng.uniform(-0.3, 0.3)])
            o = target - u * rng.uniform(3, 6)
        elif cls == "far":
            target = c + half * rng.uniform(-0.5, 0.5, 3)
            o = target - u * 1e13
        elif cls == "parallel":
            ax = rng.integers(3)
            u[ax] = rng.choice([0.0, -0.0])
            u /= np.linalg.norm(u)
            target = c + half * rng.uniform(-0.9, 0.9, 3)
            o = target - u * rng.uniform(3, 9)
        else:
            target = c + half * 3.0 * rng.choice([-1.0, 1.0], 3) * rng.uniform(1.0, 2.0, 3)
            o = target - u * rng.uniform(3, 9)
            if abs(np.dot(c - o, u)) > 0:
                u = u - 0.0
        d = u * (1.0 if cls in ("clip", "far") else rng.uniform(0.5, 2.0))
        ow, dw = _to_world(ops, o), _dir_world(ops, d)
        if cls == "parallel" and not ops:
            dw = d  # keep the exact zero
        rays.append(list(ow) + list(dw) + [tm])
        labels.append(cls)
    return np.array(rays), np.array(labels)


@pytest.mark.parametrize("name", ["sphere", "moving", "box", "dupbox", "quad"])
def test_volume_two_hits_is_the_two_passes(gpu_available, name):
    """volume_two_hits (one walk) against the two traverse passes volume_hit falls back to, on
    every ray, bit for bit: `both`, t1 and t2 wherever `fallback` is not set. Under `fallback` the
    caller reruns the second query (the walk's contract), so there the walk's `both` only says
    that a first hit exists, t1 is the first pass's bit for bit, and the two passes give both
    and t2."""
    blob, _, _ = _boundary_scene(name)
    recs = P.scene_records(blob)
    vol = recs[recs[:, 1] == P.RTL_VOLUME]
    kind = P.RTL_VOLF_SPHERE if name in ("sphere", "moving") else P.RTL_VOLF_QUADS
    assert len(vol) == 1 and vol[0, 2] & 3 == kind and vol[0, 4] == -1
    rays, labels = _boundary_rays(name, 500 + len(name))
    g = P.volume_bounds(blob, int(vol[0, 0]), rays)
    both, t1, t2, fb, hit1, both2, p1, p2 = (g[:, k] for k in range(8))
    fbm = fb > 0
    assert np.array_equal(both[~fbm], both2[~fbm]), np.nonzero(both[~fbm] != both2[~fbm])[0][:5]
    ok = (both > 0) & ~fbm
    assert np.array_equal(_bits(t1[ok]), _bits(p1[ok])) and np.array_equal(_bits(t2[ok]), _bits(p2[ok]))
    assert np.array_equal(both[fbm], hit1[fbm]) and (both[fbm] == 1).all()
    assert np.array_equal(_bits(t1[fbm]), _bits(p1[fbm]))
    assert (both2[fbm & (both2 > 0)] <= both[fbm & (both2 > 0)]).all()
    h1 = hit1 > 0
    cls = {c: labels == c for c in set(labels.tolist())}
    seen = {
        "through": int((cls["through"] & (both2 > 0) & (p2 - p1 > 1e-4)).sum()),
        "inside": int((cls["inside"] & (both2 > 0) & (p1 < 0)).sum()),
        "clip": int((cls["clip"] & h1 & (both2 == 0)).sum()),
        "far": int((cls["far"] & h1 & (p1 + 1e-4 == p1)).sum()),
        "parallel": int((cls["parallel"] & ((rays[:, 3:6] == 0).any(axis=1) | bool(name != "quad"))).sum()),
        "miss": int((cls["miss"] & ~h1).sum()),
        "dup": int((cls["dup"] & fbm & (both2 > 0)).sum()),
        "fallback": int(fbm.sum()),
        "fallback, no third candidate": int((fbm & (both2 == 0)).sum()),
    }
    print(f"volume_two_hits[{name}]: {len(rays)} rays, {int((both2 > 0).sum())} with both hits; " +
          ", ".join(f"{k} {v}" for k, v in seen.items()))
    need = ["far", "miss", "parallel", "clip"]
    if name != "quad":  # one quad has one candidate: no body to go through or to be inside of
        need += ["through", "inside"]
    if name == "dupbox":
        need += ["dup", "fallback"]
    for k in need:
        assert seen[k] > 0, (name, k, seen)
    if name in ("sphere", "moving"):
        assert seen["fallback"] == 0  # two roots: the walk never needs a third candidate


# ---------------------------------------------------------------- the light-list PDF
LIGHT_QUAD = ((-1, 4, -1), (2, 0, 0), (0, 0, 2))
LIGHT_GQUAD = ((-1, 4, -1), (2, 0.5, 0), (0, 0.25, 2))
LIGHT_LISTS = ["aquad", "gquad", "sphere", "spheres2", "quad_sphere", "single", "nested", "other",
               "far_sphere"]


@functools.lru_cache(maxsize=None)
def _light_scene(name):
    sc = rt.Scene(51)
    w = sc.lambertian((0.7, 0.7, 0.7))
    li = sc.diffuse_light((5, 5, 5))
    ball, ball2 = ((0.5, 2.0, 0.25), 0.5), ((-2.0, 1.0, 1.0), 0.75)
    if name == "aquad":
        lights = sc.hittable_list(sc.quad(*LIGHT_QUAD, li))
    elif name == "gquad":
        lights = sc.hittable_list(sc.quad(*LIGHT_GQUAD, li))
    elif name == "sphere":
        lights = sc.hittable_list(sc.sphere(*ball, li))
    elif name == "spheres2":
        lights = sc.hittable_list(sc.sphere(*ball, li), sc.sphere(*ball2, li))
    elif name == "quad_sphere":
        lights = sc.hittable_list(sc.quad(*LIGHT_QUAD, li), sc.sphere(*ball, li))
    elif name == "single":
        lights = sc.quad(*LIGHT_QUAD, li)
    elif name == "nested":  # RTL_LIGHT_NEST = 4 lists below the top-level one
        lights = sc.hittable_list(sc.quad(*LIGHT_GQUAD, li), sc.sphere(*ball2, li))
        for k in range(4):
            extra = sc.sphere(*ball, li) if k == 1 else sc.quad((-1 + k, 4 + 0.25 * k, -1), (1, 0, 0), (0, 0, 1), li)
            lights = sc.hittable_list(extra, lights)
    elif name == "other":  # a Translate is no quad, sphere or list: Object::pdf_value's default arm
        lights = sc.hittable_list(sc.quad(*LIGHT_QUAD, li),
                                  sc.translate(sc.quad((2, 3, 0), (1, 0, 0), (0, 0, 1), li), (0.5, 0, 0)))
    elif name == "far_sphere":  # (r / dist)^2 ~ 1.5e-9: cos_theta_max within 2^-30 of 1 from every origin
        lights = sc.hittable_list(sc.sphere((0.5, 400.0, 0.25), 0.0156, li))
    else:
        raise AssertionError(name)
    world = sc.hittable_list(sc.quad((-5, 0, -5), (10, 0, 0), (0, 0, 10), w))
    return sc.serialize(world, lights)


def _light_leaves(node, out):
    if node["tag"] == OBJ_LIST:
        for k in node["kids"]:
            _light_leaves(k, out)
    elif node["tag"] in (OBJ_QUAD, OBJ_SPHERE):
        out.append(node)
    return out


def _light_records(name, seed, n_dirs=176):
    """origins x directions -> (records [n, 7] with cos_sl0, origin index per record)."""
    blob = _light_scene(name)
    root = _lights(blob)
    leaves = _light_leaves(root, [])
    spheres = [nd for nd in leaves if nd["tag"] == OBJ_SPHERE]
    rng = np.random.default_rng(seed)
    origins = [(0.0, 0.5, 0.0), (3.0, 0.25, -2.0), (-4.0, 1.0, 3.0), (0.25, 3.0, 0.5), (0.0, 6.0, 0.0),
               (6.0, 4.5, 6.0)]
    if spheres and name != "far_sphere":  # inside the first and the last sphere light
        for nd in (spheres[0], spheres[-1]):
            origins.append(tuple((np.array(nd["c"]) + 0.4 * nd["r"] * _unit(rng)).tolist()))
    recs, oi = [], []
    for i, o in enumerate(origins):
        o = np.array(o)
        cos0 = math.nan
        if spheres:  # object.rs:196 in IEEE f64, as the caller of light_pdf hands it over
            s0 = spheres[0]
            cmo = [s0["c"][k] - o[k] for k in range(3)]
            with np.errstate(invalid="ignore"):
                cos0 = float(np.sqrt(np.float64(1.0 - s0["r"] * s0["r"] / ((cmo[0] * cmo[0] + cmo[1] * cmo[1]) + cmo[2] * cmo[2]))))
        for k in range(n_dirs):
            nd = leaves[rng.integers(len(leaves))]
            if nd["tag"] == OBJ_QUAD:
                a, b = rng.uniform(-0.2, 1.2, 2)
                if k % 8 == 1:  # at an edge, just inside or outside
                    a = rng.choice([0.0, 1.0]) + rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-7, -3)
                target = np.array(nd["q"]) + a * np.array(nd["u"]) + b * np.array(nd["v"])
                nrm = np.array(nd["n"])
            else:
                spread = 1.3 * rng.random() ** (1 / 3)
                if name == "far_sphere":
                    # disc / half_b^2 <= (r / dist)^2 lies in the guard band's 1e-9 unless the ray
                    # passes well inside the rim or well outside it: aim there
                    spread = 0.4 * rng.random() if rng.random() < 0.6 else rng.uniform(2.0, 4.0)
                side = _unit(rng)
                if name == "far_sphere":  # across the line of sight: spread r is the impact parameter
                    side = np.cross(np.array(nd["c"]) - o, side)
                    side /= np.linalg.norm(side)
                target = np.array(nd["c"]) + nd["r"] * spread * side
                nrm = None
            v = target - o
            cls = k % 8
            if cls == 2:
                d = -v
            elif cls == 3 and nrm is not None and np.dot(nrm, v) != 0:  # |n . d| on both sides of 1e-8
                d = v * (1e-8 * rng.choice([0.5, 0.9, 1.1, 2.0]) / abs(np.dot(nrm, v)))
            elif cls == 4:  # t on both sides of 0.001
                d = v * rng.choice([500.0, 900.0, 1100.0, 2000.0])
            elif cls == 5:
                d = _unit(rng)
            else:
                d = v * rng.uniform(0.3, 3.0)
            recs.append(list(o) + list(d) + [cos0])
            oi.append(i)
    return np.array(recs), np.array(oi), origins


def _pdf_f32(node, o, d, hits, cos0, first_sphere):
    """The light object's pdf_value in plain float32 on the exact hit decisions and f64 hit t
    (object.rs:190-202, 492-501; hittable.rs:115-124)."""
    f = np.float32
    if node["tag"] == OBJ_LIST:
        tot = None
        for k in node["kids"]:
            pv = _pdf_f32(k, o, d, hits, cos0, first_sphere)
            tot = pv if tot is None else f(tot + pv)
        return f(tot * f(1.0 / len(node["kids"])))
    t = hits.get(id(node))
    if t is None:
        return f(0)
    if node["tag"] == OBJ_QUAD:
        d32, n32 = [f(x) for x in d], [f(x) for x in node["n"]]
        l32 = f(f(d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2])
        dn = f(f(d32[0] * n32[0] + d32[1] * n32[1]) + d32[2] * n32[2])
        t32 = f(float(_m(t)))
        with np.errstate(all="ignore"):
            return f(f(f(t32 * t32) * l32) / f(abs(f(dn / np.sqrt(l32))) * f(node["area"])))
    cmo = [node["c"][k] - o[k] for k in range(3)]
    with np.errstate(invalid="ignore"):
        cm = cos0 if node is first_sphere else float(np.sqrt(np.float64(
            1.0 - node["r"] * node["r"] / ((cmo[0] * cmo[0] + cmo[1] * cmo[1]) + cmo[2] * cmo[2]))))
    with np.errstate(all="ignore"):
        return f(f(1) / f(f(f(2) * f(math.pi)) * f(f(1) - f(cm))))


@functools.lru_cache(maxsize=None)
def _light_reference(name):
    """No GPU: records, the oracle's f64 values, the exact zero / non-zero decision and guard per
    record, the float32 restatement; asserts the oracle's decisions and the set's shape."""
    blob = _light_scene(name)
    recs, oi, origins = _light_records(name, 600 + LIGHT_LISTS.index(name))
    root = _lights(blob)
    leaves = _light_leaves(root, [])
    first_sphere = next((nd for nd in leaves if nd["tag"] == OBJ_SPHERE), None)
    ora = np.zeros(len(recs))
    for i, o in enumerate(origins):
        sel = np.nonzero(oi == i)[0]
        ora[sel] = O.light_pdf_batch(blob, o, recs[sel, 3:6])
    nonzero, guard, f32 = [], [], []
    for r in recs.tolist():
        cx = _Ctx(0.0)
        o, d = _fr(r[0:3]), _fr(r[3:6])
        hits = {}
        for nd in leaves:
            t = (_quad_x if nd["tag"] == OBJ_QUAD else _sphere_x)(cx, nd, o, d, Fr(0.001), INF)
            if t is not None:
                hits[id(nd)] = t
        nonzero.append(bool(hits))
        guard.append(cx.guard)
        f32.append(float(_pdf_f32(root, r[0:3], r[3:6], hits, r[6], first_sphere)))
    nonzero, guard, f32 = np.array(nonzero), np.array(guard), np.array(f32)
    keep = ~guard
    assert np.array_equal((ora != 0)[keep], nonzero[keep]), ("oracle", name)
    share = guard.mean()
    assert share <= 0.01, (name, share)
    assert 0.2 * len(recs) <= nonzero[keep].sum() <= 0.8 * len(recs), (name, int(nonzero.sum()))
    return recs, ora, nonzero, guard, f32, share


def _rel_err(x, ref):
    with np.errstate(all="ignore"):
        e = np.abs(x / ref - 1.0)
    return float(e.max()) if len(e) else 0.0


@pytest.mark.parametrize("name", LIGHT_LISTS)
def test_light_pdf(gpu_available, name):
    """light_pdf<true> (the root test) and light_pdf<false> (the root-free sphere predicate)
    against oracle_light_pdf_batch: a zero is an exact zero and the reverse, a NaN (an origin
    inside a sphere light) is a NaN, the two builds agree, non-zero values by the f32 rule."""
    blob = _light_scene(name)
    recs, ora, nonzero, guard, f32, share = _light_reference(name)
    got = P.scene_run("light_pdf", blob, recs)
    keep = ~guard
    n_nan = int(np.isnan(ora[keep]).sum())
    for col, build in ((0, "light_pdf<true>"), (1, "light_pdf<false>")):
        g = got[keep, col]
        assert np.array_equal(g != 0, nonzero[keep]), (name, build, np.nonzero((g != 0) != nonzero[keep])[0][:5])
        assert np.array_equal(np.isnan(g), np.isnan(ora[keep])), (name, build)
        assert (g[~np.isnan(g)] >= 0).all()
    assert np.array_equal(got[keep, 0], got[keep, 1], equal_nan=True), name
    val = keep & nonzero & np.isfinite(ora)
    # the far sphere's cos_theta_max rounds to 1 in float32 (the restatement divides by zero):
    # it is held to the bound of the ordinary sphere list, as sphere_light_w near 1 is
    bound_from = "sphere" if name == "far_sphere" else name
    if bound_from != name:
        r2 = _light_reference(bound_from)
        v2 = ~r2[3] & r2[2] & np.isfinite(r2[1])
        ref_w = _rel_err(r2[4][v2], r2[1][v2])
        assert np.isfinite(got[val, 0]).all() and (1.0 - recs[val, 6] < 2.0 ** -30).all()
    else:
        ref_w = _rel_err(f32[val], ora[val])
    print(f"light_pdf[{name}]: {len(recs)} records, {int(nonzero[keep].sum())} non-zero, {n_nan} NaN, "
          f"guard band leaves out {100 * share:.2f} %")
    _rule(f"light_pdf[{name}] (relative)", _rel_err(got[val, 0], ora[val]), ref_w)
    if name in ("sphere", "spheres2", "quad_sphere", "nested"):
        assert n_nan > 0


# ---------------------------------------------------------------- textures
from test_device_primitives_gpu import _turb_f32  # noqa: E402

IMAGE_SHAPES = [(1, 1), (1, 7), (7, 1), (37, 53)]  # (W, H)


@functools.lru_cache(maxsize=None)
def _texture_scene():
    """Every texture under test in one blob -> (blob, ids by name, the images)."""
    sc = rt.Scene(61)
    ids, imgs = {}, {}
    col = [sc.solid_color((0.1 * k, 1.0 - 0.1 * k, 0.03125 * k)) for k in range(8)]
    ids["solid"] = col[3]
    # a checker of checkers, three deep, dyadic scales: cell edges at multiples of 0.25, 0.5 and 1
    lvl2 = [sc.checker_texture(0.25, col[2 * k], col[2 * k + 1]) for k in range(4)]
    lvl1 = [sc.checker_texture(0.5, lvl2[0], lvl2[1]), sc.checker_texture(0.5, lvl2[2], lvl2[3])]
    ids["checker3"] = sc.checker_texture(1.0, lvl1[0], lvl1[1])
    ids["checker_0.3"] = sc.checker_texture(0.3, col[0], col[5])
    ids["checker_1e-10"] = sc.checker_texture(1e-10, col[1], col[6])  # test_saturating_texture_coordinates
    rng = np.random.default_rng(62)
    for w, h in IMAGE_SHAPES:
        imgs[(w, h)] = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        ids[f"image{w}x{h}"] = sc.image_texture(imgs[(w, h)])
    ids["noise4"] = sc.noise_texture(4.0)
    ids["noise0.35"] = sc.noise_texture(0.35)
    names = ["solid", "checker3", "checker_0.3", "checker_1e-10"] + [f"image{w}x{h}" for w, h in IMAGE_SHAPES] + [
        "noise4", "noise0.35"]
    balls = [sc.sphere((3.0 * k, 0, 0), 1.0, sc.lambertian(tex=ids[n])) for k, n in enumerate(names)]
    blob = sc.serialize(sc.hittable_list(*balls), None)
    # the serialiser numbers the textures itself: ball k's material names texture `names[k]`
    s = blob.slots
    for nd, n in zip(_world(blob)["kids"], names):
        ids[n] = int(s[int(s[6]) + 8 * nd["mat"] + 1])
    assert len(set(ids.values())) == len(names)
    return blob, ids, imgs


def _ulp_sides(x):
    return [math.nextafter(x, -INF), x, math.nextafter(x, INF)]


def _tex_run(blob, tex, uvp):
    """device (both Perlin-table paths, which must agree bit for bit) and oracle RGB."""
    uvp = np.ascontiguousarray(uvp, np.float64).reshape(-1, 5)
    got = P.scene_run("tex_value", blob, np.concatenate([np.full((len(uvp), 1), float(tex)), uvp], 1))
    assert np.array_equal(_bits(got[:, 0:3]), _bits(got[:, 3:6])), tex
    return got[:, 0:3], O.tex_value_batch(blob, tex, uvp)


def test_tex_value_solid_and_checkers_are_exact(gpu_available):
    blob, ids, _ = _texture_scene()
    rng = np.random.default_rng(700)
    pts = [rng.uniform(-3, 3, (512, 3)), rng.uniform(-300, 0, (256, 3))]  # negative coordinates too
    # exactly on and one ulp either side of a cell edge of each level, in each axis
    edge = []
    for ax in range(3):
        for e in (0.0, 0.25, -0.25, 0.5, -0.5, 0.75, 1.0, -1.0, 1.25, -2.0, 2.5, 16.25):
            for x in _ulp_sides(e):
                p = rng.uniform(-2, 2, 3)
                p[ax] = x
                edge.append(p)
    # a checker on its own discontinuity planes: every coordinate on an edge
    for e in (0.0, -0.0, 0.25, -0.5, 1.0):
        edge.append([e, e, e])
    pts = np.concatenate(pts + [np.array(edge)])
    uvp = np.concatenate([np.zeros((len(pts), 2)), pts], 1)
    g, r = _tex_run(blob, ids["solid"], uvp[:8])
    assert np.array_equal(_bits(g), _bits(r)) and np.array_equal(g, np.tile([0.1 * 3, 1.0 - 0.1 * 3, 0.03125 * 3], (8, 1)))
    # the dyadic checker: inv_scale p is exact, so the cell is floor() of an exact product
    g, r = _tex_run(blob, ids["checker3"], uvp)
    assert np.array_equal(_bits(g), _bits(r))
    want = []
    for p in pts.tolist():
        par = lambda inv: sum(math.floor(Fr(inv) * Fr(x)) for x in p) & 1  # noqa: E731
        a, b, c = par(1), par(2), par(4)
        k = 4 * a + 2 * b + c  # lvl1[a] -> its lvl2[b] -> colour c
        want.append([0.1 * k, 1.0 - 0.1 * k, 0.03125 * k])
    assert np.array_equal(g, np.array(want))
    assert len({tuple(x) for x in g.tolist()}) == 8  # every leaf colour of the three levels occurs
    # scale 0.3: both sides form fl(inv_scale p) with one f64 product, so they agree on every point
    g, r = _tex_run(blob, ids["checker_0.3"], uvp)
    assert np.array_equal(_bits(g), _bits(r)) and len({tuple(x) for x in g.tolist()}) == 2
    # scale 1e-10: floor(1e10 p) saturates the i32 conversion for |p| >= 1 and does not below 0.2
    sat = np.concatenate([pts, rng.uniform(-0.2, 0.2, (256, 3)), [[1.0, -1.0, 1.0], [0.3, 1e300, -1e300],
                                                                   [INF, 0.0, 0.0], [-INF, -INF, 0.5]]])
    g, r = _tex_run(blob, ids["checker_1e-10"], np.concatenate([np.zeros((len(sat), 2)), sat], 1))
    assert np.array_equal(_bits(g), _bits(r)) and len({tuple(x) for x in g.tolist()}) == 2
    print(f"tex_value: solid and 4 checkers, {len(pts) + len(sat)} points, equal to the oracle bit for bit")


@pytest.mark.parametrize("shape", IMAGE_SHAPES)
def test_tex_value_image_is_exact(gpu_available, shape):
    """texture.rs:95-107 and rt_image.rs:37-46: clamp, i = (u W) as u32, j = (v H) as u32, x = min(i,
    W - 1), y = H - j - 1 clamped to H - 1 (at v = 1 the u32 difference wraps and the clamp gives
    the bottom row)."""
    blob, ids, imgs = _texture_scene()
    w, h = shape
    img = imgs[shape]
    rng = np.random.default_rng(710 + w)
    special = [-0.5, 0.0, -0.0, math.nextafter(1.0, 0.0), 1.0, 1.5, 0.5, 1.0 / w, 1.0 / h]
    uv = [(a, b) for a in special for b in special] + rng.uniform(-0.1, 1.1, (512, 2)).tolist()
    uvp = np.array([[a, b, 0.0, 0.0, 0.0] for a, b in uv])
    g, r = _tex_run(blob, ids[f"image{w}x{h}"], uvp)
    want, rows = [], set()
    for a, b in uv:
        cu, cv = min(max(a, 0.0), 1.0), min(max(b, 0.0), 1.0)
        i, j = int(cu * float(w)), int(cv * float(h))
        x = min(i, w - 1)
        y = h - j - 1
        y = h - 1 if y < 0 else min(y, h - 1)
        rows.add(y)
        want.append([float(c) * (1.0 / 255.0) for c in img[y, x]])
    assert np.array_equal(_bits(g), _bits(np.array(want))) and np.array_equal(_bits(r), _bits(np.array(want)))
    assert {0, h - 1} <= rows and len(rows) >= min(h, 7)  # the top and the bottom row both occur
    print(f"tex_value image {w}x{h}: {len(uv)} lookups, the texels exactly")


def _perlin_tables(blob, k):
    s = blob.slots
    base = int(s[8]) + 1536 * k
    ranvec = s[base:base + 768].view(np.float64).reshape(256, 3).copy()
    perms = s[base + 768:base + 1536].astype(np.int32).reshape(3, 256).copy()
    return ranvec, perms


def test_tex_value_noise(gpu_available):
    """texture.rs:127-130: 0.5 (1 + sin(s z + 10 turb(s p))) of two noise textures with their own
    Perlin tables and scales; the turbulence is an f32 weight on the device."""
    blob, ids, _ = _texture_scene()
    assert blob.header()["n_perlin"] == 2
    rng = np.random.default_rng(720)
    pts = np.concatenate([rng.uniform(-3, 3, (768, 3)), rng.uniform(-300, 300, (256, 3))])
    uvp = np.concatenate([np.zeros((len(pts), 2)), pts], 1)
    for k, (name, scale) in enumerate((("noise4", 4.0), ("noise0.35", 0.35))):
        g, r = _tex_run(blob, ids[name], uvp)
        assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 0], g[:, 2])
        assert (g >= 0).all() and (g <= 1).all() and g[:, 0].std() > 0.05
        sp = pts * scale
        table = int(blob.slots[int(blob.slots[4]) + 8 * ids[name] + 2])  # the texture's Perlin index
        assert table in (0, 1)
        t32 = _turb_f32(*_perlin_tables(blob, table), sp).astype(np.float64)
        f32 = 0.5 * (1.0 + np.sin(10.0 * t32 + sp[:, 2]))
        _rule(f"tex_value {name} (absolute)", float(np.abs(g[:, 0] - r[:, 0]).max()),
              float(np.abs(f32 - r[:, 0]).max()))
