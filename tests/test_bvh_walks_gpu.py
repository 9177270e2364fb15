"""The ordered BVH walkers of rt_kernel.h (cbvh_walk_t, obvh_walk, obvh_leaf, bvh_subtree), ray by
ray against the reference-order walk.

The render tests reach these walks only with camera rays and unit-length scattered rays, and
compare pixels. Here one thread runs one ray through the compact tree in LDS (cbvh_walk), the
octant streams in global memory (obvh_walk) and the reference tree in the reference order
(traverse over [node, skip)), through the scene probe's bvh_walks entry; world_hit_bvh runs the
whole world query as the BVH kernels do (bvh_subtree's ballot and re-walk, instances, a
ConstantMedium with a BVH boundary), once as the product build and once as the COUNT build.

Scenes (rt.Scene, seeded, every tree 64 leaves or fewer): `mixed` (spheres of radius 0.02-0.9, two
moving, axis-aligned and general quads, three make_box), `ties` (dyadic: eight boxes in a row whose
faces touch, a sphere twice with two materials, two coplanar overlapping quads), `lattice` (a 4 x 4
grid of dyadic boxes with shared heights, spheres in the empty cells), `deep` (48 spheres in a row,
each 1.3 times the last: a compact tree 13 levels deep where a balanced one has 6), `instance`
(Translate(RotateY(BVH of 24 spheres)) beside a top-level BVH of 12 items and a plain sphere),
`fog_bvh` (two ConstantMediums whose boundaries are a BVH of make_box's sides and a BVH of eight
overlapping spheres, between opaque quads), `ineligible` (a BVH with a Translate among its leaves:
no ordered BVH, only the reference tree), `near_ties` (twelve pairs of spheres that touch from
inside at a pole, whose z agrees to within rounding only; rays up the common axis).

Ray classes, a fixed share of each set: aimed inside and just outside leaves from outside the
scene; bounce rays from the oracle's own hit point (tmin 1e-4); an origin inside a make_box leaf,
inside a sphere; one and two components of d exactly +-0 through a target, in `ties` and `lattice`
also with the origin's coordinate on a shared face plane (a NaN slab time); one component of d of
magnitude 1e-45..1e-39 (its f32 reciprocal overflows); |d| of 1e-3 and 1e3; an origin 1e6 and 1e13
away; a finite tmax at 0.5-1.5 times the first hit; in `ties` a tmax equal to a candidate; tmin =
1e3 with hits beyond it; for the boundary form tmin = -inf from inside, from outside and pointing
away from the whole scene, then tmin = t1 + 1e-4.

(a) test_ordered_walks_are_the_reference_walk: no tolerance. Where a walk's tie flag is clear its
    (hit, t bits, hit node) are the reference-order walk's, with MAIN = true and MAIN = false; the
    streams walk's flag implies the LDS walk's; in `ties` every ray whose two smallest values of
    {tmax, exact candidates} are equal is flagged by both. The flagged share is printed, not capped.
(b) test_product_walk_is_the_count_walk: world_hit_bvh's product half and COUNT half are equal bit
    for bit (hit, t, node, frame, material word, generator state), and equal to (a)'s
    reference-order result where the world is the one tree.
(c) test_reference_walk_against_exact_arithmetic: the rules of tests/test_scene_functions_gpu.py.
    In exact arithmetic a BvhNode is the list of its leaves; whenever the two smallest candidates
    lie within a relative 1e-9 the ray joins the guard band (the reference's tree order decides
    there). Outside it the f64 oracle and the device take the exact decision (hit, primitive,
    material) and the device's worst t error is at most twice the oracle's. 512 rays per scene;
    the classes without an exact reference of their own (1e13 away, |d_a| < 1e-39), the origins
    1e6 away (a sphere's discriminant is then below 1e-9 of its own terms: every such decision
    lies inside the band; in `deep`, whose radii span 1e8, so does every origin outside the scene,
    and its rays start 2 to 9 target radii from their target) and the ones that are exact ties by
    construction (an origin on a shared plane, tmax equal to a candidate; in `ties` and `lattice`
    every ray that leaves a box through a face it shares: an origin inside a box, a bounce into
    one, tmin = 1e3 behind an entry; in `ties` also targets on the duplicated sphere and the
    coplanar quads) are left to (a) and (b). The oracle walks the reference's tree with Aabb::hit in f64;
    it agrees with the list semantics on every ray outside the band, so the exact walker needs no
    box test of its own: a box the reference culls holds no candidate (the reference's Aabb of a
    primitive contains it; that is the flattener's condition for an ordered BVH, rt_flatten.hpp
    PrimBox::ref_complete, and _general_uv keeps the general quads inside it), except where the ray grazes the box within its padding, which is inside the band.

Ill-conditioned rays. _ill() sets aside the rays whose origin lies further than 2^26 radii from a
leaf (the origins 1e13 away; in `deep` also five of the origins 1e6 away): r^2 is then below half an
ulp of the terms of a sphere's discriminant (and a quad's hit point is off by more than the quad),
so rounding decides the candidate. The same assertions run on them in tests of their own,
test_ordered_walks_on_ill_conditioned_rays and test_product_walk_on_ill_conditioned_rays.

FINDING (fixed in rt_kernel.h: obvh_far). On ill-conditioned rays a leaf test can report a hit for a
ray that passes the leaf at a distance. The reference tree never runs that test: its f64 boxes cull
the leaf. The ordered walks' f32 boxes cannot (at 1e13 an f32 ulp is 1e6, and the kBoxRel widening
is relative to t), so they tested the leaf, took its closer t and left the flag clear. With the
flag clear the LDS walk differed from the reference-order walk on 31 / 71 / 12 / 44 and the streams
walk on 70 / 88 / 50 / 75 of the 128 / 128 / 133 / 128 such rays of `mixed` / `lattice` / `deep` /
`instance`; the product half differed from the COUNT half on 31 / 71 / 12 / 52 / 35 (`fog_bvh`
last); `near_ties`: 24 and 73 of 128. The first failing ray of `mixed`: o = (-5016111379796.734,
-2939577580871.0527, 8136185240735.941), d = (0.5272004347865259, 0.30895378140210344,
-0.855124631738418), time 0.83, tmin 1e-4, tmax inf: both ordered walks hit record 2432 at t =
9514619034880.258, flag clear; the reference-order walk misses. Neither answer means anything
geometrically and no camera or scattered ray is in that regime, but it contradicted "the result is
the reference order's" (rt_kernel.h, the comment above kTieRel). Both walks now end with obvh_far,
once per walk that hits: the winning record is read again and the lane is flagged when that
record's own test carries more rounding noise than 2^-12 of the primitive (a sphere further than
2^20 radii from the origin; a quad whose planar coordinates carry 2^-52 (|o| + t |d|) (|A| + |B|) >
2^-12), so the reference order decides there. With it both tests pass in every scene (0 rays
differ), and every hit from 1e13 away and the hits on spheres of radius below 0.95 from 1e6 away are
flagged (the shares below).

Measured on an MI355X (the same table stands in DESIGN.md section 2):
  (c) t, device worst / oracle worst (bound: a factor 2), 512 rays per scene; hits; guard band:
    mixed     1.173e-13 / 1.316e-13   313 hits  0.00 %     ties       1.095e-16 / 1.095e-16  326 hits  0.20 %
    lattice   1.836e-14 / 1.669e-14   380 hits  0.00 %     deep       1.218e-14 / 3.263e-14  340 hits  0.00 %
    instance  4.873e-14 / 6.065e-14   333 hits  0.00 %     fog_bvh    8.888e-15 / 1.106e-14  257 hits  0.00 %
    ineligible 5.631e-14 / 4.657e-14  308 hits  0.00 %     near_ties  2.711e-14 / 3.206e-14  377 hits  0.00 %
    fog_bvh: 175 draws, 58 hits in a medium. The CPU-only run (exact arithmetic and the oracle, no
    GPU) gives the same hits and guard shares. The oracle and the list semantics disagree on no
    ray outside the band.
  (a) flagged for the reference-order re-walk, LDS walk / streams walk, of 2048 rays:
    mixed 8.50 % / 8.50 %, instance 8.74 % / 8.74 %: far13 128 and 126 of 128, far6 46 and 53 of 128;
      every other class 0
    deep 10.50 % / 10.50 %: far13 126, far6 29, aim 28 of 640, long 10, tiny 8, short 6, zero2 4,
      zero1 2, tmax 1, tmin1e3 1 (its radii span 3e5: a ray that starts beside a large sphere and hits
      a small one is further than 2^20 radii from it)
    ties 33.20 % / 33.20 %: tmax_eq 128 of 128, in_sphere 128, plane 127, far13 99, in_box 40, aim 33 of
      256, bounce 26, tiny 18, zero2 17, far6 14, tmin1e3 13, long 12, zero1 11, short 9, tmax 5;
      195 of the 683 rays decided in exact arithmetic tie exactly, all flagged by both walks
    lattice 13.28 % / 13.23 %: far13 120, plane 58, in_box 34, bounce 24, far6 14 / 13, tmin1e3 7, aim 5
      of 384, zero1 4, tiny 3, zero2 2, tmax 1
    near_ties 12.50 % / 12.45 %: all 128 rays up a pair's axis (pole 128 of 256), far13 127, far6 1 / 0
    boundary form (512 + the first query's hits): no ray flagged but 25 of 256 from outside in ties,
      and 34 of 256 from outside and 18 of 128 pointing away in deep
  deep: compact tree depth 13 (a balanced tree of 48 leaves: 6), 52 B of stack per lane.
Mutations in a scratch copy of rt_kernel.h (with obvh_far in place):
  kBoxPos = 1.0f and kBoxRel = 0: test_ordered_walks_are_the_reference_walk[mixed, lattice, deep],
    test_product_walk_is_the_count_walk[mixed, lattice, deep, fog_bvh] and both ill-conditioned tests
    in every scene fail
  the bf16 entry time rounded up: test_ordered_walks_are_the_reference_walk[mixed, ties, lattice,
    near_ties] and test_product_walk_is_the_count_walk[mixed, ties, lattice, fog_bvh, near_ties] fail
  obvh_leaf's shortcut never testing the far sides: test_ordered_walks_are_the_reference_walk[mixed,
    ties, lattice, instance], test_product_walk_is_the_count_walk[the same four] and
    test_reference_walk_against_exact_arithmetic[mixed, ties, instance] fail
  kTieRel = 0: test_ordered_walks_are_the_reference_walk[near_ties] and
    test_product_walk_is_the_count_walk[near_ties] fail (17 rays up a pair's axis return the other
    sphere of the pair with the flag clear); no other scene notices, which is why `near_ties` exists
  close_f without its 2 kTieRel margin: NOT caught, by any scene. The margin is redundant as the
    code stands: (float) rounds closest by at most 2^-25 relative and the margin adds 2^-29, while
    every box test that reads close_f widens it by kBoxPos = 1 + 2^-18 (or kBoxRel = 2^-20 on both
    ends); a candidate within kTieRel = 2^-30 above closest lies in a box whose entry time passes
    either way. Only together with the first mutation could it matter.
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
from test_device_primitives_gpu import INF, M, _bits, _fr, _dot, _rng_py, _rule
from test_scene_functions_gpu import (OBJ_BVH, OBJ_LIST, OBJ_QUAD, OBJ_SPHERE, OBJ_VOLUME, _Ctx, _hit_x,
                                      _bvh_leaves, _keys, _m, _mats, _oracle_world, _prims, _rel,
                                      _sphere_roots, _unit, _world, _world_records)

pytestmark = pytest.mark.gpu

SCENES = ["mixed", "ties", "lattice", "deep", "instance", "fog_bvh", "ineligible", "near_ties"]
WALK_SCENES = ["mixed", "ties", "lattice", "deep", "instance", "near_ties"]  # a top-level root with an ordered BVH
N_AB, N_C, N_BOUNDARY = 2048, 512, 512
TIES_BOXES = [((float(k), 0.0, 0.0), (float(k + 1), 1.0, 1.0)) for k in range(8)]


# ---------------------------------------------------------------- scenes
def _general_uv(rng):
    """Edges of a general quad with u_a v_a >= 0 on every axis: the reference's Aabb of a quad spans
    q and q + u + v only (object.rs:427-431), and a subtree gets an ordered BVH only when that box
    holds the whole of every leaf (rt_flatten.hpp PrimBox::ref_complete)."""
    s = rng.choice([-1.0, 1.0], 3)
    return s * rng.uniform(0.2, 1.5, 3), s * rng.uniform(0.2, 1.5, 3)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """-> dict(blob, tg: (centre, radius) of every region rays are aimed at, c_tg: those of part
    (c), boxes: make_box leaves in world space, spheres: static spheres in world space, planes:
    (axis, coordinate, a point on the shared face, its half extent), ctr / rad: the scene's ball)."""
    sc = rt.Scene(61)
    rng = np.random.default_rng(6100 + SCENES.index(name))
    tg, boxes, spheres, planes, c_tg = [], [], [], [], None

    def sphere(c, r, m):
        tg.append((c, 1.5 * r)), spheres.append((c, r))
        return sc.sphere(c, r, m)

    def box(lo, hi, m):
        lo, hi = np.array(lo, float), np.array(hi, float)
        tg.append(((lo + hi) / 2, 0.6 * float(np.linalg.norm(hi - lo)))), boxes.append((lo, hi))
        return sc.make_box(tuple(lo), tuple(hi), m)

    def quad(q, u, v, m):
        q, u, v = (np.array(x, float) for x in (q, u, v))
        tg.append((q + (u + v) / 2, 0.6 * float(np.linalg.norm(u + v))))
        return sc.quad(tuple(q), tuple(u), tuple(v), m)

    if name == "mixed":
        m = _mats(sc, 8)
        it = [sphere(tuple(rng.uniform(0.5, 9.5, 3)), float(0.02 * 45.0 ** rng.random()), m[k % 8])
              for k in range(22)]
        for k in range(2):
            c = rng.uniform(1, 9, 3)
            it.append(sc.sphere_moving(tuple(c), tuple(c + rng.uniform(-0.5, 0.5, 3)), 0.4, m[k]))
            tg.append((c, 0.9))
        for k in range(5):  # axis-aligned quads
            a = k % 3
            u, v = np.zeros(3), np.zeros(3)
            u[(a + 1) % 3], v[(a + 2) % 3] = rng.uniform(0.5, 2.5, 2)
            it.append(quad(rng.uniform(0, 7.5, 3), u, v, m[k]))
        for k in range(4):  # general quads
            it.append(quad(rng.uniform(0, 7.5, 3), *_general_uv(rng), m[k + 3]))
        for k in range(3):
            lo = rng.uniform(0.5, 7.5, 3)
            it.append(box(lo, lo + rng.uniform(0.4, 2.0, 3), m[k + 5]))
        objs = [sc.create_bvh(sc.hittable_list(*it))]
    elif name == "ties":
        m = _mats(sc, 6)
        it = [box(lo, hi, m[k % 3]) for k, (lo, hi) in enumerate(TIES_BOXES)]
        c_tg = list(tg)  # part (c): the boxes from outside; the rest ties by construction
        # small and off to the sides, so that few rays aimed at the boxes cross them
        it += [sphere((2.0, 0.5, -6.0), 0.25, m[3]), sphere((2.0, 0.5, -6.0), 0.25, m[4])]
        it += [quad((5.0, 0.0, 8.0), (0.5, 0, 0), (0, 0.5, 0), m[4]), quad((5.25, 0.25, 8.0), (0.5, 0, 0), (0, 0.5, 0), m[5])]
        planes = [(0, float(k), np.array([float(k), 0.5, 0.5]), 0.375) for k in range(1, 8)]
        objs = [sc.create_bvh(sc.hittable_list(*it))]
    elif name == "lattice":
        m = _mats(sc, 4)
        it = []
        for i in range(4):
            for j in range(4):
                if (i + 2 * j) % 5 == 0:  # an empty cell: a sphere
                    it.append(sphere((i + 0.5, 0.25, j + 0.5), 0.25, m[(i + j) % 4]))
                else:
                    h = (0.5, 1.0, 1.5)[(3 * i + j) % 3]
                    it.append(box((float(i), 0.0, float(j)), (i + 1.0, h, j + 1.0), m[(i + j) % 4]))
        for k in range(1, 4):
            planes += [(0, float(k), np.array([float(k), 0.25, 1.5]), 0.125),
                       (2, float(k), np.array([2.5, 0.25, float(k)]), 0.125)]
        planes += [(1, h, np.array([2.0, h, 2.0]), 1.5) for h in (0.5, 1.0, 1.5)]  # the shared heights
        objs = [sc.create_bvh(sc.hittable_list(*it))]
    elif name == "deep":
        m = _mats(sc, 4)
        it, x = [], 0.0
        for k in range(48):
            r = 0.01 * 1.3 ** k
            x += 2.5 * r
            it.append(sphere((x, 0.0, 0.0), r, m[k % 4]))
            x += 2.5 * r
        objs = [sc.create_bvh(sc.hittable_list(*it))]
    elif name == "instance":
        m = _mats(sc, 6)
        inner = [sc.sphere(tuple(rng.uniform(-2, 2, 3)), float(rng.uniform(0.15, 0.6)), m[k % 6]) for k in range(24)]
        inst = sc.translate(sc.rotate_y(sc.create_bvh(sc.hittable_list(*inner)), 35.0), (8.0, 0.5, 0.0))
        tg.append((np.array([8.0, 0.5, 0.0]), 3.0))
        top = [sphere(tuple(rng.uniform(-2, 2, 3)), float(rng.uniform(0.15, 0.6)), m[k % 6]) for k in range(9)]
        top += [quad(rng.uniform(-2, 1, 3), *_general_uv(rng), m[k]) for k in range(2)]
        top.append(box((-0.5, -2.5, -0.5), (0.75, -1.5, 0.5), m[5]))
        objs = [inst, sc.create_bvh(sc.hittable_list(*top)), sphere((4.0, 3.0, 0.0), 0.8, m[0])]
    elif name == "fog_bvh":
        m = _mats(sc, 4)
        fog1 = sc.constant_medium(sc.create_bvh(sc.make_box((-1.0, -0.5, -0.75), (1.0, 0.5, 0.75), m[0])),
                                  0.9, (0.9, 0.9, 0.9))
        tg.append((np.zeros(3), 1.4)), boxes.append((np.array([-1.0, -0.5, -0.75]), np.array([1.0, 0.5, 0.75])))
        blobs = [sc.sphere(tuple(np.array([4.0, 0.0, 0.0]) + 0.5 * rng.uniform(-1, 1, 3)), 0.7, m[1]) for _ in range(8)]
        fog2 = sc.constant_medium(sc.create_bvh(sc.hittable_list(*blobs)), 0.7, (0.9, 0.9, 0.9))
        tg.append((np.array([4.0, 0.0, 0.0]), 1.4))
        objs = [quad((-3.0, -1.5, 1.5), (9.0, 0, 0), (0, 3.0, 0), m[2]), fog1, fog2,
                quad((-3.0, -1.5, -1.5), (9.0, 0, 0), (0, 3.0, 0), m[3])]
    elif name == "ineligible":
        m = _mats(sc, 4)
        it = [sphere(tuple(rng.uniform(-2, 2, 3)), float(rng.uniform(0.2, 0.6)), m[k % 4]) for k in range(7)]
        it.append(sc.translate(sc.sphere((0.0, 0.0, 0.0), 0.5, m[1]), (0.0, 3.0, 0.0)))
        tg.append((np.array([0.0, 3.0, 0.0]), 0.6))
        objs = [sc.create_bvh(sc.hittable_list(*it))]
    elif name == "near_ties":
        # twelve pairs of spheres, the smaller inside the larger and touching it at its pole z = 4:
        # c_z - r is 5 - 1 for one and fl(5 + a) - fl(1 + a) for the other, equal to within rounding
        # but (a is no dyadic number) mostly not equal. A ray up the pair's axis has two candidates
        # an ulp or so apart, and the reference tree's f64 box test of the second sphere compares
        # that box's entry time, not the sphere's root, with the first sphere's t.
        m = _mats(sc, 4)
        it = []
        for k in range(12):
            x, y, a = 12.0 * (k % 4), 12.0 * (k // 4), float(rng.uniform(0.3, 2.5))
            it += [sphere((x, y, 5.0), 1.0, m[k % 4]), sphere((x, y, 5.0 + a), 1.0 + a, m[(k + 1) % 4])]
        objs = [sc.create_bvh(sc.hittable_list(*it))]
    else:
        raise AssertionError(name)
    blob = sc.serialize(sc.hittable_list(*objs), None)
    tg = [(np.array(c, float), float(r)) for c, r in tg]
    pts = np.array([c for c, _ in tg])
    ctr = (pts.min(0) + pts.max(0)) / 2
    rad = float(max(np.linalg.norm(c - ctr) + r for c, r in tg))
    return dict(blob=blob, tg=tg, c_tg=[(np.array(c, float), float(r)) for c, r in c_tg] if c_tg else tg,
                boxes=boxes, spheres=spheres, planes=planes, ctr=ctr, rad=rad)


def _root(name):
    """The word offset of the scene's top-level BVH record that has an ordered BVH."""
    recs = P.scene_records(_scene(name)["blob"])
    top = recs[(recs[:, 1] == P.RTL_BVH) & (recs[:, 4] == -1) & (recs[:, 3] != 0)]
    assert len(top) == 1, (name, recs[recs[:, 1] == P.RTL_BVH])
    return int(top[0, 0])


# ---------------------------------------------------------------- rays
AB_CLASSES = ["aim", "bounce", "in_box", "in_sphere", "zero1", "zero2", "tiny", "short", "long", "far6",
              "far13", "tmax", "tmin1e3", "tmax_eq", "plane", "aim"]
TOUCHING = ("ties", "lattice")  # boxes whose faces touch: a ray that leaves a box ties by construction
NO_EXACT = ("far13", "tiny", "far6", "tmax_eq", "plane", "pole")  # part (c) leaves these to (a) and (b)


def _applies(name, cls, part):
    S = _scene(name)
    if part == "c" and (cls in NO_EXACT or (name in TOUCHING and cls in ("in_box", "tmin1e3")) or
                        (name == "ties" and cls == "in_sphere")):
        return False
    return {"in_box": bool(S["boxes"]), "in_sphere": bool(S["spheres"]), "plane": bool(S["planes"]),
            "tmax_eq": name == "ties", "pole": name == "near_ties"}.get(cls, True)


def _axis_ray(target, o, keep, fill):
    """A ray through `target` along the axes `keep`; the other components of d are fill()."""
    o2 = target.copy()
    for a in keep:
        o2[a] = o[a]
    d = np.array([(target - o2)[a] if a in keep else fill() for a in range(3)])
    if not any(d[a] != 0 for a in keep):
        d[keep[0]] = 1.0
    return o2, d


@functools.lru_cache(maxsize=None)
def _rays(name, seed, n, part):
    """Seeded rays [n, 9] (o3, d3, time, tmin, tmax) and their class labels."""
    S = _scene(name)
    blob, tg = S["blob"], (S["c_tg"] if part == "c" else S["tg"])
    rng = np.random.default_rng(seed)
    rays, labels = [], []
    for k in range(n):
        cls = AB_CLASSES[k % 16]
        if name == "near_ties" and cls in ("tmax_eq", "plane"):
            cls = "pole"
        if not _applies(name, cls, part):
            cls = "aim"
        c, r = tg[rng.integers(len(tg))]
        target = c + _unit(rng) * r * rng.random() ** (1 / 3)
        near = (k // 16) % 2 == 1
        if part == "c" and (name == "deep" or name in TOUCHING):
            near = name == "deep"
        if near:  # from 2 to 9 target radii away (in `ties` and `lattice` that may be inside a box)
            o = c + _unit(rng) * r * rng.uniform(2.0, 9.0)
        else:  # from outside the scene
            o = S["ctr"] + _unit(rng) * S["rad"] * rng.uniform(1.5, 3.0)
        d = (target - o) * rng.uniform(0.5, 2.0)
        tmin, tmax = 1e-4, INF
        if cls == "in_box":
            lo, hi = S["boxes"][rng.integers(len(S["boxes"]))]
            o, d = lo + (hi - lo) * rng.uniform(0.1, 0.9, 3), _unit(rng) * rng.uniform(0.5, 2.0)
        elif cls == "in_sphere":
            cs, rs = S["spheres"][rng.integers(len(S["spheres"]))]
            o, d = np.array(cs) + _unit(rng) * rs * 0.8 * rng.random() ** (1 / 3), _unit(rng) * rng.uniform(0.5, 2.0)
        elif cls in ("zero1", "zero2", "tiny"):
            ax = int(rng.integers(3))
            keep = [ax, (ax + 1) % 3] if cls == "zero2" else [ax]
            if cls == "tiny":
                keep = [ax, (ax + 1) % 3]
                fill = lambda: float(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-45, -39))  # noqa: E731
            else:
                fill = lambda: float(rng.choice([0.0, -0.0]))  # noqa: E731
            o, d = _axis_ray(target, o, keep, fill)
        elif cls == "plane":  # the origin's coordinate on a shared face plane, d's exactly +-0 there
            ax, x0, q, half = S["planes"][rng.integers(len(S["planes"]))]
            p = q.copy()
            for a in range(3):
                if a != ax:
                    p[a] += half * rng.uniform(-1, 1)
            others = [a for a in range(3) if a != ax]
            keep = [others[int(rng.integers(2))]] if k % 32 < 16 else others
            o, d = _axis_ray(p, o, keep, lambda: float(rng.choice([0.0, -0.0])))
            assert o[ax] == x0 and d[ax] == 0.0
        elif cls == "pole":  # up (or down) the common axis of a pair of touching spheres
            cs, _ = S["spheres"][2 * int(rng.integers(12))]
            up = k % 32 < 16
            o = np.array([cs[0], cs[1], rng.uniform(-3.0, 2.0) if up else rng.uniform(12.0, 20.0)])
            d = np.array([float(rng.choice([0.0, -0.0])), float(rng.choice([0.0, -0.0])),
                          rng.uniform(0.3, 3.0) * (1.0 if up else -1.0)])
        elif cls == "short":
            d = d / np.linalg.norm(d) * 1e-3
        elif cls == "long":
            d = d / np.linalg.norm(d) * 1e3
        elif cls in ("far6", "far13"):
            u = _unit(rng)
            o, d = target - u * (1e6 if cls == "far6" else 1e13), u * rng.uniform(0.5, 2.0)
        elif cls == "tmin1e3":
            d = d / np.linalg.norm(d) * float(np.linalg.norm(target - o)) / rng.uniform(500.0, 3000.0)
            tmin = 1e3
        elif cls == "tmax_eq":  # dyadic: along x through the row of boxes, tmax on a face's exact t
            y, z = (float(rng.integers(1, 8)) / 8 for _ in range(2))
            x0 = float(rng.choice([-2.0, -0.5, 1.5, 2.25, 4.5, 9.0, 10.5]))
            sgn = 1.0 if x0 < 4 else -1.0
            scale = float(rng.choice([0.5, 1.0, 2.0]))
            face = (math.floor(x0) + 1 if x0 >= 0 else 0) if sgn > 0 else (math.ceil(x0) - 1 if x0 <= 8 else 8)
            o, d = np.array([x0, y, z]), np.array([sgn * scale, float(rng.choice([0.0, -0.0])), 0.0])
            tmax = (face - x0) / (sgn * scale)
            assert tmax > 0 and Fr(tmax) * Fr(sgn * scale) + Fr(x0) == face
        tm = (0.0, 1.0, float(rng.random()))[k % 3]
        rays.append(list(o) + list(d) + [tm, tmin, tmax])
        labels.append(cls)
    rays, labels = np.array(rays), np.array(labels)
    # the oracle's first hits: a finite tmax around them, and bounce origins on a leaf (leaving at
    # |n . d| >= 0.2 |d|, the cut of test_scene_functions_gpu._world_rays, for its reason)
    first = O.world_hit_batch(blob, rays[:, :7], None, 1e-4, INF)
    src = np.nonzero((first[:, 0] > 0) & np.isin(labels, ("aim", "zero1", "short", "long")))[0]
    for k in np.nonzero(labels == "tmax")[0]:
        t0 = first[k, 1] if first[k, 0] > 0 else float(np.linalg.norm(tg[0][0] - rays[k, 0:3]) / np.linalg.norm(rays[k, 3:6]))
        rays[k, 8] = t0 * rng.uniform(0.5, 1.5)
    for k in np.nonzero(labels == "bounce")[0]:
        for _ in range(64):  # a surface hit (the one-ray hook draws a medium's distance from its own stream)
            j = src[rng.integers(len(src))]
            rec = O.world_hit(blob, rays[j, :7], 1e-4, INF)
            if rec is not None and rec[0] == first[j, 1]:
                break
        else:
            raise AssertionError(name)
        while True:
            u = _unit(rng)
            cos = float(np.dot(u, rec[4:7]))  # the normal faces the ray that found the point
            if (cos if part == "c" and name in TOUCHING else abs(cos)) >= 0.2:
                break
        rays[k, 0:3], rays[k, 3:6], rays[k, 6] = rec[1:4], u * rng.uniform(0.5, 2.0), rays[j, 6]
    rays.setflags(write=False)
    return rays, labels


@functools.lru_cache(maxsize=None)
def _boundary_rays(name, seed, n=N_BOUNDARY):
    """tmin = -inf, tmax = inf, as a ConstantMedium asks its boundary: from outside, from inside a
    leaf, and pointing away from the whole scene (every slab time negative)."""
    S = _scene(name)
    rng = np.random.default_rng(seed)
    rays, labels = [], []
    for k in range(n):
        cls = ("outside", "inside", "away", "outside")[k % 4]
        c, r = S["tg"][rng.integers(len(S["tg"]))]
        target = c + _unit(rng) * r * rng.random() ** (1 / 3)
        o = S["ctr"] + _unit(rng) * S["rad"] * rng.uniform(1.5, 3.0)
        d = (target - o) * rng.uniform(0.5, 2.0)
        if cls == "inside":
            if S["boxes"] and k % 8 < 4:
                lo, hi = S["boxes"][rng.integers(len(S["boxes"]))]
                o = lo + (hi - lo) * rng.uniform(0.1, 0.9, 3)
            else:
                cs, rs = S["spheres"][rng.integers(len(S["spheres"]))]
                o = np.array(cs) + _unit(rng) * rs * 0.8 * rng.random() ** (1 / 3)
            d = _unit(rng) * rng.uniform(0.5, 2.0)
        elif cls == "away":
            d = -d
        rays.append(list(o) + list(d) + [float(rng.random()), -INF, INF])
        labels.append(cls)
    return np.array(rays), np.array(labels)


def _ill(name, rays):
    """Rays whose origin lies further than 2^26 radii from some target. A sphere's test subtracts
    r^2 from |o - c|^2 (disc = half_b^2 - a c, in every walker); beyond |o - c| / r = 2^26 the radius
    is below half an ulp of those terms, so rounding alone decides the candidate: it can hit from
    anywhere nearby, also from outside the boxes the reference tree culls first. Such rays are
    asserted on in tests of their own (the same assertions): see the module docstring."""
    o = rays[:, None, 0:3]
    c = np.array([c for c, _ in _scene(name)["tg"]])[None]
    r = np.array([r for _, r in _scene(name)["tg"]])[None]
    return (np.linalg.norm(o - c, axis=2) > 2.0 ** 26 * r).any(axis=1)


# ---------------------------------------------------------------- (a) the ordered walks
def _walks(name, rays):
    """bvh_walks -> per MAIN value (cbvh [hit, t, node, flag], obvh [...], ref [hit, t, node])."""
    g = P.bvh_walks(_scene(name)["blob"], _root(name), rays)
    return [(g[:, b:b + 4], g[:, b + 4:b + 8], g[:, b + 8:b + 11]) for b in (0, 11)]


def _assert_walks(name, rays, labels, got, tag, sel, mains=(True, False)):
    """Assertion (a) on the rays `sel` of one bvh_walks result, for the given MAIN values."""
    for main, (cb, ob, ref) in zip((True, False), got):
        if main not in mains:
            continue
        fc, fo = cb[:, 3] > 0, ob[:, 3] > 0
        for walk, w, fl in (("cbvh", cb, fc), ("obvh", ob, fo)):
            bad = sel & ~fl & (_bits(w[:, 0:3]) != _bits(ref[:, 0:3])).any(axis=1)
            k = np.nonzero(bad)[0][:1]
            assert not bad.any(), (name, tag, walk, main, int(bad.sum()), sorted(set(labels[bad].tolist())),
                                   rays[k].tolist(), w[k].tolist(), ref[k].tolist())
        both = sel & ~fc & ~fo
        assert np.array_equal(_bits(cb[both, 0:3]), _bits(ob[both, 0:3])), (name, tag, main)
        bad = sel & fo & ~fc  # rt_kernel.h cbvh_walk_t: "flags every lane obvh_walk flags"
        assert not bad.any(), (name, tag, main, labels[bad][:4].tolist(), rays[bad][:2].tolist())


def _flagged(labels, got):
    """-> {class: (rays, flagged by cbvh, by obvh)} of the MAIN = true pass."""
    fc, fo = got[0][0][:, 3] > 0, got[0][1][:, 3] > 0
    return {c: (int((labels == c).sum()), int(fc[labels == c].sum()), int(fo[labels == c].sum()))
            for c in sorted(set(labels.tolist()))}


def _boundary_walks(name):
    """The boundary's two queries: tmin = -inf, then tmin = t1 + 1e-4 (constant_medium.rs), t1 the
    reference-order walk's. Only the MAIN = false half is the boundary instantiation (with MAIN =
    true the tie flags, which are relative to a positive closest t, are not meant for t < 0)."""
    b_rays, b_labels = _boundary_rays(name, 950 + SCENES.index(name))
    g1 = _walks(name, b_rays)
    t1, h1 = g1[1][2][:, 1], g1[1][2][:, 0] > 0
    b2 = b_rays[h1].copy()
    b2[:, 7] = t1[h1] + 0.0001
    return b_rays, b_labels, g1, t1, h1, b2, _walks(name, b2)


def _candidates_x(leaves, r):
    """The ordered walks' candidates of one ray in exact arithmetic (a quad's t in [tmin, inf), a
    sphere's near root in (tmin, inf) else its far root) -> [(t, key)]; equal keys are equal t."""
    o, d, tmin = _fr(r[0:3]), _fr(r[3:6]), (-INF if math.isinf(r[7]) else Fr(r[7]))
    out = []

    def leaf(nd):
        cx = _Ctx(r[6])
        if nd["tag"] == OBJ_LIST:
            for k in nd["kids"]:
                leaf(k)
        elif nd["tag"] == OBJ_QUAD:
            h = _hit_x(cx, nd, o, d, tmin, INF)
            if h:
                out.append((h[0], ("q", h[0])))
        else:
            assert nd["tag"] == OBJ_SPHERE
            for i, t in enumerate(_sphere_roots(cx, nd, o, d) or []):
                if _m(tmin) < t:
                    out.append((t, ("s", i, tuple(nd["c"]), nd["r"], nd["moving"], tuple(nd["cv"]))))
                    break
    for nd in leaves:
        leaf(nd)
    return out


def _exact_tie(leaves, r):
    """The two smallest values of {tmax, every exact candidate} are equal (`ties`: dyadic boxes and
    quads, so their t are Fractions and compare exactly; the duplicated sphere's roots are equal as
    the same expression; a sphere root and a Fraction never tie here: the spheres lie off the
    boxes' and quads' planes by construction, checked at 200 bits)."""
    cands = _candidates_x(leaves, r)
    if not math.isinf(r[8]):
        cands.append((Fr(r[8]), ("q", Fr(r[8]))))
    cands.sort(key=lambda c: _m(c[0]))
    if len(cands) < 2:
        return False
    (t0, k0), (t1, k1) = cands[0], cands[1]
    if k0 == k1:
        return True
    assert abs(_m(t0) - _m(t1)) > M(2) ** -150 * abs(_m(t1)), (r, k0, k1)
    return False


@pytest.mark.parametrize("name", WALK_SCENES)
def test_ordered_walks_are_the_reference_walk(gpu_available, name):
    rays, labels = _rays(name, 900 + SCENES.index(name), N_AB, "ab")
    got = _walks(name, rays)
    well = ~_ill(name, rays)
    _assert_walks(name, rays, labels, got, "ab", well)
    share = _flagged(labels, got)
    ref = got[0][2]
    seen = {c: int(((labels == c) & (ref[:, 0] > 0)).sum()) for c in share}
    print(f"bvh_walks[{name}]: {len(rays)} rays ({int((~well).sum())} of them ill-conditioned: "
          f"{sorted(set(labels[~well].tolist()))}), {int((ref[:, 0] > 0).sum())} hits; hits per class {seen}")
    assert set(labels[~well].tolist()) <= {"far13"} or name == "deep"
    print(f"bvh_walks[{name}]: flagged (rays, cbvh, obvh) per class {share}; in all "
          f"{100 * (got[0][0][:, 3] > 0).mean():.2f} % cbvh, {100 * (got[0][1][:, 3] > 0).mean():.2f} % obvh")
    if name == "near_ties":
        pole = (labels == "pole") & (rays[:, 5] > 0)
        t2 = np.sort(np.stack([got[0][0][pole, 1], ref[pole, 1]]), axis=0)
        print(f"bvh_walks[near_ties]: {int(pole.sum())} rays up a pair's axis, {share['pole']} flagged")
        assert pole.sum() >= N_AB // 16 and (ref[pole, 0] > 0).all() and (got[0][0][pole, 3] > 0).all()
        # the class is what it is meant to be: two candidates far inside the tie window, mostly not equal
        assert (t2[1] - t2[0] <= 2.0 ** -40 * t2[1]).all() and (t2[1] != t2[0]).sum() > 16
    for c in AB_CLASSES:
        if _applies(name, c, "ab") and not (name == "near_ties" and c in ("tmax_eq", "plane")):
            assert share[c][0] >= N_AB // 16 and seen[c] > 0, (name, c, share.get(c), seen.get(c))
    hit = ref[:, 0] > 0
    assert (rays[(labels == "tmin1e3") & hit, 7] < ref[(labels == "tmin1e3") & hit, 1]).all()
    tiny = np.abs(rays[labels == "tiny", 3:6])
    assert (((tiny > 0) & (tiny < 1e-38)).sum(axis=1) == 1).all()
    for c, zeros in (("zero1", 2), ("zero2", 1)):  # along one axis: two components +-0; along two: one
        assert ((rays[labels == c, 3:6] == 0).sum(axis=1) == zeros).all(), c
    if name == "ties":
        world = _world(_scene(name)["blob"])
        top = world["kids"][0]
        while top["tag"] != OBJ_BVH:  # create_bvh hands back a list of the one BvhNode
            assert top["tag"] == OBJ_LIST and len(top["kids"]) == 1
            top = top["kids"][0]
        leaves = _bvh_leaves(top)
        assert len(leaves) == 12
        n_tie, by_cls = 0, {}
        for k in range(0, len(rays), 3):  # exact arithmetic on every third ray: every class, seconds not minutes
            if well[k] and _exact_tie(leaves, rays[k].tolist()):  # (1e13 away the device's candidates are not the exact ones)
                n_tie += 1
                by_cls[labels[k]] = by_cls.get(labels[k], 0) + 1
                assert got[0][0][k, 3] > 0 and got[0][1][k, 3] > 0, (labels[k], rays[k].tolist(), got[0][0][k], got[0][1][k])
        print(f"bvh_walks[ties]: {n_tie} of {len(range(0, len(rays), 3))} rays tie exactly, all flagged by both walks: {by_cls}")
        assert by_cls.get("tmax_eq", 0) >= 32 and by_cls.get("in_box", 0) > 0 and by_cls.get("aim", 0) > 0
    # the boundary form
    b_rays, b_labels, g1, t1, h1, b2, g2 = _boundary_walks(name)
    assert not _ill(name, b_rays).any()
    _assert_walks(name, b_rays, b_labels, g1, "boundary 1", np.ones(len(b_rays), bool), (False,))
    _assert_walks(name, b2, b_labels[h1], g2, "boundary 2", np.ones(len(b2), bool), (False,))
    s1 = _flagged(b_labels, (g1[1], g1[1]))
    away = b_labels == "away"
    inside_neg = int(((b_labels == "inside") & h1 & (t1 < 0)).sum())
    print(f"bvh_walks[{name}] boundary: first query hits {int(h1.sum())} of {len(b_rays)}, second "
          f"{int((g2[1][2][:, 0] > 0).sum())}; {int((away & h1 & (t1 < 0)).sum())} of {int(away.sum())} rays pointing "
          f"away hit behind the origin, {inside_neg} from inside; flagged {s1}")
    assert (away & h1 & (t1 < 0)).sum() > 20 and inside_neg > 20 and (g2[1][2][:, 0] > 0).sum() > 50


@pytest.mark.parametrize("name", WALK_SCENES)
def test_ordered_walks_on_ill_conditioned_rays(gpu_available, name):
    """Assertion (a) on the rays _ill() sets aside: the origins 1e13 away. Failed in `mixed`,
    `lattice`, `deep`, `instance` and `near_ties` before obvh_far: see FINDING in the module docstring."""
    rays, labels = _rays(name, 900 + SCENES.index(name), N_AB, "ab")
    got = _walks(name, rays)
    ill = _ill(name, rays)
    assert ill.sum() >= N_AB // 16
    for main, (cb, ob, ref) in zip((True, False), got):
        for walk, w in (("cbvh", cb), ("obvh", ob)):
            bad = ill & (w[:, 3] == 0) & (_bits(w[:, 0:3]) != _bits(ref[:, 0:3])).any(axis=1)
            print(f"bvh_walks[{name}] ill-conditioned, MAIN = {main}: {walk} differs from the reference-order "
                  f"walk with its flag clear on {int(bad.sum())} of {int(ill.sum())} rays")
    _assert_walks(name, rays, labels, got, "ill-conditioned", ill)


def test_deep_tree_depth():
    """Host only (no GPU needed, but the module is a GPU module): the `deep` scene's compact tree is
    at least twice as deep as a balanced tree of its 48 leaves, and `ineligible` has no ordered BVH."""
    chk = rt.lds_check(_scene("deep")["blob"], 0, 0, 1)
    depth = chk["cbvh_stack"] // 4
    print(f"deep: compact tree depth {depth} (balanced: {math.ceil(math.log2(48))}), stack {chk['cbvh_stack']} B per lane")
    assert depth == chk["max_depth"] and depth >= 2 * math.ceil(math.log2(48)) and chk["errors"] == 0
    recs = P.scene_records(_scene("ineligible")["blob"])
    bvh = recs[recs[:, 1] == P.RTL_BVH]
    assert len(bvh) >= 7 and (bvh[:, 3] == 0).all() and bvh[0, 4] == -1
    assert (recs[:, 1] == P.RTL_TRANSLATE).sum() == 1


# ---------------------------------------------------------------- (b) the product path
@functools.lru_cache(maxsize=None)
def _world_run(name, seed, n, part):
    rays, _ = _rays(name, seed, n, part)
    return P.scene_run("world_hit_bvh", _scene(name)["blob"], _world_records(rays, _keys(n)))


def _one_primitive(blob, got):
    """world_hit / world_hit_bvh output with both hit nodes replaced by the primitive's number (its
    first copy's: the COUNT build walks the second copy of a duplicated span-1 leaf, the product
    build jumps over it; both return the one primitive's record, at two addresses)."""
    prim_of, _ = _prims(blob)
    canon = _canon(_world(blob))
    out = got.copy()
    for c in (2, 9):
        out[:, c] = [canon(prim_of[int(x)]) if x >= 0 else -1.0 for x in got[:, c]]
    return out


def _assert_product_is_count(name, rays, labels, got, sel):
    got = _one_primitive(_scene(name)["blob"], got)
    bad = sel & (_bits(got[:, 0:7]) != _bits(got[:, 7:14])).any(axis=1)
    k = np.nonzero(bad)[0][:1]
    assert not bad.any(), (name, int(bad.sum()), sorted(set(labels[bad].tolist())), rays[k].tolist(), got[k].tolist())


@pytest.mark.parametrize("name", [n for n in SCENES if n != "ineligible"])
def test_product_walk_on_ill_conditioned_rays(gpu_available, name):
    """Assertion (b) on the rays _ill() sets aside. Failed wherever (a) did, and in `fog_bvh`, before
    obvh_far."""
    rays, labels = _rays(name, 900 + SCENES.index(name), N_AB, "ab")
    got = _world_run(name, 900 + SCENES.index(name), N_AB, "ab")
    ill = _ill(name, rays)
    assert ill.sum() >= N_AB // 16
    _assert_product_is_count(name, rays, labels, got, ill)


@pytest.mark.parametrize("name", SCENES)
def test_product_walk_is_the_count_walk(gpu_available, name):
    rays, labels = _rays(name, 900 + SCENES.index(name), N_AB, "ab")
    got = _world_run(name, 900 + SCENES.index(name), N_AB, "ab")
    well = ~_ill(name, rays) | (name == "ineligible")  # no ordered BVH there: every ray
    _assert_product_is_count(name, rays, labels, got, well)
    frames = sorted(set(got[got[:, 0] > 0, 3].astype(int).tolist()))
    print(f"world_hit_bvh[{name}]: {len(rays)} rays, {int((got[:, 0] > 0).sum())} hits, frames {frames}, "
          f"product == COUNT bit for bit")
    if name not in WALK_SCENES:
        return
    ref = _walks(name, rays)[0][2]
    if name != "instance":  # the world is the one tree
        assert np.array_equal(_bits(got[well, 0:3]), _bits(ref[well, 0:3])), name
        return
    assert len(frames) == 2 and frames[0] == -1
    recs = P.scene_records(_scene(name)["blob"])
    plain = int(recs[recs[:, 1] == P.RTL_SPHERE][-1, 0])
    tree = well & (got[:, 0] > 0) & (got[:, 3] == -1) & (got[:, 2] != plain)  # the world's hit lies in the top-level tree
    assert tree.sum() > 100 and np.array_equal(_bits(got[tree, 0:3]), _bits(ref[tree, 0:3]))
    other = well & ~tree & (ref[:, 0] > 0)  # something else was closer (or tied: the list order decides)
    assert (got[other, 0] > 0).all() and (got[other, 1] <= ref[other, 1]).all()


# ---------------------------------------------------------------- (c) exact arithmetic and the oracle
def _canon(world):
    """blob-order primitive number -> the number of its first copy (a duplicated span-1 leaf: the
    reference returns the right copy's record for a quad, the renderer the left one's; they are
    one primitive)."""
    canon = {}

    def prims(nd, out):
        if "prim" in nd:
            out.append(nd["prim"])
        for k in nd.get("kids", []):
            prims(k, out)
        return out

    def walk(nd):
        for k in nd.get("kids", []):
            walk(k)
        if nd["tag"] == OBJ_BVH and nd["dup"]:
            for a, b in zip(prims(nd["kids"][0], []), prims(nd["kids"][1], [])):
                canon[b] = canon.get(a, a)
    walk(world)
    return lambda p: canon.get(int(p), int(p))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """No GPU: part (c)'s rays, keys, exact answers [(t, prim, mat) or None, guard, draws], the
    oracle's, its worst t error, the guard share and the hits; asserts the oracle's decisions."""
    blob = _scene(name)["blob"]
    rays, labels = _rays(name, 800 + SCENES.index(name), N_C, "c")
    keys = _keys(N_C)
    world = _world(blob)
    canon = _canon(world)
    ora = _oracle_world(blob, rays, keys)
    exact, left, hits, ora_w = [], 0, 0, M(0)
    for r, k, g in zip(rays.tolist(), keys.tolist(), ora):
        cx = _Ctx(r[6], O.rng_draws(k[0], k[1], k[2], 4).tolist())
        tmax = INF if math.isinf(r[8]) else Fr(r[8])
        h = _hit_x(cx, world, _fr(r[0:3]), _fr(r[3:6]), Fr(r[7]), tmax)
        exact.append((None if h is None else (h[0], canon(h[1]["prim"]), h[1]["mat"]), cx.guard, cx.draws))
        if cx.guard:
            left += 1
            continue
        assert bool(g[0]) == (h is not None), ("oracle", name, r)
        if h:
            hits += 1
            assert (canon(g[4]), g[2]) == (canon(h[1]["prim"]), h[1]["mat"]), ("oracle", name, r, g.tolist())
            ora_w = max(ora_w, _rel(g[1], h[0]))
    share = left / len(rays)
    print(f"reference[{name}]: {len(rays)} rays, {hits} hits, guard band leaves out {100 * share:.2f} %, "
          f"oracle worst t error {float(ora_w):.3e}")
    assert share <= 0.01, (name, share)
    assert 0.2 * len(rays) <= hits <= 0.8 * len(rays), (name, hits)
    return rays, labels, keys, exact, float(ora_w), share, hits, canon


@pytest.mark.parametrize("name", SCENES)
def test_reference_walk_against_exact_arithmetic(gpu_available, name):
    blob = _scene(name)["blob"]
    rays, labels, keys, exact, ora_w, share, hits, canon = _reference(name)
    got = _world_run(name, 800 + SCENES.index(name), N_C, "c")
    assert not _ill(name, rays).any()
    _assert_product_is_count(name, rays, labels, got, np.ones(len(rays), bool))
    prim_of, _ = _prims(blob)
    dev_w, worst = M(0), None
    for r, k, (h, guard, draws), g in zip(rays.tolist(), keys.tolist(), exact, got):
        if guard:
            continue
        _, state, _ = _rng_py(k[0], k[1], k[2], draws)
        assert bool(g[0]) == (h is not None), ("device", name, r, g.tolist())
        assert g[5:7].tolist() == [float(state[0]), float(state[1])], ("draws", name, r, draws)
        if h is None:
            continue
        assert canon(prim_of[int(g[2])]) == h[1] and g[4] == h[2], ("device", name, r, g.tolist(), h[1:])
        if _rel(g[1], h[0]) > dev_w:
            dev_w, worst = _rel(g[1], h[0]), (r, h[1], float(g[1]))
    print(f"world_hit_bvh[{name}]: {len(rays)} rays, {hits} hits, guard band leaves out {100 * share:.2f} %")
    print(f"world_hit_bvh[{name}]: the device's worst ray {worst}")
    _rule(f"world_hit_bvh[{name}] t", float(dev_w), ora_w)
    if name == "fog_bvh":
        draws = sum(e[2] for e in exact)
        vols = {nd["prim"] for nd in _world(blob)["kids"] if nd["tag"] == OBJ_VOLUME}
        assert len(vols) == 2
        fog = sum(1 for e in exact if e[0] is not None and not e[1] and e[0][1] in vols)
        print(f"world_hit_bvh[fog_bvh]: {draws} draws, {fog} hits in a medium")
        assert draws > 0.2 * N_C and fog > 25
