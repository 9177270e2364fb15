"""Scenes for the deferred light-list PDF (rt_jit.cpp kLpdfDefer): light lists whose entries are,
or are not, also world-frame records of the generated walker. Shared by
test_lpdf_defer_host.py (which scenes qualify) and test_lpdf_defer_gpu.py (parity)."""
import re

import surely_rt as rt

LOW_QUAD = ((4.5, -1e-9, -1), (1, 0, 0), (0, 0, 2))
TOP_QUAD = ((-1, 4, -1), (2, 0, 0), (0, 0, 2))


def defers(src):
    """The generated walker's kLpdfDefer (true unless -DRT_LPDF_NOW overrides it)."""
    assert re.search(r"static constexpr bool kLpdfDefer = (true|false);", src), "no kLpdfDefer"
    return "static constexpr bool kLpdfDefer = true;" in src


def zero_pdf_matched(depth, sphere_light=False):
    """test_gpu_parity._zero_pdf_scene with its low light quad in the world as well, so every
    light entry has a world record; sphere_light: the sphere is glass and also a light entry."""
    sc = rt.Scene(9)
    white = sc.lambertian((0.73, 0.73, 0.73))
    light = sc.diffuse_light((6, 6, 6))
    ball = sc.dielectric(1.5) if sphere_light else white
    floor = sc.quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), white)
    top = sc.quad(*TOP_QUAD, light)
    walls = [sc.quad((6, -1, -6), (0, 4, 0), (0, 0, 12), light),
             sc.quad((-6, -1, -6), (0, 0, 12), (0, 4, 0), light),
             sc.quad((-6, -1, 6), (0, 4, 0), (12, 0, 0), light),
             sc.quad((-6, -1, -6), (12, 0, 0), (0, 4, 0), light)]
    world = sc.hittable_list(floor, top, sc.sphere((0, 1, 0), 1.0, ball), *walls,
                             sc.quad(*LOW_QUAD, light))
    lights = sc.hittable_list(sc.quad(*LOW_QUAD, light), sc.quad(*TOP_QUAD, light))
    if sphere_light:
        sc.add(lights, sc.sphere((0, 1, 0), 1.0, ball))
    blob = sc.serialize(world, lights)
    cam = rt.camera_new(1.0, 48, 16, depth, 60, (0, 3, 5), (0, 0.5, 0), (0, 1, 0), 0, 0, (0, 0, 0))
    return blob, cam


def nested_light_list():
    """The scene of test_gpu_parity.test_nested_light_list_parity."""
    sc = rt.Scene(12)
    white = sc.lambertian((0.73, 0.73, 0.73))
    red = sc.lambertian((0.65, 0.05, 0.05))
    light = sc.diffuse_light((9, 9, 9))
    glass = sc.dielectric(1.5)
    world = sc.hittable_list(
        sc.quad((-5, 0, -5), (10, 0, 0), (0, 0, 10), white),
        sc.quad((-5, 0, -3), (10, 0, 0), (0, 6, 0), red),
        sc.quad(*TOP_QUAD, light),
        sc.quad((2.5, 3, 0), (1, 0, 0), (0, 0, 1), light),
        sc.sphere((0, 1, 1), 1.0, glass))
    inner = sc.hittable_list(sc.sphere((0, 1, 1), 1.0, glass),
                             sc.quad((2.5, 3, 0), (1, 0, 0), (0, 0, 1), light))
    lights = sc.hittable_list(sc.quad(*TOP_QUAD, light), inner)
    return sc.serialize(world, lights)


def room(kind, width=32, spp=16, depth=8):
    """A floor, a back wall and a light quad (in the world and in the light list), varied:
    'checker'   the floor is a checker texture (atten varies per bounce);
    'volume'    plus a ConstantMedium sphere (isotropic bounces under deferral);
    'translate' the world's light quad sits inside a Translate (same world position);
    'general'   the light quad is not axis-aligned;
    'moving'    plus a moving sphere, in the world and in the light list;
    'spheres2'  plus two glass spheres, both also light entries."""
    sc = rt.Scene(21)
    white = sc.lambertian((0.73, 0.73, 0.73))
    light = sc.diffuse_light((7, 7, 7))
    floor_mat = white
    if kind == "checker":
        floor_mat = sc.lambertian(tex=sc.checker_from_color(0.8, (0.9, 0.2, 0.1), (0.1, 0.3, 0.9)))
    # the floor off the checker's discontinuity plane y = 0 (test_gpu_parity's mix test)
    objs = [sc.quad((-4, -0.3, -4), (8, 0, 0), (0, 0, 8), floor_mat),
            sc.quad((-4, -0.3, -3), (8, 0, 0), (0, 6, 0), white)]
    lq = TOP_QUAD
    if kind == "general":
        lq = ((-1, 4, -1), (2, 0.5, 0), (0, 0, 2))
    entries = [sc.quad(*lq, light)]
    if kind == "translate":
        q = ((lq[0][0] - 1.0, lq[0][1], lq[0][2]), lq[1], lq[2])
        objs.append(sc.translate(sc.quad(*q, light), (1.0, 0, 0)))
    else:
        objs.append(sc.quad(*lq, light))
    if kind == "volume":
        objs.append(sc.constant_medium(sc.sphere((0.3, 0.9, 0.2), 1.1, white), 0.9, (0.8, 0.7, 0.9)))
    if kind == "moving":
        objs.append(sc.sphere_moving((1, 0.5, 0), (1, 0.9, 0), 0.5, white))
        entries.append(sc.sphere_moving((1, 0.5, 0), (1, 0.9, 0), 0.5, white))
    if kind == "spheres2":
        glass = sc.dielectric(1.5)
        for c in ((-1.2, 0.5, 0.5), (1.2, 0.5, 0.5)):
            objs.append(sc.sphere(c, 0.8, glass))
            entries.append(sc.sphere(c, 0.8, glass))
    blob = sc.serialize(sc.hittable_list(*objs), sc.hittable_list(*entries))
    cam = rt.camera_new(1.0, width, spp, depth, 45, (0, 2.5, 8), (0, 1, 0), (0, 1, 0), 0, 0,
                        (0.05, 0.05, 0.08))
    return blob, cam
