// capi.cpp — C API (include/rt_host.h) over the C++ scene builder, plus the host output stage
// (color.rs write_color / linear_to_gamma / exposure, render.rs auto_expose + P3 header).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/rt_host.h"
#include "../rt_frame3.h"
#include "scene.hpp"

using namespace rt;

struct rth_scene {
  explicit rth_scene(uint64_t seed) : rng(seed) {}
  SceneRng rng;
  std::vector<TexturePtr> textures;
  std::vector<MaterialPtr> materials;
  std::vector<ObjectPtr> objects;
  std::vector<uint64_t> blob;
  std::vector<uint8_t> texels;
};

static thread_local std::string g_err;

static int32_t fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

extern "C" const char* rth_last_error(void) { return g_err.c_str(); }

static Vec3 v3(const double* p) { return Vec3(p[0], p[1], p[2]); }

template <class T>
static int32_t push(std::vector<T>& vec, T v) {
  vec.push_back(std::move(v));
  return (int32_t)vec.size() - 1;
}

#define CHECK_S(s) \
  if (!(s)) return fail("null scene")
#define TEX(s, id) (((id) >= 0 && (size_t)(id) < (s)->textures.size()) ? (s)->textures[id] : nullptr)
#define MAT(s, id) (((id) >= 0 && (size_t)(id) < (s)->materials.size()) ? (s)->materials[id] : nullptr)
#define OBJ(s, id) (((id) >= 0 && (size_t)(id) < (s)->objects.size()) ? (s)->objects[id] : nullptr)

extern "C" {

rth_scene* rth_scene_new(uint64_t build_seed) { return new rth_scene(build_seed); }
void rth_scene_free(rth_scene* s) { delete s; }
double rth_random_double(rth_scene* s) { return s->rng.random_double(); }
double rth_random_range(rth_scene* s, double mn, double mx) { return s->rng.random_range(mn, mx); }
int64_t rth_random_int(rth_scene* s, int64_t mn, int64_t mx) { return s->rng.random_int(mn, mx); }

int32_t rth_solid_color(rth_scene* s, double r, double g, double b) {
  CHECK_S(s);
  return push(s->textures, SolidColor({r, g, b}));
}
int32_t rth_checker_texture(rth_scene* s, double scale, int32_t even, int32_t odd) {
  CHECK_S(s);
  auto e = TEX(s, even), o = TEX(s, odd);
  if (!e || !o) return fail("checker: bad texture id");
  return push(s->textures, CheckerTexture(scale, e, o));
}
int32_t rth_noise_texture(rth_scene* s, double scale) {
  CHECK_S(s);
  return push(s->textures, NoiseTexture(scale, s->rng));
}
int32_t rth_image_texture(rth_scene* s, int32_t w, int32_t h, const uint8_t* rgb8) {
  CHECK_S(s);
  if (w < 0 || h < 0) return fail("image: negative size");
  return push(s->textures, ImageTexture(w, h, rgb8));
}

static int32_t mat_with_tex(rth_scene* s, int32_t tex, MaterialPtr (*ctor)(TexturePtr)) {
  CHECK_S(s);
  auto t = TEX(s, tex);
  if (!t) return fail("bad texture id");
  return push(s->materials, ctor(t));
}
int32_t rth_lambertian(rth_scene* s, double r, double g, double b) {
  return mat_with_tex(s, rth_solid_color(s, r, g, b), Lambertian);
}
int32_t rth_lambertian_tex(rth_scene* s, int32_t tex) { return mat_with_tex(s, tex, Lambertian); }
int32_t rth_metal(rth_scene* s, double r, double g, double b, double fuzz) {
  CHECK_S(s);
  return push(s->materials, Metal({r, g, b}, fuzz));
}
int32_t rth_dielectric(rth_scene* s, double ir, double r, double g, double b) {
  CHECK_S(s);
  return push(s->materials, Dielectric(ir, {r, g, b}));
}
int32_t rth_diffuse_light(rth_scene* s, double r, double g, double b) {
  return mat_with_tex(s, rth_solid_color(s, r, g, b), DiffuseLight);
}
int32_t rth_diffuse_light_tex(rth_scene* s, int32_t tex) { return mat_with_tex(s, tex, DiffuseLight); }
int32_t rth_isotropic(rth_scene* s, double r, double g, double b) {
  return mat_with_tex(s, rth_solid_color(s, r, g, b), Isotropic);
}
int32_t rth_isotropic_tex(rth_scene* s, int32_t tex) { return mat_with_tex(s, tex, Isotropic); }

int32_t rth_sphere(rth_scene* s, const double c[3], double radius, int32_t mat) {
  CHECK_S(s);
  auto m = MAT(s, mat);
  if (!m) return fail("sphere: bad material id");
  return push(s->objects, Sphere(v3(c), radius, m));
}
int32_t rth_sphere_moving(rth_scene* s, const double c1[3], const double c2[3], double radius,
                          int32_t mat) {
  CHECK_S(s);
  auto m = MAT(s, mat);
  if (!m) return fail("sphere: bad material id");
  return push(s->objects, SphereMoving(v3(c1), v3(c2), radius, m));
}
int32_t rth_quad(rth_scene* s, const double q[3], const double u[3], const double v[3],
                 int32_t mat) {
  CHECK_S(s);
  auto m = MAT(s, mat);
  if (!m) return fail("quad: bad material id");
  return push(s->objects, Quad(v3(q), v3(u), v3(v), m));
}
int32_t rth_make_box(rth_scene* s, const double a[3], const double b[3], int32_t mat) {
  CHECK_S(s);
  auto m = MAT(s, mat);
  if (!m) return fail("make_box: bad material id");
  return push(s->objects, make_box(v3(a), v3(b), m));
}
int32_t rth_list_new(rth_scene* s) {
  CHECK_S(s);
  return push(s->objects, HittableList());
}
int32_t rth_list_add(rth_scene* s, int32_t list, int32_t obj) {
  CHECK_S(s);
  auto l = OBJ(s, list), o = OBJ(s, obj);
  if (!l || l->tag != RT_OBJ_LIST) return fail("list_add: not a list");
  if (!o) return fail("list_add: bad object id");
  if (o.get() == l.get()) return fail("list_add: a list cannot contain itself");
  list_add(l, o);
  return 0;
}
int32_t rth_list_create_bvh(rth_scene* s, int32_t list) {
  CHECK_S(s);
  auto l = OBJ(s, list);
  if (!l || l->tag != RT_OBJ_LIST) return fail("create_bvh: not a list");
  if (l->objects.empty()) return fail("create_bvh: empty list");  // reference indexes [0] and panics
  return push(s->objects, create_bvh(l, s->rng));
}
int32_t rth_list_len(rth_scene* s, int32_t list) {
  CHECK_S(s);
  auto l = OBJ(s, list);
  if (!l || l->tag != RT_OBJ_LIST) return fail("list_len: not a list");
  return (int32_t)l->objects.size();
}
int32_t rth_translate(rth_scene* s, int32_t obj, const double off[3]) {
  CHECK_S(s);
  auto o = OBJ(s, obj);
  if (!o) return fail("translate: bad object id");
  return push(s->objects, Translate(o, v3(off)));
}
int32_t rth_rotate_y(rth_scene* s, int32_t obj, double angle) {
  CHECK_S(s);
  auto o = OBJ(s, obj);
  if (!o) return fail("rotate_y: bad object id");
  return push(s->objects, RotateY(o, angle));
}
int32_t rth_constant_medium(rth_scene* s, int32_t boundary, double density, double r, double g,
                            double b) {
  return rth_constant_medium_tex(s, boundary, density, rth_solid_color(s, r, g, b));
}
int32_t rth_constant_medium_tex(rth_scene* s, int32_t boundary, double density, int32_t tex) {
  CHECK_S(s);
  auto o = OBJ(s, boundary);
  auto t = TEX(s, tex);
  if (!o || !t) return fail("constant_medium: bad id");
  return push(s->objects, ConstantMedium(o, density, t));
}
int rth_object_bbox(rth_scene* s, int32_t obj, double out6[6]) {
  CHECK_S(s);
  auto o = OBJ(s, obj);
  if (!o) return fail("bbox: bad object id");
  const Aabb& b = o->bbox;
  double v[6] = {b.x.min, b.x.max, b.y.min, b.y.max, b.z.min, b.z.max};
  std::memcpy(out6, v, sizeof(v));
  return 0;
}

int rth_serialize(rth_scene* s, int32_t world_list, int32_t lights, rt_scene_blob* out) {
  CHECK_S(s);
  auto w = OBJ(s, world_list);
  if (!w || w->tag != RT_OBJ_LIST) return fail("serialize: world must be a HittableList");
  ObjectPtr l;
  if (lights >= 0) {
    l = OBJ(s, lights);
    if (!l) return fail("serialize: bad lights id");
  }
  s->blob = serialize(w, l, &s->texels);
  out->slots = s->blob.data();
  out->n_slots = s->blob.size();
  out->texels = s->texels.empty() ? nullptr : s->texels.data();
  out->n_texels = s->texels.size();
  return 0;
}

int rth_camera_new(double aspect_ratio, int32_t image_width, int32_t spp, int32_t max_depth,
                   double vfov, const double lookfrom[3], const double lookat[3],
                   const double vup[3], double defocus_angle, double focus_dist,
                   const double background[3], rt_camera* out) {
  if (!out || image_width <= 0 || spp <= 0 || max_depth < 0 || !(aspect_ratio > 0))
    return fail("camera: invalid arguments");
  *out = camera_new(aspect_ratio, image_width, spp, max_depth, vfov, v3(lookfrom), v3(lookat),
                    v3(vup), defocus_angle, focus_dist, v3(background));
  return 0;
}

int rth_camera_orbit_y(const rt_camera* in, const double pivot[3], double degrees,
                       rt_camera* out) {
  if (!in || !pivot || !out || !std::isfinite(degrees)) return fail("camera_orbit_y: invalid arguments");
  rt_camera c = *in;
  if (degrees != 0.0) {
    const double th = degrees * M_PI / 180.0, cs = std::cos(th), sn = std::sin(th);
    // (x, z) -> (cs x + sn z, -sn x + cs z): RotateY's rotation (transform.rs:143-186)
    auto turn = [&](double* v, const double* about) {
      const double x = v[0] - about[0], z = v[2] - about[2];
      v[0] = about[0] + (cs * x + sn * z);
      v[2] = about[2] + (-sn * x + cs * z);
    };
    const double origin[3] = {0.0, 0.0, 0.0};
    turn(c.center, pivot);
    turn(c.pixel00_loc, pivot);
    turn(c.pixel_delta_u, origin);
    turn(c.pixel_delta_v, origin);
    turn(c.defocus_disk_u, origin);
    turn(c.defocus_disk_v, origin);
  }
  *out = c;
  return 0;
}

// ---- rth_projection_rays: host ray generator for rt_render_rays
namespace {
// csrc/rt_rng.h restated for the host (rng_seed: pcg2d key; rng_step: xoroshiro64*);
// tests/test_rays_host.py pins the draws to the oracle's camera ray bit for bit
struct HostRng {
  uint32_t s0, s1;
};
uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
HostRng host_rng_seed(uint64_t seed, uint32_t pixel, uint32_t sample) {
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  const uint32_t k0 = (lo ^ 0x85EBCA6Bu) * 0x9E3779B9u + 1013904223u;
  const uint32_t k1 = (hi ^ 0xC2B2AE35u) * 0x9E3779B9u + (k0 ^ 0x27D4EB2Fu);
  uint32_t v0 = pixel * 1664525u + k0, v1 = sample * 1664525u + k1;
  for (int r = 0; r < 2; ++r) {
    v0 += v1 * 1664525u;
    v1 += v0 * 1664525u;
    v0 ^= v0 >> 16;
    v1 ^= v1 >> 16;
  }
  if ((v0 | v1) == 0u) v0 = 0x9E3779B9u;
  return {v0, v1};
}
double host_rnd(HostRng& g) {
  const uint32_t s0 = g.s0;
  uint32_t s1 = g.s1;
  const uint32_t result = s0 * 0x9E3779BBu;
  s1 ^= s0;
  g.s0 = rotl32(s0, 26) ^ s1 ^ (s1 << 9);
  g.s1 = rotl32(s1, 13);
  return (double)result * 0x1p-32;
}
// the view frame's helpers: shared with the device generator's host side (rt_raygen.hip)
using rtframe::cross3;
using rtframe::unit3;
}  // namespace

int rth_projection_rays(const rth_projection* pr, const rt_camera* cam, uint64_t seed, int32_t s_i,
                        int32_t s_j, rt_ray* out) {
  if (!pr || !out) return fail("projection_rays: null argument");
  const bool pin = pr->kind == RTH_PROJ_PINHOLE;
  if (pr->kind < RTH_PROJ_PINHOLE || pr->kind > RTH_PROJ_FISHEYE) return fail("projection_rays: unknown kind");
  if (pin && !cam) return fail("projection_rays: the pinhole projection needs a camera");
  const int W = pin ? cam->image_width : pr->width, H = pin ? cam->image_height : pr->height;
  const int S = pin ? cam->sqrt_spp : pr->sqrt_spp;
  if (W < 1 || H < 1 || S < 1 || (int64_t)W * H >= (1ll << 31))
    return fail("projection_rays: width, height and sqrt_spp must be >= 1 (and width * height < 2^31)");
  if (s_i < 0 || s_i >= S || s_j < 0 || s_j >= S) return fail("projection_rays: stratum outside sqrt_spp");
  double f[3] = {0, 0, 0}, r[3] = {0, 0, 0}, u[3] = {0, 0, 0};
  if (!pin) {
    double fxu[3];
    if (!unit3(pr->forward, f)) return fail("projection_rays: forward is zero or not finite");
    cross3(f, pr->up, fxu);
    if (!unit3(fxu, r)) return fail("projection_rays: up is zero, not finite or parallel to forward");
    cross3(r, f, u);
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(pr->origin[k])) return fail("projection_rays: origin is not finite");
    if (pr->kind != RTH_PROJ_PANORAMA && !(pr->fov > 0.0 && std::isfinite(pr->fov)))
      return fail("projection_rays: fov must be positive and finite");
  }
  // recip_sqrt_spp as Camera::new forms it (render.rs:76); the pinhole takes the camera's own
  const double rs = pin ? cam->recip_sqrt_spp : 1.0 / (double)S;
  for (int j = 0; j < H; ++j) {
    for (int i = 0; i < W; ++i) {
      rt_ray& q = out[(size_t)j * W + i];
      q.pixel = (uint32_t)(j * W + i);
      q.sample = (uint32_t)(s_j * S + s_i);
      HostRng g = host_rng_seed(seed, q.pixel, q.sample);
      const double px = std::fma(rs, (double)s_i + host_rnd(g), -0.5);
      const double py = std::fma(rs, (double)s_j + host_rnd(g), -0.5);
      q.time = host_rnd(g);
      q.tmin = 1e-4;
      q.tmax = INFINITY;
      if (pin) {  // get_ray (render.rs:218-249) without the defocus disk, the device's fma forms
        for (int k = 0; k < 3; ++k) {
          const double pc = std::fma((double)j, cam->pixel_delta_v[k],
                                     std::fma((double)i, cam->pixel_delta_u[k], cam->pixel00_loc[k]));
          const double ps = pc + std::fma(px, cam->pixel_delta_u[k], cam->pixel_delta_v[k] * py);
          q.origin[k] = cam->center[k];
          q.dir[k] = ps - cam->center[k];
        }
        continue;
      }
      const double x = ((double)i + 0.5 + px) / (double)W, y = ((double)j + 0.5 + py) / (double)H;
      double a = 0.0, b = 0.0, c = 0.0;  // dir = a r + b u + c f
      double oa = 0.0, ob = 0.0;         // origin offset along r and u
      if (pr->kind == RTH_PROJ_ORTHO) {
        c = 1.0;
        oa = (x - 0.5) * pr->fov * (double)W / (double)H;
        ob = (0.5 - y) * pr->fov;
      } else if (pr->kind == RTH_PROJ_PANORAMA) {
        const double lon = (x - 0.5) * 2.0 * M_PI, lat = (0.5 - y) * M_PI;
        a = std::cos(lat) * std::sin(lon);
        b = std::sin(lat);
        c = std::cos(lat) * std::cos(lon);
      } else {
        const double m = (double)(W < H ? W : H);
        const double nx = (2.0 * x - 1.0) * (double)W / m, ny = (1.0 - 2.0 * y) * (double)H / m;
        const double th = std::hypot(nx, ny) * (pr->fov * M_PI / 180.0) * 0.5;
        if (th <= M_PI) {
          const double ph = std::atan2(ny, nx);
          a = std::sin(th) * std::cos(ph);
          b = std::sin(th) * std::sin(ph);
          c = std::cos(th);
        }
      }
      for (int k = 0; k < 3; ++k) {
        q.origin[k] = pr->origin[k] + oa * r[k] + ob * u[k];
        q.dir[k] = a * r[k] + b * u[k] + c * f[k];
      }
    }
  }
  return 0;
}

// ---- rth_ao_rays: ambient-occlusion ray batches for any-hit queries (rt_mi355x.h)
int rth_ao_rays(const rt_ray* primary, const rt_hit* hits, uint64_t n, const rth_ao_params* p,
                rt_ray* out) {
  if (!primary || !hits || !p || !out) return fail("ao_rays: null argument");
  if (p->_pad0 != 0u) return fail("ao_rays: _pad0 must be 0");
  if (!(std::isfinite(p->tmin) && p->tmin >= 0.0)) return fail("ao_rays: tmin must be finite and >= 0");
  if (!(p->radius > p->tmin)) return fail("ao_rays: radius must be > tmin (NaN is invalid)");
  for (uint64_t i = 0; i < n; ++i) {
    rt_ray& q = out[i];
    const rt_hit& h = hits[i];
    const uint32_t pixel = primary[i].pixel;
    const double time = primary[i].time;  // read before q is written: out may be primary
    q.time = time;
    q.tmin = p->tmin;
    q.tmax = p->radius;
    q.pixel = pixel;
    q.sample = p->dir_index;
    if (h.hit != 1) {  // no surface: an invalid ray, which the query answers with 255
      for (int k = 0; k < 3; ++k) q.origin[k] = q.dir[k] = 0.0;
      continue;
    }
    HostRng g = host_rng_seed(p->seed, pixel, p->dir_index);
    const double r1 = host_rnd(g), r2 = host_rnd(g);
    // random_cosine_direction (vec3.rs:240-250)
    const double phi = 2. * M_PI * r1;
    const double x = std::cos(phi) * std::sqrt(r2), y = std::sin(phi) * std::sqrt(r2);
    const double z = std::sqrt(1. - r2);
    // Onb::build_from_w (onb.rs:32-47)
    double w[3], a[3] = {1., 0., 0.}, wa[3], v[3], u[3];
    const double wl = std::sqrt(h.normal[0] * h.normal[0] + h.normal[1] * h.normal[1] +
                                h.normal[2] * h.normal[2]);
    for (int k = 0; k < 3; ++k) w[k] = h.normal[k] / wl;
    if (std::fabs(w[0]) > 0.9) a[0] = 0., a[1] = 1.;
    cross3(w, a, wa);
    const double vl = std::sqrt(wa[0] * wa[0] + wa[1] * wa[1] + wa[2] * wa[2]);
    for (int k = 0; k < 3; ++k) v[k] = wa[k] / vl;
    cross3(w, v, u);
    for (int k = 0; k < 3; ++k) {
      q.origin[k] = h.p[k];
      q.dir[k] = x * u[k] + y * v[k] + z * w[k];  // Onb::local (onb.rs:24-26)
    }
  }
  return 0;
}

int rth_preset(rth_scene* s, const char* name, const char* variant, int32_t width, int32_t spp,
               int32_t depth, double aspect, int32_t* world_out, int32_t* lights_out,
               rt_camera* cam_out) {
  CHECK_S(s);
  Preset p;
  std::string err;
  if (!preset(name ? name : "", variant ? variant : "", s->rng, width, spp, depth, aspect, &p, &err))
    return fail(err);
  *world_out = push(s->objects, p.world);
  *lights_out = p.lights ? push(s->objects, p.lights) : -1;
  *cam_out = p.cam;
  return 0;
}

// ---------------------------------------------------------------- output stage (color.rs)
static double linear_to_gamma(double linear) {  // color.rs:53-59
  if (linear <= 0.0031308) return 12.92 * linear;
  return 1.055 * std::pow(linear, 1. / 2.4) - 0.055;
}
static double exposure(double linear, double v) {  // color.rs:37-39: 1 - E^(-v*linear)
  return 1. - std::pow(2.718281828459045, -v * linear);
}
// Rust `f64 as u8`: saturating, NaN -> 0.
static uint8_t as_u8(double x) {
  if (!(x == x)) return 0;
  if (x <= 0.) return 0;
  if (x >= 255.) return 255;
  return (uint8_t)x;
}

double rth_auto_expose(const float* accum, int64_t n, int32_t spp) {  // render.rs:325-339
  double medium_weight = 1. / (double)n;
  double medium_point = 0.;
  for (int64_t i = 0; i < n; ++i) {
    double lum = 0.2126 * accum[3 * i] + 0.71516 * accum[3 * i + 1] + 0.072169 * accum[3 * i + 2];
    medium_point = medium_point + medium_weight * (lum * lum);
  }
  medium_point = medium_point / (double)((int64_t)spp * spp);
  if (medium_point > 0.001) return -std::log(0.6) / std::sqrt(medium_point);
  return 1.;
}

int rth_write_color(const float* accum, int64_t n, double spp, int use_exposure, double ev,
                    uint8_t* out) {  // color.rs:8-33
  double scale = 1.0 / spp;
  for (int64_t i = 0; i < 3 * n; ++i) {
    double x = (double)accum[i] * scale;
    if (use_exposure) x = exposure(x, ev);
    x = linear_to_gamma(x);
    if (x < 0.) x = 0.;             // Interval{0, 0.999}.clamp (interval.rs:29-37)
    else if (x > 0.999) x = 0.999;  // NaN falls through both tests, as in the reference
    out[i] = as_u8(256. * x);
  }
  return 0;
}

int rth_write_ppm(const char* path, const uint8_t* rgb, int32_t w, int32_t h) {
  // Same text as render.rs:151 + write_color's "r g b\n" lines.
  FILE* f = std::fopen(path, "w");
  if (!f) return fail(std::string("cannot open ") + path);
  std::fprintf(f, "P3\n%d %d\n255\n", w, h);
  for (int64_t i = 0; i < (int64_t)w * h; ++i)
    std::fprintf(f, "%d %d %d\n", rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  std::fclose(f);
  return 0;
}

}  // extern "C"
