/*
 * rt_host.h — C API of the host-side scene builder `librthost.so`.
 *
 * The reference keeps scene construction in Rust (main.rs + the constructors of hittable.rs,
 * object.rs, transform.rs, constant_medium.rs, material.rs, texture.rs, perlin.rs). The north
 * star keeps that API on the host and hands a flattened buffer across the C ABI
 * (rt_mi355x.h). Rust is not available in this image, so the host mirror is C++
 * (surely-raytracing_amd/csrc/host/scene.hpp, same constructor vocabulary); this header exposes
 * it to C / ctypes / cgo-style callers. Every constructor cites the reference function whose
 * construction-time arithmetic it restates.
 *
 * Object/material/texture handles are small non-negative int32 ids owned by an rth_scene.
 * Negative return = error (message in rth_last_error()).
 */
#ifndef RT_HOST_H
#define RT_HOST_H

#include <stdint.h>
#include "rt_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rth_scene rth_scene;

const char* rth_last_error(void);

/* Scene-build randomness (main.rs:617,688; hittable.rs:150; perlin.rs:19,111) comes from one
 * seeded stream owned by the scene. */
rth_scene* rth_scene_new(uint64_t build_seed);
void rth_scene_free(rth_scene* s);
double rth_random_double(rth_scene* s);                       /* utils.rs:5-7   */
double rth_random_range(rth_scene* s, double min, double max); /* utils.rs:9-11  */
int64_t rth_random_int(rth_scene* s, int64_t min, int64_t max); /* utils.rs:13-15 */

/* textures (texture.rs) */
int32_t rth_solid_color(rth_scene* s, double r, double g, double b);              /* :36-39   */
int32_t rth_checker_texture(rth_scene* s, double scale, int32_t even, int32_t odd); /* :55-61 */
int32_t rth_noise_texture(rth_scene* s, double scale); /* :116-121, Perlin::new perlin.rs:15-28 */
int32_t rth_image_texture(rth_scene* s, int32_t width, int32_t height,
                          const uint8_t* rgb8); /* :89-93; width=height=0 -> absent image */

/* materials (material.rs) */
int32_t rth_lambertian(rth_scene* s, double r, double g, double b); /* :81-85  */
int32_t rth_lambertian_tex(rth_scene* s, int32_t tex);                /* :87-89  */
int32_t rth_metal(rth_scene* s, double r, double g, double b, double fuzz); /* :118-121 */
int32_t rth_dielectric(rth_scene* s, double ir, double r, double g, double b); /* :148-154 */
int32_t rth_diffuse_light(rth_scene* s, double r, double g, double b); /* :200-204 */
int32_t rth_diffuse_light_tex(rth_scene* s, int32_t tex);               /* :206-208 */
int32_t rth_isotropic(rth_scene* s, double r, double g, double b);     /* :230-234 */
int32_t rth_isotropic_tex(rth_scene* s, int32_t tex);                   /* :236-238 */

/* objects (object.rs, hittable.rs, transform.rs, constant_medium.rs) */
int32_t rth_sphere(rth_scene* s, const double center[3], double radius, int32_t mat); /* :83-92 */
int32_t rth_sphere_moving(rth_scene* s, const double c1[3], const double c2[3], double radius,
                          int32_t mat);                                            /* :94-105 */
int32_t rth_quad(rth_scene* s, const double q[3], const double u[3], const double v[3],
                 int32_t mat);                                                     /* :427-446 */
int32_t rth_make_box(rth_scene* s, const double a[3], const double b[3], int32_t mat); /* :509-560 */
int32_t rth_list_new(rth_scene* s);                                   /* hittable.rs:61-66  */
int32_t rth_list_add(rth_scene* s, int32_t list, int32_t obj);        /* hittable.rs:74-80  */
int32_t rth_list_create_bvh(rth_scene* s, int32_t list);              /* hittable.rs:82-84  */
int32_t rth_list_len(rth_scene* s, int32_t list);
int32_t rth_translate(rth_scene* s, int32_t obj, const double offset[3]); /* transform.rs:43-54 */
int32_t rth_rotate_y(rth_scene* s, int32_t obj, double angle_deg);     /* transform.rs:143-186 */
int32_t rth_constant_medium(rth_scene* s, int32_t boundary, double density, double r, double g,
                            double b);                            /* constant_medium.rs:21-27 */
int32_t rth_constant_medium_tex(rth_scene* s, int32_t boundary, double density, int32_t tex);
int rth_object_bbox(rth_scene* s, int32_t obj, double out6[6]);

/* Serialise world (a list) + lights (any object, or -1 = empty list as render_par) into the
 * rt_scene_blob format. The blob memory is owned by `s` and valid until the next call. */
int rth_serialize(rth_scene* s, int32_t world_list, int32_t lights, rt_scene_blob* out);

/* Camera::new (render.rs:62-133) in f64; spp is rounded by nearest_square (render.rs:38-41). */
int rth_camera_new(double aspect_ratio, int32_t image_width, int32_t samples_per_pixel,
                   int32_t max_depth, double vfov, const double lookfrom[3],
                   const double lookat[3], const double vup[3], double defocus_angle,
                   double focus_dist, const double background[3], rt_camera* out);

/* Turn a camera `degrees` about the vertical (y) axis through `pivot`, in RotateY's sense
 * (transform.rs:143-186): center and pixel00_loc turn about the pivot, both pixel deltas and both
 * defocus vectors about the origin. rt_camera holds only Camera's derived fields, so this is how a
 * caller moves one (an orbit, a turntable; the camera motion rt_temporal_* reprojects across).
 * degrees == 0 is a bitwise copy; out may be in. */
int rth_camera_orbit_y(const rt_camera* in, const double pivot[3], double degrees, rt_camera* out);

/* Scene presets restating main.rs (scene fns + their Camera::new literals). Overrides <= 0 keep
 * the reference value. variant: "" or "mixed_pdf" (cornell_box with box2 and lights = quad only,
 * the revision behind final_images/mixed_pdf.png). Names: cornell_box, cornell_smoke,
 * final_scene, quads, simple_light, two_spheres, two_perlin_spheres, random_balls,
 * three_spheres, earth. */
int rth_preset(rth_scene* s, const char* name, const char* variant, int32_t width,
               int32_t samples_per_pixel, int32_t max_depth, double aspect_ratio,
               int32_t* world_out, int32_t* lights_out, rt_camera* cam_out);

/* Output stage (color.rs:8-59, render.rs:325-339): raw sums -> sRGB8 exactly as write_color. */
double rth_auto_expose(const float* accum, int64_t n_pixels, int32_t samples_per_pixel);
int rth_write_color(const float* accum, int64_t n_pixels, double samples_per_pixel,
                    int use_exposure, double exposure, uint8_t* rgb8_out);
int rth_write_ppm(const char* path, const uint8_t* rgb8, int32_t width, int32_t height);

/* Host ray generator for rt_render_rays (rt_mi355x.h): the rt_ray of every pixel of a width x
 * height frame for ONE stratum (s_i, s_j) of sqrt_spp x sqrt_spp, out[j * width + i]. Each ray
 * carries pixel = j * width + i, sample = s_j * sqrt_spp + s_i, tmin = 1e-4, tmax = +inf, and the
 * generator rng_seed(seed, pixel, sample) (csrc/rt_rng.h) supplies, in this order, the two jitter
 * draws and the time draw (ray.time), as get_ray does for a camera without defocus
 * (render.rs:218-249). Frames made here are therefore rendered with stream_skip = 3 and
 * RT_RAYS_STREAM_TIME, one path per ray and pass, accumulating over the S * S strata.
 * The sample's position in its pixel is (px, py) = (rs * (s_i + draw1) - 0.5, rs * (s_j + draw2) -
 * 0.5), rs = 1 / sqrt_spp, and x = (i + 0.5 + px) / width, y = (j + 0.5 + py) / height, y down.
 * Frame of the last three kinds: f = unit(forward), r = unit(f x up), u = r x f.
 *   RTH_PROJ_PINHOLE   cam's own ray without its lens: get_ray restated with the same fma forms
 *                      (origin cam->center, dir not normalised); width, height, sqrt_spp, origin,
 *                      forward, up and fov are not read (the camera's are used).
 *   RTH_PROJ_ORTHO     dir = f (unit); origin + (x - 0.5) * fov * width / height * r + (0.5 - y) *
 *                      fov * u: fov is the height of the view volume in world units.
 *   RTH_PROJ_PANORAMA  equirectangular, full sphere: lon = (x - 0.5) * 2 pi, lat = (0.5 - y) * pi,
 *                      dir = cos(lat) * (sin(lon) * r + cos(lon) * f) + sin(lat) * u (unit length
 *                      to rounding); the frame's centre looks along f, its top row up.
 *   RTH_PROJ_FISHEYE   equidistant: with m = min(width, height), (nx, ny) = ((2x - 1) * width / m,
 *                      (1 - 2y) * height / m), theta = hypot(nx, ny) * fov / 2 (fov: the full angle
 *                      in degrees across the short side), phi = atan2(ny, nx), dir = sin(theta) *
 *                      (cos(phi) * r + sin(phi) * u) + cos(theta) * f (unit length to rounding). A
 *                      pixel with theta > pi lies outside the sphere: its dir is all zero, an
 *                      invalid ray, which rt_render_rays answers with NaN.
 * Returns 0, or -1 (rth_last_error): null arguments, sizes < 1, a stratum outside sqrt_spp, an
 * unknown kind, a zero or non-finite frame vector, a non-positive fov where it is read. */
#define RTH_PROJ_PINHOLE 0
#define RTH_PROJ_ORTHO 1
#define RTH_PROJ_PANORAMA 2
#define RTH_PROJ_FISHEYE 3
typedef struct rth_projection {   /* 96 bytes, no padding */
  int32_t kind;                   /* RTH_PROJ_* */
  int32_t width, height, sqrt_spp;
  double origin[3], forward[3], up[3];
  double fov;
} rth_projection;
int rth_projection_rays(const rth_projection* proj, const rt_camera* cam /* pinhole only */,
                        uint64_t seed, int32_t s_i, int32_t s_j, rt_ray* out);

/* Host generator of ambient-occlusion ray batches for any-hit queries (rt_mi355x.h, RT_QUERY_ANY_HIT):
 * from a batch of primary rays and their records (rt_query_rays, record mode), the k-th of K
 * cosine-distributed directions about each hit's normal. For ray i with hits[i].hit == 1 the
 * generator rng_seed(seed, primary[i].pixel, dir_index) (csrc/rt_rng.h) supplies r1 and r2, the local
 * direction is random_cosine_direction's (vec3.rs:240-250), the frame Onb::build_from_w(hits[i].
 * normal) (onb.rs:32-47) and dir = local(x, y, z) (unit length to rounding, dir . normal >= 0);
 * origin = hits[i].p, time = primary[i].time, tmin = p->tmin, tmax = p->radius, pixel = primary[i].
 * pixel, sample = dir_index. For any other hits[i].hit, dir is all zero and origin 0 (the other
 * fields as above): an invalid ray, which the query answers with 255. A pixel's ambient occlusion
 * is then unoccluded / K over K batches. out may be primary.
 * Returns 0, or -1 (rth_last_error): null arguments, a tmin that is not finite or < 0, a radius
 * that is NaN or <= tmin, _pad0 != 0. */
typedef struct rth_ao_params {   /* 32 bytes, no padding */
  uint64_t seed;
  double radius;       /* becomes tmax; > tmin, may be +inf; NaN invalid */
  double tmin;         /* finite, >= 0; 1e-4 is the reference's */
  uint32_t dir_index;  /* k: which of the K directions this batch is */
  uint32_t _pad0;      /* must be 0 */
} rth_ao_params;
int rth_ao_rays(const rt_ray* primary, const rt_hit* hits, uint64_t n, const rth_ao_params* p,
                rt_ray* out);

#ifdef __cplusplus
}
#endif
#endif /* RT_HOST_H */
