// rt_render_cli — the host program: the reference's main() (main.rs:713-729) on this stack.
//
//   scene selector (main.rs:714-728) -> preset scene (C++ builder, rt_host.h)
//   -> rt_render (gfx950, rt_mi355x.h)    [render_par_lights, render.rs:144-216]
//   -> with --denoise: rt_render_aov + rt_denoise (the a-trous filter over the first-hit guides)
//   -> with --denoise-var: rt_render_moments + rt_render_aov + rt_denoise_var (the same filter
//      guided by the per-pixel variance of the row totals; needs spp >= 4)
//   -> with --adaptive T: rt_render_adaptive (tiles stop once their estimated relative error is
//      <= T) and the resolved frame; combines with --denoise (the filter reads the resolved frame)
//   -> auto_expose / write_color -> P3 PPM [render.rs:151, 199-215; color.rs:8-33]; with
//      --device-output the two run on the GPU (rt_output) over whichever frame the options made
//   -> with --frames N [--orbit DEG] [--temporal]: N frames, the camera turned DEG degrees per
//      frame about the vertical axis through the centre of the world's bounding box, frame f with
//      seed + f; each frame runs rt_render_moments, rt_render_aov, with --temporal
//      rt_temporal_accumulate (the frame history reprojected and blended; with --denoise-var in
//      the scale of the accumulated mean's variance), then the denoise and output options above,
//      and is written to NAME_%03d.ppm
//   -> with --pick X Y: no render; rt_query_rays with the pixel-centre ray of the preset's camera,
//      `hit t distance p normal front material prim` on one line of stdout
//   -> with --projection ortho|panorama|fisheye [--fov F]: the frame's rays come from
//      rth_projection_rays (eye, view direction and up of the preset's camera) and are path traced
//      by rt_render_rays, S * S passes of one path per ray accumulated without RT_FLAG_OVERWRITE;
//      the output options apply to the frame as to any other (the denoisers, --adaptive, --frames
//      and --pick need the pinhole camera's AOVs or tiles and do not combine)
//   -> with --ao K [--ao-radius R]: no path tracing; the pixel-centre rays (as --pick forms them)
//      go to one record query, then K passes of rth_ao_rays and an any-hit query (RT_QUERY_ANY_HIT)
//      over [1e-4, R] (default: no limit); a pixel is unoccluded / K in all three channels through
//      write_color, a pixel that sees no surface 0; does not combine with the render modes
//   -> with --device-rays: the rays of --ao and --projection are formed on the GPU and stay there.
//      --ao: the primaries are uploaded once, rt_ambient_occlusion_device counts the unoccluded
//      directions and rt_output_device writes the frame; --projection: each pass's rays come from
//      rt_projection_rays_device straight into the buffer rt_render_rays_device reads, the sums
//      are downloaded once. Without the flag both run as above.
//
// Usage: rt_render_cli [--scene N|name] [--variant mixed_pdf] [--width W] [--spp S]
//                      [--depth D] [--aspect A] [--seed K] [--build-seed K] [--device N]
//                      [--reference-semantics] [--auto-exposure] [--denoise [levels]]
//                      [--denoise-var [levels]] [--adaptive threshold] [--passes P] [--floor F]
//                      [--device-output] [--frames N] [--orbit DEG] [--temporal] [--out file.ppm]
//                      [--pick X Y] [--projection ortho|panorama|fisheye] [--fov F]
//                      [--ao K] [--ao-radius R] [--device-rays]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>  // --device-rays: the buffers the *_device calls take

#include "../../../include/rt_host.h"
#include "../../../include/rt_mi355x.h"

static const char* scene_name(int n) {  // main.rs:715-728 selector values
  switch (n) {
    case -1: return "three_spheres";
    case 1: return "random_balls";
    case 2: return "two_spheres";
    case 3: return "earth";
    case 4: return "two_perlin_spheres";
    case 5: return "quads";
    case 6: return "simple_light";
    case 7: return "cornell_box";
    case 8: return "cornell_smoke";
    case 9: return "final_scene";
    default: return "final_scene";  // `_` arm: final_scene(400, 250, 4)
  }
}

// exposure, gamma and RGB8 of one frame, on the device or on the host, and the PPM
static int write_frame(const std::vector<float>& accum, const rt_camera& cam, bool device_output,
                       bool autoexp, int device, const std::string& path) {
  const int64_t n = (int64_t)cam.image_width * cam.image_height;
  std::vector<uint8_t> rgb(accum.size());
  if (device_output) {
    rt_output_stage* os = nullptr;
    rt_output_params op;
    std::memset(&op, 0, sizeof(op));
    op.width = cam.image_width;
    op.height = cam.image_height;
    op.flags = autoexp ? RT_OUTPUT_AUTO_EXPOSE : 0u;
    op.samples_per_pixel = (double)cam.samples_per_pixel;
    double ev = 0.0;
    rt_stats st_out;
    int rc = rt_output_create(device, &os);
    if (rc == RT_OK) rc = rt_output(os, &op, accum.data(), rgb.data(), &ev, &st_out);
    rt_output_destroy(os);
    if (rc != RT_OK) {
      std::fprintf(stderr, "rt_output: %d %s\n", rc, rt_last_error());
      return 1;
    }
    std::fprintf(stderr, "device output %.3f ms", st_out.ms_kernel);
    if (autoexp) std::fprintf(stderr, ", exposure %.17g", ev);
    std::fprintf(stderr, "\n");
  } else {
    double ev = autoexp ? rth_auto_expose(accum.data(), n, cam.samples_per_pixel) : 0.0;
    rth_write_color(accum.data(), n, (double)cam.samples_per_pixel, autoexp ? 1 : 0, ev, rgb.data());
  }
  if (rth_write_ppm(path.c_str(), rgb.data(), cam.image_width, cam.image_height) != 0) {
    std::fprintf(stderr, "%s\n", rth_last_error());
    return 1;
  }
  return 0;
}

// --frames: the orbit. Every frame: moments, AOVs, the temporal accumulation, the filter, the
// output stage, NAME_%03d.ppm.
static int render_frames(const rt_scene_blob& blob, const rt_camera& cam0, rt_render_opts o,
                         const double pivot[3], int frames, double orbit, bool temporal,
                         int denoise_levels, bool denoise_var, bool device_output, bool autoexp,
                         const std::string& out) {
  const int W = cam0.image_width, H = cam0.image_height;
  const size_t n_px = (size_t)W * H;
  std::vector<float> accum(n_px * 3, 0.f), m2(n_px * 3, 0.f), aov(n_px * RT_AOV_CHANNELS, 0.f);
  std::vector<float> len(n_px, 0.f);
  rt_scene* sc = nullptr;
  rt_temporal* tp = nullptr;
  rt_denoiser* dn = nullptr;
  rt_temporal_params tpar;
  rt_denoise_params dp;
  rt_denoise_var_params dvp;
  int rc = rt_scene_create(&blob, o.device, &sc);
  if (rc == RT_OK && temporal) rc = rt_temporal_create(o.device, &tp);
  if (rc == RT_OK && temporal) rc = rt_temporal_default_params(W, H, &tpar);
  if (rc == RT_OK && temporal) {
    tpar.beauty_rows = cam0.sqrt_spp;
    if (denoise_levels && denoise_var) tpar.flags |= RT_TEMPORAL_VARIANCE_OF_MEAN;
  }
  if (rc == RT_OK && denoise_levels) rc = rt_denoiser_create(o.device, &dn);
  if (rc == RT_OK && denoise_levels && denoise_var) {
    rc = rt_denoise_var_default_params(W, H, cam0.samples_per_pixel, cam0.sqrt_spp,
                                       cam0.samples_per_pixel, &dvp);
    if (rc == RT_OK && denoise_levels > 0) dvp.levels = denoise_levels;
  } else if (rc == RT_OK && denoise_levels) {
    rc = rt_denoise_default_params(W, H, cam0.samples_per_pixel, cam0.samples_per_pixel, &dp);
    if (rc == RT_OK && denoise_levels > 0) dp.levels = denoise_levels;
  }
  const std::string::size_type dot = out.rfind('.');
  const std::string stem = dot == std::string::npos ? out : out.substr(0, dot);
  const std::string ext = dot == std::string::npos ? "" : out.substr(dot);
  const uint64_t seed0 = o.seed;
  int status = 0;
  for (int f = 0; rc == RT_OK && status == 0 && f < frames; ++f) {
    rt_camera cam;
    if (rth_camera_orbit_y(&cam0, pivot, orbit * f, &cam) != 0) {
      std::fprintf(stderr, "%s\n", rth_last_error());
      status = 1;
      break;
    }
    o.seed = seed0 + (uint64_t)f;
    rt_stats st, st_aov, st_tp, st_dn;
    std::memset(&st_aov, 0, sizeof(st_aov));
    std::memset(&st_tp, 0, sizeof(st_tp));
    std::memset(&st_dn, 0, sizeof(st_dn));
    rc = rt_render_moments(sc, &cam, &o, accum.data(), m2.data(), &st);
    if (rc == RT_OK && (temporal || denoise_levels)) rc = rt_render_aov(sc, &cam, &o, aov.data(), &st_aov);
    double reused = 0.0;
    if (rc == RT_OK && temporal) {
      rc = rt_temporal_accumulate(tp, &tpar, &cam, accum.data(), m2.data(), aov.data(),
                                  accum.data(), m2.data(), len.data(), &st_tp);
      for (float l : len) reused += l > 1.f ? 1.0 : 0.0;
    }
    if (rc == RT_OK && denoise_levels && denoise_var)
      rc = rt_denoise_var(dn, &dvp, accum.data(), m2.data(), aov.data(), accum.data(), nullptr,
                          &st_dn);
    else if (rc == RT_OK && denoise_levels)
      rc = rt_denoise(dn, &dp, accum.data(), aov.data(), accum.data(), &st_dn);
    if (rc != RT_OK) break;
    std::fprintf(stderr,
                 "frame %d: kernel %.2f ms, aov %.2f ms, temporal %.3f ms (history at %.1f %% of "
                 "the pixels), denoise %.3f ms\n",
                 f, st.ms_kernel, st_aov.ms_kernel, st_tp.ms_kernel, 100.0 * reused / (double)n_px,
                 st_dn.ms_kernel);
    char num[16];
    std::snprintf(num, sizeof(num), "_%03d", f);
    const std::string path = stem + num + ext;
    status = write_frame(accum, cam, device_output, autoexp, o.device, path);
    if (status == 0) std::fprintf(stderr, "wrote %s\n", path.c_str());
  }
  if (rc != RT_OK) std::fprintf(stderr, "rt_render --frames: %d %s\n", rc, rt_last_error());
  rt_denoiser_destroy(dn);
  rt_temporal_destroy(tp);
  rt_scene_destroy(sc);
  return rc != RT_OK ? 1 : status;
}

// --pick X Y: the ray from the camera centre through the centre of pixel (X, Y) (no jitter, no
// defocus, time 0), one rt_query_rays over [1e-4, inf), one line on stdout:
//   hit t distance p normal front material prim
static int pick_pixel(const rt_scene_blob& blob, const rt_camera& cam, int x, int y, uint64_t seed,
                      int device) {
  if (x < 0 || y < 0 || x >= cam.image_width || y >= cam.image_height) {
    std::fprintf(stderr, "--pick %d %d: outside the %dx%d image\n", x, y, cam.image_width,
                 cam.image_height);
    return 2;
  }
  alignas(16) rt_ray r;  // the query takes 16-byte aligned records
  std::memset(&r, 0, sizeof(r));
  for (int k = 0; k < 3; ++k) {
    r.origin[k] = cam.center[k];
    r.dir[k] = cam.pixel00_loc[k] + x * cam.pixel_delta_u[k] + y * cam.pixel_delta_v[k] -
               cam.center[k];
  }
  r.tmin = 1e-4;
  r.tmax = HUGE_VAL;
  r.pixel = (uint32_t)(y * cam.image_width + x);
  rt_query_params qp;
  std::memset(&qp, 0, sizeof(qp));
  qp.seed = seed;
  alignas(16) rt_hit h;
  rt_scene* sc = nullptr;
  int rc = rt_scene_create(&blob, device, &sc);
  if (rc == RT_OK) rc = rt_query_rays(sc, &qp, &r, 1, &h, nullptr);
  rt_scene_destroy(sc);
  if (rc != RT_OK) {
    std::fprintf(stderr, "rt_query_rays: %d %s\n", rc, rt_last_error());
    return 1;
  }
  std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d\n", h.hit, h.t,
              h.distance, h.p[0], h.p[1], h.p[2], h.normal[0], h.normal[1], h.normal[2],
              h.front_face, h.material, h.prim);
  return 0;
}

// --device-rays: one device allocation, freed on every exit path
struct DeviceBuffer {
  void* p = nullptr;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
  bool alloc(int device, size_t bytes) {
    return hipSetDevice(device) == hipSuccess && hipMalloc(&p, bytes) == hipSuccess;
  }
};

// the pixel-centre rays of --ao, each formed as --pick forms its one ray
static std::vector<rt_ray> pixel_centre_rays(const rt_camera& cam) {
  const int W = cam.image_width, H = cam.image_height;
  std::vector<rt_ray> primary((size_t)W * H);  // operator new: 16-byte aligned
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      rt_ray& r = primary[(size_t)y * W + x];
      std::memset(&r, 0, sizeof(r));
      for (int k = 0; k < 3; ++k) {
        r.origin[k] = cam.center[k];
        r.dir[k] = cam.pixel00_loc[k] + x * cam.pixel_delta_u[k] + y * cam.pixel_delta_v[k] -
                   cam.center[k];
      }
      r.tmin = 1e-4;
      r.tmax = HUGE_VAL;
      r.pixel = (uint32_t)(y * W + x);
    }
  return primary;
}

// --ao K: ambient occlusion of the first hits. Record query, K x (rth_ao_rays, any-hit query).
static int render_ao(const rt_scene_blob& blob, const rt_camera& cam, int K, double radius,
                     uint64_t seed, int device, const std::string& out) {
  const int W = cam.image_width, H = cam.image_height;
  const size_t n = (size_t)W * H;
  // std::vector's allocation is 16-byte aligned for these 80-byte records (operator new)
  const std::vector<rt_ray> primary = pixel_centre_rays(cam);
  std::vector<rt_ray> ao(n);
  std::vector<rt_hit> hits(n);
  std::vector<uint8_t> occ(n);
  std::vector<float> sums(3 * n, 0.0f);
  rt_query_params qp;
  std::memset(&qp, 0, sizeof(qp));
  qp.seed = seed;
  rth_ao_params ap;
  std::memset(&ap, 0, sizeof(ap));
  ap.seed = seed;
  ap.radius = radius;
  ap.tmin = 1e-4;
  rt_scene* sc = nullptr;
  double ms = 0.0;
  int rc = rt_scene_create(&blob, device, &sc);
  if (rc == RT_OK) rc = rt_query_rays(sc, &qp, primary.data(), n, hits.data(), nullptr);
  qp.mode = RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT;
  for (int k = 0; k < K && rc == RT_OK; ++k) {
    ap.dir_index = (uint32_t)k;
    if (rth_ao_rays(primary.data(), hits.data(), n, &ap, ao.data()) != 0) {
      std::fprintf(stderr, "rth_ao_rays: %s\n", rth_last_error());
      rt_scene_destroy(sc);
      return 1;
    }
    rt_stats st;
    rc = rt_query_rays(sc, &qp, ao.data(), n, occ.data(), &st);
    if (rc != RT_OK) break;
    ms += st.ms_kernel;
    for (size_t i = 0; i < n; ++i)
      if (occ[i] == 0) sums[3 * i] += 1.0f, sums[3 * i + 1] += 1.0f, sums[3 * i + 2] += 1.0f;
  }
  rt_scene_destroy(sc);
  if (rc != RT_OK) {
    std::fprintf(stderr, "rt_query_rays: %d %s\n", rc, rt_last_error());
    return 1;
  }
  std::vector<uint8_t> rgb(3 * n);
  rth_write_color(sums.data(), (int64_t)n, (double)K, 0, 1.0, rgb.data());
  if (rth_write_ppm(out.c_str(), rgb.data(), W, H) != 0) {
    std::fprintf(stderr, "%s\n", rth_last_error());
    return 1;
  }
  std::fprintf(stderr, "ambient occlusion %dx%d, %d directions, radius %g: %.3f ms in any-hit kernels -> %s\n",
               W, H, K, radius, ms, out.c_str());
  return 0;
}

// --ao K --device-rays: the primaries go up once; records, AO rays, occlusion bytes and the count
// stay on the device (rt_ambient_occlusion_device), rt_output_device writes the RGB8 frame.
static int render_ao_device(const rt_scene_blob& blob, const rt_camera& cam, int K, double radius,
                            uint64_t seed, int device, const std::string& out) {
  const int W = cam.image_width, H = cam.image_height;
  const size_t n = (size_t)W * H;
  const std::vector<rt_ray> primary = pixel_centre_rays(cam);
  DeviceBuffer d_primary, d_sums, d_rgb;
  if (!d_primary.alloc(device, n * sizeof(rt_ray)) || !d_sums.alloc(device, 3 * n * sizeof(float)) ||
      !d_rgb.alloc(device, 3 * n) ||
      hipMemcpy(d_primary.p, primary.data(), n * sizeof(rt_ray), hipMemcpyHostToDevice) !=
          hipSuccess) {
    std::fprintf(stderr, "--device-rays: device buffers: %s\n",
                 hipGetErrorString(hipGetLastError()));
    return 1;
  }
  rt_ao_frame_params fp;
  std::memset(&fp, 0, sizeof(fp));
  fp.seed = seed;
  fp.radius = radius;
  fp.tmin = 1e-4;
  fp.directions = (uint32_t)K;
  fp.flags = RT_FLAG_OVERWRITE;
  fp.channels = 3;
  rt_output_params op;
  std::memset(&op, 0, sizeof(op));
  op.width = W;
  op.height = H;
  op.samples_per_pixel = (double)K;
  rt_scene* sc = nullptr;
  rt_raygen* rg = nullptr;
  rt_output_stage* os = nullptr;
  rt_stats st, st_out;
  std::vector<uint8_t> rgb(3 * n);
  int rc = rt_scene_create(&blob, device, &sc);
  if (rc == RT_OK) rc = rt_raygen_create(device, &rg);
  if (rc == RT_OK) rc = rt_output_create(device, &os);
  if (rc == RT_OK)
    rc = rt_ambient_occlusion_device(rg, sc, &fp, (const rt_ray*)d_primary.p, n, (float*)d_sums.p,
                                     nullptr, nullptr, &st);
  if (rc == RT_OK)
    rc = rt_output_device(os, &op, (const float*)d_sums.p, (uint8_t*)d_rgb.p, nullptr, nullptr,
                          &st_out);
  if (rc != RT_OK) std::fprintf(stderr, "--ao --device-rays: %d %s\n", rc, rt_last_error());
  rt_output_destroy(os);
  rt_raygen_destroy(rg);
  rt_scene_destroy(sc);
  if (rc != RT_OK) return 1;
  if (hipMemcpy(rgb.data(), d_rgb.p, 3 * n, hipMemcpyDeviceToHost) != hipSuccess) {
    std::fprintf(stderr, "--device-rays: download: %s\n", hipGetErrorString(hipGetLastError()));
    return 1;
  }
  if (rth_write_ppm(out.c_str(), rgb.data(), W, H) != 0) {
    std::fprintf(stderr, "%s\n", rth_last_error());
    return 1;
  }
  std::fprintf(stderr,
               "ambient occlusion %dx%d, %d directions, radius %g, rays on the device: %.3f ms in %u "
               "kernels, output %.3f ms -> %s\n",
               W, H, K, radius, st.ms_kernel, st.launches, st_out.ms_kernel, out.c_str());
  return 0;
}

// --projection: the preset's eye and view frame, another projection. fov <= 0: the height of the
// pinhole's viewport for ortho, 180 degrees for fisheye. Pixels whose ray is invalid (a fisheye
// pixel outside the sphere) come back NaN and are written black.
// device_rays: each pass's rays are formed by rt_projection_rays_device in the buffer
// rt_render_rays_device reads; the sums stay on the device until the last pass.
static int render_projection(const rt_scene_blob& blob, const rt_camera& cam, int kind, double fov,
                             uint64_t seed, uint32_t flags, int device, bool device_rays,
                             std::vector<float>& accum, rt_stats* total) {
  const int W = cam.image_width, H = cam.image_height, S = cam.sqrt_spp;
  rth_projection pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.kind = kind;
  pr.width = W;
  pr.height = H;
  pr.sqrt_spp = S;
  double vh = 0.0;
  for (int k = 0; k < 3; ++k) {
    pr.origin[k] = cam.center[k];
    pr.forward[k] = cam.pixel00_loc[k] + 0.5 * (W - 1) * cam.pixel_delta_u[k] +
                    0.5 * (H - 1) * cam.pixel_delta_v[k] - cam.center[k];
    pr.up[k] = -cam.pixel_delta_v[k];
    vh += cam.pixel_delta_v[k] * cam.pixel_delta_v[k];
  }
  pr.fov = fov > 0.0 ? fov : (kind == RTH_PROJ_ORTHO ? std::sqrt(vh) * H : 180.0);
  rt_rays_params rp;
  std::memset(&rp, 0, sizeof(rp));
  rp.seed = seed;
  rp.mode = RT_RAYS_STREAM_TIME;
  rp.sqrt_paths = 1;
  rp.max_depth = cam.max_depth;
  rp.stream_skip = 3;  // the generator's two jitter draws and its time draw
  for (int k = 0; k < 3; ++k) rp.background[k] = cam.background[k];
  const size_t n_rays = (size_t)W * H;
  std::vector<rt_ray> rays(device_rays ? 0 : n_rays);  // operator new: 16-byte aligned
  DeviceBuffer d_rays, d_accum;
  rt_projection dpr;  // the layout of rth_projection
  static_assert(sizeof(dpr) == sizeof(pr), "rt_projection mirrors rth_projection");
  std::memcpy(&dpr, &pr, sizeof(dpr));
  rt_scene* sc = nullptr;
  rt_raygen* rg = nullptr;
  int rc = rt_scene_create(&blob, device, &sc);
  std::memset(total, 0, sizeof(*total));
  if (rc == RT_OK && device_rays) {
    if (!d_rays.alloc(device, n_rays * sizeof(rt_ray)) ||
        !d_accum.alloc(device, accum.size() * sizeof(float))) {
      std::fprintf(stderr, "--device-rays: device buffers: %s\n",
                   hipGetErrorString(hipGetLastError()));
      rt_scene_destroy(sc);
      return 1;
    }
    rc = rt_raygen_create(device, &rg);
  }
  double ms_gen = 0.0;
  for (int s_j = 0; rc == RT_OK && device_rays && s_j < S; ++s_j)
    for (int s_i = 0; rc == RT_OK && s_i < S; ++s_i) {
      rt_stats st_gen, st;
      rc = rt_projection_rays_device(rg, &dpr, nullptr, seed, s_i, s_j, 0, H, (rt_ray*)d_rays.p,
                                     nullptr, &st_gen);
      if (rc != RT_OK) break;
      rp.flags = (flags & ~RT_FLAG_OVERWRITE) | (s_i + s_j == 0 ? RT_FLAG_OVERWRITE : 0u);
      rc = rt_render_rays_device(sc, &rp, (const rt_ray*)d_rays.p, n_rays, (float*)d_accum.p,
                                 nullptr, &st);
      ms_gen += st_gen.ms_kernel;
      total->ms_kernel += st.ms_kernel;
      total->samples += st.samples;
      total->launches += st.launches;
    }
  if (device_rays) {
    rt_raygen_destroy(rg);
    if (rc == RT_OK && hipMemcpy(accum.data(), d_accum.p, accum.size() * sizeof(float),
                                 hipMemcpyDeviceToHost) != hipSuccess) {
      std::fprintf(stderr, "--device-rays: download: %s\n", hipGetErrorString(hipGetLastError()));
      rt_scene_destroy(sc);
      return 1;
    }
    if (rc == RT_OK)
      std::fprintf(stderr, "rays formed on the device: %.3f ms in %d kernels\n", ms_gen, S * S);
  }
  for (int s_j = 0; rc == RT_OK && !device_rays && s_j < S; ++s_j)
    for (int s_i = 0; rc == RT_OK && s_i < S; ++s_i) {
      if (rth_projection_rays(&pr, nullptr, seed, s_i, s_j, rays.data()) != 0) {
        std::fprintf(stderr, "projection: %s\n", rth_last_error());
        rt_scene_destroy(sc);
        return 1;
      }
      rp.flags = (flags & ~RT_FLAG_OVERWRITE) | (s_i + s_j == 0 ? RT_FLAG_OVERWRITE : 0u);
      rt_stats st;
      rc = rt_render_rays(sc, &rp, rays.data(), rays.size(), accum.data(), &st);
      total->ms_kernel += st.ms_kernel;
      total->samples += st.samples;
      total->launches += st.launches;
    }
  rt_scene_destroy(sc);
  if (rc != RT_OK) {
    std::fprintf(stderr, "rt_render_rays%s: %d %s\n", device_rays ? " --device-rays" : "", rc,
                 rt_last_error());
    return 1;
  }
  for (float& v : accum)
    if (v != v) v = 0.f;
  return 0;
}

int main(int argc, char** argv) {
  std::string scene = "cornell_box", variant, out = "image.ppm";
  int width = 0, spp = 0, depth = 0, device = 0;
  double aspect = 0;
  uint64_t seed = 1, build_seed = 1;
  bool refsem = false, autoexp = false;
  bool device_output = false;  // exposure, gamma and RGB8 through rt_output, not on the host
  int denoise_levels = 0;  // 0 = no denoising
  bool denoise_var = false;  // the variance-guided filter instead of the plain one
  bool adaptive = false;
  double ad_threshold = 0.0, ad_floor = 1e-2;
  int ad_passes = 0;  // 0 = min(8, sqrt_spp / 2)
  int frames = 0;  // 0 = one frame, written to --out itself
  double orbit = 0.0;  // degrees per frame
  bool temporal = false;
  int ao_k = 0;  // > 0: ambient occlusion with ao_k directions per pixel instead of a render
  double ao_radius = HUGE_VAL;
  bool pick = false;  // one ray query through pixel (pick_x, pick_y) instead of a render
  int pick_x = 0, pick_y = 0;
  int projection = RTH_PROJ_PINHOLE;  // another one: the frame through rt_render_rays
  bool device_rays = false;  // --ao and --projection form their rays on the GPU
  double fov = 0.0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "missing value for %s\n", a.c_str());
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "--scene") {
      std::string v = next();
      char* end = nullptr;
      long n = std::strtol(v.c_str(), &end, 10);
      if (end && *end == 0) {
        scene = scene_name((int)n);
        if (n != 9 && std::string(scene) == "final_scene") {  // `_` arm parameters
          if (!width) width = 400;
          if (!spp) spp = 250;
          if (!depth) depth = 4;
        }
      } else {
        scene = v;
      }
    } else if (a == "--variant") variant = next();
    else if (a == "--width") width = std::atoi(next());
    else if (a == "--spp") spp = std::atoi(next());
    else if (a == "--depth") depth = std::atoi(next());
    else if (a == "--aspect") aspect = std::atof(next());
    else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
    else if (a == "--build-seed") build_seed = std::strtoull(next(), nullptr, 10);
    else if (a == "--device") device = std::atoi(next());
    else if (a == "--reference-semantics") refsem = true;
    else if (a == "--auto-exposure") autoexp = true;
    else if (a == "--denoise" || a == "--denoise-var") {  // the level count is optional
      denoise_var = a == "--denoise-var";
      denoise_levels = -1;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9')
        denoise_levels = std::atoi(argv[++i]);
    } else if (a == "--adaptive") {
      adaptive = true;
      ad_threshold = std::atof(next());
    } else if (a == "--passes") ad_passes = std::atoi(next());
    else if (a == "--floor") ad_floor = std::atof(next());
    else if (a == "--device-output") device_output = true;
    else if (a == "--frames") frames = std::atoi(next());
    else if (a == "--orbit") orbit = std::atof(next());
    else if (a == "--temporal") temporal = true;
    else if (a == "--out") out = next();
    else if (a == "--pick") {
      pick = true;
      pick_x = std::atoi(next());
      pick_y = std::atoi(next());
    } else if (a == "--projection") {
      const std::string v = next();
      projection = v == "ortho" ? RTH_PROJ_ORTHO : v == "panorama" ? RTH_PROJ_PANORAMA
                   : v == "fisheye" ? RTH_PROJ_FISHEYE : -1;
      if (projection < 0) {
        std::fprintf(stderr, "--projection %s: ortho, panorama or fisheye\n", v.c_str());
        return 2;
      }
    } else if (a == "--fov") fov = std::atof(next());
    else if (a == "--ao") {
      ao_k = std::atoi(next());
      if (ao_k < 1) {
        std::fprintf(stderr, "--ao K: K >= 1 directions per pixel\n");
        return 2;
      }
    } else if (a == "--ao-radius") ao_radius = std::atof(next());
    else if (a == "--device-rays") device_rays = true;
    else {
      std::fprintf(stderr, "unknown argument %s\n", a.c_str());
      return 2;
    }
  }
  if (adaptive && denoise_levels && denoise_var) {
    std::fprintf(stderr,
                 "--adaptive does not combine with --denoise-var: that filter takes one beauty_rows "
                 "for the whole frame, and an adaptive frame holds a different number of stratum "
                 "rows per tile (use --denoise, which reads the resolved frame)\n");
    return 2;
  }
  if (frames < 0 || ((orbit != 0.0 || temporal) && frames == 0) || (frames && adaptive)) {
    std::fprintf(stderr,
                 "--orbit and --temporal need --frames N (N >= 1); --frames does not combine with "
                 "--adaptive (rt_temporal takes one sample count for the whole frame)\n");
    return 2;
  }
  if (projection != RTH_PROJ_PINHOLE && (denoise_levels || adaptive || frames || pick)) {
    std::fprintf(stderr,
                 "--projection does not combine with --denoise, --denoise-var, --adaptive, --frames "
                 "or --pick: they take the pinhole camera's AOVs, tiles or pixels\n");
    return 2;
  }
  if (ao_k && (denoise_levels || adaptive || frames || pick || projection != RTH_PROJ_PINHOLE ||
               device_output || autoexp)) {
    std::fprintf(stderr,
                 "--ao does not combine with --denoise, --denoise-var, --adaptive, --frames, --pick, "
                 "--projection, --device-output or --auto-exposure: it renders no radiance\n");
    return 2;
  }
  if (device_rays && !ao_k && projection == RTH_PROJ_PINHOLE) {
    std::fprintf(stderr,
                 "--device-rays needs --ao or --projection: the other modes take no caller rays\n");
    return 2;
  }
  if (ao_k && !(ao_radius > 1e-4)) {
    std::fprintf(stderr, "--ao-radius R: R > 1e-4\n");
    return 2;
  }
  rth_scene* s = rth_scene_new(build_seed);
  int32_t world = -1, lights = -1;
  rt_camera cam;
  if (rth_preset(s, scene.c_str(), variant.c_str(), width, spp, depth, aspect, &world, &lights,
                 &cam) != 0) {
    std::fprintf(stderr, "preset: %s\n", rth_last_error());
    return 1;
  }
  rt_scene_blob blob;
  if (rth_serialize(s, world, lights, &blob) != 0) {
    std::fprintf(stderr, "serialize: %s\n", rth_last_error());
    return 1;
  }
  if (pick) {
    const int status = pick_pixel(blob, cam, pick_x, pick_y, seed, device);
    rth_scene_free(s);
    return status;
  }
  if (ao_k) {
    const int status = device_rays ? render_ao_device(blob, cam, ao_k, ao_radius, seed, device, out)
                                   : render_ao(blob, cam, ao_k, ao_radius, seed, device, out);
    rth_scene_free(s);
    return status;
  }
  std::fprintf(stderr, "Rendering %s %dx%d, %d spp (requested %d), depth %d on HIP device %d\n",
               scene.c_str(), cam.image_width, cam.image_height, cam.samples_per_pixel,
               spp ? spp : cam.samples_per_pixel, cam.max_depth, device);
  rt_render_opts o;
  std::memset(&o, 0, sizeof(o));
  o.seed = seed;
  o.row_begin = 0;
  o.row_step = 1;
  o.n_rows = cam.image_height;
  o.flags = RT_FLAG_OVERWRITE | (refsem ? RT_FLAG_SEMANTICS_REFERENCE : 0u);
  o.device = device;
  if (frames) {
    double box[6];
    if (rth_object_bbox(s, world, box) != 0) {
      std::fprintf(stderr, "bbox: %s\n", rth_last_error());
      return 1;
    }
    const double pivot[3] = {0.5 * (box[0] + box[1]), 0.5 * (box[2] + box[3]),
                             0.5 * (box[4] + box[5])};
    const int status = render_frames(blob, cam, o, pivot, frames, orbit, temporal, denoise_levels,
                                     denoise_var, device_output, autoexp, out);
    rth_scene_free(s);
    return status;
  }
  std::vector<float> accum((size_t)cam.image_width * cam.image_height * 3, 0.f);
  rt_stats st;
  int rc;
  if (projection != RTH_PROJ_PINHOLE) {
    if (render_projection(blob, cam, projection, fov, seed, o.flags, device, device_rays, accum,
                          &st) != 0)
      return 1;
  } else if (adaptive) {
    // the adaptive driver; with --denoise the plain filter over its resolved frame
    rt_scene* sc = nullptr;
    rt_adaptive* ad = nullptr;
    rt_denoiser* dn = nullptr;
    rt_adaptive_params ap;
    ap.passes = ad_passes > 0 ? ad_passes : std::max(1, std::min(8, cam.sqrt_spp / 2));
    ap.min_passes = 1;
    ap.threshold = ad_threshold;
    ap.floor = ad_floor;
    std::vector<float> sums(accum.size(), 0.f), m2(accum.size(), 0.f);
    std::vector<uint32_t> per((size_t)ap.passes, 0u);
    rc = rt_scene_create(&blob, device, &sc);
    if (rc == RT_OK) rc = rt_adaptive_create(device, &ad);
    if (rc == RT_OK)
      rc = rt_render_adaptive(ad, sc, &cam, &o, &ap, sums.data(), m2.data(), accum.data(), nullptr,
                              nullptr, per.data(), &st);
    if (rc == RT_OK) {
      const uint64_t total = (uint64_t)cam.image_width * cam.image_height * cam.samples_per_pixel;
      std::fprintf(stderr, "adaptive: traced %llu of %llu samples (%.1f %%), tiles per pass:",
                   (unsigned long long)st.samples, (unsigned long long)total,
                   100.0 * (double)st.samples / (double)total);
      for (uint32_t t : per) std::fprintf(stderr, " %u", t);
      std::fprintf(stderr, "\n");
    }
    if (rc == RT_OK && denoise_levels) {
      rt_denoise_params dp;
      std::vector<float> aov((size_t)cam.image_width * cam.image_height * RT_AOV_CHANNELS, 0.f);
      rt_stats st_aov, st_dn;
      rc = rt_denoise_default_params(cam.image_width, cam.image_height, cam.samples_per_pixel,
                                     cam.samples_per_pixel, &dp);
      if (rc == RT_OK && denoise_levels > 0) dp.levels = denoise_levels;
      if (rc == RT_OK) rc = rt_render_aov(sc, &cam, &o, aov.data(), &st_aov);
      if (rc == RT_OK) rc = rt_denoiser_create(device, &dn);
      if (rc == RT_OK) rc = rt_denoise(dn, &dp, accum.data(), aov.data(), accum.data(), &st_dn);
      if (rc == RT_OK)
        std::fprintf(stderr, "aov %.2f ms, denoise (%d levels) %.3f ms\n", st_aov.ms_kernel,
                     dp.levels, st_dn.ms_kernel);
    }
    if (rc != RT_OK) std::fprintf(stderr, "rt_render --adaptive: %d %s\n", rc, rt_last_error());
    rt_denoiser_destroy(dn);
    rt_adaptive_destroy(ad);
    rt_scene_destroy(sc);
    if (rc != RT_OK) return 1;
  } else if (!denoise_levels) {
    rc = rt_render_blob(&blob, &cam, &o, accum.data(), &st);
    if (rc != RT_OK) {
      std::fprintf(stderr, "rt_render: %d %s\n", rc, rt_last_error());
      return 1;
    }
  } else if (denoise_var) {
    // the moments render, the first-hit AOVs of the same camera, options and seed, the filter
    rt_scene* sc = nullptr;
    rt_denoiser* dn = nullptr;
    rt_denoise_var_params dp;
    std::vector<float> m2(accum.size(), 0.f);
    std::vector<float> aov((size_t)cam.image_width * cam.image_height * RT_AOV_CHANNELS, 0.f);
    rt_stats st_aov, st_dn;
    rc = rt_denoise_var_default_params(cam.image_width, cam.image_height, cam.samples_per_pixel,
                                       cam.sqrt_spp, cam.samples_per_pixel, &dp);
    if (rc == RT_OK && denoise_levels > 0) dp.levels = denoise_levels;
    if (rc == RT_OK) rc = rt_scene_create(&blob, device, &sc);
    if (rc == RT_OK) rc = rt_render_moments(sc, &cam, &o, accum.data(), m2.data(), &st);
    if (rc == RT_OK) rc = rt_render_aov(sc, &cam, &o, aov.data(), &st_aov);
    if (rc == RT_OK) rc = rt_denoiser_create(device, &dn);
    if (rc == RT_OK)
      rc = rt_denoise_var(dn, &dp, accum.data(), m2.data(), aov.data(), accum.data(), nullptr,
                          &st_dn);
    if (rc != RT_OK) std::fprintf(stderr, "rt_render --denoise-var: %d %s\n", rc, rt_last_error());
    rt_denoiser_destroy(dn);
    rt_scene_destroy(sc);
    if (rc != RT_OK) return 1;
    std::fprintf(stderr, "aov %.2f ms, variance-guided denoise (%d levels) %.3f ms\n",
                 st_aov.ms_kernel, dp.levels, st_dn.ms_kernel);
  } else {
    // the beauty render, the first-hit AOVs of the same camera, options and seed, the filter
    rt_scene* sc = nullptr;
    rt_denoiser* dn = nullptr;
    rt_denoise_params dp;
    std::vector<float> aov((size_t)cam.image_width * cam.image_height * RT_AOV_CHANNELS, 0.f);
    rt_stats st_aov, st_dn;
    rc = rt_denoise_default_params(cam.image_width, cam.image_height, cam.samples_per_pixel,
                                   cam.samples_per_pixel, &dp);
    if (rc == RT_OK && denoise_levels > 0) dp.levels = denoise_levels;
    if (rc == RT_OK) rc = rt_scene_create(&blob, device, &sc);
    if (rc == RT_OK) rc = rt_render(sc, &cam, &o, accum.data(), &st);
    if (rc == RT_OK) rc = rt_render_aov(sc, &cam, &o, aov.data(), &st_aov);
    if (rc == RT_OK) rc = rt_denoiser_create(device, &dn);
    if (rc == RT_OK) rc = rt_denoise(dn, &dp, accum.data(), aov.data(), accum.data(), &st_dn);
    if (rc != RT_OK) std::fprintf(stderr, "rt_render --denoise: %d %s\n", rc, rt_last_error());
    rt_denoiser_destroy(dn);
    rt_scene_destroy(sc);
    if (rc != RT_OK) return 1;
    std::fprintf(stderr, "aov %.2f ms, denoise (%d levels) %.3f ms\n", st_aov.ms_kernel, dp.levels,
                 st_dn.ms_kernel);
  }
  double msps = (double)st.samples / (st.ms_kernel * 1e3);
  std::fprintf(stderr, "kernel %.2f ms, %.1f Msamples/s\n", st.ms_kernel, msps);
  if (write_frame(accum, cam, device_output, autoexp, device, out) != 0) return 1;
  std::fprintf(stderr, "Done! wrote %s\n", out.c_str());
  rth_scene_free(s);
  return 0;
}
