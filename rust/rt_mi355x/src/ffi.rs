//! Mirrors of `include/rt_mi355x.h` (RT_ABI_VERSION 3): the C ABI of librtmi355x.so that
//! replaces the body of `render_par_lights` (reference src/render.rs:144-216). Field order and
//! widths match the header; tests/test_binding_mirror.py compares them with it.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

pub const RT_ABI_VERSION: c_int = 3;

// status codes (rt_mi355x.h "status codes")
pub const RT_OK: c_int = 0;
pub const RT_ERR_INVALID_ARG: c_int = -1;
pub const RT_ERR_BAD_BLOB: c_int = -2;
pub const RT_ERR_UNSUPPORTED: c_int = -3;
pub const RT_ERR_EMPTY_LIGHTS: c_int = -4;
pub const RT_ERR_HIP: c_int = -5;
pub const RT_ERR_NO_DEVICE: c_int = -6;

// scene blob (rt_mi355x.h "scene blob")
pub const RT_BLOB_MAGIC: u64 = 0x52545343;
pub const RT_BLOB_VERSION: u64 = 1;
pub const RT_BLOB_HEADER_SLOTS: usize = 16;
pub const RT_TEX_SLOTS: usize = 8;
pub const RT_MAT_SLOTS: usize = 8;
pub const RT_PERLIN_POINTS: usize = 256;

// object tags, material and texture kinds
pub const RT_OBJ_LIST: i64 = 1;
pub const RT_OBJ_BVH: i64 = 2;
pub const RT_OBJ_SPHERE: i64 = 3;
pub const RT_OBJ_QUAD: i64 = 4;
pub const RT_OBJ_TRANSLATE: i64 = 5;
pub const RT_OBJ_ROTATE_Y: i64 = 6;
pub const RT_OBJ_VOLUME: i64 = 7;
pub const RT_MAT_LAMBERTIAN: u64 = 1;
pub const RT_MAT_METAL: u64 = 2;
pub const RT_MAT_DIELECTRIC: u64 = 3;
pub const RT_MAT_DIFFUSE_LIGHT: u64 = 4;
pub const RT_MAT_ISOTROPIC: u64 = 5;
pub const RT_TEX_SOLID: i64 = 1;
pub const RT_TEX_CHECKER: i64 = 2;
pub const RT_TEX_IMAGE: i64 = 3;
pub const RT_TEX_NOISE: i64 = 4;

// render flags
pub const RT_FLAG_OVERWRITE: u32 = 0x1;
pub const RT_FLAG_COUNT_OPS: u32 = 0x2;
/// Exact reference semantics: empty lights -> error, Isotropic scattering_pdf = 0 (S1/S2).
/// S9: a path whose throughput is exactly zero in all channels and that carries no special value
/// ends with radiance 0; the reference goes on and returns NaN if a later bounce has a zero or NaN
/// pdf; RT_FLAG_SEMANTICS_REFERENCE keeps the reference's behaviour.
pub const RT_FLAG_SEMANTICS_REFERENCE: u32 = 0x4;
pub const RT_FLAG_INTERPRETER: u32 = 0x8;
pub const RT_FLAG_REFERENCE_BVH: u32 = 0x10;

pub const RT_LAYOUT_STATS: c_int = 11;
pub const RT_LDS_CHECK: c_int = 19;
pub const RT_TRACE_HISTORY: c_int = 64;

// first-hit AOV pass: floats per pixel and the channel offsets
pub const RT_AOV_CHANNELS: usize = 12;
pub const RT_AOV_HITS: usize = 0;
pub const RT_AOV_T: usize = 1;
pub const RT_AOV_NORMAL: usize = 2;
pub const RT_AOV_ALBEDO: usize = 5;
pub const RT_AOV_EMISSION: usize = 8;
pub const RT_AOV_MATID: usize = 11;

// a-trous denoiser
pub const RT_DENOISE_MAX_LEVELS: i32 = 8;
pub const RT_DENOISE_DEMODULATE: u32 = 0x1;

// device output stage
pub const RT_OUTPUT_EXPOSURE: u32 = 0x1;
pub const RT_OUTPUT_AUTO_EXPOSE: u32 = 0x2;
pub const RT_OUTPUT_RGBA: u32 = 0x4;

// temporal accumulation
pub const RT_TEMPORAL_RESET: u32 = 0x1;
pub const RT_TEMPORAL_VARIANCE_OF_MEAN: u32 = 0x2;

// ray queries
pub const RT_QUERY_OCCLUSION: u32 = 0x1;
pub const RT_QUERY_ANY_HIT: u32 = 0x2; // with RT_QUERY_OCCLUSION only

// ray renders
pub const RT_RAYS_STREAM_TIME: u32 = 0x1;
pub const RT_RAYS_MAX_SKIP: u32 = 16;

// ray generators on the device (rt_projection.kind)
pub const RT_PROJ_PINHOLE: i32 = 0;
pub const RT_PROJ_ORTHO: i32 = 1;
pub const RT_PROJ_PANORAMA: i32 = 2;
pub const RT_PROJ_FISHEYE: i32 = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_scene_blob {
    pub slots: *const u64,
    pub n_slots: u64,
    pub texels: *const u8, // RGB8 images, row-major, top row first (image::to_rgb8)
    pub n_texels: u64,
}

/// Camera's derived fields (render.rs:15-36), computed on the host in f64.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_camera {
    pub image_width: i32,
    pub image_height: i32,
    pub samples_per_pixel: i32, // nearest_square(spp), render.rs:38-41, 108
    pub sqrt_spp: i32,
    pub max_depth: i32, // < 2^24
    pub _pad0: i32,
    pub recip_sqrt_spp: f64,
    pub center: [f64; 3],
    pub pixel00_loc: [f64; 3],
    pub pixel_delta_u: [f64; 3],
    pub pixel_delta_v: [f64; 3],
    pub defocus_angle: f64,
    pub defocus_disk_u: [f64; 3],
    pub defocus_disk_v: [f64; 3],
    pub background: [f64; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_render_opts {
    pub seed: u64,      // render RNG seed
    pub row_begin: i32, // first image row of this call
    pub row_step: i32,  // 1 = contiguous band; G = cyclic tiling
    pub n_rows: i32,    // accum holds n_rows * image_width * 3 floats
    pub flags: u32,     // RT_FLAG_*
    pub sj_begin: i32,  // stratum rows [sj_begin, sj_begin + sj_count); 0 = all
    pub sj_count: i32,
    pub device: i32, // HIP device ordinal (rt_render only)
    pub _pad0: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rt_stats {
    pub ms_kernel: f64,
    pub ms_total: f64,
    pub samples: u64,
    pub ops: [u64; 32],  // rt_op_counter values (RT_FLAG_COUNT_OPS only)
    pub out_bytes: u64,  // f64 workspace bytes the path kernel stored
    pub launches: u32,   // path-kernel launches of the render
    pub _pad0: u32,
}

impl Default for rt_stats {
    fn default() -> Self {
        rt_stats { ms_kernel: 0.0, ms_total: 0.0, samples: 0, ops: [0; 32], out_bytes: 0,
                   launches: 0, _pad0: 0 }
    }
}

/// Parameters of the edge-avoiding a-trous denoiser (rt_denoise*); 48 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_denoise_params {
    pub width: i32,          // pixels per row
    pub height: i32,         // rows; full contiguous frames, top row first
    pub levels: i32,         // 1..RT_DENOISE_MAX_LEVELS; level k steps 2^k pixels
    pub flags: u32,          // RT_DENOISE_*
    pub beauty_samples: f64, // samples each beauty sum holds
    pub aov_samples: f64,    // samples each AOV sum holds
    pub sigma_color: f32,    // edge-stopping widths; <= 0 switches the term off
    pub sigma_normal: f32,
    pub sigma_depth: f32,
    pub sigma_albedo: f32,
}

/// Parameters of the variance-guided a-trous denoiser (rt_denoise_var*); 56 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_denoise_var_params {
    pub width: i32,
    pub height: i32,
    pub levels: i32,
    pub flags: u32,          // RT_DENOISE_DEMODULATE only
    pub beauty_samples: f64,
    pub aov_samples: f64,
    pub beauty_rows: i32,    // stratum rows the beauty and m2 sums hold, >= 2
    pub _pad0: i32,          // must be 0
    pub sigma_color: f32,    // in units of the pair's standard deviation; <= 0: term off
    pub sigma_normal: f32,
    pub sigma_depth: f32,
    pub sigma_albedo: f32,
}

/// Parameters of the adaptive driver (rt_render_adaptive_device); 24 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_adaptive_params {
    pub passes: i32,     // P, 1..sqrt_spp/2
    pub min_passes: i32, // 1..P: passes every tile receives
    pub threshold: f64,  // a tile continues while its error > threshold; NaN invalid
    pub floor: f64,      // finite, > 0
}

/// Parameters of the device output stage (rt_output*); 32 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_output_params {
    pub width: i32,
    pub height: i32,            // a contiguous buffer of height rows, top row first
    pub flags: u32,             // RT_OUTPUT_*
    pub _pad0: i32,             // must be 0
    pub samples_per_pixel: f64, // what the sums hold (finite, > 0)
    pub exposure: f64,          // used with RT_OUTPUT_EXPOSURE alone; finite
}

/// Parameters of the temporal accumulation (rt_temporal_*); 32 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_temporal_params {
    pub width: i32,
    pub height: i32,      // a contiguous frame of height rows, top row first
    pub flags: u32,       // RT_TEMPORAL_*
    pub beauty_rows: i32, // n of the estimator; >= 2 with RT_TEMPORAL_VARIANCE_OF_MEAN, else >= 0
    pub max_history: f32, // finite, >= 1
    pub depth_tol: f32,   // relative; <= 0 off
    pub normal_tol: f32,  // <= 0 off
    pub min_weight: f32,  // finite, in [0, 1)
}

/// A caller-supplied ray of rt_query_rays*; 80 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_ray {
    pub origin: [f64; 3],
    pub dir: [f64; 3], // not normalised: t is the ray parameter
    pub time: f64,     // Ray::time: a moving Sphere's centre
    pub tmin: f64,     // the interval handed to world.hit; tmax may be +inf
    pub tmax: f64,
    pub pixel: u32,    // the ray's random stream: rng_seed(params.seed, pixel, sample)
    pub sample: u32,
}

/// The closest hit of one ray (rt_query_rays*); 80 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_hit {
    pub t: f64,            // rec.t; the ray's own tmax on a miss; 0 for an invalid ray
    pub distance: f64,     // t * sqrt(dir . dir); 0 unless hit == 1
    pub p: [f64; 3],       // rec.p, world space; 0 unless hit == 1
    pub normal: [f64; 3],  // rec.normal after set_face_normal; 0 unless hit == 1
    pub hit: i32,          // 1 hit, 0 miss, -1 invalid ray
    pub front_face: i32,   // rec.front_face; 0 unless hit == 1
    pub material: i32,     // blob material-table index; -1 on a miss, 0 for an invalid ray
    pub prim: i32,         // place among the world's primitives; -1 on a miss, 0 for an invalid ray
}

/// Parameters of rt_query_rays*; 16 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_query_params {
    pub seed: u64,
    pub flags: u32, // RT_FLAG_REFERENCE_BVH only
    pub mode: u32,  // 0, RT_QUERY_OCCLUSION or RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT
}

/// Parameters of rt_render_rays*; 56 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_rays_params {
    pub seed: u64,
    pub flags: u32,       // RT_FLAG_OVERWRITE | INTERPRETER | REFERENCE_BVH | SEMANTICS_REFERENCE
    pub mode: u32,        // RT_RAYS_*
    pub sqrt_paths: i32,  // S >= 1: S*S paths per ray
    pub max_depth: i32,   // 0 .. 0xffffff
    pub stream_skip: u32, // generator steps discarded before a path starts, 0..RT_RAYS_MAX_SKIP
    pub _pad0: u32,       // must be 0
    pub background: [f64; 3],
}

/// A projection of rt_projection_rays_device; 96 bytes, the layout of rth_projection.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_projection {
    pub kind: i32, // RT_PROJ_*
    pub width: i32,
    pub height: i32,
    pub sqrt_spp: i32,
    pub origin: [f64; 3],
    pub forward: [f64; 3],
    pub up: [f64; 3],
    pub fov: f64,
}

/// Parameters of rt_ao_rays_device; 32 bytes, the layout of rth_ao_params.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_ao_params {
    pub seed: u64,
    pub radius: f64,    // becomes tmax; > tmin, may be +inf
    pub tmin: f64,      // finite, >= 0
    pub dir_index: u32, // k: which of the K directions this batch is
    pub _pad0: u32,     // must be 0
}

/// Parameters of rt_ambient_occlusion_device; 40 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rt_ao_frame_params {
    pub seed: u64,
    pub radius: f64,
    pub tmin: f64,
    pub directions: u32, // K >= 1
    pub flags: u32,      // RT_FLAG_OVERWRITE | RT_FLAG_REFERENCE_BVH only
    pub channels: u32,   // 1 or 3
    pub chunk_rays: u32, // 0 = default (2^22); else rays per internal chunk
}

/// Opaque handles (rt_scene, rt_multi, rt_denoiser, rt_adaptive, rt_output_stage, rt_temporal,
/// rt_raygen).
#[repr(C)]
pub struct rt_scene {
    _private: [u8; 0],
}
#[repr(C)]
pub struct rt_multi {
    _private: [u8; 0],
}
#[repr(C)]
pub struct rt_denoiser {
    _private: [u8; 0],
}
#[repr(C)]
pub struct rt_adaptive {
    _private: [u8; 0],
}
#[repr(C)]
pub struct rt_output_stage {
    _private: [u8; 0],
}
#[repr(C)]
pub struct rt_temporal {
    _private: [u8; 0],
}
#[repr(C)]
pub struct rt_raygen {
    _private: [u8; 0],
}

#[link(name = "rtmi355x")]
extern "C" {
    pub fn rt_abi_version() -> c_int;
    pub fn rt_last_error() -> *const c_char;
    pub fn rt_device_count(count: *mut c_int) -> c_int;
    pub fn rt_scene_validate(blob: *const rt_scene_blob) -> c_int;
    pub fn rt_scene_layout_stats(blob: *const rt_scene_blob, out: *mut u32, n: c_int) -> c_int;
    pub fn rt_scene_lds_check(blob: *const rt_scene_blob, flags: u32, n_rays: u32, seed: u64,
                              out: *mut u64, n: c_int, msg: *mut c_char, msg_len: u32) -> c_int;
    pub fn rt_scene_create(blob: *const rt_scene_blob, device: c_int, out: *mut *mut rt_scene)
        -> c_int;
    pub fn rt_scene_destroy(scene: *mut rt_scene);
    pub fn rt_scene_device_bytes(scene: *const rt_scene) -> u64;
    pub fn rt_scene_jit_info(scene: *mut rt_scene, state: *mut c_int, msg: *mut c_char,
                             msg_len: u32) -> c_int;
    pub fn rt_jit_check(blob: *const rt_scene_blob, arch: *const c_char, state: *mut c_int,
                        msg: *mut c_char, msg_len: u32) -> c_int;
    pub fn rt_render(scene: *mut rt_scene, cam: *const rt_camera, opts: *const rt_render_opts,
                     accum_rgb: *mut f32, stats: *mut rt_stats) -> c_int;
    pub fn rt_render_device(scene: *mut rt_scene, cam: *const rt_camera,
                            opts: *const rt_render_opts, accum_rgb_device: *mut f32,
                            hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_scene_trace_ms(scene: *mut rt_scene, ms_out: *mut f32, max_n: c_int,
                             n_out: *mut c_int) -> c_int;
    pub fn rt_scene_prof_counters(scene: *mut rt_scene, out: *mut u64, n: c_int) -> c_int;
    pub fn rt_render_multi(blob: *const rt_scene_blob, cam: *const rt_camera,
                           opts: *const rt_render_opts, devices: *const c_int, n_devices: c_int,
                           accum_rgb: *mut f32, stats: *mut rt_stats) -> c_int;
    pub fn rt_multi_create(blob: *const rt_scene_blob, devices: *const c_int, n_devices: c_int,
                           out: *mut *mut rt_multi) -> c_int;
    pub fn rt_multi_render(multi: *mut rt_multi, cam: *const rt_camera,
                           opts: *const rt_render_opts, accum_rgb_device0: *mut f32,
                           hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_multi_info(multi: *mut rt_multi, out: *mut u64, n: c_int) -> c_int;
    pub fn rt_multi_destroy(multi: *mut rt_multi);
    pub fn rt_render_blob(blob: *const rt_scene_blob, cam: *const rt_camera,
                          opts: *const rt_render_opts, accum_rgb: *mut f32,
                          stats: *mut rt_stats) -> c_int;
    pub fn rt_render_aov(scene: *mut rt_scene, cam: *const rt_camera,
                         opts: *const rt_render_opts, aov_host: *mut f32,
                         stats: *mut rt_stats) -> c_int;
    pub fn rt_render_aov_device(scene: *mut rt_scene, cam: *const rt_camera,
                                opts: *const rt_render_opts, aov_device: *mut f32,
                                hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_denoise_default_params(width: c_int, height: c_int, beauty_samples: f64,
                                     aov_samples: f64, out: *mut rt_denoise_params) -> c_int;
    pub fn rt_denoiser_create(device: c_int, out: *mut *mut rt_denoiser) -> c_int;
    pub fn rt_denoiser_destroy(dn: *mut rt_denoiser);
    pub fn rt_denoise_device(dn: *mut rt_denoiser, p: *const rt_denoise_params,
                             beauty_dev: *const f32, aov_dev: *const f32, out_dev: *mut f32,
                             hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_denoise(dn: *mut rt_denoiser, p: *const rt_denoise_params, beauty: *const f32,
                      aov: *const f32, out: *mut f32, stats: *mut rt_stats) -> c_int;
    pub fn rt_render_moments_device(scene: *mut rt_scene, cam: *const rt_camera,
                                    opts: *const rt_render_opts, accum_rgb_device: *mut f32,
                                    m2_rgb_device: *mut f32, hip_stream: *mut c_void,
                                    stats: *mut rt_stats) -> c_int;
    pub fn rt_render_moments(scene: *mut rt_scene, cam: *const rt_camera,
                             opts: *const rt_render_opts, accum_rgb: *mut f32, m2_rgb: *mut f32,
                             stats: *mut rt_stats) -> c_int;
    pub fn rt_denoise_var_default_params(width: c_int, height: c_int, beauty_samples: f64,
                                         beauty_rows: c_int, aov_samples: f64,
                                         out: *mut rt_denoise_var_params) -> c_int;
    pub fn rt_denoise_var_device(dn: *mut rt_denoiser, p: *const rt_denoise_var_params,
                                 beauty_dev: *const f32, m2_dev: *const f32,
                                 aov_dev: *const f32, out_dev: *mut f32, var_out_dev: *mut f32,
                                 hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_denoise_var(dn: *mut rt_denoiser, p: *const rt_denoise_var_params,
                          beauty: *const f32, m2: *const f32, aov: *const f32, out: *mut f32,
                          var_out: *mut f32, stats: *mut rt_stats) -> c_int;
    pub fn rt_render_tiles_device(scene: *mut rt_scene, cam: *const rt_camera,
                                  opts: *const rt_render_opts, tiles: *const u32, n_list: u32,
                                  sj_step: i32, accum_rgb_device: *mut f32,
                                  m2_rgb_device: *mut f32, hip_stream: *mut c_void,
                                  stats: *mut rt_stats) -> c_int;
    pub fn rt_adaptive_schedule(sqrt_spp: c_int, passes: c_int, pass: c_int,
                                sj_begin: *mut c_int, sj_step: *mut c_int,
                                sj_count: *mut c_int) -> c_int;
    pub fn rt_adaptive_create(device: c_int, out: *mut *mut rt_adaptive) -> c_int;
    pub fn rt_adaptive_destroy(ad: *mut rt_adaptive);
    pub fn rt_adaptive_tile_error(ad: *mut rt_adaptive, width: c_int, height: c_int,
                                  sqrt_spp: c_int, floor: f64, accum_dev: *const f32,
                                  m2_dev: *const f32, rows_held: *const u32, err_out: *mut f32,
                                  n_invalid_out: *mut u64, hip_stream: *mut c_void) -> c_int;
    pub fn rt_adaptive_resolve_device(ad: *mut rt_adaptive, width: c_int, height: c_int,
                                      sqrt_spp: c_int, rows_held: *const u32,
                                      accum_dev: *const f32, out_dev: *mut f32,
                                      samples_dev: *mut f32, hip_stream: *mut c_void) -> c_int;
    pub fn rt_render_adaptive_device(ad: *mut rt_adaptive, scene: *mut rt_scene,
                                     cam: *const rt_camera, opts: *const rt_render_opts,
                                     params: *const rt_adaptive_params,
                                     accum_rgb_device: *mut f32, m2_rgb_device: *mut f32,
                                     out_dev: *mut f32, samples_dev: *mut f32,
                                     rows_held_out: *mut u32, tiles_per_pass: *mut u32,
                                     hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_render_adaptive(ad: *mut rt_adaptive, scene: *mut rt_scene, cam: *const rt_camera,
                              opts: *const rt_render_opts, params: *const rt_adaptive_params,
                              accum_rgb: *mut f32, m2_rgb: *mut f32, out: *mut f32,
                              samples: *mut f32, rows_held_out: *mut u32,
                              tiles_per_pass: *mut u32, stats: *mut rt_stats) -> c_int;
    pub fn rt_output_create(device: c_int, out: *mut *mut rt_output_stage) -> c_int;
    pub fn rt_output_destroy(o: *mut rt_output_stage);
    pub fn rt_output_device(o: *mut rt_output_stage, p: *const rt_output_params, sums_dev: *const f32,
                            rgb8_dev: *mut u8, exposure_out: *mut f64, hip_stream: *mut c_void,
                            stats: *mut rt_stats) -> c_int;
    pub fn rt_output(o: *mut rt_output_stage, p: *const rt_output_params, sums: *const f32,
                     rgb8: *mut u8, exposure_out: *mut f64, stats: *mut rt_stats) -> c_int;
    pub fn rt_temporal_default_params(width: c_int, height: c_int,
                                      out: *mut rt_temporal_params) -> c_int;
    pub fn rt_temporal_create(device: c_int, out: *mut *mut rt_temporal) -> c_int;
    pub fn rt_temporal_destroy(t: *mut rt_temporal);
    pub fn rt_temporal_info(t: *mut rt_temporal, out: *mut u64, n: c_int) -> c_int;
    pub fn rt_temporal_accumulate_device(t: *mut rt_temporal, p: *const rt_temporal_params,
                                         cam: *const rt_camera, beauty_dev: *const f32,
                                         m2_dev: *const f32, aov_dev: *const f32,
                                         out_beauty_dev: *mut f32, out_m2_dev: *mut f32,
                                         hist_len_dev: *mut f32, hip_stream: *mut c_void,
                                         stats: *mut rt_stats) -> c_int;
    pub fn rt_temporal_accumulate(t: *mut rt_temporal, p: *const rt_temporal_params,
                                  cam: *const rt_camera, beauty: *const f32, m2: *const f32,
                                  aov: *const f32, out_beauty: *mut f32, out_m2: *mut f32,
                                  hist_len: *mut f32, stats: *mut rt_stats) -> c_int;
    pub fn rt_query_rays_device(scene: *mut rt_scene, params: *const rt_query_params,
                                rays_dev: *const rt_ray, n_rays: u64, out_dev: *mut c_void,
                                hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_query_rays(scene: *mut rt_scene, params: *const rt_query_params,
                         rays: *const rt_ray, n_rays: u64, out: *mut c_void,
                         stats: *mut rt_stats) -> c_int;
    pub fn rt_scene_prim_map(blob: *const rt_scene_blob, node_word: *mut u32, prim: *mut u32,
                             cap: u32, n_out: *mut u32) -> c_int;
    pub fn rt_render_rays_device(scene: *mut rt_scene, params: *const rt_rays_params,
                                 rays_dev: *const rt_ray, n_rays: u64, rgb_dev: *mut f32,
                                 hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_render_rays(scene: *mut rt_scene, params: *const rt_rays_params,
                          rays: *const rt_ray, n_rays: u64, rgb: *mut f32,
                          stats: *mut rt_stats) -> c_int;
    pub fn rt_raygen_create(device: c_int, out: *mut *mut rt_raygen) -> c_int;
    pub fn rt_raygen_destroy(g: *mut rt_raygen);
    pub fn rt_projection_rays_device(g: *mut rt_raygen, proj: *const rt_projection,
                                     cam: *const rt_camera, seed: u64, s_i: i32, s_j: i32,
                                     row_begin: i32, n_rows: i32, rays_dev: *mut rt_ray,
                                     hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
    pub fn rt_ao_rays_device(g: *mut rt_raygen, p: *const rt_ao_params,
                             primary_dev: *const rt_ray, hits_dev: *const rt_hit, n: u64,
                             out_dev: *mut rt_ray, hip_stream: *mut c_void,
                             stats: *mut rt_stats) -> c_int;
    pub fn rt_ao_accumulate_device(g: *mut rt_raygen, occ_dev: *const u8, n: u64, channels: u32,
                                   flags: u32, sums_dev: *mut f32, hip_stream: *mut c_void,
                                   stats: *mut rt_stats) -> c_int;
    pub fn rt_ambient_occlusion_device(g: *mut rt_raygen, scene: *mut rt_scene,
                                       p: *const rt_ao_frame_params, primary_dev: *const rt_ray,
                                       n: u64, sums_dev: *mut f32, hits_out_dev: *mut rt_hit,
                                       hip_stream: *mut c_void, stats: *mut rt_stats) -> c_int;
}
