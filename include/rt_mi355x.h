/*
 * rt_mi355x.h — C ABI of the MI355X (gfx950) path-tracing library `librtmi355x.so`.
 *
 * This is the drop-in boundary for the reference's per-pixel render loop:
 *
 *   reference (Rust, no FFI exists upstream)           this ABI
 *   -----------------------------------------------    ------------------------------------------
 *   render_par_lights(cam, world, pixels, suns, lights) rt_render / rt_render_device
 *       /root/reference/src/render.rs:144-216               (scene blob + camera + opts -> accum)
 *   render_par(cam, world, pixels, suns)                rt_render with blob.lights_off == -1
 *       /root/reference/src/render.rs:140-142               (empty light list, see RT_FLAG_SEMANTICS_REFERENCE)
 *   Camera::new derived fields                          rt_camera (filled host-side, render.rs:62-133)
 *       /root/reference/src/render.rs:15-36
 *   HittableList / Object tree (world, lights)          rt_scene_blob (prefix-serialised tree,
 *       /root/reference/src/hittable.rs:55-130,             f64 slots, see "Scene blob" below)
 *       object.rs:17-71, transform.rs, constant_medium.rs
 *   pixels: &mut Vec<Color> (raw sums, pre-zeroed)      float* accum_rgb (raw sums over spp,
 *       /root/reference/src/render.rs:136-138, 189          added into unless RT_FLAG_OVERWRITE)
 *   panics (expect / panic!)                            int status < 0 + rt_last_error()
 *
 * accum holds raw per-pixel sums exactly like the reference's `pixels` vector; auto_expose and
 * write_color (color.rs:8-33) are rt_output* at the end of this file; the PPM writer stays host-side.
 *
 * Every entry point is plain C: pointers, sizes, PODs. No torch, no C++ types.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------------------------ */
#define RT_OK 0
#define RT_ERR_INVALID_ARG (-1)
#define RT_ERR_BAD_BLOB (-2)      /* malformed scene blob                                   */
#define RT_ERR_UNSUPPORTED (-3)   /* valid reference scene the device path cannot express    */
#define RT_ERR_EMPTY_LIGHTS (-4)  /* reference semantics: empty light list panics            */
                                  /* (hittable.rs:115-129 via render.rs:140-142)            */
#define RT_ERR_HIP (-5)           /* HIP runtime failure (message in rt_last_error)         */
#define RT_ERR_NO_DEVICE (-6)

/* ---- scene blob ---------------------------------------------------------------------------
 * A flat array of 64-bit slots. A slot holds an int64 or the bit pattern of an IEEE f64.
 * The host computes every derived quantity in f64 exactly as the reference constructors do
 * (Quad::new object.rs:427-446, Sphere::new 83-105, RotateY::new transform.rs:143-186, ...);
 * consumers round to their working precision.
 *
 * Header (slot index: meaning)
 *   0 magic RT_BLOB_MAGIC      1 version RT_BLOB_VERSION    2 n_slots
 *   3 n_textures  4 textures_off   (RT_TEX_SLOTS slots each)
 *   5 n_materials 6 materials_off  (RT_MAT_SLOTS slots each)
 *   7 n_perlin    8 perlin_off     (RT_PERLIN_SLOTS each: ranvec 256x3 f64, perm_x/y/z 3x256 int)
 *   9 world_off                    (object tree: the world HittableList)
 *  10 lights_off                   (object tree, or -1 = empty light list, as render_par)
 *  11 n_texel_bytes                (size of blob.texels; images index into it)
 *
 * Object tree: prefix order, records by tag (slot counts include the tag):
 *   RT_OBJ_LIST      [tag, n, bbox6]                       then n children      (hittable.rs:55-130)
 *   RT_OBJ_BVH       [tag, bbox6]                          then left, right     (hittable.rs:135-241)
 *   RT_OBJ_SPHERE    [tag, mat, moving, c3, radius, cvec3, bbox6]               (object.rs:73-213)
 *   RT_OBJ_QUAD      [tag, mat, q3, u3, v3, normal3, w3, d, area, bbox6]        (object.rs:414-507)
 *   RT_OBJ_TRANSLATE [tag, offset3, bbox6]                 then child           (transform.rs:19-74)
 *   RT_OBJ_ROTATE_Y  [tag, sin, cos, bbox6]                then child           (transform.rs:76-186)
 *   RT_OBJ_VOLUME    [tag, mat, neg_inv_density, bbox6]    then boundary        (constant_medium.rs)
 *   bbox6 = xmin xmax ymin ymax zmin zmax.
 * Material record [kind, p0..p6]:
 *   LAMBERTIAN [1, tex]   METAL [2, r, g, b, fuzz]   DIELECTRIC [3, ir, r, g, b]
 *   DIFFUSE_LIGHT [4, tex]   ISOTROPIC [5, tex]                                 (material.rs:25-248)
 * Texture record [kind, p0..p6]:
 *   SOLID [1, r, g, b]   CHECKER [2, inv_scale, even_tex, odd_tex]
 *   IMAGE [3, width, height, texel_byte_offset]  (width or height 0 = image absent -> (0,1,1))
 *   NOISE [4, scale, perlin_index]                                              (texture.rs:10-131)
 * ------------------------------------------------------------------------------------------ */
#define RT_BLOB_MAGIC 0x52545343 /* 'RTSC' */
#define RT_BLOB_VERSION 1
#define RT_BLOB_HEADER_SLOTS 16
#define RT_TEX_SLOTS 8
#define RT_MAT_SLOTS 8
#define RT_PERLIN_POINTS 256
#define RT_PERLIN_SLOTS (RT_PERLIN_POINTS * 3 + RT_PERLIN_POINTS * 3)

enum rt_obj_tag {
  RT_OBJ_LIST = 1,
  RT_OBJ_BVH = 2,
  RT_OBJ_SPHERE = 3,
  RT_OBJ_QUAD = 4,
  RT_OBJ_TRANSLATE = 5,
  RT_OBJ_ROTATE_Y = 6,
  RT_OBJ_VOLUME = 7
};
enum rt_mat_kind {
  RT_MAT_LAMBERTIAN = 1,
  RT_MAT_METAL = 2,
  RT_MAT_DIELECTRIC = 3,
  RT_MAT_DIFFUSE_LIGHT = 4,
  RT_MAT_ISOTROPIC = 5
};
enum rt_tex_kind { RT_TEX_SOLID = 1, RT_TEX_CHECKER = 2, RT_TEX_IMAGE = 3, RT_TEX_NOISE = 4 };

typedef struct rt_scene_blob {
  const uint64_t* slots;
  uint64_t n_slots;
  const uint8_t* texels; /* RGB8 images, row-major, top row first (as image::to_rgb8) */
  uint64_t n_texels;
} rt_scene_blob;

/* ---- camera: Camera's derived fields (render.rs:15-36), computed on the host in f64 ---------- */
typedef struct rt_camera {
  int32_t image_width;
  int32_t image_height;
  int32_t samples_per_pixel; /* effective spp = nearest_square(spp) (render.rs:38-41, 108) */
  int32_t sqrt_spp;
  int32_t max_depth;
  int32_t _pad0;
  double recip_sqrt_spp;
  double center[3];
  double pixel00_loc[3];
  double pixel_delta_u[3];
  double pixel_delta_v[3];
  double defocus_angle;
  double defocus_disk_u[3];
  double defocus_disk_v[3];
  double background[3];
} rt_camera;

/* ---- render options ---------------------------------------------------------------------- */
#define RT_FLAG_OVERWRITE 0x1u             /* accum = sums instead of accum += sums          */
#define RT_FLAG_COUNT_OPS 0x2u             /* run the op-counting build, fill rt_stats.ops   */
#define RT_FLAG_SEMANTICS_REFERENCE 0x4u   /* exact reference semantics: empty lights -> error, */
                                           /* Isotropic scattering_pdf = 0. */
/* S9: a path whose throughput is exactly zero in all channels and that carries no special value
 * ends with radiance 0; the reference goes on and returns NaN if a later bounce has a zero or NaN
 * pdf; RT_FLAG_SEMANTICS_REFERENCE keeps the reference's behaviour. */
#define RT_FLAG_INTERPRETER 0x8u           /* product render with the interpreter walker, not the */
                                           /* scene-specialised kernel (same image, bit for bit)  */
#define RT_FLAG_REFERENCE_BVH 0x10u        /* product render walks BVH subtrees in the reference's */
                                           /* own tree and order, not their ordered BVHs (same    */
                                           /* image, bit for bit)                                 */

typedef struct rt_render_opts {
  uint64_t seed;      /* render RNG seed                                   */
  int32_t row_begin;  /* first image row of this call                                          */
  int32_t row_step;   /* 1 = contiguous band; G = cyclic tiling (rows row_begin + k*G)         */
  int32_t n_rows;     /* rows rendered; accum holds n_rows * image_width * 3 floats            */
  uint32_t flags;     /* RT_FLAG_*                                                             */
  int32_t sj_begin;   /* stratum rows [sj_begin, sj_begin+sj_count) of the sqrt_spp x sqrt_spp */
  int32_t sj_count;   /* grid (render.rs:185); 0 = all. A subset keeps the full-spp jitter.   */
  int32_t device;     /* HIP device ordinal (rt_render only)                                   */
  int32_t _pad0;
} rt_render_opts;

/* Deterministic op counters (RT_FLAG_COUNT_OPS). Identical paths => identical counts on the
 * CPU oracle and the GPU, so per-sample work is measured, not assumed. */
enum rt_op_counter {
  RT_OP_SAMPLES = 0,      /* camera paths started                                     */
  RT_OP_WORLD_QUERIES,    /* world.hit calls (render.rs:264)                          */
  RT_OP_QUAD_TESTS,       /* Quad::hit entered (object.rs:453)                        */
  RT_OP_QUAD_PLANE,       /* ... passed the |n.d| >= 1e-8 test                        */
  RT_OP_QUAD_INTERVAL,    /* ... t inside the interval: planar coords computed        */
  RT_OP_QUAD_HITS,        /* ... accepted                                             */
  RT_OP_SPHERE_TESTS,     /* Sphere::hit entered (object.rs:145)                      */
  RT_OP_SPHERE_ROOTS,     /* ... discriminant >= 0                                    */
  RT_OP_SPHERE_HITS,      /* ... accepted                                             */
  RT_OP_AABB_TESTS,       /* Aabb::hit (object.rs:340) from BvhNode::hit              */
  RT_OP_TRANSLATE,        /* Translate::hit entered                                   */
  RT_OP_ROTATE_Y,         /* RotateY::hit entered                                     */
  RT_OP_VOLUME_TESTS,     /* ConstantMedium::hit entered                              */
  RT_OP_VOLUME_DRAWS,     /* ... free-flight distance drawn                           */
  RT_OP_MISSES,           /* world miss -> background                                 */
  RT_OP_EMISSIVE_HITS,    /* DiffuseLight hit (path ends)                             */
  RT_OP_LAMBERTIAN,       /* Lambertian scatter + mixture PDF                         */
  RT_OP_METAL,
  RT_OP_DIELECTRIC,
  RT_OP_ISOTROPIC,
  RT_OP_LIGHT_PDF_QUAD,   /* Quad::pdf_value (object.rs:492)                          */
  RT_OP_LIGHT_PDF_SPHERE, /* Sphere::pdf_value (object.rs:190)                        */
  RT_OP_LIGHT_GEN,        /* light-PDF generate (pdf.rs:120-126, first branch)        */
  RT_OP_COSINE_GEN,       /* material-PDF generate                                    */
  RT_OP_NOISE_EVALS,      /* NoiseTexture::value (texture.rs:127-130)                 */
  RT_OP_DEPTH_CUTOFF,     /* path ended by max_depth                                  */
  RT_OP_COUNT
};

typedef struct rt_stats {
  double ms_kernel;  /* device time of the render kernels (HIP events)             */
  double ms_total;   /* host wall time of the call                                  */
  uint64_t samples;  /* pixel-samples rendered by this call                         */
  uint64_t ops[32];  /* rt_op_counter values (RT_FLAG_COUNT_OPS only)               */
  uint64_t out_bytes; /* f64 workspace bytes the path kernel stored (row totals, block   */
                      /* partials, tail samples) and rt_reduce read back: a design choice, */
                      /* not the path's algorithmic bytes (the W*H*12 B f32 framebuffer)   */
  uint32_t launches;  /* path-kernel launches (stratum-row chunks) of the render        */
  uint32_t _pad0;
} rt_stats;

typedef struct rt_scene rt_scene; /* opaque: device-resident flattened scene + workspace */

int rt_abi_version(void);
const char* rt_last_error(void);
int rt_device_count(int* count);

/* Validate a blob without touching a device (hittable/object invariants, tag and index ranges). */
int rt_scene_validate(const rt_scene_blob* blob);

/* Host-only diagnostics of the flattened layout (no device needed): out[0..8] = node words,
 * BVH-region words, BVH records, DUP records (span-1 leaves tested once), ConstantMedium
 * records, of which one-walk sphere / one-walk quad boundaries, light records, and BVH
 * subtrees walked through an ordered BVH by the product kernels, of those the ones with a compact
 * copy for the walk from LDS, and the bytes of that compact region. */
#define RT_LAYOUT_STATS 11
int rt_scene_layout_stats(const rt_scene_blob* blob, uint32_t* out, int n);

/* Host-only check of a product render's LDS plan and of the compact BVHs its walk reads from LDS
 * (no device needed): out[0..18] = workgroup size, static LDS bound, staged table
 * bytes, compact-tree LDS offset (0xffffffff: not in LDS), compact-tree bytes, stack LDS offset,
 * stack bytes per lane (header cbvh_stack), dynamic LDS, static + dynamic, the CU's LDS, compact
 * trees, deepest tree (internal nodes, root = 1), structural errors, largest stack slot the
 * walk stores to, largest number of pending entries, rays walked, box steps, one past the
 * largest compact-region byte read, the row totals' LDS offset (0xffffffff: the launch renders
 * no row items). The walks are a host restatement of the LDS walk over
 * n_rays random rays per tree without closest-hit culling (the worst case for the stack).
 * msg (may be NULL) receives the first structural error. `flags`: the render's RT_FLAG_*. */
#define RT_LDS_CHECK 19
int rt_scene_lds_check(const rt_scene_blob* blob, uint32_t flags, uint32_t n_rays, uint64_t seed,
                       uint64_t* out, int n, char* msg, uint32_t msg_len);

/* Validate, flatten (threaded node array, f64 payloads; rt_layout.h) and upload to `device`. */
int rt_scene_create(const rt_scene_blob* blob, int device, rt_scene** out);
void rt_scene_destroy(rt_scene* scene);
/* Bytes of the device-side flattened scene (nodes + materials + textures + tables). */
uint64_t rt_scene_device_bytes(const rt_scene* scene);
/* Scene-specialised product kernel (the world walker generated from the scene and compiled by
 * hiprtc on the first product render; a BVH subtree record calls the per-lane BVH walk from the
 * generated walker, so BVH scenes such as final_scene run it too).
 * *state: 1 compiled and in use, 0 not compiled yet, -1 not generated for this scene (or
 * RT_JIT=0), -2 compilation failed (the interpreter kernel runs). msg: the reason or the log. */
int rt_scene_jit_info(rt_scene* scene, int* state, char* msg, uint32_t msg_len);
/* Host-only check of the scene-specialised kernel (no device needed): generate the walker for
 * `blob` and compile it with hiprtc for `arch` (e.g. "gfx950"). RT_OK with *state = 1 (compiled;
 * msg receives the generated walker source) or -1 (not generated; msg says why); a negative
 * status when compilation fails (msg receives the log). */
int rt_jit_check(const rt_scene_blob* blob, const char* arch, int* state, char* msg,
                 uint32_t msg_len);

/* Re-entrancy (render_par_lights takes &HittableList and may run concurrently, render.rs:144-150):
 * renders of ONE scene may be issued from several host threads and on several streams at once,
 * each into its own output buffer. Every render call takes a private slot of per-render state
 * (pool-queue word, op counters, f64 workspace, events): a slot whose previous render has
 * finished or went to the same stream handle, else a new one (up to 8 per scene; beyond that a
 * call waits for a slot to finish); the call's stream always waits for the slot's previous
 * render (an event wait: equal handles such as hipStreamPerThread are different streams in
 * different threads), and a call that fails after enqueuing work still marks the slot busy
 * until that work ends. Renders on different streams therefore run concurrently and each
 * gives its serial image bit for bit. Two renders into the SAME output buffer are ordered only by
 * the caller (same stream, or events). rt_scene_destroy must not race with renders of the scene. */

/* Synchronous: render into a HOST buffer (n_rows * W * 3 floats). */
int rt_render(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts, float* accum_rgb,
              rt_stats* stats);

/* Asynchronous on `hip_stream` (hipStream_t, may be NULL): render into a DEVICE buffer.
 * If stats != NULL the call synchronises the stream to fill it. Limits: image_width <= 65535
 * and samples_per_pixel < 2^30 (sqrt_spp <= 32768; RT_ERR_UNSUPPORTED beyond); any number of
 * rows (row ranges taller than 32760 rows run as consecutive sub-renders, same image).
 * rt_scene_destroy waits for the scene's renders. */
int rt_render_device(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                     float* accum_rgb_device, void* hip_stream, rt_stats* stats);

/* Device time (ms) of the path-tracing kernel alone (rt_trace, every chunk of one render summed;
 * HIP events recorded on the render stream around its launches) for the most recent renders
 * of `scene`, oldest first: up to max_n values, *n_out = count. Waits for those events. Used by
 * the benchmark's roofline so the figure excludes the per-pixel reduction. */
#define RT_TRACE_HISTORY 64
int rt_scene_trace_ms(rt_scene* scene, float* ms_out, int max_n, int* n_out);

/* Diagnostics: counters of a profiling build of the library (-DRT_PROF, tools_gpu/) from the
 * scene's latest render; zeros in the product build. */
int rt_scene_prof_counters(rt_scene* scene, uint64_t* out, int n);

/* Multi-GPU in ONE host process (no RCCL needed): the call's rows are dealt cyclically over
 * devices[0..n_devices) (row r of the call -> device r mod n), every device renders
 * its rows concurrently on its own stream, and the host buffer accum_rgb (opts->n_rows * W * 3)
 * receives the de-interleaved frame. Bit for bit the image of rt_render on one device (the RNG
 * is keyed by global pixel and sample). A device may be listed more than once. stats: samples,
 * ms_total (= ms_kernel: host wall time), launches = n_devices. render_par_lights over N GPUs
 * (render.rs:144-216). One process per GPU instead: rt_render_device on cyclic rows + an RCCL
 * gather. */
int rt_render_multi(const rt_scene_blob* blob, const rt_camera* cam, const rt_render_opts* opts,
                    const int* devices, int n_devices, float* accum_rgb, rt_stats* stats);

/* Persistent multi-GPU handle (one host process driving N GPUs, frame after frame; the same
 * role as render_par_lights rendering one frame per call over every core, render.rs:144-216).
 * rt_multi_create uploads the scene to each listed device ONCE (a device may be listed more than
 * once); every device keeps its scene, workspace, stream, row buffer and compiled kernel across
 * calls. rt_multi_render: the call's rows are dealt cyclically (row r of the call -> devices[r mod
 * n]), every device renders its rows on its own stream, the rows are copied peer to peer
 * (hipMemcpyPeerAsync, xGMI) into a staging buffer on devices[0], and a kernel there
 * de-interleaves them into accum_rgb_device0 (a devices[0] buffer of opts->n_rows * W * 3
 * floats; overwritten or added to as opts->flags says). Asynchronous on hip_stream (a devices[0]
 * stream, may be NULL); stats != NULL synchronises it. Bit for bit the image of rt_render_device
 * on one device, for any number of rows (the de-interleave kernel loops over the rows beyond a
 * grid's 65535 blocks in y, and every device splits its share as rt_render_device does).
 * Consecutive frames of one handle are ordered on devices[0] (a frame waits for the previous
 * frame's gather, whatever stream each was issued on); calls from several host threads are
 * serialised. rt_multi_info: out[0..3] = frames rendered, scene uploads, staging-buffer
 * allocations, devices. */
typedef struct rt_multi rt_multi;
int rt_multi_create(const rt_scene_blob* blob, const int* devices, int n_devices, rt_multi** out);
int rt_multi_render(rt_multi* multi, const rt_camera* cam, const rt_render_opts* opts,
                    float* accum_rgb_device0, void* hip_stream, rt_stats* stats);
int rt_multi_info(rt_multi* multi, uint64_t* out, int n);
void rt_multi_destroy(rt_multi* multi);

/* One-shot drop-in for render_par_lights: create + render + destroy. */
int rt_render_blob(const rt_scene_blob* blob, const rt_camera* cam, const rt_render_opts* opts,
                   float* accum_rgb, rt_stats* stats);

/* ---- first-hit AOV pass --------------------------------------------------------------------
 * The guides a denoiser or compositor wants next to the beauty sums, and a flip-free view of
 * primary visibility: every pixel-sample of the call (same rows, strata, seed and therefore the
 * same RNG stream as rt_render_device) forms its camera ray as the beauty pass does (jitter,
 * defocus disk, time), runs ONE world query over [1e-4, inf) with the sample's own generator and
 * writes what it found. cam->max_depth is ignored. Output: n_rows * W * RT_AOV_CHANNELS floats,
 * pixel-interleaved. Channels 0-10 are sums over the call's samples (f64 per pixel in the
 * reference's sample order, rounded once to f32):
 *   RT_AOV_HITS      1 per hit (coverage = hits / spp)
 *   RT_AOV_T         rec.t: the RAY PARAMETER of the reference's unnormalised camera ray
 *                    (direction = pixel sample - origin), not a Euclidean distance; 0 on a miss
 *   RT_AOV_NORMAL    rec.normal after set_face_normal, world space (3); a ConstantMedium hit has
 *                    (1,0,0) (constant_medium.rs:82-90); 0 on a miss
 *   RT_AOV_ALBEDO    the attenuation the first bounce would multiply by (3): tex.value(u,v,p) for
 *                    Lambertian and Isotropic, Metal's albedo, Dielectric's tint, 0 for
 *                    DiffuseLight; 0 on a miss
 *   RT_AOV_EMISSION  ray_color at depth 1 (3): DiffuseLight's tex.value(u,v,p) when front_face,
 *                    0 for every other hit, cam->background on a miss
 *   RT_AOV_MATID     NOT a sum: the blob material-table index hit by the call's first sample
 *                    (first stratum row of the call, s_i = 0), -1 on a miss; always overwritten
 * Without RT_FLAG_OVERWRITE channels 0-10 are added into the buffer, (float)((double)a + sum).
 * RT_FLAG_REFERENCE_BVH is honoured; RT_FLAG_INTERPRETER and RT_FLAG_SEMANTICS_REFERENCE are
 * accepted (neither changes a first hit); RT_FLAG_COUNT_OPS is RT_ERR_INVALID_ARG. Limits, status
 * codes, the split of tall row ranges, re-entrancy and lifetime are those of rt_render_device; a
 * call with n_rows == 0 returns RT_OK and touches nothing. rt_stats: ms_kernel, ms_total, samples;
 * launches = AOV kernel launches; out_bytes = bytes written; ops all zero. */
#define RT_AOV_CHANNELS 12
#define RT_AOV_HITS 0
#define RT_AOV_T 1
#define RT_AOV_NORMAL 2
#define RT_AOV_ALBEDO 5
#define RT_AOV_EMISSION 8
#define RT_AOV_MATID 11

/* Synchronous: AOVs into a HOST buffer (n_rows * W * RT_AOV_CHANNELS floats). */
int rt_render_aov(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                  float* aov_host, rt_stats* stats);

/* Asynchronous on `hip_stream` (may be NULL): AOVs into a DEVICE buffer. If stats != NULL the
 * call synchronises the stream to fill it. */
int rt_render_aov_device(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                         float* aov_device, void* hip_stream, rt_stats* stats);

/* ---- edge-avoiding a-trous denoiser ---------------------------------------------------------
 * The first consumer of the AOV guides: the wavelet filter of Dammertz et al. 2010 over a full
 * contiguous frame. `beauty` is height*width*3 raw sums (what rt_render* writes), `aov` is
 * height*width*RT_AOV_CHANNELS (what rt_render_aov* writes), `out` is height*width*3 floats in
 * the scale of the beauty sums (the output stage reads it as it reads the beauty). out may be
 * the beauty pointer itself (in place); any other overlap is undefined. The buffers need only
 * 4-byte alignment. Per pixel, with B = beauty_samples and A = aov_samples:
 *   c = beauty / B; n = normal_sum / hits and z = t_sum / hits (0 where hits == 0; n is not
 *   renormalised); a = albedo_sum / A; e = emission_sum / A; m = max(a, 1e-3) per channel;
 *   x0 = (c - e) / m with RT_DENOISE_DEMODULATE, else c.
 * A pixel whose x0 has a non-finite component is invalid: it is no one's neighbour and its
 * output is a bitwise copy of its beauty sums. Level k = 0 .. levels-1 steps s = 2^k pixels over
 * the 5x5 taps q = p + s*(i, j), j outer, i inner; taps outside the frame or on invalid pixels
 * are skipped; w = h[i]*h[j]*exp(-E), h = (1/16, 1/4, 3/8, 1/4, 1/16), E the sum of the enabled
 *   colour |x_p - x_q|^2 / (sigma_color * 2^-k)^2      normal |n_p - n_q|^2 / sigma_normal^2
 *   albedo |a_p - a_q|^2 / sigma_albedo^2
 *   depth  (z_p - z_q)^2 / (sigma_depth^2 * max(z_p^2, z_q^2, 1e-30))
 * and x_{k+1}(p) = sum w x_k(q) / sum w. Then y = x*m + e (demodulated) or x, out = y * B.
 * f32 arithmetic, no atomics, fixed tap order: the same inputs give the same bits on every call.
 *
 * A handle owns one device workspace, grown on demand: 48 B per pixel of guides and colour plus,
 * for levels > 1, the 16 B per pixel the levels alternate with. Calls on one handle are
 * serialised by a mutex and each call's stream waits for the handle's previous call (an event
 * wait, whatever stream that was issued on); different handles run concurrently;
 * rt_denoiser_destroy waits for the handle's work. Null pointers, params and flags are checked
 * before the handle is read and before any HIP call: width <= 0, height < 0, width*height >=
 * 2^31, levels outside 1..RT_DENOISE_MAX_LEVELS, non-finite or non-positive sample counts,
 * non-finite sigmas and unknown flag bits are RT_ERR_INVALID_ARG; height == 0 returns RT_OK and
 * touches nothing. rt_stats: ms_kernel (events around the call's launches), ms_total, samples =
 * pixels, launches = kernel launches, out_bytes = bytes written to out; ops all zero. */
#define RT_DENOISE_MAX_LEVELS 8
#define RT_DENOISE_DEMODULATE 0x1u   /* filter (beauty - emission) / max(albedo, 1e-3), re-modulate after */

typedef struct rt_denoise_params {   /* 48 bytes, no padding */
  int32_t width;           /* pixels per row */
  int32_t height;          /* rows; the buffers are full contiguous frames, top row first */
  int32_t levels;          /* a-trous levels 1..RT_DENOISE_MAX_LEVELS; level k steps 2^k pixels */
  uint32_t flags;          /* RT_DENOISE_* ; unknown bits are RT_ERR_INVALID_ARG */
  double beauty_samples;   /* samples each beauty sum holds (> 0, finite) */
  double aov_samples;      /* samples each AOV sum holds (> 0, finite) */
  float sigma_color;       /* edge-stopping widths; <= 0 switches that term off */
  float sigma_normal;
  float sigma_depth;
  float sigma_albedo;
} rt_denoise_params;

typedef struct rt_denoiser rt_denoiser;   /* opaque: device ordinal + workspace + ordering event */

/* host only: levels 5, RT_DENOISE_DEMODULATE, sigmas 4.0 / 0.3 / 0.1 / 0.1 */
int  rt_denoise_default_params(int width, int height, double beauty_samples, double aov_samples,
                               rt_denoise_params* out);
int  rt_denoiser_create(int device, rt_denoiser** out);
void rt_denoiser_destroy(rt_denoiser* dn);
/* asynchronous on hip_stream (may be NULL); stats != NULL synchronises */
int  rt_denoise_device(rt_denoiser* dn, const rt_denoise_params* p, const float* beauty_dev,
                       const float* aov_dev, float* out_dev, void* hip_stream, rt_stats* stats);
/* synchronous, host buffers */
int  rt_denoise(rt_denoiser* dn, const rt_denoise_params* p, const float* beauty,
                const float* aov, float* out, rt_stats* stats);

/* ---- per-pixel sample moments ----------------------------------------------------------------
 * rt_render_device plus the second moment of what it sums. accum_rgb is exactly what
 * rt_render_device writes for the same arguments, bit for bit. m2_rgb holds n_rows * W * 3 floats:
 * per pixel and channel Q = sum_j R_j^2 over the call's stratum rows s_j in s_j order, R_j being
 * the f64 total of row s_j's samples that the reduction adds into the running sum (whatever item
 * kinds the launch split the row into); each step is q = fma(R, R, q) in f64 and the result is
 * rounded once to f32. RT_FLAG_OVERWRITE governs both buffers: without it each m2 value becomes
 * (float)((double)old + q), as for accum, so calls over disjoint sj ranges compose into the sums
 * of the whole frame. A non-finite row total gives the non-finite Q of IEEE arithmetic. Flags,
 * limits, status codes, re-entrancy, slots and the split of tall row ranges are those of
 * rt_render_device; a null m2 pointer is RT_ERR_INVALID_ARG; n_rows == 0 returns RT_OK and touches
 * nothing; rt_stats as rt_render_device fills it. A render that runs as several stratum-row chunks
 * carries Q in a second f64 buffer of its render slot (24 B per pixel, allocated by the slot's
 * first such render).
 *
 * The estimator the pair supports: with n stratum rows held (n >= 2), B samples held and S the
 * beauty sum,
 *   Var(mean) ~= max(0, Q - S^2 / n) * n / ((n - 1) * B^2),
 * the between-row estimate of the variance of the pixel mean S / B (slightly conservative under
 * stratification: the rows are not identically distributed). */
int rt_render_moments_device(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                             float* accum_rgb_device, float* m2_rgb_device, void* hip_stream,
                             rt_stats* stats);
/* synchronous, host buffers */
int rt_render_moments(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                      float* accum_rgb, float* m2_rgb, rt_stats* stats);

/* ---- variance-guided a-trous denoiser ---------------------------------------------------------
 * rt_denoise with the colour distance normalised by a per-pixel variance estimate that is
 * propagated through the levels (Dammertz et al. with the variance guidance of SVGF, Schied et al.
 * 2017). Everything said of rt_denoise_device holds: c, n, z, a, e, m, x0, invalid pixels and
 * their bitwise pass-through, taps and their order, skipped taps, the normal, albedo and depth
 * terms, re-modulation, out == beauty, 4-byte alignment, handle serialisation, stream order, the
 * argument checks (made before the handle is read and before any HIP call). The differences:
 *   m2      height*width*3 floats as rt_render_moments* writes them, over the same
 *           beauty_rows = n stratum rows as the beauty sums S.
 *   var_c   = max(0, Q_c - S_c^2 / n) * n / ((n - 1) * B^2) per channel, evaluated in f64 from the
 *           f32 inputs; v_raw = sum_c var_c / m_c^2 (demodulating) or sum_c var_c, rounded to f32.
 *           A pixel whose Q (or v_raw) has a non-finite component is invalid, like one with a
 *           non-finite x0.
 *   v_0(p)  = sum g v_raw(q) / sum g over the valid in-frame pixels q of the 3x3 block around p,
 *           g = (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), j outer, i inner.
 *   colour  term of level k: |x_p - x_q|^2 / (sigma_color^2 * (v_k(p) + v_k(q) + 1e-10)); no
 *           2^-k factor, the propagated variance takes its place.
 *   v_{k+1}(p) = sum w^2 v_k(q) / (sum w)^2 over the taps and weights that form x_{k+1}(p).
 *   var_out (may be NULL) height*width floats: v_levels(p), the variance of the filtered value in
 *           filter space (demodulated when that flag is set); 0 for invalid pixels. The quantity
 *           an adaptive sampler would threshold.
 * Also RT_ERR_INVALID_ARG: beauty_rows < 2, _pad0 != 0, a null m2. The workspace of a handle that
 * has run this mode is 64 B per pixel whatever the level count (the prefilter writes the second
 * colour record). rt_stats: launches = kernel launches (2 + levels), out_bytes = bytes written to
 * out and var_out. */
typedef struct rt_denoise_var_params {   /* 56 bytes, no padding */
  int32_t width;           /* as rt_denoise_params */
  int32_t height;
  int32_t levels;
  uint32_t flags;          /* RT_DENOISE_DEMODULATE only */
  double beauty_samples;
  double aov_samples;
  int32_t beauty_rows;     /* stratum rows the beauty and m2 sums hold, >= 2 */
  int32_t _pad0;           /* must be 0 */
  float sigma_color;       /* in units of the pair's standard deviation; <= 0 switches the term off */
  float sigma_normal;
  float sigma_depth;
  float sigma_albedo;
} rt_denoise_var_params;

/* host only: levels 5, RT_DENOISE_DEMODULATE, sigmas 4.0 / 0.3 / 0.1 / 0.1 (sigma_color: the best
 * of 0.5, 1, 2, 4 on cornell_box at 4 and at 16 spp) */
int  rt_denoise_var_default_params(int width, int height, double beauty_samples, int beauty_rows,
                                   double aov_samples, rt_denoise_var_params* out);
/* asynchronous on hip_stream (may be NULL); stats != NULL synchronises */
int  rt_denoise_var_device(rt_denoiser* dn, const rt_denoise_var_params* p,
                           const float* beauty_dev, const float* m2_dev, const float* aov_dev,
                           float* out_dev, float* var_out_dev, void* hip_stream, rt_stats* stats);
/* synchronous, host buffers */
int  rt_denoise_var(rt_denoiser* dn, const rt_denoise_var_params* p, const float* beauty,
                    const float* m2, const float* aov, float* out, float* var_out,
                    rt_stats* stats);

/* ---- adaptive sampling: tile-list renders driven by the sample moments --------------------------
 * The consumer of the moments: render some 8x8 tiles and not others, over stratum rows that cover
 * the pixel evenly, and stop a tile once the between-row estimate of its error is small.
 *
 * rt_render_tiles_device: rt_render_moments_device restricted to a list of tiles and a strided
 * set of stratum rows. tiles: HOST array of n_list tile indices of the call's tile grid
 * (tile = ty * ceil(W/8) + tx over the call's n_rows x W pixels), strictly ascending, each <
 * tiles_x * tiles_y; validated on the host (RT_ERR_INVALID_ARG) before any HIP call and copied
 * before the call returns. Stratum rows rendered: sj_begin + k * sj_step, k in [0, sj_count);
 * sj_step >= 1, sj_count >= 1 (0 does not mean "all" here), last row < sqrt_spp. accum/m2: full
 * n_rows*W*3 device buffers; only pixels of listed tiles are read or written (overwritten or added
 * to as RT_FLAG_OVERWRITE says, exactly as rt_render_moments_device does per pixel); m2 may be
 * NULL. With the full list and sj_step 1 both buffers are those of rt_render_moments_device bit for
 * bit; with sj_step = sqrt_spp and sj_count 1 a tile's pixels are rt_render_device's for that row.
 * RT_FLAG_INTERPRETER and RT_FLAG_REFERENCE_BVH are honoured; RT_FLAG_COUNT_OPS is
 * RT_ERR_INVALID_ARG (the op-counting kernels have no tile-list variant); n_rows > 32760 is
 * RT_ERR_UNSUPPORTED (no split into sub-renders: the tile grid is the call's); n_list == 0 or
 * n_rows == 0 returns RT_OK and touches nothing. Asynchronous on hip_stream; stats != NULL
 * synchronises; rt_stats as rt_render_device fills it, samples = pixel-samples of the listed
 * tiles. Re-entrancy, slots and lifetime are those of rt_render_device. */
int rt_render_tiles_device(rt_scene* scene, const rt_camera* cam, const rt_render_opts* opts,
                           const uint32_t* tiles, uint32_t n_list, int32_t sj_step,
                           float* accum_rgb_device, float* m2_rgb_device, void* hip_stream,
                           rt_stats* stats);

/* Host only. Pass p of P over sqrt_spp rows renders rows p, p+P, p+2P, ...: every pass covers the
 * pixel's stratum rows evenly (a contiguous prefix of rows would sample only the top of the
 * pixel). Valid for 1 <= passes <= sqrt_spp / 2 and 0 <= pass < passes, so pass 0 always holds at
 * least 2 rows and the variance estimate exists; otherwise RT_ERR_INVALID_ARG. */
int rt_adaptive_schedule(int sqrt_spp, int passes, int pass, int* sj_begin, int* sj_step,
                         int* sj_count);

/* A handle owns a device workspace (12 B per tile), a mutex that serialises its calls and an
 * ordering event, as rt_denoiser does. Null pointers and value ranges are checked before the
 * handle is read and before any HIP call. width x height is a full contiguous frame whose 8x8
 * tile grid is that of a render of height rows; rows_held: HOST array, one uint32 per tile, the
 * stratum rows the tile's sums hold (<= sqrt_spp).
 *
 * rt_adaptive_tile_error (synchronous): per pixel of a tile with n = rows_held[tile] >= 2 and
 * B = n * sqrt_spp, evaluated in f64 from the f32 inputs,
 *   var_c = max(0, Q_c - S_c^2 / n) * n / ((n - 1) * B^2)      (the estimator above)
 *   e = sqrt(var_r + var_g + var_b) / (max(S_r,0)/B + max(S_g,0)/B + max(S_b,0)/B + floor),
 * the relative standard error of the pixel mean; floor (finite, > 0) keeps black pixels finite.
 * A pixel with a non-finite S, Q or e is invalid: it contributes nothing and is counted in
 * *n_invalid_out (may be NULL); more samples do not cure a NaN. err_out[tile] (HOST, one float per
 * tile) = the maximum of e over the tile's valid pixels rounded to f32, 0 if it has none; +inf for
 * a tile with rows_held < 2, whose pixels are not examined. height == 0 returns RT_OK.
 *
 * rt_adaptive_resolve_device (asynchronous on hip_stream; rows_held is copied before it returns;
 * every rows_held >= 1): per pixel with B_p = rows_held[tile] * sqrt_spp,
 *   out = (float)((double)accum * (sqrt_spp^2 / B_p)),  samples = B_p  (one float per pixel,
 * samples_dev may be NULL): the sums in the scale of a full-spp render, which write_color and
 * rt_denoise with beauty_samples = spp take unchanged. A pixel that holds every row is a bitwise
 * copy. out_dev may equal accum_dev. */
typedef struct rt_adaptive rt_adaptive;
int  rt_adaptive_create(int device, rt_adaptive** out);
void rt_adaptive_destroy(rt_adaptive* ad);
int  rt_adaptive_tile_error(rt_adaptive* ad, int width, int height, int sqrt_spp, double floor,
                            const float* accum_dev, const float* m2_dev, const uint32_t* rows_held,
                            float* err_out, uint64_t* n_invalid_out, void* hip_stream);
int  rt_adaptive_resolve_device(rt_adaptive* ad, int width, int height, int sqrt_spp,
                                const uint32_t* rows_held, const float* accum_dev, float* out_dev,
                                float* samples_dev, void* hip_stream);

/* The driver (synchronous: accum, m2 and the optional outputs are complete on return).
 * opts->sj_begin and sj_count must be 0, RT_FLAG_OVERWRITE must be set (the moments must be the
 * frame's own) and RT_FLAG_COUNT_OPS clear; row_begin, row_step, n_rows (<= 32760), seed and the
 * other flags as for rt_render_device. With S = sqrt_spp and P = passes:
 *   1. the active set starts as all tiles;
 *   2. pass p renders the active list (rt_render_tiles_device) over rt_adaptive_schedule(S, P, p);
 *      pass 0 overwrites, later passes add;
 *   3. rows_held[t] += sj_count for active t;
 *   4. if p + 1 >= min_passes and p + 1 < P: rt_adaptive_tile_error, and the next active set is
 *      {t active : err_t > threshold}, kept ascending;
 *   5. stop when the active set is empty or p = P - 1;
 *   6. a tile never re-enters the active set.
 * out_dev (may be NULL) and samples_dev (may be NULL) receive rt_adaptive_resolve_device's outputs;
 * rows_held_out (HOST, one per tile, may be NULL); tiles_per_pass (HOST, P entries, may be NULL):
 * the length of each pass's list, 0 for passes not run. rt_stats: samples = pixel-samples actually
 * traced, launches = path-kernel launches, ms_kernel = the passes' kernel times summed, ms_total =
 * wall time. Not covered: rt_multi_* and the RCCL path, adaptive AOVs. */
typedef struct rt_adaptive_params {  /* 24 bytes, no padding */
  int32_t passes;      /* P, 1..sqrt_spp/2 */
  int32_t min_passes;  /* 1..P: passes every tile receives */
  double threshold;    /* a tile continues while its error > threshold; may be negative or +inf; NaN invalid */
  double floor;        /* rt_adaptive_tile_error's floor: finite, > 0 */
} rt_adaptive_params;
int rt_render_adaptive_device(rt_adaptive* ad, rt_scene* scene, const rt_camera* cam,
                              const rt_render_opts* opts, const rt_adaptive_params* params,
                              float* accum_rgb_device, float* m2_rgb_device, float* out_dev,
                              float* samples_dev, uint32_t* rows_held_out, uint32_t* tiles_per_pass,
                              void* hip_stream, rt_stats* stats);
/* the same with HOST buffers (accum, m2: n_rows*W*3 floats, written; out and samples may be NULL) */
int rt_render_adaptive(rt_adaptive* ad, rt_scene* scene, const rt_camera* cam,
                       const rt_render_opts* opts, const rt_adaptive_params* params,
                       float* accum_rgb, float* m2_rgb, float* out, float* samples,
                       uint32_t* rows_held_out, uint32_t* tiles_per_pass, rt_stats* stats);

/* ---- device output stage: exposure, gamma and RGB8 ----------------------------------------------
 * The reference's output stage (render.rs:199-213: auto_expose, then write_color per pixel,
 * color.rs:8-59) on the device, so that a frame rendered, denoised or resolved into device memory
 * becomes displayable bytes without a trip through the host. The host functions rth_auto_expose
 * and rth_write_color (rt_host.h) are the single source of truth; this is their definition:
 *
 *   sums    height*width*3 raw f32 sums, top row first, as every render, denoise and resolve entry
 *           point writes them (4-byte aligned). Per value, in f64 and in the host's order:
 *             x = (double)sum * (1.0 / samples_per_pixel)
 *             x = 1. - pow(2.718281828459045, -ev * x)           with an exposure step (color.rs:37-39)
 *             x = x <= 0.0031308 ? 12.92 * x : 1.055 * pow(x, 1. / 2.4) - 0.055    (linear_to_gamma)
 *             x = clamp to [0, 0.999]; a NaN passes the clamp
 *             byte = Rust's saturating `as u8` of 256 * x: NaN -> 0
 *           No product is fused into a sum. The device's pow and the host's may differ in the last
 *           bit, so a byte can differ from rth_write_color's, by 1, only where the host's 256 * x
 *           lies within rounding of an integer.
 *   rgb8    height*width*3 bytes r g b, or height*width*4 bytes r g b 255 with RT_OUTPUT_RGBA; any
 *           alignment; must not overlap sums.
 *   ev      with RT_OUTPUT_EXPOSURE alone, params->exposure. With RT_OUTPUT_AUTO_EXPOSE, over the
 *           N = width*height pixels, lum = 0.2126 r + 0.71516 g + 0.072169 b of the raw sums added
 *           left to right,
 *             m = (sum_p (1/N) * lum_p^2) / samples_per_pixel^2
 *             ev = m > 0.001 ? -ln(0.6) / sqrt(m) : 1
 *           The sum runs in f64 in a fixed order that depends on N alone: reduction block b owns
 *           pixels [2048 b, 2048 (b+1)); its lane t (of 256) adds pixels 2048 b + 256 k + t for
 *           k = 0..7 in that order; the block adds its lanes in a fixed tree (lane t += lane t + s,
 *           s = 128, 64, .. 1); one block then adds the block sums, lane t taking blocks t, t + 256,
 *           .. in ascending order, and the same tree. No atomics: the same inputs give the same ev
 *           and the same bytes on every call; ev agrees with rth_auto_expose to the rounding of
 *           two differently ordered sums of N non-negative terms. IEEE propagation gives the
 *           host's special cases: a NaN pixel makes m NaN and ev = 1; an infinite m gives ev = 0.
 *           ev stays in device memory, where the conversion kernel reads it: an asynchronous call
 *           never waits on the host.
 *
 * A handle owns one device workspace, grown on demand (8 B per 2048 pixels: the block sums, and
 * ev), a mutex that serialises its calls and an ordering event: each call's stream waits for the
 * handle's previous call, whatever stream that was issued on; different handles run concurrently;
 * rt_output_destroy waits for the handle's work. Checked before the handle is read and before any
 * HIP call, RT_ERR_INVALID_ARG each: a null handle, params, sums or rgb8; width <= 0, height < 0,
 * width*height >= 2^31; samples_per_pixel non-finite or <= 0; exposure non-finite with
 * RT_OUTPUT_EXPOSURE set and RT_OUTPUT_AUTO_EXPOSE clear; unknown flag bits; _pad0 != 0.
 * height == 0 returns RT_OK and touches no buffer. exposure_out (may be NULL) receives the ev the
 * call applied, 0 if it had no exposure step. rt_stats: ms_kernel (events around the call's
 * launches), ms_total, samples = pixels, launches = kernel launches (1, or 3 with auto-exposure),
 * out_bytes = bytes written to rgb8; ops all zero.
 *
 * Not covered: auto-exposure over rows spread across ranks or rt_multi_* (a rank may convert its
 * own rows with an explicit exposure it obtained elsewhere); AOV visualisation; dithering; image
 * file encoding. */
#define RT_OUTPUT_EXPOSURE 0x1u     /* x = 1 - E^(-exposure * x) before the gamma (color.rs:37-39)   */
#define RT_OUTPUT_AUTO_EXPOSE 0x2u  /* exposure = auto_expose(frame) (render.rs:325-339), computed on */
                                    /* the device; implies the exposure step; params->exposure ignored */
#define RT_OUTPUT_RGBA 0x4u         /* 4 bytes per pixel, alpha 255; else 3 bytes per pixel           */

typedef struct rt_output_params {   /* 32 bytes, no padding */
  int32_t width, height;            /* a contiguous buffer of height rows, top row first */
  uint32_t flags;                   /* RT_OUTPUT_*; unknown bits are RT_ERR_INVALID_ARG */
  int32_t _pad0;                    /* must be 0 */
  double samples_per_pixel;         /* what the sums hold (finite, > 0): scale = 1.0 / it */
  double exposure;                  /* used with RT_OUTPUT_EXPOSURE alone; finite */
} rt_output_params;

/* opaque: device ordinal, reduction workspace, ordering event (C keeps typedef and function names
 * in one namespace, so the handle cannot share the name of rt_output()) */
typedef struct rt_output_stage rt_output_stage;
int  rt_output_create(int device, rt_output_stage** out);
void rt_output_destroy(rt_output_stage* o);
/* asynchronous on hip_stream (may be NULL); stats != NULL or exposure_out != NULL synchronises */
int  rt_output_device(rt_output_stage* o, const rt_output_params* p, const float* sums_dev,
                      uint8_t* rgb8_dev, double* exposure_out, void* hip_stream, rt_stats* stats);
/* synchronous, host buffers */
int  rt_output(rt_output_stage* o, const rt_output_params* p, const float* sums, uint8_t* rgb8,
               double* exposure_out, rt_stats* stats);

/* ---- temporal accumulation with reprojection of the frame history -------------------------------
 * The third leg of SVGF (Schied et al. 2017) beside the variance estimate and the a-trous filter: a
 * handle keeps the accumulated frame (the history) with the guides and the camera of the frame
 * that wrote it; each call finds every pixel's first-hit point in world space, projects it into
 * the previous camera, gathers the history there with a bilinear footprint whose taps on another
 * surface are rejected, and blends history and new sample sums. Its inputs are what
 * rt_render_moments_device and rt_render_aov_device write, its outputs raw sums in the scale that
 * rt_denoise*, rt_denoise_var* and rt_output* take with the per-frame beauty_samples and
 * beauty_rows unchanged.
 *
 * Buffers: full contiguous frames, height x width, top row first, 4-byte aligned.
 *   beauty  H*W*3 floats, raw sums        m2   H*W*3 floats as rt_render_moments* writes them; may
 *   aov     H*W*RT_AOV_CHANNELS floats         be NULL
 *   cam     the camera that rendered the frame; cam->image_width and image_height must equal the
 *           params'
 * Guides of pixel p = (i, j), column i, row j: hits = aov[RT_AOV_HITS]; where hits > 0,
 * z = T / hits and n = normal_sum / hits in f32, as the denoiser forms them, else z = 0, n = 0;
 * id = aov[RT_AOV_MATID].
 * S = the pixel's beauty sums, Q = its m2 sums. A pixel whose S (or, with m2, Q) has a non-finite
 * component is invalid: its outputs are bitwise copies of its inputs and its history length is
 * stored as 0, so that no later frame takes it as a tap.
 *
 * Reprojection, in f64 from the f32 guides:
 *   D = pixel00_loc + i * pixel_delta_u + j * pixel_delta_v - center     (this call's camera)
 *   X = center + z * D
 *   M' = [pixel00_loc' - center' | pixel_delta_u' | pixel_delta_v'] as columns (previous camera)
 *   M' (s, a, b)^T = X - center';  x' = a / s,  y' = b / s.
 * s is the point's ray parameter in the previous camera, directly comparable with the previous
 * frame's z: both cameras use the reference's unnormalised ray direction. The host inverts M' once
 * per camera in f64 (adjugate over determinant); a camera whose determinant is zero or non-finite
 * is RT_ERR_INVALID_ARG at the call that brings it. (The device forms pixel00_loc - center and
 * center - center' on the host and adds the products to them with fused multiply-adds: the last
 * bits of x' and y' are not specified.)
 *
 * Taps: i0 = floor(x'), j0 = floor(y'), fx = x' - i0, fy = y' - j0; the taps q are (i0, j0),
 * (i0+1, j0), (i0, j0+1), (i0+1, j0+1) in that order, their weights (1-fx)(1-fy), fx(1-fy),
 * (1-fx)fy, fx*fy formed in f64 and rounded to f32. A tap is accepted when it lies in the frame,
 * its stored length is >= 1, its stored z_h > 0, its stored id_h == id (compared exactly),
 * |n_h - n|^2 <= normal_tol^2 (f32) and |z_h - s| <= depth_tol * s (f64). normal_tol <= 0 switches
 * the normal test off, depth_tol <= 0 the depth test.
 *
 * The history is usable at p when the handle holds a frame of the same size, p is valid with
 * hits > 0, s, x' and y' are finite with s > 0, and Wsum, the sum of the accepted weights, is
 * > min_weight. Then S_h, Q_h and L_h are the accepted taps' stored colour, moments and length,
 * each weighted sum divided by Wsum, and
 *   L = min(L_h + 1, max_history),  alpha = 1 / L,  out = (1 - alpha) * S_h + alpha * S
 * in f32, Q blended the same way. Otherwise L = 1 and the outputs are bitwise copies of S and Q.
 * The handle stores per pixel the blended S, the blended Q and L (0 for an invalid pixel), the
 * frame's n, z and id, and the camera, which is the previous camera of the next call.
 *
 * Outputs, in the scale of the inputs: out_beauty H*W*3 (may be the beauty pointer itself);
 * out_m2 H*W*3, required exactly when m2 is given (may equal m2); hist_len H*W floats, L per
 * pixel (may be NULL). Any other overlap is undefined.
 *
 * RT_TEMPORAL_RESET discards the history before the call. RT_TEMPORAL_VARIANCE_OF_MEAN (needs m2
 * and beauty_rows = n >= 2): where the history was used,
 *   out_m2 = S^2 / n + max(0, Q - S^2 / n) / L   per channel,
 * evaluated in f64 from the blended f32 values and rounded once, so that the between-row estimator
 * above returns the variance of the accumulated mean and not of one frame: what rt_denoise_var
 * should be guided by after accumulation. Where the history was not used (L = 1, where the
 * expression is Q itself for every Q >= S^2 / n) out_m2 stays the bitwise copy. The handle stores
 * the plain blended Q either way.
 *
 * The first call, a call with another frame size and a call with RT_TEMPORAL_RESET have no history;
 * each starts a new one. Whether a history carries moments is fixed by the call that starts it; a
 * later call that disagrees (m2 given against a history without moments, or the reverse) is
 * RT_ERR_INVALID_ARG. rt_temporal_info: out[0..3] = frames accumulated since the history started,
 * its width, its height, 1 if it carries moments.
 *
 * f32 arithmetic apart from the projection, the weights and the depth test; no atomics, fixed tap
 * order: the same sequence of calls gives the same bits.
 *
 * A handle owns one device workspace, grown on demand: two history sets of three 16-byte records
 * per pixel, {S, L}, {n, z}, {Q, id} (96 B per pixel), which alternate between calls; a mutex
 * that serialises its calls and an ordering event that every call's stream waits on, whatever
 * stream the call before went to; different handles run concurrently; rt_temporal_destroy waits
 * for the handle's work. Checked before the handle is read and before any HIP call,
 * RT_ERR_INVALID_ARG each: a null handle, params, camera, beauty, aov or out_beauty; width <= 0,
 * height < 0, width*height >= 2^31; unknown flag bits; beauty_rows < 0, or < 2 with
 * RT_TEMPORAL_VARIANCE_OF_MEAN; max_history non-finite or < 1; a non-finite tolerance; min_weight
 * non-finite or outside [0, 1); m2 without out_m2 or the reverse; RT_TEMPORAL_VARIANCE_OF_MEAN
 * without m2; a camera of another size or with a singular M. height == 0 returns RT_OK and
 * touches nothing, the history included. rt_stats: ms_kernel, ms_total, samples = pixels,
 * launches = 1, out_bytes = bytes written to the caller's buffers; ops all zero.
 *
 * Not covered: demodulated accumulation (albedo divided out before the blend); feeding a filtered
 * frame back as history; motion of objects (only the camera moves; a moving Sphere's blur is inside
 * a frame); defocus (the position is formed from center, not from the sampled origin); rows spread
 * over ranks or rt_multi_*; adaptive frames with per-pixel sample counts. */
#define RT_TEMPORAL_RESET 0x1u             /* discard the history before this call */
#define RT_TEMPORAL_VARIANCE_OF_MEAN 0x2u  /* out_m2 in the scale of the accumulated mean's variance */

typedef struct rt_temporal_params {   /* 32 bytes, no padding */
  int32_t width, height;  /* a contiguous frame of height rows, top row first */
  uint32_t flags;         /* RT_TEMPORAL_*; unknown bits are RT_ERR_INVALID_ARG */
  int32_t beauty_rows;    /* n of the estimator; >= 2 with VARIANCE_OF_MEAN, else must be >= 0 */
  float max_history;      /* finite, >= 1: the longest history length, alpha >= 1 / max_history */
  float depth_tol;        /* relative; <= 0 off */
  float normal_tol;       /* <= 0 off */
  float min_weight;       /* finite, in [0, 1) */
} rt_temporal_params;

typedef struct rt_temporal rt_temporal;   /* opaque: device ordinal, history, camera, ordering event */

/* host only: flags 0, beauty_rows 0, max_history 4, depth_tol 0.1 and normal_tol 0.3 (the
 * denoiser's sigma_depth and sigma_normal: a neighbour more than one edge width away is another
 * surface; max_history: the best of 4, 8, 16, 32 for accumulation followed by rt_denoise_var on
 * cornell_box and on final_scene at 4 spp over an 8-frame orbit of 2 degrees per frame, DESIGN.md
 * section 4.2h), min_weight 0.01 */
int  rt_temporal_default_params(int width, int height, rt_temporal_params* out);
int  rt_temporal_create(int device, rt_temporal** out);
void rt_temporal_destroy(rt_temporal* t);
int  rt_temporal_info(rt_temporal* t, uint64_t* out, int n);
/* asynchronous on hip_stream (may be NULL); stats != NULL synchronises */
int  rt_temporal_accumulate_device(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam,
                                   const float* beauty_dev, const float* m2_dev,
                                   const float* aov_dev, float* out_beauty_dev, float* out_m2_dev,
                                   float* hist_len_dev, void* hip_stream, rt_stats* stats);
/* synchronous, host buffers */
int  rt_temporal_accumulate(rt_temporal* t, const rt_temporal_params* p, const rt_camera* cam,
                            const float* beauty, const float* m2, const float* aov,
                            float* out_beauty, float* out_m2, float* hist_len, rt_stats* stats);

/* ---- ray queries: closest hits for caller-supplied rays -----------------------------------------
 * What does this ray hit? Every other entry point forms its rays from an rt_camera; this one takes
 * them from the caller, so picking, depth or visibility for camera models rt_camera cannot express
 * (orthographic, fisheye, panoramas, lidar patterns), ambient-occlusion or shadow-ray batches and
 * geometric checks of a scene need no second ray tracer.
 *
 * Each ray runs ONE world.hit(r, Interval{tmin, tmax}) (hittable.rs:88-109) through the interpreter
 * walker, exactly as the AOV pass runs its query: the scene's ordered BVHs are walked from LDS, or
 * the reference tree in the reference's order under RT_FLAG_REFERENCE_BVH (same records, bit for
 * bit). The interval ends are the reference's: a Quad accepts t == tmin and t == tmax (object.rs:
 * 462), a Sphere's root must lie strictly inside (object.rs:156-163), and of two quads at the same
 * t the later one in the list wins. A ConstantMedium's free-flight draw comes from a generator
 * freshly seeded with rng_seed(params->seed, ray.pixel, ray.sample), the keying of the render
 * passes; scenes without media ignore seed, pixel and sample. A ray's record depends on that ray
 * and the params alone: not on its place in the batch, its neighbours or n_rays.
 *
 * prim: the place of the hit primitive among the world's spheres, quads and ConstantMediums in the
 * blob's pre-order (a ConstantMedium's boundary primitives are counted after it), so a caller can
 * map it back to the object it serialised. It is the primitive the reference's own hit record
 * comes from. That matters in one case: a BvhNode over a span of one leaf holds the leaf twice
 * (hittable.rs:161-162) and re-tests it over [tmin, rec.t]; a quad's inclusive interval accepts
 * again, so the reference's record is the second copy's, while a sphere's strict one is the first
 * copy's. rt_scene_prim_map returns the table behind it, by leaf-record word offset of the
 * flattened node array, ascending in word: every QUAD, SPHERE and VOLUME record of the world is
 * listed, the copies a BvhNode layout duplicates included, and the prims are exactly 0 .. n-1. In
 * a duplicated quad pair the first copy's record (the one the walker reports) carries the second
 * copy's prim and the second copy's record the first's. *n_out is the entry count even if cap is
 * smaller; at most cap entries are written. rt_scene_create keeps the table; the scene's first
 * query uploads it, under the scene mutex.
 *
 * Invalid rays: a non-finite origin, dir or time component, a dir that is all zero, a NaN tmin or
 * tmax, an infinite tmin. Such a ray never reaches the walker (its lane walks a fixed harmless ray
 * with its wave); its record is hit = -1 and every other field 0, in occlusion mode the byte 255.
 * The other rays' records are unaffected and the call returns RT_OK.
 *
 * Any-hit mode (mode == RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT): the users of occlusion mode (shadow
 * rays, ambient occlusion, visibility between two points, lidar returns) need no closest hit, only
 * whether anything lies in [tmin, tmax]. The any-hit walk leaves at the first primitive that accepts
 * and writes, for every ray, the byte RT_QUERY_OCCLUSION alone writes for the same ray and params
 * (1, 0, or 255 for an invalid ray), with and without RT_FLAG_REFERENCE_BVH and on scenes with
 * ConstantMedium records. Why the bytes are equal: a primitive's accept test is monotone in the
 * upper end of the interval (a quad's t <= closest, a sphere's choice of root: whatever accepts
 * under a smaller upper end accepts under a larger one), so "some primitive accepts in
 * [tmin, tmax]" is the closest-hit walk's final hit flag. Up to the first accept both walks see the
 * same interval and the same generator state, so a ConstantMedium draws the same numbers, and after
 * the first accept the closest-hit flag never goes back to false. A ray with tmax < tmin can be
 * accepted by nothing and leaves at once (byte 0). Argument checks, slots, stream order and rt_stats
 * are those of occlusion mode. The bit is valid only together with RT_QUERY_OCCLUSION: any-hit has
 * no record to fill.
 *
 * Checked before the scene is read and before any HIP call, RT_ERR_INVALID_ARG each: a null scene,
 * params, rays or out; n_rays >= 2^31; flag bits other than RT_FLAG_REFERENCE_BVH; mode bits other
 * than RT_QUERY_OCCLUSION and RT_QUERY_ANY_HIT, or RT_QUERY_ANY_HIT without RT_QUERY_OCCLUSION; rays
 * not 16-byte aligned; out not 16-byte aligned in record mode.
 * n_rays == 0 returns RT_OK and touches nothing. Slots, stream ordering, re-entrancy and lifetime
 * are those of rt_render_aov_device. rt_stats: ms_kernel, ms_total; samples = n_rays; launches = 1;
 * out_bytes = bytes written (80 or 1 per ray); ops all zero.
 *
 * Not covered: u, v, albedo or emission at the hit; the scene-specialised hiprtc walker, whose interval is
 * fixed; rt_multi_*. */
typedef struct rt_ray {        /* 80 bytes, no padding */
  double origin[3];
  double dir[3];               /* not normalised: t is the ray parameter, as everywhere in this ABI */
  double time;                 /* Ray::time: a moving Sphere's centre */
  double tmin, tmax;           /* the interval handed to world.hit; tmax may be +inf */
  uint32_t pixel, sample;      /* the ray's random stream: rng_seed(params->seed, pixel, sample) */
} rt_ray;

typedef struct rt_hit {        /* 80 bytes, no padding */
  double t;                    /* rec.t; the ray's own tmax on a miss; 0 for an invalid ray */
  double distance;             /* t * sqrt(dir . dir), f64; 0 unless hit == 1 */
  double p[3];                 /* rec.p, world space; 0 unless hit == 1 */
  double normal[3];            /* rec.normal after set_face_normal, world space; a ConstantMedium hit has (1,0,0) */
  int32_t hit;                 /* 1 hit, 0 miss, -1 invalid ray */
  int32_t front_face;          /* rec.front_face (1 for a ConstantMedium hit); 0 unless hit == 1 */
  int32_t material;            /* blob material-table index; -1 on a miss, 0 for an invalid ray */
  int32_t prim;                /* see above; -1 on a miss, 0 for an invalid ray */
} rt_hit;

#define RT_QUERY_OCCLUSION 0x1u   /* out is one uint8 per ray: 1 hit, 0 miss, 255 invalid */
#define RT_QUERY_ANY_HIT 0x2u     /* with RT_QUERY_OCCLUSION only: the same bytes from a walk that
                                     leaves at the first accepted primitive */

typedef struct rt_query_params {  /* 16 bytes */
  uint64_t seed;
  uint32_t flags;              /* RT_FLAG_REFERENCE_BVH only; any other RT_FLAG_* bit is RT_ERR_INVALID_ARG */
  uint32_t mode;               /* 0, RT_QUERY_OCCLUSION or RT_QUERY_OCCLUSION | RT_QUERY_ANY_HIT;
                                  anything else RT_ERR_INVALID_ARG */
} rt_query_params;

/* asynchronous on hip_stream (may be NULL): device buffers; stats != NULL synchronises */
int rt_query_rays_device(rt_scene* scene, const rt_query_params* params, const rt_ray* rays_dev,
                         uint64_t n_rays, void* out_dev, void* hip_stream, rt_stats* stats);
/* synchronous, host buffers */
int rt_query_rays(rt_scene* scene, const rt_query_params* params, const rt_ray* rays,
                  uint64_t n_rays, void* out, rt_stats* stats);
/* host only, no device: the table behind rt_hit.prim */
int rt_scene_prim_map(const rt_scene_blob* blob, uint32_t* node_word, uint32_t* prim, uint32_t cap,
                      uint32_t* n_out);

/* ---- ray renders: path-traced radiance for caller-supplied rays ----------------------------------
 * What does this ray see? rt_query_rays answers what a caller's ray hits; this entry point runs the
 * path tracer itself on it, through the kernels of rt_render (the ahead-of-time instance of the
 * scene's variant or its scene-specialised kernel, the same flags), so a panorama or fisheye frame,
 * an irradiance probe, a light-map texel or one pixel's radiance for debugging come out at the
 * parity of the pinhole render. The result is a plain n_rays*3 float buffer of sums, as rt_render's
 * accum: the denoisers, the temporal pass and the output stage take a frame made of it unchanged.
 *
 * Paths and streams. Ray r runs S*S paths, S = sqrt_paths: k = s_j*S + s_i, s_j outer, s_i inner.
 * Path k
 *   1. seeds its generator with rng_seed(seed, ray.pixel, ray.sample + k) (the sample key mod 2^32);
 *   2. discards stream_skip generator steps;
 *   3. takes its time: with RT_RAYS_STREAM_TIME (needs stream_skip >= 1) the last discarded step,
 *      read as random_double; otherwise ray.time;
 *   4. L_k = ray_color(Ray{origin, dir, time}, max_depth) (render.rs:251-311) continues that
 *      generator, with `background` as the miss colour.
 * stream_skip = 3 with RT_RAYS_STREAM_TIME leaves the stream exactly where get_ray leaves it for a
 * camera without defocus (two jitter draws, the time draw): a ray that equals a camera ray then
 * gives that pixel-sample's value bit for bit, and a host ray generator may spend draws 1-2 on its
 * own jitter (rt_host.h rth_projection_rays does). ray.tmin and ray.tmax are NOT read: ray_color's
 * interval is [1e-4, inf) at every bounce, and the scene-specialised walker's is fixed.
 *
 * Sum. rgb[3r ..] is the sum of the L_k formed exactly as rt_render forms a pixel's sum at
 * sqrt_spp = S: per s_j block partials of 8 consecutive s_i, the row total over the blocks, then
 * the rows in order, in f64, rounded once to f32. Without RT_FLAG_OVERWRITE the value written is
 * (float)((double)old + sum). A ray's result depends on that ray and the params alone: not on its
 * place in the batch, on n_rays, or on how the call was split into launches or chunks.
 *
 * Invalid rays: a non-finite origin, dir or time component, or a dir that is all zero. Such a ray
 * never hands its values to the walker (its lane walks a fixed harmless ray with its wave); its
 * three outputs become quiet NaN whatever the flags. The other rays are unaffected and the call
 * returns RT_OK.
 *
 * Checked before the scene is read and before any HIP call, RT_ERR_INVALID_ARG each: a null scene,
 * params, rays or rgb; n_rays >= 2^31; flag bits other than RT_FLAG_OVERWRITE, RT_FLAG_INTERPRETER,
 * RT_FLAG_REFERENCE_BVH and RT_FLAG_SEMANTICS_REFERENCE (RT_FLAG_COUNT_OPS included: the counting
 * kernels have no ray variant); unknown mode bits; _pad0 != 0; sqrt_paths < 1; max_depth < 0;
 * stream_skip > RT_RAYS_MAX_SKIP; RT_RAYS_STREAM_TIME with stream_skip == 0; rays not 16-byte
 * aligned. The background is passed through as it is, non-finite values included, as the
 * reference's. sqrt_paths > 32768 or max_depth > 0xffffff: RT_ERR_UNSUPPORTED. With
 * RT_FLAG_SEMANTICS_REFERENCE, an empty light list and a diffuse or volume material:
 * RT_ERR_EMPTY_LIGHTS, as a render. n_rays == 0 returns RT_OK and touches nothing. Slots, stream
 * ordering, re-entrancy and lifetime are those of rt_render_device. rt_stats as rt_render_device
 * fills it: samples = n_rays * S * S, launches = path-kernel launches.
 *
 * Not covered: second moments for ray renders, subsets of the stratum rows, rt_multi_*, op
 * counting. */
#define RT_RAYS_STREAM_TIME 0x1u  /* a path's time is the last skipped draw, not ray.time */
#define RT_RAYS_MAX_SKIP 16

typedef struct rt_rays_params {   /* 56 bytes, no padding */
  uint64_t seed;
  uint32_t flags;        /* RT_FLAG_OVERWRITE | INTERPRETER | REFERENCE_BVH | SEMANTICS_REFERENCE */
  uint32_t mode;         /* RT_RAYS_*; unknown bits RT_ERR_INVALID_ARG */
  int32_t  sqrt_paths;   /* S >= 1: S*S paths per ray, S <= 32768 */
  int32_t  max_depth;    /* 0 .. 0xffffff, as rt_camera.max_depth */
  uint32_t stream_skip;  /* generator steps discarded before a path starts, 0..RT_RAYS_MAX_SKIP */
  uint32_t _pad0;        /* must be 0 */
  double   background[3];
} rt_rays_params;

/* asynchronous on hip_stream (may be NULL): device buffers; stats != NULL synchronises */
int rt_render_rays_device(rt_scene* scene, const rt_rays_params* params, const rt_ray* rays_dev,
                          uint64_t n_rays, float* rgb_dev /* n_rays*3 */, void* hip_stream,
                          rt_stats* stats);
/* synchronous, host buffers */
int rt_render_rays(rt_scene* scene, const rt_rays_params* params, const rt_ray* rays,
                   uint64_t n_rays, float* rgb, rt_stats* stats);

/* ---- ray generators on the device: projection rays, AO ray batches, an AO frame -------------------
 * rt_query_rays and rt_render_rays answer rays at device speed; these entry points form the rays
 * there too, so a panorama, fisheye or ortho frame and an ambient-occlusion frame need no host loop
 * and no transfer of 80-byte records. The host generators of rt_host.h (rth_projection_rays,
 * rth_ao_rays) remain the definition of every field; the kernels restate them in f64 with the
 * host's operations in the host's order, fma exactly where the host writes fma. Pinhole and ortho
 * rays, and every field of the other kinds that takes no sin, cos, atan2 or hypot, are therefore
 * the host's bit for bit; a panorama, fisheye or AO direction differs from the host's by the last
 * bits of those four functions (the device math library's against the host libm's; DESIGN.md
 * section 4.2k gives the measured bound).
 *
 * rt_raygen is a stage handle as rt_output_stage: a device ordinal, a workspace (used by
 * rt_ambient_occlusion_device alone) and an ordering event. Calls on one handle are serialised
 * and ordered, whatever streams they go to. Every call is asynchronous on hip_stream (may be
 * NULL); stats != NULL synchronises.
 *
 * rt_projection_rays_device: rth_projection_rays restricted to the frame rows [row_begin,
 * row_begin + n_rows) of ONE stratum (s_i, s_j). With W the frame width, ray (i, j) goes to
 * rays_dev[(j - row_begin) * W + i] and carries pixel = j * W + i, so a frame can be generated and
 * consumed in bands. proj has the layout and the meaning of rth_projection, RT_PROJ_* the values of
 * RTH_PROJ_*; cam is read for RT_PROJ_PINHOLE only (its width, height and sqrt_spp are then the
 * frame's). The frame vectors f, r, u are formed on the host by rth_projection_rays' own code and
 * reach the kernel as arguments. Checked as rth_projection_rays checks (sizes >= 1 and width *
 * height < 2^31, a stratum outside sqrt_spp, an unknown kind, a zero or non-finite frame vector, a
 * non-finite origin, a non-positive fov where it is read), and: row_begin < 0, n_rows < 0,
 * row_begin + n_rows > height, rays_dev not 16-byte aligned. n_rows == 0 returns RT_OK and touches
 * nothing. rt_stats: samples = rays written, out_bytes = 80 per ray, launches = 1.
 *
 * rt_ao_rays_device: rth_ao_rays on device buffers: from n primary rays and their records
 * (rt_query_rays_device, record mode) the dir_index-th cosine-distributed direction about each
 * hit's normal, origin = hits[i].p, time and pixel the primary's, sample = dir_index, the interval
 * [tmin, radius]. A lane whose hits[i].hit != 1 writes an all-zero origin and dir (an invalid ray:
 * the query answers 255). out_dev may be primary_dev. rt_stats as above.
 *
 * rt_ao_accumulate_device: for every ray i and c < channels
 *   sums[i * channels + c] = (flags & RT_FLAG_OVERWRITE ? 0 : old) + (occ[i] == 0 ? 1.0f : 0.0f),
 * so the bytes 1 (occluded) and 255 (no surface: an invalid AO ray) add nothing and a pixel that
 * saw no surface stays black. channels is 1 or 3 (the count replicated: what rt_output and
 * rt_denoise take). rt_stats: samples = n, out_bytes = 4 * channels per ray, launches = 1.
 *
 * rt_ambient_occlusion_device: the ambient-occlusion frame of n primary rays without a host round
 * trip. Per chunk of at most chunk_rays rays: a record-mode rt_query_rays_device of the primaries
 * into the workspace (into hits_out_dev if given), then for k = 0 .. directions-1
 * rt_ao_rays_device with dir_index = k into the workspace, an any-hit query (RT_QUERY_OCCLUSION |
 * RT_QUERY_ANY_HIT, the caller's RT_FLAG_REFERENCE_BVH, the params' seed) into workspace bytes and
 * rt_ao_accumulate_device, which overwrites at k == 0 only, and only when RT_FLAG_OVERWRITE is set.
 * sums_dev[i * channels + c] ends as the number of unoccluded directions of ray i (plus its old
 * value without RT_FLAG_OVERWRITE): divide by `directions`, or hand it to rt_output with
 * samples_per_pixel = directions. Everything goes on hip_stream; nothing waits on the host unless
 * stats != NULL. A ray's result depends on that ray and the params alone, so the chunking is
 * invisible in the output; the workspace is at most 161 bytes x the chunk. The scene must live on
 * the handle's device. rt_stats: samples = n * directions; launches = the kernel launches of the
 * call; ms_kernel = the sum over those launches; out_bytes = the bytes written to the caller's
 * buffers (sums, and hits_out_dev if given).
 *
 * Checked before the handle is read and before any HIP call, RT_ERR_INVALID_ARG each: null
 * pointers (hits_out_dev and stats may be NULL); n >= 2^31; ray or hit buffers not 16-byte
 * aligned; _pad0 != 0; a tmin that is not finite or < 0; a radius that is NaN or <= tmin;
 * directions == 0; channels not 1 or 3; unknown flag bits (rt_ao_accumulate_device takes
 * RT_FLAG_OVERWRITE, rt_ambient_occlusion_device RT_FLAG_OVERWRITE | RT_FLAG_REFERENCE_BVH); and
 * the projection's checks above. n == 0 returns RT_OK and touches nothing.
 *
 * Not covered: sorting or compacting rays, bent normals, distance-weighted AO, rt_multi_*. */
#define RT_PROJ_PINHOLE 0   /* values and meaning of RTH_PROJ_* (rt_host.h) */
#define RT_PROJ_ORTHO 1
#define RT_PROJ_PANORAMA 2
#define RT_PROJ_FISHEYE 3
typedef struct rt_projection {   /* 96 bytes, the layout of rth_projection */
  int32_t kind;
  int32_t width, height, sqrt_spp;
  double origin[3], forward[3], up[3];
  double fov;
} rt_projection;
typedef struct rt_ao_params {    /* 32 bytes, the layout of rth_ao_params */
  uint64_t seed;
  double radius;
  double tmin;
  uint32_t dir_index;
  uint32_t _pad0;
} rt_ao_params;
typedef struct rt_ao_frame_params {  /* 40 bytes, no padding */
  uint64_t seed;
  double radius;
  double tmin;
  uint32_t directions;   /* K >= 1 */
  uint32_t flags;        /* RT_FLAG_OVERWRITE | RT_FLAG_REFERENCE_BVH only */
  uint32_t channels;     /* 1 or 3 (the count replicated: what rt_output / rt_denoise take) */
  uint32_t chunk_rays;   /* 0 = default (2^22); else rays per internal chunk, >= 1 */
} rt_ao_frame_params;

typedef struct rt_raygen rt_raygen;  /* opaque: device ordinal, workspace, ordering event */
int  rt_raygen_create(int device, rt_raygen** out);
void rt_raygen_destroy(rt_raygen* g);

int rt_projection_rays_device(rt_raygen* g, const rt_projection* proj, const rt_camera* cam,
                              uint64_t seed, int32_t s_i, int32_t s_j, int32_t row_begin,
                              int32_t n_rows, rt_ray* rays_dev, void* hip_stream, rt_stats* stats);
int rt_ao_rays_device(rt_raygen* g, const rt_ao_params* p, const rt_ray* primary_dev,
                      const rt_hit* hits_dev, uint64_t n, rt_ray* out_dev, void* hip_stream,
                      rt_stats* stats);
int rt_ao_accumulate_device(rt_raygen* g, const uint8_t* occ_dev, uint64_t n, uint32_t channels,
                            uint32_t flags, float* sums_dev, void* hip_stream, rt_stats* stats);
int rt_ambient_occlusion_device(rt_raygen* g, rt_scene* scene, const rt_ao_frame_params* p,
                                const rt_ray* primary_dev, uint64_t n, float* sums_dev,
                                rt_hit* hits_out_dev /* may be NULL */, void* hip_stream,
                                rt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
