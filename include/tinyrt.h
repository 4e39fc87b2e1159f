/*
 * tinyrt.h — C ABI of the MI355X-native path-tracing sampler (libtinyrt.so).
 *
 * Drop-in boundary for ONE path of cheolwanpark/tiny-raytracer: the per-pixel Monte-Carlo
 * bounce loop (`CpuSampler::single_point_sampling`, raytracer/src/renderer/sampler/cpu.rs:39-65)
 * together with the primary-ray generation that feeds it (renderer/pointgen.rs:37-52,
 * camera.rs:58-66) and the f32 accumulation that drains it (renderer/imager.rs:34-60).
 *
 * The reference's plug-in point is `trait Sampler::sampling(world, Receiver<SamplePoint>,
 * Sender<SampledColor>)` (renderer/sampler/mod.rs:10-17), invoked by `Renderer::render`
 * (renderer/renderer.rs:45-49,68-70).  One 32-byte message in and one 20-byte message out
 * per sample cannot feed a GPU, so the boundary sits one level up, at the
 * World / Camera / Renderer::render() surface; `trt_sample_batch` keeps the literal
 * batch form (SamplePoint[] -> SampledColor[]) the reference's own GPU sampler uses
 * (renderer/sampler/metal/sampler.rs:49-65,107-130).
 *
 * Conventions: plain C, POD only, no exceptions cross this boundary.  Every function that
 * can fail returns `int`: 0 = TRT_OK, negative = error; `trt_last_error()` gives the
 * message of the calling thread's last failure.  (The reference panics instead:
 * cpu.rs:35,85; world.rs:29-31; renderer.rs:75-77.)  Handles are opaque and owned by the
 * library; every buffer is caller-allocated and caller-owned; the library keeps no caller
 * pointer after a call returns.  All arithmetic is f32 (`pub type Float = f32`, lib.rs:4).
 */
#ifndef TINYRT_H
#define TINYRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRT_ABI_VERSION 4   /* 2 (round 3): + trt_scene_trim, trt_streamed_launch_plan, trt_band_copy_plan
                             * 3 (round 4): tuning moved out of the process environment: trt_tuning (trt_render_params.tuning),
                             *              trt_scene_options + trt_scene_create_ex; trt_stats.gather_per_band
                             * 4 (round 5): + trt_world_add_spheres; trt_scene_options.top_nodes is ignored (the LDS cache of a large scene's upper
                             *              tree levels is gone: measured slower in every form); d_counters[12..15] = shades by material kind.
                             *              No struct changed size or moved a field.
 *              Later under 4 (new symbols only): trt_scene_create_on_device, trt_scene_get_packed; trt_hit, trt_intersect, trt_occluded,
 *              trt_intersect_device, trt_occluded_device; trt_query_plan, trt_query_launch_plan; trt_primary_rays,
 *              trt_primary_rays_device; trt_aov_buffers, trt_render_aov, trt_render_aov_device, trt_aov_launch_plan;
 *              trt_denoise_params, trt_denoise_params_default, trt_denoise_inputs, trt_denoise_scratch_bytes, trt_denoise,
 *              trt_denoise_device; trt_render_moments, trt_render_moments_device, trt_variance, trt_variance_device;
 *              trt_denoise_color, trt_denoise_color_default, trt_denoise_ex, trt_denoise_ex_device; trt_render_pixels,
 *              trt_render_pixels_device, trt_pixels_launch_plan, trt_select_pixels, trt_select_pixels_device,
 *              trt_select_scratch_bytes; trt_radiance_params, trt_radiance_params_default, trt_radiance, trt_radiance_device,
 *              trt_radiance_launch_plan; trt_lobe, trt_gather_params, trt_gather_params_default, trt_gather, trt_gather_device,
 *              trt_gather_launch_plan; trt_ambient_params, trt_ambient_params_default, trt_ambient, trt_ambient_device,
 *              trt_ambient_launch_plan; trt_probe_domain, trt_probe_params, trt_probe_params_default, trt_probe, trt_probe_device,
 *              trt_probe_launch_plan; trt_passes_source, trt_passes_params, trt_passes_params_default, trt_passes, trt_passes_device,
 *              trt_passes_launch_plan; trt_emitter, trt_scene_emitters, trt_emitter_init_quad, trt_emitter_init_sphere, trt_direct_params,
 *              trt_direct_params_default, trt_direct, trt_direct_device, trt_direct_launch_plan; trt_nee_params, trt_nee_params_default,
 *              trt_nee, trt_nee_device, trt_nee_launch_plan; trt_mis_heuristic, trt_nee_mis_params, trt_nee_mis_params_default,
 *              trt_nee_mis, trt_nee_mis_device, trt_nee_mis_launch_plan; trt_direct_mis_params, trt_direct_mis_params_default,
 *              trt_direct_mis, trt_direct_mis_device, trt_direct_mis_launch_plan; trt_emitter_pick, trt_emitter_pick_build,
 *              trt_direct_pick, trt_direct_pick_device, trt_direct_pick_launch_plan, trt_direct_mis_pick, trt_direct_mis_pick_device,
 *              trt_direct_mis_pick_launch_plan; trt_nee_pick, trt_nee_pick_device, trt_nee_pick_launch_plan, trt_nee_mis_pick,
 *              trt_nee_mis_pick_device, trt_nee_mis_pick_launch_plan; trt_sample_source, trt_samples_params, trt_samples_params_default,
 *              trt_samples, trt_samples_device, trt_samples_launch_plan, trt_fold_samples, trt_fold_samples_device;
 *              trt_nee_samples_params, trt_nee_samples_params_default, trt_nee_samples, trt_nee_samples_device,
 *              trt_nee_samples_launch_plan; trt_project_samples, trt_project_samples_device, trt_probe_parallel,
 *              trt_probe_parallel_device, trt_probe_parallel_launch_plan. */

enum trt_status {
    TRT_OK = 0,
    TRT_ERR_INVALID_ARG = -1,     /* null pointer, bad index, empty world, bad range */
    TRT_ERR_DUPLICATE = -2,       /* material name already present (world.rs:29-31 panics) */
    TRT_ERR_NOT_FOUND = -3,       /* material name absent (world.rs:35-41 returns None) */
    TRT_ERR_HIP = -4,             /* HIP runtime error; message carries hipGetErrorString */
    TRT_ERR_NO_DEVICE = -5,       /* no gfx950 device visible: the product never falls back to a CPU path */
    TRT_ERR_OOM = -6
};

/* ---- POD layouts fixed by the reference (#[repr(C)], tightly packed, 4-byte aligned) ---- */
typedef struct { float x, y, z; } trt_vec3;                          /* math/vec3.rs:9-15      12 B */
typedef struct { trt_vec3 origin, direction; } trt_ray;              /* ray.rs:4-9             24 B */
typedef struct { uint32_t x, y; trt_ray ray; } trt_sample_point;     /* renderer/pointgen.rs:7-13  32 B */
typedef struct { uint32_t x, y; trt_vec3 color; } trt_sampled_color; /* renderer/imager.rs:9-15    20 B */

/* ---- materials (material/{lambertian,metal,dielectric,light}.rs) ---- */
enum trt_material_kind {
    TRT_LAMBERTIAN = 0,   /* Lambertian::new(albedo)                  lambertian.rs:10-12 */
    TRT_METAL = 1,        /* Metal::new(albedo, fuzz), fuzz clamped   metal.rs:12-14      */
    TRT_DIELECTRIC = 2,   /* Dielectric::new(albedo, refraction_index) dielectric.rs:12-14 */
    TRT_LIGHT = 3         /* Light::new(color)                        light.rs:11-13      */
};
typedef struct {
    uint32_t kind;        /* enum trt_material_kind */
    trt_vec3 albedo;      /* albedo, or emitted colour for TRT_LIGHT */
    float param;          /* fuzz (metal) | refraction index (dielectric) | unused */
} trt_material;

/* ---- World: the scene container (hittable/world.rs:10-45) ---- */
typedef struct trt_world trt_world;
int trt_world_create(trt_world **out);                                            /* World::new        world.rs:16-21 */
void trt_world_destroy(trt_world *w);
int trt_world_add_material(trt_world *w, const char *name, const trt_material *m); /* World::add_material world.rs:27-33 */
int trt_world_get_material(const trt_world *w, const char *name, uint32_t *index); /* World::get_material world.rs:35-41 */
/* World::add_geometry(Box::new(Sphere::new(center, radius, material)))  world.rs:23-25, sphere.rs:16-26 */
int trt_world_add_sphere(trt_world *w, trt_vec3 center, float radius, uint32_t material);
/* The same for n spheres in array order - exactly the loop `for i in 0..n { world.add_geometry(Sphere::new(..)) }` (world.rs:23-25), one call
 * instead of n for scenes of millions of primitives.  center_radius: 4n floats (x, y, z, radius); material: n indices.  All or nothing:
 * an index out of range adds no sphere. */
int trt_world_add_spheres(trt_world *w, uint32_t n, const float *center_radius, const uint32_t *material);
/* World::add_geometry(Box::new(Quad::new(corner, u, v, material)))      world.rs:23-25, quad.rs:20-29 */
int trt_world_add_quad(trt_world *w, trt_vec3 corner, trt_vec3 u, trt_vec3 v, uint32_t material);
int trt_world_num_geometries(const trt_world *w);
int trt_world_num_materials(const trt_world *w);

/* ---- Scene: World::get_bvh() (world.rs:43-45 -> bvh.rs:12-22,42-84), flattened for the GPU ----
 * Host-only work (BVH build in the reference's median-split order, threading into a
 * pre-order skip-link array, packing into 16-byte planes).  Device upload happens lazily
 * on first render, so a scene can be compiled and inspected on a machine without a GPU. */
typedef struct trt_scene trt_scene;
int trt_scene_create(const trt_world *w, trt_scene **out);                          /* = trt_scene_create_ex(w, NULL, out) */
/* How a scene is compiled and how much idle device scratch its handle keeps.  PLACEMENT ONLY: every value renders the same
 * frames, bit for bit (the reference has one BVH layout and no such choice: bvh.rs:42-84).  Fill with
 * trt_scene_options_default() and change fields; NULL = the defaults. */
typedef struct {
    float cull_prune;             /* culling tree: an inner node whose box is >= this share of its nearest kept ancestor's is dropped (0.5) */
    int32_t flat_walk;            /* lock-step leaf list instead of a tree walk: -1 = for at most 32 primitives (default), 0 never, 1 always */
    int32_t compact_nodes;        /* 16-byte f16 culling nodes: -1 = for scenes too large for LDS (default), 0 never, 1 always */
    uint32_t top_nodes;           /* ignored since ABI 4 (rounds 1-4: upper tree levels of a large scene cached in LDS; slower in every form measured) */
    uint64_t scratch_cap_bytes;   /* idle scratch (workspaces + context frames) kept per device between renders; default 32 GiB */
    uint32_t reserved[6];         /* zero */
} trt_scene_options;
void trt_scene_options_default(trt_scene_options *out);
int trt_scene_create_ex(const trt_world *w, const trt_scene_options *options, trt_scene **out);
/* Same scene as trt_scene_create_ex(w, options, out), compiled on the calling thread's current device
 * (trt_set_device).  The packed scene, node dumps, info and launch plans are identical, byte for byte;
 * the scene is already resident on that device.  TRT_ERR_NO_DEVICE without a gfx950 device, TRT_ERR_OOM
 * if device scratch cannot be had (no silent fall-back to the host compiler). */
int trt_scene_create_on_device(const trt_world *w, const trt_scene_options *options, trt_scene **out);
/* Must not run while another host thread is inside a render call on this scene; renders enqueued with trt_render_device
 * that still run on the device are waited for. */
void trt_scene_destroy(trt_scene *s);
/* The scene handle caches device resources per device: the uploaded scene, render scratch ("workspaces": up to 8 per device,
 * each 12 bytes per pixel and sample of one launch: 3.2 GB for 64 spp at 2048x2048, at most 16 GB - trt_tuning.radiance_gb - for
 * renders of 256 spp and more; renders enqueued back to back on one stream share ONE) and, for the blocking entry points, contexts
 * (stream, events, counters, a device frame).
 * Idle scratch beyond 32 GiB per device (trt_scene_options.scratch_cap_bytes) is freed when a render ends; this call frees ALL idle
 * scratch now (whatever running renders own is skipped).  The uploaded scene stays. */
int trt_scene_trim(trt_scene *s);

typedef struct {
    uint32_t num_nodes, num_spheres, num_quads, num_materials;
    uint32_t max_depth;           /* BVH depth (root = 1) */
    uint32_t device_bytes;        /* size of the packed scene in HBM */
    uint32_t lds_bytes;           /* bytes the kernels stage into LDS (0 = traverses from global memory) */
    uint32_t num_cull_nodes;      /* nodes of the culling tree the kernels walk (same leaves, same order, fewer inner nodes) */
} trt_scene_info;
int trt_scene_get_info(const trt_scene *s, trt_scene_info *out);
/* Pre-order node dump of the REFERENCE tree (bvh.rs:42-84, node for node): bbox6[6*i..] = min.xyz,max.xyz;
 * prim[i] = geometry insertion index or -1 for an inner node; skip[i] = pre-order index of the next node
 * once subtree i is done. */
int trt_scene_get_nodes(const trt_scene *s, float *bbox6, int32_t *prim, int32_t *skip, uint32_t cap);
/* Same dump of the CULLING tree: another hierarchy over the reference tree's leaf sequence (identical leaf boxes
 * in identical order, inner boxes = exact unions), which gives bit-identical hits with fewer box tests. */
int trt_scene_get_cull_nodes(const trt_scene *s, float *bbox6, int32_t *prim, int32_t *skip, uint32_t cap);
/* Scenes too large for LDS also carry the culling tree as 16-byte nodes, boxes rounded OUTWARD to IEEE half precision
 * (one load per box step instead of two; postponed leaves are re-tested against their exact f32 boxes).  Copies
 * num_cull_nodes x 4 words: (lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16, link), link = skip index of an
 * inner node (the device copy keeps it as a byte offset, index x 16), or 0x80000000 | leaf sequence number.  Returns
 * TRT_ERR_NOT_FOUND if the scene has no such array. */
int trt_scene_get_compact_nodes(const trt_scene *s, uint32_t *words4, uint32_t cap);
/* Copies the packed scene (trt_scene_info.device_bytes bytes) as it is uploaded to a device.  TRT_ERR_INVALID_ARG if cap
 * (bytes) is smaller. */
int trt_scene_get_packed(const trt_scene *s, uint8_t *bytes, uint32_t cap);

/* ---- Camera (camera.rs:4-14, 17-56) ---- */
typedef struct {
    trt_vec3 position, viewport_upper_left, forward, horizontal, vertical;
    trt_vec3 defocus_disk_u, defocus_disk_v;
    uint32_t width, height;
} trt_camera;
/* Camera::new(focus_distance, defocus_angle[deg], position, look_at, up, vertical_fov[deg], width, height) */
int trt_camera_init(trt_camera *out, float focus_distance, float defocus_angle_deg, trt_vec3 position,
                    trt_vec3 look_at, trt_vec3 up, float vertical_fov_deg, uint32_t width, uint32_t height);

/* ---- Renderer (renderer/renderer.rs:12-35) ---- */
enum trt_backend {
    TRT_BACKEND_MEGAKERNEL = 0,   /* one persistent lane per pixel, whole bounce loop in one kernel */
    TRT_BACKEND_WAVEFRONT = 1,    /* workgroup-resident wavefront: path state SoA in HBM, ray queues in LDS,
                                     generate / extend / sort-by-material / shade as phases of one persistent kernel */
    TRT_BACKEND_AUTO = 2,         /* the fastest measured backend (currently TRT_BACKEND_STREAMED for every scene) */
    TRT_BACKEND_STREAMED = 3      /* samples as work items pulled by persistent waves; radiances folded per pixel in sample order */
};
/* Scheduling of a render.  EVERY field is scheduling or placement only: any value renders the same frame, bit for bit, with the
 * same ray count (each is covered by a bit-equality test).  The reference configures a render through constructor arguments
 * (renderer.rs:21-35), never through the environment; so does this library: fill with trt_tuning_default() - the built-in
 * defaults, overridden ONCE, when the library is loaded, by the TRT_* environment variables named below (for sweeps from a shell) -
 * change fields, and hand it over in trt_render_params.tuning (NULL = trt_tuning_default()).  Nothing on the launch path reads
 * the environment; two threads may render one scene with different tunings at the same time. */
typedef struct {
    uint32_t stream_waves_per_simd;   /* streamed backend: waves per SIMD grid and launch bound are sized for; 0 = by scene (6 for scenes
                                         in LDS, 7 for scenes in global memory that fit the 32 MiB of L2, 8 beyond); 5..8 (4 with dual_walk on a
                                         scene in global memory)                                            TRT_STREAM_MINW */
    uint32_t stream_big_threads;      /* lanes per workgroup for LDS scene copies above 20 KB: 0 = auto, 512, 768   TRT_BIG_THREADS */
    uint32_t stream_batch_spp;        /* samples per pixel in one work batch of a wave (8)                  TRT_STREAM_BATCH_SPP */
    uint32_t radiance_gb;             /* radiance records of one streamed launch, GiB (16; 1..64)           TRT_RADIANCE_GB */
    uint32_t leaf_slots;              /* postponed leaves per lane and walk; 0 = by launch plan             TRT_LEAF_SLOTS */
    uint32_t lds_leaf_stack;          /* where they live: 0 registers, 1 LDS where it costs no occupancy (default), 2 LDS always   TRT_LDS_LEAF_STACK */
    uint32_t ray_pool;                /* 1 (default): per-wave LDS pool of primary rays where it fits; 0: one ray in stock per lane   TRT_RAY_POOL */
    uint32_t stragglers;              /* 16-byte-node walk: lanes that may carry an unfinished walk into the next round (8; 0 = none)   TRT_STRAGGLERS */
    uint32_t lds_stragglers;          /* the same for the LDS tree walk (8)                                 TRT_LDS_STRAGGLERS */
    uint32_t dual_walk;               /* scenes in global memory: two paths per lane, two node loads in flight per wave: 0 = by scene (on where the
                                         scene's hot part exceeds the 32 MiB of L2), 1 = wherever the kernel exists, 2 = never   TRT_DUAL_WALK */
    uint32_t runtime_walk;            /* 1: the kernels that choose the walk at run time instead of the specialised ones (0)   TRT_RUNTIME_WALK */
    uint32_t xcd_remap;               /* 1: contiguous image regions per XCD (0: measured 2x slower)        TRT_XCD_REMAP */
    uint32_t mega_waves_per_simd;     /* megakernel backend: 0 = default (7)                                TRT_MINW */
    uint32_t mega_threads;            /* megakernel: lanes per workgroup, 0 = auto, 256, 512                TRT_MEGA_THREADS */
    uint32_t mega_global_waves8;      /* megakernel on scenes in global memory: 8 waves per SIMD (0)        TRT_MINW8 */
    uint32_t wf_waves_per_simd;       /* wavefront backend: 0 = default                                     TRT_WF_MINW */
    uint32_t wf_serve_min;            /* wavefront backend: lanes that must wait before a refill; 0 = default (12)   TRT_WF_SERVE_MIN */
    uint32_t reserved[7];             /* zero */
} trt_tuning;
void trt_tuning_default(trt_tuning *out);

typedef struct {
    uint32_t samples_per_pixel;   /* Renderer::samples_per_pixel: fixes the 1/spp scale (imager.rs:35) */
    uint32_t max_bounces;         /* Renderer::max_bounces */
    trt_vec3 background;          /* Renderer::background_color (None -> 0, renderer.rs:33) */
    uint32_t seed;                /* trt-rng v1 seed (the reference has no seed API: utils/random.rs:15-18) */
    uint32_t backend;             /* enum trt_backend */
    /* progressive / sharded rendering; zero-initialised = whole image, all samples */
    uint32_t sample_begin, sample_end;   /* render samples [begin,end) of 0..spp; end==0 means spp */
    uint32_t accumulate;                 /* 0: pixels start at 0; 1: continue the running sums in the buffer */
    /* image rows owned by this call: local row r (0..rows_local) is image row
     *   ((r / band_rows) * band_stride + band_offset) * band_rows + r % band_rows.
     * band_rows==0 means the identity map over all `height` rows. */
    uint32_t band_rows, band_stride, band_offset, rows_local;
    uint32_t collect_stats;       /* 0: count samples and rays only.  1: counting kernel variant walking the REFERENCE tree:
                                     node/primitive test counts equal the CPU path's (SURVEY §8d's algorithmic bytes).
                                     2: counting variant walking the culling tree: the box tests actually performed. */
    const trt_tuning *tuning;     /* scheduling knobs (see trt_tuning); NULL = trt_tuning_default().  Read during the call only. */
} trt_render_params;

typedef struct {
    uint64_t samples;             /* single_point_sampling calls */
    uint64_t rays;                /* closest-hit queries = world.hit calls (cpu.rs:48): the Mray/s unit */
    uint64_t node_tests;          /* AABB slab tests (bvh.rs:89); 0 unless collect_stats */
    uint64_t sphere_tests;        /* 0 unless collect_stats */
    uint64_t quad_plane_tests;    /* 0 unless collect_stats */
    uint64_t quad_inside_tests;   /* 0 unless collect_stats */
    uint64_t shades;              /* hits whose material was evaluated; 0 unless collect_stats */
    double kernel_ms;             /* device time of the launch(es), HIP events on the launch stream (host-buffer calls only) */
    uint64_t wave_trips[4];       /* diagnostics, collect_stats only: per-wave loop trips (bounce rounds, box-test steps,
                                     leaf phases, ray generations); lane-level counts / (64 x these) = SIMD utilisation */
    uint64_t gather_per_band;     /* trt_render_multi*: shards whose rows were gathered band by band instead of by one strided 2-D copy
                                     (no peer access between two devices, or the runtime refused the strided peer copy); else 0 */
} trt_stats;

/* Renderer::render(camera, world) (renderer.rs:37-79), synchronous.  `accum` is a HOST buffer
 * of rows*width*3 f32 linear running sums (Imager's `pixels`, imager.rs:43,50), rows =
 * rows_local or height.  Gamma/quantisation is not applied: see trt_tonemap_u8. */
int trt_render(trt_scene *s, const trt_camera *cam, const trt_render_params *p, float *accum, trt_stats *stats);

/* Renderer::render over several GPUs of one node: still ONE call that returns the whole frame (renderer.rs:37-79;
 * src/main.rs:19).  The scene is replicated, the image is cut into bands of 16 rows dealt round-robin over the shards
 * (band b -> shard b % ndev), one host thread per shard drives its device, and each shard's bands are copied straight to their
 * place in `accum` (HOST buffer, height*width*3 f32; read first when p->accumulate is set) with one strided 2-D copy
 * (trt_band_copy_plan).  The frame is bit-identical for
 * every ndev and equals trt_render's: the RNG is keyed by the image pixel and every pixel is folded in sample order.
 * `devices`: ndev device ordinals (a device may appear more than once: its shards then run concurrently on it), or NULL
 * for 0..ndev-1; ndev == 0 means every visible device.  p->band_rows must be 0.  stats (may be NULL): counters summed over
 * the shards, kernel_ms of the slowest one. */
int trt_render_multi(trt_scene *s, const trt_camera *cam, const trt_render_params *p, const int *devices, uint32_t ndev,
                     float *accum, trt_stats *stats);
/* The same with the frame gathered into HBM: `d_accum` is a buffer of height*width*3 f32 on devices[0] (device 0 when
 * `devices` is NULL); every shard sends its bands there with one strided 2-D device-to-device copy (xGMI between the GPUs of a node; staged
 * through the host per band where two devices have no peer access).
 * Synchronous: the frame is complete when the call returns. */
int trt_render_multi_device(trt_scene *s, const trt_camera *cam, const trt_render_params *p, const int *devices,
                            uint32_t ndev, float *d_accum, trt_stats *stats);
/* Rows of an image of `height` rows that shard `rank` of `ndev` owns under that band layout (host arithmetic only). */
int trt_band_rows_local(uint32_t height, uint32_t ndev, uint32_t rank, uint32_t *rows_local);
/* The gather of one shard as trt_render_multi[_device] performs it (host arithmetic only; bytes).  A shard keeps its rows
 * contiguous; in the frame its k-th band starts at row (k * ndev + rank) * 16, i.e. at a constant pitch: ONE strided 2-D copy
 * (`full_bands` rows of `band_bytes`, source pitch `local_pitch`, destination `frame_offset` + k * `frame_pitch`) moves all
 * full bands, one 1-D copy of `tail_bytes` the ragged last band if the shard owns it. */
typedef struct {
    uint32_t rows_local, full_bands, tail_rows, reserved;
    uint64_t band_bytes, local_pitch, frame_pitch, frame_offset;
    uint64_t tail_bytes, tail_local_offset, tail_frame_offset;
} trt_band_copy;
int trt_band_copy_plan(uint32_t width, uint32_t height, uint32_t ndev, uint32_t rank, trt_band_copy *out);

/* Same, on buffers already resident in HBM.  `d_accum`: device pointer, rows*width*3 f32.
 * `d_counters`: device pointer to 16 uint64 (zeroed by the caller; [0..6] = trt_stats' first seven
 * fields, [8..11] = wave_trips, [12..15] with collect_stats: `shades` by material kind in enum trt_material_kind order) or NULL.  `stream`: a hipStream_t (NULL = default stream).  Asynchronous: returns after
 * enqueueing; the caller synchronises the stream.
 *
 * Concurrency (all render entry points): a scene is immutable once created and may be rendered by several host threads
 * and on several streams at the same time; every render takes private device scratch from a pool on the scene handle
 * (at most 8 scratch buffers per device: further concurrent renders queue behind running ones on the device).
 * trt_scene_destroy must not run while a host thread is inside a render call of that scene. */
int trt_render_device(trt_scene *s, const trt_camera *cam, const trt_render_params *p, float *d_accum,
                      uint64_t *d_counters, void *stream);

/* ---- The frame with its per-pixel second moments, and the variance of the pixel estimate ----
 * trt_render / trt_render_device that also write `moment2` (rows*width*3 f32, the frame's layout): where the frame folds
 *   accum.ch = accum.ch + c_s.ch * inv_spp                      (imager.rs:35,50; inv_spp = 1 / samples_per_pixel)
 * over the samples s of a pixel in order, the same pass also folds
 *   moment2.ch = moment2.ch + (c_s.ch * c_s.ch) * inv_spp
 * per channel; each operator is one IEEE f32 operation, nothing is fused.  `accum` is bit-identical to what trt_render /
 * trt_render_device write for the same arguments.  Bands, sample_begin / sample_end and accumulate behave for `moment2` exactly as
 * for the frame: with samples_per_pixel equal, the result does not depend on how the sample range is split over calls.  Nothing to
 * trace (no rows, an empty sample range, max_bounces == 0): both buffers are zeroed unless accumulate.  collect_stats and tuning as in
 * trt_render.
 * Only the streamed backend keeps per-sample records: p->backend must be TRT_BACKEND_STREAMED or TRT_BACKEND_AUTO.  Any other backend,
 * or a NULL `moment2`, is TRT_ERR_INVALID_ARG before any device work.  Several GPUs: shard with the band fields; there is no multi form.
 * trt_render_moments: HOST buffers, synchronous (the second device frame is allocated for the call and freed before it returns).
 * trt_render_moments_device: buffers in HBM, asynchronous on `stream`, as trt_render_device. */
int trt_render_moments(trt_scene *s, const trt_camera *cam, const trt_render_params *p, float *accum, float *moment2, trt_stats *stats);
int trt_render_moments_device(trt_scene *s, const trt_camera *cam, const trt_render_params *p, float *d_accum, float *d_moment2,
                              uint64_t *d_counters, void *stream);
/* Variance of the pixel estimate, 1 f32 per pixel: the trace over the channels of the unbiased variance of the mean.  With S = accum
 * (the mean of the N = samples_per_pixel samples) and M = moment2 (the mean of their squares), all f32, one IEEE operation per operator:
 *   per channel  d = M - S*S;  d = d > 0 ? d : 0          (a NaN becomes 0)
 *   variance = ((d.r + d.g) + d.b) * (1.0f / float(N - 1))
 * N <= 1 writes +inf: unknown.  M - S*S cancels: its error is about 2^-23 * M relative to M (M is at most 225 for the light of 15 in
 * the Cornell box, so about 3e-5 absolute), which matters only where the variance is that small anyway - and is the reason for the clamp:
 * a constant pixel may give a tiny negative d.  The square root of a channel's share is the standard error of that pixel.
 * trt_variance: HOST buffers, synchronous (uploads, runs the device kernel, downloads; there is no CPU path).  trt_variance_device:
 * buffers in HBM on the calling thread's current device, asynchronous on `stream`.  A NULL buffer with npixels > 0 is
 * TRT_ERR_INVALID_ARG before any device work; npixels == 0 succeeds and touches nothing, with or without a device. */
int trt_variance(const float *accum, const float *moment2, uint32_t npixels, uint32_t samples_per_pixel, float *variance);
int trt_variance_device(const float *d_accum, const float *d_moment2, uint32_t npixels, uint32_t samples_per_pixel, float *d_variance,
                        void *stream);

/* The literal Sampler plug-in form (sampler/mod.rs:10-17): n SamplePoints in, n SampledColors
 * out, HOST buffers.  Point i uses RNG stream (seed, pixel=i, sample=0).  With `stats` non-NULL the counting kernel runs
 * (reference-order walk of the reference tree: its counters equal the CPU path's); with NULL the production walk. */
int trt_sample_batch(trt_scene *s, const trt_sample_point *in, uint32_t n, trt_sampled_color *out,
                     uint32_t max_bounces, trt_vec3 background, uint32_t seed, trt_stats *stats);

/* ---- Ray queries: BVH::hit (hittable/bvh.rs:24-27,88-107) for caller-supplied rays ----
 * What does ray i hit, and is the segment blocked: picking, visibility between two points, occlusion and shadow probes, depth / normal /
 * material buffers, collision probes.  No shading, no random numbers.
 *  - Query.  Ray i is queried over [0.001, t_max[i]); t_max == NULL means +inf for every ray.  The lower end is the reference's own
 *    constant (renderer/sampler/cpu.rs:48) and is compiled into every walk: a caller-supplied t_min is NOT offered.
 *  - The ray is used as given: the direction is not normalised (trt_ray is the POD, not Ray::new, ray.rs:12-14), and t counts in units
 *    of the direction's length.
 *  - Exactness.  The answer is BVH::hit's, bit for bit: the same primitive, the same t, the same HitRecord (hittable/mod.rs:28-48) as the
 *    reference returns for Range { 0.001..t_max }.  That includes the part the leaf BOXES play: a primitive is tested only where the ray
 *    passes its box in the current interval, so the answer can differ from a brute-force loop over the primitives.
 *  - A ray with a NaN component hits nothing.  A ray whose t_max is not > 0.001 (NaN included) is a miss and is not walked.
 *  - trt_occluded: occluded[i] is 1 if trt_intersect reports a hit for the same ray and t_max, else 0.  It does not pay for the closest
 *    hit: its walk ends at the first primitive accepted (a prefix of trt_intersect's walk, hence exact: DESIGN.md 6).
 *  - Order and coherence.  Answer i belongs to ray i.  A wave of the GPU works through a contiguous run of the caller's rays; nothing is
 *    sorted, so neighbouring rays that travel together (image order, not a random permutation) are the caller's to arrange.
 *  - Errors.  A NULL scene, or a NULL buffer with n > 0, is TRT_ERR_INVALID_ARG before any device work; then TRT_ERR_NO_DEVICE, as in
 *    trt_sample_batch.  n == 0 then succeeds and touches nothing.
 *  - Concurrency: as for the render entry points.  The scene is immutable; several threads and streams may query and render it at once. */
typedef struct {
    float t;                      /* +inf on a miss */
    uint32_t geometry;            /* insertion index of the primitive (order of the trt_world_add_* calls); 0xFFFFFFFF on a miss */
    uint32_t material;            /* index into the world's material table; 0xFFFFFFFF on a miss */
    uint32_t front_face;          /* HitRecord::front_face (hittable/mod.rs:35); 0 on a miss */
    trt_vec3 normal;              /* HitRecord::normal (mod.rs:36-40): unit, facing the ray; 0,0,0 on a miss */
} trt_hit;                        /* 28 B */
/* HOST buffers, synchronous: n rays (and n t_max, or NULL) in, n records / n bytes out. */
int trt_intersect(trt_scene *s, const trt_ray *rays, const float *t_max, uint32_t n, trt_hit *hits);
int trt_occluded(trt_scene *s, const trt_ray *rays, const float *t_max, uint32_t n, uint8_t *occluded);
/* The same on buffers resident in HBM, on the calling thread's current device (trt_set_device), asynchronous on `stream` (a hipStream_t,
 * NULL = default): returns after enqueueing; the caller synchronises the stream. */
int trt_intersect_device(trt_scene *s, const trt_ray *d_rays, const float *d_t_max, uint32_t n, trt_hit *d_hits, void *stream);
int trt_occluded_device(trt_scene *s, const trt_ray *d_rays, const float *d_t_max, uint32_t n, uint8_t *d_occluded, void *stream);

/* How a query batch of n rays is launched on this scene (host arithmetic only, the one copy of the rule: the four entry points above take
 * their numbers from it).  The kernel follows the streamed launch plan of the scene under the built-in tuning (streamed_walk,
 * streamed_threads); a plan without a query instantiation runs the register-slot walk instead (fallback = 1).  A wave owns rays_per_wave
 * consecutive rays: 256, or more - a multiple of 64 - once ceil(n / 256) exceeds wave_slots = 4 x compute_units x workgroups_per_cu x
 * waves per workgroup.  compute_units == 0: the count of the calling thread's current device (TRT_ERR_NO_DEVICE without one); any other
 * value needs no device, so the invariants can be checked for every scene, option and batch size without a GPU (tests/test_query_abi.py). */
typedef struct {
    uint32_t scene_mode;              /* 0 scene read from global memory, 1 whole hot scene copied into LDS */
    uint32_t walk;                    /* numbered as trt_launch_plan.walk: 1 LDS tree, 2 lock-step list, 3 16-byte nodes, 5 register slots */
    uint32_t threads_per_workgroup, kernel_waves_per_simd, workgroups_per_cu;
    uint32_t leaf_slots, stragglers;  /* LDS leaf-stack depth per lane (0: register slots); lanes that may carry a walk into the next round */
    uint32_t lds_bytes, scene_lds_bytes;      /* dynamic LDS per workgroup; the scene copy's share */
    uint32_t has_kernel;              /* 0 would be a bug: the launch then fails */
    uint32_t fallback;                /* 1: the streamed plan has no query instantiation, the register-slot walk answers */
    uint32_t streamed_walk, streamed_threads; /* the streamed launch plan's walk and workgroup shape for this scene */
    uint32_t compute_units;           /* as given, or the current device's */
    uint32_t rays_per_wave;           /* wave w owns rays [w * rays_per_wave, ...) */
    uint32_t workgroups;              /* the grid: ceil(waves / (threads_per_workgroup / 64)); 0 for n == 0 (nothing is launched) */
    uint64_t wave_slots, waves;
} trt_query_plan;
int trt_query_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- The camera's own rays: primary-ray export and first-hit feature buffers (AOVs) ----
 * Primary rays.  Entry (r, x) of `rays` - row-major, rows x width, rows = p->rows_local, or height when p->band_rows == 0 - is the ray the
 * render entry points trace for sample s of image pixel (x, image row of local row r): RNG stream (p->seed, pixel y * width + x,
 * sample s), then SamplePointGenerator::generate (pointgen.rs:41-43) and Camera::get_ray (camera.rs:58-66), normalised by Ray::new.
 * Handed to trt_intersect it gives that sample's first hit.  Of `p` only seed, samples_per_pixel (s must be below it) and the band
 * fields are read.  trt_primary_rays: HOST buffer, synchronous.  trt_primary_rays_device: buffer in HBM on the calling thread's current
 * device, asynchronous on `stream`.  Errors: TRT_ERR_INVALID_ARG (a NULL pointer, s >= samples_per_pixel, bad bands) before any device
 * work, then TRT_ERR_NO_DEVICE: the rays are made by the device code that renders, there is no CPU path. */
int trt_primary_rays(const trt_camera *cam, const trt_render_params *p, uint32_t s, trt_ray *rays);
int trt_primary_rays_device(const trt_camera *cam, const trt_render_params *p, uint32_t s, trt_ray *d_rays, void *stream);

/* Feature buffers of a frame: what the first hit of every camera ray says, folded per pixel over the samples - the guides a denoiser
 * takes, an alpha matte, a picking buffer.  "First hit of sample s" is BVH::hit over [0.001, +inf) for the primary ray above: bit for bit
 * the trt_hit record trt_intersect gives for that ray (a ray with a NaN component hits nothing).  Each pointer may be NULL (not wanted);
 * all six NULL is TRT_ERR_INVALID_ARG.  Every buffer holds rows x width pixels, row-major, rows as above.
 *  - Sums run in sample order with the imager's rule, acc = acc + value * (1 / samples_per_pixel) (imager.rs:35,50): with
 *    samples_per_pixel equal, the result does not depend on how [sample_begin, sample_end) is split over calls.  p->accumulate as in
 *    trt_render: 0 starts the sums at 0, 1 continues the ones in the buffers.  The two index buffers are written only by a call whose
 *    sample range contains sample 0.
 *  - Bands (band_rows, band_stride, band_offset, rows_local) as in trt_render.
 *  - max_bounces, backend, collect_stats and tuning are ignored.
 * One kernel makes the ray, walks and folds; neither rays nor hit records go through memory.  trt_render_aov: HOST buffers, synchronous.
 * trt_render_aov_device: buffers in HBM (the struct itself is read on the host, during the call), asynchronous on `stream`.  Errors and
 * concurrency as for the ray queries: TRT_ERR_INVALID_ARG before any device work, then TRT_ERR_NO_DEVICE. */
typedef struct {
    float *albedo;                /* 3 f32 per pixel: sum of a_s / spp; a_s = albedo of the first hit's material (the emitted colour for TRT_LIGHT), p->background on a miss */
    float *normal;                /* 3 f32: sum of n_s / spp; n_s = trt_hit.normal of the first hit (unit, facing the ray), 0 on a miss; not renormalised */
    float *depth;                 /* f32: sum of t_s / spp over the samples that hit; a miss adds nothing */
    float *coverage;              /* f32: sum of hit_s / spp: the alpha of the geometry */
    uint32_t *geometry;           /* insertion index of the first hit of sample 0; 0xFFFFFFFF on a miss */
    uint32_t *material;           /* material index of the first hit of sample 0; 0xFFFFFFFF on a miss */
} trt_aov_buffers;                /* 48 B */
int trt_render_aov(trt_scene *s, const trt_camera *cam, const trt_render_params *p, const trt_aov_buffers *buffers);
int trt_render_aov_device(trt_scene *s, const trt_camera *cam, const trt_render_params *p, const trt_aov_buffers *d_buffers, void *stream);
/* How trt_render_aov[_device] launches a local image of n_pixels on this scene: trt_query_launch_plan's rule and fields with pixels in
 * place of rays (rays_per_wave = pixels a wave owns, each for all of its samples), over the feature-buffer kernels' own table. */
int trt_aov_launch_plan(const trt_scene *s, uint32_t n_pixels, uint32_t compute_units, trt_query_plan *out);

/* ---- Sparse rendering of chosen pixels, and the selection of the pixels that are still too noisy ----
 * Every render entry point above traces all pixels of its rows; the band fields cut rows, never columns.  trt_render_pixels traces a
 * LIST: `pixels` holds n local pixel indices r * width + x over the rows the call owns (rows = p->rows_local, or height when
 * p->band_rows == 0).  Re-render a screen region, refine what a user looks at, finish the neighbourhood of a firefly - or sample
 * adaptively: render a few samples everywhere, then loop over trt_select_pixels and trt_render_pixels.
 * Contract: after the call the bytes of every listed pixel in `accum` (and in `moment2`, which may be NULL: not wanted) are what
 * trt_render_moments_device leaves there for the same `p` - sample range, accumulate, band fields, seed, background, max_bounces - and
 * the same prior contents.  That includes "nothing to trace" (an empty sample range, max_bounces == 0): the listed pixels are zeroed
 * unless accumulate.  Every other byte of both buffers is untouched, also with accumulate == 0.  The fold is the imager's own sequence
 * of f32 additions in sample order, so with samples_per_pixel equal a pixel refined later is bit-identical to the same pixel of a
 * full render of the same samples.  `backend` and `tuning` are ignored, as in trt_render_aov; collect_stats must be 0
 * (TRT_ERR_INVALID_ARG otherwise: there are no counting kernels); stats / d_counters receive samples and rays ([0] and [1]) only.
 * One kernel of its own (a lane owns a pixel for all samples of the call and folds in registers); none of the render kernels takes part.
 * A wave works through a contiguous run of the list, so neighbouring entries that are neighbouring pixels travel together.
 * trt_render_pixels: HOST buffers (`accum`, `moment2`: whole local frames, rows * width * 3 f32), synchronous.  The list is validated
 *   before any device work: an index >= rows * width, or one listed twice, is TRT_ERR_INVALID_ARG.  A NULL scene, camera or params, or
 *   a NULL list or `accum` with n > 0, is TRT_ERR_INVALID_ARG; then TRT_ERR_NO_DEVICE.  n == 0 succeeds and touches nothing.
 * trt_render_pixels_device: buffers in HBM on the calling thread's current device, asynchronous on `stream`.  The list is NOT validated:
 *   an entry >= rows * width is skipped (neither read nor written); duplicate indices are the caller's error - that pixel's value is
 *   unspecified, nothing else is affected.  With `d_count` non-NULL the kernel uses the first min(*d_count, n) entries - the count
 *   trt_select_pixels_device wrote earlier on the same stream - and n only sizes the launch.  `d_counters`: 16 uint64 as in
 *   trt_render_device, or NULL. */
int trt_render_pixels(trt_scene *s, const trt_camera *cam, const trt_render_params *p, const uint32_t *pixels, uint32_t n,
                      float *accum, float *moment2, trt_stats *stats);
int trt_render_pixels_device(trt_scene *s, const trt_camera *cam, const trt_render_params *p, const uint32_t *d_pixels, uint32_t n,
                             const uint32_t *d_count, float *d_accum, float *d_moment2, uint64_t *d_counters, void *stream);
/* How trt_render_pixels[_device] launches a list of n pixels on this scene: trt_query_launch_plan's rule and fields with list entries in
 * place of rays (rays_per_wave = entries a wave owns, each for all samples of the call), over the sparse render kernels' own table. */
int trt_pixels_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* Selection: from a candidate list, the pixels whose estimate is still too noisy, in candidate order (stable; a deterministic scan, the
 * same output on every run).  `accum` = S and `moment2` = M are the running sums as trt_render_moments leaves them after samples_done = n
 * of N = samples_per_pixel samples (both carry the frame's fixed 1 / N scale); n is the same for every candidate.  `candidates` holds
 * n_candidates pixel indices, or is NULL: candidate i is pixel i.  On the host, once: k = float(N) / float(n), inv = 1.0f / float(n - 1),
 * rel2 = rel_tol * rel_tol, abs2 = abs_tol * abs_tol.  Per candidate, all f32, one IEEE operation per operator, nothing fused:
 *   per channel: s = S.ch * k;  q = M.ch * k;  d = q - s*s;  d = d > 0 ? d : 0
 *   v = ((d.r + d.g) + d.b) * inv                    (the variance of the mean after n samples, as trt_variance defines it)
 *   l = (s.r + s.g) + s.b;  b = rel2 * (l*l);  b = b + abs2
 *   keep = v > b                                     (a NaN on either side: not kept)
 * n <= 1 keeps every candidate: the variance is unknown.  A candidate index >= npixels is not kept and is not read.  `selected` has
 * room for n_candidates indices; the first *count are written.
 * trt_select_pixels: HOST buffers, synchronous.  trt_select_pixels_device: buffers in HBM, asynchronous on `stream`; allocates nothing:
 * `d_scratch` holds at least trt_select_scratch_bytes(n_candidates) bytes (host arithmetic only; 4-byte aligned).
 * Aliasing: the HOST form works on device copies of its own, so `selected` may be `candidates` (a list shrunk in place).  The DEVICE form
 * must not select in place: a workgroup writes d_selected[k] while others still read d_candidates[i], and although k <= i the slot k may
 * be a candidate of an earlier tile that has not been read yet.  [d_candidates, d_candidates + 4 n_candidates) and [d_selected,
 * d_selected + 4 n_candidates) must not overlap (TRT_ERR_INVALID_ARG; adjacent ranges are fine): keep two lists and swap them.
 * Errors: TRT_ERR_INVALID_ARG before any device work - a NULL count, samples_per_pixel == 0, samples_done > samples_per_pixel, with
 * n_candidates > 0 a NULL `accum`, `moment2` or `selected`, for the device form a NULL or too small scratch or a `d_selected` that
 * overlaps `d_candidates` - then TRT_ERR_NO_DEVICE.
 * n_candidates == 0 succeeds, writes count 0 and touches nothing else, with or without a device (without one the device form has no
 * buffer to write and writes nothing). */
int trt_select_pixels(const float *accum, const float *moment2, uint32_t npixels, uint32_t samples_per_pixel, uint32_t samples_done,
                      const uint32_t *candidates, uint32_t n_candidates, float rel_tol, float abs_tol, uint32_t *selected, uint32_t *count);
int trt_select_pixels_device(const float *d_accum, const float *d_moment2, uint32_t npixels, uint32_t samples_per_pixel,
                             uint32_t samples_done, const uint32_t *d_candidates, uint32_t n_candidates, float rel_tol, float abs_tol,
                             uint32_t *d_selected, uint32_t *d_count, void *d_scratch, uint64_t scratch_bytes, void *stream);
uint64_t trt_select_scratch_bytes(uint32_t n_candidates);

/* ---- Radiance queries: path tracing of caller-supplied rays ----
 * The ray queries answer "what does this ray hit" for any ray; these answer "what light arrives along it": another camera (panorama,
 * fisheye, orthographic, a lens model of the caller's own), a sensor that is no image, a probe along one fixed direction (K samples of
 * one ray differ only after the first hit: texels and probes, which need K different first rays, are trt_gather's below), or the
 * render's own rays (trt_primary_rays) traced again with more samples.
 *  - Path.  For ray i and sample s of 0..K, K = samples_per_ray, the colour c is CpuSampler::single_point_sampling (cpu.rs:39-65) for
 *    ray i AS GIVEN: the direction is not normalised, as in trt_intersect and trt_sample_batch.
 *  - RNG stream (seed, pixel = first_stream + i * K + s, sample = 0); no primary-ray draws are consumed.  This is trt_sample_batch's own
 *    numbering (point j uses stream (seed, j, 0)) opened by an offset, and that is the reason for it: with K == 1 and first_stream == 0
 *    radiance[i] is trt_sample_batch's out[i].color bit for bit, and every sample of any call can be checked against that entry point
 *    (and the oracle's restatement of it) on a list with each ray repeated K times.
 *  - Fold: the imager's own, per ray, in sample order, all f32, one IEEE operation per operator, nothing fused:
 *      radiance.ch = radiance.ch + c.ch * inv_K;   moment2.ch = moment2.ch + (c.ch * c.ch) * inv_K;   inv_K = 1.0f / float(K)
 *    `radiance` and `moment2` hold n x 3 f32; `moment2` may be NULL (not wanted).  trt_variance(radiance, moment2, n, K, ...) is then
 *    the variance of each ray's estimate, and the pair feeds trt_select_pixels and the denoiser as a frame and its moments do.
 *  - samples [sample_begin, sample_end) of 0..K are traced; sample_end == 0 means K.  accumulate == 0 starts the sums at 0, 1 continues
 *    the ones in the buffers.  K fixes the 1 / K scale whatever the range, as samples_per_pixel does for a frame.
 *  - Split invariance.  By samples: with K equal, [0, a) and then [a, K) with accumulate == 1 leave the bytes of one pass over [0, K).
 *    By rays: rays [0, a) in one call and rays [a, n) in another with first_stream + a * K leave the bytes of one call over [0, n).
 *  - Nothing to trace (an empty sample range, max_bounces == 0): the n entries are zeroed unless accumulate.  No byte outside [0, 12 n)
 *    of either buffer is ever written.
 *  - A ray with a NaN component hits nothing (the rule of the ray queries): its samples are `background`.
 *  - stats / d_counters receive samples ([0]) and rays ([1]) only: there are no counting kernels.  `rays` counts the reference's
 *    world.hit calls for these samples (cpu.rs:48) - what trt_sample_batch reports for the repeated list - whatever the kernel shares
 *    between the samples of a ray (in most kernel shapes the closest hit of the caller's ray is found once per ray and call).  kernel_ms as in
 *    trt_render_pixels.  `d_counters`: 16 uint64 as in trt_render_device, added to, or NULL.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL scene or params; with n > 0 a NULL `rays` or `radiance`;
 *    samples_per_ray == 0; sample_begin > sample_end or sample_end > K (after the end == 0 rule); a non-zero reserved word;
 *    first_stream + n * K > 2^32 (computed in 64 bits: the stream index must not wrap).  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the
 *    host form's buffers.  n == 0 succeeds and touches nothing, with or without a device.
 * trt_radiance: HOST buffers, synchronous; one device allocation for the call; the running sums are uploaded only when accumulate is set.
 * trt_radiance_device: buffers in HBM on the calling thread's current device, asynchronous on `stream`; allocates nothing.
 * Order, coherence and concurrency as for the ray queries: a wave works through a contiguous run of the caller's rays, each for all
 * samples of the call; nothing is sorted. */
typedef struct {
    uint32_t samples_per_ray;     /* K >= 1: fixes the 1/K scale, as samples_per_pixel does for a frame */
    uint32_t max_bounces;
    trt_vec3 background;
    uint32_t seed;
    uint32_t sample_begin, sample_end;   /* samples [begin,end) of 0..K; end == 0 means K */
    uint32_t accumulate;          /* 0: sums start at 0; 1: continue the sums in the buffers */
    uint32_t first_stream;        /* RNG stream of sample 0 of ray 0 */
    uint32_t reserved[6];         /* zero */
} trt_radiance_params;            /* 64 B */
void trt_radiance_params_default(trt_radiance_params *out);   /* K 1, max_bounces 50, background 0, seed 1, rest 0 */
int trt_radiance(trt_scene *s, const trt_ray *rays, uint32_t n, const trt_radiance_params *p, float *radiance, float *moment2,
                 trt_stats *stats);
int trt_radiance_device(trt_scene *s, const trt_ray *d_rays, uint32_t n, const trt_radiance_params *p, float *d_radiance,
                        float *d_moment2, uint64_t *d_counters, void *stream);
/* How trt_radiance[_device] launches n rays on this scene: trt_query_launch_plan's rule and fields (rays_per_wave = rays a wave owns, each
 * for all samples of the call), over the radiance kernels' own table. */
int trt_radiance_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Gather queries: radiance queries whose rays the device draws about caller-supplied surfels ----
 * trt_radiance traces the SAME ray K times; a lightmap texel, an irradiance probe or a glossy gather needs K DIFFERENT first rays about
 * a surface normal.  A gather query draws them on the device with one of the reference's two scatter rules, then traces and folds per
 * item exactly as trt_radiance does: nothing per sample crosses the bus.  With the cosine lobe the result is the radiance a white
 * Lambertian surface at the point would reflect (irradiance / pi: what a lightmap bakes); with the cone lobe a glossy or soft gather,
 * and with a small spread the direction jitter that anti-aliases a camera of the caller's own.
 *  - Item i is (origin = point, direction = axis), both used AS GIVEN: the axis is not normalised.
 *  - First ray.  For sample s of 0..K, K = path.samples_per_ray, the stream index is j = path.first_stream + i * K + s (32 bits).  With
 *    g = RNG (seed, pixel = j, sample = 1) and v = random_in_unit_sphere(g) (vec3extend.rs:15-30; three draws, nothing else is taken from g):
 *      TRT_LOBE_COSINE, Lambertian::scatter (lambertian.rs:16-22):  dir = axis + normalize(v); if near_zero(dir) then dir = axis
 *      TRT_LOBE_CONE, Metal::scatter with the axis as the mirror direction (metal.rs:18-25):  dir = axis + spread * v
 *    and the ray is Ray::new(point, dir), which normalises dir.  `spread` is Metal's fuzz, not clamped; the cosine lobe ignores it.
 *  - Path.  The sample's colour is CpuSampler::single_point_sampling (cpu.rs:39-65) for that ray with RNG (seed, j, 0) and the budget
 *    max_bounces - what trt_radiance and trt_sample_batch do for stream j; the surfel is not a bounce.  Both streams start fresh, so the
 *    draw can be restated with the reference's scatter functions and the path with trt_sample_batch, sample by sample.
 *  - Fold, second moments, sample range, accumulate, split invariance by samples and by items (first_stream + a * K), "nothing to trace",
 *    the output bounds [0, 12 n), stats / d_counters (samples and rays only; `rays` counts the reference's world.hit calls), kernel_ms,
 *    order, coherence and concurrency: as in trt_radiance.
 *  - A first ray with a NaN component hits nothing: its sample is `background`.  That includes a NaN or infinite axis or point, and a
 *    draw with u3 == 0 under the cosine lobe, where the reference normalises a zero vector.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL params; trt_radiance's own errors, applied to `path`; `lobe` not 1 or 2;
 *    with TRT_LOBE_CONE a `spread` that is NaN, infinite or negative; a non-zero reserved word.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM
 *    for the host form's buffers.  n == 0 succeeds and touches nothing, with or without a device.
 * trt_gather: HOST buffers, synchronous, as trt_radiance.  trt_gather_device: buffers in HBM, asynchronous on `stream`; allocates nothing. */
enum trt_lobe { TRT_LOBE_COSINE = 1, TRT_LOBE_CONE = 2 };
typedef struct {
    trt_radiance_params path;     /* every field as in trt_radiance, same rules, same errors; K = path.samples_per_ray */
    uint32_t lobe;                /* enum trt_lobe */
    float spread;                 /* CONE: radius of the sphere added to the axis (Metal's fuzz, not clamped); COSINE: ignored */
    uint32_t reserved[6];         /* zero */
} trt_gather_params;              /* 96 B */
void trt_gather_params_default(trt_gather_params *out);   /* path = trt_radiance_params_default, lobe COSINE, spread 0 */
int trt_gather(trt_scene *s, const trt_ray *items, uint32_t n, const trt_gather_params *p, float *radiance, float *moment2,
               trt_stats *stats);
int trt_gather_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_gather_params *p, float *d_radiance,
                      float *d_moment2, uint64_t *d_counters, void *stream);
/* How trt_gather[_device] launches n items on this scene: trt_radiance_launch_plan's rule and fields over the gather kernels' own table
 * (the same shapes; kernel_waves_per_simd is that table's bound). */
int trt_gather_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Ambient queries: how open is the lobe about a surfel, and towards where ----
 * Before "what light arrives here" (trt_gather) a baker or a probe system asks "how much of the hemisphere is open": ambient occlusion,
 * sky visibility, and the bent normal - the mean unoccluded direction.  An ambient query draws trt_gather's first rays on the device and
 * asks trt_occluded's question of each: nothing per sample crosses the bus, no closest hit is searched and nothing is shaded.
 *  - Item i is a surfel (origin = point, direction = axis), both used AS GIVEN, as in trt_gather.
 *  - First ray.  For sample s of 0..K, K = gather.path.samples_per_ray, the stream index is j = gather.path.first_stream + i * K + s, and
 *    the ray is trt_gather's first ray for the same `gather` parameters, bit for bit: three draws from RNG (seed, pixel = j, sample = 1),
 *    the cosine or the cone rule, Ray::new - which normalises, so the direction d below is a unit vector.  Stream (seed, j, 0) is not
 *    touched: there is no path.  gather.path.max_bounces and gather.path.background are not read.
 *  - Sample.  o = 1 if BVH::hit (hittable/bvh.rs:24-27,88-107) over [0.001, max_distance) finds anything for that ray, else 0: exactly
 *    what trt_occluded answers for it with t_max = max_distance.  Every material occludes, lights and glass included.  A first ray with a
 *    NaN component hits nothing (the rule of the ray queries).  If max_distance is not > 0.001 the range is empty: nothing is walked and
 *    every sample is unoccluded.  max_distance = +inf asks for sky visibility.
 *  - Fold, per item, in sample order, all f32, one IEEE operation per operator, nothing fused; inv_K = 1.0f / float(K).  An unoccluded
 *    sample adds
 *      visibility = visibility + inv_K;   bent.ch = bent.ch + d.ch * inv_K
 *    and an occluded sample adds nothing (it does not add 0).  `visibility` holds n f32 and is required; `bent` holds n x 3 f32 and may
 *    be NULL (not wanted; `visibility` is the same either way).  `bent` is not renormalised: its direction is the bent normal, its length
 *    says how one-sided the opening is.  With the cosine lobe 1 - visibility is cosine-weighted ambient occlusion.
 *  - Sample range, accumulate, the 1 / K scale fixed by K, and split invariance by samples (split the range, set accumulate) and by items
 *    (first_stream + a * K): as in trt_radiance.  An empty sample range zeroes the n entries unless accumulate, which touches nothing;
 *    max_bounces == 0 is NOT "nothing to trace" here.  No byte outside [0, 4 n) of `visibility` or [0, 12 n) of `bent` is ever written.
 *  - stats / d_counters receive samples ([0]) and rays ([1]) only.  `rays` is the number of occlusion walks: one per traced sample when
 *    max_distance > 0.001, else 0.  kernel_ms as in trt_radiance.  `d_counters`: 16 uint64 as in trt_render_device, added to, or NULL.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL scene or params; with n > 0 a NULL `items` or `visibility`; every error
 *    trt_gather reports for `gather` (K == 0, a bad sample range, first_stream + n * K > 2^32, a bad lobe or spread, a non-zero reserved
 *    word); a NaN max_distance; a non-zero reserved word of this struct.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the host form's
 *    buffers.  n == 0 succeeds and touches nothing, with or without a device.
 * trt_ambient: HOST buffers, synchronous; one device allocation for the call; the sums are uploaded only when accumulate is set.
 * trt_ambient_device: buffers in HBM on the calling thread's current device, asynchronous on `stream`; allocates nothing.
 * Order, coherence and concurrency as in trt_gather: a wave works through a contiguous run of the items, each for all samples of the
 * call.  The launch rule gives a wave 256 items whatever K is, as it does for trt_radiance and trt_gather. */
typedef struct {
    trt_gather_params gather;     /* lobe, spread and, of gather.path: samples_per_ray (K), seed, sample_begin, sample_end, accumulate,
                                     first_stream - same rules, same errors as trt_gather.  gather.path.max_bounces and
                                     gather.path.background are IGNORED (not read, not validated): there is no path. */
    float max_distance;           /* occluders count in [0.001, max_distance) along the unit first ray; +inf: sky visibility */
    uint32_t reserved[7];         /* zero */
} trt_ambient_params;             /* 128 B: offsets 0, 96, 100 */
void trt_ambient_params_default(trt_ambient_params *out);   /* gather = trt_gather_params_default, max_distance = +inf, rest 0; NULL tolerated */
int trt_ambient(trt_scene *s, const trt_ray *items, uint32_t n, const trt_ambient_params *p, float *visibility, float *bent,
                trt_stats *stats);
int trt_ambient_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_ambient_params *p, float *d_visibility, float *d_bent,
                       uint64_t *d_counters, void *stream);
/* How trt_ambient[_device] launches n items on this scene: trt_query_launch_plan's rule and fields over the ambient kernels' own table
 * (the same shapes; kernel_waves_per_simd is that table's bound). */
int trt_ambient_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Probe queries: the radiance arriving at a point as a function of direction, in spherical harmonics ----
 * trt_gather returns ONE colour per (point, axis): a lightmap texel.  A light probe, or a directional lightmap texel, stores the incoming
 * radiance as a function of direction, so that a dynamic object or a normal-mapped surface can be lit from it afterwards.  A probe query
 * draws K first rays uniformly over the sphere (or the hemisphere about the axis) on the device, traces each as trt_gather does, and folds
 * the colours against the real spherical-harmonic (SH) basis at the ray's direction: 1, 4 or 9 coefficients per colour channel come back
 * per item and nothing per sample crosses the bus.
 *  - Item i is (origin = point, direction = axis), both used AS GIVEN.  The axis is read only by the hemisphere domain.
 *  - First ray.  For sample s of 0..K, K = path.samples_per_ray, the stream index is j = path.first_stream + i * K + s (32 bits).  With
 *    g = RNG (seed, pixel = j, sample = 1) and u = normalize(random_in_unit_sphere(g)) (Vec3::new_random_unit_vector, vec3extend.rs:32-34;
 *    three draws, nothing else is taken from g):
 *      TRT_PROBE_SPHERE:      dir = u
 *      TRT_PROBE_HEMISPHERE:  dir = dot(u, axis) > 0 ? u : -u   (Vec3::new_random_on_hemisphere, vec3extend.rs:36-43; a zero or NaN dot flips)
 *    and the ray is Ray::new(point, dir), which normalises AGAIN.  d below is that ray's stored direction, not u: the second normalisation
 *    changes the bits of about a quarter of the directions.
 *  - Path.  The sample's colour c is CpuSampler::single_point_sampling (cpu.rs:39-65) for that ray with RNG (seed, j, 0) and the budget
 *    max_bounces, exactly as trt_gather traces its drawn ray.  stats / d_counters (samples and rays only; `rays` counts the reference's
 *    world.hit calls) and kernel_ms: as in trt_gather.
 *  - Basis.  Real SH in the graphics convention: no Condon-Shortley sign, coefficient index k = l (l + 1) + m.  With (x, y, z) = d, all f32,
 *    one IEEE operation per operator, nothing fused, in exactly this parenthesisation:
 *      c0 = 0.282094792f  c1 = 0.488602512f  c2 = 1.092548431f  c3 = 0.315391565f  c4 = 0.546274215f
 *      b0 = c0            b1 = c1*y          b2 = c1*z          b3 = c1*x
 *      b4 = c2*(x*y)      b5 = c2*(y*z)      b6 = c3*((3.0f*(z*z)) - 1.0f)           b7 = c2*(x*z)      b8 = c4*((x*x) - (y*y))
 *  - Fold, per item, in sample order, inv_K = 1.0f / float(K): for k < C = bands * bands
 *      t = b_k * inv_K;   sh[k].ch = sh[k].ch + c.ch * t     per channel
 *    `sh` holds n x C x 3 f32: item-major, then coefficient, then channel.  The bytes of coefficient k do not depend on `bands`.
 *  - A sample whose first ray has a NaN component (a NaN point; the draw with u3 == 0, where the reference normalises a zero vector) is
 *    traced and counted as trt_gather counts it and ADDS NOTHING to the sums - neither 0 nor NaN: one such draw in 2^23 must not poison a
 *    probe.
 *  - Meaning.  The sums are the plain mean of c * Y_k(d).  4 pi sh[k] (SPHERE) or 2 pi sh[k] (HEMISPHERE: the function is 0 in the other
 *    half-space) estimates the integral of L Y_k over the directions, and the irradiance about a unit normal n is
 *    sum_k A_l(k) * (4 pi sh[k]) * Y_k(n) with A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4.
 *  - Sample range, accumulate (the C x 3 sums per item are read back), the 1 / K scale fixed by K, split invariance by samples (split the
 *    range, set accumulate) and by items (first_stream + a * K), order, coherence and concurrency: as in trt_radiance.  "Nothing to
 *    trace" - an empty sample range or max_bounces == 0 - zeroes [0, 12 C n) unless accumulate, which touches nothing.  No byte outside
 *    [0, 12 C n) of `sh` is ever written.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL params; trt_radiance's own errors, applied to `path` with `sh` as the
 *    required buffer; a `domain` that is not 1 or 2; `bands` outside 1..3; a non-zero reserved word.  Then TRT_ERR_NO_DEVICE, then
 *    TRT_ERR_OOM for the host form's buffers.  n == 0 succeeds and touches nothing, with or without a device.
 * trt_probe: HOST buffers, synchronous, as trt_gather.  trt_probe_device: buffers in HBM, asynchronous on `stream`; allocates nothing. */
enum trt_probe_domain { TRT_PROBE_SPHERE = 1, TRT_PROBE_HEMISPHERE = 2 };
typedef struct {
    trt_radiance_params path;     /* every field as in trt_radiance, same rules, same errors; K = path.samples_per_ray */
    uint32_t domain;              /* enum trt_probe_domain */
    uint32_t bands;               /* 1, 2 or 3: SH bands l = 0 .. bands-1, C = bands*bands coefficients (1, 4, 9) */
    uint32_t reserved[6];         /* zero */
} trt_probe_params;               /* 96 B: offsets 0, 64, 68, 72 */
void trt_probe_params_default(trt_probe_params *out);   /* path = trt_radiance_params_default, SPHERE, bands 3; NULL tolerated */
int trt_probe(trt_scene *s, const trt_ray *items, uint32_t n, const trt_probe_params *p, float *sh, trt_stats *stats);
int trt_probe_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_probe_params *p, float *d_sh, uint64_t *d_counters,
                     void *stream);
/* How trt_probe[_device] launches n items on this scene: trt_gather_launch_plan's rule and fields over the probe kernels' own table for
 * that `bands` (the same shapes; kernel_waves_per_simd is that table's bound, lower than the gather's: a lane carries 3 C sums more).
 * `bands` outside 1..3 is TRT_ERR_INVALID_ARG.  The rule gives a wave 256 items whatever K is, as it does for trt_radiance and
 * trt_gather: a few probes with many samples fill few lanes.  The exact workaround: list such a probe m times with K / m samples each and
 * distinct first_streams, then average the m rows - every row is a plain mean over its own samples. */
int trt_probe_launch_plan(const trt_scene *s, uint32_t n, uint32_t bands, uint32_t compute_units, trt_query_plan *out);

/* ---- Light-path passes: the gathered radiance split by the depth and the end of each path ----
 * trt_radiance and trt_gather say how much light arrives; a passes query says by what kind of path.  A baker that lights directly at run
 * time bakes only the indirect part; a frame filters emitters seen directly apart from smooth indirect light; a probe placer asks what
 * share of a probe's paths die by their budget, the sign of a probe inside geometry.  The split is exact, not a difference of two noisy
 * runs: in CpuSampler::single_point_sampling (cpu.rs:39-65) a sample's colour comes from exactly one terminal event - Light::scatter
 * returns None, or a miss adds the background and breaks - and every other hit adds +0, so each sample belongs to exactly one class and
 * the same paths, on the same RNG draws, are folded per class.
 *  - First ray.  With gather.lobe == TRT_PASSES_RAYS item i is a ray used AS GIVEN, as in trt_radiance: not normalised, nothing is drawn,
 *    and gather.spread is ignored (not read, not validated).  With TRT_PASSES_COSINE or TRT_PASSES_CONE (the values of enum trt_lobe) item
 *    i is a surfel (point, axis) and the first ray of sample s is trt_gather's for the same `gather`, bit for bit: three draws from RNG
 *    (seed, pixel = j, sample = 1), j = gather.path.first_stream + i * K + s, K = gather.path.samples_per_ray, the cosine or the cone rule,
 *    Ray::new.
 *  - Path.  The sample's colour c is CpuSampler::single_point_sampling (cpu.rs:39-65) for that ray with RNG (seed, j, 0) and the budget
 *    max_bounces - exactly what trt_radiance (RAYS) or trt_gather (COSINE, CONE) folds for stream j.
 *  - Class of a sample.  d is the number of scatters before the path ended (the times cpu.rs:52-54 ran), and the end is one of
 *      LIGHT: the path hit a TRT_LIGHT material (scatter returned None, cpu.rs:55-57);
 *      SKY:   the ray missed (cpu.rs:58-61);
 *      SPENT: the budget ran out (d == max_bounces), so c is 0.
 *    With B = depth_bins and b = min(d, B - 1) the sample's slot is b for LIGHT and B + b for SKY.  SPENT has no slot.
 *  - Fold, per item, in sample order, all f32, one IEEE operation per operator, nothing fused; inv_K = 1.0f / float(K):
 *      passes[i][slot].ch = passes[i][slot].ch + c.ch * inv_K          (LIGHT, SKY)
 *      spent[i] = spent[i] + inv_K                                     (SPENT)
 *    A sample touches its own slot only: the other slots of the item are NOT touched by it, which is not the same as adding 0 (a slot
 *    that holds -0 or NaN keeps it).  `passes` holds n x 2B x 3 f32: item-major, then slot (LIGHT 0..B-1, SKY 0..B-1), then channel.
 *    `spent` holds n f32 and may be NULL (not wanted; `passes` is the same either way).
 *  - A first ray with a NaN component hits nothing (the rule of the queries): the sample is SKY at d = 0, slot B receives `background`.
 *  - Identities.  (1) On a scene whose light colours and albedos are non-negative, with background == 0 and B == 1, slot 0 is
 *    trt_gather's `radiance` (RAYS: trt_radiance's) byte for byte: there every sample adds c.ch * inv_K to the one sum, here the LIGHT
 *    samples do, and every other sample's c is +0, which changes no sum that started at +0 (x + (+0) == x for every x but -0, and no sum
 *    is -0).  (2) The LIGHT and SKY slots at depth d < B - 1 do not depend on B: LIGHT slot d of a call with B bins equals LIGHT slot d
 *    of a call with B' bins, and SKY slot B + d equals SKY slot B' + d, for d < min(B, B') - 1.
 *  - Meaning.  For a surfel, LIGHT and SKY at d = 0 are its direct light (the first ray reached an emitter or the sky); everything at
 *    d >= 1 is indirect.  For a camera ray, d = 0 is what is seen directly.  The sum of all slots is trt_gather's radiance up to the
 *    rounding of a different summation order; `spent` is the share of the K samples that ended by their budget.
 *  - Sample range, accumulate (the 2B x 3 sums per item and `spent` are read back), the 1 / K scale fixed by K, split invariance by
 *    samples (split the range, set accumulate) and by items (first_stream + a * K), order, coherence and concurrency: as in trt_radiance.
 *    "Nothing to trace" - an empty sample range or max_bounces == 0 - zeroes [0, 24 B n) of `passes` and [0, 4 n) of `spent` unless
 *    accumulate, which touches nothing.  No byte outside those ranges is ever written.
 *  - stats / d_counters receive samples ([0]) and rays ([1]) only; `rays` counts the reference's world.hit calls for these samples,
 *    as in trt_radiance.  kernel_ms as in trt_radiance.  `d_counters`: 16 uint64 as in trt_render_device, added to, or NULL.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL params; trt_radiance's own errors, applied to gather.path with `passes`
 *    as the required buffer; gather.lobe not 0, 1 or 2; with TRT_PASSES_CONE a `spread` that is NaN, infinite or negative; depth_bins
 *    outside 1..4; a non-zero reserved word of `gather` or of this struct.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the host form's
 *    buffers.  n == 0 succeeds and touches nothing, with or without a device.
 * trt_passes: HOST buffers, synchronous, as trt_gather.  trt_passes_device: buffers in HBM, asynchronous on `stream`; allocates nothing.
 * A frame in passes: for sample s take trt_primary_rays_device for s, then trt_passes_device with K = spp, the sample range [s, s + 1)
 * and accumulate (from s = 1 on).  Such a frame uses the query stream numbering (seed, first_stream + pixel * K + s, 0), not trt_render's. */
enum trt_passes_source { TRT_PASSES_RAYS = 0, TRT_PASSES_COSINE = 1, TRT_PASSES_CONE = 2 };   /* 1, 2 = enum trt_lobe */
typedef struct {
    trt_gather_params gather;     /* path, lobe (read as enum trt_passes_source) and spread: trt_gather's rules and errors */
    uint32_t depth_bins;          /* B = 1..4: depths 0 .. B-2 have a slot each, depths >= B-1 share the last */
    uint32_t reserved[7];         /* zero */
} trt_passes_params;              /* 128 B: offsets 0, 96, 100 */
void trt_passes_params_default(trt_passes_params *out);   /* gather = trt_gather_params_default (source COSINE), depth_bins 3; NULL tolerated */
int trt_passes(trt_scene *s, const trt_ray *items, uint32_t n, const trt_passes_params *p, float *passes, float *spent, trt_stats *stats);
int trt_passes_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_passes_params *p, float *d_passes, float *d_spent,
                      uint64_t *d_counters, void *stream);
/* How trt_passes[_device] launches n items on this scene: trt_gather_launch_plan's rule and fields over the passes kernels' own table for
 * that `depth_bins` (the same shapes; B = 1 and 2 run the kernels that carry 2 bins, B = 3 and 4 those that carry 4;
 * kernel_waves_per_simd is that table's bound: a lane carries 6 sums per bin).  `depth_bins` outside 1..4 is TRT_ERR_INVALID_ARG. */
int trt_passes_launch_plan(const trt_scene *s, uint32_t n, uint32_t depth_bins, uint32_t compute_units, trt_query_plan *out);

/* ---- Direct-light queries: shadow rays the device draws towards a table of emitters ----
 * trt_gather, trt_probe and trt_passes find the lights as the reference does, by chance: in the Cornell box the lamp covers about 0.5 % of
 * a floor texel's cosine lobe, so the d = 0 LIGHT slot of trt_passes - the texel's direct light - holds about K / 200 samples worth 15
 * each.  A direct-light query aims: every sample picks an emitter of a caller-supplied table, a point on it, and asks trt_occluded's
 * question of the segment between the surfel and that point.  A baker, a probe placer or an engine that lights a surfel at run time
 * gets the same mean from about a hundredth of the samples.
 *
 * The emitter table is the caller's: trt_scene_emitters lists the scene's own lights, and the table handed to trt_direct may be that
 * list, a part of it, or lights that are no geometry of the scene at all (trt_emitter_init_quad, trt_emitter_init_sphere) - a scene
 * without a TRT_LIGHT material can be lit by a virtual lamp.
 *  - trt_scene_emitters: the geometries whose material kind is TRT_LIGHT, in insertion order.  Host only, needs no device.  *count
 *    receives their number; the first min(cap, *count) are written to `out` (which may be NULL with cap == 0).  A NULL scene or count is
 *    TRT_ERR_INVALID_ARG.
 *  - The two init functions fill geometry = 0xFFFFFFFF, reserved = 0 and compute `normal` and `area` with the host code
 *    trt_scene_emitters uses, all f32, one IEEE operation per operator, nothing fused:
 *      cross = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x);  length = sqrt((c.x*c.x + c.y*c.y) + c.z*c.z)
 *      quad:   normal = cross / length (what Ray::new makes of the cross product, ray.rs:12-14; the value the packed scene holds,
 *              quad.rs:20-29), area = length;      sphere:  area = 12.566371f * (r * r), normal = 0 (unread)
 *    A NULL `out` is tolerated.
 *
 * Contract of a sample.  Item i is a surfel (x = origin, n = direction), both used AS GIVEN.  K = path.samples_per_ray, E = n_emitters;
 * sample s of 0..K has stream index j = path.first_stream + i * K + s (32 bits).  All f32, one IEEE operation per operator, nothing fused:
 *  1. g = RNG (seed, pixel = j, sample = 1).  Stream (seed, j, 0) is not touched; path.max_bounces and path.background are not read.
 *  2. u0 = random(g) (utils/random.rs:11-13);  e = min(uint32(u0 * float(E)), E - 1): emitters are chosen uniformly.
 *  3. Quad:    a = random(g), then b = random(g);  y = (corner + u * a) + v * b;  nl = normal.
 *     Sphere:  nl = Vec3::new_random_unit_vector(g) (vec3extend.rs:32-34: three draws, as trt_probe draws it);  y = centre + nl * radius.
 *  4. w = y - x;  d2 = dot(w, w);  cs = dot(n, w);  cl = |dot(nl, w)|.  Emitters shine from both faces, as Light::emitted ignores the
 *     face (light.rs).
 *  5. scale = (area * float(E)) * 0.318309886f;  geom = (cs * cl) / (d2 * d2);  wgt = geom * scale.
 *  6. The sample is LIVE iff cs > 0 and d2 > 0 and wgt is finite.  A NaN in the item, the record or the draw fails one of the three.  A
 *     dead sample is counted in `samples`, walks nothing and adds nothing.
 *  7. Shadow ray: ray = Ray::new(x, w), which normalises (ray.rs:12-14);  t_max = sqrt(d2) * shadow_end.  The sample is occluded iff
 *     BVH::hit (hittable/bvh.rs:24-27,88-107) over [0.001, t_max) finds anything: exactly what trt_occluded answers for that ray and
 *     t_max.  Every material occludes, lights and glass included.  If t_max is not > 0.001 the range is empty: nothing is walked, the
 *     sample is unoccluded and is not counted in `rays`.
 *  8. Fold, per item, in sample order, inv_K = 1.0f / float(K).  A live, unoccluded sample has c.ch = color.ch * wgt and adds
 *       radiance.ch = radiance.ch + c.ch * inv_K;   moment2.ch = moment2.ch + (c.ch * c.ch) * inv_K
 *     Every other sample adds nothing (it does not add 0).  `radiance` and `moment2` hold n x 3 f32; `moment2` may be NULL (not wanted).
 * Meaning.  With a unit axis the mean is the radiance a white Lambertian surfel reflects from the table's emitters alone - direct
 * irradiance / pi: trt_gather's convention, so the two are comparable, and this result plus trt_passes' indirect slots is a full bake.
 * trt_variance(radiance, moment2, n, K, ...) is the variance of each estimate.
 * Limits.  (1) Emitters are chosen with probability 1 / E whatever their power: where powers differ much, split the table over calls and
 * add the results.  (2) An occluder within (1 - shadow_end) of the distance to the emitter point is not seen; shadow_end < 1 keeps the
 * emitter's own surface, which is geometry of the scene, from shadowing itself.  The ray is normalised and t_max is a SHARE of the
 * distance on purpose: an un-normalised segment to t = 1 would put the walks' fixed lower end 0.001 at 0.1 % of the lamp's distance and
 * leak light at contact corners.  (3) A non-unit axis is used as given: the result scales linearly with its length.  (4) An emitter
 * coplanar with other geometry - the stock Cornell box's lamp lies in the ceiling's plane, both y = 100 - is seen fully by the shadow
 * ray, while the reference's own paths (trt_gather, trt_passes) see it only where rounding lets the lamp win the tie with the ceiling
 * (about a quarter of the time in one measurement: 0.038 against 0.128 over 40 surfels of the box).  That is a property of that scene, not
 * of this query: compare the two on a lamp lowered to y = 99.
 *  - Sample range, accumulate, the 1 / K scale fixed by K, split invariance by samples (split the range, set accumulate) and by items
 *    (first_stream + a * K), order, coherence and concurrency: as in trt_radiance.  An empty sample range zeroes the n entries unless
 *    accumulate, which touches nothing; max_bounces == 0 is NOT "nothing to trace" here.  No byte outside [0, 12 n) of either buffer is
 *    ever written.
 *  - stats / d_counters receive samples ([0]: every sample of the range) and rays ([1]: the occlusion walks made) only.  kernel_ms as
 *    in trt_radiance.  `d_counters`: 16 uint64 as in trt_render_device, added to, or NULL.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL params; trt_radiance's own errors, applied to `path`; with n > 0 a NULL
 *    `emitters` or n_emitters outside 1 .. 2^20; shadow_end NaN, <= 0 or > 1; a non-zero reserved word; and, host form only (the
 *    device form cannot read the table), an emitter whose kind is above 1 or that has a non-zero reserved word.  The device form reads
 *    any kind other than 1 as a sphere.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the host form's buffers.  n == 0 succeeds and
 *    touches nothing, with or without a device.
 * trt_direct: HOST buffers, synchronous; one device allocation for the call (items, table, sums); the sums are uploaded only when
 * accumulate is set.  trt_direct_device: buffers in HBM on the calling thread's current device - the table included, n_emitters x 80
 * bytes, 4-byte aligned - asynchronous on `stream`; allocates nothing.  The launch rule gives a wave 256 items whatever K is, as it does
 * for trt_radiance and trt_gather. */
typedef struct {
    uint32_t kind;                /* 0 sphere, 1 quad */
    uint32_t geometry;            /* insertion index in the world, or 0xFFFFFFFF: a light of the caller's own that is not in the scene; not read by trt_direct */
    trt_vec3 a, b, c;             /* sphere: a = centre, b.x = radius; quad: a = corner, b = u, c = v */
    trt_vec3 normal;              /* quad: Quad::new's unit normal (quad.rs:20-29); sphere: unread */
    trt_vec3 color;               /* emitted colour (Light::emitted) */
    float area;                   /* quad: length(cross(u, v)); sphere: 12.566371f * (r * r) */
    uint32_t reserved[2];         /* zero */
} trt_emitter;                    /* 80 B: offsets 0, 4, 8, 20, 32, 44, 56, 68, 72 */
int trt_scene_emitters(const trt_scene *s, trt_emitter *out, uint32_t cap, uint32_t *count);
void trt_emitter_init_quad(trt_emitter *out, trt_vec3 corner, trt_vec3 u, trt_vec3 v, trt_vec3 color);
void trt_emitter_init_sphere(trt_emitter *out, trt_vec3 centre, float radius, trt_vec3 color);
typedef struct {
    trt_radiance_params path;     /* samples_per_ray (K), seed, sample_begin, sample_end, accumulate, first_stream: trt_radiance's rules and
                                     errors.  max_bounces and background are IGNORED (not read): there is no path. */
    float shadow_end;             /* the shadow ray covers [0.001, distance * shadow_end): in (0, 1] */
    uint32_t reserved[7];         /* zero */
} trt_direct_params;              /* 96 B: offsets 0, 64, 68 */
void trt_direct_params_default(trt_direct_params *out);   /* path = trt_radiance_params_default, shadow_end = 0.999f; NULL tolerated */
int trt_direct(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, uint32_t n_emitters,
               const trt_direct_params *p, float *radiance, float *moment2, trt_stats *stats);
int trt_direct_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters, uint32_t n_emitters,
                      const trt_direct_params *p, float *d_radiance, float *d_moment2, uint64_t *d_counters, void *stream);
/* How trt_direct[_device] launches n items on this scene: trt_ambient_launch_plan's rule and fields over the direct-light kernels' own
 * table (the same shapes; kernel_waves_per_simd is that table's bound). */
int trt_direct_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Next-event queries: the paths of trt_radiance / trt_gather with a shadow ray to the emitter table at every diffuse hit ----
 * trt_direct aims at the lights for the surfel itself; every query that carries light along a path (trt_radiance, trt_gather, trt_probe,
 * trt_passes) still finds them by chance at every later bounce.  A next-event query traces the same path - the same vertices, bit for
 * bit - and at every Lambertian vertex sends one device-drawn shadow ray to a caller-supplied emitter table (trt_direct's table and
 * draw).  A light the path then reaches by a diffuse scatter is hidden, so nothing is counted twice: the expectation is the
 * reference's at the same max_bounces, the variance is not.
 *
 * Contract of a sample.  Item i is a ray (source RAYS) or a surfel (COSINE, CONE), used AS GIVEN.  E = n_emitters,
 * K = gather.path.samples_per_ray, B = gather.path.max_bounces; sample s of 0..K has stream index j = first_stream + i * K + s (32 bits).
 * All f32, one IEEE operation per operator, nothing fused:
 *  1. First ray: exactly trt_passes' for the source.  RAYS: the item.  COSINE, CONE: trt_gather's draw on stream (seed, j, 1).
 *  2. The path runs on stream (seed, j, 0) and makes exactly the draws of CpuSampler::single_point_sampling (cpu.rs:39-65): its vertices
 *     are those of trt_radiance / trt_gather for the same j, bit for bit.  color = 0, atten = 1, remain = B;
 *     after_diffuse = (source_is_diffuse != 0).
 *  3. At a hit (cpu.rs:49-50) color = color + atten * emission, where emission is the light's colour, except that it is Vec3::zero()
 *     when the material is a light AND after_diffuse is set.  This is the only change to the reference's loop body.
 *  4. Scatter, atten = atten * attenuation and remain -= 1 as in the reference (cpu.rs:51-54).  after_diffuse becomes (material kind ==
 *     TRT_LAMBERTIAN): metal of any fuzz and dielectric count as specular, a light they lead to is seen by the path itself.
 *  5. Next event.  If the hit was Lambertian AND remain > 0 after the decrement, the sample at that vertex is trt_direct's contract
 *     steps 2-7 with x = rec.p (the new ray's origin), n = rec.normal (unit, facing against the incoming ray), g = RNG (seed, j, 2 + d)
 *     where d = scatters made before this vertex, the same shadow_end and the same "an empty range walks nothing, is unoccluded".  A
 *     live, unoccluded sample has c.ch = emitter colour.ch * wgt and adds  color = color + atten * c  with atten as step 4 left it;
 *     every other sample adds nothing.  The term is added before the next vertex's emission.  The shadow ray stands for the emission
 *     the reference would find at hit number h + 1 <= B, hence the condition on remain.
 *  6. Miss: color = color + atten * background, as in the reference (cpu.rs:58-61).  The sky is never hidden.
 *  7. The fold (radiance.ch = radiance.ch + color.ch * inv_K, moment2.ch = moment2.ch + (color.ch * color.ch) * inv_K; moment2 may be
 *     NULL), the sample range, accumulate, split invariance by samples and by items (first_stream + a * K), "nothing to trace" (an empty
 *     range or B == 0 zeroes the n entries unless accumulate, which touches nothing), the NaN-first-ray rule and the output bounds
 *     ([0, 12 n) of either buffer): trt_radiance's, unchanged.
 *  8. stats / d_counters: samples ([0]) counts the samples of the range, rays ([1]) the world.hit calls (cpu.rs:48) plus the shadow
 *     walks made.  kernel_ms and `d_counters` as in trt_radiance.
 *  9. Errors, before any device work, TRT_ERR_INVALID_ARG: trt_passes' own on `gather` (trt_radiance's on the path, a source other than
 *     0, 1, 2, a cone spread that is negative or not finite, a non-zero reserved word); trt_direct's on the table (with n > 0 a NULL
 *     table or n_emitters outside 1 .. 2^20; host form only: a record whose kind is above 1 or with a non-zero reserved word) and on
 *     shadow_end (NaN, <= 0, > 1); source_is_diffuse above 1; a non-zero reserved word.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the
 *     host form's buffers.  n == 0 succeeds and touches nothing, with or without a device.
 * Meaning of source_is_diffuse = 1.  The first hit is treated as reached by a diffuse scatter: with the COSINE source the result is the
 * surfel's INDIRECT light only, and trt_direct(surfel) + trt_nee(surfel) is a full bake with aimed light at every bounce.  With 0 the
 * first hit's emission counts, as for a camera ray: the result estimates what trt_radiance / trt_gather estimate.
 * Identities.  (1) With B == 1 there is no next event and, with source_is_diffuse == 0, nothing is hidden: the result is trt_radiance's
 * (RAYS) / trt_gather's (COSINE, CONE), byte for byte.  (2) On a scene without a Lambertian material the result is trt_radiance's /
 * trt_gather's for any B (source_is_diffuse == 0).
 * Limits.  (1) The table should list every TRT_LIGHT geometry of the scene, which trt_scene_emitters does: a light left out of the table
 * is still hidden after a diffuse scatter, so its bounced light is lost.  (2) Virtual emitters (trt_emitter_init_*) add light no path can
 * hit: the result is then no estimate of trt_gather's.  (3) trt_direct's limits are inherited: the uniform choice among emitters,
 * shadow_end, and the lamp coplanar with other geometry (the stock Cornell box: compare on a lamp lowered to y = 99).
 * trt_nee: HOST buffers, synchronous; one device allocation for the call.  trt_nee_device: buffers in HBM (the table included),
 * asynchronous on `stream`; allocates nothing.  A frame: per sample s, trt_primary_rays_device for s, then trt_nee_device with source
 * RAYS, K = spp, the sample range [s, s + 1) and accumulate from the second pass on, as trt_passes' frame.  The launch rule gives a wave
 * 256 items whatever K is, as it does for every query. */
typedef struct {
    trt_gather_params gather;     /* path, lobe read as enum trt_passes_source (RAYS 0, COSINE 1, CONE 2), spread: trt_passes' rules and errors */
    float shadow_end;             /* as trt_direct: in (0, 1] */
    uint32_t source_is_diffuse;   /* 0 or 1: after_diffuse at the first hit */
    uint32_t reserved[6];         /* zero */
} trt_nee_params;                 /* 128 B: offsets 0, 96, 100, 104 */
void trt_nee_params_default(trt_nee_params *out);   /* gather = trt_passes_params_default's (source COSINE), shadow_end 0.999f, source_is_diffuse 0; NULL tolerated */
int trt_nee(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, uint32_t n_emitters, const trt_nee_params *p,
            float *radiance, float *moment2, trt_stats *stats);
int trt_nee_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters, uint32_t n_emitters,
                   const trt_nee_params *p, float *d_radiance, float *d_moment2, uint64_t *d_counters, void *stream);
/* How trt_nee[_device] launches n items on this scene: trt_passes_launch_plan's rule and fields over the next-event kernels' own table
 * (the same shapes; kernel_waves_per_simd is that table's bound, the same for every source). */
int trt_nee_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Next-event queries with multiple importance sampling: the shadow ray and the hit the path makes anyway, weighted by their densities ----
 * trt_nee counts a light after a diffuse scatter through the shadow ray alone.  For a vertex beside a lamp the shadow sample's 1/d2 weight
 * is hundreds of times the mean, and that tail carries the variance above the plain gather's.  A light after a diffuse
 * scatter can be found two ways - by the shadow ray of the vertex before (density p_light) and by the scattered ray itself (density
 * p_bsdf) - and this query counts BOTH, each weighted so that the two weights of one point sum to 1.  Near the lamp p_bsdf / p_light is
 * large, the shadow sample's weight small: the tail is gone, the expectation stays.
 *
 * Contract of a sample.  trt_nee's, with params->nee in the place of its params, except for what a sample ADDS in steps 3 and 5.
 * Unchanged: streams, vertices, the draws of steps 1-2 and 4-6, the fold, sample ranges, accumulate, both split invariances, "nothing
 * to trace", the NaN-first-ray rule, output bounds and counters; the paths and the shadow rays walked are trt_nee's.  All f32, one IEEE
 * operation per operator, nothing fused.  E = n_emitters;  sc(a) = (a * float(E)) * 0.318309886f;  q(x) = x for TRT_MIS_BALANCE and
 * x * x for TRT_MIS_POWER.
 *  - Lambertian scatter (step 4).  After every Lambertian scatter csh = dot(rec.normal, new_ray.direction): the facing unit normal with
 *    the direction as Ray::new normalised it.  It is kept until the next hit.
 *  - Next event (step 5).  With wgt from trt_direct's step 5 for the drawn record:  wl = 1.0f / (1.0f + q(wgt));  if the record's
 *    `geometry` word is 0xFFFFFFFF, wl = 1.0f (a virtual emitter cannot be hit: its shadow ray counts in full).  A live, unoccluded
 *    sample has c.ch = (colour.ch * wgt) * wl and adds color = color + atten * c.  Liveness, t_max, which samples walk and the condition on
 *    remain are unchanged.
 *  - Light hit (step 3).  When the material is a light and after_diffuse is set, color = color + atten * Vec3::zero() happens as in
 *    trt_nee.  At hit number 1 (which has after_diffuse only through source_is_diffuse) nothing more is added: it is hidden in full, as
 *    trt_direct, which that mode pairs with, has no weights.  At any later hit, with t = rec.t and the incoming ray:
 *      clh = |dot(rec.normal, ray.direction)|
 *      area = the hit primitive's own: quad sqrt((n.x*n.x + n.y*n.y) + n.z*n.z) of the un-normalised normal the packed scene holds,
 *             sphere 12.566371f * (r * r) - the bits trt_scene_emitters writes for that geometry
 *      g = ((csh * clh) / (t * t)) * sc(area)
 *      wb = q(g) / (1.0f + q(g)) if csh > 0 and q(g) is finite, else 1.0f (the matching shadow sample would have been dead)
 *      color = color + atten * (emission * wb)
 *    A light reached without after_diffuse counts in full, as in trt_nee.
 *  - Why the weights sum to 1: wgt is f cos / p_light = p_bsdf / p_light for the cosine lobe, g is the same ratio seen from the hit, so
 *    1 / (1 + wgt) and g / (1 + g) are the balance weights of the two strategies at one point; the power form squares the ratio.
 *  - Bound.  With the scene's own table, BALANCE and albedos <= 1 every term is at most the emitter's colour up to rounding: a sample is
 *    at most B x the largest colour channel.
 *  - Table rule.  The entries whose `geometry` is not 0xFFFFFFFF must be exactly the scene's TRT_LIGHT geometries, each once, as
 *    trt_scene_emitters wrote them; any order, with any virtual entries among them.  The device does not look the hit up in the table:
 *    it takes E from the table and the area from the hit.  The host form checks the set of `geometry` words against the scene; THE
 *    DEVICE FORM CANNOT CHECK: with another table its weights do not sum to 1 and the result is biased.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL params; trt_nee's on `nee`; heuristic above 1; a non-zero reserved word;
 *    the table rule (host form, n > 0).  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM.  n == 0 succeeds and touches nothing.
 *  - Identities.  (1) With B == 1 and source_is_diffuse == 0 the result is trt_radiance's / trt_gather's, byte for byte.  (2) On a scene
 *    without a Lambertian the result is theirs for any B.  (3) With a table of virtual emitters only, on a scene without a TRT_LIGHT
 *    geometry, the result is trt_nee's bytes for both heuristics.  (4) stats.rays and stats.samples equal trt_nee's for the same call.
 *  - Limits.  The uniform choice among emitters and shadow_end are inherited.  On the stock Cornell box, whose lamp is coplanar with the
 *    ceiling, the two strategies disagree about visibility and the weights do not sum to 1 there: compare on the lowered lamp. */
enum trt_mis_heuristic { TRT_MIS_BALANCE = 0, TRT_MIS_POWER = 1 };
typedef struct {
    trt_nee_params nee;           /* trt_nee's rules and errors, unchanged */
    uint32_t heuristic;           /* enum trt_mis_heuristic */
    uint32_t reserved[7];         /* zero */
} trt_nee_mis_params;             /* 160 B: offsets 0, 128, 132 */
void trt_nee_mis_params_default(trt_nee_mis_params *out);   /* nee = trt_nee_params_default's, heuristic TRT_MIS_BALANCE; NULL tolerated */
int trt_nee_mis(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, uint32_t n_emitters,
                const trt_nee_mis_params *p, float *radiance, float *moment2, trt_stats *stats);
int trt_nee_mis_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters, uint32_t n_emitters,
                       const trt_nee_mis_params *p, float *d_radiance, float *d_moment2, uint64_t *d_counters, void *stream);
/* How trt_nee_mis[_device] launches n items on this scene: trt_nee_launch_plan's rule and fields over the weighted kernels' own table
 * (the same shapes; kernel_waves_per_simd is that table's bound, the same for every source and heuristic). */
int trt_nee_mis_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Direct-light queries with multiple importance sampling: the shadow ray and a cosine-lobe ray from the surfel, weighted by their densities ----
 * trt_direct finds a surfel's direct light by the shadow ray alone.  For a surfel beside a lamp - the ceiling, the top rows of the walls - the
 * shadow sample's 1/d2 weight is a thousand times the mean, and trt_nee_mis hides hit 1 in full under source_is_diffuse = 1 because
 * trt_direct has no weights.  The surfel's direct light can be found two ways - by the shadow ray (density p_light) and by a cosine-lobe
 * ray from the surfel (density p_bsdf) - and this query counts BOTH in one sample, each weighted so that the two weights of one point sum
 * to 1.  It costs one closest-hit walk more per sample: where no surfel is near a light trt_direct stays the cheaper choice.
 *
 * Contract of a sample.  Unchanged from trt_direct, with params->direct in the place of its params: the items, used as given; K, E and
 * j = first_stream + i * K + s; sample ranges and accumulate; both split invariances; the output bounds; max_bounces and background are
 * not read.  All f32, one IEEE operation per operator, nothing fused.  q(x) = x for TRT_MIS_BALANCE and x * x for TRT_MIS_POWER;
 * sc(a) = (a * float(E)) * 0.318309886f.
 *  1. Shadow sample.  trt_direct's steps 1-7 exactly, on stream (seed, j, 1): the same emitter, point, wgt, liveness, ray, t_max, walk, and
 *     "an empty range walks nothing".  wl = 1.0f / (1.0f + q(wgt));  if the record's `geometry` word is 0xFFFFFFFF, wl = 1.0f (a virtual
 *     emitter cannot be hit: its shadow ray counts in full).  A live, unoccluded sample has  T_l.ch = (colour.ch * wgt) * wl.
 *  2. Lobe sample.  g = RNG(seed, j, 0xFFFFFFFF) - no other query reaches this stream (trt_nee's 2 + d would need 2^32 - 3 scatters); it
 *     is independent of stream 1, which the shadow draw uses and on which trt_gather / trt_nee draw their first ray, and of the path
 *     stream 0.  The ray is trt_gather's TRT_LOBE_COSINE draw about the item: three draws, axis + random_unit_vector, the axis itself
 *     if that is near zero, and Ray::new normalises.  It is walked as the gather walks its first ray: BVH::hit over [0.001, inf), closest
 *     hit; a ray with a NaN component hits nothing.  A miss, or a hit on anything but a TRT_LIGHT material, adds nothing: the background
 *     is not light from the table.  At a light, with t = rec.t:
 *       csh = dot(axis as given, ray.direction)
 *       clh = |dot(rec.normal, ray.direction)|
 *       area = the hit primitive's own, as in trt_nee_mis: quad sqrt((n.x*n.x + n.y*n.y) + n.z*n.z) of the un-normalised normal the
 *              packed scene holds, sphere 12.566371f * (r * r)
 *       g = ((csh * clh) / (t * t)) * sc(area)
 *       wb = q(g) / (1.0f + q(g)) if csh > 0 and q(g) is finite, else 1.0f
 *       T_b.ch = emission.ch * wb
 *  3. Fold.  A sample with neither term adds nothing, as in trt_direct.  Otherwise c = T_l, or T_b, or T_l + T_b (c.ch = T_l.ch + T_b.ch)
 *     - ONE sample, so moment2 is the second moment of the sum:
 *       radiance.ch = radiance.ch + c.ch * inv_K;   moment2.ch = moment2.ch + (c.ch * c.ch) * inv_K
 *  4. Counters.  stats.samples is trt_direct's.  stats.rays counts the shadow walks made plus one per sample for the lobe ray, counted
 *     as trt_gather counts its first world.hit call (cpu.rs:48).
 *  5. Table rule and errors.  The table rule is trt_nee_mis': the entries whose `geometry` is not 0xFFFFFFFF must be exactly the scene's
 *     TRT_LIGHT geometries, each once, as trt_scene_emitters wrote them; any order, with any virtual entries among them.  The host form
 *     checks it; THE DEVICE FORM CANNOT CHECK: with another table its weights do not sum to 1 and the result is biased.  Errors, before
 *     any device work, TRT_ERR_INVALID_ARG: a NULL params; trt_direct's on `direct`; heuristic above 1; a non-zero reserved word; the
 *     table rule (host form, n > 0).  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM.  n == 0 succeeds and touches nothing.
 *  6. Meaning and limits.  With a unit axis wgt = p_bsdf / p_light, and g is the same ratio seen from the hit, so 1 / (1 + wgt) and
 *     g / (1 + g) are the balance weights of the two strategies at one point and sum to 1 (the power form squares the ratio): the mean
 *     is trt_direct's - irradiance / pi from the scene's lights, plus virtual emitters in full.  With BALANCE and the scene's own table
 *     every term is at most the emitter's colour up to rounding: a sample is at most 2 x the largest colour channel.
 *     trt_direct_mis + trt_nee_mis(source_is_diffuse = 1) is the full bake with no unbounded term.  A non-unit axis is used as given in
 *     both draws and the bits are defined, but the weights no longer sum to 1 and the result does not scale linearly as trt_direct's
 *     does.  The coplanar lamp of the stock Cornell box (the two strategies disagree about its visibility), shadow_end and the uniform
 *     choice among emitters are inherited.
 *  7. Identities.  (1) On a scene without a TRT_LIGHT geometry and with a table of virtual emitters, radiance and moment2 are
 *     trt_direct's bytes for both heuristics.  (2) stats.samples equals trt_direct's.  (3) stats.rays equals trt_direct's plus
 *     trt_gather's at max_bounces = 1 for the same items and K. */
typedef struct {
    trt_direct_params direct;     /* trt_direct's rules and errors, unchanged */
    uint32_t heuristic;           /* enum trt_mis_heuristic */
    uint32_t reserved[7];         /* zero */
} trt_direct_mis_params;          /* 128 B: offsets 0, 96, 100 */
void trt_direct_mis_params_default(trt_direct_mis_params *out);   /* direct = trt_direct_params_default's, heuristic TRT_MIS_BALANCE; NULL tolerated */
int trt_direct_mis(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, uint32_t n_emitters,
                   const trt_direct_mis_params *p, float *radiance, float *moment2, trt_stats *stats);
int trt_direct_mis_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters, uint32_t n_emitters,
                          const trt_direct_mis_params *p, float *d_radiance, float *d_moment2, uint64_t *d_counters, void *stream);
/* How trt_direct_mis[_device] launches n items on this scene: trt_direct_launch_plan's rule and fields over the weighted kernels' own
 * table (the same shapes; kernel_waves_per_simd is that table's bound, the same for both heuristics). */
int trt_direct_mis_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Direct-light queries that choose the emitter by power: an alias table over the emitter table ----
 * trt_direct and trt_direct_mis choose an emitter with probability 1 / E whatever its power (limit (1) of trt_direct).  In a room with one
 * lamp and sixty dim lights sixty of sixty-one shadow rays go to a few percent of the light, and the one that reaches the lamp is scaled
 * by E.  trt_direct_pick and trt_direct_mis_pick are the same two queries with the emitter chosen through a Walker/Vose alias table the
 * caller builds once per emitter table: probability prob[e], one draw and two loads more per sample.  trt_direct,
 * trt_direct_mis, trt_nee and trt_nee_mis are unchanged and still choose uniformly; the next-event queries have PICK forms of their own
 * (trt_nee_pick, trt_nee_mis_pick below).
 *
 * The pick table: E records, record k for slot k AND for emitter k.  trt_emitter_pick_build is host only, needs no device and is
 * deterministic - the same input gives the same bytes:
 *  - Weights.  weights == NULL: w_e is the emitter's power, f32, one IEEE operation per operator, nothing fused:
 *      power_e = ((0.2126f * color.x + 0.7152f * color.y) + 0.0722f * color.z) * area
 *    Else w_e = weights[e], taken as given: any finite, non-negative values with a positive sum (distance, importance; trt_direct_pick
 *    only - trt_direct_mis_pick needs the power rule).
 *  - Total.  *total = the sum of the w_e accumulated in double in table order, rounded once to f32.  `total` may be NULL.
 *  - Probability.  prob[e] = w_e / *total: one f32 division.  These three rules are contract: the weighted kernel recomputes prob from a
 *    hit (trt_direct_mis_pick below).
 *  - Construction (Vose), in double, every step in this order so that the bytes are reproducible:
 *      (a) c_e = w_e where prob[e] > 0, else 0: a weight so small that the division underflows is built as weight 0.
 *      (b) S = the sum of the c_e in table order, compensated (Neumaier):  t = s + c;  lost += s >= c ? (s - t) + c : (c - t) + s;
 *          s = t;  at the end S = s + lost.  (A plain sum's rounding, times E, would land whole on the slot step (d) ends with.)
 *      (c) scaled_e = (c_e * double(E)) / S.  Two work lists, small (scaled_e < 1) and large (the others), are filled in increasing
 *          index order and emptied FROM THE BACK.
 *      (d) While neither is empty: take s off small and l off large;  q[s] = scaled_s, alias[s] = l;
 *          scaled_l = (scaled_l + scaled_s) - 1;  l goes to the back of small if scaled_l < 1, else to the back of large.
 *      (e) Every slot left on either list gets q = 1 and alias = its own index - except a slot left on small with scaled = 0, which gets
 *          q = 0 and the first emitter of largest c as its alias.
 *      (f) q is rounded to f32 and clamped to [0, 1]; reserved = 0.
 *    An emitter of weight 0 has q = 0 and is nobody's alias: it is never chosen.
 *  - Errors, all TRT_ERR_INVALID_ARG, in this order: a NULL `emitters` or `out`; E outside 1 .. 2^20; a weight that is negative or not
 *    finite; a total that is not positive and finite.  `out` is not written then.
 *
 * trt_direct_pick.  The contract of a sample is trt_direct's, word for word, except steps 2 and 5:
 *  2. u0 = random(g);  k = min(uint32(u0 * float(E)), E - 1);  u1 = random(g);  e = (u1 < pick[k].q) ? k : min(pick[k].alias, E - 1).
 *     One draw more than trt_direct: four for a quad, five for a sphere.  The min on the alias is contract: no table the device form is
 *     handed, however wrong, makes the kernel read outside the E records of either table.  A NaN q takes the alias.
 *  5. p = pick[e].prob;  scale = (area / p) * 0.318309886f;  geom = (cs * cl) / (d2 * d2);  wgt = geom * scale.  p == 0, or any p that
 *     makes wgt no finite number, is a dead sample under step 6.
 * Liveness, the shadow ray, t_max and the walk, the fold, sample ranges and accumulate, both split invariances, the output bounds and the
 * counters are trt_direct's.  With the table trt_emitter_pick_build makes of all-equal weights the choice is uniform but the bits are
 * not trt_direct's: one draw more is taken, and area / (1 / E) is not always area * E.
 *  - Errors: trt_direct's, in trt_direct's order, as far as its table size and reserved words; then with n > 0 a NULL `pick`; then, HOST
 *    FORM ONLY, trt_direct's check of the emitter records; then for each pick record in table order: q NaN or outside [0, 1], alias >= E,
 *    prob NaN, negative or above 1, a non-zero reserved word; then an emitter that can be chosen (q[k] > 0, or the alias of a slot with
 *    q < 1) whose prob is 0.  THE DEVICE FORM CHECKS ONLY THE POINTER: with a table whose prob is not the probability its q and alias
 *    imply the result is biased; the reads stay in bounds regardless.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM.  n == 0 succeeds and
 *    touches nothing.
 *  - trt_direct_pick: host buffers, the pick table in the call's one device allocation.  trt_direct_pick_device: `d_pick` in HBM,
 *    n_emitters x 16 bytes, 4-byte aligned; allocates nothing.
 *
 * trt_direct_mis_pick.  The contract is trt_direct_mis', with `total_power` = the builder's *total, and these changes:
 *  - The shadow sample uses steps 2 and 5 above;  wl = 1 / (1 + q(wgt)), 1 for a virtual emitter, as before.
 *  - At a light the lobe ray hits, sc(area) is replaced by the same ratio seen from the hit:
 *      pw = ((0.2126f * em.x + 0.7152f * em.y) + 0.0722f * em.z) * area      (em the hit material's emitted colour, area the hit primitive's own)
 *      ph = pw / total_power
 *      g = ((csh * clh) / (t * t)) * ((area / ph) * 0.318309886f)
 *    wb is unchanged: 1 when csh <= 0 or q(g) is not finite, which covers a black light (ph = 0).
 *  - ph repeats the builder's operations on the bits trt_scene_emitters writes, so it has the bits of prob[e] of that light: the two
 *    weights of one point sum to 1 as in trt_direct_mis, and with BALANCE a sample is at most 2 x the largest colour channel.
 *  - Table rule: trt_nee_mis' AND the pick table is the power-rule table (weights == NULL) of that emitter table.  The host form checks,
 *    after trt_direct_pick's checks and the emitter table rule: total_power positive and finite, then pick[e].prob bit for bit against
 *    power_e / total_power for every e.  THE DEVICE FORM CANNOT CHECK EITHER RULE: with a caller-weighted table or another total the
 *    weights do not sum to 1 and the result is biased.
 * The launch plans: trt_direct_launch_plan's rule and fields over the PICK kernels' own tables. */
typedef struct {
    float q;                      /* slot k keeps emitter k where u1 < q, else takes `alias`: in [0, 1] */
    uint32_t alias;               /* below E */
    float prob;                   /* the probability with which emitter k is chosen: w_k / total */
    uint32_t reserved;            /* zero */
} trt_emitter_pick;               /* 16 B: offsets 0, 4, 8, 12 */
int trt_emitter_pick_build(const trt_emitter *emitters, uint32_t n_emitters, const float *weights, trt_emitter_pick *out, float *total);
int trt_direct_pick(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, const trt_emitter_pick *pick,
                    uint32_t n_emitters, const trt_direct_params *p, float *radiance, float *moment2, trt_stats *stats);
int trt_direct_pick_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters, const trt_emitter_pick *d_pick,
                           uint32_t n_emitters, const trt_direct_params *p, float *d_radiance, float *d_moment2, uint64_t *d_counters,
                           void *stream);
int trt_direct_pick_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);
int trt_direct_mis_pick(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, const trt_emitter_pick *pick,
                        uint32_t n_emitters, const trt_direct_mis_params *p, float total_power, float *radiance, float *moment2,
                        trt_stats *stats);
int trt_direct_mis_pick_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters,
                               const trt_emitter_pick *d_pick, uint32_t n_emitters, const trt_direct_mis_params *p, float total_power,
                               float *d_radiance, float *d_moment2, uint64_t *d_counters, void *stream);
int trt_direct_mis_pick_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Next-event queries that choose the emitter by power: the same alias table at every diffuse vertex ----
 * trt_nee and trt_nee_mis draw the emitter of every vertex's shadow ray with probability 1 / E.  A sample runs up to B - 1 such draws
 * against the direct query's one, so in a room whose lights differ in power most of a bake's shadow rays are spent here.  trt_nee_pick and
 * trt_nee_mis_pick are the same two queries with every vertex draw taken through the pick table above (trt_emitter_pick,
 * trt_emitter_pick_build): one draw and two loads more per vertex.  `pick` and `total_power` stand where
 * trt_direct_pick / trt_direct_mis_pick have them.
 *
 * trt_nee_pick.  The contract is trt_nee's, word for word, except the vertex draw: on stream (seed, j, 2 + d) it uses steps 2 and 5 of
 * trt_direct_pick in place of trt_direct's -
 *    u0 = random(g);  k = min(uint32(u0 * float(E)), E - 1);  u1 = random(g);  e = (u1 < pick[k].q) ? k : min(pick[k].alias, E - 1)
 *    scale = (area / pick[e].prob) * 0.318309886f
 * - one draw more per vertex than trt_nee.  The min on the alias is contract here too: no table the device form is handed makes the kernel
 * read outside the E records of either table.  A NaN q takes the alias; prob == 0, or any prob that makes wgt no finite number, is a dead
 * sample.  The path and its streams, the hiding of diffusely reached lights, source_is_diffuse, the last-vertex rule, the fold, sample
 * ranges and accumulate, both split invariances, the output bounds and the counters are trt_nee's.  With max_bounces == 1 no vertex draws
 * and the result is trt_gather's (trt_nee's) bit for bit.
 *  - Errors: trt_nee's, in trt_nee's order, as far as its table size and reserved words; then with n > 0 a NULL `pick`; then, HOST FORM
 *    ONLY, trt_nee's check of the emitter records, then trt_direct_pick's checks of the pick records, in their order.  THE DEVICE FORM
 *    CHECKS ONLY THE POINTER: with a table whose prob is not the probability its q and alias imply the result is biased; the reads stay
 *    in bounds regardless.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM.  n == 0 succeeds and touches nothing.
 *  - trt_nee_pick: host buffers, the pick table in the call's one device allocation.  trt_nee_pick_device: `d_pick` in HBM, n_emitters x
 *    16 bytes, 4-byte aligned; allocates nothing.
 *
 * trt_nee_mis_pick.  The contract is trt_nee_mis', with `total_power` = the builder's *total, and two changes:
 *  - The shadow sample is drawn as above;  wl = 1 / (1 + q(wgt)), 1 for a virtual emitter, as before.
 *  - A light reached after a diffuse scatter at hit >= 2 is weighed with the light's own choice probability in place of 1 / E, as in
 *    trt_direct_mis_pick:
 *      pw = ((0.2126f * em.x + 0.7152f * em.y) + 0.0722f * em.z) * area      (em the hit material's emitted colour, area the hit primitive's own)
 *      ph = pw / total_power
 *      g = ((csh * clh) / (t * t)) * ((area / ph) * 0.318309886f)
 *    wb is unchanged: 1 when csh <= 0 or q(g) is not finite, which covers a black light (ph = 0).  ph has the bits of prob[e] of that
 *    light, so the two weights of one point sum to 1 as in trt_nee_mis.
 *  A light at hit 1 under source_is_diffuse stays hidden in full, as in trt_nee_mis.
 *  - Table rule: trt_nee_mis' AND the pick table is the power-rule table (weights == NULL) of that emitter table.  The host form checks,
 *    after trt_nee_mis' argument checks, the pointer, the emitter records and the pick records: trt_nee_mis' table rule, then total_power
 *    positive and finite, then pick[e].prob bit for bit against power_e / total_power for every e.  THE DEVICE FORM CANNOT CHECK EITHER
 *    RULE: with a caller-weighted table or another total the weights do not sum to 1 and the result is biased.
 * The launch plans: trt_nee_launch_plan's rule and fields over the PICK kernels' own tables. */
int trt_nee_pick(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, const trt_emitter_pick *pick,
                 uint32_t n_emitters, const trt_nee_params *p, float *radiance, float *moment2, trt_stats *stats);
int trt_nee_pick_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters, const trt_emitter_pick *d_pick,
                        uint32_t n_emitters, const trt_nee_params *p, float *d_radiance, float *d_moment2, uint64_t *d_counters,
                        void *stream);
int trt_nee_pick_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);
int trt_nee_mis_pick(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters, const trt_emitter_pick *pick,
                     uint32_t n_emitters, const trt_nee_mis_params *p, float total_power, float *radiance, float *moment2,
                     trt_stats *stats);
int trt_nee_mis_pick_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters,
                            const trt_emitter_pick *d_pick, uint32_t n_emitters, const trt_nee_mis_params *p, float total_power,
                            float *d_radiance, float *d_moment2, uint64_t *d_counters, void *stream);
int trt_nee_mis_pick_launch_plan(const trt_scene *s, uint32_t n, uint32_t compute_units, trt_query_plan *out);

/* ---- Sample queries: every sample's colour and first direction, and the device fold of those records ----
 * Every query above traces K samples per item and returns only their fold.  A caller with an estimator of its own (median of means, a
 * clamp against fireflies, an outlier test, a histogram) or a projection of its own (more SH bands, an octahedral map, spherical
 * Gaussians, moments) needs the samples; and the fold pins an item's K samples to one lane, so that the launch rule gives a wave 256
 * items whatever K is.  A sample query gives every SAMPLE a lane, writes that sample's colour and on request its first ray's direction,
 * and trt_fold_samples turns the colours into exactly the bytes trt_radiance / trt_gather would have written.
 *  - Stream index.  K = path.samples_per_ray; [b, e) = [sample_begin, sample_end), sample_end == 0 meaning K; R = e - b.  Sample s of item i
 *    has stream index j = first_stream + i * K + s: the numbering of every other query.
 *  - First ray.  TRT_SAMPLE_RAYS: item i as given, as in trt_radiance.  COSINE, CONE: trt_gather's draw for that lobe and `spread`, bit
 *    for bit.  SPHERE, HEMISPHERE: trt_probe's draw for that domain, bit for bit.  The last four draw on RNG (seed, j, 1).
 *  - Colour.  c = CpuSampler::single_point_sampling (cpu.rs:39-65) for that ray on RNG (seed, j, 0) with budget max_bounces: exactly
 *    what the folding queries fold for stream j.
 *  - Outputs.  colors[3 * (i * K + s) ..] = c.  With `directions` not NULL, directions[3 * (i * K + s) ..] = the traced ray's stored
 *    direction: RAYS: the item's direction as given; otherwise what Ray::new left (ray.rs:12-14), the d of the probe contract.  Both
 *    buffers hold n x K x 3 f32 whatever the range.  Entries of samples outside [b, e) are never written, and no byte outside
 *    [0, 12 n K) of either buffer is: calls over disjoint ranges fill one buffer, and a split by items (items [a, n) with
 *    first_stream + a * K, the buffers advanced by 3 a K floats) leaves the bytes of one call.
 *  - Nothing to trace.  An empty range touches nothing.  With max_bounces == 0 the colours of the range become +0, the colour the
 *    reference returns; `directions` is not written, and samples / rays are counted as trt_gather counts them for that call: 0.
 *  - stats / d_counters (samples and rays only): what trt_radiance / trt_gather / trt_probe report for the same items, range and
 *    parameters.  kernel_ms and `d_counters` as in trt_radiance.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG: a NULL params; trt_radiance's own errors, applied to `path` with `colors` as the
 *    required buffer; accumulate != 0 (a record is written, never added to); a source outside 0..4; with CONE a spread that is negative,
 *    infinite or NaN; a non-zero reserved word; n * R > 2^32 - 1.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the host form's buffers.
 *    n == 0 succeeds and touches nothing, with or without a device.
 *  - Order, coherence and concurrency.  The n * R samples of the call are numbered q = i' * R + s', and a wave works through a contiguous
 *    run of q: the samples of an item travel together, then the next item's.  Nothing is sorted.  Concurrency as for the ray queries.
 * trt_samples: HOST buffers, synchronous, staged as trt_gather's; a call that leaves records of the buffers alone (R < K, or
 * max_bounces == 0) uploads the caller's buffers first, so what it does not write comes back as it was.
 * trt_samples_device: buffers in HBM, asynchronous on `stream`; allocates nothing. */
enum trt_sample_source { TRT_SAMPLE_RAYS = 0, TRT_SAMPLE_COSINE = 1, TRT_SAMPLE_CONE = 2,   /* = enum trt_passes_source */
                         TRT_SAMPLE_SPHERE = 3, TRT_SAMPLE_HEMISPHERE = 4 };                /* trt_probe's two domains */
typedef struct {
    trt_radiance_params path;     /* K, max_bounces, background, seed, sample range, first_stream: trt_radiance's rules and errors;
                                     accumulate must be 0 (TRT_ERR_INVALID_ARG): a record is written, never added to */
    uint32_t source;              /* enum trt_sample_source */
    float spread;                 /* CONE only: trt_gather's rule and error; not read otherwise */
    uint32_t reserved[6];         /* zero */
} trt_samples_params;             /* 96 B: offsets 0, 64, 68, 72 */
void trt_samples_params_default(trt_samples_params *out);   /* path = trt_radiance_params_default, COSINE; NULL tolerated */
int trt_samples(trt_scene *s, const trt_ray *items, uint32_t n, const trt_samples_params *p, float *colors, float *directions,
                trt_stats *stats);
int trt_samples_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_samples_params *p, float *d_colors,
                       float *d_directions, uint64_t *d_counters, void *stream);
/* How trt_samples[_device] launches n items with a range of range_length = R samples on this scene: trt_gather_launch_plan's rule and
 * fields over the sample kernels' own table with n * R in the place of n - rays_per_wave = samples a wave owns, 256 or more once
 * ceil(n * R / 256) exceeds wave_slots.  n * R > 2^32 - 1 is TRT_ERR_INVALID_ARG. */
int trt_samples_launch_plan(const trt_scene *s, uint32_t n, uint32_t range_length, uint32_t compute_units, trt_query_plan *out);
/* The fold of sample records: for every item, over the samples of [b, e) in order, with inv_K = 1.0f / float(K), all f32, one IEEE
 * operation per operator, nothing fused:
 *   radiance.ch = radiance.ch + c.ch * inv_K;   moment2.ch = moment2.ch + (c.ch * c.ch) * inv_K
 * where c = colors[3 * (i * K + s) ..].  Of `p` only samples_per_ray, sample_begin, sample_end and accumulate are read (and the reserved
 * words, which must be zero).  The sums start from 0, or from the buffers with accumulate; `moment2` may be NULL.  An empty range zeroes
 * the n entries unless accumulate.  `colors` holds n x K x 3 f32, `radiance` and `moment2` n x 3; no other byte is written.
 * IDENTITY.  For source RAYS, COSINE or CONE, max_bounces > 0 and any split of [0, K) into ranges, trt_fold_samples over the records of
 * trt_samples leaves in `radiance` / `moment2` the bytes trt_radiance / trt_gather leave for the same items and parameters (a split
 * folded range by range with accumulate).  For SPHERE / HEMISPHERE the records and directions, folded by the probe fold above
 * (t = b_k(d) * inv_K; sh[k].ch = sh[k].ch + c.ch * t, a sample whose direction or point has a NaN adding nothing), give trt_probe's
 * bytes: trt_project_samples below is that fold on the device.  (Every number by its bits; a sum that is NaN is NaN in both, with a sign and payload that are not fixed.)  This is the K-aware
 * route: the paths run a sample to a lane, and the serial chain the fold's order demands is a few operations per sample.
 * No scene handle, like trt_variance.  The outputs must not overlap `colors`: the device form checks this from the sizes above
 * (TRT_ERR_INVALID_ARG), as trt_denoise_device checks its buffers.  Errors, TRT_ERR_INVALID_ARG: a NULL `p`; K == 0 or a bad range; with
 * n > 0 a NULL `colors` or `radiance`; a non-zero reserved word.  Then TRT_ERR_NO_DEVICE; n == 0 succeeds and touches nothing.
 * trt_fold_samples: HOST buffers, synchronous (uploads, runs the device kernel, downloads; there is no CPU path).
 * trt_fold_samples_device: buffers in HBM on the calling thread's current device, asynchronous on `stream`; allocates nothing. */
int trt_fold_samples(const float *colors, uint32_t n, const trt_radiance_params *p, float *radiance, float *moment2);
int trt_fold_samples_device(const float *d_colors, uint32_t n, const trt_radiance_params *p, float *d_radiance, float *d_moment2,
                            void *stream);
/* The PROBE fold of sample records: what trt_fold_samples is to trt_radiance / trt_gather, for trt_probe.  For every item, over the
 * samples of [b, e) in order, with inv_K = 1.0f / float(K), c = colors[3 * (i * K + s) ..], d = directions[3 * (i * K + s) ..] and the
 * basis b_k(d) exactly as the probe contract above parenthesises it:
 *   t = b_k * inv_K;   sh[k].ch = sh[k].ch + c.ch * t        for k < C = bands * bands
 * all f32, one IEEE operation per operator, nothing fused.
 *  - Fields read.  Of `p` only path.samples_per_ray (K), path.sample_begin, path.sample_end (0 = K), path.accumulate and bands (1..3) are
 *    read, and both reserved arrays, which must be zero.  `domain` is not read, nor any other field of `path`.
 *  - A sample that adds nothing.  A sample whose d has a NaN component adds nothing, neither 0 nor NaN.  With `items` not NULL (n x
 *    trt_ray; only items[i].origin, the point, is read) every sample of an item whose point has a NaN component adds nothing either:
 *    the rule under which the result is trt_probe's.  `items` may be NULL.  An item none of whose samples folds keeps the exact bits of
 *    its prior sums with accumulate, -0 and a NaN's payload included - no arithmetic touches them; without accumulate it is +0.
 *  - Layout.  `colors` and `directions` hold n x K x 3 f32 and are read only; `sh` holds n x C x 3 f32, item-major, then coefficient,
 *    then channel, and the bytes of coefficient k do not depend on `bands`.  The sums start from 0, or from `sh` with accumulate.  An
 *    empty range zeroes [0, 12 C n) unless accumulate, which touches nothing.  No byte outside [0, 12 C n) of `sh` is written.
 *  - IDENTITY.  For source SPHERE or HEMISPHERE, max_bounces > 0 and any split of [0, K) into ranges, trt_project_samples over the
 *    colours and directions of trt_samples, with the items, leaves in `sh` the bytes trt_probe leaves for the same items and parameters
 *    (a split folded range by range with accumulate; a NaN sum is NaN in both, with a sign and payload that are not fixed).
 *  - Errors, before any device work, all TRT_ERR_INVALID_ARG, in this order: a NULL `p`; K == 0 or a bad range; `bands` outside 1..3; a
 *    non-zero reserved word; with n > 0 a NULL `colors`, `directions` or `sh`.  The device form then refuses an `sh` that overlaps either
 *    record buffer (from the sizes above, as trt_fold_samples_device).  Then TRT_ERR_NO_DEVICE; n == 0 succeeds and touches nothing,
 *    with or without a device.
 * No scene handle, like trt_fold_samples.
 * trt_project_samples: HOST buffers, synchronous (uploads, runs the device kernel, downloads; there is no CPU path).
 * trt_project_samples_device: buffers in HBM on the calling thread's current device, asynchronous on `stream`; allocates nothing. */
int trt_project_samples(const float *colors, const float *directions, const trt_ray *items, uint32_t n, const trt_probe_params *p,
                        float *sh);
int trt_project_samples_device(const float *d_colors, const float *d_directions, const trt_ray *d_items, uint32_t n,
                               const trt_probe_params *p, float *d_sh, void *stream);
/* trt_probe's contract with a launch that fills the device whatever K is: the paths run a sample to a lane (trt_samples' kernels for
 * SPHERE / HEMISPHERE, with directions) into a record buffer and trt_project_samples folds the records.
 *  - Results.  `sh`, stats.samples / d_counters[samples] and stats.rays / d_counters[rays] are trt_probe's, bit for bit, for the same
 *    arguments: sample ranges, accumulate, first_stream, both split invariances, the NaN rules and "nothing to trace" (an empty range
 *    or max_bounces == 0: zero unless accumulate, and no sample launch) included.
 *  - Chunks.  With K = path.samples_per_ray and R the range's length, the call runs chunks of
 *      m = min(n, record_bytes / (24 K), (2^32 - 1) / R)
 *    items: the sample kernels for items [a, a + m) on the streams from first_stream + a K, then the projection of those records into
 *    rows [a, a + m) of `sh` with the caller's accumulate.  Within the record buffer a chunk's colours come first (12 K bytes per item
 *    of the chunk), then its directions.  No byte of the record buffer beyond 24 K m is touched.
 *  - Errors, TRT_ERR_INVALID_ARG before any device work: trt_probe's, in trt_probe's order; then, with n > 0, m == 0 (the message says
 *    how many bytes one item needs); for the device form a NULL `d_records`, and a `d_sh` that overlaps the 24 K m bytes of the record
 *    buffer.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the host form's buffers.  n == 0 succeeds and touches nothing.
 * trt_probe_parallel: HOST buffers, synchronous, staged as trt_probe's.  The record buffer is the call's own, allocated with its staging
 *   (24 K m bytes) and freed by it.  record_bytes == 0 means the library's default: 96 MiB - the records of 4 Mi samples, eight times
 *   the 524 288 samples that fill the wave slots of a 256-CU device at the sample kernels' 8 waves per SIMD, so that a chunk's launch has a
 *   tail of several rounds to even out - or one item's 24 K bytes where that is more.  Chosen by that reasoning, not swept.  kernel_ms
 *   covers all launches of the call, from the first to the last.
 * trt_probe_parallel_device: buffers in HBM, `d_records` the caller's scratch of record_bytes bytes; allocates nothing, and everything is
 *   enqueued on `stream` in order. */
int trt_probe_parallel(trt_scene *s, const trt_ray *items, uint32_t n, const trt_probe_params *p, float *sh, trt_stats *stats,
                       uint64_t record_bytes);
int trt_probe_parallel_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_probe_params *p, float *d_sh,
                              uint64_t *d_counters, void *d_records, uint64_t record_bytes, void *stream);
/* How trt_probe_parallel[_device] launches the sample kernels of ONE chunk of n items with a range of range_length = R samples: exactly
 * trt_samples_launch_plan's answer for (n, R), errors included.  (The projection behind it is a lane per item, or a wave per item where
 * R >= 64 and n <= 4096.) */
int trt_probe_parallel_launch_plan(const trt_scene *s, uint32_t n, uint32_t range_length, uint32_t compute_units, trt_query_plan *out);

/* ---- Sample-parallel next-event queries: every sample's colour of trt_nee / trt_nee_mis / trt_nee_pick / trt_nee_mis_pick ----
 * The four next-event queries trace K samples per item and return only their fold, a lane owning an item for all K.  trt_nee_samples
 * is to them what trt_samples is to trt_radiance / trt_gather: a lane owns one SAMPLE, the call writes that sample's colour and on
 * request its first ray's direction, and trt_fold_samples turns the colours into the folding query's bytes.  A caller with a robust
 * estimator of its own (median of means, a clamp against the 1 / d^2 tail) gets the samples; a caller that wants the sums gets them
 * from a launch that fills the device whatever K is.
 *  - Which query.  `weighted` and `pick` select the sibling: weighted == 0 and pick == NULL: trt_nee; weighted == 1 and pick == NULL:
 *    trt_nee_mis; weighted == 0 and pick != NULL: trt_nee_pick; weighted == 1 and pick != NULL: trt_nee_mis_pick, whose `total_power`
 *    argument is p->total_power.  p->query.nee is read always and means what it means to trt_nee; p->query.heuristic and
 *    p->query.reserved are read only when weighted != 0; total_power only when weighted != 0 and pick != NULL.
 *  - Stream index.  K = samples_per_ray of p->query.nee.gather.path; [b, e) = [sample_begin, sample_end), sample_end == 0 meaning K;
 *    R = e - b.  Sample s of item i has stream index j = first_stream + i * K + s: the numbering of every other query.
 *  - Colour.  colors[3 * (i * K + s) ..] = the colour the sibling folds for sample s of item i, BIT FOR BIT: the path on (seed, j, 0),
 *    a drawn first ray on (seed, j, 1), the vertex draws on (seed, j, 2 + d), the hiding of diffusely reached lights, the last-vertex
 *    rule, source_is_diffuse, shadow_end, the alias clamp, and the weights wl / wb with the weighted form's csh: all the sibling's.  The
 *    sources are trt_nee's three (TRT_PASSES_RAYS, _COSINE, _CONE).
 *  - Direction.  With `directions` not NULL, directions[3 * (i * K + s) ..] = the first ray's stored direction, as trt_samples writes it.
 *  - Ranges.  Both buffers hold n x K x 3 f32 whatever the range.  Only the records of [b, e) are written, and no byte outside
 *    [0, 12 n K) of either buffer is: calls over disjoint ranges fill one buffer, and a split by items (items [a, n) with
 *    first_stream + a * K, the buffers advanced by 3 a K floats) leaves the bytes of one call.  An empty range touches nothing.  With
 *    max_bounces == 0 the colours of the range become +0 and `directions` is not written; samples and rays are counted 0, as the
 *    siblings count them.
 *  - stats / d_counters (samples and rays only) count the n x R samples of the range; rays are the sibling's for the same range: the
 *    path walks plus the shadow walks.  An empty shadow range and a dead sample walk nothing.  kernel_ms and `d_counters` as in trt_nee.
 *  - Errors, before any device work, TRT_ERR_INVALID_ARG, IN THIS ORDER: a NULL `p`; (1) trt_nee's own errors in trt_nee's order,
 *    applied to p->query.nee with `colors` as the required buffer, as far as its table size, shadow_end, source_is_diffuse and reserved
 *    words; (2) accumulate != 0 (a record is written, never added to: trt_samples' rule and message); (3) weighted > 1; (4) when
 *    weighted, trt_nee_mis' own fields: the heuristic, then p->query.reserved; (5) a non-zero word of p->reserved; (6) n * R > 2^32 - 1;
 *    (7) the table checks of the sibling that (weighted, pick != NULL) selects, unchanged and in the sibling's order - trt_nee: the
 *    emitter records; trt_nee_mis: the emitter records, the table rule; trt_nee_pick: the emitter records, the pick records;
 *    trt_nee_mis_pick: the emitter records, the pick records, the table rule, total_power, prob by bits.  THE HOST FORM READS THE
 *    TABLES; THE DEVICE FORM CHECKS ONLY WHAT THE SIBLINGS' DEVICE FORMS CHECK, and a wrong pick table's reads stay inside the E
 *    records of either table, as theirs do.  Then TRT_ERR_NO_DEVICE, then TRT_ERR_OOM for the host form's buffers.  n == 0 succeeds
 *    and touches nothing, with or without a device.
 *  - Order, coherence and concurrency as in trt_samples: the n * R samples are numbered q = i' * R + s', a wave works through a
 *    contiguous run of q.
 * IDENTITY.  For max_bounces > 0 and any split of [0, K) into ranges, trt_fold_samples over the records of trt_nee_samples leaves in
 * `radiance` / `moment2` the bytes the folding query - trt_nee, trt_nee_mis, trt_nee_pick or trt_nee_mis_pick, by (weighted, pick) -
 * leaves for the same arguments (a split folded range by range with accumulate), and stats agree.  Every number by its bits.  It holds
 * because the next-event kernels' fold is trt_radiance's, operator for operator.  The n x K x 12 bytes of records are the caller's
 * memory.  A split of the range folds part by part with accumulate into the same sums but does not shrink the buffer, which holds
 * n x K records whatever the range; a caller short of memory splits by ITEMS, tracing and folding one chunk of items after the other
 * through one buffer of chunk x K records.
 * trt_nee_samples: HOST buffers, synchronous, staged as trt_samples' (items, colours, directions, counters) with the emitter table and
 * the pick table in the call's one device allocation; a call that leaves records of the buffers alone (R < K, or max_bounces == 0)
 * uploads the caller's buffers first, so what it does not write comes back as it was.
 * trt_nee_samples_device: buffers and tables in HBM, asynchronous on `stream`; allocates nothing. */
typedef struct trt_nee_samples_params {
    trt_nee_mis_params query;     /* 160 B.  query.nee is read always and means what it means to trt_nee; query.heuristic and
                                     query.reserved are read only when weighted != 0 (reserved must then be 0) */
    uint32_t weighted;            /* 0: the sample of trt_nee / trt_nee_pick; 1: of trt_nee_mis / trt_nee_mis_pick */
    float    total_power;         /* read only when weighted != 0 and pick != NULL (trt_nee_mis_pick's argument) */
    uint32_t reserved[6];         /* zero */
} trt_nee_samples_params;         /* 192 B: offsets 0, 160, 164, 168 */
void trt_nee_samples_params_default(trt_nee_samples_params *out);   /* query = trt_nee_mis_params_default's, weighted 0, total_power 0;
                                                                       NULL tolerated */
int trt_nee_samples(trt_scene *s, const trt_ray *items, uint32_t n, const trt_emitter *emitters,
                    const trt_emitter_pick *pick /* NULL: uniform choice */, uint32_t n_emitters, const trt_nee_samples_params *p,
                    float *colors, float *directions /* NULL: not wanted */, trt_stats *stats);
int trt_nee_samples_device(trt_scene *s, const trt_ray *d_items, uint32_t n, const trt_emitter *d_emitters,
                           const trt_emitter_pick *d_pick, uint32_t n_emitters, const trt_nee_samples_params *p, float *d_colors,
                           float *d_directions, uint64_t *d_counters, void *stream);
/* How trt_nee_samples[_device] launches n items with a range of range_length = R samples on this scene: trt_nee_launch_plan's rule and
 * fields over the sample-parallel next-event kernels' own table for (weighted, pick), each 0 or not, with n * R in the place of n -
 * rays_per_wave = samples a wave owns, 256 or more once ceil(n * R / 256) exceeds wave_slots.  n * R > 2^32 - 1 is
 * TRT_ERR_INVALID_ARG. */
int trt_nee_samples_launch_plan(const trt_scene *s, uint32_t n, uint32_t range_length, uint32_t weighted, uint32_t pick,
                                uint32_t compute_units, trt_query_plan *out);

/* ---- Denoising a frame with its feature buffers: an edge-avoiding a-trous wavelet filter ----
 * Takes the frame as trt_render leaves it (`color`, 3 f32 per pixel, required) and the guides as trt_render_aov writes them (`albedo`
 * and `normal` 3 f32, `depth` 1 f32; each optional, NULL switches its term off), all row-major height x width, and writes `out`
 * (3 f32 per pixel).  The weights come from the guides only.  Every output bit is determined: all arithmetic is f32, one IEEE operation
 * per operator below, nothing fused, division correctly rounded, f32 denormals kept (0.5^128 is a denormal weight and occurs).
 *
 * Pass i = 0 .. iterations-1 has step = 1 << i, reads image c_i (c_0 = color) and writes c_{i+1}; the last one is `out`.  For pixel
 * p = (x, y) the 25 taps are q = (x + dx*step, y + dy*step), dy = -2..2 outer, dx = -2..2 inner, h = {0.0625, 0.25, 0.375, 0.25, 0.0625}.
 * A tap outside the image is skipped.  w = h[dy+2] * h[dx+2]; then, for every tap but the centre (dx == dy == 0), in this order:
 *   normal given:    d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  d = d > 0 ? d : 0;  normal_power_log2 times d = d*d;  w = w*d
 *   albedo term on:  da = a_p - a_q;  e = (da.r*da.r + da.g*da.g) + da.b*da.b;  m = 1 - e*inv_a;  m = m > 0 ? m : 0;  w = w*(m*m)
 *                    with inv_a = 1 / (sigma_albedo*sigma_albedo), computed once
 *   depth term on:   dz = z_p - z_q;  m = 1 - ((dz*dz) * inv_z(p)) * (1.0f / float(dx*dx + dy*dy));  m = m > 0 ? m : 0;  w = w*(m*m)
 *                    with inv_z(p) = 1 / (s*s), s = (sigma_depth * z_p) * float(step): one division per pixel and pass - a relative
 *                    depth change per pixel of tap distance; a miss pixel (z_p = 0) gives inf / NaN, which the comparison turns into 0
 * A tap is taken only if w > 0 (a zero or NaN weight adds nothing, not 0 * c): acc.c = acc.c + w * c_q.c per channel, ws = ws + w.  The
 * centre tap is always taken, so ws > 0; r = 1 / ws, out.c = acc.c * r.  A term is on when its buffer is given and, for albedo and
 * depth, its sigma is > 0.
 * Consequences: a pixel whose normal is 0 (every sample missed) keeps its colour (to the rounding of (w*c) * (1/w)); a NaN guide removes its taps and never poisons the
 * frame; a NaN colour spreads only through taps with positive weight.  The weights do not depend on the colour (no colour edge-stop:
 * with unknown variance it made a 4-spp frame worse; trt_denoise_ex below has one, scaled by the variance) and the albedo is not divided out (it is constant per material here).
 * Whole frames only: a band of a sharded render has no neighbours across its seams, so bands and several GPUs are out of scope - gather
 * the frame and its buffers first.  width and height are at most 65536.
 *
 * trt_denoise: HOST buffers, synchronous; uploads, runs the device kernels, downloads.  There is no CPU path.
 * trt_denoise_device: buffers in HBM on the calling thread's current device (the struct itself is read on the host, during the call),
 * asynchronous on `stream`; allocates nothing - the ping-pong images and the packed guides live in `d_scratch`, at least
 * trt_denoise_scratch_bytes(width, height, params) bytes (host arithmetic, needs no device; 0 for invalid arguments); any alignment.  The
 * inputs are not written.  params == NULL means the defaults.  Both take no scene handle, like trt_tonemap_u8_device.
 * Errors: TRT_ERR_INVALID_ARG before any device work - a NULL `in`, `color` or `out`, width or height 0 (or above 65536), iterations
 * outside 1..8, normal_power_log2 above 10, a NaN sigma, a non-zero reserved word, an output that overlaps an input, for the device form
 * a NULL scratch or one smaller than required - then TRT_ERR_NO_DEVICE or TRT_ERR_OOM. */
typedef struct {
    uint32_t iterations;          /* 1..8 (default 4): passes, steps 1, 2, 4, ... */
    uint32_t normal_power_log2;   /* 0..10 (default 7): the normal stop is max(n_p . n_q, 0)^(2^this) */
    float sigma_albedo;           /* default 0.1; <= 0 switches the albedo term off */
    float sigma_depth;            /* default 0.05; <= 0 switches the depth term off */
    uint32_t reserved[4];         /* zero */
} trt_denoise_params;             /* 32 B */
void trt_denoise_params_default(trt_denoise_params *out);
typedef struct {
    const float *color;           /* 3 f32 per pixel: the frame (required) */
    const float *albedo;          /* 3 f32 per pixel, or NULL */
    const float *normal;          /* 3 f32 per pixel, or NULL */
    const float *depth;           /* 1 f32 per pixel, or NULL */
} trt_denoise_inputs;             /* 32 B */
uint64_t trt_denoise_scratch_bytes(uint32_t width, uint32_t height, const trt_denoise_params *params);
int trt_denoise(const trt_denoise_inputs *in, uint32_t width, uint32_t height, const trt_denoise_params *params, float *out);
int trt_denoise_device(const trt_denoise_inputs *d_in, uint32_t width, uint32_t height, const trt_denoise_params *params,
                       float *d_out, void *d_scratch, uint64_t scratch_bytes, void *stream);

/* ---- The same filter with a variance-guided colour stop ----
 * trt_denoise's weights ignore the colour, so what the guides do not show - a shadow edge, the falloff of the light on a wall, a
 * reflection - is blurred by the same amount at 4 and at 4096 samples per pixel.  trt_denoise_ex adds one more stop, scaled by the
 * variance of each pixel's estimate (trt_variance): it backs off as the frame converges.  `color` == NULL, `variance` == NULL or
 * sigma_color <= 0 switch the term off: the output is then trt_denoise's, byte for byte.  With the term on, all f32, one IEEE operation
 * per operator, nothing fused:
 *   prefilter (once): v_0(p) = sv * (1.0f / sw), with sv = sv + k*variance_q and sw = sw + k accumulated from 0 over the taps
 *                    q = (x + dx, y + dy), dy = -1..1 outer, dx = -1..1 inner, that lie inside the image, k = b[dy+1] * b[dx+1],
 *                    b = {0.25, 0.5, 0.25} (at 4 spp a single pixel's variance is itself an estimate from 4 numbers)
 *   pass i, for every tap but the centre, after the depth term, on that pass's input image c_i:
 *                    dc = c_p - c_q;  e = (dc.r*dc.r + dc.g*dc.g) + dc.b*dc.b;  m = 1 - e*inv_c(p);  m = m > 0 ? m : 0;  w = w*(m*m)
 *                    with inv_c(p) = 1 / ((sigma_color*sigma_color) * v_i(p)): one division per pixel and pass
 *   propagation:     beside acc and ws, va = va + (w*w) * v_i(q) over the taken taps (the centre among them), from 0;
 *                    v_{i+1}(p) = va * (r*r) with r = 1 / ws: the variance of the weighted mean, were the taps independent.  Without it
 *                    later passes would compare smoothed colours against the raw variance and the stop would go slack.
 * Consequences: v_i(p) = +inf gives inv_c = 0, every m = 1 for a finite e, the term multiplies by 1 and the pass is trt_denoise's, bit
 * for bit.  v_i(p) = 0 gives inv_c = inf, every neighbour's m is -inf or NaN, then 0: a converged pixel keeps its colour (to the
 * rounding of (w*c) * (1/w)) and its v stays 0.  A NaN v_i(p) likewise keeps the pixel.  The prefilter spreads an inf or NaN of
 * `variance` to the 3 x 3 around it, and the propagation carries a NaN v to every pixel that takes a tap on it: those are kept from the
 * next pass on.  That also limits the first consequence over SEVERAL passes: a taken tap whose w*w underflows to 0 (w below about 2^-75:
 * an edge pixel's normal stop) gives 0 * inf = NaN.  A 1-spp frame (trt_variance writes +inf everywhere) therefore comes out as from
 * trt_denoise after one pass, but after four passes only where no such tap was in reach - on a 4-spp Cornell frame with v = +inf, 43 %
 * of the pixels.  At 1 spp pass no variance.
 * Scratch: trt_denoise_scratch_bytes, unchanged - v_i rides in the unused fourth word of the 16-byte colour records.
 * Errors, besides trt_denoise's: a NaN sigma_color, a non-zero reserved word, an output that overlaps `variance`. */
typedef struct {
    const float *variance;        /* 1 f32 per pixel as trt_variance writes it, or NULL: term off */
    float sigma_color;            /* <= 0: term off; NaN: TRT_ERR_INVALID_ARG */
    uint32_t reserved[5];         /* zero */
} trt_denoise_color;              /* 32 B */
void trt_denoise_color_default(trt_denoise_color *out);
int trt_denoise_ex(const trt_denoise_inputs *in, const trt_denoise_color *color, uint32_t width, uint32_t height,
                   const trt_denoise_params *params, float *out);
int trt_denoise_ex_device(const trt_denoise_inputs *d_in, const trt_denoise_color *color, uint32_t width, uint32_t height,
                          const trt_denoise_params *params, float *d_out, void *d_scratch, uint64_t scratch_bytes, void *stream);

/* Imager finalisation + Image -> RgbImage (imager.rs:52-53; utils/image.rs:92-111): c^(1/gamma),
 * clamp to [0, 0.999], *255, truncate; NaN -> 0.  HOST buffers, npixels*3 each. */
int trt_tonemap_u8(const float *accum, uint32_t npixels, float gamma, uint8_t *rgb);

/* The same on buffers resident in HBM (device pointers), asynchronous on `stream` (a hipStream_t, NULL = default): the
 * frame never has to leave the GPU as f32.  Host form and device kernel evaluate c^(1/gamma) with the same function (trt-math v2
 * powf, csrc/trt_pow.h): their u8 frames are equal byte for byte.  Against the reference, which calls the platform's libm powf
 * (utils/image.rs:94-96), a channel may differ by one least-significant bit where that powf is not correctly rounded. */
int trt_tonemap_u8_device(const float *d_accum, uint32_t npixels, float gamma, uint8_t *d_rgb, void *stream);

/* How the streamed backend launches a render of this scene with these settings (host arithmetic only: works without a GPU).
 * The kernels' view of their dynamic LDS - scene copy | postponed-leaf stack (threads x leaf_slots x 8 B) | ray pool (36 B per
 * lane) - is decided in ONE place (csrc/stream_plan.h: LdsLayout and the stages of streamed_launch_plan) and reported here, so that its
 * invariants can be checked for every scene size and every tuning knob without a device (tests/test_host_boundary.py, tests/test_stream_plan.py). */
typedef struct {
    uint32_t scene_mode;              /* 0 scene read from global memory, 1 whole hot scene copied into LDS */
    uint32_t threads_per_workgroup, waves_per_simd, workgroups_per_cu;
    uint32_t lds_bytes, scene_lds_bytes;      /* dynamic LDS per workgroup; the scene copy's share */
    uint32_t leaf_slots, lds_leaf_stack, ray_pool;
    uint32_t walk;                    /* 1 tree walk with LDS leaf stack, 2 lock-step leaf list, 3 16-byte nodes, 5 tree walk with register slots */
    uint32_t specialised;             /* 1: a kernel with the walk fixed at compile time */
    uint32_t has_kernel;              /* 0 would be a bug: no instantiation for the plan (the launch then fails, it never falls back) */
    uint32_t kernel_waves_per_simd, kernel_threads, kernel_walk /* 0 = chosen at run time */, kernel_ray_pool, kernel_counting;
    uint32_t chunk_spp;               /* samples per pixel per launch under p->tuning (= trt_streamed_chunk_spp(width, rows) for the default tuning) */
    uint32_t dual_walk;               /* 1: two paths per lane (two leaf stacks per lane in LDS) */
    uint64_t workspace_bytes;         /* device scratch one render of this size takes from the scene's pool */
} trt_launch_plan;
int trt_streamed_launch_plan(const trt_scene *s, const trt_camera *cam, const trt_render_params *p, trt_launch_plan *out);

/* Samples per pixel the streamed backend traces per kernel launch for an image of this size under the default tuning (it splits
 * longer sample ranges into such chunks; one chunk = one tracing-kernel launch + one fold launch).  For another tuning:
 * trt_streamed_launch_plan's chunk_spp. */
uint32_t trt_streamed_chunk_spp(uint32_t width, uint32_t rows);

/* Measurement aid: between _begin and _end every launch of a render's dominant kernel (streamed backend: the sample
 * kernel, not the fold) is bracketed by HIP events on the stream it is launched on; _end waits for them and returns the
 * summed device time and the number of launches.  Process-wide switch; a launch's two events are paired on the host thread
 * that makes the launch, so renders on several threads, streams or devices (trt_render_multi) never mix their brackets. */
int trt_kernel_timing_begin(void);
int trt_kernel_timing_end(double *total_ms, uint32_t *launches);

/* Name of the GPU kernel that dominates a render of this scene with these settings ("trt::stream_pool_kernel", ...): what
 * a kernel trace of the call shows, for profiles and benchmark records.  "" on invalid arguments. */
const char *trt_dominant_kernel(const trt_scene *s, const trt_camera *cam, const trt_render_params *p);

/* The lock-step kernel compiled per scene at run time (environment TRT_FLAT_LITERAL: 0 never, 1 at the first streamed render of a scene,
 * unset: at the first render call of 2^26 samples or more): a scene of at most 32 primitives gets its own build of the streamed kernel
 * with its leaf planes as literals in the instruction stream - the same frame, bit for bit, faster.  The compiler (hiprtc) is looked for
 * at run time; if it is missing, or compiling or loading fails, the scene renders through the built-in kernel and no call fails.
 * _compilations: compilations this process has started.  _diagnostic: why the last one that failed did, "" if none has (the string is
 * the calling thread's until its next call). */
uint64_t trt_flat_literal_compilations(void);
const char *trt_flat_literal_diagnostic(void);
/* What that kernel is told about its scene besides the planes (environment TRT_SCENE_FACTS: 0 nothing, 1 "no sphere" and the kinds as
 * compile-time constants, unset or anything else: those and the straight-line shade of scenes with Lambertian and light quads only; bits
 * 1 to 3 are reported and stay run-time switches in the kernel).  Each fact is claimed only
 * where the packed scene proves it; the frame is the same, bit for bit, whatever is claimed.  One word: bit 0 no sphere, bit 1 every quad
 * axis-exact (and no sphere), bit 2 the nearest-first leaf phase (with bit 1), bit 3 lazy colour, bit 4 the straight-line shade,
 * bits 8 ... 11 the trt_material_kind values some primitive references (0: not claimed).  0 for NULL, a scene of more than 32 primitives
 * and TRT_SCENE_FACTS=0.  Host only, needs no device. */
uint32_t trt_scene_facts(const trt_scene *s);
/* The same word for the unit this process compiled and loaded last: the facts its source was written with (0 before any, and for a
 * unit compiled without facts).  After a scene's first streamed render with TRT_FLAT_LITERAL=1 it equals trt_scene_facts(scene). */
uint32_t trt_flat_literal_facts(void);

/* ---- library ---- */
const char *trt_last_error(void);
int trt_device_count(void);               /* gfx950 devices visible; 0 without a GPU (never an error) */
int trt_set_device(int ordinal);          /* device used by this thread's later calls */
uint32_t trt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TINYRT_H */
