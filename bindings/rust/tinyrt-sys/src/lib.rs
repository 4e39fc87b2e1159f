//! Raw declarations of `include/tinyrt.h` (ABI version 3).  Field order, scalar types and function parameter lists are
//! checked against the header by tests/test_rust_bindings.py; the crate itself has never been compiled (no Rust
//! toolchain in the build image).
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

pub const TRT_ABI_VERSION: u32 = 4;

// enum trt_status
pub const TRT_OK: c_int = 0;
pub const TRT_ERR_INVALID_ARG: c_int = -1;
pub const TRT_ERR_DUPLICATE: c_int = -2;
pub const TRT_ERR_NOT_FOUND: c_int = -3;
pub const TRT_ERR_HIP: c_int = -4;
pub const TRT_ERR_NO_DEVICE: c_int = -5;
pub const TRT_ERR_OOM: c_int = -6;

// enum trt_material_kind
pub const TRT_LAMBERTIAN: u32 = 0;
pub const TRT_METAL: u32 = 1;
pub const TRT_DIELECTRIC: u32 = 2;
pub const TRT_LIGHT: u32 = 3;

// enum trt_backend
pub const TRT_BACKEND_MEGAKERNEL: u32 = 0;
pub const TRT_BACKEND_WAVEFRONT: u32 = 1;
pub const TRT_BACKEND_AUTO: u32 = 2;
pub const TRT_BACKEND_STREAMED: u32 = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_vec3 {
    pub x: f32,
    pub y: f32,
    pub z: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_ray {
    pub origin: trt_vec3,
    pub direction: trt_vec3,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_sample_point {
    pub x: u32,
    pub y: u32,
    pub ray: trt_ray,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_sampled_color {
    pub x: u32,
    pub y: u32,
    pub color: trt_vec3,
}

/// The answer of a closest-hit query (28 bytes).  A miss: `t` = +inf, `geometry` = `material` = 0xFFFFFFFF, the rest 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_hit {
    pub t: f32,
    pub geometry: u32,
    pub material: u32,
    pub front_face: u32,
    pub normal: trt_vec3,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_material {
    pub kind: u32,
    pub albedo: trt_vec3,
    pub param: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_scene_info {
    pub num_nodes: u32,
    pub num_spheres: u32,
    pub num_quads: u32,
    pub num_materials: u32,
    pub max_depth: u32,
    pub device_bytes: u32,
    pub lds_bytes: u32,
    pub num_cull_nodes: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_camera {
    pub position: trt_vec3,
    pub viewport_upper_left: trt_vec3,
    pub forward: trt_vec3,
    pub horizontal: trt_vec3,
    pub vertical: trt_vec3,
    pub defocus_disk_u: trt_vec3,
    pub defocus_disk_v: trt_vec3,
    pub width: u32,
    pub height: u32,
}

/// Placement of a compiled scene (every value renders the same frames); fill with `trt_scene_options_default`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_scene_options {
    pub cull_prune: f32,
    pub flat_walk: i32,
    pub compact_nodes: i32,
    pub top_nodes: u32,
    pub scratch_cap_bytes: u64,
    pub reserved: [u32; 6],
}

/// Scheduling of a render (every value renders the same frame); fill with `trt_tuning_default`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_tuning {
    pub stream_waves_per_simd: u32,
    pub stream_big_threads: u32,
    pub stream_batch_spp: u32,
    pub radiance_gb: u32,
    pub leaf_slots: u32,
    pub lds_leaf_stack: u32,
    pub ray_pool: u32,
    pub stragglers: u32,
    pub lds_stragglers: u32,
    pub dual_walk: u32,
    pub runtime_walk: u32,
    pub xcd_remap: u32,
    pub mega_waves_per_simd: u32,
    pub mega_threads: u32,
    pub mega_global_waves8: u32,
    pub wf_waves_per_simd: u32,
    pub wf_serve_min: u32,
    pub reserved: [u32; 7],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct trt_render_params {
    pub samples_per_pixel: u32,
    pub max_bounces: u32,
    pub background: trt_vec3,
    pub seed: u32,
    pub backend: u32,
    pub sample_begin: u32,
    pub sample_end: u32,
    pub accumulate: u32,
    pub band_rows: u32,
    pub band_stride: u32,
    pub band_offset: u32,
    pub rows_local: u32,
    pub collect_stats: u32,
    pub tuning: *const trt_tuning,
}
impl Default for trt_render_params {
    fn default() -> Self {
        // all-zero: whole image, all samples, the library's default tuning (null)
        unsafe { std::mem::zeroed() }
    }
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_band_copy {
    pub rows_local: u32,
    pub full_bands: u32,
    pub tail_rows: u32,
    pub reserved: u32,
    pub band_bytes: u64,
    pub local_pitch: u64,
    pub frame_pitch: u64,
    pub frame_offset: u64,
    pub tail_bytes: u64,
    pub tail_local_offset: u64,
    pub tail_frame_offset: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_launch_plan {
    pub scene_mode: u32,
    pub threads_per_workgroup: u32,
    pub waves_per_simd: u32,
    pub workgroups_per_cu: u32,
    pub lds_bytes: u32,
    pub scene_lds_bytes: u32,
    pub leaf_slots: u32,
    pub lds_leaf_stack: u32,
    pub ray_pool: u32,
    pub walk: u32,
    pub specialised: u32,
    pub has_kernel: u32,
    pub kernel_waves_per_simd: u32,
    pub kernel_threads: u32,
    pub kernel_walk: u32,
    pub kernel_ray_pool: u32,
    pub kernel_counting: u32,
    pub chunk_spp: u32,
    pub dual_walk: u32,
    pub workspace_bytes: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_query_plan {
    pub scene_mode: u32,
    pub walk: u32,
    pub threads_per_workgroup: u32,
    pub kernel_waves_per_simd: u32,
    pub workgroups_per_cu: u32,
    pub leaf_slots: u32,
    pub stragglers: u32,
    pub lds_bytes: u32,
    pub scene_lds_bytes: u32,
    pub has_kernel: u32,
    pub fallback: u32,
    pub streamed_walk: u32,
    pub streamed_threads: u32,
    pub compute_units: u32,
    pub rays_per_wave: u32,
    pub workgroups: u32,
    pub wave_slots: u64,
    pub waves: u64,
}

/// Samples, depth, RNG numbering and sample range of `trt_radiance` (64 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_radiance_params {
    pub samples_per_ray: u32,
    pub max_bounces: u32,
    pub background: trt_vec3,
    pub seed: u32,
    pub sample_begin: u32,
    pub sample_end: u32,
    pub accumulate: u32,
    pub first_stream: u32,
    pub reserved: [u32; 6],
}

/// `enum trt_lobe`: the rule the first ray of a gather sample is drawn by.
pub const TRT_LOBE_COSINE: u32 = 1;
pub const TRT_LOBE_CONE: u32 = 2;

/// `trt_radiance_params` and the lobe of `trt_gather` (96 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_gather_params {
    pub path: trt_radiance_params,
    pub lobe: u32,
    pub spread: f32,
    pub reserved: [u32; 6],
}

/// One light of the table `trt_direct` samples (80 bytes): made by `trt_scene_emitters`, `trt_emitter_init_quad` or
/// `trt_emitter_init_sphere`; `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_emitter {
    pub kind: u32,
    pub geometry: u32,
    pub a: trt_vec3,
    pub b: trt_vec3,
    pub c: trt_vec3,
    pub normal: trt_vec3,
    pub color: trt_vec3,
    pub area: f32,
    pub reserved: [u32; 2],
}

/// `trt_radiance_params` (its `max_bounces` and `background` are not read) and the share of the distance to the emitter point the
/// shadow ray covers, for `trt_direct` (96 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_direct_params {
    pub path: trt_radiance_params,
    pub shadow_end: f32,
    pub reserved: [u32; 7],
}

/// `trt_gather_params` and the distance within which an occluder counts, for `trt_ambient` (128 bytes); `gather.path.max_bounces` and
/// `gather.path.background` are not read; `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_ambient_params {
    pub gather: trt_gather_params,
    pub max_distance: f32,
    pub reserved: [u32; 7],
}

/// `enum trt_sample_source`: where the first ray of a sample of `trt_samples` comes from (0 - 2 are `enum trt_passes_source`).
pub const TRT_SAMPLE_RAYS: u32 = 0;
pub const TRT_SAMPLE_COSINE: u32 = 1;
pub const TRT_SAMPLE_CONE: u32 = 2;
pub const TRT_SAMPLE_SPHERE: u32 = 3;
pub const TRT_SAMPLE_HEMISPHERE: u32 = 4;

/// `trt_radiance_params` (accumulate stays 0), the source of the first ray and the cone's spread of `trt_samples` (96 bytes); `reserved`
/// stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_samples_params {
    pub path: trt_radiance_params,
    pub source: u32,
    pub spread: f32,
    pub reserved: [u32; 6],
}

/// `enum trt_probe_domain`: the directions the first ray of a probe sample is drawn over.
pub const TRT_PROBE_SPHERE: u32 = 1;
pub const TRT_PROBE_HEMISPHERE: u32 = 2;

/// `trt_radiance_params`, the domain and the number of spherical-harmonic bands of `trt_probe` (96 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_probe_params {
    pub path: trt_radiance_params,
    pub domain: u32,
    pub bands: u32,
    pub reserved: [u32; 6],
}

/// `enum trt_passes_source`: where the first ray of a passes sample comes from; 1 and 2 are `enum trt_lobe`.
pub const TRT_PASSES_RAYS: u32 = 0;
pub const TRT_PASSES_COSINE: u32 = 1;
pub const TRT_PASSES_CONE: u32 = 2;

/// `trt_gather_params`, whose `lobe` is read as `enum trt_passes_source`, and the number of depth bins of `trt_passes` (128 bytes);
/// `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_passes_params {
    pub gather: trt_gather_params,
    pub depth_bins: u32,
    pub reserved: [u32; 7],
}

/// `trt_gather_params`, whose `lobe` is read as `enum trt_passes_source`, the share of the distance to the emitter point a shadow ray
/// covers and whether the first hit counts as reached by a diffuse scatter, for `trt_nee` (128 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_nee_params {
    pub gather: trt_gather_params,
    pub shadow_end: f32,
    pub source_is_diffuse: u32,
    pub reserved: [u32; 6],
}

pub const TRT_MIS_BALANCE: u32 = 0;
pub const TRT_MIS_POWER: u32 = 1;

/// `trt_nee_params` and the heuristic (`enum trt_mis_heuristic`) that weights a shadow ray against the hit the path makes anyway, for
/// `trt_nee_mis` (160 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_nee_mis_params {
    pub nee: trt_nee_params,
    pub heuristic: u32,
    pub reserved: [u32; 7],
}

/// `trt_nee_mis_params` (accumulate stays 0; the heuristic is read only when `weighted` is 1), whether the sample is the weighted
/// queries' and `trt_nee_mis_pick`'s `total_power`, for `trt_nee_samples` (192 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_nee_samples_params {
    pub query: trt_nee_mis_params,
    pub weighted: u32,
    pub total_power: f32,
    pub reserved: [u32; 6],
}

/// One record of the alias table `trt_direct_pick` / `trt_direct_mis_pick` choose their emitter through (16 bytes): slot k keeps
/// emitter k where the second draw is below `q`, else takes `alias`; `prob` is the probability with which emitter k is chosen.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_emitter_pick {
    pub q: f32,
    pub alias: u32,
    pub prob: f32,
    pub reserved: u32,
}

/// `trt_direct_params` and the heuristic (`enum trt_mis_heuristic`) that weights a shadow ray against a cosine-lobe ray from the surfel,
/// for `trt_direct_mis` (128 bytes); `reserved` stays zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_direct_mis_params {
    pub direct: trt_direct_params,
    pub heuristic: u32,
    pub reserved: [u32; 7],
}

/// The six feature buffers of `trt_render_aov`; a null pointer = not wanted.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct trt_aov_buffers {
    pub albedo: *mut f32,
    pub normal: *mut f32,
    pub depth: *mut f32,
    pub coverage: *mut f32,
    pub geometry: *mut u32,
    pub material: *mut u32,
}
impl Default for trt_aov_buffers {
    fn default() -> Self {
        // all-null: no buffer wanted yet
        unsafe { std::mem::zeroed() }
    }
}

/// Passes and edge stops of `trt_denoise`; take the defaults from `trt_denoise_params_default`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_denoise_params {
    pub iterations: u32,
    pub normal_power_log2: u32,
    pub sigma_albedo: f32,
    pub sigma_depth: f32,
    pub reserved: [u32; 4],
}

/// The frame and its guides for `trt_denoise`; a null guide switches its term off.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct trt_denoise_inputs {
    pub color: *const f32,
    pub albedo: *const f32,
    pub normal: *const f32,
    pub depth: *const f32,
}
impl Default for trt_denoise_inputs {
    fn default() -> Self {
        // all-null: no buffer given yet
        unsafe { std::mem::zeroed() }
    }
}

/// The variance image and sigma of `trt_denoise_ex`'s colour stop; take the default sigma from `trt_denoise_color_default`.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct trt_denoise_color {
    pub variance: *const f32,
    pub sigma_color: f32,
    pub reserved: [u32; 5],
}
impl Default for trt_denoise_color {
    fn default() -> Self {
        // null variance, sigma 0: the term is off
        unsafe { std::mem::zeroed() }
    }
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct trt_stats {
    pub samples: u64,
    pub rays: u64,
    pub node_tests: u64,
    pub sphere_tests: u64,
    pub quad_plane_tests: u64,
    pub quad_inside_tests: u64,
    pub shades: u64,
    pub kernel_ms: f64,
    pub wave_trips: [u64; 4],
    pub gather_per_band: u64,
}

/// Opaque handles (owned by the library).
#[repr(C)]
pub struct trt_world {
    _private: [u8; 0],
}
#[repr(C)]
pub struct trt_scene {
    _private: [u8; 0],
}

extern "C" {
    pub fn trt_world_create(out: *mut *mut trt_world) -> c_int;
    pub fn trt_world_destroy(w: *mut trt_world);
    pub fn trt_world_add_material(w: *mut trt_world, name: *const c_char, m: *const trt_material) -> c_int;
    pub fn trt_world_get_material(w: *const trt_world, name: *const c_char, index: *mut u32) -> c_int;
    pub fn trt_world_add_sphere(w: *mut trt_world, center: trt_vec3, radius: f32, material: u32) -> c_int;
    pub fn trt_world_add_spheres(w: *mut trt_world, n: u32, center_radius: *const f32, material: *const u32) -> c_int;
    pub fn trt_world_add_quad(w: *mut trt_world, corner: trt_vec3, u: trt_vec3, v: trt_vec3, material: u32) -> c_int;
    pub fn trt_world_num_geometries(w: *const trt_world) -> c_int;
    pub fn trt_world_num_materials(w: *const trt_world) -> c_int;

    pub fn trt_scene_create(w: *const trt_world, out: *mut *mut trt_scene) -> c_int;
    pub fn trt_scene_options_default(out: *mut trt_scene_options);
    pub fn trt_scene_create_ex(w: *const trt_world, options: *const trt_scene_options, out: *mut *mut trt_scene) -> c_int;
    pub fn trt_scene_create_on_device(w: *const trt_world, options: *const trt_scene_options, out: *mut *mut trt_scene) -> c_int;
    pub fn trt_tuning_default(out: *mut trt_tuning);
    pub fn trt_scene_destroy(s: *mut trt_scene);
    pub fn trt_scene_trim(s: *mut trt_scene) -> c_int;
    pub fn trt_scene_get_info(s: *const trt_scene, out: *mut trt_scene_info) -> c_int;
    pub fn trt_scene_get_nodes(s: *const trt_scene, bbox6: *mut f32, prim: *mut i32, skip: *mut i32, cap: u32) -> c_int;
    pub fn trt_scene_get_cull_nodes(s: *const trt_scene, bbox6: *mut f32, prim: *mut i32, skip: *mut i32, cap: u32) -> c_int;
    pub fn trt_scene_get_compact_nodes(s: *const trt_scene, words4: *mut u32, cap: u32) -> c_int;
    pub fn trt_scene_get_packed(s: *const trt_scene, bytes: *mut u8, cap: u32) -> c_int;

    pub fn trt_camera_init(out: *mut trt_camera, focus_distance: f32, defocus_angle_deg: f32, position: trt_vec3,
                           look_at: trt_vec3, up: trt_vec3, vertical_fov_deg: f32, width: u32, height: u32) -> c_int;

    pub fn trt_render(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, accum: *mut f32,
                      stats: *mut trt_stats) -> c_int;
    pub fn trt_render_multi(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, devices: *const c_int,
                            ndev: u32, accum: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_render_multi_device(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params,
                                   devices: *const c_int, ndev: u32, d_accum: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_band_rows_local(height: u32, ndev: u32, rank: u32, rows_local: *mut u32) -> c_int;
    pub fn trt_band_copy_plan(width: u32, height: u32, ndev: u32, rank: u32, out: *mut trt_band_copy) -> c_int;
    pub fn trt_streamed_launch_plan(s: *const trt_scene, cam: *const trt_camera, p: *const trt_render_params,
                                    out: *mut trt_launch_plan) -> c_int;
    pub fn trt_render_device(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, d_accum: *mut f32,
                             d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_render_moments(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, accum: *mut f32,
                              moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_render_moments_device(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, d_accum: *mut f32,
                                     d_moment2: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_variance(accum: *const f32, moment2: *const f32, npixels: u32, samples_per_pixel: u32, variance: *mut f32) -> c_int;
    pub fn trt_variance_device(d_accum: *const f32, d_moment2: *const f32, npixels: u32, samples_per_pixel: u32,
                               d_variance: *mut f32, stream: *mut c_void) -> c_int;
    pub fn trt_render_pixels(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, pixels: *const u32, n: u32,
                             accum: *mut f32, moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_render_pixels_device(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, d_pixels: *const u32, n: u32,
                                    d_count: *const u32, d_accum: *mut f32, d_moment2: *mut f32, d_counters: *mut u64,
                                    stream: *mut c_void) -> c_int;
    pub fn trt_pixels_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_select_pixels(accum: *const f32, moment2: *const f32, npixels: u32, samples_per_pixel: u32, samples_done: u32,
                             candidates: *const u32, n_candidates: u32, rel_tol: f32, abs_tol: f32, selected: *mut u32,
                             count: *mut u32) -> c_int;
    // (host form above: `selected` may alias `candidates`; device form below: the n_candidates words at `d_selected` must not overlap the
    // n_candidates words at `d_candidates` - TRT_ERR_INVALID_ARG - because the kernels cannot compact in place)
    pub fn trt_select_pixels_device(d_accum: *const f32, d_moment2: *const f32, npixels: u32, samples_per_pixel: u32, samples_done: u32,
                                    d_candidates: *const u32, n_candidates: u32, rel_tol: f32, abs_tol: f32, d_selected: *mut u32,
                                    d_count: *mut u32, d_scratch: *mut c_void, scratch_bytes: u64, stream: *mut c_void) -> c_int;
    pub fn trt_select_scratch_bytes(n_candidates: u32) -> u64;
    pub fn trt_radiance_params_default(out: *mut trt_radiance_params);
    pub fn trt_radiance(s: *mut trt_scene, rays: *const trt_ray, n: u32, p: *const trt_radiance_params, radiance: *mut f32,
                        moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_radiance_device(s: *mut trt_scene, d_rays: *const trt_ray, n: u32, p: *const trt_radiance_params, d_radiance: *mut f32,
                               d_moment2: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_radiance_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_gather_params_default(out: *mut trt_gather_params);
    pub fn trt_gather(s: *mut trt_scene, items: *const trt_ray, n: u32, p: *const trt_gather_params, radiance: *mut f32,
                      moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_gather_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, p: *const trt_gather_params, d_radiance: *mut f32,
                             d_moment2: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_gather_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_ambient_params_default(out: *mut trt_ambient_params);
    pub fn trt_ambient(s: *mut trt_scene, items: *const trt_ray, n: u32, p: *const trt_ambient_params, visibility: *mut f32,
                       bent: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_ambient_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, p: *const trt_ambient_params, d_visibility: *mut f32,
                              d_bent: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_ambient_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_scene_emitters(s: *const trt_scene, out: *mut trt_emitter, cap: u32, count: *mut u32) -> c_int;
    pub fn trt_emitter_init_quad(out: *mut trt_emitter, corner: trt_vec3, u: trt_vec3, v: trt_vec3, color: trt_vec3);
    pub fn trt_emitter_init_sphere(out: *mut trt_emitter, centre: trt_vec3, radius: f32, color: trt_vec3);
    pub fn trt_direct_params_default(out: *mut trt_direct_params);
    pub fn trt_direct(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, n_emitters: u32,
                      p: *const trt_direct_params, radiance: *mut f32, moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_direct_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter, n_emitters: u32,
                             p: *const trt_direct_params, d_radiance: *mut f32, d_moment2: *mut f32, d_counters: *mut u64,
                             stream: *mut c_void) -> c_int;
    pub fn trt_direct_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_nee_params_default(out: *mut trt_nee_params);
    pub fn trt_nee(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, n_emitters: u32,
                   p: *const trt_nee_params, radiance: *mut f32, moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_nee_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter, n_emitters: u32,
                          p: *const trt_nee_params, d_radiance: *mut f32, d_moment2: *mut f32, d_counters: *mut u64,
                          stream: *mut c_void) -> c_int;
    pub fn trt_nee_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_nee_mis_params_default(out: *mut trt_nee_mis_params);
    pub fn trt_nee_mis(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, n_emitters: u32,
                       p: *const trt_nee_mis_params, radiance: *mut f32, moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_nee_mis_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter, n_emitters: u32,
                              p: *const trt_nee_mis_params, d_radiance: *mut f32, d_moment2: *mut f32, d_counters: *mut u64,
                              stream: *mut c_void) -> c_int;
    pub fn trt_nee_mis_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_direct_mis_params_default(out: *mut trt_direct_mis_params);
    pub fn trt_direct_mis(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, n_emitters: u32,
                          p: *const trt_direct_mis_params, radiance: *mut f32, moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_direct_mis_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter, n_emitters: u32,
                                 p: *const trt_direct_mis_params, d_radiance: *mut f32, d_moment2: *mut f32, d_counters: *mut u64,
                                 stream: *mut c_void) -> c_int;
    pub fn trt_direct_mis_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_emitter_pick_build(emitters: *const trt_emitter, n_emitters: u32, weights: *const f32, out: *mut trt_emitter_pick,
                                  total: *mut f32) -> c_int;
    pub fn trt_direct_pick(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, pick: *const trt_emitter_pick,
                           n_emitters: u32, p: *const trt_direct_params, radiance: *mut f32, moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_direct_pick_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter,
                                  d_pick: *const trt_emitter_pick, n_emitters: u32, p: *const trt_direct_params, d_radiance: *mut f32,
                                  d_moment2: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_direct_pick_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_direct_mis_pick(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, pick: *const trt_emitter_pick,
                               n_emitters: u32, p: *const trt_direct_mis_params, total_power: f32, radiance: *mut f32, moment2: *mut f32,
                               stats: *mut trt_stats) -> c_int;
    pub fn trt_direct_mis_pick_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter,
                                      d_pick: *const trt_emitter_pick, n_emitters: u32, p: *const trt_direct_mis_params, total_power: f32,
                                      d_radiance: *mut f32, d_moment2: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_direct_mis_pick_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_nee_pick(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, pick: *const trt_emitter_pick,
                        n_emitters: u32, p: *const trt_nee_params, radiance: *mut f32, moment2: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_nee_pick_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter,
                               d_pick: *const trt_emitter_pick, n_emitters: u32, p: *const trt_nee_params, d_radiance: *mut f32,
                               d_moment2: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_nee_pick_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_nee_mis_pick(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, pick: *const trt_emitter_pick,
                            n_emitters: u32, p: *const trt_nee_mis_params, total_power: f32, radiance: *mut f32, moment2: *mut f32,
                            stats: *mut trt_stats) -> c_int;
    pub fn trt_nee_mis_pick_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter,
                                   d_pick: *const trt_emitter_pick, n_emitters: u32, p: *const trt_nee_mis_params, total_power: f32,
                                   d_radiance: *mut f32, d_moment2: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_nee_mis_pick_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_probe_params_default(out: *mut trt_probe_params);
    pub fn trt_probe(s: *mut trt_scene, items: *const trt_ray, n: u32, p: *const trt_probe_params, sh: *mut f32,
                     stats: *mut trt_stats) -> c_int;
    pub fn trt_probe_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, p: *const trt_probe_params, d_sh: *mut f32,
                            d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_probe_launch_plan(s: *const trt_scene, n: u32, bands: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_samples_params_default(out: *mut trt_samples_params);
    pub fn trt_samples(s: *mut trt_scene, items: *const trt_ray, n: u32, p: *const trt_samples_params, colors: *mut f32, directions: *mut f32,
                       stats: *mut trt_stats) -> c_int;
    pub fn trt_samples_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, p: *const trt_samples_params, d_colors: *mut f32,
                              d_directions: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_samples_launch_plan(s: *const trt_scene, n: u32, range_length: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_fold_samples(colors: *const f32, n: u32, p: *const trt_radiance_params, radiance: *mut f32, moment2: *mut f32) -> c_int;
    pub fn trt_fold_samples_device(d_colors: *const f32, n: u32, p: *const trt_radiance_params, d_radiance: *mut f32, d_moment2: *mut f32,
                                   stream: *mut c_void) -> c_int;
    pub fn trt_project_samples(colors: *const f32, directions: *const f32, items: *const trt_ray, n: u32, p: *const trt_probe_params,
                               sh: *mut f32) -> c_int;
    pub fn trt_project_samples_device(d_colors: *const f32, d_directions: *const f32, d_items: *const trt_ray, n: u32,
                                      p: *const trt_probe_params, d_sh: *mut f32, stream: *mut c_void) -> c_int;
    pub fn trt_probe_parallel(s: *mut trt_scene, items: *const trt_ray, n: u32, p: *const trt_probe_params, sh: *mut f32,
                              stats: *mut trt_stats, record_bytes: u64) -> c_int;
    pub fn trt_probe_parallel_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, p: *const trt_probe_params, d_sh: *mut f32,
                                     d_counters: *mut u64, d_records: *mut c_void, record_bytes: u64, stream: *mut c_void) -> c_int;
    pub fn trt_probe_parallel_launch_plan(s: *const trt_scene, n: u32, range_length: u32, compute_units: u32,
                                          out: *mut trt_query_plan) -> c_int;
    pub fn trt_nee_samples_params_default(out: *mut trt_nee_samples_params);
    pub fn trt_nee_samples(s: *mut trt_scene, items: *const trt_ray, n: u32, emitters: *const trt_emitter, pick: *const trt_emitter_pick,
                           n_emitters: u32, p: *const trt_nee_samples_params, colors: *mut f32, directions: *mut f32, stats: *mut trt_stats) -> c_int;
    pub fn trt_nee_samples_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, d_emitters: *const trt_emitter,
                                  d_pick: *const trt_emitter_pick, n_emitters: u32, p: *const trt_nee_samples_params, d_colors: *mut f32,
                                  d_directions: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_nee_samples_launch_plan(s: *const trt_scene, n: u32, range_length: u32, weighted: u32, pick: u32, compute_units: u32,
                                       out: *mut trt_query_plan) -> c_int;
    pub fn trt_passes_params_default(out: *mut trt_passes_params);
    pub fn trt_passes(s: *mut trt_scene, items: *const trt_ray, n: u32, p: *const trt_passes_params, passes: *mut f32, spent: *mut f32,
                      stats: *mut trt_stats) -> c_int;
    pub fn trt_passes_device(s: *mut trt_scene, d_items: *const trt_ray, n: u32, p: *const trt_passes_params, d_passes: *mut f32,
                             d_spent: *mut f32, d_counters: *mut u64, stream: *mut c_void) -> c_int;
    pub fn trt_passes_launch_plan(s: *const trt_scene, n: u32, depth_bins: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_sample_batch(s: *mut trt_scene, input: *const trt_sample_point, n: u32, out: *mut trt_sampled_color,
                            max_bounces: u32, background: trt_vec3, seed: u32, stats: *mut trt_stats) -> c_int;
    pub fn trt_intersect(s: *mut trt_scene, rays: *const trt_ray, t_max: *const f32, n: u32, hits: *mut trt_hit) -> c_int;
    pub fn trt_occluded(s: *mut trt_scene, rays: *const trt_ray, t_max: *const f32, n: u32, occluded: *mut u8) -> c_int;
    pub fn trt_intersect_device(s: *mut trt_scene, d_rays: *const trt_ray, d_t_max: *const f32, n: u32, d_hits: *mut trt_hit,
                                stream: *mut c_void) -> c_int;
    pub fn trt_occluded_device(s: *mut trt_scene, d_rays: *const trt_ray, d_t_max: *const f32, n: u32, d_occluded: *mut u8,
                               stream: *mut c_void) -> c_int;
    pub fn trt_query_launch_plan(s: *const trt_scene, n: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_primary_rays(cam: *const trt_camera, p: *const trt_render_params, s: u32, rays: *mut trt_ray) -> c_int;
    pub fn trt_primary_rays_device(cam: *const trt_camera, p: *const trt_render_params, s: u32, d_rays: *mut trt_ray,
                                   stream: *mut c_void) -> c_int;
    pub fn trt_render_aov(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params, buffers: *const trt_aov_buffers) -> c_int;
    pub fn trt_render_aov_device(s: *mut trt_scene, cam: *const trt_camera, p: *const trt_render_params,
                                 d_buffers: *const trt_aov_buffers, stream: *mut c_void) -> c_int;
    pub fn trt_aov_launch_plan(s: *const trt_scene, n_pixels: u32, compute_units: u32, out: *mut trt_query_plan) -> c_int;
    pub fn trt_denoise_params_default(out: *mut trt_denoise_params);
    pub fn trt_denoise_scratch_bytes(width: u32, height: u32, params: *const trt_denoise_params) -> u64;
    pub fn trt_denoise(input: *const trt_denoise_inputs, width: u32, height: u32, params: *const trt_denoise_params, out: *mut f32) -> c_int;
    pub fn trt_denoise_device(d_in: *const trt_denoise_inputs, width: u32, height: u32, params: *const trt_denoise_params,
                              d_out: *mut f32, d_scratch: *mut c_void, scratch_bytes: u64, stream: *mut c_void) -> c_int;
    pub fn trt_denoise_color_default(out: *mut trt_denoise_color);
    pub fn trt_denoise_ex(input: *const trt_denoise_inputs, color: *const trt_denoise_color, width: u32, height: u32,
                          params: *const trt_denoise_params, out: *mut f32) -> c_int;
    pub fn trt_denoise_ex_device(d_in: *const trt_denoise_inputs, color: *const trt_denoise_color, width: u32, height: u32,
                                 params: *const trt_denoise_params, d_out: *mut f32, d_scratch: *mut c_void, scratch_bytes: u64,
                                 stream: *mut c_void) -> c_int;
    pub fn trt_tonemap_u8(accum: *const f32, npixels: u32, gamma: f32, rgb: *mut u8) -> c_int;
    pub fn trt_tonemap_u8_device(d_accum: *const f32, npixels: u32, gamma: f32, d_rgb: *mut u8, stream: *mut c_void) -> c_int;
    pub fn trt_streamed_chunk_spp(width: u32, rows: u32) -> u32;
    pub fn trt_kernel_timing_begin() -> c_int;
    pub fn trt_kernel_timing_end(total_ms: *mut f64, launches: *mut u32) -> c_int;

    pub fn trt_dominant_kernel(s: *const trt_scene, cam: *const trt_camera, p: *const trt_render_params) -> *const c_char;
    pub fn trt_flat_literal_compilations() -> u64;
    pub fn trt_flat_literal_diagnostic() -> *const c_char;
    pub fn trt_scene_facts(s: *const trt_scene) -> u32;
    pub fn trt_flat_literal_facts() -> u32;

    pub fn trt_last_error() -> *const c_char;
    pub fn trt_device_count() -> c_int;
    pub fn trt_set_device(ordinal: c_int) -> c_int;
    pub fn trt_abi_version() -> u32;
}
