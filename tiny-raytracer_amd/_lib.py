"""ctypes binding of libtinyrt.so — exactly the entry points include/tinyrt.h declares.

The library is the product: hand-written HIP for gfx950 behind a C ABI.  There is no Python or
CPU fallback; if the shared object is missing or fails to load, importing this module raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRT_LIB_PATH") or os.path.join(_HERE, "libtinyrt.so")     # override: A/B of two builds
CSRC = os.path.join(_HERE, "csrc")

TRT_OK = 0
ABI_VERSION = 4          # include/tinyrt.h TRT_ABI_VERSION
ERR_INVALID_ARG, ERR_DUPLICATE, ERR_NOT_FOUND, ERR_HIP, ERR_NO_DEVICE, ERR_OOM = -1, -2, -3, -4, -5, -6
LAMBERTIAN, METAL, DIELECTRIC, LIGHT = 0, 1, 2, 3
BACKEND_MEGAKERNEL, BACKEND_WAVEFRONT, BACKEND_AUTO, BACKEND_STREAMED = 0, 1, 2, 3


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(float(x), float(y), float(z))

    def tolist(self):
        return [self.x, self.y, self.z]


class Ray(C.Structure):
    _fields_ = [("origin", Vec3), ("direction", Vec3)]


class SamplePoint(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("ray", Ray)]


class SampledColor(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("color", Vec3)]


class Hit(C.Structure):
    """tinyrt.h trt_hit: the answer of a closest-hit query (28 bytes)."""
    _fields_ = [("t", C.c_float), ("geometry", C.c_uint32), ("material", C.c_uint32), ("front_face", C.c_uint32), ("normal", Vec3)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("albedo", Vec3), ("param", C.c_float)]


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ("num_nodes", "num_spheres", "num_quads", "num_materials", "max_depth", "device_bytes", "lds_bytes",
                 "num_cull_nodes")]


class CameraPOD(C.Structure):
    _fields_ = [("position", Vec3), ("viewport_upper_left", Vec3), ("forward", Vec3), ("horizontal", Vec3),
                ("vertical", Vec3), ("defocus_disk_u", Vec3), ("defocus_disk_v", Vec3),
                ("width", C.c_uint32), ("height", C.c_uint32)]


class BandCopy(C.Structure):
    _fields_ = [("rows_local", C.c_uint32), ("full_bands", C.c_uint32), ("tail_rows", C.c_uint32), ("reserved", C.c_uint32),
                ("band_bytes", C.c_uint64), ("local_pitch", C.c_uint64), ("frame_pitch", C.c_uint64), ("frame_offset", C.c_uint64),
                ("tail_bytes", C.c_uint64), ("tail_local_offset", C.c_uint64), ("tail_frame_offset", C.c_uint64)]


class LaunchPlan(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ("scene_mode", "threads_per_workgroup", "waves_per_simd", "workgroups_per_cu", "lds_bytes", "scene_lds_bytes",
                 "leaf_slots", "lds_leaf_stack", "ray_pool", "walk", "specialised", "has_kernel", "kernel_waves_per_simd",
                 "kernel_threads", "kernel_walk", "kernel_ray_pool", "kernel_counting", "chunk_spp", "dual_walk")] + [("workspace_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class QueryPlan(C.Structure):
    """tinyrt.h trt_query_plan: how a batch of n rays is launched on a scene."""
    _fields_ = [(n, C.c_uint32) for n in
                ("scene_mode", "walk", "threads_per_workgroup", "kernel_waves_per_simd", "workgroups_per_cu", "leaf_slots", "stragglers",
                 "lds_bytes", "scene_lds_bytes", "has_kernel", "fallback", "streamed_walk", "streamed_threads", "compute_units",
                 "rays_per_wave", "workgroups")] + [("wave_slots", C.c_uint64), ("waves", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AovBuffers(C.Structure):
    """tinyrt.h trt_aov_buffers: the six feature buffers of trt_render_aov, each a pointer or NULL (not wanted)."""
    FIELDS = ("albedo", "normal", "depth", "coverage", "geometry", "material")
    _fields_ = [(n, C.c_void_p) for n in FIELDS]


class DenoiseParams(C.Structure):
    """tinyrt.h trt_denoise_params: passes and edge stops of trt_denoise (32 bytes)."""
    FIELDS = ("iterations", "normal_power_log2", "sigma_albedo", "sigma_depth")
    _fields_ = [("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {n: getattr(self, n) for n in self.FIELDS}


class DenoiseInputs(C.Structure):
    """tinyrt.h trt_denoise_inputs: the frame and its guides, each guide a pointer or NULL (term off)."""
    FIELDS = ("color", "albedo", "normal", "depth")
    _fields_ = [(n, C.c_void_p) for n in FIELDS]


class DenoiseColor(C.Structure):
    """tinyrt.h trt_denoise_color: the variance image and sigma of trt_denoise_ex's colour stop (32 bytes)."""
    _fields_ = [("variance", C.c_void_p), ("sigma_color", C.c_float), ("reserved", C.c_uint32 * 5)]


class RadianceParams(C.Structure):
    """tinyrt.h trt_radiance_params: samples, depth, RNG numbering and sample range of trt_radiance (64 bytes)."""
    FIELDS = ("samples_per_ray", "max_bounces", "background", "seed", "sample_begin", "sample_end", "accumulate", "first_stream")
    _fields_ = [("samples_per_ray", C.c_uint32), ("max_bounces", C.c_uint32), ("background", Vec3), ("seed", C.c_uint32),
                ("sample_begin", C.c_uint32), ("sample_end", C.c_uint32), ("accumulate", C.c_uint32), ("first_stream", C.c_uint32),
                ("reserved", C.c_uint32 * 6)]


LOBE_COSINE, LOBE_CONE = 1, 2                                                # tinyrt.h enum trt_lobe


class GatherParams(C.Structure):
    """tinyrt.h trt_gather_params: trt_radiance_params and the lobe the first ray of a sample is drawn from (96 bytes)."""
    _fields_ = [("path", RadianceParams), ("lobe", C.c_uint32), ("spread", C.c_float), ("reserved", C.c_uint32 * 6)]


class AmbientParams(C.Structure):
    """tinyrt.h trt_ambient_params: trt_gather_params (its path's max_bounces and background are not read) and the distance within which
    an occluder counts (128 bytes)."""
    _fields_ = [("gather", GatherParams), ("max_distance", C.c_float), ("reserved", C.c_uint32 * 7)]


EMITTER_SPHERE, EMITTER_QUAD = 0, 1                                         # tinyrt.h trt_emitter.kind
NO_GEOMETRY = 0xFFFFFFFF                                                    # trt_emitter.geometry of a light that is not in the scene


class Emitter(C.Structure):
    """tinyrt.h trt_emitter: one light of the table a direct-light query samples (80 bytes)."""
    _fields_ = [("kind", C.c_uint32), ("geometry", C.c_uint32), ("a", Vec3), ("b", Vec3), ("c", Vec3), ("normal", Vec3), ("color", Vec3),
                ("area", C.c_float), ("reserved", C.c_uint32 * 2)]


class EmitterPick(C.Structure):
    """tinyrt.h trt_emitter_pick: one record of the alias table a PICK direct-light query chooses its emitter through (16 bytes)."""
    _fields_ = [("q", C.c_float), ("alias", C.c_uint32), ("prob", C.c_float), ("reserved", C.c_uint32)]


class DirectParams(C.Structure):
    """tinyrt.h trt_direct_params: trt_radiance_params (its max_bounces and background are not read) and the share of the distance to
    the emitter point the shadow ray covers (96 bytes)."""
    _fields_ = [("path", RadianceParams), ("shadow_end", C.c_float), ("reserved", C.c_uint32 * 7)]


PROBE_SPHERE, PROBE_HEMISPHERE = 1, 2                                       # tinyrt.h enum trt_probe_domain


class ProbeParams(C.Structure):
    """tinyrt.h trt_probe_params: trt_radiance_params, the domain the first ray of a sample is drawn over and the number of spherical-
    harmonic bands the colours are folded into (96 bytes)."""
    _fields_ = [("path", RadianceParams), ("domain", C.c_uint32), ("bands", C.c_uint32), ("reserved", C.c_uint32 * 6)]


SAMPLE_RAYS, SAMPLE_COSINE, SAMPLE_CONE, SAMPLE_SPHERE, SAMPLE_HEMISPHERE = 0, 1, 2, 3, 4      # tinyrt.h enum trt_sample_source


class SamplesParams(C.Structure):
    """tinyrt.h trt_samples_params: trt_radiance_params (accumulate must be 0) and the source of a sample's first ray (96 bytes)."""
    _fields_ = [("path", RadianceParams), ("source", C.c_uint32), ("spread", C.c_float), ("reserved", C.c_uint32 * 6)]


PASSES_RAYS, PASSES_COSINE, PASSES_CONE = 0, 1, 2                           # tinyrt.h enum trt_passes_source (1, 2 = enum trt_lobe)


class PassesParams(C.Structure):
    """tinyrt.h trt_passes_params: trt_gather_params, whose lobe is read as the source of the first ray, and the number of depth bins
    the samples are split into (128 bytes)."""
    _fields_ = [("gather", GatherParams), ("depth_bins", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class NeeParams(C.Structure):
    """tinyrt.h trt_nee_params: trt_gather_params, whose lobe is read as the source of the first ray (PASSES_*), the share of the distance
    to the emitter point a shadow ray covers and whether the first hit counts as reached by a diffuse scatter (128 bytes)."""
    _fields_ = [("gather", GatherParams), ("shadow_end", C.c_float), ("source_is_diffuse", C.c_uint32), ("reserved", C.c_uint32 * 6)]


MIS_BALANCE, MIS_POWER = 0, 1                                               # tinyrt.h enum trt_mis_heuristic


class NeeMisParams(C.Structure):
    """tinyrt.h trt_nee_mis_params: trt_nee_params and the heuristic that weights a shadow ray against the path's own hit (160 bytes)."""
    _fields_ = [("nee", NeeParams), ("heuristic", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class NeeSamplesParams(C.Structure):
    """tinyrt.h trt_nee_samples_params: trt_nee_mis_params (accumulate must be 0; heuristic read only when weighted), whether the sample
    is the weighted queries' and trt_nee_mis_pick's total_power (192 bytes)."""
    _fields_ = [("query", NeeMisParams), ("weighted", C.c_uint32), ("total_power", C.c_float), ("reserved", C.c_uint32 * 6)]


class DirectMisParams(C.Structure):
    """tinyrt.h trt_direct_mis_params: trt_direct_params and the heuristic that weights a shadow ray against a cosine-lobe ray from the
    surfel (128 bytes)."""
    _fields_ = [("direct", DirectParams), ("heuristic", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class Tuning(C.Structure):
    """tinyrt.h trt_tuning: scheduling / placement knobs of a render; every value renders the same frame."""
    FIELDS = ("stream_waves_per_simd", "stream_big_threads", "stream_batch_spp", "radiance_gb", "leaf_slots", "lds_leaf_stack", "ray_pool",
              "stragglers", "lds_stragglers", "dual_walk", "runtime_walk", "xcd_remap", "mega_waves_per_simd", "mega_threads",
              "mega_global_waves8", "wf_waves_per_simd", "wf_serve_min")
    _fields_ = [(n, C.c_uint32) for n in FIELDS] + [("reserved", C.c_uint32 * 7)]

    def as_dict(self):
        return {n: getattr(self, n) for n in self.FIELDS}


class SceneOptions(C.Structure):
    """tinyrt.h trt_scene_options: how a scene is compiled (placement only) and how much idle device scratch its handle keeps."""
    _fields_ = [("cull_prune", C.c_float), ("flat_walk", C.c_int32), ("compact_nodes", C.c_int32), ("top_nodes", C.c_uint32),
                ("scratch_cap_bytes", C.c_uint64), ("reserved", C.c_uint32 * 6)]


class RenderParams(C.Structure):
    _fields_ = [("samples_per_pixel", C.c_uint32), ("max_bounces", C.c_uint32), ("background", Vec3),
                ("seed", C.c_uint32), ("backend", C.c_uint32),
                ("sample_begin", C.c_uint32), ("sample_end", C.c_uint32), ("accumulate", C.c_uint32),
                ("band_rows", C.c_uint32), ("band_stride", C.c_uint32), ("band_offset", C.c_uint32),
                ("rows_local", C.c_uint32), ("collect_stats", C.c_uint32), ("tuning", C.POINTER(Tuning))]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("node_tests", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("quad_plane_tests", C.c_uint64), ("quad_inside_tests", C.c_uint64),
                ("shades", C.c_uint64), ("kernel_ms", C.c_double), ("wave_trips", C.c_uint64 * 4), ("gather_per_band", C.c_uint64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "wave_trips"}
        d["wave_trips"] = list(self.wave_trips)
        return d


# name -> (restype, argtypes); the test-suite checks this table against include/tinyrt.h
SIGNATURES = {
    "trt_world_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "trt_world_destroy": (None, [C.c_void_p]),
    "trt_world_add_material": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(Material)]),
    "trt_world_get_material": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    "trt_world_add_sphere": (C.c_int, [C.c_void_p, Vec3, C.c_float, C.c_uint32]),
    "trt_world_add_spheres": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "trt_world_add_quad": (C.c_int, [C.c_void_p, Vec3, Vec3, Vec3, C.c_uint32]),
    "trt_world_num_geometries": (C.c_int, [C.c_void_p]),
    "trt_world_num_materials": (C.c_int, [C.c_void_p]),
    "trt_scene_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "trt_scene_options_default": (None, [C.POINTER(SceneOptions)]),
    "trt_scene_create_ex": (C.c_int, [C.c_void_p, C.POINTER(SceneOptions), C.POINTER(C.c_void_p)]),
    "trt_scene_create_on_device": (C.c_int, [C.c_void_p, C.POINTER(SceneOptions), C.POINTER(C.c_void_p)]),
    "trt_tuning_default": (None, [C.POINTER(Tuning)]),
    "trt_scene_destroy": (None, [C.c_void_p]),
    "trt_scene_trim": (C.c_int, [C.c_void_p]),
    "trt_scene_get_info": (C.c_int, [C.c_void_p, C.POINTER(SceneInfo)]),
    "trt_scene_get_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "trt_scene_get_cull_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "trt_scene_get_compact_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "trt_scene_get_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "trt_camera_init": (C.c_int, [C.POINTER(CameraPOD), C.c_float, C.c_float, Vec3, Vec3, Vec3, C.c_float,
                                  C.c_uint32, C.c_uint32]),
    "trt_render": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_void_p, C.POINTER(Stats)]),
    "trt_render_multi": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.POINTER(C.c_int), C.c_uint32,
                                   C.c_void_p, C.POINTER(Stats)]),
    "trt_render_multi_device": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.POINTER(C.c_int),
                                          C.c_uint32, C.c_void_p, C.POINTER(Stats)]),
    "trt_band_rows_local": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "trt_band_copy_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BandCopy)]),
    "trt_streamed_launch_plan": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.POINTER(LaunchPlan)]),
    "trt_kernel_timing_begin": (C.c_int, []),
    "trt_kernel_timing_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "trt_render_device": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "trt_render_moments": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_render_moments_device": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "trt_variance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "trt_variance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "trt_render_pixels": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.POINTER(Stats)]),
    "trt_render_pixels_device": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_pixels_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_select_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                    C.c_void_p, C.POINTER(C.c_uint32)]),
    "trt_select_pixels_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "trt_select_scratch_bytes": (C.c_uint64, [C.c_uint32]),
    "trt_radiance_params_default": (None, [C.POINTER(RadianceParams)]),
    "trt_radiance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RadianceParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_radiance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RadianceParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "trt_radiance_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_gather_params_default": (None, [C.POINTER(GatherParams)]),
    "trt_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(GatherParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_gather_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(GatherParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "trt_gather_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_ambient_params_default": (None, [C.POINTER(AmbientParams)]),
    "trt_ambient": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(AmbientParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_ambient_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(AmbientParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "trt_ambient_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_scene_emitters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "trt_emitter_init_quad": (None, [C.POINTER(Emitter), Vec3, Vec3, Vec3, Vec3]),
    "trt_emitter_init_sphere": (None, [C.POINTER(Emitter), Vec3, C.c_float, Vec3]),
    "trt_direct_params_default": (None, [C.POINTER(DirectParams)]),
    "trt_direct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(DirectParams), C.c_void_p, C.c_void_p,
                             C.POINTER(Stats)]),
    "trt_direct_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(DirectParams), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "trt_direct_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_nee_params_default": (None, [C.POINTER(NeeParams)]),
    "trt_nee": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(NeeParams), C.c_void_p, C.c_void_p,
                          C.POINTER(Stats)]),
    "trt_nee_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(NeeParams), C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "trt_nee_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_nee_mis_params_default": (None, [C.POINTER(NeeMisParams)]),
    "trt_nee_mis": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(NeeMisParams), C.c_void_p, C.c_void_p,
                              C.POINTER(Stats)]),
    "trt_nee_mis_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(NeeMisParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "trt_nee_mis_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_direct_mis_params_default": (None, [C.POINTER(DirectMisParams)]),
    "trt_direct_mis": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(DirectMisParams), C.c_void_p, C.c_void_p,
                                 C.POINTER(Stats)]),
    "trt_direct_mis_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(DirectMisParams), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_direct_mis_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_emitter_pick_build": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "trt_direct_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(DirectParams), C.c_void_p,
                                  C.c_void_p, C.POINTER(Stats)]),
    "trt_direct_pick_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(DirectParams),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_direct_pick_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_direct_mis_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(DirectMisParams),
                                      C.c_float, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_direct_mis_pick_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(DirectMisParams),
                                             C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_direct_mis_pick_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_nee_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(NeeParams), C.c_void_p,
                               C.c_void_p, C.POINTER(Stats)]),
    "trt_nee_pick_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(NeeParams),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_nee_pick_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_nee_mis_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(NeeMisParams),
                                   C.c_float, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_nee_mis_pick_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(NeeMisParams),
                                          C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_nee_mis_pick_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_probe_params_default": (None, [C.POINTER(ProbeParams)]),
    "trt_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ProbeParams), C.c_void_p, C.POINTER(Stats)]),
    "trt_probe_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ProbeParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_probe_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_samples_params_default": (None, [C.POINTER(SamplesParams)]),
    "trt_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(SamplesParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(SamplesParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "trt_samples_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_fold_samples": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RadianceParams), C.c_void_p, C.c_void_p]),
    "trt_fold_samples_device": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(RadianceParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_project_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ProbeParams), C.c_void_p]),
    "trt_project_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ProbeParams), C.c_void_p, C.c_void_p]),
    "trt_probe_parallel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ProbeParams), C.c_void_p, C.POINTER(Stats), C.c_uint64]),
    "trt_probe_parallel_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ProbeParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint64, C.c_void_p]),
    "trt_probe_parallel_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_nee_samples_params_default": (None, [C.POINTER(NeeSamplesParams)]),
    "trt_nee_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(NeeSamplesParams), C.c_void_p,
                                  C.c_void_p, C.POINTER(Stats)]),
    "trt_nee_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(NeeSamplesParams),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "trt_nee_samples_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_passes_params_default": (None, [C.POINTER(PassesParams)]),
    "trt_passes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(PassesParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "trt_passes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(PassesParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "trt_passes_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_sample_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, Vec3, C.c_uint32,
                                   C.POINTER(Stats)]),
    "trt_intersect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "trt_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "trt_intersect_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "trt_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "trt_query_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_primary_rays": (C.c_int, [C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_uint32, C.c_void_p]),
    "trt_primary_rays_device": (C.c_int, [C.POINTER(CameraPOD), C.POINTER(RenderParams), C.c_uint32, C.c_void_p, C.c_void_p]),
    "trt_render_aov": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.POINTER(AovBuffers)]),
    "trt_render_aov_device": (C.c_int, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams), C.POINTER(AovBuffers), C.c_void_p]),
    "trt_aov_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(QueryPlan)]),
    "trt_denoise_params_default": (None, [C.POINTER(DenoiseParams)]),
    "trt_denoise_scratch_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams)]),
    "trt_denoise": (C.c_int, [C.POINTER(DenoiseInputs), C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.c_void_p]),
    "trt_denoise_device": (C.c_int, [C.POINTER(DenoiseInputs), C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p]),
    "trt_denoise_color_default": (None, [C.POINTER(DenoiseColor)]),
    "trt_denoise_ex": (C.c_int, [C.POINTER(DenoiseInputs), C.POINTER(DenoiseColor), C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), C.c_void_p]),
    "trt_denoise_ex_device": (C.c_int, [C.POINTER(DenoiseInputs), C.POINTER(DenoiseColor), C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams),
                                        C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "trt_streamed_chunk_spp": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "trt_tonemap_u8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "trt_tonemap_u8_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
    "trt_dominant_kernel": (C.c_char_p, [C.c_void_p, C.POINTER(CameraPOD), C.POINTER(RenderParams)]),
    "trt_last_error": (C.c_char_p, []),
    "trt_device_count": (C.c_int, []),
    "trt_set_device": (C.c_int, [C.c_int]),
    "trt_abi_version": (C.c_uint32, []),
    "trt_flat_literal_compilations": (C.c_uint64, []),
    "trt_flat_literal_diagnostic": (C.c_char_p, []),
    "trt_scene_facts": (C.c_uint32, [C.c_void_p]),
    "trt_flat_literal_facts": (C.c_uint32, []),
}


def build(force=False):
    """Compile libtinyrt.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.run(["make", "-C", CSRC, "--no-print-directory"], check=True)
    return LIB_PATH


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so (same SONAMEs as /opt/rocm's).
    Two HSA runtimes in one process cannot both own the GPU, so when torch is installed its copy is mapped first
    and libtinyrt.so (DT_NEEDED libamdhip64.so.7) binds to that one: device pointers and streams handed over
    from torch then belong to the same runtime.  Without torch the system ROCm runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        return cand
    return None


def load():
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C tiny-raytracer_amd/csrc). There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)            # AttributeError here = ABI symbol missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.trt_abi_version() != ABI_VERSION:
        raise ImportError("libtinyrt.so ABI version mismatch")
    return lib


lib = load()


class TinyRTError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"tinyrt error {code}: {message}")
        self.code = code


def check(rc):
    if rc != TRT_OK:
        raise TinyRTError(rc, lib.trt_last_error().decode("utf-8", "replace"))
