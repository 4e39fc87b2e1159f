"""Host-side mirror of the reference crate's World / Camera / Renderer surface over the C ABI.

Names, argument order and meaning follow the reference (paths relative to raytracer/src):
  World.add_material / add_geometry / get_material / get_bvh      hittable/world.rs:16-45
  Sphere(center, radius, material), Quad(corner, u, v, material)  hittable/sphere.rs:16, quad.rs:20
  Lambertian / Metal / Dielectric / Light                          material/*.rs
  Camera(focus_distance, defocus_angle, position, look_at, up, vertical_fov, width, height)   camera.rs:17-26
  Renderer(samples_per_pixel, num_sampler_threads, max_bounces, progressbar, background_color)   renderer/renderer.rs:21-35
  Renderer.render(camera, world) -> Image                          renderer/renderer.rs:37-79
Where the reference panics (duplicate material name, world.rs:29-31) this raises TinyRTError.
Everything numeric happens inside libtinyrt.so; this file only moves arguments.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BACKEND_MEGAKERNEL, BACKEND_WAVEFRONT, DIELECTRIC, LAMBERTIAN, LIGHT, METAL, CameraPOD, Material,
                   RenderParams, SampledColor, SamplePoint, SceneInfo, SceneOptions, Stats, TinyRTError, Tuning, Vec3, check, lib)
from .lights import EMITTER_DTYPE, PICK_DTYPE


def _v(v):
    return v if isinstance(v, Vec3) else Vec3(*v)


# ---- materials (material/{lambertian,metal,dielectric,light}.rs) ----
class Lambertian:
    def __init__(self, albedo):
        self.pod = Material(LAMBERTIAN, _v(albedo), 0.0)


class Metal:
    def __init__(self, albedo, fuzz):
        self.pod = Material(METAL, _v(albedo), float(fuzz))


class Dielectric:
    def __init__(self, albedo, refraction_index):
        self.pod = Material(DIELECTRIC, _v(albedo), float(refraction_index))


class Light:
    def __init__(self, color):
        self.pod = Material(LIGHT, _v(color), 0.0)


# ---- geometry (hittable/sphere.rs, quad.rs) ----
class Sphere:
    def __init__(self, center, radius, material):
        self.center, self.radius, self.material = _v(center), float(radius), int(material)


class Quad:
    def __init__(self, corner, u, v, material):
        self.corner, self.u, self.v, self.material = _v(corner), _v(u), _v(v), int(material)


# tinyrt.h trt_hit as a numpy record (28 bytes, no padding)
HIT_DTYPE = np.dtype([("t", np.float32), ("geometry", np.uint32), ("material", np.uint32), ("front_face", np.uint32), ("normal", np.float32, (3,))])
assert HIT_DTYPE.itemsize == C.sizeof(_lib.Hit) == 28


# tinyrt.h trt_aov_buffers: channel -> (numpy type, values per pixel)
AOV_CHANNELS = {"albedo": (np.float32, 3), "normal": (np.float32, 3), "depth": (np.float32, 1), "coverage": (np.float32, 1),
                "geometry": (np.uint32, 1), "material": (np.uint32, 1)}
assert tuple(AOV_CHANNELS) == _lib.AovBuffers.FIELDS and C.sizeof(_lib.AovBuffers) == 48


def _rays_and_t_max(rays, t_max):
    """float32 [n, 6] (origin, direction: used as given) and float32 [n] or None, contiguous."""
    r = np.ascontiguousarray(rays, np.float32)
    if r.ndim != 2 or r.shape[1] != 6:
        raise ValueError("rays must be [n, 6]: origin, direction")
    if t_max is None:
        return r, None
    t = np.ascontiguousarray(t_max, np.float32).reshape(-1)
    if len(t) != len(r):
        raise ValueError("one t_max per ray")
    return r, t


def scene_options(**over):
    """The library's default trt_scene_options with `over` applied."""
    opt = SceneOptions()
    lib.trt_scene_options_default(C.byref(opt))
    for k, v in over.items():
        if k not in dict(SceneOptions._fields_) or k == "reserved":
            raise TypeError(f"unknown scene option {k!r}")
        setattr(opt, k, v)
    return opt


def tuning(**over):
    """The library's default trt_tuning (built-in values, overridden once at load by TRT_* environment variables) with `over` applied."""
    t = Tuning()
    lib.trt_tuning_default(C.byref(t))
    for k, v in over.items():
        if k not in Tuning.FIELDS:
            raise TypeError(f"unknown tuning field {k!r}")
        setattr(t, k, int(v))
    return t


class Scene:
    """World::get_bvh(): the reference-order BVH, packed for the GPU (uploaded on first render)."""

    def __init__(self, world, on_device=False, **options):
        """options: fields of tinyrt.h trt_scene_options (cull_prune, flat_walk, compact_nodes, top_nodes, scratch_cap_bytes) - placement
        only: whatever they are, the scene renders the same frames.  on_device: compile it on the current device
        (trt_scene_create_on_device): the same bytes, already resident there."""
        self._h = C.c_void_p()
        opt = scene_options(**options)
        create = lib.trt_scene_create_on_device if on_device else lib.trt_scene_create_ex
        check(create(world._h, C.byref(opt), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.trt_scene_destroy(self._h)
            self._h = None

    def info(self):
        out = SceneInfo()
        check(lib.trt_scene_get_info(self._h, C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def _dump(self, fn, n):
        bbox = np.zeros((n, 6), np.float32)
        prim = np.zeros(n, np.int32)
        skip = np.zeros(n, np.int32)
        check(fn(self._h, bbox.ctypes.data, prim.ctypes.data, skip.ctypes.data, n))
        return bbox, prim, skip

    def nodes(self):
        """The reference tree (bvh.rs:42-84 node for node), pre-order: (bbox[n,6], prim[n], skip[n])."""
        return self._dump(lib.trt_scene_get_nodes, self.info()["num_nodes"])

    def cull_nodes(self):
        """The culling tree the kernels walk: same leaves in the same order, re-clustered inner nodes."""
        return self._dump(lib.trt_scene_get_cull_nodes, self.info()["num_cull_nodes"])


    def packed(self):
        """The packed scene as uploaded to a device: uint8[device_bytes]."""
        n = self.info()["device_bytes"]
        out = np.zeros(n, np.uint8)
        check(lib.trt_scene_get_packed(self._h, out.ctypes.data, n))
        return out

    # ---- ray queries (tinyrt.h trt_intersect / trt_occluded): BVH::hit over [0.001, t_max) for caller-supplied rays ----
    def intersect(self, rays, t_max=None):
        """Closest hit of rays float32 [n, 6] (origin, direction; used as given, never normalised) over [0.001, t_max[i]) (None = inf):
        a record array with the trt_hit fields t, geometry (insertion index), material, front_face, normal; a miss has t = inf and
        geometry = material = 0xFFFFFFFF.  Answer i belongs to ray i; rays that travel together should be neighbours."""
        r, t = _rays_and_t_max(rays, t_max)
        out = np.zeros(len(r), HIT_DTYPE)
        check(lib.trt_intersect(self._h, r.ctypes.data if len(r) else None, t.ctypes.data if t is not None and len(r) else None, len(r),
                                out.ctypes.data if len(r) else None))
        return out

    def occluded(self, rays, t_max=None):
        """bool [n]: does ray i hit anything in [0.001, t_max[i]) - intersect()'s `hit?` without paying for the closest hit."""
        r, t = _rays_and_t_max(rays, t_max)
        out = np.zeros(len(r), np.uint8)
        check(lib.trt_occluded(self._h, r.ctypes.data if len(r) else None, t.ctypes.data if t is not None and len(r) else None, len(r),
                               out.ctypes.data if len(r) else None))
        return out.view(np.bool_)

    def intersect_device(self, d_rays_ptr, n, d_hits_ptr, d_t_max_ptr=0, stream_ptr=0):
        """Enqueue intersect() on buffers already in HBM (device pointers as integers: n x 24 bytes of rays, n floats or 0, n x 28 bytes
        of records) on the current device; asynchronous on the stream."""
        check(lib.trt_intersect_device(self._h, C.c_void_p(d_rays_ptr), C.c_void_p(d_t_max_ptr), int(n), C.c_void_p(d_hits_ptr), C.c_void_p(stream_ptr)))

    def occluded_device(self, d_rays_ptr, n, d_occluded_ptr, d_t_max_ptr=0, stream_ptr=0):
        """Enqueue occluded() on buffers already in HBM (n bytes out, each 0 or 1); asynchronous on the stream."""
        check(lib.trt_occluded_device(self._h, C.c_void_p(d_rays_ptr), C.c_void_p(d_t_max_ptr), int(n), C.c_void_p(d_occluded_ptr), C.c_void_p(stream_ptr)))

    def query_plan(self, n, compute_units=0):
        """trt_query_launch_plan: how intersect() / occluded() launch a batch of n rays on this scene, as a dict (host arithmetic only;
        compute_units = 0: the current device's count, which needs a device)."""
        plan = _lib.QueryPlan()
        check(lib.trt_query_launch_plan(self._h, int(n), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    def aov_plan(self, n, compute_units=0):
        """trt_aov_launch_plan: how Renderer.render_aov launches a local image of n pixels on this scene, as a dict with query_plan()'s
        fields (rays_per_wave = pixels a wave owns)."""
        plan = _lib.QueryPlan()
        check(lib.trt_aov_launch_plan(self._h, int(n), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    def pixels_plan(self, n, compute_units=0):
        """trt_pixels_launch_plan: how Renderer.render_pixels launches a list of n pixels on this scene, as a dict with query_plan()'s
        fields (rays_per_wave = list entries a wave owns)."""
        plan = _lib.QueryPlan()
        check(lib.trt_pixels_launch_plan(self._h, int(n), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    # ---- radiance queries (tinyrt.h trt_radiance): path tracing of caller-supplied rays ----
    @staticmethod
    def _radiance_params(samples_per_ray, max_bounces=50, background=(0.0, 0.0, 0.0), seed=1, first_stream=0, sample_begin=0, sample_end=None,
                         accumulate=False):
        p = _lib.RadianceParams()
        lib.trt_radiance_params_default(C.byref(p))
        p.samples_per_ray, p.max_bounces, p.background, p.seed = int(samples_per_ray), int(max_bounces), _v(background), int(seed)
        p.first_stream, p.sample_begin, p.sample_end = int(first_stream), int(sample_begin), 0 if sample_end is None else int(sample_end)
        p.accumulate = 1 if accumulate else 0
        if sample_end is not None and int(sample_end) == 0:
            # tinyrt.h: sample_end == 0 means K; the empty range [0, 0) is asked for as begin == end elsewhere
            raise ValueError("sample_end = 0 means samples_per_ray at the C boundary: pass None for that")
        return p

    def radiance(self, rays, samples_per_ray, max_bounces=50, background=(0.0, 0.0, 0.0), seed=1, first_stream=0, sample_begin=0,
                 sample_end=None, accumulate=False, radiance=None, moment2=None):
        """trt_radiance: the light that arrives along rays float32 [n, 6] (origin, direction; used as given, never normalised), path
        traced with samples [sample_begin, sample_end) of samples_per_ray = K per ray (None: K) and folded with the imager's 1 / K rule.
        Sample s of ray i uses RNG stream (seed, first_stream + i * K + s, 0).  `radiance`, `moment2`: float32 [n, 3] to write or, with
        accumulate, to continue (changed in place); radiance=None allocates one, moment2=None: True allocates one, None = not wanted.
        Returns (radiance[n, 3], moment2 or None, stats with samples and rays)."""
        r, _ = _rays_and_t_max(rays, None)
        n = len(r)
        p = self._radiance_params(samples_per_ray, max_bounces, background, seed, first_stream, sample_begin, sample_end, accumulate)
        if radiance is None:
            radiance = np.zeros((n, 3), np.float32)
        if moment2 is True:
            moment2 = np.zeros((n, 3), np.float32)
        for a in (radiance, moment2):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (n, 3))
        st = Stats()
        check(lib.trt_radiance(self._h, r.ctypes.data if n else None, n, C.byref(p), radiance.ctypes.data if n else None,
                               moment2.ctypes.data if moment2 is not None and n else None, C.byref(st)))
        return radiance, moment2, st.as_dict()

    def radiance_device(self, d_rays_ptr, n, d_radiance_ptr, d_moment2_ptr=0, d_counters_ptr=0, stream_ptr=0, **params):
        """Enqueue radiance() on buffers already in HBM (device pointers as integers: n x 24 bytes of rays, n x 12 bytes of sums each) on
        the current device; asynchronous on the stream, allocates nothing.  `params`: radiance()'s keywords, samples_per_ray included."""
        p = self._radiance_params(**params)
        check(lib.trt_radiance_device(self._h, C.c_void_p(d_rays_ptr), int(n), C.byref(p), C.c_void_p(d_radiance_ptr), C.c_void_p(d_moment2_ptr),
                                      C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))

    def radiance_plan(self, n, compute_units=0):
        """trt_radiance_launch_plan: how radiance() launches n rays on this scene, as a dict with query_plan()'s fields (rays_per_wave =
        rays a wave owns, each for all samples of the call)."""
        plan = _lib.QueryPlan()
        check(lib.trt_radiance_launch_plan(self._h, int(n), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    # ---- gather queries (tinyrt.h trt_gather): radiance queries whose first rays the device draws about caller-supplied surfels ----
    LOBES = {"cosine": _lib.LOBE_COSINE, "cone": _lib.LOBE_CONE}

    @classmethod
    def _gather_params(cls, samples_per_item, lobe="cosine", spread=0.0, **path):
        if lobe not in cls.LOBES:
            raise ValueError("lobe must be 'cosine' or 'cone'")
        p = _lib.GatherParams()
        lib.trt_gather_params_default(C.byref(p))
        p.path = cls._radiance_params(samples_per_item, **path)
        p.lobe, p.spread = cls.LOBES[lobe], float(spread)
        return p

    def gather(self, items, samples_per_item, lobe="cosine", spread=0.0, max_bounces=50, background=(0.0, 0.0, 0.0), seed=1, first_stream=0,
               sample_begin=0, sample_end=None, accumulate=False, radiance=None, moment2=None):
        """trt_gather: the light gathered at surfels float32 [n, 6] (point, axis; used as given, the axis is never normalised).  For each of
        samples_per_item = K samples the device draws a first ray about the axis - lobe "cosine": Lambertian::scatter's rule, the result is
        what a white diffuse surface there reflects (irradiance / pi); lobe "cone": axis + spread * (a point in the unit sphere), Metal's
        rule - from RNG stream (seed, first_stream + i * K + s, 1), traces its path on stream (.., 0) and folds per item.  Everything else
        - sample range, accumulate, `radiance`, `moment2`, the returns - as in radiance()."""
        r, _ = _rays_and_t_max(items, None)
        n = len(r)
        p = self._gather_params(samples_per_item, lobe, spread, max_bounces=max_bounces, background=background, seed=seed, first_stream=first_stream,
                                sample_begin=sample_begin, sample_end=sample_end, accumulate=accumulate)
        if radiance is None:
            radiance = np.zeros((n, 3), np.float32)
        if moment2 is True:
            moment2 = np.zeros((n, 3), np.float32)
        for a in (radiance, moment2):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (n, 3))
        st = Stats()
        check(lib.trt_gather(self._h, r.ctypes.data if n else None, n, C.byref(p), radiance.ctypes.data if n else None,
                             moment2.ctypes.data if moment2 is not None and n else None, C.byref(st)))
        return radiance, moment2, st.as_dict()

    def gather_device(self, d_items_ptr, n, d_radiance_ptr, d_moment2_ptr=0, d_counters_ptr=0, stream_ptr=0, **params):
        """Enqueue gather() on buffers already in HBM (device pointers as integers: n x 24 bytes of surfels, n x 12 bytes of sums each) on
        the current device; asynchronous on the stream, allocates nothing.  `params`: gather()'s keywords, samples_per_item included."""
        p = self._gather_params(**params)
        check(lib.trt_gather_device(self._h, C.c_void_p(d_items_ptr), int(n), C.byref(p), C.c_void_p(d_radiance_ptr), C.c_void_p(d_moment2_ptr),
                                    C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))

    def gather_plan(self, n, compute_units=0):
        """trt_gather_launch_plan: how gather() launches n surfels on this scene, as a dict with radiance_plan()'s fields."""
        plan = _lib.QueryPlan()
        check(lib.trt_gather_launch_plan(self._h, int(n), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    # ---- ambient queries (tinyrt.h trt_ambient): occlusion and bent normals from the first rays a gather query would draw ----
    @classmethod
    def _ambient_params(cls, samples_per_item, lobe="cosine", spread=0.0, max_distance=float("inf"), seed=1, first_stream=0, sample_begin=0,
                        sample_end=0, accumulate=False):
        """sample_end = 0 means samples_per_item, as at the C boundary."""
        if lobe not in cls.LOBES:
            raise ValueError("lobe must be 'cosine' or 'cone'")
        p = _lib.AmbientParams()
        lib.trt_ambient_params_default(C.byref(p))
        path = p.gather.path
        path.samples_per_ray, path.seed, path.first_stream = int(samples_per_item), int(seed), int(first_stream)
        path.sample_begin, path.sample_end, path.accumulate = int(sample_begin), int(sample_end), 1 if accumulate else 0
        p.gather.lobe, p.gather.spread, p.max_distance = cls.LOBES[lobe], float(spread), float(max_distance)
        return p

    def ambient(self, items, samples_per_item, lobe="cosine", spread=0.0, max_distance=float("inf"), seed=1, first_stream=0, sample_begin=0,
                sample_end=0, accumulate=False, visibility=None, bent=False):
        """trt_ambient: how open the lobe about surfels float32 [n, 6] (point, axis; used as given) is.  For each of samples_per_item = K
        samples the device draws gather()'s first ray - the same lobe, spread, seed and first_stream give the same rays, bit for bit - and
        asks occluded()'s question of it over [0.001, max_distance); an unoccluded sample adds 1 / K to visibility[i] and its unit
        direction / K to bent[i], an occluded one nothing.  With the cosine lobe 1 - visibility is ambient occlusion; max_distance = inf
        is sky visibility; bent is the bent normal, not renormalised.  Samples [sample_begin, sample_end) are traced (sample_end = 0: K).
        `visibility`: float32 [n] to write or, with accumulate, to continue (changed in place); None allocates one.  `bent`: float32
        [n, 3] likewise; True allocates one, False or None = not wanted.  Returns (visibility[n], bent[n, 3] or None, stats with samples
        and rays = occlusion walks)."""
        r, _ = _rays_and_t_max(items, None)
        n = len(r)
        p = self._ambient_params(samples_per_item, lobe, spread, max_distance, seed, first_stream, sample_begin, sample_end, accumulate)
        if visibility is None:
            visibility = np.zeros(n, np.float32)
        if bent is True:
            bent = np.zeros((n, 3), np.float32)
        elif bent is False:
            bent = None
        assert visibility.dtype == np.float32 and visibility.flags.c_contiguous and visibility.shape == (n,)
        assert bent is None or (bent.dtype == np.float32 and bent.flags.c_contiguous and bent.shape == (n, 3))
        st = Stats()
        check(lib.trt_ambient(self._h, r.ctypes.data if n else None, n, C.byref(p), visibility.ctypes.data if n else None,
                              bent.ctypes.data if bent is not None and n else None, C.byref(st)))
        return visibility, bent, st.as_dict()

    def ambient_device(self, d_items_ptr, n, d_visibility_ptr, d_bent_ptr=0, d_counters_ptr=0, stream_ptr=0, **params):
        """Enqueue ambient() on buffers already in HBM (device pointers as integers: n x 24 bytes of surfels, n x 4 bytes of visibility,
        n x 12 bytes of bent sums or 0) on the current device; asynchronous on the stream, allocates nothing.  `params`: ambient()'s
        keywords, samples_per_item included."""
        p = self._ambient_params(**params)
        check(lib.trt_ambient_device(self._h, C.c_void_p(d_items_ptr), int(n), C.byref(p), C.c_void_p(d_visibility_ptr), C.c_void_p(d_bent_ptr),
                                     C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))

    def ambient_plan(self, n, compute_units=0):
        """trt_ambient_launch_plan: how ambient() launches n surfels on this scene, as a dict with gather_plan()'s fields."""
        plan = _lib.QueryPlan()
        check(lib.trt_ambient_launch_plan(self._h, int(n), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    # ---- direct-light queries (tinyrt.h trt_direct): shadow rays the device draws towards a table of emitters ----
    def emitters(self):
        """trt_scene_emitters: the scene's own lights - the geometries whose material is a Light, in insertion order - as a record array
        of lights.EMITTER_DTYPE; needs no device.  A table for direct(): use it whole, slice it, or join it with lights.quad(...) /
        lights.sphere(...) records (lights.table)."""
        count = C.c_uint32(0)
        check(lib.trt_scene_emitters(self._h, None, 0, C.byref(count)))
        out = np.zeros(count.value, EMITTER_DTYPE)
        if count.value:
            check(lib.trt_scene_emitters(self._h, out.ctypes.data, count.value, C.byref(count)))
        return out

    @staticmethod
    def _direct_params(samples_per_item, shadow_end=None, seed=1, first_stream=0, sample_begin=0, sample_end=0, accumulate=False, mis=None):
        """sample_end = 0 means samples_per_item, as at the C boundary; shadow_end = None: the library's default (0.999).  mis = None: a
        trt_direct_params; "balance" or "power": a trt_direct_mis_params."""
        if mis is not None and mis not in Scene.MIS:
            raise ValueError("mis must be None, 'balance' or 'power'")
        p = _lib.DirectParams()
        lib.trt_direct_params_default(C.byref(p))
        path = p.path
        path.samples_per_ray, path.seed, path.first_stream = int(samples_per_item), int(seed), int(first_stream)
        path.sample_begin, path.sample_end, path.accumulate = int(sample_begin), int(sample_end), 1 if accumulate else 0
        if shadow_end is not None:
            p.shadow_end = float(shadow_end)
        return Scene._with_mis("direct", p, mis)

    @staticmethod
    def _emitter_table(emitters):
        e = np.ascontiguousarray(emitters)
        if e.dtype != EMITTER_DTYPE or e.ndim != 1:
            raise ValueError("emitters must be a one-dimensional record array of lights.EMITTER_DTYPE")
        return e

    @staticmethod
    def _pick_and_total(pick, mis):
        """pick= as direct() takes it: the records, or (records, total) as lights.pick_table returns them; mis needs the total."""
        total = None
        if isinstance(pick, tuple):
            pick, total = pick
        if mis is not None and total is None:
            raise ValueError("with mis, pick must be (records, total) as lights.pick_table(table) returns them")
        return pick, total

    def direct(self, items, emitters, samples_per_item, shadow_end=None, seed=1, first_stream=0, sample_begin=0, sample_end=0,
               accumulate=False, radiance=None, moment2=None, mis=None, pick=None):
        """trt_direct: the light that reaches surfels float32 [n, 6] (point, axis; used as given) straight from the emitters of a table
        (emitters(), lights.quad / lights.sphere records, or any mix).  Each of samples_per_item = K samples picks an emitter uniformly and
        a point on it from RNG stream (seed, first_stream + i * K + s, 1), and asks occluded()'s question of the normalised ray towards
        it over [0.001, distance * shadow_end); an unoccluded sample that faces the point adds colour * cos * |cos_l| * area * E /
        (pi * distance^2) / K.  With a unit axis the result is what a white diffuse surface reflects from those emitters alone -
        gather()'s convention, with far less noise.  Sample range, accumulate, `radiance`, `moment2` and the returns as in radiance()
        (sample_end = 0: K); stats carry samples and rays = the occlusion walks made.
        mis = "balance" | "power" (trt_direct_mis): every sample also sends one cosine-lobe ray from the surfel (stream (seed, j,
        0xFFFFFFFF)), and a light of the scene is counted both ways, the shadow sample scaled by 1 / (1 + q(p_bsdf / p_light)) and the
        lobe ray's hit on a light by its complement, q(x) = x or x * x: the same expectation without the 1/d2 tail of surfels beside a
        lamp, for one closest-hit walk more per sample (rays = occlusion walks + samples).  `emitters` must then hold exactly the scene's
        own lights (emitters()), each once, plus any virtual ones; anything else is an error.
        pick = lights.pick_table(emitters) (trt_direct_pick; with mis trt_direct_mis_pick): the emitter is chosen through that alias
        table, by power or by the weights the table was built from, not uniformly - one draw more per sample, far less noise where the
        emitters' powers differ much.  The records alone will do without mis; with mis the (records, total) pair is needed and the table
        must be the power table (weights=None).  pick=None: the calls and bytes of before."""
        return self._emitter_query("direct", items, emitters, pick, radiance, moment2, samples_per_item=samples_per_item, shadow_end=shadow_end, seed=seed,
                                   first_stream=first_stream, sample_begin=sample_begin, sample_end=sample_end, accumulate=accumulate, mis=mis)

    def direct_device(self, d_items_ptr, n, d_emitters_ptr, n_emitters, d_radiance_ptr, d_moment2_ptr=0, d_counters_ptr=0, stream_ptr=0, pick=None,
                      **params):
        """Enqueue direct() on buffers already in HBM (device pointers as integers: n x 24 bytes of surfels, n_emitters x 80 bytes of
        trt_emitter records, n x 12 bytes of sums each) on the current device; asynchronous on the stream, allocates nothing.  `params`:
        direct()'s keywords, samples_per_item and mis included (trt_direct_mis_device where mis is given: the device form cannot check the
        table rule).  pick: the device pointer of the n_emitters x 16 bytes of lights.pick_table's records (trt_direct_pick_device), or
        with mis (pointer, total) (trt_direct_mis_pick_device); the device form checks neither table."""
        self._emitter_query_device("direct", d_items_ptr, n, d_emitters_ptr, n_emitters, d_radiance_ptr, d_moment2_ptr, d_counters_ptr, stream_ptr, pick, params)

    def direct_plan(self, n, compute_units=0, mis=None, pick=None):
        """trt_direct_launch_plan (mis given: trt_direct_mis_launch_plan; pick given, as anything but None: the _pick_ plans): how
        direct() launches n surfels on this scene, as a dict with ambient_plan()'s fields."""
        return self._emitter_query_plan("direct", n, compute_units, mis, pick)

    # ---- what the eight queries over an emitter table share: {direct, nee} x {plain, mis} x {uniform, pick} ----
    @staticmethod
    def _with_mis(family, p, mis):
        """`p` as it is, or with mis the family's weighted parameters around it: trt_<family>_mis_params with their defaults."""
        if mis is None:
            return p
        m = {"direct": _lib.DirectMisParams, "nee": _lib.NeeMisParams}[family]()
        getattr(lib, "trt_%s_mis_params_default" % family)(C.byref(m))
        setattr(m, family, p)
        m.heuristic = Scene.MIS[mis]
        return m

    @staticmethod
    def _emitter_symbol(family, mis, pick, form=""):
        """trt_<family>[_mis][_pick]<form>: form is "", "_device" or "_launch_plan"; pick counts as given when it is anything but None."""
        return getattr(lib, "trt_" + family + ("" if mis is None else "_mis") + ("" if pick is None else "_pick") + form)

    def _emitter_query(self, family, items, emitters, pick, radiance, moment2, **params):
        """The host form of direct() / nee(): `params` are the keywords of the family's _params function, mis among them."""
        r, _ = _rays_and_t_max(items, None)
        n = len(r)
        e = self._emitter_table(emitters)
        p = getattr(self, "_%s_params" % family)(**params)
        mis = params["mis"]
        if radiance is None:
            radiance = np.zeros((n, 3), np.float32)
        if moment2 is True:
            moment2 = np.zeros((n, 3), np.float32)
        for a in (radiance, moment2):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (n, 3))
        st = Stats()
        args = [self._h, r.ctypes.data if n else None, n, e.ctypes.data if len(e) else None, len(e), C.byref(p)]
        if pick is not None:                                                # the records stand behind the table, the total behind the parameters
            pick, total = self._pick_and_total(pick, mis)
            k = np.ascontiguousarray(pick)
            if k.dtype != PICK_DTYPE or k.shape != (len(e),):
                raise ValueError("pick must be lights.PICK_DTYPE records, one per emitter")
            args.insert(4, k.ctypes.data if len(k) else None)
            if mis is not None:
                args.append(C.c_float(total))
        check(self._emitter_symbol(family, mis, pick)(*args, radiance.ctypes.data if n else None, moment2.ctypes.data if moment2 is not None and n else None,
                                                      C.byref(st)))
        return radiance, moment2, st.as_dict()

    def _emitter_query_device(self, family, d_items_ptr, n, d_emitters_ptr, n_emitters, d_radiance_ptr, d_moment2_ptr, d_counters_ptr, stream_ptr, pick, params):
        """The device form of direct() / nee(): pick is the table's device pointer, or with mis (pointer, total)."""
        p = getattr(self, "_%s_params" % family)(**params)
        mis = params.get("mis")
        args = [self._h, C.c_void_p(d_items_ptr), int(n), C.c_void_p(d_emitters_ptr), int(n_emitters), C.byref(p)]
        if pick is not None:
            d_pick_ptr, total = self._pick_and_total(pick, mis)
            args.insert(4, C.c_void_p(d_pick_ptr))
            if mis is not None:
                args.append(C.c_float(total))
        check(self._emitter_symbol(family, mis, pick, "_device")(*args, C.c_void_p(d_radiance_ptr), C.c_void_p(d_moment2_ptr), C.c_void_p(d_counters_ptr),
                                                                 C.c_void_p(stream_ptr)))

    def _emitter_query_plan(self, family, n, compute_units, mis, pick):
        plan = _lib.QueryPlan()
        check(self._emitter_symbol(family, mis, pick, "_launch_plan")(self._h, int(n), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    # ---- probe queries (tinyrt.h trt_probe): spherical-harmonic radiance from first rays the device draws over the sphere ----
    DOMAINS = {"sphere": _lib.PROBE_SPHERE, "hemisphere": _lib.PROBE_HEMISPHERE}

    @classmethod
    def _probe_params(cls, samples_per_item, bands=3, domain="sphere", **path):
        if domain not in cls.DOMAINS:
            raise ValueError("domain must be 'sphere' or 'hemisphere'")
        p = _lib.ProbeParams()
        lib.trt_probe_params_default(C.byref(p))
        p.path = cls._radiance_params(samples_per_item, **path)
        p.domain, p.bands = cls.DOMAINS[domain], int(bands)
        return p

    def probe(self, items, samples_per_item, bands=3, domain="sphere", max_bounces=50, background=(0.0, 0.0, 0.0), seed=1, first_stream=0,
              sample_begin=0, sample_end=None, accumulate=False, sh=None):
        """trt_probe: the radiance arriving at items float32 [n, 6] (point, axis; used as given) as a function of direction.  For each of
        samples_per_item = K samples the device draws a first ray uniformly over the sphere (domain "sphere") or over the hemisphere about
        the axis ("hemisphere") from RNG stream (seed, first_stream + i * K + s, 1), traces its path on stream (.., 0) as gather() does and
        adds colour * Y_k(direction) / K to coefficient k of the item, for the C = bands ** 2 real spherical-harmonic basis functions of
        tiny-raytracer_amd.sh.  Sample range and accumulate as in radiance().  `sh`: float32 [n, C, 3] to write or, with accumulate, to
        continue (changed in place); None allocates one.  Returns (sh[n, C, 3], stats with samples and rays)."""
        r, _ = _rays_and_t_max(items, None)
        n = len(r)
        p = self._probe_params(samples_per_item, bands, domain, max_bounces=max_bounces, background=background, seed=seed, first_stream=first_stream,
                               sample_begin=sample_begin, sample_end=sample_end, accumulate=accumulate)
        coeffs = int(bands) ** 2
        if sh is None:
            sh = np.zeros((n, coeffs, 3), np.float32)
        assert sh.dtype == np.float32 and sh.flags.c_contiguous and sh.shape == (n, coeffs, 3)
        st = Stats()
        check(lib.trt_probe(self._h, r.ctypes.data if n else None, n, C.byref(p), sh.ctypes.data if n else None, C.byref(st)))
        return sh, st.as_dict()

    def probe_device(self, d_items_ptr, n, d_sh_ptr, d_counters_ptr=0, stream_ptr=0, **params):
        """Enqueue probe() on buffers already in HBM (device pointers as integers: n x 24 bytes of items, n x bands ** 2 x 12 bytes of
        sums) on the current device; asynchronous on the stream, allocates nothing.  `params`: probe()'s keywords, samples_per_item
        included."""
        p = self._probe_params(**params)
        check(lib.trt_probe_device(self._h, C.c_void_p(d_items_ptr), int(n), C.byref(p), C.c_void_p(d_sh_ptr), C.c_void_p(d_counters_ptr),
                                   C.c_void_p(stream_ptr)))

    def probe_plan(self, n, bands=3, compute_units=0):
        """trt_probe_launch_plan: how probe() launches n items with this many bands on this scene, as a dict with gather_plan()'s fields."""
        plan = _lib.QueryPlan()
        check(lib.trt_probe_launch_plan(self._h, int(n), int(bands), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    def probe_parallel(self, items, samples_per_item, bands=3, domain="sphere", max_bounces=50, background=(0.0, 0.0, 0.0), seed=1,
                       first_stream=0, sample_begin=0, sample_end=None, accumulate=False, sh=None, record_bytes=0):
        """trt_probe_parallel: probe()'s arguments and probe()'s results, bit for bit, from a launch that fills the device whatever K is -
        the paths run a sample to a lane into a record buffer of the call's own and project_samples() folds the records, in chunks of
        min(n, record_bytes // (24 K)) items.  record_bytes = 0: the library's default (96 MiB, or one item's 24 K bytes where that is
        more); a buffer that holds no item is refused.  Returns (sh[n, C, 3], stats with samples and rays)."""
        r, _ = _rays_and_t_max(items, None)
        n = len(r)
        p = self._probe_params(samples_per_item, bands, domain, max_bounces=max_bounces, background=background, seed=seed, first_stream=first_stream,
                               sample_begin=sample_begin, sample_end=sample_end, accumulate=accumulate)
        coeffs = int(bands) ** 2
        if sh is None:
            sh = np.zeros((n, coeffs, 3), np.float32)
        assert sh.dtype == np.float32 and sh.flags.c_contiguous and sh.shape == (n, coeffs, 3)
        st = Stats()
        check(lib.trt_probe_parallel(self._h, r.ctypes.data if n else None, n, C.byref(p), sh.ctypes.data if n else None, C.byref(st),
                                     int(record_bytes)))
        return sh, st.as_dict()

    def probe_parallel_device(self, d_items_ptr, n, d_sh_ptr, d_records_ptr, record_bytes, d_counters_ptr=0, stream_ptr=0, **params):
        """Enqueue probe_parallel() on buffers already in HBM (device pointers as integers: n x 24 bytes of items, n x bands ** 2 x 12
        bytes of sums, record_bytes bytes of scratch for the records, which the sums must not overlap) on the current device;
        asynchronous on the stream, allocates nothing.  `params`: probe()'s keywords, samples_per_item included."""
        p = self._probe_params(**params)
        check(lib.trt_probe_parallel_device(self._h, C.c_void_p(d_items_ptr), int(n), C.byref(p), C.c_void_p(d_sh_ptr), C.c_void_p(d_counters_ptr),
                                            C.c_void_p(d_records_ptr), int(record_bytes), C.c_void_p(stream_ptr)))

    def probe_parallel_plan(self, n, range_length=None, compute_units=0):
        """trt_probe_parallel_launch_plan: how probe_parallel() launches the sample kernels of one chunk of n items with range_length
        samples each (None: 1) on this scene - samples_plan()'s answer."""
        plan = _lib.QueryPlan()
        check(lib.trt_probe_parallel_launch_plan(self._h, int(n), 1 if range_length is None else int(range_length), int(compute_units),
                                                 C.byref(plan)))
        return plan.as_dict()

    # ---- sample queries (tinyrt.h trt_samples): every sample's colour and first direction, a sample to a lane ----
    SAMPLE_SOURCES = {"rays": _lib.SAMPLE_RAYS, "cosine": _lib.SAMPLE_COSINE, "cone": _lib.SAMPLE_CONE, "sphere": _lib.SAMPLE_SPHERE,
                      "hemisphere": _lib.SAMPLE_HEMISPHERE}

    @classmethod
    def _samples_params(cls, samples_per_item, source="cosine", spread=0.0, **path):
        if source not in cls.SAMPLE_SOURCES:
            raise ValueError("source must be 'rays', 'cosine', 'cone', 'sphere' or 'hemisphere'")
        p = _lib.SamplesParams()
        lib.trt_samples_params_default(C.byref(p))
        p.path = cls._radiance_params(samples_per_item, **path)
        p.source, p.spread = cls.SAMPLE_SOURCES[source], float(spread)
        return p

    def samples(self, items, samples_per_item, source="cosine", spread=0.0, max_bounces=50, background=(0.0, 0.0, 0.0), seed=1, first_stream=0,
                sample_begin=0, sample_end=None, colors=None, directions=False):
        """trt_samples: the colour of EVERY sample of items float32 [n, 6], unfolded.  Sample s of item i, of samples_per_item = K, runs on
        RNG stream (seed, first_stream + i * K + s, 0); its first ray is the item itself (source "rays", as radiance()), gather()'s draw
        ("cosine", "cone" with `spread`) or probe()'s ("sphere", "hemisphere"), drawn on stream (.., 1).  Only samples [sample_begin,
        sample_end) are traced and written (None: K): calls over disjoint ranges fill one buffer.  `colors`: float32 [n, K, 3] to write
        into, None allocates zeros.  `directions`: True allocates float32 [n, K, 3] for the traced rays' stored directions, an array is
        written into, False / None = not wanted.  Returns (colors[n, K, 3], directions or None, stats with samples and rays).
        fold_samples() turns the colours into radiance() / gather()'s bytes, sh.project() colours and directions into probe()'s."""
        r, _ = _rays_and_t_max(items, None)
        n, k = len(r), int(samples_per_item)
        p = self._samples_params(k, source, spread, max_bounces=max_bounces, background=background, seed=seed, first_stream=first_stream,
                                 sample_begin=sample_begin, sample_end=sample_end)
        if colors is None:
            colors = np.zeros((n, k, 3), np.float32)
        if directions is True:
            directions = np.zeros((n, k, 3), np.float32)
        elif directions is False:
            directions = None
        for a in (colors, directions):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (n, k, 3))
        st = Stats()
        check(lib.trt_samples(self._h, r.ctypes.data if n else None, n, C.byref(p), colors.ctypes.data if n else None,
                              directions.ctypes.data if directions is not None and n else None, C.byref(st)))
        return colors, directions, st.as_dict()

    def samples_device(self, d_items_ptr, n, d_colors_ptr, d_directions_ptr=0, d_counters_ptr=0, stream_ptr=0, **params):
        """Enqueue samples() on buffers already in HBM (device pointers as integers: n x 24 bytes of items, n x K x 12 bytes of colours and,
        where wanted, of directions) on the current device; asynchronous on the stream, allocates nothing.  `params`: samples()'s
        keywords, samples_per_item included."""
        p = self._samples_params(**params)
        check(lib.trt_samples_device(self._h, C.c_void_p(d_items_ptr), int(n), C.byref(p), C.c_void_p(d_colors_ptr), C.c_void_p(d_directions_ptr),
                                     C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))

    def samples_plan(self, n, range_length=None, compute_units=0):
        """trt_samples_launch_plan: how samples() launches n items with range_length samples each (None: 1) on this scene, as a dict with
        gather_plan()'s fields; rays_per_wave = samples a wave owns."""
        plan = _lib.QueryPlan()
        check(lib.trt_samples_launch_plan(self._h, int(n), 1 if range_length is None else int(range_length), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    # ---- passes queries (tinyrt.h trt_passes): the gathered radiance split by the depth and the end of each path ----
    SOURCES = {"rays": _lib.PASSES_RAYS, "cosine": _lib.PASSES_COSINE, "cone": _lib.PASSES_CONE}

    @classmethod
    def _passes_params(cls, samples_per_item, depth_bins=3, source="cosine", spread=0.0, **path):
        if source not in cls.SOURCES:
            raise ValueError("source must be 'rays', 'cosine' or 'cone'")
        p = _lib.PassesParams()
        lib.trt_passes_params_default(C.byref(p))
        p.gather.path = cls._radiance_params(samples_per_item, **path)
        p.gather.lobe, p.gather.spread, p.depth_bins = cls.SOURCES[source], float(spread), int(depth_bins)
        return p

    def passes(self, items, samples_per_item, depth_bins=3, source="cosine", spread=0.0, max_bounces=50, background=(0.0, 0.0, 0.0), seed=1,
               first_stream=0, sample_begin=0, sample_end=None, accumulate=False, passes=None, spent=None):
        """trt_passes: the light radiance() (source "rays": items float32 [n, 6] are rays, used as given) or gather() (source "cosine" or
        "cone": items are surfels, the device draws gather()'s first rays bit for bit) folds into one colour, split by how each path ended
        and after how many scatters.  With B = depth_bins (1 .. 4) and b = min(depth, B - 1) a sample that ended at a light adds
        colour / K to slot b, one that missed everything to slot B + b, and one that ran out of bounces adds 1 / K to spent[i]; a sample
        touches no other slot (tiny-raytracer_amd.passes names the slots and sums them).  Sample range and accumulate as in radiance().
        `passes`: float32 [n, 2 B, 3] to write or, with accumulate, to continue (changed in place); None allocates one.  `spent`:
        float32 [n] likewise; None allocates one, False = not wanted.  Returns (passes[n, 2 B, 3], spent[n] or None, stats with samples
        and rays)."""
        r, _ = _rays_and_t_max(items, None)
        n = len(r)
        p = self._passes_params(samples_per_item, depth_bins, source, spread, max_bounces=max_bounces, background=background, seed=seed,
                                first_stream=first_stream, sample_begin=sample_begin, sample_end=sample_end, accumulate=accumulate)
        slots = 2 * int(depth_bins)
        if passes is None:
            passes = np.zeros((n, slots, 3), np.float32)
        if spent is None:
            spent = np.zeros(n, np.float32)
        elif spent is False:
            spent = None
        assert passes.dtype == np.float32 and passes.flags.c_contiguous and passes.shape == (n, slots, 3)
        assert spent is None or (spent.dtype == np.float32 and spent.flags.c_contiguous and spent.shape == (n,))
        st = Stats()
        check(lib.trt_passes(self._h, r.ctypes.data if n else None, n, C.byref(p), passes.ctypes.data if n else None,
                             spent.ctypes.data if spent is not None and n else None, C.byref(st)))
        return passes, spent, st.as_dict()

    def passes_device(self, d_items_ptr, n, d_passes_ptr, d_spent_ptr=0, d_counters_ptr=0, stream_ptr=0, **params):
        """Enqueue passes() on buffers already in HBM (device pointers as integers: n x 24 bytes of items, n x 2 depth_bins x 12 bytes of
        sums, n x 4 bytes of spent shares or 0) on the current device; asynchronous on the stream, allocates nothing.  `params`: passes()'s
        keywords, samples_per_item included."""
        p = self._passes_params(**params)
        check(lib.trt_passes_device(self._h, C.c_void_p(d_items_ptr), int(n), C.byref(p), C.c_void_p(d_passes_ptr), C.c_void_p(d_spent_ptr),
                                    C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))

    def passes_plan(self, n, depth_bins=3, compute_units=0):
        """trt_passes_launch_plan: how passes() launches n items with this many depth bins on this scene, as a dict with gather_plan()'s
        fields."""
        plan = _lib.QueryPlan()
        check(lib.trt_passes_launch_plan(self._h, int(n), int(depth_bins), int(compute_units), C.byref(plan)))
        return plan.as_dict()

    # ---- next-event queries (tinyrt.h trt_nee): the paths of radiance() / gather() with a shadow ray to the table at every diffuse hit ----
    MIS = {"balance": _lib.MIS_BALANCE, "power": _lib.MIS_POWER}

    @classmethod
    def _nee_params(cls, samples_per_item, source="cosine", spread=0.0, shadow_end=None, source_is_diffuse=False, mis=None, **path):
        """shadow_end = None: the library's default (0.999).  mis = None: a trt_nee_params; "balance" or "power": a trt_nee_mis_params."""
        if source not in cls.SOURCES:
            raise ValueError("source must be 'rays', 'cosine' or 'cone'")
        if mis is not None and mis not in cls.MIS:
            raise ValueError("mis must be None, 'balance' or 'power'")
        p = _lib.NeeParams()
        lib.trt_nee_params_default(C.byref(p))
        p.gather.path = cls._radiance_params(samples_per_item, **path)
        p.gather.lobe, p.gather.spread, p.source_is_diffuse = cls.SOURCES[source], float(spread), int(source_is_diffuse)
        if shadow_end is not None:
            p.shadow_end = float(shadow_end)
        return cls._with_mis("nee", p, mis)

    def nee(self, items, emitters, samples_per_item, source="cosine", spread=0.0, shadow_end=None, source_is_diffuse=False, max_bounces=50,
            background=(0.0, 0.0, 0.0), seed=1, first_stream=0, sample_begin=0, sample_end=None, accumulate=False, radiance=None, moment2=None,
            mis=None, pick=None):
        """trt_nee: what radiance() (source "rays": items float32 [n, 6] are rays, used as given) or gather() (source "cosine" or "cone":
        items are surfels) estimates, with the lights aimed at: the path of every sample is gather()'s bit for bit, at every Lambertian
        hit that leaves bounce budget one shadow ray goes to the emitter table as in direct() (stream (seed, j, 2 + scatters before)), and
        a light the path then reaches by a diffuse scatter counts as black, so nothing is counted twice.  `emitters` should be
        emitters(): a light left out is still hidden.  source_is_diffuse=True treats the first hit as diffusely reached too: with the
        cosine source the result is the surfel's indirect light only, and direct() + nee(source_is_diffuse=True) is a full bake.
        Sample range, accumulate, `radiance`, `moment2` and the returns as in radiance(); stats carry samples and rays = path segments
        plus shadow walks.
        mis = "balance" | "power" (trt_nee_mis): the same paths and shadow rays, but a light reached after a diffuse scatter (from the
        second hit on) is counted both ways, the shadow sample scaled by 1 / (1 + q(p_bsdf / p_light)) and the hit by its complement,
        q(x) = x or x * x: the same expectation without the 1/d2 tail of shadow samples beside a lamp.  `emitters` must then hold
        exactly the scene's own lights (emitters()), each once, plus any virtual ones; anything else is an error.
        pick = lights.pick_table(emitters) (trt_nee_pick; with mis trt_nee_mis_pick): every vertex's emitter is chosen through that alias
        table, by power or by the weights the table was built from, not uniformly - one draw more per vertex, as in direct().  The
        records alone will do without mis; with mis the (records, total) pair is needed and the table must be the power table
        (weights=None).  pick=None: the calls and bytes of before."""
        return self._emitter_query("nee", items, emitters, pick, radiance, moment2, samples_per_item=samples_per_item, source=source, spread=spread,
                                   shadow_end=shadow_end, source_is_diffuse=source_is_diffuse, mis=mis, max_bounces=max_bounces, background=background,
                                   seed=seed, first_stream=first_stream, sample_begin=sample_begin, sample_end=sample_end, accumulate=accumulate)

    def nee_device(self, d_items_ptr, n, d_emitters_ptr, n_emitters, d_radiance_ptr, d_moment2_ptr=0, d_counters_ptr=0, stream_ptr=0, pick=None,
                   **params):
        """Enqueue nee() on buffers already in HBM (device pointers as integers: n x 24 bytes of items, n_emitters x 80 bytes of
        trt_emitter records, n x 12 bytes of sums each) on the current device; asynchronous on the stream, allocates nothing.  `params`:
        nee()'s keywords, samples_per_item and mis included (trt_nee_mis_device where mis is given: the device form cannot check the
        table rule).  pick: the device pointer of the n_emitters x 16 bytes of lights.pick_table's records (trt_nee_pick_device), or with
        mis (pointer, total) (trt_nee_mis_pick_device); the device form checks neither table."""
        self._emitter_query_device("nee", d_items_ptr, n, d_emitters_ptr, n_emitters, d_radiance_ptr, d_moment2_ptr, d_counters_ptr, stream_ptr, pick, params)

    def nee_plan(self, n, compute_units=0, mis=None, pick=None):
        """trt_nee_launch_plan (mis given: trt_nee_mis_launch_plan; pick given, as anything but None: the _pick_ plans): how nee() launches
        n items on this scene, as a dict with gather_plan()'s fields."""
        return self._emitter_query_plan("nee", n, compute_units, mis, pick)

    # ---- sample-parallel next-event queries (tinyrt.h trt_nee_samples): every sample's colour of nee(), a lane per sample ----
    @classmethod
    def _nee_samples_params(cls, samples_per_item, mis=None, total=None, **nee):
        """A trt_nee_samples_params: nee()'s keywords (accumulate is not one), weighted where mis is given, total_power = total or 0."""
        q = cls._nee_params(samples_per_item, mis=mis, **nee)
        p = _lib.NeeSamplesParams()
        lib.trt_nee_samples_params_default(C.byref(p))
        if mis is None:
            p.query.nee = q
        else:
            p.query, p.weighted = q, 1
        p.total_power = 0.0 if total is None else float(total)
        return p

    def nee_samples(self, items, emitters, samples_per_item, source="cosine", spread=0.0, shadow_end=None, source_is_diffuse=False, max_bounces=50,
                    background=(0.0, 0.0, 0.0), seed=1, first_stream=0, sample_begin=0, sample_end=None, mis=None, pick=None, colors=None,
                    directions=False):
        """trt_nee_samples: the colour of EVERY sample of nee(), unfolded, traced a sample to a lane.  Keyword meanings are nee()'s: mis
        None | "balance" | "power", pick None or lights.pick_table(emitters) (with mis the (records, total) pair); together they choose
        the sibling whose sample is written - nee(), its mis, its pick or its mis + pick form - bit for bit.  Only samples [sample_begin,
        sample_end) are traced and written (None: K): calls over disjoint ranges fill one buffer.  `colors`, `directions` and the returns
        as in samples(): (colors[n, K, 3], directions or None, stats with samples and rays = path segments plus shadow walks).
        fold_samples() turns the colours into the sibling's radiance / moment2 bytes."""
        r, _ = _rays_and_t_max(items, None)
        n, k = len(r), int(samples_per_item)
        e = self._emitter_table(emitters)
        d_pick, total = None, None
        if pick is not None:
            pick, total = self._pick_and_total(pick, mis)
            pk = np.ascontiguousarray(pick)
            if pk.dtype != PICK_DTYPE or pk.shape != (len(e),):
                raise ValueError("pick must be lights.PICK_DTYPE records, one per emitter")
            d_pick = pk.ctypes.data if len(pk) else None
        p = self._nee_samples_params(k, mis=mis, total=total, source=source, spread=spread, shadow_end=shadow_end, source_is_diffuse=source_is_diffuse,
                                     max_bounces=max_bounces, background=background, seed=seed, first_stream=first_stream, sample_begin=sample_begin,
                                     sample_end=sample_end)
        if colors is None:
            colors = np.zeros((n, k, 3), np.float32)
        if directions is True:
            directions = np.zeros((n, k, 3), np.float32)
        elif directions is False:
            directions = None
        for a in (colors, directions):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (n, k, 3))
        st = Stats()
        check(lib.trt_nee_samples(self._h, r.ctypes.data if n else None, n, e.ctypes.data if len(e) else None, d_pick, len(e), C.byref(p),
                                  colors.ctypes.data if n else None, directions.ctypes.data if directions is not None and n else None, C.byref(st)))
        return colors, directions, st.as_dict()

    def nee_samples_device(self, d_items_ptr, n, d_emitters_ptr, n_emitters, d_colors_ptr, d_directions_ptr=0, d_counters_ptr=0, stream_ptr=0,
                           pick=None, **params):
        """Enqueue nee_samples() on buffers already in HBM (device pointers as integers: n x 24 bytes of items, n_emitters x 80 bytes of
        trt_emitter records, n x K x 12 bytes of colours and, where wanted, of directions) on the current device; asynchronous on the
        stream, allocates nothing.  `params`: nee_samples()'s keywords, samples_per_item and mis included.  pick: the device pointer of
        the n_emitters x 16 bytes of lights.pick_table's records, or with mis (pointer, total); the device form checks neither table."""
        mis = params.pop("mis", None)
        d_pick_ptr, total = None, None
        if pick is not None:
            d_pick_ptr, total = self._pick_and_total(pick, mis)
        p = self._nee_samples_params(mis=mis, total=total, **params)
        check(lib.trt_nee_samples_device(self._h, C.c_void_p(d_items_ptr), int(n), C.c_void_p(d_emitters_ptr), C.c_void_p(d_pick_ptr), int(n_emitters),
                                         C.byref(p), C.c_void_p(d_colors_ptr), C.c_void_p(d_directions_ptr), C.c_void_p(d_counters_ptr),
                                         C.c_void_p(stream_ptr)))

    def nee_samples_plan(self, n, range_length=None, mis=None, pick=False, compute_units=0):
        """trt_nee_samples_launch_plan: how nee_samples() launches n items with range_length samples each (None: 1) on this scene with the
        kernels of (mis given, pick given), as a dict with gather_plan()'s fields; rays_per_wave = samples a wave owns."""
        plan = _lib.QueryPlan()
        check(lib.trt_nee_samples_launch_plan(self._h, int(n), 1 if range_length is None else int(range_length), 0 if mis is None else 1,
                                              0 if pick is None or pick is False else 1, int(compute_units), C.byref(plan)))
        return plan.as_dict()

    def compact_nodes(self):
        """The culling tree as 16-byte nodes (f16 boxes rounded outward) if the scene is walked from global memory:
        (lo[n,3] float16, hi[n,3] float16, link[n] uint32), else None."""
        n = self.info()["num_cull_nodes"]
        words = np.zeros((n, 4), np.uint32)
        rc = lib.trt_scene_get_compact_nodes(self._h, words.ctypes.data, n)
        if rc == _lib.ERR_NOT_FOUND:
            return None
        check(rc)
        h = words[:, :3].copy().view(np.float16).reshape(n, 6)
        return h[:, :3], h[:, 3:], words[:, 3].copy()


class World:
    def __init__(self):
        self._h = C.c_void_p()
        check(lib.trt_world_create(C.byref(self._h)))
        self._scene = None
        self._scene_options = {}

    @property
    def scene_options(self):
        """trt_scene_options fields get_bvh() compiles the scene with (placement only: the frames never change)."""
        return dict(self._scene_options)

    @scene_options.setter
    def scene_options(self, options):
        self._scene_options = dict(options)
        self._scene = None

    def __del__(self):
        if getattr(self, "_h", None):
            lib.trt_world_destroy(self._h)
            self._h = None

    def add_material(self, name, material):
        check(lib.trt_world_add_material(self._h, name.encode(), C.byref(material.pod)))

    def get_material(self, name):
        idx = C.c_uint32()
        rc = lib.trt_world_get_material(self._h, name.encode(), C.byref(idx))
        if rc == _lib.ERR_NOT_FOUND:
            return None                      # world.rs:35-41 returns Option
        check(rc)
        return idx.value

    def add_geometry(self, geometry):
        self._scene = None
        if isinstance(geometry, Sphere):
            check(lib.trt_world_add_sphere(self._h, geometry.center, geometry.radius, geometry.material))
        elif isinstance(geometry, Quad):
            check(lib.trt_world_add_quad(self._h, geometry.corner, geometry.u, geometry.v, geometry.material))
        else:
            raise TypeError("geometry must be a Sphere or a Quad")

    def add_spheres(self, center_radius, material):
        """n x add_geometry(Sphere(...)) in array order, one call: center_radius float32 [n, 4] (x, y, z, radius), material uint32 [n]."""
        self._scene = None
        cr = np.ascontiguousarray(center_radius, np.float32).reshape(-1, 4)
        m = np.ascontiguousarray(material, np.uint32).reshape(-1)
        if len(m) != len(cr):
            raise ValueError("one material index per sphere")
        check(lib.trt_world_add_spheres(self._h, len(cr), cr.ctypes.data, m.ctypes.data))

    def num_geometries(self):
        return lib.trt_world_num_geometries(self._h)

    def get_bvh(self, on_device=False, **options):
        """World::get_bvh (world.rs:43-45).  `options`: see Scene; a scene compiled with options, or on the device, is not cached."""
        if options or on_device:
            return Scene(self, on_device=on_device, **options)
        if self._scene is None:
            self._scene = Scene(self, **self._scene_options)
        return self._scene


class Camera:
    def __init__(self, focus_distance, defocus_angle, position, look_at, up, vertical_fov, width, height):
        self.pod = CameraPOD()
        check(lib.trt_camera_init(C.byref(self.pod), focus_distance, defocus_angle, _v(position), _v(look_at), _v(up),
                                  vertical_fov, width, height))

    def get_image_size(self):
        return (self.pod.width, self.pod.height)

    @staticmethod
    def _ray_params(samples_per_pixel, seed, bands):
        p = RenderParams()
        p.samples_per_pixel, p.seed = int(samples_per_pixel), int(seed)
        for k, v in bands.items():
            if k not in ("band_rows", "band_stride", "band_offset", "rows_local"):
                raise TypeError(f"unknown band field {k!r}")
            setattr(p, k, v)
        return p

    def primary_rays(self, sample, samples_per_pixel, seed=1, **bands):
        """trt_primary_rays: float32 [rows, width, 6] (origin, direction) - the rays the render traces for sample `sample` of every pixel
        under this seed; `bands`: band_rows, band_stride, band_offset, rows_local as in trt_render_params (none: all rows)."""
        p = self._ray_params(samples_per_pixel, seed, bands)
        rows = p.rows_local if p.band_rows else self.pod.height
        out = np.zeros((rows, self.pod.width, 6), np.float32)
        check(lib.trt_primary_rays(C.byref(self.pod), C.byref(p), int(sample), out.ctypes.data if out.size else None))
        return out

    def primary_rays_device(self, sample, samples_per_pixel, d_rays_ptr, seed=1, stream_ptr=0, **bands):
        """Enqueue primary_rays() into a buffer already in HBM (rows x width x 24 bytes); asynchronous on the stream."""
        p = self._ray_params(samples_per_pixel, seed, bands)
        check(lib.trt_primary_rays_device(C.byref(self.pod), C.byref(p), int(sample), C.c_void_p(d_rays_ptr), C.c_void_p(stream_ptr)))


class Image:
    """utils/image.rs Image with gamma: holds the Imager's linear f32 sums; quantises on demand."""

    def __init__(self, accum, gamma=2.2):
        self.data = accum                    # (H, W, 3) float32, linear
        self.gamma = gamma

    @property
    def height(self):
        return self.data.shape[0]

    @property
    def width(self):
        return self.data.shape[1]

    def size(self):
        return (self.width, self.height)

    def to_u8(self):
        rgb = np.zeros(self.data.shape, np.uint8)
        src = np.ascontiguousarray(self.data, np.float32)
        check(lib.trt_tonemap_u8(src.ctypes.data, self.width * self.height, self.gamma, rgb.ctypes.data))
        return rgb

    def save(self, filename):
        from PIL import Image as PILImage
        PILImage.fromarray(self.to_u8(), "RGB").save(filename)


class Renderer:
    def __init__(self, samples_per_pixel, num_sampler_threads=1, max_bounces=50, progressbar=False,
                 background_color=None, seed=1, backend=_lib.BACKEND_AUTO):
        self.samples_per_pixel = int(samples_per_pixel)
        self.num_sampler_threads = int(num_sampler_threads)      # kept for signature parity; the GPU ignores it
        self.max_bounces = int(max_bounces)
        self.progressbar = bool(progressbar)
        self.background_color = _v(background_color) if background_color is not None else Vec3(0.0, 0.0, 0.0)
        self.seed = int(seed)
        self.backend = int(backend)
        self.last_stats = None
        self.tuning = {}                 # trt_tuning fields this renderer overrides (scheduling only: frames never change)

    def params(self, tuning=None, **over):
        """trt_render_params for this renderer; `tuning`: dict of trt_tuning fields for this call (on top of self.tuning)."""
        p = RenderParams()
        knobs = dict(self.tuning)
        knobs.update(tuning or {})
        if knobs:
            p._tuning_keepalive = globals()["tuning"](**knobs)       # the POD holds a pointer: keep the struct alive with it
            p.tuning = C.pointer(p._tuning_keepalive)
        p.samples_per_pixel = self.samples_per_pixel
        p.max_bounces = self.max_bounces
        p.background = self.background_color
        p.seed = self.seed
        p.backend = self.backend
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def render(self, camera, world, collect_stats=False, accum=None, **over):
        """Renderer::render: returns the finished Image (the reference returns a JoinHandle<Image>).
        `accum` continues earlier passes when over["accumulate"] is set."""
        scene = world.get_bvh() if isinstance(world, World) else world
        p = self.params(collect_stats=int(collect_stats), **over)      # 0 | 1 (reference tree) | 2 (culling tree)
        w, h = camera.get_image_size()
        rows = p.rows_local if p.band_rows else h
        if accum is None:
            accum = np.zeros((rows, w, 3), np.float32)
        assert accum.dtype == np.float32 and accum.flags.c_contiguous and accum.shape == (rows, w, 3)
        st = Stats()
        check(lib.trt_render(scene._h, C.byref(camera.pod), C.byref(p), accum.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        return Image(accum)

    def render_multi(self, camera, world, devices=None, accum=None, d_accum_ptr=None, collect_stats=False, **over):
        """Renderer::render over several GPUs of one node (trt_render_multi): one call, the whole Image back.  `devices`:
        list of ordinals (None = all visible).  With d_accum_ptr the frame is gathered into that buffer on devices[0]
        instead (trt_render_multi_device) and nothing is returned."""
        scene = world.get_bvh() if isinstance(world, World) else world
        p = self.params(collect_stats=int(collect_stats), **over)
        w, h = camera.get_image_size()
        ndev = len(devices) if devices is not None else 0
        dv = (C.c_int * ndev)(*devices) if ndev else None
        st = Stats()
        if d_accum_ptr is not None:
            check(lib.trt_render_multi_device(scene._h, C.byref(camera.pod), C.byref(p), dv, ndev, C.c_void_p(d_accum_ptr), C.byref(st)))
            self.last_stats = st.as_dict()
            return None
        if accum is None:
            accum = np.zeros((h, w, 3), np.float32)
        assert accum.dtype == np.float32 and accum.flags.c_contiguous and accum.shape == (h, w, 3)
        check(lib.trt_render_multi(scene._h, C.byref(camera.pod), C.byref(p), dv, ndev, accum.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        return Image(accum)

    def launch_plan(self, camera, scene, **over):
        """trt_streamed_launch_plan: how the streamed backend launches this render (host arithmetic only), as a dict."""
        plan = _lib.LaunchPlan()
        p = self.params(**over)
        check(lib.trt_streamed_launch_plan(scene._h, C.byref(camera.pod), C.byref(p), C.byref(plan)))
        return {n: getattr(plan, n) for n, _ in plan._fields_}

    def render_device(self, camera, scene, d_accum_ptr, stream_ptr=0, d_counters_ptr=0, **over):
        """Enqueue one pass on buffers already in HBM (device pointers as integers); asynchronous."""
        p = self.params(**over)
        check(lib.trt_render_device(scene._h, C.byref(camera.pod), C.byref(p), C.c_void_p(d_accum_ptr),
                                    C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))


    def render_moments(self, camera, world, collect_stats=False, accum=None, moment2=None, **over):
        """trt_render_moments: render() that also returns the per-pixel second moments - (accum, moment2, stats), both float32
        [rows, width, 3]: accum is render()'s frame bit for bit, moment2 the sum of c_s * c_s / spp over the same samples in the same order.
        Streamed backend only (BACKEND_AUTO or BACKEND_STREAMED).  `accum`, `moment2`: the buffers of earlier passes to continue
        (over["accumulate"] = 1); `over`: sample range, bands.  variance(accum, moment2, spp) turns the pair into the variance per pixel."""
        scene = world.get_bvh() if isinstance(world, World) else world
        p = self.params(collect_stats=int(collect_stats), **over)
        w, h = camera.get_image_size()
        rows = p.rows_local if p.band_rows else h
        bufs = []
        for a in (accum, moment2):
            if a is None:
                a = np.zeros((rows, w, 3), np.float32)
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (rows, w, 3)
            bufs.append(a)
        st = Stats()
        check(lib.trt_render_moments(scene._h, C.byref(camera.pod), C.byref(p), bufs[0].ctypes.data, bufs[1].ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        return bufs[0], bufs[1], self.last_stats

    def render_moments_device(self, camera, scene, d_accum_ptr, d_moment2_ptr, stream_ptr=0, d_counters_ptr=0, **over):
        """Enqueue render_moments() on buffers already in HBM (device pointers as integers, each rows x width x 12 bytes); asynchronous."""
        p = self.params(**over)
        check(lib.trt_render_moments_device(scene._h, C.byref(camera.pod), C.byref(p), C.c_void_p(d_accum_ptr), C.c_void_p(d_moment2_ptr),
                                            C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))

    def render_pixels(self, camera, world, pixels, accum, moment2=None, **over):
        """trt_render_pixels: trace only the listed pixels - `pixels`: uint32 local indices r * width + x, each at most once - and leave in
        `accum` (and `moment2`, or None: not wanted; float32 [rows, width, 3], changed in place) the bytes render_moments() would leave
        there for the same sample range, accumulate flag, bands and prior contents; every other pixel is untouched.  `over`: sample
        range, accumulate, bands.  Returns the stats (samples and rays)."""
        scene = world.get_bvh() if isinstance(world, World) else world
        p = self.params(**over)
        w, h = camera.get_image_size()
        rows = p.rows_local if p.band_rows else h
        px = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        for a in (accum, moment2):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (rows, w, 3))
        st = Stats()
        check(lib.trt_render_pixels(scene._h, C.byref(camera.pod), C.byref(p), px.ctypes.data if len(px) else None, len(px),
                                    accum.ctypes.data if accum is not None and accum.size else None,
                                    moment2.ctypes.data if moment2 is not None and moment2.size else None, C.byref(st)))
        self.last_stats = st.as_dict()
        return self.last_stats

    def render_pixels_device(self, camera, scene, d_pixels_ptr, n, d_accum_ptr, d_moment2_ptr=0, d_count_ptr=0, stream_ptr=0,
                             d_counters_ptr=0, **over):
        """Enqueue render_pixels() on buffers already in HBM (device pointers as integers: n uint32 indices, frames of rows x width x 12
        bytes); asynchronous on the stream.  The list is not validated: an index past the local image is skipped, duplicates are the
        caller's error.  `d_count_ptr`: a uint32 in HBM (as select_pixels_device writes it); the first min(count, n) entries are used."""
        p = self.params(**over)
        check(lib.trt_render_pixels_device(scene._h, C.byref(camera.pod), C.byref(p), C.c_void_p(d_pixels_ptr), int(n), C.c_void_p(d_count_ptr),
                                           C.c_void_p(d_accum_ptr), C.c_void_p(d_moment2_ptr), C.c_void_p(d_counters_ptr), C.c_void_p(stream_ptr)))

    def render_adaptive(self, camera, world, min_spp, step_spp, rel_tol, abs_tol=0.0):
        """Adaptive sampling with this renderer's samples_per_pixel N as the cap: every pixel gets samples [0, min_spp); then, while some
        are still too noisy (select_pixels) and fewer than N samples are done, those pixels alone get the next step_spp samples
        (render_pixels).  The active set only shrinks: a pixel once dropped is never sampled again.  Returns (frame, accum, moment2, count):
        the raw sums with their fixed 1 / N scale, count uint32 [H, W] = samples each pixel received (min_spp plus a multiple of
        step_spp, capped at N), and frame = accum * (float32(N) / float32(count)), the estimate of every pixel at its own count.  A
        pixel with count c holds exactly the bytes a full render of samples [0, c) would."""
        n_cap, min_spp, step_spp = self.samples_per_pixel, int(min_spp), int(step_spp)
        if not 2 <= min_spp <= n_cap or step_spp < 1:
            raise ValueError("render_adaptive needs 2 <= min_spp <= samples_per_pixel and step_spp >= 1")
        w, h = camera.get_image_size()
        accum, moment2, _ = self.render_moments(camera, world, sample_begin=0, sample_end=min_spp)
        count = np.full(h * w, min_spp, np.uint32)
        done = min_spp
        active = select_pixels(accum, moment2, n_cap, done, rel_tol, abs_tol)
        while len(active) and done < n_cap:
            nxt = min(done + step_spp, n_cap)
            self.render_pixels(camera, world, active, accum, moment2, sample_begin=done, sample_end=nxt, accumulate=1)
            count[active] = nxt
            done = nxt
            active = select_pixels(accum, moment2, n_cap, done, rel_tol, abs_tol, candidates=active)
        count = count.reshape(h, w)
        scale = np.float32(n_cap) / count.astype(np.float32)
        return accum * scale[..., None], accum, moment2, count

    def render_aov(self, camera, world, channels=tuple(AOV_CHANNELS), buffers=None, **over):
        """trt_render_aov: the first-hit feature buffers of this renderer's frame (same seed, samples and rays as render()), as a dict
        channel -> array [rows, width, 3] or [rows, width] for the `channels` asked (albedo, normal, depth, coverage: float32 sums over the
        samples; geometry, material: uint32 of sample 0, 0xFFFFFFFF on a miss).  `buffers`: the dict of an earlier pass to continue
        (over["accumulate"] = 1); `over`: sample range, bands."""
        scene = world.get_bvh() if isinstance(world, World) else world
        p = self.params(**over)
        w, h = camera.get_image_size()
        rows = p.rows_local if p.band_rows else h
        out = {}
        pod = _lib.AovBuffers()
        for name in channels:
            dtype, k = AOV_CHANNELS[name]                                  # KeyError: no such channel
            shape = (rows, w, 3) if k == 3 else (rows, w)
            a = buffers[name] if buffers is not None else np.zeros(shape, dtype)
            assert a.dtype == dtype and a.flags.c_contiguous and a.shape == shape
            out[name] = a
            setattr(pod, name, a.ctypes.data if a.size else None)
        check(lib.trt_render_aov(scene._h, C.byref(camera.pod), C.byref(p), C.byref(pod)))
        return out

    def render_aov_device(self, camera, scene, d_buffer_ptrs, stream_ptr=0, **over):
        """Enqueue render_aov() on buffers already in HBM: d_buffer_ptrs is a dict channel -> device pointer (as an integer) for the
        channels wanted; asynchronous on the stream."""
        p = self.params(**over)
        pod = _lib.AovBuffers()
        for name, ptr in d_buffer_ptrs.items():
            if name not in AOV_CHANNELS:
                raise KeyError(name)
            setattr(pod, name, ptr or None)
        check(lib.trt_render_aov_device(scene._h, C.byref(camera.pod), C.byref(p), C.byref(pod), C.c_void_p(stream_ptr)))


def tonemap_u8_device(d_accum_ptr, npixels, d_rgb_ptr, gamma=2.2, stream_ptr=0):
    """Imager finalisation on buffers in HBM (device pointers as integers): linear f32 sums -> gamma-corrected RGB8."""
    check(lib.trt_tonemap_u8_device(C.c_void_p(d_accum_ptr), int(npixels), float(gamma), C.c_void_p(d_rgb_ptr),
                                    C.c_void_p(stream_ptr)))


def variance(accum, moment2, samples_per_pixel):
    """trt_variance: the variance of every pixel's estimate from a frame and its second moments (Renderer.render_moments), float32 with
    the frames' shape less the channel axis: the trace over r, g, b of the unbiased variance of the mean; +inf where samples_per_pixel <= 1."""
    s = np.ascontiguousarray(accum, np.float32)
    m = np.ascontiguousarray(moment2, np.float32)
    if s.ndim < 1 or s.shape[-1] != 3 or m.shape != s.shape:
        raise ValueError("accum and moment2 must have the same shape [..., 3]")
    out = np.zeros(s.shape[:-1], np.float32)
    check(lib.trt_variance(s.ctypes.data if s.size else None, m.ctypes.data if s.size else None, out.size, int(samples_per_pixel),
                           out.ctypes.data if out.size else None))
    return out


def variance_device(d_accum_ptr, d_moment2_ptr, npixels, samples_per_pixel, d_variance_ptr, stream_ptr=0):
    """Enqueue variance() on buffers already in HBM (device pointers as integers; npixels floats out); asynchronous on the stream."""
    check(lib.trt_variance_device(C.c_void_p(d_accum_ptr), C.c_void_p(d_moment2_ptr), int(npixels), int(samples_per_pixel),
                                  C.c_void_p(d_variance_ptr), C.c_void_p(stream_ptr)))


def _fold_params(samples_per_item, sample_begin=0, sample_end=0, accumulate=False):
    p = _lib.RadianceParams()
    lib.trt_radiance_params_default(C.byref(p))
    p.samples_per_ray, p.sample_begin, p.sample_end, p.accumulate = int(samples_per_item), int(sample_begin), int(sample_end), 1 if accumulate else 0
    return p


def fold_samples(colors, samples_per_item, sample_begin=0, sample_end=0, radiance=None, moment2=None, accumulate=False):
    """trt_fold_samples: Scene.samples()'s colours float32 [n, K, 3] folded per item over samples [sample_begin, sample_end) (0: K) in
    order with the imager's rule, radiance += c / K and moment2 += c * c / K in f32 - for colours of source "rays", "cosine" or "cone" the
    bytes Scene.radiance() / Scene.gather() return.  `radiance`, `moment2`: float32 [n, 3] to write or, with accumulate, to continue (the
    fold of a later range; changed in place); radiance=None allocates one, moment2=None: True allocates one, None = not wanted.  Runs
    on the device; there is no CPU path.  Returns (radiance[n, 3], moment2 or None)."""
    c = np.ascontiguousarray(colors, np.float32)
    k = int(samples_per_item)
    if c.ndim != 3 or c.shape[1] != k or c.shape[2] != 3:
        raise ValueError("colors must have the shape [n, samples_per_item, 3]")
    n = c.shape[0]
    if radiance is None:
        radiance = np.zeros((n, 3), np.float32)
    if moment2 is True:
        moment2 = np.zeros((n, 3), np.float32)
    for a in (radiance, moment2):
        assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (n, 3))
    p = _fold_params(k, sample_begin, sample_end, accumulate)
    check(lib.trt_fold_samples(c.ctypes.data if n else None, n, C.byref(p), radiance.ctypes.data if n else None,
                               moment2.ctypes.data if moment2 is not None and n else None))
    return radiance, moment2


def fold_samples_device(d_colors_ptr, n, samples_per_item, d_radiance_ptr, d_moment2_ptr=0, sample_begin=0, sample_end=0, accumulate=False,
                        stream_ptr=0):
    """Enqueue fold_samples() on buffers already in HBM (device pointers as integers: n x K x 12 bytes of colours, n x 12 bytes of sums
    each; the sums must not overlap the colours); asynchronous on the stream, allocates nothing.  accumulate continues the sums."""
    p = _fold_params(samples_per_item, sample_begin, sample_end, accumulate)
    check(lib.trt_fold_samples_device(C.c_void_p(d_colors_ptr), int(n), C.byref(p), C.c_void_p(d_radiance_ptr), C.c_void_p(d_moment2_ptr),
                                      C.c_void_p(stream_ptr)))


def _project_params(samples_per_item, bands=3, sample_begin=0, sample_end=0, accumulate=False):
    p = _lib.ProbeParams()
    lib.trt_probe_params_default(C.byref(p))
    p.path = _fold_params(samples_per_item, sample_begin, sample_end, accumulate)
    p.bands = int(bands)
    return p


def project_samples(colors, directions, bands=3, sample_begin=0, sample_end=0, sh=None, accumulate=False, items=None):
    """trt_project_samples: Scene.samples()'s colours and directions float32 [n, K, 3] of source "sphere" or "hemisphere" folded per item
    over samples [sample_begin, sample_end) (0: K) in order against the bands ** 2 = C real spherical harmonics of tiny-raytracer_amd.sh,
    sh[k] += c * (Y_k(d) / K) in f32 - with `items` float32 [n, 6] (the probes; a sample of an item whose point has a NaN adds nothing,
    as one whose direction has) the bytes Scene.probe() returns.  `sh`: float32 [n, C, 3] to write or, with accumulate, to continue
    (changed in place); None allocates one.  Runs on the device; there is no CPU path (sh.project() is the numpy restatement).  Returns
    sh[n, C, 3]."""
    c, d = np.ascontiguousarray(colors, np.float32), np.ascontiguousarray(directions, np.float32)
    if c.ndim != 3 or c.shape[2] != 3 or d.shape != c.shape:
        raise ValueError("colors and directions must have the same shape [n, K, 3]")
    n, k = c.shape[0], c.shape[1]
    coeffs = int(bands) ** 2
    if sh is None:
        sh = np.zeros((n, coeffs, 3), np.float32)
    assert sh.dtype == np.float32 and sh.flags.c_contiguous and sh.shape == (n, coeffs, 3)
    if items is not None:
        items = np.ascontiguousarray(items, np.float32)
        assert items.shape == (n, 6)
    p = _project_params(k, bands, sample_begin, sample_end, accumulate)
    check(lib.trt_project_samples(c.ctypes.data if n else None, d.ctypes.data if n else None, items.ctypes.data if items is not None and n else None,
                                  n, C.byref(p), sh.ctypes.data if n else None))
    return sh


def project_samples_device(d_colors_ptr, d_directions_ptr, n, samples_per_item, d_sh_ptr, bands=3, sample_begin=0, sample_end=0, accumulate=False,
                           d_items_ptr=0, stream_ptr=0):
    """Enqueue project_samples() on buffers already in HBM (device pointers as integers: n x K x 12 bytes of colours and of directions,
    n x bands ** 2 x 12 bytes of sums, which must overlap neither; n x 24 bytes of items or 0); asynchronous on the stream, allocates
    nothing.  accumulate continues the sums."""
    p = _project_params(samples_per_item, bands, sample_begin, sample_end, accumulate)
    check(lib.trt_project_samples_device(C.c_void_p(d_colors_ptr), C.c_void_p(d_directions_ptr), C.c_void_p(d_items_ptr), int(n), C.byref(p),
                                         C.c_void_p(d_sh_ptr), C.c_void_p(stream_ptr)))


def select_pixels(accum, moment2, samples_per_pixel, samples_done, rel_tol, abs_tol=0.0, candidates=None):
    """trt_select_pixels: the candidates (uint32 pixel indices; None = every pixel) whose estimate after samples_done of samples_per_pixel
    samples is still too noisy - variance of the mean > rel_tol^2 * (r + g + b)^2 + abs_tol^2, as tinyrt.h spells it out - in candidate
    order, as a uint32 array.  `accum`, `moment2`: the running sums as Renderer.render_moments leaves them, float32 [..., 3].
    samples_done <= 1 keeps every candidate."""
    s = np.ascontiguousarray(accum, np.float32)
    m = np.ascontiguousarray(moment2, np.float32)
    if s.ndim < 1 or s.shape[-1] != 3 or m.shape != s.shape:
        raise ValueError("accum and moment2 must have the same shape [..., 3]")
    npixels = s.size // 3
    cand = None if candidates is None else np.ascontiguousarray(candidates, np.uint32).reshape(-1)
    n = npixels if cand is None else len(cand)
    out = np.zeros(n, np.uint32)
    count = C.c_uint32(0)
    check(lib.trt_select_pixels(s.ctypes.data if s.size else None, m.ctypes.data if s.size else None, npixels, int(samples_per_pixel),
                                int(samples_done), cand.ctypes.data if cand is not None and n else None, n, float(rel_tol), float(abs_tol),
                                out.ctypes.data if n else None, C.byref(count)))
    return out[:count.value].copy()


def select_scratch_bytes(n):
    """trt_select_scratch_bytes: what select_pixels_device needs as scratch for n candidates (host arithmetic)."""
    return int(lib.trt_select_scratch_bytes(int(n)))


def select_pixels_device(d_accum_ptr, d_moment2_ptr, npixels, samples_per_pixel, samples_done, n, rel_tol, abs_tol, d_selected_ptr, d_count_ptr,
                         d_scratch_ptr, scratch_bytes, d_candidates_ptr=0, stream_ptr=0):
    """Enqueue select_pixels() on buffers already in HBM (device pointers as integers): n candidates (d_candidates_ptr 0: pixel i), up to n
    indices and a uint32 count out; nothing is allocated, `d_scratch_ptr` holds at least select_scratch_bytes(n) bytes; asynchronous.
    The n words at d_selected_ptr must not overlap the n words at d_candidates_ptr (TinyRTError, ERR_INVALID_ARG): the kernels cannot
    compact in place - keep two lists and swap them.  (select_pixels, the host form, may be given its candidates' own array.)"""
    check(lib.trt_select_pixels_device(C.c_void_p(d_accum_ptr), C.c_void_p(d_moment2_ptr), int(npixels), int(samples_per_pixel), int(samples_done),
                                       C.c_void_p(d_candidates_ptr), int(n), float(rel_tol), float(abs_tol), C.c_void_p(d_selected_ptr),
                                       C.c_void_p(d_count_ptr), C.c_void_p(d_scratch_ptr), int(scratch_bytes),
                                       C.c_void_p(stream_ptr)))


def denoise_params(**over):
    """The library's default trt_denoise_params (iterations 4, normal_power_log2 7, sigma_albedo 0.1, sigma_depth 0.05) with `over`
    applied."""
    p = _lib.DenoiseParams()
    lib.trt_denoise_params_default(C.byref(p))
    for k, v in over.items():
        if k not in _lib.DenoiseParams.FIELDS:
            raise TypeError(f"unknown denoise parameter {k!r}")
        setattr(p, k, v)
    return p


def denoise_scratch_bytes(width, height, **params):
    """trt_denoise_scratch_bytes: what denoise_device needs as scratch for a width x height frame (host arithmetic; 0 = invalid)."""
    return int(lib.trt_denoise_scratch_bytes(int(width), int(height), C.byref(denoise_params(**params))))


def denoise_color(variance_ptr=None, sigma_color=None):
    """trt_denoise_color for trt_denoise_ex: the library's default sigma_color unless one is given; `variance_ptr`: address of the
    variance image (1 float per pixel, as variance() returns it) or None (term off)."""
    c = _lib.DenoiseColor()
    lib.trt_denoise_color_default(C.byref(c))
    c.variance = variance_ptr or None
    if sigma_color is not None:
        c.sigma_color = float(sigma_color)
    return c


def denoise(color, albedo=None, normal=None, depth=None, variance=None, sigma_color=None, **params):
    """trt_denoise: the edge-avoiding a-trous filter of tinyrt.h over a frame (float32 [H, W, 3], as Renderer.render leaves it) guided by
    the feature buffers of Renderer.render_aov - albedo and normal [H, W, 3], depth [H, W]; None switches a term off.  `params`:
    iterations, normal_power_log2, sigma_albedo, sigma_depth.  Returns float32 [H, W, 3]; the inputs are not changed.
    `variance` (float32 [H, W], as variance() returns it) switches on trt_denoise_ex's variance-guided colour stop with `sigma_color`
    (None: the library's default; <= 0: term off); without `variance` the call is trt_denoise as before."""
    c = np.ascontiguousarray(color, np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("color must be [H, W, 3]")
    h, w = c.shape[:2]
    pod = _lib.DenoiseInputs()
    keep = [c]
    pod.color = c.ctypes.data if c.size else None
    for name, a, shape in (("albedo", albedo, (h, w, 3)), ("normal", normal, (h, w, 3)), ("depth", depth, (h, w))):
        if a is None:
            continue
        a = np.ascontiguousarray(a, np.float32)
        if a.shape != shape:
            raise ValueError(f"{name} must be {list(shape)}")
        keep.append(a)
        setattr(pod, name, a.ctypes.data if a.size else None)
    out = np.zeros((h, w, 3), np.float32)
    if variance is None:
        check(lib.trt_denoise(C.byref(pod), w, h, C.byref(denoise_params(**params)), out.ctypes.data if out.size else None))
        return out
    v = np.ascontiguousarray(variance, np.float32)
    if v.shape != (h, w):
        raise ValueError(f"variance must be {[h, w]}")
    col = denoise_color(v.ctypes.data if v.size else None, sigma_color)
    check(lib.trt_denoise_ex(C.byref(pod), C.byref(col), w, h, C.byref(denoise_params(**params)), out.ctypes.data if out.size else None))
    return out


def denoise_device(d_color_ptr, width, height, d_out_ptr, d_scratch_ptr, scratch_bytes, d_albedo_ptr=0, d_normal_ptr=0, d_depth_ptr=0,
                   stream_ptr=0, d_variance_ptr=0, sigma_color=None, **params):
    """Enqueue denoise() on buffers already in HBM (device pointers as integers; a guide pointer of 0 switches its term off): nothing is
    allocated, `d_scratch_ptr` holds at least denoise_scratch_bytes(width, height) bytes; asynchronous on the stream.  `d_variance_ptr`
    (width x height floats, as variance_device() writes them) and `sigma_color` as in denoise(): trt_denoise_ex_device, same scratch."""
    pod = _lib.DenoiseInputs()
    pod.color, pod.albedo, pod.normal, pod.depth = (d_color_ptr or None, d_albedo_ptr or None, d_normal_ptr or None, d_depth_ptr or None)
    if d_variance_ptr:
        col = denoise_color(d_variance_ptr, sigma_color)
        check(lib.trt_denoise_ex_device(C.byref(pod), C.byref(col), int(width), int(height), C.byref(denoise_params(**params)),
                                        C.c_void_p(d_out_ptr), C.c_void_p(d_scratch_ptr), int(scratch_bytes), C.c_void_p(stream_ptr)))
        return
    check(lib.trt_denoise_device(C.byref(pod), int(width), int(height), C.byref(denoise_params(**params)), C.c_void_p(d_out_ptr),
                                 C.c_void_p(d_scratch_ptr), int(scratch_bytes), C.c_void_p(stream_ptr)))


def sample_batch(scene, points, max_bounces, background, seed=1, collect_stats=True):
    """trait Sampler in batch form: ctypes array of SamplePoint -> SampledColor.  collect_stats=False runs the production walk
    (no traversal counters) instead of the counting kernel on the reference tree."""
    n = len(points)
    out = (SampledColor * max(n, 1))()
    st = Stats()
    check(lib.trt_sample_batch(scene._h, C.byref(points) if n else None, n, C.byref(out), max_bounces, _v(background),
                               seed, C.byref(st) if collect_stats else None))
    return out, st.as_dict()
