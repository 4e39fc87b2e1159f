//! The reference crate's World / Camera / Renderer::render surface over libtinyrt.so (MI355X).
//!
//! Names, argument order and meaning follow the reference (paths relative to raytracer/src):
//!   World::{new, add_material, get_material, add_geometry}     hittable/world.rs:16-41
//!   Sphere::new(center, radius, material), Quad::new(corner, u, v, material)   sphere.rs:16, quad.rs:20
//!   Lambertian / Metal / Dielectric / Light ::new              material/*.rs
//!   Camera::new(focus_distance, defocus_angle, position, look_at, up, vertical_fov, width, height)   camera.rs:17-26
//!   Renderer::new(samples_per_pixel, num_sampler_threads, max_bounces, progressbar, background_color)   renderer.rs:21-35
//!   Renderer::render(&camera, &world)                          renderer.rs:37-79
//! Where the reference panics (duplicate material name, world.rs:29-31) this returns `Err(Error)`.
//! Never compiled (no Rust toolchain in the build image); see ../README.md.

use std::ffi::{CStr, CString};
use std::io::Write;
use std::ptr;

use tinyrt_sys as sys;

pub type Float = f32; // lib.rs:4

#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub message: String,
}

impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "tinyrt error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}

fn check(rc: i32) -> Result<(), Error> {
    if rc == sys::TRT_OK {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(sys::trt_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct Vec3 {
    pub x: Float,
    pub y: Float,
    pub z: Float,
}

impl Vec3 {
    pub fn new(x: Float, y: Float, z: Float) -> Self {
        Vec3 { x, y, z }
    }
    pub fn new_diagonal(v: Float) -> Self {
        Vec3 { x: v, y: v, z: v } // math/vec3.rs:23-25
    }
    pub fn zero() -> Self {
        Vec3::default() // math/vec3.rs:27-29
    }
    fn raw(self) -> sys::trt_vec3 {
        sys::trt_vec3 { x: self.x, y: self.y, z: self.z }
    }
}

/// Stands in for `Arc<Box<dyn Material>>`: an index into the world's material table.
pub type MaterialHandle = u32;

pub trait Material {
    fn pod(&self) -> sys::trt_material;
}

pub struct Lambertian(Vec3);
pub struct Metal(Vec3, Float);
pub struct Dielectric(Vec3, Float);
pub struct Light(Vec3);

impl Lambertian {
    pub fn new(albedo: Vec3) -> Self {
        Lambertian(albedo)
    }
}
impl Metal {
    pub fn new(albedo: Vec3, fuzz: Float) -> Self {
        Metal(albedo, fuzz)
    }
}
impl Dielectric {
    pub fn new(albedo: Vec3, refraction_index: Float) -> Self {
        Dielectric(albedo, refraction_index)
    }
}
impl Light {
    pub fn new(color: Vec3) -> Self {
        Light(color)
    }
}
impl Material for Lambertian {
    fn pod(&self) -> sys::trt_material {
        sys::trt_material { kind: sys::TRT_LAMBERTIAN, albedo: self.0.raw(), param: 0.0 }
    }
}
impl Material for Metal {
    fn pod(&self) -> sys::trt_material {
        sys::trt_material { kind: sys::TRT_METAL, albedo: self.0.raw(), param: self.1 }
    }
}
impl Material for Dielectric {
    fn pod(&self) -> sys::trt_material {
        sys::trt_material { kind: sys::TRT_DIELECTRIC, albedo: self.0.raw(), param: self.1 }
    }
}
impl Material for Light {
    fn pod(&self) -> sys::trt_material {
        sys::trt_material { kind: sys::TRT_LIGHT, albedo: self.0.raw(), param: 0.0 }
    }
}

/// The rule `World::gather` and `World::ambient` draw the first ray of a sample by (`enum trt_lobe`); `Cone` carries the spread.
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum Lobe {
    Cosine,
    Cone(Float),
}

/// The directions `World::probe` draws the first ray of a sample over (`enum trt_probe_domain`).
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum ProbeDomain {
    Sphere,
    Hemisphere,
}

/// Where `World::samples` takes the first ray of a sample from (`enum trt_sample_source`): the items are rays, surfels `World::gather`
/// draws about, or points `World::probe` draws about.
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum SampleSource {
    Rays,
    Lobe(Lobe),
    Probe(ProbeDomain),
}

/// Where `World::passes` takes the first ray of a sample from (`enum trt_passes_source`): the items are rays, or surfels the device draws
/// `World::gather`'s first rays about.
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum PassesSource {
    Rays,
    Lobe(Lobe),
}

/// How `World::nee_mis` and `World::direct_mis` weight a shadow ray against the hit a scattered ray makes (`enum trt_mis_heuristic`).
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum MisHeuristic {
    Balance,
    Power,
}

/// The `trt_nee_params` of `World::nee` and `World::nee_mis`.
fn nee_params(samples_per_item: u32, source: PassesSource, source_is_diffuse: bool, shadow_end: Float, max_bounces: u32, background: Vec3,
              seed: u32, first_stream: u32) -> sys::trt_nee_params {
    let mut params = sys::trt_nee_params::default();
    unsafe { sys::trt_nee_params_default(&mut params) };
    params.gather.path.samples_per_ray = samples_per_item;
    params.gather.path.max_bounces = max_bounces;
    params.gather.path.background = background.raw();
    params.gather.path.seed = seed;
    params.gather.path.first_stream = first_stream;
    params.shadow_end = shadow_end;
    params.source_is_diffuse = source_is_diffuse as u32;
    match source {
        PassesSource::Rays => params.gather.lobe = sys::TRT_PASSES_RAYS,
        PassesSource::Lobe(Lobe::Cosine) => params.gather.lobe = sys::TRT_PASSES_COSINE,
        PassesSource::Lobe(Lobe::Cone(spread)) => {
            params.gather.lobe = sys::TRT_PASSES_CONE;
            params.gather.spread = spread;
        }
    }
    params
}

pub enum Geometry {
    Sphere { center: Vec3, radius: Float, material: MaterialHandle },
    Quad { corner: Vec3, u: Vec3, v: Vec3, material: MaterialHandle },
}

pub struct Sphere;
impl Sphere {
    pub fn new(center: Vec3, radius: Float, material: MaterialHandle) -> Geometry {
        Geometry::Sphere { center, radius, material }
    }
}
pub struct Quad;
impl Quad {
    pub fn new(corner: Vec3, u: Vec3, v: Vec3, material: MaterialHandle) -> Geometry {
        Geometry::Quad { corner, u, v, material }
    }
}

/// A quad lamp that is no geometry of the scene, for the table of `World::direct` (`trt_emitter_init_quad`): it emits `color` from both faces.
pub fn quad_emitter(corner: Vec3, u: Vec3, v: Vec3, color: Vec3) -> sys::trt_emitter {
    let mut e = sys::trt_emitter::default();
    unsafe { sys::trt_emitter_init_quad(&mut e, corner.raw(), u.raw(), v.raw(), color.raw()) };
    e
}
/// A sphere lamp that is no geometry of the scene (`trt_emitter_init_sphere`).
pub fn sphere_emitter(centre: Vec3, radius: Float, color: Vec3) -> sys::trt_emitter {
    let mut e = sys::trt_emitter::default();
    unsafe { sys::trt_emitter_init_sphere(&mut e, centre.raw(), radius, color.raw()) };
    e
}

/// The fold of `World::samples`' colours (`trt_fold_samples`; runs on the device, needs no scene): per item over all `samples_per_item`
/// samples in order, `radiance += c / K` and `moment2 += c * c / K` in f32 - for the sources `Rays` and `Lobe` the sums `World::radiance` /
/// `World::gather` return.  `colors` holds `samples_per_item * 3` floats per item.  Returns `(radiance, moment2)`, 3 floats per item each.
pub fn fold_samples(colors: &[Float], samples_per_item: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
    let per_item = samples_per_item as usize * 3;
    if per_item == 0 || colors.len() % per_item != 0 || colors.len() / per_item > u32::MAX as usize {
        return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "colors holds n x samples_per_item x 3 floats".to_string() });
    }
    let n = colors.len() / per_item;
    let mut params = sys::trt_radiance_params::default();
    unsafe { sys::trt_radiance_params_default(&mut params) };
    params.samples_per_ray = samples_per_item;
    let mut radiance = vec![0.0 as Float; n * 3];
    let mut moment2 = vec![0.0 as Float; n * 3];
    check(unsafe { sys::trt_fold_samples(colors.as_ptr(), n as u32, &params, radiance.as_mut_ptr(), moment2.as_mut_ptr()) })?;
    Ok((radiance, moment2))
}

/// The probe fold of `World::samples`' colours and directions for `SampleSource::Probe` (`trt_project_samples`; runs on the device, needs
/// no scene): per item over all `samples_per_item` samples in order, `sh[k] += c * (Y_k(d) / K)` in f32 for the `bands * bands` real
/// spherical harmonics.  A sample whose direction has a NaN adds nothing; with `items` (the probes) neither does a sample of an item
/// whose point has one - then the result is `World::probe`'s, byte for byte.  Returns `bands * bands * 3` floats per item.
pub fn project_samples(colors: &[Float], directions: &[Float], samples_per_item: u32, bands: u32, items: Option<&[[Float; 6]]>)
                       -> Result<Vec<Float>, Error> {
    let per_item = samples_per_item as usize * 3;
    if per_item == 0 || colors.len() % per_item != 0 || colors.len() / per_item > u32::MAX as usize || directions.len() != colors.len() {
        return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "colors and directions hold n x samples_per_item x 3 floats each".to_string() });
    }
    let n = colors.len() / per_item;
    if !(1..=3).contains(&bands) {
        return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "bands must be 1, 2 or 3".to_string() });
    }
    if let Some(items) = items {
        if items.len() != n {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "items holds one probe per item".to_string() });
        }
    }
    let mut params = sys::trt_probe_params::default();
    unsafe { sys::trt_probe_params_default(&mut params) };
    params.path.samples_per_ray = samples_per_item;
    params.bands = bands;
    let mut sh = vec![0.0 as Float; n * (bands * bands) as usize * 3];
    let items_ptr = items.map_or(ptr::null(), |i| i.as_ptr() as *const sys::trt_ray);
    check(unsafe { sys::trt_project_samples(colors.as_ptr(), directions.as_ptr(), items_ptr, n as u32, &params, sh.as_mut_ptr()) })?;
    Ok(sh)
}

pub struct World {
    handle: *mut sys::trt_world,
    scene: *mut sys::trt_scene, // World::get_bvh(), cached until the world changes
}

// The library's handles are plain host data behind a mutex-free API; one thread at a time per handle.
unsafe impl Send for World {}

impl World {
    pub fn new() -> Result<Self, Error> {
        let mut handle = ptr::null_mut();
        check(unsafe { sys::trt_world_create(&mut handle) })?;
        Ok(World { handle, scene: ptr::null_mut() })
    }

    pub fn add_material(&mut self, name: &str, material: &dyn Material) -> Result<(), Error> {
        let cname = CString::new(name).map_err(|_| Error { code: sys::TRT_ERR_INVALID_ARG, message: "name contains NUL".into() })?;
        let pod = material.pod();
        check(unsafe { sys::trt_world_add_material(self.handle, cname.as_ptr(), &pod) })
    }

    pub fn get_material(&self, name: &str) -> Option<MaterialHandle> {
        let cname = CString::new(name).ok()?;
        let mut index = 0u32;
        let rc = unsafe { sys::trt_world_get_material(self.handle, cname.as_ptr(), &mut index) };
        if rc == sys::TRT_OK {
            Some(index)
        } else {
            None // world.rs:35-41 returns Option
        }
    }

    pub fn add_geometry(&mut self, geometry: Geometry) -> Result<(), Error> {
        self.invalidate();
        match geometry {
            Geometry::Sphere { center, radius, material } => {
                check(unsafe { sys::trt_world_add_sphere(self.handle, center.raw(), radius, material) })
            }
            Geometry::Quad { corner, u, v, material } => {
                check(unsafe { sys::trt_world_add_quad(self.handle, corner.raw(), u.raw(), v.raw(), material) })
            }
        }
    }

    /// World::get_bvh (world.rs:43-45): the reference-order BVH, packed for the GPU.
    fn get_bvh(&mut self) -> Result<*mut sys::trt_scene, Error> {
        if self.scene.is_null() {
            check(unsafe { sys::trt_scene_create(self.handle, &mut self.scene) })?;
        }
        Ok(self.scene)
    }

    /// The light that arrives along caller-supplied rays (`trt_radiance`): each `(origin, direction)` as six floats, used as given, is
    /// path traced with `samples_per_ray` samples and folded with the imager's 1 / K rule.  Sample `s` of ray `i` uses RNG stream
    /// `(seed, first_stream + i * samples_per_ray + s, 0)`.  Returns `(radiance, moment2)`, 3 floats per ray each: the mean colour and the
    /// mean of its square, as `trt_variance` takes them.
    pub fn radiance(&mut self, rays: &[[Float; 6]], samples_per_ray: u32, max_bounces: u32, background: Vec3, seed: u32,
                    first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if rays.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 rays in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_radiance_params::default();
        unsafe { sys::trt_radiance_params_default(&mut params) };
        params.samples_per_ray = samples_per_ray;
        params.max_bounces = max_bounces;
        params.background = background.raw();
        params.seed = seed;
        params.first_stream = first_stream;
        let mut radiance = vec![0.0 as Float; rays.len() * 3];
        let mut moment2 = vec![0.0 as Float; rays.len() * 3];
        check(unsafe {
            sys::trt_radiance(scene, rays.as_ptr() as *const sys::trt_ray, rays.len() as u32, &params, radiance.as_mut_ptr(),
                              moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// The light gathered at caller-supplied surfels (`trt_gather`): each `(point, axis)` as six floats, used as given.  For every one of
    /// `samples_per_item` samples the device draws a first ray about the axis - `Lobe::Cosine`: `Lambertian::scatter`'s rule, the result
    /// is what a white diffuse surface there reflects (irradiance / pi); `Lobe::Cone(spread)`: axis + spread * (a point in the unit
    /// sphere), `Metal::scatter`'s rule - from RNG stream `(seed, first_stream + i * samples_per_item + s, 1)`, traces its path on stream
    /// `(.., 0)` and folds per item.  Returns `(radiance, moment2)` as `radiance` does.
    pub fn gather(&mut self, items: &[[Float; 6]], samples_per_item: u32, lobe: Lobe, max_bounces: u32, background: Vec3, seed: u32,
                  first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_gather_params::default();
        unsafe { sys::trt_gather_params_default(&mut params) };
        params.path.samples_per_ray = samples_per_item;
        params.path.max_bounces = max_bounces;
        params.path.background = background.raw();
        params.path.seed = seed;
        params.path.first_stream = first_stream;
        match lobe {
            Lobe::Cosine => params.lobe = sys::TRT_LOBE_COSINE,
            Lobe::Cone(spread) => {
                params.lobe = sys::TRT_LOBE_CONE;
                params.spread = spread;
            }
        }
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_gather(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, &params, radiance.as_mut_ptr(),
                            moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// How open the lobe about caller-supplied surfels is (`trt_ambient`): for every one of `samples_per_item` samples the device draws
    /// the first ray `gather` would draw for the same `lobe`, `seed` and `first_stream`, and asks whether anything lies in
    /// `[0.001, max_distance)` along it (`Float::INFINITY`: sky visibility).  An unoccluded sample adds 1 / K to the item's visibility
    /// and its unit direction / K to the item's bent sum; an occluded one adds nothing.  Returns `(visibility, bent)`: one float and
    /// three floats per item; `bent` is not renormalised.
    pub fn ambient(&mut self, items: &[[Float; 6]], samples_per_item: u32, lobe: Lobe, max_distance: Float, seed: u32,
                   first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_ambient_params::default();
        unsafe { sys::trt_ambient_params_default(&mut params) };
        params.gather.path.samples_per_ray = samples_per_item;
        params.gather.path.seed = seed;
        params.gather.path.first_stream = first_stream;
        params.max_distance = max_distance;
        match lobe {
            Lobe::Cosine => params.gather.lobe = sys::TRT_LOBE_COSINE,
            Lobe::Cone(spread) => {
                params.gather.lobe = sys::TRT_LOBE_CONE;
                params.gather.spread = spread;
            }
        }
        let mut visibility = vec![0.0 as Float; items.len()];
        let mut bent = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_ambient(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, &params, visibility.as_mut_ptr(),
                             bent.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((visibility, bent))
    }

    /// The scene's own lights (`trt_scene_emitters`): the geometries whose material is a `Light`, in insertion order - a table for
    /// `direct`.  Needs no device.
    pub fn emitters(&mut self) -> Result<Vec<sys::trt_emitter>, Error> {
        let scene = self.get_bvh()?;
        let mut count = 0u32;
        check(unsafe { sys::trt_scene_emitters(scene, ptr::null_mut(), 0, &mut count) })?;
        let mut table = vec![sys::trt_emitter::default(); count as usize];
        if count > 0 {
            check(unsafe { sys::trt_scene_emitters(scene, table.as_mut_ptr(), count, &mut count) })?;
        }
        Ok(table)
    }

    /// The light that reaches caller-supplied surfels straight from the emitters of a table (`trt_direct`): `emitters()`, a part of it,
    /// or lights that are no geometry of the scene (`quad_emitter`, `sphere_emitter`).  Every one of `samples_per_item` samples picks an
    /// emitter uniformly and a point on it from RNG stream `(seed, first_stream + i * samples_per_item + s, 1)` and asks whether
    /// anything lies in `[0.001, distance * shadow_end)` along the normalised ray towards it; an unoccluded sample that faces the point
    /// adds its weighted colour / K.  With a unit axis the result is what a white diffuse surface reflects from those emitters alone:
    /// `gather`'s convention.  Returns `(radiance, moment2)` as `radiance` does.
    pub fn direct(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], samples_per_item: u32, shadow_end: Float, seed: u32,
                  first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items or emitters in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_direct_params::default();
        unsafe { sys::trt_direct_params_default(&mut params) };
        params.path.samples_per_ray = samples_per_item;
        params.path.seed = seed;
        params.path.first_stream = first_stream;
        params.shadow_end = shadow_end;
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_direct(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), emitters.len() as u32,
                            &params, radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// `direct` with multiple importance sampling (`trt_direct_mis`): every sample also sends one cosine-lobe ray from the surfel (RNG
    /// stream `(seed, j, 0xFFFFFFFF)`), and a light of the scene counts both ways, the shadow sample scaled by
    /// 1 / (1 + q(p_bsdf / p_light)) and the lobe ray's hit on a light by the complement, q(x) = x (`MisHeuristic::Balance`) or x * x
    /// (`Power`): the same expectation without the 1/d2 tail of surfels beside a lamp, for one closest-hit walk more per sample.
    /// `emitters` must hold exactly the scene's own lights (`emitters()`), each once, plus any virtual ones; anything else is an error.
    /// Returns `(radiance, moment2)` as `direct` does.
    pub fn direct_mis(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], samples_per_item: u32, heuristic: MisHeuristic,
                      shadow_end: Float, seed: u32, first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items or emitters in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_direct_mis_params::default();
        unsafe { sys::trt_direct_mis_params_default(&mut params) };
        params.direct.path.samples_per_ray = samples_per_item;
        params.direct.path.seed = seed;
        params.direct.path.first_stream = first_stream;
        params.direct.shadow_end = shadow_end;
        params.heuristic = match heuristic {
            MisHeuristic::Balance => sys::TRT_MIS_BALANCE,
            MisHeuristic::Power => sys::TRT_MIS_POWER,
        };
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_direct_mis(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), emitters.len() as u32,
                                &params, radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// The alias table over `emitters` (`trt_emitter_pick_build`) through which `direct_pick` and `direct_mis_pick` choose their
    /// emitter, and the weights' total: by power (`weights` = `None`; the table `direct_mis_pick` needs) or by the caller's weights,
    /// one finite non-negative value per emitter.  Host only.
    pub fn pick_table(emitters: &[sys::trt_emitter], weights: Option<&[Float]>) -> Result<(Vec<sys::trt_emitter_pick>, Float), Error> {
        if emitters.len() > u32::MAX as usize || weights.map_or(false, |w| w.len() != emitters.len()) {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "one weight per emitter, at most 2^32 - 1 emitters".to_string() });
        }
        let mut pick = vec![sys::trt_emitter_pick::default(); emitters.len()];
        let mut total: Float = 0.0;
        check(unsafe {
            sys::trt_emitter_pick_build(emitters.as_ptr(), emitters.len() as u32, weights.map_or(ptr::null(), |w| w.as_ptr()), pick.as_mut_ptr(),
                                        &mut total)
        })?;
        Ok((pick, total))
    }

    /// `direct` with the emitter of a sample chosen through `pick` (`trt_direct_pick`) - by power or by the weights the table was built
    /// from, not uniformly: one draw more per sample, far less noise where the emitters' powers differ much.
    pub fn direct_pick(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], pick: &[sys::trt_emitter_pick], samples_per_item: u32,
                       shadow_end: Float, seed: u32, first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize || pick.len() != emitters.len() {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "one pick record per emitter, at most 2^32 - 1 items or emitters".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_direct_params::default();
        unsafe { sys::trt_direct_params_default(&mut params) };
        params.path.samples_per_ray = samples_per_item;
        params.path.seed = seed;
        params.path.first_stream = first_stream;
        params.shadow_end = shadow_end;
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_direct_pick(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), pick.as_ptr(),
                                 emitters.len() as u32, &params, radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// `direct_mis` with the emitter chosen through `pick` (`trt_direct_mis_pick`): `pick` must be `pick_table(emitters, None)` - the
    /// power table - and `total_power` the total it returned; the lobe ray's hit on a light is weighted by the same probability.
    pub fn direct_mis_pick(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], pick: &[sys::trt_emitter_pick], total_power: Float,
                           samples_per_item: u32, heuristic: MisHeuristic, shadow_end: Float, seed: u32, first_stream: u32)
                           -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize || pick.len() != emitters.len() {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "one pick record per emitter, at most 2^32 - 1 items or emitters".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_direct_mis_params::default();
        unsafe { sys::trt_direct_mis_params_default(&mut params) };
        params.direct.path.samples_per_ray = samples_per_item;
        params.direct.path.seed = seed;
        params.direct.path.first_stream = first_stream;
        params.direct.shadow_end = shadow_end;
        params.heuristic = match heuristic {
            MisHeuristic::Balance => sys::TRT_MIS_BALANCE,
            MisHeuristic::Power => sys::TRT_MIS_POWER,
        };
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_direct_mis_pick(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), pick.as_ptr(),
                                     emitters.len() as u32, &params, total_power, radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// The radiance arriving at caller-supplied points as a function of direction (`trt_probe`): each `(point, axis)` as six floats, used
    /// as given.  For every one of `samples_per_item` samples the device draws a first ray uniformly over the sphere
    /// (`ProbeDomain::Sphere`) or over the hemisphere about the axis (`ProbeDomain::Hemisphere`) from RNG stream
    /// `(seed, first_stream + i * samples_per_item + s, 1)`, traces its path on stream `(.., 0)` and adds colour * Y_k(direction) / K to
    /// coefficient `k` of the item.  Returns `bands * bands * 3` floats per item: real spherical harmonics, coefficient `l (l + 1) + m`,
    /// then channel.
    pub fn probe(&mut self, items: &[[Float; 6]], samples_per_item: u32, bands: u32, domain: ProbeDomain, max_bounces: u32,
                 background: Vec3, seed: u32, first_stream: u32) -> Result<Vec<Float>, Error> {
        if items.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items in one call".to_string() });
        }
        if !(1..=3).contains(&bands) {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "bands must be 1, 2 or 3".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_probe_params::default();
        unsafe { sys::trt_probe_params_default(&mut params) };
        params.path.samples_per_ray = samples_per_item;
        params.path.max_bounces = max_bounces;
        params.path.background = background.raw();
        params.path.seed = seed;
        params.path.first_stream = first_stream;
        params.bands = bands;
        params.domain = match domain {
            ProbeDomain::Sphere => sys::TRT_PROBE_SPHERE,
            ProbeDomain::Hemisphere => sys::TRT_PROBE_HEMISPHERE,
        };
        let mut sh = vec![0.0 as Float; items.len() * (bands * bands) as usize * 3];
        check(unsafe {
            sys::trt_probe(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, &params, sh.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok(sh)
    }

    /// `probe` with a launch that fills the device whatever `samples_per_item` is (`trt_probe_parallel`): the same arguments and the same
    /// coefficients, bit for bit.  The paths run a sample to a GPU lane into a record buffer of the call's own and the records are
    /// folded on the device, in chunks of `min(n, record_bytes / (24 K))` items; `record_bytes = 0` takes the library's default.
    pub fn probe_parallel(&mut self, items: &[[Float; 6]], samples_per_item: u32, bands: u32, domain: ProbeDomain, max_bounces: u32,
                          background: Vec3, seed: u32, first_stream: u32, record_bytes: u64) -> Result<Vec<Float>, Error> {
        if items.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items in one call".to_string() });
        }
        if !(1..=3).contains(&bands) {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "bands must be 1, 2 or 3".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_probe_params::default();
        unsafe { sys::trt_probe_params_default(&mut params) };
        params.path.samples_per_ray = samples_per_item;
        params.path.max_bounces = max_bounces;
        params.path.background = background.raw();
        params.path.seed = seed;
        params.path.first_stream = first_stream;
        params.bands = bands;
        params.domain = match domain {
            ProbeDomain::Sphere => sys::TRT_PROBE_SPHERE,
            ProbeDomain::Hemisphere => sys::TRT_PROBE_HEMISPHERE,
        };
        let mut sh = vec![0.0 as Float; items.len() * (bands * bands) as usize * 3];
        check(unsafe {
            sys::trt_probe_parallel(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, &params, sh.as_mut_ptr(), ptr::null_mut(),
                                    record_bytes)
        })?;
        Ok(sh)
    }

    /// Every sample's colour and first direction, unfolded (`trt_samples`): a sample to a GPU lane, where `radiance`, `gather` and `probe`
    /// give the samples of an item one lane.  Sample `s` of item `i` runs on RNG stream `(seed, first_stream + i * samples_per_item + s, 0)`
    /// from the first ray `source` names.  Returns `(colors, directions)`, each `samples_per_item * 3` floats per item, record
    /// `i * samples_per_item + s`; `directions` holds the traced rays' stored directions.  `fold_samples` turns the colours of the sources
    /// `Rays` and `Lobe` into `radiance` / `gather`'s sums.
    pub fn samples(&mut self, items: &[[Float; 6]], samples_per_item: u32, source: SampleSource, max_bounces: u32, background: Vec3, seed: u32,
                   first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_samples_params::default();
        unsafe { sys::trt_samples_params_default(&mut params) };
        params.path.samples_per_ray = samples_per_item;
        params.path.max_bounces = max_bounces;
        params.path.background = background.raw();
        params.path.seed = seed;
        params.path.first_stream = first_stream;
        let (source, spread) = match source {
            SampleSource::Rays => (sys::TRT_SAMPLE_RAYS, 0.0),
            SampleSource::Lobe(Lobe::Cosine) => (sys::TRT_SAMPLE_COSINE, 0.0),
            SampleSource::Lobe(Lobe::Cone(spread)) => (sys::TRT_SAMPLE_CONE, spread),
            SampleSource::Probe(ProbeDomain::Sphere) => (sys::TRT_SAMPLE_SPHERE, 0.0),
            SampleSource::Probe(ProbeDomain::Hemisphere) => (sys::TRT_SAMPLE_HEMISPHERE, 0.0),
        };
        params.source = source;
        params.spread = spread;
        let floats = items.len() * samples_per_item as usize * 3;
        let mut colors = vec![0.0 as Float; floats];
        let mut directions = vec![0.0 as Float; floats];
        check(unsafe {
            sys::trt_samples(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, &params, colors.as_mut_ptr(), directions.as_mut_ptr(),
                             ptr::null_mut())
        })?;
        Ok((colors, directions))
    }

    /// The light `radiance` or `gather` folds into one colour, split by how each path ended and after how many scatters (`trt_passes`).
    /// With `PassesSource::Rays` each item is a ray used as given; with `PassesSource::Lobe` a surfel `(point, axis)` about which the
    /// device draws `gather`'s first rays, bit for bit.  With `B = depth_bins` (1 to 4) and `b = min(depth, B - 1)` a sample that ended
    /// at a light adds colour / K to slot `b`, one that missed everything to slot `B + b`, and one that ran out of bounces adds 1 / K
    /// to the item's spent share.  Returns `(passes, spent)`: `2 * depth_bins * 3` floats per item and one float per item.
    pub fn passes(&mut self, items: &[[Float; 6]], samples_per_item: u32, depth_bins: u32, source: PassesSource, max_bounces: u32,
                  background: Vec3, seed: u32, first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items in one call".to_string() });
        }
        if !(1..=4).contains(&depth_bins) {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "depth_bins must be 1, 2, 3 or 4".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_passes_params::default();
        unsafe { sys::trt_passes_params_default(&mut params) };
        params.gather.path.samples_per_ray = samples_per_item;
        params.gather.path.max_bounces = max_bounces;
        params.gather.path.background = background.raw();
        params.gather.path.seed = seed;
        params.gather.path.first_stream = first_stream;
        params.depth_bins = depth_bins;
        match source {
            PassesSource::Rays => params.gather.lobe = sys::TRT_PASSES_RAYS,
            PassesSource::Lobe(Lobe::Cosine) => params.gather.lobe = sys::TRT_PASSES_COSINE,
            PassesSource::Lobe(Lobe::Cone(spread)) => {
                params.gather.lobe = sys::TRT_PASSES_CONE;
                params.gather.spread = spread;
            }
        }
        let mut passes = vec![0.0 as Float; items.len() * 2 * depth_bins as usize * 3];
        let mut spent = vec![0.0 as Float; items.len()];
        check(unsafe {
            sys::trt_passes(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, &params, passes.as_mut_ptr(), spent.as_mut_ptr(),
                            ptr::null_mut())
        })?;
        Ok((passes, spent))
    }

    /// What `radiance` (`PassesSource::Rays`) or `gather` (`PassesSource::Lobe`) estimates, with the lights aimed at (`trt_nee`): the
    /// path of every sample is theirs bit for bit, at every Lambertian hit that leaves bounce budget one shadow ray goes to the emitter
    /// table as in `direct`, and a light the path then reaches by a diffuse scatter counts as black.  `emitters` should be
    /// `emitters()`: a light left out is still hidden.  With `source_is_diffuse` the first hit counts as diffusely reached too: for a
    /// cosine source the result is the surfel's indirect light, and `direct` + `nee` is a full bake.  Returns `(radiance, moment2)` as
    /// `radiance` does.
    pub fn nee(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], samples_per_item: u32, source: PassesSource,
               source_is_diffuse: bool, shadow_end: Float, max_bounces: u32, background: Vec3, seed: u32, first_stream: u32)
               -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items or emitters in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let params = nee_params(samples_per_item, source, source_is_diffuse, shadow_end, max_bounces, background, seed, first_stream);
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_nee(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), emitters.len() as u32, &params,
                         radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// `nee` with multiple importance sampling (`trt_nee_mis`): the same paths and shadow rays, but a light reached after a diffuse
    /// scatter (from the second hit on) counts both ways, the shadow sample scaled by 1 / (1 + q(p_bsdf / p_light)) and the hit by the
    /// complement, q(x) = x (`MisHeuristic::Balance`) or x * x (`Power`): the same expectation without the 1/d2 tail of shadow samples
    /// beside a lamp.  `emitters` must hold exactly the scene's own lights (`emitters()`), each once, plus any virtual ones; anything else
    /// is an error.  Returns `(radiance, moment2)` as `nee` does.
    pub fn nee_mis(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], samples_per_item: u32, source: PassesSource,
                   source_is_diffuse: bool, heuristic: MisHeuristic, shadow_end: Float, max_bounces: u32, background: Vec3, seed: u32,
                   first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items or emitters in one call".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_nee_mis_params::default();
        unsafe { sys::trt_nee_mis_params_default(&mut params) };
        params.nee = nee_params(samples_per_item, source, source_is_diffuse, shadow_end, max_bounces, background, seed, first_stream);
        params.heuristic = match heuristic {
            MisHeuristic::Balance => sys::TRT_MIS_BALANCE,
            MisHeuristic::Power => sys::TRT_MIS_POWER,
        };
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_nee_mis(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), emitters.len() as u32, &params,
                             radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// `nee` with the emitter of every vertex's shadow ray chosen through `pick` (`trt_nee_pick`; `pick_table`) - by power or by the
    /// weights the table was built from, not uniformly: one draw more per vertex, far less noise where the emitters' powers differ much.
    pub fn nee_pick(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], pick: &[sys::trt_emitter_pick], samples_per_item: u32,
                    source: PassesSource, source_is_diffuse: bool, shadow_end: Float, max_bounces: u32, background: Vec3, seed: u32,
                    first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items or emitters in one call".to_string() });
        }
        if pick.len() != emitters.len() {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "the pick table needs one record per emitter".to_string() });
        }
        let scene = self.get_bvh()?;
        let params = nee_params(samples_per_item, source, source_is_diffuse, shadow_end, max_bounces, background, seed, first_stream);
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_nee_pick(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), pick.as_ptr(),
                              emitters.len() as u32, &params, radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// `nee_mis` with the emitter chosen through `pick` (`trt_nee_mis_pick`): `pick` must be `pick_table(emitters, None)` - the power
    /// table - and `total_power` the total it reported; a light reached after a diffuse scatter is weighted by the same probability.
    pub fn nee_mis_pick(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], pick: &[sys::trt_emitter_pick], total_power: Float,
                        samples_per_item: u32, source: PassesSource, source_is_diffuse: bool, heuristic: MisHeuristic, shadow_end: Float,
                        max_bounces: u32, background: Vec3, seed: u32, first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items or emitters in one call".to_string() });
        }
        if pick.len() != emitters.len() {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "the pick table needs one record per emitter".to_string() });
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_nee_mis_params::default();
        unsafe { sys::trt_nee_mis_params_default(&mut params) };
        params.nee = nee_params(samples_per_item, source, source_is_diffuse, shadow_end, max_bounces, background, seed, first_stream);
        params.heuristic = match heuristic {
            MisHeuristic::Balance => sys::TRT_MIS_BALANCE,
            MisHeuristic::Power => sys::TRT_MIS_POWER,
        };
        let mut radiance = vec![0.0 as Float; items.len() * 3];
        let mut moment2 = vec![0.0 as Float; items.len() * 3];
        check(unsafe {
            sys::trt_nee_mis_pick(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), pick.as_ptr(),
                                  emitters.len() as u32, &params, total_power, radiance.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((radiance, moment2))
    }

    /// Every sample's colour and first direction of the next-event queries, unfolded (`trt_nee_samples`): `samples` for `nee`, `nee_mis`,
    /// `nee_pick` and `nee_mis_pick`.  `heuristic` (`None`: unweighted) and `pick` (`None`: the uniform choice; else the records and, for
    /// the weighted sample, the total `pick_table` reported) select the sibling whose sample is written, bit for bit.  Returns
    /// `(colors, directions)`, each `samples_per_item * 3` floats per item, record `i * samples_per_item + s`; `fold_samples` turns the
    /// colours into the sibling's sums.
    pub fn nee_samples(&mut self, items: &[[Float; 6]], emitters: &[sys::trt_emitter], pick: Option<(&[sys::trt_emitter_pick], Float)>,
                       samples_per_item: u32, source: PassesSource, source_is_diffuse: bool, heuristic: Option<MisHeuristic>, shadow_end: Float,
                       max_bounces: u32, background: Vec3, seed: u32, first_stream: u32) -> Result<(Vec<Float>, Vec<Float>), Error> {
        if items.len() > u32::MAX as usize || emitters.len() > u32::MAX as usize {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "more than 2^32 - 1 items or emitters in one call".to_string() });
        }
        if let Some((records, _)) = pick {
            if records.len() != emitters.len() {
                return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "the pick table needs one record per emitter".to_string() });
            }
        }
        let scene = self.get_bvh()?;
        let mut params = sys::trt_nee_samples_params::default();
        unsafe { sys::trt_nee_samples_params_default(&mut params) };
        params.query.nee = nee_params(samples_per_item, source, source_is_diffuse, shadow_end, max_bounces, background, seed, first_stream);
        if let Some(h) = heuristic {
            params.weighted = 1;
            params.query.heuristic = match h {
                MisHeuristic::Balance => sys::TRT_MIS_BALANCE,
                MisHeuristic::Power => sys::TRT_MIS_POWER,
            };
        }
        let pick_ptr = match pick {
            Some((records, total)) => {
                params.total_power = total;
                records.as_ptr()
            }
            None => ptr::null(),
        };
        let floats = items.len() * samples_per_item as usize * 3;
        let mut colors = vec![0.0 as Float; floats];
        let mut directions = vec![0.0 as Float; floats];
        check(unsafe {
            sys::trt_nee_samples(scene, items.as_ptr() as *const sys::trt_ray, items.len() as u32, emitters.as_ptr(), pick_ptr, emitters.len() as u32,
                                 &params, colors.as_mut_ptr(), directions.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((colors, directions))
    }

    /// Frees the device scratch (render workspaces, frame buffers) the compiled scene caches between renders.
    pub fn trim(&mut self) -> Result<(), Error> {
        if self.scene.is_null() {
            return Ok(());
        }
        check(unsafe { sys::trt_scene_trim(self.scene) })
    }

    fn invalidate(&mut self) {
        if !self.scene.is_null() {
            unsafe { sys::trt_scene_destroy(self.scene) };
            self.scene = ptr::null_mut();
        }
    }
}

impl Drop for World {
    fn drop(&mut self) {
        self.invalidate();
        unsafe { sys::trt_world_destroy(self.handle) };
    }
}

pub struct Camera {
    pod: sys::trt_camera,
}

impl Camera {
    #[allow(clippy::too_many_arguments)]
    pub fn new(focus_distance: Float, defocus_angle: Float, position: Vec3, look_at: Vec3, up: Vec3, vertical_fov: Float,
               width: usize, height: usize) -> Result<Self, Error> {
        let mut pod = sys::trt_camera::default();
        check(unsafe {
            sys::trt_camera_init(&mut pod, focus_distance, defocus_angle, position.raw(), look_at.raw(), up.raw(), vertical_fov,
                                 width as u32, height as u32)
        })?;
        Ok(Camera { pod })
    }

    pub fn get_image_size(&self) -> (usize, usize) {
        (self.pod.width as usize, self.pod.height as usize) // camera.rs:68-70
    }

    /// The rays `Renderer::render` traces for sample `sample` of every pixel under `seed` (trt_primary_rays): width * height rays,
    /// row-major, each (origin, direction) as six floats.
    pub fn primary_rays(&self, sample: u32, samples_per_pixel: u32, seed: u32) -> Result<Vec<[Float; 6]>, Error> {
        let (width, height) = self.get_image_size();
        let params = sys::trt_render_params { samples_per_pixel, seed, ..Default::default() };
        let mut rays = vec![[0.0 as Float; 6]; width * height];
        check(unsafe { sys::trt_primary_rays(&self.pod, &params, sample, rays.as_mut_ptr() as *mut sys::trt_ray) })?;
        Ok(rays)
    }
}

/// The first-hit feature buffers of a frame (trt_render_aov): sums over the samples in the imager's order, indices of sample 0
/// (0xFFFFFFFF on a miss).  Row-major, width * height pixels each.
pub struct FeatureBuffers {
    pub width: usize,
    pub height: usize,
    pub albedo: Vec<Float>,   // 3 per pixel
    pub normal: Vec<Float>,   // 3 per pixel; not renormalised
    pub depth: Vec<Float>,
    pub coverage: Vec<Float>,
    pub geometry: Vec<u32>,
    pub material: Vec<u32>,
}

/// utils/image.rs Image with gamma 2.2 as the Imager builds it (imager.rs:37-41); holds the linear sums.
pub struct Image {
    width: usize,
    height: usize,
    gamma: Float,
    data: Vec<Float>,
}

impl Image {
    pub fn size(&self) -> (usize, usize) {
        (self.width, self.height)
    }
    /// Linear (not gamma-corrected) pixel, image.rs:46-48.
    pub fn get_pixel(&self, x: usize, y: usize) -> Vec3 {
        let i = (y * self.width + x) * 3;
        Vec3::new(self.data[i], self.data[i + 1], self.data[i + 2])
    }
    pub fn linear(&self) -> &[Float] {
        &self.data
    }
    /// Color::gamma_correction + From<Color> for Rgb<u8> (image.rs:92-111).
    pub fn to_rgb8(&self) -> Result<Vec<u8>, Error> {
        let mut rgb = vec![0u8; self.data.len()];
        check(unsafe { sys::trt_tonemap_u8(self.data.as_ptr(), (self.width * self.height) as u32, self.gamma, rgb.as_mut_ptr()) })?;
        Ok(rgb)
    }
    /// Binary PPM; the reference writes PNG through the `image` crate (image.rs:66-69): feed `to_rgb8` to it for that.
    pub fn save(&self, filename: &str) -> Result<(), Box<dyn std::error::Error>> {
        let rgb = self.to_rgb8()?;
        let mut f = std::fs::File::create(filename)?;
        write!(f, "P6\n{} {}\n255\n", self.width, self.height)?;
        f.write_all(&rgb)?;
        Ok(())
    }
}

#[derive(Clone, Copy)]
pub struct Renderer {
    samples_per_pixel: usize,
    #[allow(dead_code)]
    num_sampler_threads: usize, // the GPU needs no sampler-task count; kept for signature parity
    max_bounces: usize,
    #[allow(dead_code)]
    progressbar: bool,
    background_color: Vec3,
    pub seed: u32,    // trt-rng v1 seed (the reference has no seed API)
    pub backend: u32, // one of the TRT_BACKEND constants of tinyrt-sys
    /// Scheduling knobs (`sys::trt_tuning`, from `Renderer::default_tuning()`); `None` = the library defaults.  Scheduling only:
    /// whatever the values, the frame is the same.
    pub tuning: Option<sys::trt_tuning>,
}

impl Renderer {
    pub fn new(samples_per_pixel: usize, num_sampler_threads: usize, max_bounces: usize, progressbar: bool,
               background_color: Option<Vec3>) -> Self {
        Renderer {
            samples_per_pixel,
            num_sampler_threads,
            max_bounces,
            progressbar,
            background_color: background_color.unwrap_or_else(Vec3::zero), // renderer.rs:33
            seed: 1,
            backend: sys::TRT_BACKEND_AUTO,
            tuning: None,
        }
    }

    /// The library's default tuning (built-in values; TRT_* environment variables override them once, when the library is loaded).
    pub fn default_tuning() -> sys::trt_tuning {
        let mut t = sys::trt_tuning::default();
        unsafe { sys::trt_tuning_default(&mut t) };
        t
    }

    /// Renderer::render (renderer.rs:37-79), synchronous; wrap in `tokio::task::spawn_blocking` for a JoinHandle<Image>.
    pub fn render(&self, camera: &Camera, world: &mut World) -> Result<Image, Error> {
        let (width, height) = camera.get_image_size();
        let scene = world.get_bvh()?;
        let params = sys::trt_render_params {
            samples_per_pixel: self.samples_per_pixel as u32,
            max_bounces: self.max_bounces as u32,
            background: self.background_color.raw(),
            seed: self.seed,
            backend: self.backend,
            tuning: self.tuning.as_ref().map_or(ptr::null(), |t| t as *const sys::trt_tuning),
            ..Default::default()
        };
        let mut data = vec![0.0 as Float; width * height * 3];
        check(unsafe { sys::trt_render(scene, &camera.pod, &params, data.as_mut_ptr(), ptr::null_mut()) })?;
        Ok(Image { width, height, gamma: 2.2, data })
    }

    /// `render` that also returns the per-pixel second moments (`trt_render_moments`; streamed backend) and the variance of every pixel's
    /// estimate (`trt_variance`: 1 value per pixel, +inf at 1 spp): `(frame, moment2, variance)`.  The frame is `render`'s, bit for bit.
    pub fn render_moments(&self, camera: &Camera, world: &mut World) -> Result<(Image, Vec<Float>, Vec<Float>), Error> {
        let (width, height) = camera.get_image_size();
        let scene = world.get_bvh()?;
        let params = sys::trt_render_params {
            samples_per_pixel: self.samples_per_pixel as u32,
            max_bounces: self.max_bounces as u32,
            background: self.background_color.raw(),
            seed: self.seed,
            backend: self.backend,
            tuning: self.tuning.as_ref().map_or(ptr::null(), |t| t as *const sys::trt_tuning),
            ..Default::default()
        };
        let n = width * height;
        let mut data = vec![0.0 as Float; n * 3];
        let mut moment2 = vec![0.0 as Float; n * 3];
        let mut variance = vec![0.0 as Float; n];
        check(unsafe { sys::trt_render_moments(scene, &camera.pod, &params, data.as_mut_ptr(), moment2.as_mut_ptr(), ptr::null_mut()) })?;
        check(unsafe { sys::trt_variance(data.as_ptr(), moment2.as_ptr(), n as u32, self.samples_per_pixel as u32, variance.as_mut_ptr()) })?;
        Ok((Image { width, height, gamma: 2.2, data }, moment2, variance))
    }

    /// Samples `[sample_begin, sample_end)` of the listed pixels only (`trt_render_pixels`), added to the running sums in `frame` and
    /// `moment2`: every listed pixel gets the bytes `render_moments` would leave there for that range, every other pixel is untouched.
    /// `pixels`: indices `y * width + x`, each at most once.
    pub fn render_pixels(&self, camera: &Camera, world: &mut World, pixels: &[u32], sample_begin: u32, sample_end: u32,
                         frame: &mut Image, moment2: &mut [Float]) -> Result<(), Error> {
        let (width, height) = camera.get_image_size();
        if frame.data.len() != width * height * 3 || moment2.len() != width * height * 3 {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "frame and moment2 have the camera's size".to_string() });
        }
        let scene = world.get_bvh()?;
        let params = sys::trt_render_params {
            samples_per_pixel: self.samples_per_pixel as u32,
            max_bounces: self.max_bounces as u32,
            background: self.background_color.raw(),
            seed: self.seed,
            sample_begin,
            sample_end,
            accumulate: 1,
            ..Default::default()
        };
        check(unsafe {
            sys::trt_render_pixels(scene, &camera.pod, &params, pixels.as_ptr(), pixels.len() as u32, frame.data.as_mut_ptr(),
                                   moment2.as_mut_ptr(), ptr::null_mut())
        })
    }

    /// The candidates (`None` = every pixel) whose estimate after `samples_done` samples is still too noisy (`trt_select_pixels`), in order.
    pub fn select_pixels(&self, frame: &Image, moment2: &[Float], samples_done: u32, rel_tol: Float, abs_tol: Float,
                         candidates: Option<&[u32]>) -> Result<Vec<u32>, Error> {
        let npixels = (frame.width * frame.height) as u32;
        let n = candidates.map_or(npixels, |c| c.len() as u32);
        let mut out = vec![0u32; n as usize];
        let mut count = 0u32;
        check(unsafe {
            sys::trt_select_pixels(frame.data.as_ptr(), moment2.as_ptr(), npixels, self.samples_per_pixel as u32, samples_done,
                                   candidates.map_or(ptr::null(), |c| c.as_ptr()), n, rel_tol, abs_tol, out.as_mut_ptr(), &mut count)
        })?;
        out.truncate(count as usize);
        Ok(out)
    }

    /// All six feature buffers of the frame `render` would trace: same seed, same samples, same primary rays.
    pub fn render_aov(&self, camera: &Camera, world: &mut World) -> Result<FeatureBuffers, Error> {
        let (width, height) = camera.get_image_size();
        let scene = world.get_bvh()?;
        let params = sys::trt_render_params {
            samples_per_pixel: self.samples_per_pixel as u32,
            background: self.background_color.raw(),
            seed: self.seed,
            ..Default::default()
        };
        let n = width * height;
        let mut out = FeatureBuffers {
            width,
            height,
            albedo: vec![0.0; n * 3],
            normal: vec![0.0; n * 3],
            depth: vec![0.0; n],
            coverage: vec![0.0; n],
            geometry: vec![0; n],
            material: vec![0; n],
        };
        let buffers = sys::trt_aov_buffers {
            albedo: out.albedo.as_mut_ptr(),
            normal: out.normal.as_mut_ptr(),
            depth: out.depth.as_mut_ptr(),
            coverage: out.coverage.as_mut_ptr(),
            geometry: out.geometry.as_mut_ptr(),
            material: out.material.as_mut_ptr(),
        };
        check(unsafe { sys::trt_render_aov(scene, &camera.pod, &params, &buffers) })?;
        Ok(out)
    }

    /// The frame denoised by its own feature buffers (`trt_denoise`: the edge-avoiding a-trous filter of tinyrt.h guided by albedo,
    /// normal and depth, default parameters): `frame` as `render` returned it, `aov` as `render_aov` returned it for the same camera.
    pub fn denoise(frame: &Image, aov: &FeatureBuffers) -> Result<Image, Error> {
        let input = sys::trt_denoise_inputs {
            color: frame.data.as_ptr(),
            albedo: aov.albedo.as_ptr(),
            normal: aov.normal.as_ptr(),
            depth: aov.depth.as_ptr(),
        };
        let mut data = vec![0.0 as Float; aov.width * aov.height * 3];
        check(unsafe { sys::trt_denoise(&input, aov.width as u32, aov.height as u32, ptr::null(), data.as_mut_ptr()) })?;
        Ok(Image { width: aov.width, height: aov.height, gamma: frame.gamma, data })
    }

    /// `denoise` with the variance-guided colour stop (`trt_denoise_ex`, default sigma): `variance` as `render_moments` returned it.
    pub fn denoise_with_variance(frame: &Image, aov: &FeatureBuffers, variance: &[Float]) -> Result<Image, Error> {
        if variance.len() != aov.width * aov.height {
            return Err(Error { code: sys::TRT_ERR_INVALID_ARG, message: "one variance per pixel".to_string() });
        }
        let input = sys::trt_denoise_inputs {
            color: frame.data.as_ptr(),
            albedo: aov.albedo.as_ptr(),
            normal: aov.normal.as_ptr(),
            depth: aov.depth.as_ptr(),
        };
        let mut color = sys::trt_denoise_color::default();
        unsafe { sys::trt_denoise_color_default(&mut color) };
        color.variance = variance.as_ptr();
        let mut data = vec![0.0 as Float; aov.width * aov.height * 3];
        check(unsafe { sys::trt_denoise_ex(&input, &color, aov.width as u32, aov.height as u32, ptr::null(), data.as_mut_ptr()) })?;
        Ok(Image { width: aov.width, height: aov.height, gamma: frame.gamma, data })
    }

    /// The same call over `ndev` GPUs of the node (0 = every visible device): the image's 16-row bands are dealt round-robin
    /// over the devices and every finished band is copied to its place in the frame (trt_render_multi).
    pub fn render_multi(&self, camera: &Camera, world: &mut World, ndev: u32) -> Result<Image, Error> {
        let (width, height) = camera.get_image_size();
        let scene = world.get_bvh()?;
        let params = sys::trt_render_params {
            samples_per_pixel: self.samples_per_pixel as u32,
            max_bounces: self.max_bounces as u32,
            background: self.background_color.raw(),
            seed: self.seed,
            backend: self.backend,
            tuning: self.tuning.as_ref().map_or(ptr::null(), |t| t as *const sys::trt_tuning),
            ..Default::default()
        };
        let mut data = vec![0.0 as Float; width * height * 3];
        check(unsafe { sys::trt_render_multi(scene, &camera.pod, &params, ptr::null(), ndev, data.as_mut_ptr(), ptr::null_mut()) })?;
        Ok(Image { width, height, gamma: 2.2, data })
    }
}
