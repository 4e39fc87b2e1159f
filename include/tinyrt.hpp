// tinyrt.hpp — C++17 host-side mirror of the reference crate's World / Camera / Renderer surface,
// header-only, over the C ABI in tinyrt.h.
//
// The reference is compiled code (Rust); no Rust toolchain exists in the build image, so the host
// side above the C ABI is C++ and keeps the crate's names, argument order and meaning (paths
// relative to raytracer/src):
//
//   World::add_material / add_geometry / get_material / get_bvh     hittable/world.rs:16-45
//   Sphere(center, radius, material), Quad(corner, u, v, material)  hittable/sphere.rs:16-26, quad.rs:20-29
//   Lambertian / Metal / Dielectric / Light                          material/*.rs
//   Camera(focus_distance, defocus_angle, position, look_at, up, vertical_fov, width, height)  camera.rs:17-26
//   Renderer(samples_per_pixel, num_sampler_threads, max_bounces, progressbar, background)     renderer/renderer.rs:21-35
//   Renderer::render(camera, world) -> Image                         renderer/renderer.rs:37-79
//   Image::get_pixel / save                                          utils/image.rs:46-48,66-69
//
// Error behaviour: where the reference panics (duplicate material name world.rs:29-31, failed
// joins renderer.rs:75-77) this throws tinyrt::Error carrying the C ABI's status and message.
// A Rust `-sys` binding of the same ABI is sketched in INTEGRATION.md.
#pragma once

#include <cstdint>
#include <cstdio>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "tinyrt.h"

namespace tinyrt {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};
inline void check(int rc) {
    if (rc != TRT_OK) throw Error(rc, std::string("tinyrt error ") + std::to_string(rc) + ": " + trt_last_error());
}

struct Vec3 : trt_vec3 {
    Vec3() : trt_vec3{0.0f, 0.0f, 0.0f} {}
    Vec3(float x_, float y_, float z_) : trt_vec3{x_, y_, z_} {}
    static Vec3 new_diagonal(float v) { return Vec3(v, v, v); }        // math/vec3.rs:23-25
    static Vec3 zero() { return Vec3(); }                              // math/vec3.rs:27-29
};

// ---- materials: values handed to World::add_material (material/*.rs) ----
struct Material { trt_material pod; };
inline Material Lambertian(Vec3 albedo) { return Material{{TRT_LAMBERTIAN, albedo, 0.0f}}; }
inline Material Metal(Vec3 albedo, float fuzz) { return Material{{TRT_METAL, albedo, fuzz}}; }
inline Material Dielectric(Vec3 albedo, float refraction_index) { return Material{{TRT_DIELECTRIC, albedo, refraction_index}}; }
inline Material Light(Vec3 color) { return Material{{TRT_LIGHT, color, 0.0f}}; }
using MaterialHandle = uint32_t;     // stands in for Arc<Box<dyn Material>>

// ---- geometry values handed to World::add_geometry ----
struct Sphere { Vec3 center; float radius; MaterialHandle material; };
struct Quad { Vec3 corner, u, v; MaterialHandle material; };

class World {
public:
    World() { check(trt_world_create(&w_)); }
    ~World() { if (scene_) trt_scene_destroy(scene_); trt_world_destroy(w_); }
    World(const World&) = delete;
    World& operator=(const World&) = delete;

    void add_material(const std::string& name, const Material& m) { check(trt_world_add_material(w_, name.c_str(), &m.pod)); }
    std::optional<MaterialHandle> get_material(const std::string& name) const {
        uint32_t idx = 0;
        int rc = trt_world_get_material(w_, name.c_str(), &idx);
        if (rc == TRT_ERR_NOT_FOUND) return std::nullopt;              // world.rs:35-41 returns Option
        check(rc);
        return idx;
    }
    void add_geometry(const Sphere& s) { invalidate(); check(trt_world_add_sphere(w_, s.center, s.radius, s.material)); }
    // n spheres in array order: the loop of add_geometry(Sphere) in one call (center_radius: 4n floats x, y, z, r)
    void add_spheres(uint32_t n, const float* center_radius, const uint32_t* material) { invalidate(); check(trt_world_add_spheres(w_, n, center_radius, material)); }
    void add_geometry(const Quad& q) { invalidate(); check(trt_world_add_quad(w_, q.corner, q.u, q.v, q.material)); }
    // new_box(a, b, material) of the reference binary (src/main.rs:89-125): six quads, same push order
    void add_box(Vec3 a, Vec3 b, MaterialHandle m) {
        Vec3 mn(a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, a.z < b.z ? a.z : b.z);
        Vec3 mx(a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y, a.z > b.z ? a.z : b.z);
        Vec3 dx(mx.x - mn.x, 0, 0), dy(0, mx.y - mn.y, 0), dz(0, 0, mx.z - mn.z);
        auto neg = [](Vec3 v) { return Vec3(-v.x, -v.y, -v.z); };
        add_geometry(Quad{Vec3(mn.x, mn.y, mx.z), dx, dy, m});
        add_geometry(Quad{Vec3(mx.x, mn.y, mx.z), neg(dz), dy, m});
        add_geometry(Quad{Vec3(mx.x, mn.y, mn.z), neg(dx), dy, m});
        add_geometry(Quad{Vec3(mn.x, mn.y, mn.z), dz, dy, m});
        add_geometry(Quad{Vec3(mn.x, mx.y, mx.z), dx, neg(dz), m});
        add_geometry(Quad{Vec3(mn.x, mn.y, mn.z), dx, dz, m});
    }
    // World::get_bvh (world.rs:43-45): the reference-order BVH, packed for the GPU; cached until the world changes
    trt_scene* get_bvh() {
        if (!scene_) check(trt_scene_create_ex(w_, has_options_ ? &options_ : nullptr, &scene_));
        return scene_;
    }
    // How the scene is compiled (trt_scene_options: placement only, every value renders the same frames).  Starts from the library
    // defaults; takes effect at the next get_bvh().
    trt_scene_options& scene_options() {
        if (!has_options_) { trt_scene_options_default(&options_); has_options_ = true; }
        invalidate();
        return options_;
    }
    // The light that arrives along caller-supplied rays (trt_radiance): each ray, used as given, is path traced with p.samples_per_ray
    // samples and folded with the imager's 1 / K rule.  `radiance` and `moment2` (nullptr: not wanted) become 3 floats per ray, or
    // continue the sums they hold when p.accumulate is set.  Start `p` from trt_radiance_params_default.
    void radiance(const std::vector<trt_ray>& rays, const trt_radiance_params& p, std::vector<float>& radiance,
                  std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        radiance.resize(rays.size() * 3);
        if (moment2) moment2->resize(rays.size() * 3);
        check(trt_radiance(get_bvh(), rays.data(), (uint32_t)rays.size(), &p, radiance.data(), moment2 ? moment2->data() : nullptr, stats));
    }
    // The light gathered at caller-supplied surfels (trt_gather): item = (origin = point, direction = axis), used as given.  For each of
    // p.path.samples_per_ray samples the device draws a first ray about the axis by p.lobe - cosine: what a white diffuse surface there
    // reflects; cone: axis + p.spread * (a point in the unit sphere) - and traces and folds it as radiance() does.  Start `p` from
    // trt_gather_params_default.
    void gather(const std::vector<trt_ray>& items, const trt_gather_params& p, std::vector<float>& radiance,
                std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        radiance.resize(items.size() * 3);
        if (moment2) moment2->resize(items.size() * 3);
        check(trt_gather(get_bvh(), items.data(), (uint32_t)items.size(), &p, radiance.data(), moment2 ? moment2->data() : nullptr, stats));
    }
    // How open the lobe about caller-supplied surfels is (trt_ambient): for each of p.gather.path.samples_per_ray samples the device draws
    // the first ray gather() would draw and asks whether anything lies in [0.001, p.max_distance) along it.  `visibility` becomes one
    // float per item - the unoccluded share; with the cosine lobe 1 - visibility is ambient occlusion - and `bent` (nullptr: not wanted)
    // three: the sum of the unoccluded unit directions / K, the bent normal, not renormalised.  Both continue the sums they hold when
    // p.gather.path.accumulate is set.  Start `p` from trt_ambient_params_default.
    void ambient(const std::vector<trt_ray>& items, const trt_ambient_params& p, std::vector<float>& visibility,
                 std::vector<float>* bent = nullptr, trt_stats* stats = nullptr) {
        visibility.resize(items.size());
        if (bent) bent->resize(items.size() * 3);
        check(trt_ambient(get_bvh(), items.data(), (uint32_t)items.size(), &p, visibility.data(), bent ? bent->data() : nullptr, stats));
    }
    // The scene's own lights (trt_scene_emitters): the geometries whose material is a Light, in insertion order - a table for direct().
    std::vector<trt_emitter> emitters() {
        uint32_t count = 0;
        check(trt_scene_emitters(get_bvh(), nullptr, 0, &count));
        std::vector<trt_emitter> table(count);
        if (count) check(trt_scene_emitters(get_bvh(), table.data(), count, &count));
        return table;
    }
    // The light that reaches caller-supplied surfels straight from the emitters of a table (trt_direct): emitters(), a part of it, or
    // lights that are no geometry of the scene (trt_emitter_init_quad, trt_emitter_init_sphere).  Each of p.path.samples_per_ray samples
    // picks an emitter and a point on it and asks whether anything lies in [0.001, distance * p.shadow_end) along the normalised ray
    // towards it.  `radiance` becomes three floats per item - with a unit axis what a white diffuse surface reflects from those emitters
    // alone, gather()'s convention - and `moment2` (nullptr: not wanted) the second moments.  Both continue the sums they hold when
    // p.path.accumulate is set.  Start `p` from trt_direct_params_default.
    void direct(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const trt_direct_params& p, std::vector<float>& radiance,
                std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        emitter_query(items, table, nullptr, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_direct(q.scene, q.items, q.n, q.table, q.n_emitters, &p, q.radiance, q.moment2, stats);
        });
    }
    // direct() with multiple importance sampling (trt_direct_mis): every sample also sends one cosine-lobe ray from the surfel, and a light
    // of the scene counts both ways, the shadow sample scaled by 1 / (1 + q(p_bsdf / p_light)) and the lobe ray's hit on a light by the
    // complement, q(x) = x (TRT_MIS_BALANCE) or x * x (TRT_MIS_POWER): the same expectation without the 1/d2 tail of surfels beside a
    // lamp, for one closest-hit walk more per sample.  `table` must hold exactly the scene's own lights (emitters()), each once, plus any
    // virtual ones; anything else is an error.  Start `p` from trt_direct_mis_params_default.
    void direct_mis(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const trt_direct_mis_params& p,
                    std::vector<float>& radiance, std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        emitter_query(items, table, nullptr, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_direct_mis(q.scene, q.items, q.n, q.table, q.n_emitters, &p, q.radiance, q.moment2, stats);
        });
    }
    // The alias table over `table` (trt_emitter_pick_build) through which direct_pick() and direct_mis_pick() choose their emitter: by
    // power (weights == nullptr; the table direct_mis_pick() needs) or by `weights`, table.size() finite non-negative values.  `total`
    // receives the weights' sum.  Host only.
    static std::vector<trt_emitter_pick> pick_table(const std::vector<trt_emitter>& table, const float* weights = nullptr, float* total = nullptr) {
        std::vector<trt_emitter_pick> pick(table.size());
        check(trt_emitter_pick_build(table.data(), (uint32_t)table.size(), weights, pick.data(), total));
        return pick;
    }
    // direct() with the emitter of a sample chosen through `pick` (trt_direct_pick) - by power, not uniformly: one draw more per sample,
    // far less noise where the emitters' powers differ much.
    void direct_pick(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const std::vector<trt_emitter_pick>& pick,
                     const trt_direct_params& p, std::vector<float>& radiance, std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        emitter_query(items, table, &pick, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_direct_pick(q.scene, q.items, q.n, q.table, q.pick, q.n_emitters, &p, q.radiance, q.moment2, stats);
        });
    }
    // direct_mis() with the emitter chosen through `pick` (trt_direct_mis_pick): `pick` must be pick_table(table) - the power table -
    // and `total_power` the total it reported; the lobe ray's hit on a light is weighted by the same probability.
    void direct_mis_pick(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const std::vector<trt_emitter_pick>& pick,
                         const trt_direct_mis_params& p, float total_power, std::vector<float>& radiance, std::vector<float>* moment2 = nullptr,
                         trt_stats* stats = nullptr) {
        emitter_query(items, table, &pick, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_direct_mis_pick(q.scene, q.items, q.n, q.table, q.pick, q.n_emitters, &p, total_power, q.radiance, q.moment2, stats);
        });
    }
    // What radiance() / gather() estimate, with the lights aimed at (trt_nee): the path of every sample is theirs bit for bit (p.gather:
    // path, source - TRT_PASSES_RAYS, _COSINE, _CONE - and spread), at every Lambertian hit that leaves bounce budget one shadow ray goes
    // to `table` as in direct(), and a light the path then reaches by a diffuse scatter counts as black.  `table` should be emitters():
    // a light left out is still hidden.  With p.source_is_diffuse the first hit counts as diffusely reached too: for a cosine source the
    // result is the surfel's indirect light, and direct() + nee() is a full bake.  Buffers as in direct().  Start `p` from
    // trt_nee_params_default.
    void nee(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const trt_nee_params& p, std::vector<float>& radiance,
             std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        emitter_query(items, table, nullptr, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_nee(q.scene, q.items, q.n, q.table, q.n_emitters, &p, q.radiance, q.moment2, stats);
        });
    }
    // nee() with multiple importance sampling (trt_nee_mis): the same paths and shadow rays, but a light reached after a diffuse scatter
    // (from the second hit on) counts both ways, the shadow sample scaled by 1 / (1 + q(p_bsdf / p_light)) and the hit by the complement,
    // q(x) = x (TRT_MIS_BALANCE) or x * x (TRT_MIS_POWER): the same expectation without the 1/d2 tail of shadow samples beside a lamp.
    // `table` must hold exactly the scene's own lights (emitters()), each once, plus any virtual ones; anything else is an error.  Start
    // `p` from trt_nee_mis_params_default.
    void nee_mis(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const trt_nee_mis_params& p, std::vector<float>& radiance,
                 std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        emitter_query(items, table, nullptr, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_nee_mis(q.scene, q.items, q.n, q.table, q.n_emitters, &p, q.radiance, q.moment2, stats);
        });
    }
    // nee() with the emitter of every vertex's shadow ray chosen through `pick` (trt_nee_pick; pick_table() above) - by power, not
    // uniformly: one draw more per vertex, far less noise where the emitters' powers differ much.
    void nee_pick(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const std::vector<trt_emitter_pick>& pick,
                  const trt_nee_params& p, std::vector<float>& radiance, std::vector<float>* moment2 = nullptr, trt_stats* stats = nullptr) {
        emitter_query(items, table, &pick, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_nee_pick(q.scene, q.items, q.n, q.table, q.pick, q.n_emitters, &p, q.radiance, q.moment2, stats);
        });
    }
    // nee_mis() with the emitter chosen through `pick` (trt_nee_mis_pick): `pick` must be pick_table(table) - the power table - and
    // `total_power` the total it reported; a light reached after a diffuse scatter is weighted by the same probability.
    void nee_mis_pick(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const std::vector<trt_emitter_pick>& pick,
                      const trt_nee_mis_params& p, float total_power, std::vector<float>& radiance, std::vector<float>* moment2 = nullptr,
                      trt_stats* stats = nullptr) {
        emitter_query(items, table, &pick, radiance, moment2, [&](const EmitterQuery& q) {
            return trt_nee_mis_pick(q.scene, q.items, q.n, q.table, q.pick, q.n_emitters, &p, total_power, q.radiance, q.moment2, stats);
        });
    }
    // The radiance arriving at caller-supplied points as a function of direction (trt_probe): for each of p.path.samples_per_ray samples
    // the device draws a first ray uniformly over the sphere, or over the hemisphere about the item's axis (p.domain), traces it as
    // gather() does and adds colour * Y_k(direction) / K to coefficient k of the item.  `sh` becomes p.bands^2 x 3 floats per item - real
    // spherical harmonics, coefficient l (l + 1) + m, then channel - and continues the sums it holds when p.path.accumulate is set.
    // Start `p` from trt_probe_params_default.
    void probe(const std::vector<trt_ray>& items, const trt_probe_params& p, std::vector<float>& sh, trt_stats* stats = nullptr) {
        sh.resize(items.size() * (p.bands <= 3u ? (size_t)p.bands * p.bands : 0u) * 3);   // (bands out of range: trt_probe says so)
        check(trt_probe(get_bvh(), items.data(), (uint32_t)items.size(), &p, sh.data(), stats));
    }
    // probe() with a launch that fills the device whatever K is (trt_probe_parallel): the same arguments, the same `sh` and the same
    // samples and rays in `stats`, bit for bit.  The paths run a sample to a GPU lane into a record buffer of the call's own and
    // project_samples' kernels fold the records, in chunks of min(n, record_bytes / (24 K)) items; record_bytes = 0 takes the
    // library's default (96 MiB, or one item's 24 K bytes where that is more), a buffer that holds no item is an error.
    void probe_parallel(const std::vector<trt_ray>& items, const trt_probe_params& p, std::vector<float>& sh, trt_stats* stats = nullptr,
                        uint64_t record_bytes = 0) {
        if (items.size() > 0xFFFFFFFFull) throw Error(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 items in one call");
        sh.resize(items.size() * (p.bands <= 3u ? (size_t)p.bands * p.bands : 0u) * 3);   // (bands out of range: trt_probe_parallel says so)
        check(trt_probe_parallel(get_bvh(), items.data(), (uint32_t)items.size(), &p, sh.data(), stats, record_bytes));
    }
    // Every sample's colour and, with `directions`, its first ray's stored direction (trt_samples): a sample to a GPU lane where radiance(),
    // gather() and probe() give the samples of an item one lane.  p.source says where the first ray comes from - TRT_SAMPLE_RAYS: the
    // items are rays; COSINE, CONE: gather()'s draw about surfels; SPHERE, HEMISPHERE: probe()'s - and p.path the samples, the range
    // (only samples [sample_begin, sample_end) are written) and the RNG numbering; accumulate must be 0.  Both vectors become
    // items.size() x K x 3 floats, record i * K + s; what they held outside the range stays.  Start `p` from trt_samples_params_default.
    void samples(const std::vector<trt_ray>& items, const trt_samples_params& p, std::vector<float>& colors, std::vector<float>* directions = nullptr,
                 trt_stats* stats = nullptr) {
        if (items.size() > 0xFFFFFFFFull) throw Error(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 items in one call");
        const size_t floats = items.size() * (size_t)p.path.samples_per_ray * 3;
        colors.resize(floats);
        if (directions) directions->resize(floats);
        check(trt_samples(get_bvh(), items.data(), (uint32_t)items.size(), &p, colors.data(), directions ? directions->data() : nullptr, stats));
    }
    // Every sample's colour of the next-event queries (trt_nee_samples): samples() for nee(), nee_mis(), nee_pick() and nee_mis_pick().
    // p.weighted and `pick` (nullptr: the uniform choice; else one record per emitter) select the sibling whose sample is written, bit
    // for bit; p.query.nee is nee()'s parameter struct (accumulate must be 0), p.total_power nee_mis_pick()'s argument.  Both vectors
    // become items.size() x K x 3 floats, record i * K + s; what they held outside the range stays.  fold_samples() turns the colours
    // into the sibling's sums.  Start `p` from trt_nee_samples_params_default.
    void nee_samples(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& emitters, const std::vector<trt_emitter_pick>* pick,
                     const trt_nee_samples_params& p, std::vector<float>& colors, std::vector<float>* directions = nullptr, trt_stats* stats = nullptr) {
        if (items.size() > 0xFFFFFFFFull) throw Error(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 items in one call");
        if (pick && pick->size() != emitters.size()) throw Error(TRT_ERR_INVALID_ARG, "pick holds one record per emitter");
        const size_t floats = items.size() * (size_t)p.query.nee.gather.path.samples_per_ray * 3;
        colors.resize(floats);
        if (directions) directions->resize(floats);
        check(trt_nee_samples(get_bvh(), items.data(), (uint32_t)items.size(), emitters.data(), pick ? pick->data() : nullptr, (uint32_t)emitters.size(), &p,
                              colors.data(), directions ? directions->data() : nullptr, stats));
    }
    // The light radiance() or gather() folds into one colour, split by how each path ended and after how many scatters (trt_passes):
    // p.gather.lobe is the source of the first ray (TRT_PASSES_RAYS: the items are rays; TRT_PASSES_COSINE, TRT_PASSES_CONE: surfels,
    // gather()'s draws).  `sums` becomes 2 x p.depth_bins x 3 floats per item - the paths that ended at a light by depth bin, then those
    // that ended in the background, then channel - and `spent`, if wanted, the share of each item's samples that ended by their bounce
    // budget; both continue the sums they hold when p.gather.path.accumulate is set.  Start `p` from trt_passes_params_default.
    void passes(const std::vector<trt_ray>& items, const trt_passes_params& p, std::vector<float>& sums, std::vector<float>* spent = nullptr,
                trt_stats* stats = nullptr) {
        sums.resize(items.size() * (p.depth_bins <= 4u ? 2u * (size_t)p.depth_bins : 0u) * 3);   // (bins out of range: trt_passes says so)
        if (spent) spent->resize(items.size());
        check(trt_passes(get_bvh(), items.data(), (uint32_t)items.size(), &p, sums.data(), spent ? spent->data() : nullptr, stats));
    }
    int num_geometries() const { return trt_world_num_geometries(w_); }
    const trt_world* handle() const { return w_; }
    // Frees the device scratch (render workspaces, frame buffers) the compiled scene caches between renders (trt_scene_trim).
    void trim() { if (scene_) check(trt_scene_trim(scene_)); }

private:
    void invalidate() { if (scene_) { trt_scene_destroy(scene_); scene_ = nullptr; } }
    // What the eight direct*() / nee*() queries share: the pick table's size, the sizes of the sums, the call and its error.  `call` is the
    // C entry point with the query's own parameters bound, handed the buffers as EmitterQuery holds them.
    struct EmitterQuery {
        trt_scene* scene;
        const trt_ray* items;
        uint32_t n;
        const trt_emitter* table;
        const trt_emitter_pick* pick;    // nullptr: no pick table
        uint32_t n_emitters;
        float *radiance, *moment2;
    };
    template <class Call>
    void emitter_query(const std::vector<trt_ray>& items, const std::vector<trt_emitter>& table, const std::vector<trt_emitter_pick>* pick,
                       std::vector<float>& radiance, std::vector<float>* moment2, Call&& call) {
        if (pick && pick->size() != table.size()) throw Error(TRT_ERR_INVALID_ARG, "the pick table needs one record per emitter");
        radiance.resize(items.size() * 3);
        if (moment2) moment2->resize(items.size() * 3);
        check(call(EmitterQuery{get_bvh(), items.data(), (uint32_t)items.size(), table.data(), pick ? pick->data() : nullptr, (uint32_t)table.size(),
                                radiance.data(), moment2 ? moment2->data() : nullptr}));
    }
    trt_world* w_ = nullptr;
    trt_scene* scene_ = nullptr;
    trt_scene_options options_{};
    bool has_options_ = false;
};

// The fold of World::samples' colours (trt_fold_samples; runs on the device, no scene needed): per item over samples [p.sample_begin,
// p.sample_end) of K = p.samples_per_ray in order, radiance += c / K and moment2 += c * c / K in f32 - for the sources RAYS, COSINE and CONE
// the bytes World::radiance / World::gather return.  `colors` holds n x K x 3 floats; `radiance` (and `moment2`, if given) become n x 3
// and continue the sums they hold when p.accumulate is set.  Of `p` nothing else is read.
inline void fold_samples(const std::vector<float>& colors, const trt_radiance_params& p, std::vector<float>& radiance, std::vector<float>* moment2 = nullptr) {
    const size_t per_item = (size_t)p.samples_per_ray * 3;
    if (per_item == 0 || colors.size() % per_item != 0) throw Error(TRT_ERR_INVALID_ARG, "colors holds n x samples_per_ray x 3 floats");
    const size_t n = colors.size() / per_item;
    if (n > 0xFFFFFFFFull) throw Error(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 items in one call");
    radiance.resize(n * 3);
    if (moment2) moment2->resize(n * 3);
    check(trt_fold_samples(colors.data(), (uint32_t)n, &p, radiance.data(), moment2 ? moment2->data() : nullptr));
}

// The probe fold of World::samples' colours and directions for the sources SPHERE and HEMISPHERE (trt_project_samples; runs on the
// device, no scene needed): per item over samples [p.path.sample_begin, p.path.sample_end) of K = p.path.samples_per_ray in order,
// sh[k] += c * (Y_k(d) / K) in f32 for the p.bands^2 real spherical harmonics.  A sample whose direction has a NaN adds nothing; with
// `items` (the probes, one per item) neither does any sample of an item whose point has one - then `sh` is World::probe's, byte for
// byte.  `sh` becomes n x p.bands^2 x 3 floats and continues the sums it holds when p.path.accumulate is set.  Of `p` only K, the
// range, accumulate and bands are read.
inline void project_samples(const std::vector<float>& colors, const std::vector<float>& directions, const trt_probe_params& p, std::vector<float>& sh,
                            const std::vector<trt_ray>* items = nullptr) {
    const size_t per_item = (size_t)p.path.samples_per_ray * 3;
    if (per_item == 0 || colors.size() % per_item != 0 || directions.size() != colors.size())
        throw Error(TRT_ERR_INVALID_ARG, "colors and directions hold n x samples_per_ray x 3 floats each");
    const size_t n = colors.size() / per_item;
    if (n > 0xFFFFFFFFull) throw Error(TRT_ERR_INVALID_ARG, "more than 2^32 - 1 items in one call");
    if (items && items->size() != n) throw Error(TRT_ERR_INVALID_ARG, "items holds one probe per item");
    sh.resize(n * (p.bands <= 3u ? (size_t)p.bands * p.bands : 0u) * 3);                  // (bands out of range: trt_project_samples says so)
    check(trt_project_samples(colors.data(), directions.data(), items ? items->data() : nullptr, (uint32_t)n, &p, sh.data()));
}


// A scene compiled on the current device (trt_scene_create_on_device): the same bytes as World::get_bvh(), already resident there.
// Owns its handle; render it through the C ABI (scene()).
class DeviceScene {
public:
    explicit DeviceScene(const World& w, const trt_scene_options* options = nullptr) { check(trt_scene_create_on_device(w.handle(), options, &s_)); }
    ~DeviceScene() { if (s_) trt_scene_destroy(s_); }
    DeviceScene(const DeviceScene&) = delete;
    DeviceScene& operator=(const DeviceScene&) = delete;
    trt_scene* scene() const { return s_; }

private:
    trt_scene* s_ = nullptr;
};

class Camera {
public:
    Camera(float focus_distance, float defocus_angle, Vec3 position, Vec3 look_at, Vec3 up, float vertical_fov, uint32_t width,
           uint32_t height) {
        check(trt_camera_init(&pod, focus_distance, defocus_angle, position, look_at, up, vertical_fov, width, height));
    }
    std::pair<uint32_t, uint32_t> get_image_size() const { return {pod.width, pod.height}; }   // camera.rs:68-70
    // The rays Renderer::render traces for sample `sample` of every pixel under `seed` (trt_primary_rays): width * height rays, row-major.
    std::vector<trt_ray> primary_rays(uint32_t sample, uint32_t samples_per_pixel, uint32_t seed = 1) const {
        trt_render_params p{};
        p.samples_per_pixel = samples_per_pixel;
        p.seed = seed;
        std::vector<trt_ray> rays((size_t)pod.width * pod.height);
        check(trt_primary_rays(&pod, &p, sample, rays.data()));
        return rays;
    }
    trt_camera pod;
};

// The first-hit feature buffers of a frame (trt_render_aov): sums over the samples in the imager's order, indices of sample 0
// (0xFFFFFFFF on a miss).  Row-major, width * height pixels each.
struct FeatureBuffers {
    uint32_t width = 0, height = 0;
    std::vector<float> albedo, normal;          // 3 per pixel; the normal is not renormalised
    std::vector<float> depth, coverage;
    std::vector<uint32_t> geometry, material;
};

// Minimal PNG writer (8-bit RGB, zlib "stored" blocks: valid for every decoder, no compression) so that
// Image::save("x.png") yields what the reference's `image` crate call yields: a PNG of the quantised frame.
namespace detail {
inline uint32_t crc32(const uint8_t* p, size_t n, uint32_t crc) {
    crc = ~crc;
    for (size_t i = 0; i < n; i++) {
        crc ^= p[i];
        for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}
inline void put_be32(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x);
}
inline void png_chunk(std::vector<uint8_t>& out, const char* type, const std::vector<uint8_t>& data) {
    put_be32(out, (uint32_t)data.size());
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), data.begin(), data.end());
    put_be32(out, crc32(out.data() + at, out.size() - at, 0u));
}
inline std::vector<uint8_t> encode_png_rgb8(const uint8_t* rgb, uint32_t w, uint32_t h) {
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, w); put_be32(ihdr, h);
    ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});                       // 8 bits, colour type 2 (RGB), deflate, no filter, no interlace
    png_chunk(out, "IHDR", ihdr);
    std::vector<uint8_t> raw;                                        // scanlines, each with filter byte 0
    raw.reserve((size_t)h * ((size_t)w * 3 + 1));
    for (uint32_t y = 0; y < h; y++) {
        raw.push_back(0);
        raw.insert(raw.end(), rgb + (size_t)y * w * 3, rgb + (size_t)(y + 1) * w * 3);
    }
    std::vector<uint8_t> z = {0x78, 0x01};                           // zlib header, then stored deflate blocks of <= 65535 bytes
    uint32_t a = 1, b = 0;                                           // Adler-32 of the raw data
    for (uint8_t c : raw) { a = (a + c) % 65521u; b = (b + a) % 65521u; }
    size_t pos = 0;
    do {
        const size_t n = raw.size() - pos < 65535 ? raw.size() - pos : 65535;
        z.push_back(pos + n == raw.size() ? 1 : 0);
        z.push_back((uint8_t)(n & 0xFF)); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 0xFF)); z.push_back((uint8_t)((~n >> 8) & 0xFF));
        z.insert(z.end(), raw.begin() + (long)pos, raw.begin() + (long)(pos + n));
        pos += n;
    } while (pos < raw.size());
    put_be32(z, b << 16 | a);
    png_chunk(out, "IDAT", z);
    png_chunk(out, "IEND", {});
    return out;
}
}  // namespace detail

// utils/image.rs: Image with gamma 2.2 as the Imager builds it (imager.rs:37-41); holds the linear sums
class Image {
public:
    Image(uint32_t w, uint32_t h, float gamma = 2.2f) : width_(w), height_(h), gamma_(gamma), data_((size_t)w * h * 3, 0.0f) {}
    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    float* linear() { return data_.data(); }
    const float* linear() const { return data_.data(); }
    std::vector<uint8_t> to_rgb8() const {
        std::vector<uint8_t> rgb(data_.size());
        check(trt_tonemap_u8(data_.data(), width_ * height_, gamma_, rgb.data()));
        return rgb;
    }
    // Image::save (image.rs:66-69; the reference writes PNG through the `image` crate): PNG for "*.png", binary PPM otherwise
    void save(const std::string& filename) const {
        auto rgb = to_rgb8();
        FILE* f = std::fopen(filename.c_str(), "wb");
        if (!f) throw Error(TRT_ERR_INVALID_ARG, "cannot open " + filename);
        const bool png = filename.size() >= 4 && filename.compare(filename.size() - 4, 4, ".png") == 0;
        if (png) {
            auto bytes = detail::encode_png_rgb8(rgb.data(), width_, height_);
            std::fwrite(bytes.data(), 1, bytes.size(), f);
        } else {
            std::fprintf(f, "P6\n%u %u\n255\n", width_, height_);
            std::fwrite(rgb.data(), 1, rgb.size(), f);
        }
        std::fclose(f);
    }

private:
    uint32_t width_, height_;
    float gamma_;
    std::vector<float> data_;
};

class Renderer {
public:
    Renderer(uint32_t samples_per_pixel, uint32_t num_sampler_threads, uint32_t max_bounces, bool progressbar,
             std::optional<Vec3> background_color, uint32_t seed = 1, uint32_t backend = TRT_BACKEND_AUTO) {
        (void)num_sampler_threads;     // the GPU needs no sampler-task count; kept for signature parity
        (void)progressbar;
        params_ = trt_render_params{};
        params_.samples_per_pixel = samples_per_pixel;
        params_.max_bounces = max_bounces;
        params_.background = background_color.value_or(Vec3::zero());  // renderer.rs:33
        params_.seed = seed;
        params_.backend = backend;
    }
    // Renderer::render (renderer.rs:37-79); synchronous (the reference returns a JoinHandle<Image> to await)
    Image render(const Camera& camera, World& world, trt_stats* stats = nullptr) const {
        Image img(camera.pod.width, camera.pod.height);
        check(trt_render(world.get_bvh(), &camera.pod, &params_, img.linear(), stats));
        return img;
    }
    // render() that also fills the per-pixel second moments (trt_render_moments; streamed backend): `moment2` gets width * height * 3
    // floats.  The frame is render()'s, bit for bit.
    Image render_moments(const Camera& camera, World& world, std::vector<float>& moment2, trt_stats* stats = nullptr) const {
        Image img(camera.pod.width, camera.pod.height);
        moment2.assign((size_t)camera.pod.width * camera.pod.height * 3, 0.0f);
        check(trt_render_moments(world.get_bvh(), &camera.pod, &params_, img.linear(), moment2.data(), stats));
        return img;
    }
    // Variance of every pixel's estimate (trt_variance: 1 float per pixel, +inf at 1 spp) from a frame and its second moments.
    std::vector<float> variance(const Image& frame, const std::vector<float>& moment2) const {
        std::vector<float> v((size_t)frame.width() * frame.height(), 0.0f);
        check(trt_variance(frame.linear(), moment2.data(), frame.width() * frame.height(), params_.samples_per_pixel, v.data()));
        return v;
    }
    // Samples [sample_begin, sample_end) of the listed pixels only (trt_render_pixels), added to the running sums in `frame` and `moment2`
    // (accumulate): every listed pixel gets the bytes render_moments would leave there for that range, every other pixel is untouched.
    // `pixels`: indices y * width + x, each at most once.
    void render_pixels(const Camera& camera, World& world, const std::vector<uint32_t>& pixels, uint32_t sample_begin, uint32_t sample_end,
                       Image& frame, std::vector<float>& moment2, trt_stats* stats = nullptr) const {
        if (moment2.size() != (size_t)camera.pod.width * camera.pod.height * 3) throw Error(TRT_ERR_INVALID_ARG, "moment2 has the frame's size");
        trt_render_params p = params_;
        p.sample_begin = sample_begin;
        p.sample_end = sample_end;
        p.accumulate = 1;
        p.collect_stats = 0;
        check(trt_render_pixels(world.get_bvh(), &camera.pod, &p, pixels.data(), (uint32_t)pixels.size(), frame.linear(), moment2.data(), stats));
    }
    // The candidates (empty = every pixel) whose estimate after `samples_done` samples is still too noisy (trt_select_pixels), in order.
    std::vector<uint32_t> select_pixels(const Image& frame, const std::vector<float>& moment2, uint32_t samples_done, float rel_tol,
                                        float abs_tol, const std::vector<uint32_t>& candidates = {}) const {
        const uint32_t npixels = frame.width() * frame.height();
        const uint32_t n = candidates.empty() ? npixels : (uint32_t)candidates.size();
        std::vector<uint32_t> out(n);
        uint32_t count = 0;
        check(trt_select_pixels(frame.linear(), moment2.data(), npixels, params_.samples_per_pixel, samples_done,
                                candidates.empty() ? nullptr : candidates.data(), n, rel_tol, abs_tol, out.data(), &count));
        out.resize(count);
        return out;
    }
    // All six feature buffers of the frame render() would trace: same seed, same samples, same primary rays.
    FeatureBuffers render_aov(const Camera& camera, World& world) const {
        FeatureBuffers out;
        out.width = camera.pod.width;
        out.height = camera.pod.height;
        const size_t n = (size_t)out.width * out.height;
        out.albedo.assign(n * 3, 0.0f); out.normal.assign(n * 3, 0.0f);
        out.depth.assign(n, 0.0f); out.coverage.assign(n, 0.0f);
        out.geometry.assign(n, 0u); out.material.assign(n, 0u);
        const trt_aov_buffers b{out.albedo.data(), out.normal.data(), out.depth.data(), out.coverage.data(), out.geometry.data(),
                                out.material.data()};
        check(trt_render_aov(world.get_bvh(), &camera.pod, &params_, &b));
        return out;
    }
    // The frame denoised by its own feature buffers (trt_denoise: the a-trous filter of tinyrt.h guided by albedo, normal and depth):
    // `frame` as render() returned it, `aov` as render_aov() returned it for the same camera.
    static Image denoise(const Image& frame, const FeatureBuffers& aov, const trt_denoise_params* params = nullptr) {
        Image out(aov.width, aov.height);
        const trt_denoise_inputs in{frame.linear(), aov.albedo.data(), aov.normal.data(), aov.depth.data()};
        check(trt_denoise(&in, aov.width, aov.height, params, out.linear()));
        return out;
    }
    // denoise() with the variance-guided colour stop (trt_denoise_ex): `variance` as variance() returned it; sigma_color <= 0 = the
    // library's default (trt_denoise_color_default).
    static Image denoise(const Image& frame, const FeatureBuffers& aov, const std::vector<float>& variance, float sigma_color = 0.0f,
                         const trt_denoise_params* params = nullptr) {
        if (variance.size() != (size_t)aov.width * aov.height) throw Error(TRT_ERR_INVALID_ARG, "one variance per pixel");
        Image out(aov.width, aov.height);
        const trt_denoise_inputs in{frame.linear(), aov.albedo.data(), aov.normal.data(), aov.depth.data()};
        trt_denoise_color col;
        trt_denoise_color_default(&col);
        col.variance = variance.data();
        if (sigma_color > 0.0f) col.sigma_color = sigma_color;
        check(trt_denoise_ex(&in, &col, aov.width, aov.height, params, out.linear()));
        return out;
    }
    // The same call over several GPUs of the node (trt_render_multi): `devices` empty = every visible device.
    Image render_multi(const Camera& camera, World& world, const std::vector<int>& devices = {}, trt_stats* stats = nullptr) const {
        Image img(camera.pod.width, camera.pod.height);
        check(trt_render_multi(world.get_bvh(), &camera.pod, &params_, devices.empty() ? nullptr : devices.data(),
                               (uint32_t)devices.size(), img.linear(), stats));
        return img;
    }
    trt_render_params& params() { return params_; }
    // Scheduling knobs of this renderer (trt_tuning: every value renders the same frame).  Starts from the library defaults.
    trt_tuning& tuning() {
        if (!params_.tuning) { trt_tuning_default(&tuning_); params_.tuning = &tuning_; }
        return tuning_;
    }
    Renderer(const Renderer& o) : params_(o.params_), tuning_(o.tuning_) { if (o.params_.tuning) params_.tuning = &tuning_; }
    Renderer& operator=(const Renderer& o) {
        params_ = o.params_; tuning_ = o.tuning_;
        if (o.params_.tuning) params_.tuning = &tuning_;
        return *this;
    }

private:
    trt_render_params params_;
    trt_tuning tuning_{};
};

}  // namespace tinyrt
