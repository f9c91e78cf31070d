// FrayTracer.hpp — C++ host mirror of the reference's F# scene-composition API over the C ABI
// (include/fraytracer_hip.h).  The reference is compiled F#; no .NET toolchain exists in the build image,
// so this header is the compiled-language host layer: same module / function names and argument order
// as the F# (C++ keywords `union` -> `unionOf`), immutable value handles, errors as exceptions carrying
// ft_last_error().  INTEGRATION.md shows the F# [<DllImport>] form of the same calls.
//
//   SdfForm::Primitive::sphere/capsule/torus/triangle   src/FrayTracer/SdfForm.fs:117-268
//   SdfForm::unionOf/subtract/intersect/unionSmooth     src/FrayTracer/SdfForm.fs:14-91
//   SdfMaterial::createSolid                            src/FrayTracer/SdfMaterial.fs:4-7
//   SdfObject::create/unionOf/subtract/intersect        src/FrayTracer/SdfObject.fs:6-64
//   SdfLight::directional/point                         src/FrayTracer/SdfLight.fs:6-42
//   Lens::create, Camera::lookAt                        src/FrayTracer/Camera.fs:11-42
//   Image::renderScene                                  src/FrayTracer/Image.fs:26-35 + SdfScene.fs:7-28
//   Image::renderViews                                  renderScene over several cameras in one launch (ft_render_views)
//   Image::renderViewsHits                              renderHits over several cameras in one launch (ft_render_views_hits)
//   Image::traceRaysHits                                SdfObject.tryTrace (+ SdfScene.trace) over an explicit ray buffer in one launch (ft_trace_rays_hits)
//   Image::shadeHits / shadeHitsRelit                   SdfScene.trace from its hit on (SdfScene.fs:11-28) over hit records (ft_shade_hits, ft_scene_relight)
//   Image::lightVisibility / shadeVisible               which lights reach each record, one bit per light, and shading from those bits with no march
//                                                       (ft_light_visibility, ft_shade_visible)
//   Field::sampleLattice / samplePoints                 sdf.Distance, SdfForm.normal and the material at the points of a lattice or a point buffer
//                                                       (ft_sample_lattice, ft_sample_points; SdfForm.fs:7-12, 106-112)
//   Field::refineSegments                               where segments cross a level of the field, by bisection on the device (ft_refine_segments)
//   Mesh::ofLattice / ofValues                          the surface distance = iso as triangles, extracted on the device (ft_mesh_lattice, ft_mesh_values)
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/fraytracer_hip.h"

namespace FrayTracer {

struct Error : std::runtime_error {
    int code;
    Error(int c) : std::runtime_error(std::string("libfraytracer_hip: ") + ft_last_error()), code(c) {}
};
inline int check(int rc) { if (rc < 0) throw Error(rc); return rc; }

using Vector3 = ft_vec3;
struct FColor { Vector3 v; static FColor ofRGB(float r, float g, float b) { return FColor{Vector3{r, g, b}}; } };

class Context {                                   // one per GPU (device -1: construction only)
public:
    explicit Context(int device = 0) {
        if (ft_abi_version() != FT_ABI_VERSION) throw std::runtime_error("libfraytracer_hip: ABI version mismatch (header vs library)");
        check(ft_ctx_create(device, &ctx_));
    }
    ~Context() { ft_ctx_destroy(ctx_); }
    // per-context switches (ft_option); e.g. setOption(FT_OPT_MATH, FT_MATH_GLIBC_FMA): MathF.Exp / Log / Pow as this host's glibc computes them
    void setOption(ft_option option, int value) { check(ft_ctx_set_option(ctx_, (int32_t)option, value)); }
    // FT_OPT_ORDER (on by default): a scene's repeated frames hand out last frame's heavy tiles first; setOption(FT_OPT_ORDER, 0) keeps index order
    // FT_OPT_OCCL (on by default): shadow rays proved to end in a hit stop marching; setOption(FT_OPT_OCCL, 0) marches every one; FT_OPT_OCCL_POLICY: its schedule
    // FT_OPT_TRY_HINT (on by default): a scene's repeated frames try each tile's bundle certificates around the rounds they held on in the last frame;
    // setOption(FT_OPT_TRY_HINT, 0) keeps every frame on the first frame's schedule, 2 records without following
    // FT_OPT_DEPART (on by default): the frames that follow try hints end lit shadow rays where they are born; setOption(FT_OPT_DEPART, 0) marches them as
    // before, 2 tries on every camera launch of the kernel family
    int getOption(ft_option option) const { int32_t v = 0; check(ft_ctx_get_option(ctx_, (int32_t)option, &v)); return v; }
    static std::string buildInfo() { return ft_build_info(); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ft_ctx* get() const { return ctx_; }
private:
    ft_ctx* ctx_ = nullptr;
};

struct SdfFormV { ft_handle Node; ft_ctx* ctx; };
struct SdfMaterialV { ft_handle Node; ft_ctx* ctx; };
struct SdfObjectV { ft_handle Node; ft_ctx* ctx; };
struct SdfLightV { ft_handle Node; ft_ctx* ctx; };
struct SdfScene { SdfObjectV Object; FColor BackgroundColor; std::vector<SdfLightV> Lights; };   // Types.fs:74-79

inline std::vector<ft_handle> nodes(const std::vector<SdfFormV>& v) { std::vector<ft_handle> h; for (auto& f : v) h.push_back(f.Node); return h; }

namespace SdfForm {
namespace Primitive {
inline SdfFormV sphere(const Context& c, const ft_sphere& d) { return {check(ft_form_sphere(c.get(), &d)), c.get()}; }
inline SdfFormV capsule(const Context& c, const ft_capsule& d) { return {check(ft_form_capsule(c.get(), &d)), c.get()}; }
inline SdfFormV torus(const Context& c, const ft_torus& d) { return {check(ft_form_torus(c.get(), &d)), c.get()}; }
inline SdfFormV triangle(const Context& c, const ft_triangle& d) { return {check(ft_form_triangle(c.get(), &d)), c.get()}; }
}  // namespace Primitive
inline SdfFormV unionOf(const std::vector<SdfFormV>& forms) {
    if (forms.empty()) throw std::invalid_argument("No SdfObjects given.");
    auto h = nodes(forms); return {check(ft_form_union(forms[0].ctx, h.data(), (int)h.size())), forms[0].ctx};
}
inline SdfFormV subtract(SdfFormV a, SdfFormV b) { return {check(ft_form_subtract(a.ctx, a.Node, b.Node)), a.ctx}; }
inline SdfFormV intersect(const std::vector<SdfFormV>& forms) {
    if (forms.empty()) throw std::invalid_argument("No SdfObjects given.");
    auto h = nodes(forms); return {check(ft_form_intersect(forms[0].ctx, h.data(), (int)h.size())), forms[0].ctx};
}
inline SdfFormV unionSmooth(float strength, const std::vector<SdfFormV>& forms) {
    if (forms.empty()) throw std::invalid_argument("blub");
    auto h = nodes(forms); return {check(ft_form_union_smooth(forms[0].ctx, strength, h.data(), (int)h.size())), forms[0].ctx};
}
}  // namespace SdfForm

namespace SdfMaterial {
inline SdfMaterialV createSolid(const Context& c, FColor color) { return {check(ft_material_solid(c.get(), &color.v.x)), c.get()}; }
// EXTENSION (not in the reference): refracting material, see ft_material_glass
inline SdfMaterialV createGlass(const Context& c, FColor tint, float ior, float dispersion = 0.0f) {
    return {check(ft_material_glass(c.get(), &tint.v.x, ior, dispersion)), c.get()};
}
}

namespace SdfObject {
inline SdfObjectV create(SdfMaterialV material, SdfFormV form) { return {check(ft_object_create(form.ctx, material.Node, form.Node)), form.ctx}; }
inline SdfObjectV unionOf(const std::vector<SdfObjectV>& objects) {
    if (objects.empty()) throw std::invalid_argument("No SdfObjects given.");
    std::vector<ft_handle> h; for (auto& o : objects) h.push_back(o.Node);
    return {check(ft_object_union(objects[0].ctx, h.data(), (int)h.size())), objects[0].ctx};
}
inline SdfObjectV subtract(SdfObjectV object, SdfFormV form) { return {check(ft_object_subtract(object.ctx, object.Node, form.Node)), object.ctx}; }
inline SdfObjectV intersect(SdfObjectV object, const std::vector<SdfFormV>& forms) {
    auto h = nodes(forms); return {check(ft_object_intersect(object.ctx, object.Node, h.data(), (int)h.size())), object.ctx};
}
}  // namespace SdfObject

namespace SdfLight {
inline SdfLightV directional(const Context& c, Vector3 direction, FColor color) { return {check(ft_light_directional(c.get(), &direction.x, &color.v.x)), c.get()}; }
inline SdfLightV point(const Context& c, Vector3 position, FColor color) { return {check(ft_light_point(c.get(), &position.x, &color.v.x)), c.get()}; }
}

struct LensV { float NearPlaneSize; };
namespace Lens { inline LensV create(float fieldOfView) { return {ft_lens_create(fieldOfView)}; } }
namespace Camera {
struct LookAt { Vector3 Position, LookAtPoint, Up; LensV Lens; };
inline ft_camera lookAt(const LookAt& c) {
    ft_camera out; check(ft_camera_look_at(&c.Position.x, &c.LookAtPoint.x, &c.Up.x, c.Lens.NearPlaneSize, &out)); return out;
}
}
struct ImageSize { int X, Y; };

// The ft_scene of one call: realised from an SdfScene — or from an object alone, in front of a black background and without lights, for tryTrace /
// formTryTrace — and destroyed on every path out of the call, exceptions included.
class SceneOfCall {
public:
    explicit SceneOfCall(const SdfScene& scene) : ctx(scene.Object.ctx) {
        std::vector<ft_handle> lights; for (auto& l : scene.Lights) lights.push_back(l.Node);
        check(ft_scene_create(ctx, scene.Object.Node, &scene.BackgroundColor.v.x, lights.data(), (int)lights.size(), &s_));
    }
    explicit SceneOfCall(const SdfObjectV& object) : ctx(object.ctx) {
        const float black[3] = {0.0f, 0.0f, 0.0f};
        check(ft_scene_create(ctx, object.Node, black, nullptr, 0, &s_));
    }
    // src's object under the background and lights of `lit` (ft_scene_relight: no flatten, no grid build); `lit.Object` is not looked at
    SceneOfCall(const SceneOfCall& src, const SdfScene& lit) : ctx(src.ctx) {
        std::vector<ft_handle> lights; for (auto& l : lit.Lights) lights.push_back(l.Node);
        check(ft_scene_relight(src.get(), &lit.BackgroundColor.v.x, lights.data(), (int)lights.size(), &s_));
    }
    ~SceneOfCall() { ft_scene_destroy(s_); }
    SceneOfCall(const SceneOfCall&) = delete;
    SceneOfCall& operator=(const SceneOfCall&) = delete;
    ft_scene* get() const { return s_; }
    // the end of every call: the error, if any, as an exception; the statistics to the caller who asked for them
    void done(int rc, ft_stats* stats) const { check(rc); if (stats) *stats = st; }
    ft_ctx* const ctx;
    ft_stats st{};
private:
    ft_scene* s_ = nullptr;
};
// the reference's parameters of a whole frame: every column, one rank, no EXTENSION
inline ft_render_params frameParams(float epsilon, float length, ImageSize size) {
    return ft_render_params{size.X, size.Y, 0, size.X, size.X, 1, 0, 1, epsilon, length, 0, 0.0f, 0, 0};
}

namespace Image {
// FColor[X,Y] as a flat vector, x-major / y contiguous (Array2D.fs:30-38): element (x, y) at 3 * (x * Y + y)
inline std::vector<float> renderScene(float epsilon, float length, ImageSize size, const ft_camera& camera, const SdfScene& scene,
                                      ft_stats* stats = nullptr) {
    SceneOfCall s(scene);
    std::vector<float> out((size_t)size.X * size.Y * 3);
    const ft_render_params p = frameParams(epsilon, length, size);
    s.done(ft_render(s.ctx, s.get(), &camera, &p, out.data(), &s.st), stats);
    return out;
}
// renderScene of one scene from every camera of `cameras` in one launch: image k at 3 * (k * X * Y + x * Y + y), bit for bit renderScene's
// image for cameras[k]; stats of the whole batch
inline std::vector<float> renderViews(float epsilon, float length, ImageSize size, const std::vector<ft_camera>& cameras, const SdfScene& scene,
                                      ft_stats* stats = nullptr) {
    SceneOfCall s(scene);
    std::vector<float> out(cameras.size() * (size_t)size.X * size.Y * 3);
    const ft_render_params p = frameParams(epsilon, length, size);
    s.done(ft_render_views(s.ctx, s.get(), cameras.data(), (int32_t)cameras.size(), &p, out.data(), &s.st), stats);
    return out;
}
// EXTENSION: Image.render's pixel loop (Image.fs:26-35) over SdfObject.tryTrace scene.Object (SdfObject.fs:66-78) instead of SdfScene.trace —
// every pixel's camera ray as ft_object_trace_result (hit == 0 is ValueNone), laid out like renderScene's image.  `material`, if given, receives
// the handle of the material each hit picked (-1 on a miss).
inline std::vector<ft_object_trace_result> renderHits(float epsilon, float length, ImageSize size, const ft_camera& camera, const SdfScene& scene,
                                                      std::vector<int32_t>* material = nullptr, ft_stats* stats = nullptr) {
    SceneOfCall s(scene);
    std::vector<ft_object_trace_result> out((size_t)size.X * size.Y);
    if (material) material->assign(out.size(), -1);
    const ft_render_params p = frameParams(epsilon, length, size);
    s.done(ft_render_hits(s.ctx, s.get(), &camera, &p, nullptr, out.data(), material ? material->data() : nullptr, &s.st), stats);
    return out;
}
// EXTENSION: renderHits of one scene from every camera of `cameras` in one launch: view k's record of pixel (x, y) at k * X * Y + x * Y + y,
// bit for bit renderHits' record for cameras[k]; `material` likewise; stats of the whole batch
inline std::vector<ft_object_trace_result> renderViewsHits(float epsilon, float length, ImageSize size, const std::vector<ft_camera>& cameras,
                                                           const SdfScene& scene, std::vector<int32_t>* material = nullptr, ft_stats* stats = nullptr) {
    SceneOfCall s(scene);
    std::vector<ft_object_trace_result> out(cameras.size() * (size_t)size.X * size.Y);
    if (material) material->assign(out.size(), -1);
    const ft_render_params p = frameParams(epsilon, length, size);
    s.done(ft_render_views_hits(s.ctx, s.get(), cameras.data(), (int32_t)cameras.size(), &p, nullptr, out.data(), material ? material->data() : nullptr, &s.st),
           stats);
    return out;
}
// EXTENSION: SdfObject.tryTrace scene.Object of every ray of an explicit ray buffer (`rays |> Array.map (SdfObject.tryTrace scene.Object)`) and, if
// `colors` is given, SdfScene.trace scene of the same rays (3 floats per ray) from the same launch (ft_trace_rays_hits); `material` as in renderHits
inline std::vector<ft_object_trace_result> traceRaysHits(const std::vector<ft_ray>& rays, const SdfScene& scene, std::vector<float>* colors = nullptr,
                                                         std::vector<int32_t>* material = nullptr, ft_stats* stats = nullptr) {
    SceneOfCall s(scene);
    std::vector<ft_object_trace_result> out(rays.size());
    if (colors) colors->assign(rays.size() * 3, 0.0f);
    if (material) material->assign(rays.size(), -1);
    s.done(ft_trace_rays_hits(s.ctx, s.get(), rays.data(), (int64_t)rays.size(), colors ? colors->data() : nullptr, out.data(),
                              material ? material->data() : nullptr, &s.st), stats);
    return out;
}
// Relighting without re-tracing: SdfScene.trace from its `| ValueSome result ->` arm on (SdfScene.fs:11-28) for every record of `hits` (what renderHits /
// traceRaysHits / tryTrace returned for a scene with the same Object; hit == 0 shades to the background) -> 3 floats per record (ft_shade_hits)
inline std::vector<float> shadeHits(const std::vector<ft_object_trace_result>& hits, const SdfScene& scene, ft_stats* stats = nullptr) {
    SceneOfCall s(scene);
    std::vector<float> out(hits.size() * 3);
    s.done(ft_shade_hits(s.ctx, s.get(), hits.data(), (int64_t)hits.size(), out.data(), &s.st), stats);
    return out;
}
// the same records under the background and lights of each scene of `lit`, whose Object is taken to be scene.Object: the object is flattened
// once and every further light set costs one ft_scene_relight (a copy and an upload) and one ft_shade_hits
inline std::vector<std::vector<float>> shadeHitsRelit(const std::vector<ft_object_trace_result>& hits, const SdfScene& scene, const std::vector<SdfScene>& lit) {
    SceneOfCall base(scene);
    std::vector<std::vector<float>> frames;
    for (auto& l : lit) {
        SceneOfCall s(base, l);
        frames.emplace_back(hits.size() * 3);
        s.done(ft_shade_hits(s.ctx, s.get(), hits.data(), (int64_t)hits.size(), frames.back().data(), &s.st), nullptr);
    }
    return frames;
}
// Light visibility masks: bit i of a record's mask is set where scene.Lights[i] reaches it, i.e. where SdfScene.fs:23 executes (ft_light_visibility).
// select: the lights to march (all by default); previous: masks whose other bits are kept, so that a moved light costs only its own shadow rays.
inline std::vector<uint32_t> lightVisibility(const std::vector<ft_object_trace_result>& hits, const SdfScene& scene, uint32_t select = 0xFFFFFFFFu,
                                             const std::vector<uint32_t>* previous = nullptr, ft_stats* stats = nullptr) {
    if (previous && previous->size() != hits.size()) throw std::invalid_argument("lightVisibility: one previous mask per record");
    SceneOfCall s(scene);
    std::vector<uint32_t> out(hits.size());
    s.done(ft_light_visibility(s.ctx, s.get(), hits.data(), (int64_t)hits.size(), select, previous ? previous->data() : nullptr, out.data(), &s.st), stats);
    return out;
}
// shadeHits with every shadow ray answered by `visibility` (masks of a scene with the same Object and the same light directions and positions): no
// march, bit for bit shadeHits' colours under `scene` (ft_shade_visible)
inline std::vector<float> shadeVisible(const std::vector<ft_object_trace_result>& hits, const std::vector<uint32_t>& visibility, const SdfScene& scene,
                                       ft_stats* stats = nullptr) {
    if (visibility.size() != hits.size()) throw std::invalid_argument("shadeVisible: one mask per record");
    SceneOfCall s(scene);
    std::vector<float> out(hits.size() * 3);
    s.done(ft_shade_visible(s.ctx, s.get(), hits.data(), visibility.data(), (int64_t)hits.size(), out.data(), &s.st), stats);
    return out;
}
// Image.toColors gamma rng image (Image.fs:37-50) on the GPU: bytes in Color[X,Y] order (R,G,B) or, with bmpOrder, in the scan-line
// order of Image.toBitmap (Image.fs:61-86: rows from the top, B,G,R).  seed < 0: no dithering noise (the reference's is racy).
inline std::vector<unsigned char> toColors(ft_ctx* ctx, float gamma, long long seed, const std::vector<float>& image, ImageSize size, bool bmpOrder = false) {
    std::vector<unsigned char> out((size_t)size.X * size.Y * 3);
    ft_tonemap_params tm{gamma, seed >= 0 ? 1 : 0, (uint32_t)(seed >= 0 ? seed : 0), bmpOrder ? 1 : 0};
    check(ft_tone_map_host(ctx, image.data(), size.X, size.Y, &tm, out.data(), nullptr));
    return out;
}
}  // namespace Image

// The distance field itself.  Samples: distance per point, and where asked for the normal (SdfForm.normal sdf normalEpsilon p) and the handle of the
// material object.Material.Color p picks.  bounded: SdfForm.tryDistance — outside the form's boundary nothing is evaluated (NaN, NaN, -1).
namespace Field {
struct Samples { std::vector<float> distance; std::vector<ft_vec3> normal; std::vector<int32_t> material; };
struct Request { bool normal = false; float normalEpsilon = 0.0f; bool material = false; bool bounded = false; };
// point (i, j, k) = origin + (i, j, k) * step per coordinate (one float32 product, one float32 sum); its results at (i * ny + j) * nz + k
inline Samples sampleLattice(const SdfScene& scene, const ft_lattice& lattice, const Request& r = Request{}) {
    SceneOfCall s(scene);
    const size_t n = (size_t)lattice.nx * (size_t)lattice.ny * (size_t)lattice.nz;
    Samples out;
    out.distance.resize(n);
    if (r.normal) out.normal.resize(n);
    if (r.material) out.material.assign(n, -1);
    s.done(ft_sample_lattice(s.ctx, s.get(), &lattice, r.normalEpsilon, r.bounded ? FT_FIELD_BOUNDED : 0u, out.distance.data(),
                             r.normal ? out.normal.data() : nullptr, r.material ? out.material.data() : nullptr), nullptr);
    return out;
}
inline Samples samplePoints(const SdfScene& scene, const std::vector<ft_vec3>& points, const Request& r = Request{}) {
    SceneOfCall s(scene);
    Samples out;
    out.distance.resize(points.size());
    if (r.normal) out.normal.resize(points.size());
    if (r.material) out.material.assign(points.size(), -1);
    s.done(ft_sample_points(s.ctx, s.get(), points.data(), (int64_t)points.size(), r.normalEpsilon, r.bounded ? FT_FIELD_BOUNDED : 0u, out.distance.data(),
                            r.normal ? out.normal.data() : nullptr, r.material ? out.material.data() : nullptr), nullptr);
    return out;
}
// where the segments a[r] .. b[r] cross the level iso, by `steps` bisection rounds (ft_refine_segments): status 1 and the crossing found (a crossing, not
// necessarily the first), or status 0 and three NaN where the ends' distances are not finite or not on opposite sides
struct Crossings { std::vector<ft_vec3> points; std::vector<int32_t> status; };
inline Crossings refineSegments(const SdfScene& scene, const std::vector<ft_vec3>& a, const std::vector<ft_vec3>& b, float iso = 0.0f, int32_t steps = 8) {
    if (a.size() != b.size()) throw std::invalid_argument("Field::refineSegments: one b per a");
    SceneOfCall s(scene);
    Crossings out;
    out.points.resize(a.size());
    out.status.assign(a.size(), 0);
    s.done(ft_refine_segments(s.ctx, s.get(), a.data(), b.data(), (int64_t)a.size(), iso, steps, out.points.data(), out.status.data()), nullptr);
    return out;
}
}  // namespace Field

// The surface {distance = iso} as triangles, extracted on the device from the distances on a lattice (ft_mesh_lattice: marching tetrahedra on the
// Kuhn subdivision; the header states the rule).  triangles: three vertex indices each, counter-clockwise seen from the outside; normal and material
// per vertex where asked for (SdfForm.normal sdf normalEpsilon v; the handle of the material object.Material.Color v picks)
namespace Mesh {
// vertexShell, triangleShell, shells, shellsInfo: filled where the request asked for shells (the header's "Shells": the mesh's connected pieces, numbered
// by their smallest vertex; -1 for a vertex no triangle names)
struct Triangles {
    std::vector<ft_vec3> vertices; std::vector<int32_t> triangles; std::vector<ft_vec3> normal; std::vector<int32_t> material; int64_t skipped = 0;
    std::vector<int32_t> vertexShell, triangleShell; std::vector<ft_shell> shells; ft_shells_info shellsInfo{};
    // shellMeasures (one per shell) and measure (the whole mesh): filled where the request asked for measures (the header's "Measures")
    std::vector<ft_shell_measure> shellMeasures; ft_shell_measure measure{};
};
// refineSteps: -1 the mesher's vertices; 0 .. 32 bisection rounds that move every vertex along its lattice edge onto the surface (ft_mesh_lattice_refined)
// shells: also label the mesh's shells (ft_mesh_shells); keepLargest: > 0 keeps only that many shells, the ones with the most triangles, ties going to
// the lower number (ft_mesh_select), and implies shells — the labels are then those of the selected mesh.  measures: also each shell's and the whole
// mesh's area, signed volume, first moment and box (ft_shells_measure, ft_mesh_measure; implies shells); keepBodies: keeps only the closed shells of
// positive volume — no cavities, no open debris — before keepLargest is applied to what is left
struct Request { float iso = 0.0f; bool normal = false; float normalEpsilon = 0.0f; bool material = false; int32_t refineSteps = -1; bool shells = false; int32_t keepLargest = 0;
                 bool measures = false; bool keepBodies = false; };
struct ShellsOwner { ft_shells* s = nullptr; ~ShellsOwner() { ft_shells_destroy(s); } };
inline void readShells(ft_mesh* mesh, Triangles& out, bool measures = false) {
    ShellsOwner sh;
    check(ft_mesh_shells(mesh, &sh.s));
    check(ft_shells_get_info(sh.s, &out.shellsInfo));
    out.vertexShell.resize((size_t)out.shellsInfo.n_vertices);
    out.triangleShell.resize((size_t)out.shellsInfo.n_triangles);
    out.shells.resize((size_t)out.shellsInfo.n_shells);
    check(ft_shells_read(sh.s, out.vertexShell.data(), out.triangleShell.data(), out.shells.data()));
    if (!measures) return;
    out.shellMeasures.resize(out.shells.size());
    check(ft_shells_measure(mesh, sh.s, out.shellMeasures.data()));
    check(ft_mesh_measure(mesh, &out.measure));                        // an empty mesh: nothing is written, the record stays zero
}
// the mesh of the closed shells of positive volume of `mesh`, which is destroyed
inline ft_mesh* keepBodies(ft_mesh* mesh) {
    struct Owner { ft_mesh* m; ~Owner() { ft_mesh_destroy(m); } } own{mesh};
    ShellsOwner sh;
    check(ft_mesh_shells(mesh, &sh.s));
    ft_shells_info info{};
    check(ft_shells_get_info(sh.s, &info));
    std::vector<ft_shell> records((size_t)info.n_shells);
    std::vector<ft_shell_measure> measures(records.size());
    check(ft_shells_read(sh.s, nullptr, nullptr, records.data()));
    check(ft_shells_measure(mesh, sh.s, measures.data()));
    std::vector<uint8_t> keep(records.size(), 0);
    for (size_t i = 0; i < keep.size(); ++i) keep[i] = records[i].n_border_edges == 0 && measures[i].volume > 0.0;
    ft_mesh* selected = nullptr;
    check(ft_mesh_select(mesh, sh.s, keep.data(), (int64_t)keep.size(), &selected));
    return selected;
}
// the mesh of the keepLargest largest shells of `mesh`, which is destroyed
inline ft_mesh* keepLargest(ft_mesh* mesh, int32_t k) {
    struct Owner { ft_mesh* m; ~Owner() { ft_mesh_destroy(m); } } own{mesh};
    ShellsOwner sh;
    check(ft_mesh_shells(mesh, &sh.s));
    ft_shells_info info{};
    check(ft_shells_get_info(sh.s, &info));
    std::vector<ft_shell> records((size_t)info.n_shells);
    check(ft_shells_read(sh.s, nullptr, nullptr, records.data()));
    std::vector<size_t> order(records.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return records[a].n_triangles > records[b].n_triangles; });
    std::vector<uint8_t> keep(records.size(), 0);
    for (size_t i = 0; i < order.size() && i < (size_t)k; ++i) keep[order[i]] = 1;
    ft_mesh* selected = nullptr;
    check(ft_mesh_select(mesh, sh.s, keep.data(), (int64_t)keep.size(), &selected));
    return selected;
}
inline Triangles read(ft_mesh* mesh, const Request& r = Request{}) {
    if (r.keepBodies) mesh = keepBodies(mesh);
    if (r.keepLargest > 0) mesh = keepLargest(mesh, r.keepLargest);
    struct Owner { ft_mesh* m; ~Owner() { ft_mesh_destroy(m); } } own{mesh};
    ft_mesh_info info{};
    check(ft_mesh_get_info(mesh, &info));
    Triangles out;
    out.skipped = info.n_skipped;
    out.vertices.resize((size_t)info.n_vertices);
    out.triangles.resize(3 * (size_t)info.n_triangles);
    if (info.has_normal) out.normal.resize((size_t)info.n_vertices);
    if (info.has_material) out.material.resize((size_t)info.n_vertices);
    check(ft_mesh_read(mesh, out.vertices.data(), out.triangles.data(), info.has_normal ? out.normal.data() : nullptr,
                       info.has_material ? out.material.data() : nullptr));
    if (r.shells || r.keepLargest > 0 || r.measures || r.keepBodies) readShells(mesh, out, r.measures);
    return out;
}
inline Triangles ofLattice(const SdfScene& scene, const ft_lattice& lattice, const Request& r = Request{}) {
    SceneOfCall s(scene);
    ft_mesh* mesh = nullptr;
    const uint32_t flags = (r.normal ? FT_MESH_NORMAL : 0u) | (r.material ? FT_MESH_MATERIAL : 0u);
    s.done(r.refineSteps < 0 ? ft_mesh_lattice(s.ctx, s.get(), &lattice, r.iso, r.normalEpsilon, flags, &mesh)
                             : ft_mesh_lattice_refined(s.ctx, s.get(), &lattice, r.iso, r.normalEpsilon, flags, r.refineSteps, &mesh), nullptr);
    return read(mesh, r);
}
// any float32 lattice already in host memory: nx * ny * nz values, k contiguous (ft_mesh_values)
inline Triangles ofValues(ft_ctx* ctx, const ft_lattice& lattice, const std::vector<float>& values, float iso = 0.0f) {
    if (values.size() != (size_t)lattice.nx * (size_t)lattice.ny * (size_t)lattice.nz) throw std::invalid_argument("Mesh::ofValues: one value per lattice point");
    ft_mesh* mesh = nullptr;
    check(ft_mesh_values(ctx, &lattice, values.data(), iso, &mesh));
    return read(mesh);
}
}  // namespace Mesh

// The contours {distance = iso} of every lattice plane normal to `axis` as ordered polylines, extracted and chained on the device (ft_slice_lattice;
// the header's "Slicing" states the rule).  polylines: points [first, first + count) of slice `slice`, closed (a loop: counter-clockwise seen from
// +axis around the inside, clockwise around a hole) or open; normal and material per point where asked for
namespace Slice {
struct Contours {
    std::vector<ft_vec3> points; std::vector<ft_polyline> polylines; std::vector<ft_vec3> normal; std::vector<int32_t> material;
    int64_t closed = 0, skipped = 0; int32_t axis = 2, slices = 0;
    // measures (one per polyline) and layerMeasures (one per slice, holes subtracted): filled where the request asked for measures (the header's
    // "Contour measures"); the centroid of a record is moment / area in the plane's (u, v)
    std::vector<ft_contour_measure> measures; std::vector<ft_slice_measure> layerMeasures;
};
// refineSteps: as Mesh::Request's (ft_slice_lattice_refined): the points are then the refined mesh vertices of the same edges.  measures: also each
// polyline's and each slice's length, signed area, first moment and box (ft_slices_measure)
struct Request { int32_t axis = 2; float iso = 0.0f; bool normal = false; float normalEpsilon = 0.0f; bool material = false; int32_t refineSteps = -1;
                 bool measures = false; };
inline Contours read(ft_slices* slices, bool measures = false) {
    struct Owner { ft_slices* s; ~Owner() { ft_slices_destroy(s); } } own{slices};
    ft_slices_info info{};
    check(ft_slices_get_info(slices, &info));
    Contours out;
    out.closed = info.n_closed; out.skipped = info.n_skipped; out.axis = info.axis; out.slices = info.n_slices;
    out.points.resize((size_t)info.n_points);
    out.polylines.resize((size_t)info.n_polylines);
    if (info.has_normal) out.normal.resize((size_t)info.n_points);
    if (info.has_material) out.material.resize((size_t)info.n_points);
    check(ft_slices_read(slices, out.points.data(), out.polylines.data(), info.has_normal ? out.normal.data() : nullptr,
                         info.has_material ? out.material.data() : nullptr));
    if (measures) {
        out.measures.resize(out.polylines.size());
        out.layerMeasures.resize((size_t)info.n_slices);
        check(ft_slices_measure(slices, out.measures.empty() ? nullptr : out.measures.data(), out.layerMeasures.empty() ? nullptr : out.layerMeasures.data()));
    }
    return out;
}
inline Contours ofLattice(const SdfScene& scene, const ft_lattice& lattice, const Request& r = Request{}) {
    SceneOfCall s(scene);
    ft_slices* slices = nullptr;
    const uint32_t flags = (r.normal ? FT_SLICE_NORMAL : 0u) | (r.material ? FT_SLICE_MATERIAL : 0u);
    s.done(r.refineSteps < 0 ? ft_slice_lattice(s.ctx, s.get(), &lattice, r.axis, r.iso, r.normalEpsilon, flags, &slices)
                             : ft_slice_lattice_refined(s.ctx, s.get(), &lattice, r.axis, r.iso, r.normalEpsilon, flags, r.refineSteps, &slices), nullptr);
    return read(slices, r.measures);
}
// any float32 lattice already in host memory: nx * ny * nz values, k contiguous (ft_slice_values)
inline Contours ofValues(ft_ctx* ctx, const ft_lattice& lattice, const std::vector<float>& values, int32_t axis = 2, float iso = 0.0f, bool measures = false) {
    if (values.size() != (size_t)lattice.nx * (size_t)lattice.ny * (size_t)lattice.nz) throw std::invalid_argument("Slice::ofValues: one value per lattice point");
    ft_slices* slices = nullptr;
    check(ft_slice_values(ctx, &lattice, values.data(), axis, iso, &slices));
    return read(slices, measures);
}
}  // namespace Slice

// SdfObject.tryTrace / SdfForm.tryTrace (SdfObject.fs:66-78, SdfForm.fs:93-104) over a ray buffer; hit == 0 is ValueNone
inline std::vector<ft_object_trace_result> tryTrace(const SdfObjectV& object, const std::vector<ft_ray>& rays) {
    SceneOfCall s(object);
    std::vector<ft_object_trace_result> out(rays.size());
    s.done(ft_object_try_trace(s.ctx, s.get(), rays.data(), (int64_t)rays.size(), out.data(), nullptr), nullptr);
    return out;
}
inline std::vector<ft_form_trace_result> formTryTrace(const SdfObjectV& object, const std::vector<ft_ray>& rays) {
    SceneOfCall s(object);
    std::vector<ft_form_trace_result> out(rays.size());
    s.done(ft_form_try_trace(s.ctx, s.get(), rays.data(), (int64_t)rays.size(), out.data(), nullptr), nullptr);
    return out;
}

}  // namespace FrayTracer
