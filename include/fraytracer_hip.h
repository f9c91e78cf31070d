/* fraytracer_hip.h — C ABI of libfraytracer_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for FrayTracer's per-pixel hot path.  The reference has no FFI: the
 * seam is `SdfScene.trace : SdfScene -> Ray -> FColor` (src/FrayTracer/SdfScene.fs:7-8)
 * driven by `Image.render` (src/FrayTracer/Image.fs:26-35), called once from
 * src/FrayTracer.Console/Program.fs:90-93.  Because an F# scene is a record of opaque
 * closures (src/FrayTracer/Types.fs:40-55), every scene constructor of the reference gets a
 * native twin here; the F# layer calls the twin next to building its closure and keeps the
 * returned handle (INTEGRATION.md shows the [<DllImport>] stubs).  The library owns
 * flattening (boundaries, uniform grids) and all device work.
 *
 * Conventions: plain C, no exceptions cross the boundary.  Functions return 0 / a handle
 * >= 0 on success and a negative ft_status on failure; ft_last_error() gives the message
 * for the calling thread.  All structs are float/int32 only, 4-byte aligned, and match the
 * sequential layout of the F# [<Struct>] records they mirror, so they are blittable.
 * Inputs are copied; the caller keeps ownership.  A context is not re-entrant; distinct
 * contexts may be used from distinct threads.  There is NO CPU fallback: every render /
 * trace entry point fails with FT_ERR_NO_DEVICE when the context has no GPU.
 */
#ifndef FRAYTRACER_HIP_H
#define FRAYTRACER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FT_ABI_VERSION 5
#define FT_FIELD_BOUNDED 1u   /* flag bit of ft_sample_points / ft_sample_lattice ("Field sampling" below): SdfForm.tryDistance, only where SdfBoundary.isInside */

typedef enum ft_status {
    FT_OK = 0,
    FT_ERR_INVALID = -1,      /* bad handle / argument */
    FT_ERR_NO_DEVICE = -2,    /* context was created without a GPU, or HIP reports none */
    FT_ERR_HIP = -3,          /* a HIP runtime call failed (message has the HIP error string) */
    FT_ERR_UNSUPPORTED = -4,  /* scene exceeds a documented limit (DESIGN.md "Limits") */
    FT_ERR_EMPTY = -5,        /* empty child list: the reference throws "No SdfObjects given." */
    FT_ERR_COMM = -6          /* RCCL failure in ft_render_multi */
} ft_status;

typedef int32_t ft_handle;                 /* index into a context-owned table; < 0 is an ft_status */
typedef struct ft_ctx ft_ctx;
typedef struct ft_scene ft_scene;

/* ---- blittable mirrors of the reference records ------------------------------------ */
typedef struct ft_vec3 { float x, y, z; } ft_vec3;                       /* System.Numerics.Vector3 */
typedef struct ft_ray {                                                  /* Types.fs:9-17 (32 B) */
    ft_vec3 origin; ft_vec3 direction; float length; float epsilon;
} ft_ray;
typedef struct ft_boundary { ft_vec3 center; float radius; } ft_boundary;/* Types.fs:19-24 (16 B) */
/* SdfFormTraceResult voption (Types.fs:32-37): `hit` = 0 is ValueNone (the other fields are then 0) */
typedef struct ft_form_trace_result { ft_ray ray; float distance; int32_t hit; } ft_form_trace_result;              /* 40 B */
/* SdfObjectTraceResult voption (Types.fs:57-65): Ray (origin pulled back by epsilon, SdfObject.fs:73), Normal, Color */
typedef struct ft_object_trace_result { ft_ray ray; ft_vec3 normal; ft_vec3 color; int32_t hit; int32_t reserved; } ft_object_trace_result;   /* 64 B */
typedef struct ft_sphere { ft_vec3 center; float radius; } ft_sphere;    /* SdfForm.fs:118-123 */
typedef struct ft_capsule { ft_vec3 from; ft_vec3 to; float radius; } ft_capsule;        /* SdfForm.fs:137-143 */
typedef struct ft_torus { ft_vec3 center; ft_vec3 normal; float major_radius; float minor_radius; } ft_torus; /* SdfForm.fs:172-179 */
typedef struct ft_triangle { ft_vec3 v1; ft_vec3 v2; ft_vec3 v3; float radius; } ft_triangle;  /* SdfForm.fs:205-212 */
typedef struct ft_box { ft_vec3 center; ft_vec3 half_extent; } ft_box;   /* EXTENSION: not in the reference */
typedef struct ft_camera {                                               /* Camera.fs:16-22 (48 B) */
    ft_vec3 position; ft_vec3 forward; ft_vec3 up_scaled; ft_vec3 right_scaled;
} ft_camera;

/* Image.render arguments (Image.fs:26) plus the column tiling used for multi-GPU.
 * Local column c in [0, n_columns) maps to image column
 *     x = x0 + (c / stripe_width) * stripe_width * stripe_ranks + stripe_rank * stripe_width + c % stripe_width
 * (stripe_ranks = 1, stripe_rank = 0 gives the contiguous range [x0, x0 + n_columns)).
 * Output is n_columns x height x 3 float32, column-major / y contiguous: exactly the
 * FColor[X,Y] layout Array2D.Parallel.init produces (Array2D.fs:30-38). */
typedef struct ft_render_params {
    int32_t width, height;        /* ImageSize.X, ImageSize.Y (Image.fs:8-13) */
    int32_t x0, n_columns;
    int32_t stripe_width, stripe_ranks, stripe_rank;
    int32_t spp;                  /* 1 = the reference (one corner sample). >1 is an EXTENSION. */
    float epsilon, length;        /* Image.render's first two arguments */
    int32_t ao_samples;           /* 0 = the reference. >0: EXTENSION ambient-occlusion rays */
    float ao_radius;              /* Length of every ambient-occlusion ray. <= 0 (the default 0 included): the rays are cast and counted, and
                                   * each ends open without an evaluation (SdfForm.tryTrace tests the Length first): the frame of ao_samples = 0 */
    int32_t max_bounces;          /* 0 = the reference (glass shades as createSolid tint). >0: EXTENSION, glass
                                   * materials refract / reflect; a path ends black after this many interactions */
    int32_t spectral;             /* 0 = off. 1..16: EXTENSION, sample k is traced at wavelength bin k % spectral
                                   * (must divide spp) and weighted with that bin's RGB response */
} ft_render_params;

typedef struct ft_stats {         /* filled per call; all counts are exact */
    uint64_t rays_primary, rays_shadow, rays_ext;
    uint64_t hits_primary, hits_shadow;
    uint64_t sdf_evals;           /* scene-SDF evaluations (march steps + normal probes) */
    uint64_t flags;               /* bit0 NaN distance met, bit2 step cap hit (reference would not terminate) */
    float kernel_ms;              /* HIP-event time of the render kernel(s) of this call */
    float culled_fraction;        /* lean kernel: share of the (child, ray) pairs of the smooth union that were dropped as exact no-ops (FT_OPT_CULL) */
    uint64_t wave_evals;          /* wave-level evaluation rounds: sdf_evals / (64 * wave_evals) = lane utilisation */
    float shader_mhz;             /* shader clock the render kernel(s) of this call ran at: s_memtime ticks / s_memrealtime ticks
                                   * (constant 100 MHz) of one wave that lives as long as the kernel; 0 if unknown */
    float tail_fraction;          /* share of sdf_evals done in latency mode (one ray per wave, FT_OPT_TAIL_K) */
} ft_stats;

/* ---- context ------------------------------------------------------------------------ */
/* device >= 0: HIP device ordinal.  device = -1: host-only context (scene construction and
 * ft_scene_export work; anything that needs the GPU fails with FT_ERR_NO_DEVICE). */
int ft_abi_version(void);
int ft_ctx_create(int device, ft_ctx** out);
void ft_ctx_destroy(ft_ctx* ctx);
const char* ft_last_error(void);
/* use an existing HIP stream (e.g. torch's current stream) for all launches; NULL = own stream */
int ft_ctx_set_stream(ft_ctx* ctx, void* hip_stream);
/* "src=<hash>;kind=<product|profile|experiment>": hash of the sources this library was built from
 * (fraytracer_amd/csrc/source_hash.py computes the same value from a source tree) and the kind of build. */
const char* ft_build_info(void);
/* Per-context switches (the library reads no environment variables).  FT_OPT_MATH selects the arithmetic of MathF.Exp / Log / Pow
 * (below); every other option is for experiments and A/B measurements only and never changes a rendered bit. */
typedef enum ft_option {
    FT_OPT_REFILL_MIN = 1,        /* 1..64 (default 64): idle lanes a wave waits for before it takes new rays */
    FT_OPT_MAX_BLOCKS_PER_CU = 2, /* 0 (default) = the occupancy limit; 1..8 caps the resident workgroups per CU */
    FT_OPT_HOST_CHUNKS = 3,       /* 0 (default) = automatic; 1..16 column chunks of ft_render's host-output pipeline */
    FT_OPT_HOST_PIN = 4,          /* 1 (default): ft_render page-locks an unregistered destination for the call; 0: leaves it pageable */
    FT_OPT_TAIL_K = 5,            /* latency mode: a wave holding at most this many rays evaluates them one at a time with all 64 lanes;
                                   * -1 (default) = the kernel's own threshold, 0 = off, 1..64 */
    FT_OPT_MATH = 6,              /* ft_math_mode (below); default FT_MATH_FIXED */
    FT_OPT_CHUNK = 8,             /* 64 (default): rays a wave takes per grab = one 8x8 tile; 32 / 16: half / quarter tiles (experiments) */
    FT_OPT_CULL = 9,              /* 1 (default): the smooth-union kernel drops, per wave and round, the children whose terms are below half an ulp
                                   * of the running sum in every ray of the wave (exact: the sum is unchanged bit for bit); 0: every child, every round */
    FT_OPT_ESCAPE = 10,           /* 1 (default): a ray that can no longer come within epsilon of the scene's support sphere — outside it and heading away, or
                                   * passing it by — ends as the miss its march is bound to end in, without further evaluations (same frame, fewer sdf_evals);
                                   * 0: every ray marches until its Length is used up, as the reference does */
    FT_OPT_LAZY_UNION = 11,       /* 1 (default): SdfForm.union as the first child of an intersect (the reference's own scene: intersect(union of tori, sphere))
                                   * stops its candidate walk at Items.[0] wherever that distance is already <= the next child's, which then decides the
                                   * intersect's value (exact; only where no hit is possible); 0: every union walk runs to its end */
    FT_OPT_CARVED = 12,           /* 1 (default): a scene that is one SdfForm.union of primitives followed by at most two single-primitive intersect / subtract
                                   * steps — the reference's own subtract(intersect(union tori, sphere), sphere) — is traced by a kernel specialised for that
                                   * shape (registers instead of LDS value slots, no interpreter, the tail decides early exits of the walk; same bits);
                                   * 0: the general interpreter kernel */
    FT_OPT_REUSE = 13,            /* 1 (default): every shadow ray (and EXTENSION ambient-occlusion ray) starts at the hit position, where the fourth probe of SdfForm.normal
                                   * has just evaluated the scene (SdfForm.fs:112, SdfObject.fs:73: the same point, bit for bit); the first evaluation of its march is
                                   * that value and is not computed again; likewise every primary ray of ft_render starts at the camera position, which each wave evaluates
                                   * once (same frame, same ray and hit counters, fewer sdf_evals); 0: evaluated once per ray, as the reference does */
    FT_OPT_CERT = 14,             /* 1 (default): the smooth-union-of-spheres kernel ends a ray as a miss once a bound over the rest of its line proves that no later
                                   * evaluation can come below epsilon (exact: same frame, counters and flags, fewer sdf_evals); only while FT_OPT_ESCAPE is on; 0: off */
    FT_OPT_CERT_POLICY = 15,      /* 0 (default policy) or, for experiments, when the miss certificate is tried: bits 0-7 the primary ray's step (255: never),
                                   * 8-15 the shadow ray's step (255: never), 16-23 the due lanes a wave waits for (1 .. 64), 24-29 steps to the next try (0: once), 30-31 the
                                   * bundle certificate (one test per wave for all its primary, then all its shadow rays): 0 the shipped schedule, 1 every evaluation round
                                   * from one ray on, 2 every second round (shadow rays from their 2nd step), 3 off.  255 / 255 in bits 0-15: the bundle alone.
                                   * Word 0 = 0 | 6 << 8 | 16 << 16 | 6 << 24 with the shipped bundle schedule, except that a camera frame (ft_render and its hits form) whose 8x8 pixel tiles are at most
                                   * the certificate's margin wide at the far side of the scene's support sphere gets the bundle alone (255 / 255): an explicit word is always taken as it stands */
    FT_OPT_ORDER = 16,            /* 1 (default): a frame (ft_render_device and the entry points built on it; the reference's sampling, whole 8x8 tiles) records per tile how many
                                   * evaluation rounds it took, and the scene's next frame of the same size, column range and stripe layout on the same render lane hands out first
                                   * the tiles that cost at least the mean, most expensive first, so that no long tile starts late and the frame's drain shortens; the other
                                   * tiles keep their index order.  Only when a tile starts changes: same frame, counters and flags.  The camera, epsilon, Length and the
                                   * lights may differ between the two frames (a stale order is only another order); a first frame runs in index order.  2: record only;
                                   * 0: off.  Not combined with FT_OPT_GUIDED = 1, which stays in index order */
    FT_OPT_OCCL = 17,             /* 1 (default): the smooth-union-of-spheres kernel ends a shadow ray as the hit its march is bound to end in once its line is proved to pass
                                   * deep enough through one of the spheres (exact: same frame, counters and flags, fewer sdf_evals); only while FT_OPT_ESCAPE and FT_OPT_CERT are on; rays of
                                   * |direction| > 1 (a point light's) and EXTENSION ambient-occlusion rays keep marching; 0: off */
    FT_OPT_OCCL_POLICY = 18,      /* 0 (default schedule) or, for experiments, when that proof is tried: bits 0-7 every how many evaluation rounds of a wave (0: the shipped 2,
                                   * 1: every round, 255: off), 8-15 the steps a shadow ray takes first, 16-23 the shadow rays a try waits for (0: the shipped 1; .. 64) */
    FT_OPT_TRY_HINT = 19,         /* 1 (default): a frame of the smooth-union-of-spheres kernel (the launches FT_OPT_ORDER covers) records per 8x8 tile on which of the tile's evaluation
                                   * rounds the bundle certificate of its primary rays and that of its shadow rays first held, and the scene's next frame of the same size, column range and
                                   * stripe layout on the same render lane tries each tile's bundles around those rounds instead of on every second round of the wave.  Only when a
                                   * try runs changes: same frame, rays, hits and flags; sdf_evals and wave_evals fall.  Followed only under FT_OPT_CERT_POLICY = 0 on frames that word
                                   * gives the bundle alone, and from a camera whose image moved by at most 16 pixels since the frame that recorded; a first frame, an explicit policy
                                   * word and every other launch keep their schedule.  2: record only; 0: off */
    FT_OPT_DEPART = 20,           /* 1 (default): on the frames that follow try hints (FT_OPT_TRY_HINT above) the smooth-union-of-spheres kernel tries each shadow ray's miss certificate where
                                   * the ray is born, under a margin that starts near zero and grows along the ray with the steps a march could take; a lit shadow ray then ends at
                                   * birth instead of creeping away from the surface it left.  Exact: same frame, rays, hits and flags; sdf_evals and wave_evals fall.  A first
                                   * frame, a wide-tiled frame, an explicit FT_OPT_CERT_POLICY word, views, ray buffers and EXTENSION launches count exactly what they counted.
                                   * 2: on every camera launch of that kernel family (tests); 0: off.  Only while FT_OPT_ESCAPE and FT_OPT_CERT are on */
    FT_OPT_GUIDED = 7             /* 1: the last jobs of a launch are handed out in half and quarter tiles (lean kernel); 0 (default): whole tiles only */
} ft_option;
/* MathF.Exp / MathF.Log (SdfForm.unionSmooth, SdfForm.fs:80,82) and MathF.Pow (FColor.gammaInverse, FColor.fs:50-55) are the C runtime's
 * expf / logf / powf under .NET: platform arithmetic, not one fixed function.
 *   FT_MATH_FIXED       one fixed algorithm per function (IEEE + - * / fma only): the same bits on every machine; <= 0.93 ulp (exp),
 *                       < 0.51 ulp (log), correctly rounded pow except at ~1e-7 of the operands.
 *   FT_MATH_GLIBC_FMA   glibc 2.35's expf / logf / powf as its x86-64 FMA build computes them (`__expf_fma` ...: the variant glibc's ifunc
 *                       selects on every CPU with FMA and AVX2) — bit for bit what the reference's CPU path returns on such a Linux host.
 *   FT_MATH_GLIBC_SSE2  the same functions as glibc's SSE2 build rounds them (x86-64 CPUs without FMA / AVX2).
 * Both glibc modes are restatements running on the GPU (csrc/ft_libm.h), proved against the running libm over all 2^32 inputs
 * (ft_selftest_libm).  Scenes without a unionSmooth trace identically in every mode. */
typedef enum ft_math_mode { FT_MATH_FIXED = 0, FT_MATH_GLIBC_FMA = 1, FT_MATH_GLIBC_SSE2 = 2 } ft_math_mode;
int ft_ctx_set_option(ft_ctx* ctx, int32_t option, int32_t value);
int ft_ctx_get_option(const ft_ctx* ctx, int32_t option, int32_t* value);

/* ---- scene construction: one entry per reference constructor ---------------------------- */
ft_handle ft_form_sphere(ft_ctx*, const ft_sphere*);                       /* SdfForm.Primitive.sphere  SdfForm.fs:125-135 */
ft_handle ft_form_capsule(ft_ctx*, const ft_capsule*);                     /* SdfForm.Primitive.capsule SdfForm.fs:145-170 */
ft_handle ft_form_torus(ft_ctx*, const ft_torus*);                         /* SdfForm.Primitive.torus   SdfForm.fs:181-203 */
ft_handle ft_form_triangle(ft_ctx*, const ft_triangle*);                   /* SdfForm.Primitive.triangle SdfForm.fs:214-268 */
ft_handle ft_form_box(ft_ctx*, const ft_box*);                             /* EXTENSION */
ft_handle ft_form_union(ft_ctx*, const ft_handle* forms, int32_t n);       /* SdfForm.union        SdfForm.fs:14-40 */
ft_handle ft_form_subtract(ft_ctx*, ft_handle a, ft_handle b);             /* SdfForm.subtract     SdfForm.fs:42-49 */
ft_handle ft_form_intersect(ft_ctx*, const ft_handle* forms, int32_t n);   /* SdfForm.intersect    SdfForm.fs:51-67 */
ft_handle ft_form_union_smooth(ft_ctx*, float strength, const ft_handle* forms, int32_t n); /* SdfForm.unionSmooth SdfForm.fs:69-91 */
int ft_form_boundary(ft_ctx*, ft_handle form, ft_boundary* out);           /* SdfForm.Boundary */

ft_handle ft_material_solid(ft_ctx*, const float rgb[3]);                  /* SdfMaterial.createSolid SdfMaterial.fs:4-7 */
/* EXTENSION (BASELINE.json config 5; the reference's SdfMaterial cannot spawn rays, Types.fs:46-49): glass with
 * index of refraction `ior` at 550 nm and Cauchy dispersion n(lambda) = ior + dispersion * (1/lambda_um^2 - 1/0.55^2).
 * Fresnel terms follow the reference's dead Light.fs:30-59 (repaired). */
ft_handle ft_material_glass(ft_ctx*, const float tint[3], float ior, float dispersion);
/* EXTENSION: the wavelength table behind ft_render_params.spectral = nw: out[nw][4] = RGB weight, Cauchy term */
int ft_spectral_table(int32_t nw, float* out);
ft_handle ft_object_create(ft_ctx*, ft_handle material, ft_handle form);   /* SdfObject.create    SdfObject.fs:6-10 */
ft_handle ft_object_union(ft_ctx*, const ft_handle* objects, int32_t n);   /* SdfObject.union     SdfObject.fs:12-48 */
ft_handle ft_object_subtract(ft_ctx*, ft_handle object, ft_handle form);   /* SdfObject.subtract  SdfObject.fs:50-54 */
ft_handle ft_object_intersect(ft_ctx*, ft_handle object, const ft_handle* forms, int32_t n); /* SdfObject.intersect SdfObject.fs:56-64 */
ft_handle ft_object_form(ft_ctx*, ft_handle object);                       /* object.Form */

ft_handle ft_light_directional(ft_ctx*, const float direction[3], const float rgb[3]);  /* SdfLight.directional SdfLight.fs:6-21 */
ft_handle ft_light_point(ft_ctx*, const float position[3], const float rgb[3]);         /* SdfLight.point       SdfLight.fs:23-42 */

/* SdfScene record (Types.fs:74-79): flattens the immutable tree and uploads it. */
int ft_scene_create(ft_ctx*, ft_handle object, const float background_rgb[3],
                    const ft_handle* lights, int32_t n_lights, ft_scene** out);
void ft_scene_destroy(ft_scene*);
/* A scene with src's Object — its flattened program, grids, support sphere, certificate clusters: shared work, not redone —
 * under another background and other lights.  Equal in every uploaded byte to ft_scene_create(object, background, lights); no flatten and
 * no grid build runs.  The light handles belong to src's context, which the new scene belongs to as well (a host-only context works);
 * src may be destroyed afterwards.  NULL, a negative count or a handle that is no light of that context: FT_ERR_INVALID. */
int ft_scene_relight(const ft_scene* src, const float background_rgb[3], const ft_handle* lights, int32_t n_lights, ft_scene** out);

/* Lens.create (Camera.fs:11-14) and Camera.lookAt (Camera.fs:33-42); host-side, once per frame. */
float ft_lens_create(float field_of_view);
int ft_camera_look_at(const float position[3], const float look_at[3], const float up[3],
                      float near_plane_size, ft_camera* out);

/* ---- the hot path --------------------------------------------------------------------- */
/* Image.render epsilon length imageSize camera (SdfScene.trace scene)  — Image.fs:26-35 +
 * SdfScene.fs:7-28.  Synchronous.  `out` is host memory (pinned or pageable; a pageable buffer is page-locked for the
 * duration of the call while the GPU renders, and the frame is copied chunk by chunk behind the rendering). */
int ft_render(ft_ctx*, const ft_scene*, const ft_camera*, const ft_render_params*,
              float* out, ft_stats* stats);
/* Page-lock a host buffer the caller reuses as ft_render's `out` (the F# side pins its FColor[,] with GCHandle, as
 * Image.fs:77-86 does for the bitmap): the frame is then written by DMA at link rate without the per-call pinning
 * ft_render otherwise does itself.  Unregister before freeing the buffer. */
int ft_host_register(ft_ctx*, void* p, uint64_t bytes);
int ft_host_unregister(ft_ctx*, void* p);
/* Same, output left in device memory `d_out`, launched on the context's stream and NOT
 * synchronised: for callers that keep the frame in HBM (multi-GPU gather, bench). */
int ft_render_device(ft_ctx*, const ft_scene*, const ft_camera*, const ft_render_params*,
                     void* d_out);
/* counters / kernel time of the launches since the last call; synchronises the stream */
int ft_collect_stats(ft_ctx*, ft_stats* stats);
/* EXTENSION: per-pixel SdfObject.tryTrace scene.Object of the reference's pixel ray (sample 0), laid out like the frame
 * (n_columns x height, y contiguous).  out_rgb NULL = hits only (no lighting, no shadow / AO / glass rays).
 * out_hits: ft_object_trace_result per pixel, exactly what ft_object_try_trace returns for that ray (miss = all zero).
 * out_material: material handle (ft_material_solid / ft_material_glass) the hit picked, -1 on a miss.
 * Any of the three may be NULL, not all.  With out_rgb the image and the statistics are those of ft_render with the same
 * parameters (any spp / ao_samples / max_bounces / spectral; the records describe the first segment of sample 0, before any
 * glass bounce); without it one ray is traced per pixel and the EXTENSION fields of the parameters do not apply.
 * The host form renders the whole frame before it copies out: 64 B of device scratch per pixel for the records. */
int ft_render_hits(ft_ctx*, const ft_scene*, const ft_camera*, const ft_render_params*,
                   float* out_rgb, ft_object_trace_result* out_hits, int32_t* out_material, ft_stats* stats);
/* Same into device memory, asynchronous like ft_render_device (pair with ft_collect_stats); d_hits 16-byte aligned. */
int ft_render_hits_device(ft_ctx*, const ft_scene*, const ft_camera*, const ft_render_params*,
                          void* d_out_rgb, void* d_hits, void* d_material);
/* n_views cameras (host memory; the library uploads them), one scene, one set of render params: out = n_views x n_columns x height x 3
 * float32, view-major; block k is bit for bit what ft_render(ctx, scene, &cameras[k], params, ...) writes, every field of the params applied
 * to each view.  One job queue covers the views, so one launch pays one drain for all of them (batches of more than 64 views take one launch
 * per 64).  stats: one ft_stats for the batch — each count the sum of the single-view calls' counts.  FT_ERR_UNSUPPORTED when
 * n_views x spp x tiles x 64 reaches 2^32.  n_views = 1 is exactly ft_render.  The host form renders the batch into device scratch and copies
 * it out once (a pageable destination is page-locked for the call, like ft_render's). */
int ft_render_views(ft_ctx*, const ft_scene*, const ft_camera* cameras, int32_t n_views,
                    const ft_render_params*, float* out, ft_stats* stats);
/* Same into device memory, asynchronous like ft_render_device (pair with ft_collect_stats).  n_views = 1 is exactly ft_render_device. */
int ft_render_views_device(ft_ctx*, const ft_scene*, const ft_camera* cameras, int32_t n_views,
                           const ft_render_params*, void* d_out);
/* EXTENSION: ft_render_hits for a batch of views, in the job queues of ft_render_views.  Every buffer is view-major: n_views x n_columns x
 * height x 3 float32 for out_rgb, one ft_object_trace_result per pixel for out_hits, one int32 per pixel for out_material; block k of each is
 * bit for bit what ft_render_hits(ctx, scene, &cameras[k], params, ...) writes.  Any of the three may be NULL, not all: with out_rgb alone
 * the call is ft_render_views; without out_rgb one ray is traced per pixel per view and the EXTENSION fields of the params do not apply
 * (the 2^32 job limit then counts one sample a view).  stats: the sums of the single-view calls' counts.  n_views = 1 is exactly
 * ft_render_hits.  The host form stages one launch group (up to 64 views) at a time in device scratch and copies it out before the next. */
int ft_render_views_hits(ft_ctx*, const ft_scene*, const ft_camera* cameras, int32_t n_views, const ft_render_params*,
                         float* out_rgb, ft_object_trace_result* out_hits, int32_t* out_material, ft_stats* stats);
/* Same into device memory, asynchronous like ft_render_device (pair with ft_collect_stats); d_hits 16-byte aligned, d_out_rgb and
 * d_material 4-byte aligned.  n_views = 1 is exactly ft_render_hits_device. */
int ft_render_views_hits_device(ft_ctx*, const ft_scene*, const ft_camera* cameras, int32_t n_views, const ft_render_params*,
                                void* d_out_rgb, void* d_hits, void* d_material);

/* ---- around the hot path: tone map + 8-bit output -------------------------------- */
/* Image.toColors gamma rng image (Image.fs:37-50): max = Max(0.01, max over all channels); per channel
 * Pow(c / max, 1 / gamma) * 254.5 + u, rounded half-to-even, `min 255` (FColor.fs:43-55).  The reference draws u from one
 * System.Random shared by a parallel map (racy, not reproducible): here u is 0.5 (dither = 0) or a counter-based hash of
 * (x, y, channel, seed) in [0, 1) (dither = 1) — comparable to the reference to +-1 LSB.  MathF.Pow is platform libm;
 * the library uses one fixed double-precision algorithm (ft_math.h ft_pow) shared with the test oracle.
 * bmp_order = 0: out[(x * Y + y) * 3 + k] = R, G, B of image[x, y] — the Color[X,Y] value of Image.toColors.
 * bmp_order = 1: the scan0 buffer Image.toBitmap builds (Image.fs:61-86): row r from the top, column c holds
 *                image[X-1-c, r] as bytes B, G, R, stride X * 3 — ready for a 24-bpp bitmap. */
typedef struct ft_tonemap_params {
    float gamma;                  /* Image.toColors' gamma (Program.fs:98 passes 2.2f) */
    int32_t dither;               /* 0: u = 0.5 everywhere; 1: hashed noise */
    uint32_t seed;
    int32_t bmp_order;
} ft_tonemap_params;
/* frame in device memory (X x Y x 3 float32 as ft_render_device writes it) -> 8-bit image in device memory; asynchronous
 * on the context's stream */
int ft_tone_map_device(ft_ctx*, const void* d_frame, int32_t X, int32_t Y, const ft_tonemap_params*, void* d_out);
/* same, 8-bit image copied to host memory (3 bytes per pixel cross PCIe instead of 12); *max_out = the normalisation */
int ft_tone_map(ft_ctx*, const void* d_frame, int32_t X, int32_t Y, const ft_tonemap_params*, uint8_t* out, float* max_out);
/* Image.toColors on a host FColor[X,Y] (drop-in for the reference call on an image that is already on the host) */
int ft_tone_map_host(ft_ctx*, const float* frame, int32_t X, int32_t Y, const ft_tonemap_params*, uint8_t* out, float* max_out);
/* Program.fs:90-100 in one call: Image.render + Image.toColors (+ toBitmap order) on the device; only the 8-bit image
 * leaves the GPU.  The render parameters must describe the whole frame. */
int ft_render_colors(ft_ctx*, const ft_scene*, const ft_camera*, const ft_render_params*, const ft_tonemap_params*,
                     uint8_t* out, float* max_out, ft_stats* stats);

/* SdfScene.trace over an explicit ray buffer (the "ray buffer" form): out_rgb is n x 3 floats. */
int ft_trace_rays(ft_ctx*, const ft_scene*, const ft_ray* rays, int64_t n, float* out_rgb, ft_stats* stats);

/* SdfForm.tryTrace scene.Object.Form ray (SdfForm.fs:93-104) over a ray buffer: the ray as it stands at the hit
 * (Origin moved, Length reduced) and the last Distance. */
int ft_form_try_trace(ft_ctx*, const ft_scene*, const ft_ray* rays, int64_t n, ft_form_trace_result* out, ft_stats* stats);
/* SdfObject.tryTrace scene.Object ray (SdfObject.fs:66-78) over a ray buffer: march, normalFromRay, Ray.move -eps,
 * material colour picked at the un-pulled hit origin. */
int ft_object_try_trace(ft_ctx*, const ft_scene*, const ft_ray* rays, int64_t n, ft_object_trace_result* out, ft_stats* stats);
/* The three above with rays and results in device memory: the kernel reads d_rays (n x ft_ray, 32 B each) and writes the caller's buffers.
 * No device scratch, no copy; launched on the context's stream and NOT synchronised (pair with ft_collect_stats), like ft_render_device.
 * d_rays and the ft_object_trace_result records (d_out of the object form) must be 16-byte aligned — a lane loads its ray as two 16-byte
 * words —, every other buffer 4-byte aligned; a misaligned buffer, or NULL where none is allowed, is FT_ERR_INVALID and nothing is launched.
 * n = 0: FT_OK, nothing launched.  n >= 0xFFFF0000: FT_ERR_UNSUPPORTED.  Input and output must not overlap (only identical pointers
 * are detected: FT_ERR_INVALID).  ft_object_try_trace_device: d_material, if not NULL, receives per ray the handle of the ft_material_* the
 * hit picked, -1 on a miss (n x int32) — the rule of ft_render_hits; with d_material = NULL it is exactly ft_object_try_trace. */
int ft_trace_rays_device(ft_ctx*, const ft_scene*, const void* d_rays, int64_t n, void* d_out_rgb);
int ft_form_try_trace_device(ft_ctx*, const ft_scene*, const void* d_rays, int64_t n, void* d_out);
int ft_object_try_trace_device(ft_ctx*, const ft_scene*, const void* d_rays, int64_t n, void* d_out, void* d_material);
/* EXTENSION: SdfScene.trace and SdfObject.tryTrace of every ray of a ray buffer in ONE launch — ft_render_hits for explicit rays.  Ray i:
 * out_rgb[i] = what ft_trace_rays writes; out_hits[i] = what ft_object_try_trace writes (a miss is all zero); out_material[i] = handle of the
 * ft_material_* the hit picked, -1 on a miss.  Any of the three may be NULL, not all.  With out_rgb the counters are those of ft_trace_rays
 * on the same rays (with out_rgb alone the call is ft_trace_rays); without it no lighting and no shadow rays are traced and the counters
 * are those of ft_object_try_trace.  There are no render params: a glass material shades as its solid tint, as in ft_trace_rays.
 * The host form stages rays and results in device scratch (32 B + up to 80 B per ray). */
int ft_trace_rays_hits(ft_ctx*, const ft_scene*, const ft_ray* rays, int64_t n,
                       float* out_rgb, ft_object_trace_result* out_hits, int32_t* out_material, ft_stats* stats);
/* Same in device memory, under the contract of the *_device forms above: d_rays and d_hits 16-byte aligned, d_out_rgb and d_material
 * 4-byte aligned; no scratch, no copy, not synchronised. */
int ft_trace_rays_hits_device(ft_ctx*, const ft_scene*, const void* d_rays, int64_t n,
                              void* d_out_rgb, void* d_hits, void* d_material);

/* Relighting without re-tracing.  SdfScene.trace from its `| ValueSome result ->` arm on (SdfScene.fs:11-28) over n records:
 * out_rgb[i] = scene.BackgroundColor where hits[i].hit == 0, else result.Color * (lightColor * piInv) with one shadow ray per light whose
 * lightCos > 0, cast from hits[i].ray.origin with hits[i].ray.epsilon through scene.Object (SdfLight.fs:10-20, 26-41).  For scenes A and B
 * that share their Object (ft_scene_relight), shading under B the records ft_object_try_trace / ft_render_hits / ft_trace_rays_hits wrote
 * under A gives bit for bit what ft_trace_rays / ft_render give under B.  Records are data: colour, normal, origin and epsilon are used as
 * they stand (a caller may recolour or filter them); a record with hit == 0 is background whatever else it holds.  There are no render
 * params: a glass material's record carries its tint and shades as a solid, as in ft_trace_rays.
 * Counters: rays_primary, hits_primary and rays_ext are 0; rays_shadow and hits_shadow are what ft_trace_rays reports for the rays that made
 * the records; flags come from the shadow marches only.  sdf_evals counts the shadow marches' evaluations: no normal probe ran here, so a
 * shadow ray's first evaluation (at the hit position) is computed, as with FT_OPT_REUSE = 0, whatever that option says.
 * The host form stages 64 B + 12 B per record in device scratch.  Arguments are checked before the device is asked for. */
int ft_shade_hits(ft_ctx*, const ft_scene*, const ft_object_trace_result* hits, int64_t n, float* out_rgb, ft_stats* stats);
/* Same in device memory, under the contract of the *_device forms above: d_hits 16-byte aligned (a lane loads its record as four 16-byte
 * words), d_out_rgb 4-byte aligned; no scratch, no copy, launched on the context's stream and not synchronised (pair with ft_collect_stats).
 * n = 0: FT_OK, nothing launched.  n >= 0xFFFF0000: FT_ERR_UNSUPPORTED.  Input and output must not overlap (only identical pointers are
 * detected: FT_ERR_INVALID). */
int ft_shade_hits_device(ft_ctx*, const ft_scene*, const void* d_hits, int64_t n, void* d_out_rgb);

/* Light visibility masks: the shadow marches of ft_shade_hits kept as one bit per (record, light), and shading from those bits with no march.
 * A shadow march yields one bit — does `light.Intensity scene.Object ray` return ValueSome or ValueNone (SdfLight.fs:17-20, 38-41) — which
 * depends on scene.Object, the record and the light's direction or position, and on no colour: it stays what it is when lights are dimmed
 * or recoloured, the background changes or records are recoloured, and when one light moves only that light's bit changes.
 *
 * ft_light_visibility.  Let L = n_lights of the scene and sel = select & (2^L - 1); select = 0xFFFFFFFF: every light.  Bit i of record r's
 * new bits is set iff i is in sel, hits[r].hit != 0, lightCos > 0 (SdfScene.fs:15-17) and the shadow ray of light i cast from the record
 * missed, i.e. exactly where SdfScene.fs:23 executes; the ray is cast from hits[r].ray.origin with hits[r].ray.epsilon, as ft_shade_hits
 * casts it.  vis_out[r] = (vis_in ? vis_in[r] & ~sel & (2^L - 1) : 0) | new bits: bits >= L are always 0.  vis_in may be NULL and may
 * equal vis_out (update in place).  Lights outside sel are skipped: no cosine is formed, no ray is cast, none is counted; sel == 0 returns
 * the kept bits.  Counters: rays_primary, hits_primary and rays_ext are 0; rays_shadow, hits_shadow, sdf_evals and flags are those of the
 * marches that ran — with every light selected, rays_shadow, hits_shadow and flags are ft_shade_hits' on the same records, and so is
 * sdf_evals with FT_OPT_CERT = 0 (how many evaluations the miss certificate saves is not part of the contract).
 * The host form stages 64 B + 4 B (+ 4 B with vis_in) per record in device scratch.  Arguments are checked before the device is asked for:
 * NULL ctx, scene, hits or vis_out, n < 0, hits == vis_out: FT_ERR_INVALID; n = 0: FT_OK, nothing launched; n >= 0xFFFF0000 or a scene
 * with more than 32 lights: FT_ERR_UNSUPPORTED. */
int ft_light_visibility(ft_ctx*, const ft_scene*, const ft_object_trace_result* hits, int64_t n,
                        uint32_t select, const uint32_t* vis_in, uint32_t* vis_out, ft_stats* stats);
/* Same in device memory, under the contract of ft_shade_hits_device: d_hits 16-byte aligned, the masks 4-byte aligned (else FT_ERR_INVALID);
 * no scratch, no copy, launched on the context's stream and not synchronised (pair with ft_collect_stats). */
int ft_light_visibility_device(ft_ctx*, const ft_scene*, const void* d_hits, int64_t n,
                               uint32_t select, const void* d_vis_in, void* d_vis_out);
/* ft_shade_visible.  out_rgb[r] = scene.BackgroundColor where hits[r].hit == 0 (SdfScene.fs:10).  Otherwise lightColor = BackgroundColor
 * (SdfScene.fs:12), then for i = 0 .. L - 1 in order: if bit i of visibility[r] is set, lightColor += intensity_i * lightCos_i (SdfScene.fs:15,
 * 23) with a directional light's direction and colour as they stand (SdfLight.fs:9, 16) and a point light's normalize(position - origin) and
 * colour / length2(position - origin) (SdfLight.fs:25, 28, 40); at last result.Color * (lightColor * piInv) (SdfScene.fs:28).  The operations,
 * operands and order are those of the tracing kernels, so that for scenes that share their Object, bit for bit:
 *   (a) shade_visible(B, rec, light_visibility(B, rec, all)) = ft_shade_hits(B, rec) = ft_trace_rays(B, rays);
 *   (b) for B' with B's lights in the same order at the same directions and positions, but other colours, another background or recoloured
 *       records rec': shade_visible(B', rec', light_visibility(B, rec)) = ft_trace_rays(B', rays);
 *   (c) for B2 = B with light j moved: light_visibility(B2, rec, 1 << j, vis_in = light_visibility(B, rec)) = light_visibility(B2, rec, all).
 * A mask is data, as records are: a set bit contributes even where the cosine is <= 0; bits >= L are ignored.  No march runs: every counter
 * is 0, kernel_ms is filled.  The host form stages 64 B + 4 B + 12 B per record.  Refusals as above, with visibility and out_rgb for vis_out;
 * visibility == out_rgb: FT_ERR_INVALID. */
int ft_shade_visible(ft_ctx*, const ft_scene*, const ft_object_trace_result* hits, const uint32_t* visibility,
                     int64_t n, float* out_rgb, ft_stats* stats);
/* Same in device memory: d_hits 16-byte aligned, masks and colours 4-byte aligned; a streaming kernel on the context's stream. */
int ft_shade_visible_device(ft_ctx*, const ft_scene*, const void* d_hits, const void* d_visibility,
                            int64_t n, void* d_out_rgb);

/* scene.Object.Form.Distance at n points (+ index of the material the hit would pick, or
 * NULL).  Test/diagnostic entry: lets parity tests compare single SDF evaluations. */
int ft_eval_distance(ft_ctx*, const ft_scene*, const ft_vec3* points, int64_t n, float* out_distance, int32_t* out_material);

/* Field sampling: the distance field itself, on the device — scene.Object.Form.Distance, SdfForm.normal and the material of
 * object.Material.Color at the points of a regular lattice or of a point buffer (SdfForm.fs:7-12, 106-112; SdfObject.fs:23-46).
 *
 * Lattice point (i, j, k), 0 <= i < nx, 0 <= j < ny, 0 <= k < nz, is
 *     (origin.x + (float)i * step.x, origin.y + (float)j * step.y, origin.z + (float)k * step.z):
 * per coordinate one float32 product, rounded, then one float32 sum, rounded — never a fused multiply-add.  Its results sit at index
 * (i * ny + j) * nz + k of every output, so k is contiguous.  Each count is 1 .. 16777216 (so that (float)i is exact); a step may be
 * zero or negative.  A point buffer is n x ft_vec3, 12 bytes apart; point r's results sit at index r.
 * Distance: sdf.Distance p — the bits ft_eval_distance gives for the same point.
 * Normal (asked for with out_normal): SdfForm.normal sdf normal_epsilon p, i.e. four evaluations in the order
 *     dx = D(p.x + e, p.y, p.z), dy = D(p.x, p.y + e, p.z), dz = D(p.x, p.y, p.z + e), d = D(p);
 *     g = (dx, dy, dz) - (d, d, d);  n = g / sqrt((g.x * g.x + g.y * g.y) + g.z * g.z), three true divisions;
 * NaN where the reference gives NaN (g = 0, an infinite distance).  The distance written is the centre evaluation d: the same bits
 * with or without the normal.  normal_epsilon is read only when a normal is asked for.
 * Material: the handle of the ft_material_* that object.Material.Color p picks — the argmin of SdfObject.union, the first object's
 * material under subtract and intersect; the rule of ft_object_try_trace_device's d_material.  There is no miss here: it is always a
 * handle (-1 only for an object without a material).
 * flags: FT_FIELD_BOUNDED is SdfForm.tryDistance: a point is evaluated only where SdfBoundary.isInside scene.Object.Form.Boundary p,
 * i.e. (dx * dx + dy * dy) + dz * dz < Radius * Radius with d = p - Boundary.Center in float32; elsewhere nothing is evaluated, distance
 * and normal are NaN and the material is -1.
 * Any output may be NULL, but not all three.  There are no ft_stats: NaN and infinity are in the outputs themselves.
 * Refusals, all made before the device is asked for: FT_ERR_INVALID for NULL where none is allowed, n < 0, a count < 1 or > 16777216,
 * unknown flag bits, a misaligned device buffer, identical pointers; FT_ERR_UNSUPPORTED for n or nx * ny * nz >= 0xFFFF0000 (and for a
 * scene whose LDS footprint no kernel fits); n = 0: FT_OK, nothing launched; then FT_ERR_NO_DEVICE on a host-only context.
 * The host forms stage through the context's scratch (12 B per point of a point buffer — the lattice form uploads nothing — and 4 + 12
 * + 4 B per point for the outputs asked for) and synchronise.
 * FT_OPT_CULL, FT_OPT_CARVED, FT_OPT_LAZY_UNION and FT_OPT_MAX_BLOCKS_PER_CU apply as to a trace launch and never change an output bit. */
typedef struct ft_lattice { ft_vec3 origin; ft_vec3 step; int32_t nx, ny, nz; } ft_lattice;   /* 36 B */
int ft_sample_points(ft_ctx*, const ft_scene*, const ft_vec3* points, int64_t n, float normal_epsilon, uint32_t flags,
                     float* out_distance, ft_vec3* out_normal, int32_t* out_material);
int ft_sample_lattice(ft_ctx*, const ft_scene*, const ft_lattice*, float normal_epsilon, uint32_t flags,
                      float* out_distance, ft_vec3* out_normal, int32_t* out_material);
/* The same in device memory, under the contract of the other *_device forms: launched on the context's stream and NOT synchronised, no
 * scratch, no copy.  Every buffer 4-byte aligned (points are 12 B apart; d_normal is n x 3 float32, d_material n x int32).  Input and
 * output must not overlap: only identical pointers are detected (FT_ERR_INVALID). */
int ft_sample_points_device(ft_ctx*, const ft_scene*, const void* d_points, int64_t n, float normal_epsilon, uint32_t flags,
                            void* d_distance, void* d_normal, void* d_material);
int ft_sample_lattice_device(ft_ctx*, const ft_scene*, const ft_lattice*, float normal_epsilon, uint32_t flags,
                             void* d_distance, void* d_normal, void* d_material);

/* Meshing: the surface {distance = iso} of a lattice of distances as triangles, extracted on the device — marching tetrahedra on the Kuhn
 * subdivision of every lattice cell.  The result is a pure function of the lattice's values; this is the rule, every bit of it.
 *
 * Input: a lattice (ft_lattice above: point rule p(q), index (i * ny + j) * nz + k), a float32 value d[q] per lattice point and a level iso.
 * Signed value: s[q] = d[q] - iso, one float32 subtraction.  Point q is inside iff s[q] < 0: +0, -0 and NaN are not inside.
 * Edge directions: seven, (di, dj, dk) with e = 4 * di + 2 * dj + dk - 1, i.e. 0 (0,0,1), 1 (0,1,0), 2 (0,1,1), 3 (1,0,0), 4 (1,0,1),
 *     5 (1,1,0), 6 (1,1,1).  Edge (q, e) joins q and q' = q + dir(e), exists where both ends are lattice points, and is owned by q.
 * Vertices: edge (q, e) carries a vertex iff s[q] and s[q'] are both finite and exactly one end is inside.  Its position, per coordinate in
 *     float32 with every operation rounded on its own, never a fused multiply-add:
 *         t = s[q] / (s[q] - s[q']), one true division;  v = p(q) + t * (p(q') - p(q)),
 *     always computed from the owner towards the far end, once, and shared by every triangle that uses it.  Vertices are numbered by the
 *     owner's linear index (i * ny + j) * nz + k, then by e.
 * Tetrahedra: cell (i, j, k), 0 <= i < nx - 1 and likewise j, k, is cut into six, one per permutation pi of the axes (i, j, k) in
 *     lexicographic order, with the corners c0 = (i, j, k), c1 = c0 + unit(pi1), c2 = c1 + unit(pi2), c3 = (i + 1, j + 1, k + 1); all their
 *     edges are among the seven directions.  A tetrahedron with a non-finite corner value emits nothing and is counted in n_skipped.
 * Triangles: one or three corners inside: one triangle on the three crossing edges; two corners inside, a1 < a2 inside and b1 < b2 outside
 *     in corner order: the quad cycle (a1 b1, a1 b2, a2 b2, a2 b1).
 * Orientation is combinatorial: decided on the integer corner offsets alone, never from floats (a zero or negative step does not change it).
 *     The vertex order is counter-clockwise seen from the outside: the triangle's normal points from the inside corners towards the outside
 *     ones.  Every triangle is rotated so that its smallest vertex index comes first; a quad is oriented the same way, rotated so that its
 *     smallest vertex index is q0, and emitted as (q0, q1, q2), then (q0, q2, q3).
 * Triangle order: by the cell's linear index (in the points' indexing), then by tetrahedron, then by the two triangles of a quad.
 * Consequences: every triangle edge is shared by exactly two triangles in opposite directions, except where the surface leaves the lattice;
 *     a corner value of exactly iso gives zero-area triangles but keeps the surface closed; a vertex next to a non-finite value may be
 *     referenced by no triangle.  A lattice with a count of 1 has no cells: FT_OK and an empty mesh, no vertices either, no device needed.
 *     The index type is int32: a mesh with 2^31 or more vertices or triangles is FT_ERR_UNSUPPORTED.
 *
 * ft_mesh_lattice evaluates the scene's distance on the lattice into the context's scratch (ft_sample_lattice_device's launch, never
 * FT_FIELD_BOUNDED: a sphere's boundary is its surface, and NaN outside it would empty the mesh), then extracts.  flags: FT_MESH_NORMAL and
 * FT_MESH_MATERIAL add per vertex SdfForm.normal (normal_epsilon, read only with FT_MESH_NORMAL) and the material handle, from one points-form
 * field launch over the vertex buffer: exactly what ft_sample_points_device gives for those points.
 * ft_mesh_values / ft_mesh_values_device mesh any float32 lattice already in host / device memory (nx * ny * nz values, k contiguous; the
 * device pointer 4-byte aligned; the values are only read): no scene, no normals, no materials.
 * The extraction cannot size its outputs before it has counted: each constructor synchronises the context's stream ONCE, to read the two
 * totals, then allocates exactly, then emits on the context's stream without synchronising again (ft_mesh_read does; the buffers of
 * ft_mesh_device_buffers are ordered with whatever the context launches next).  Scratch: 4 B per point for ft_mesh_lattice's and
 * ft_mesh_values' distances, 5 B per point and 12 B per tile of points for the extraction.
 * Refusals, all made before the device is asked for, in this order: FT_ERR_INVALID for NULL where none is allowed (context, scene, lattice,
 * values, out), a scene of another context, a count < 1 or > 16777216, unknown flag bits, a misaligned device pointer; FT_ERR_UNSUPPORTED for
 * nx * ny * nz >= 0xFFFF0000 (and for a scene whose LDS footprint no kernel fits); then FT_ERR_NO_DEVICE on a host-only context; FT_ERR_HIP
 * for a failed allocation.  On any failure *out is NULL.
 * A mesh owns device memory of its context: it outlives its scene but not its context.  ft_mesh_read copies to the caller's buffers (n_vertices x
 * 3 float32, n_triangles x 3 int32, n_vertices x 3 float32, n_vertices x int32; host memory, or device memory: the direction of each copy is
 * taken from the address), synchronises the context's stream and accepts NULL for any part; asking for normals or materials the mesh was not
 * built with is FT_ERR_INVALID.  ft_mesh_device_buffers gives the device addresses (NULL for a part the mesh does not have or
 * that is empty); each of its out-parameters may be NULL. */
#define FT_MESH_NORMAL 1u
#define FT_MESH_MATERIAL 2u
typedef struct ft_mesh ft_mesh;                       /* opaque; owns device memory of its context */
typedef struct ft_mesh_info { int64_t n_vertices, n_triangles, n_skipped; int32_t has_normal, has_material; } ft_mesh_info;
int ft_mesh_lattice(ft_ctx*, const ft_scene*, const ft_lattice*, float iso, float normal_epsilon, uint32_t flags, ft_mesh** out);
int ft_mesh_values_device(ft_ctx*, const ft_lattice*, const void* d_values, float iso, ft_mesh** out);
int ft_mesh_values(ft_ctx*, const ft_lattice*, const float* values, float iso, ft_mesh** out);
int ft_mesh_get_info(const ft_mesh*, ft_mesh_info* out);
int ft_mesh_device_buffers(const ft_mesh*, void** d_vertices, void** d_triangles, void** d_normals, void** d_materials);
int ft_mesh_read(const ft_mesh*, ft_vec3* vertices, int32_t* triangles, ft_vec3* normals, int32_t* materials);
void ft_mesh_destroy(ft_mesh*);

/* Slicing: per lattice plane the contour {distance = iso} of a lattice of distances as ordered, consistently oriented polylines, extracted and
 * chained on the device.  A slice is exactly the section of the mesher's surface by a lattice plane: the Kuhn subdivision of a cell, restricted to a
 * cell face, is the face's two triangles split by the (0,0)-(1,1) diagonal.  The result is a pure function of the lattice's values; this is the rule,
 * every bit of it.  What it shares with "Meshing" above is stated there.
 *
 * Input: a lattice, a float32 value d[q] per point and a level iso as in "Meshing", and an axis a in {0, 1, 2} (x, y, z), the planes' normal.
 * Planes: slice w, 0 <= w < n_a, is the 2D lattice of the points whose index along a is w.  Its in-plane axes are u = (a + 1) % 3 and
 *     v = (a + 2) % 3, so (u, v, a) is right-handed.  A count of 1 along a is one slice.  A count of 1 along u or v leaves no cells: FT_OK, an empty
 *     result, no device needed.
 * Signed value and inside: the mesher's, s[q] = d[q] - iso, inside iff s[q] < 0.
 * Edges: the mesher's seven directions and their numbers e, of which each plane uses the three with no component along a, +v, +u and +u+v:
 *     e 0, 1, 2 for axis 0; 0, 3, 4 for axis 1; 1, 3, 5 for axis 2.
 * Vertices: ownership, the existence rule and the position are the mesher's, operation for operation, all three coordinates: a contour point is
 *     bit for bit the vertex the mesher puts on the same edge.  A vertex's key is (q, e) with the mesher's e; keys order by q, then e.
 * Triangles: cell (cu, cv) of slice w, with c0 its point of smallest indices, is cut in two, in this order: T0 = {c0, c0 + u, c0 + u + v}, then
 *     T1 = {c0, c0 + v, c0 + u + v}.  A triangle with a non-finite corner value emits nothing and is counted in n_skipped.  A triangle with one or
 *     two corners inside emits one segment, between the vertices of its two crossing edges.
 * Direction is combinatorial: decided from the integer (u, v) corner offsets alone, never from floats or the sign of a step.  With u to the right and
 *     v up, the inside corners lie to the segment's left: with L the corner that differs from the other two, M1 and M2, the segment runs from the
 *     vertex on (L, M1) to the one on (L, M2) iff (det(M2 - M1, L - M1) > 0) == (L is inside).  Outer boundaries therefore run counter-clockwise
 *     seen from +a, and holes run clockwise.  Every vertex is the start of at most one segment and the end of at most one.
 * Polylines: a polyline is a maximal chain of segments joined at shared vertices.  Closed: a cycle of m segments, written as its m points, starting
 *     at the vertex of smallest key and following the segments' direction.  Open: a chain whose first vertex no segment ends in (where the contour
 *     leaves the lattice or meets a skipped triangle), written as its m + 1 points from that vertex to the last.  A vertex that no segment uses is
 *     not written.  Polylines are ordered by the key of their first point, and each carries the slice it lies in: for axis 0 that order is already
 *     slice by slice; for axes 1 and 2 it is not, and ft_polyline.slice tells them apart.
 * Consequences: on an all-finite lattice every polyline is closed unless it ends on the lattice's border; a value of exactly iso gives zero-length
 *     segments but keeps loops closed.  Counts and indices are int32: 2^31 or more points or polylines is FT_ERR_UNSUPPORTED.
 *
 * Lifetime and forms are the mesher's, item for item: ft_slice_lattice evaluates the scene's distance on the lattice into the context's scratch
 * (never FT_FIELD_BOUNDED), then extracts; FT_SLICE_NORMAL and FT_SLICE_MATERIAL add per point SdfForm.normal (normal_epsilon, read only with
 * FT_SLICE_NORMAL) and the material handle from one points-form field launch over the finished point buffer: exactly what
 * ft_sample_points_device gives for those points.  ft_slice_values / ft_slice_values_device slice any float32 lattice already in host / device
 * memory (the device pointer 4-byte aligned; the values are only read): no scene, no normals, no materials.
 * The extraction cannot size its outputs before it has counted: each constructor synchronises the context's stream TWICE, once to read the vertex
 * and segment totals (the chaining's work is sized from them) and once to read the point and polyline totals; then it allocates exactly and writes
 * the points and the records on the context's stream without synchronising again (ft_slices_read does).  The chaining is pointer doubling, R rounds
 * with 2^R at least the vertex total, run twice and launched without a synchronisation between them; nothing is written at or beyond the counted
 * totals.  Scratch: as the mesher's for the lattice; 57 B per vertex and 12 B per tile of vertices of chaining work that the context keeps.
 * Refusals, all made before the device is asked for, in the mesher's order, with an axis outside 0 .. 2 (FT_ERR_INVALID) after the counts and
 * before the flag bits.  On any failure *out is NULL.
 * The contours own device memory of their context: they outlive their scene but not their context.  ft_slices_read copies to the caller's buffers
 * (n_points x 3 float32, n_polylines x ft_polyline, n_points x 3 float32, n_points x int32; host or device memory: the direction of each copy is
 * taken from the address), synchronises the context's stream and accepts NULL for any part; asking for normals or materials the contours were not
 * built with is FT_ERR_INVALID.  ft_slices_device_buffers gives the device addresses (NULL for a part that is missing or empty); each of its
 * out-parameters may be NULL. */
#define FT_SLICE_NORMAL 1u
#define FT_SLICE_MATERIAL 2u
typedef struct ft_slices ft_slices;                   /* opaque; owns device memory of its context */
typedef struct ft_polyline { int32_t first, count, slice, closed; } ft_polyline;   /* 16 B: points [first, first + count) */
typedef struct ft_slices_info { int64_t n_points, n_polylines, n_closed, n_skipped; int32_t axis, n_slices, has_normal, has_material; } ft_slices_info;  /* 48 B */
int ft_slice_lattice(ft_ctx*, const ft_scene*, const ft_lattice*, int32_t axis, float iso, float normal_epsilon, uint32_t flags, ft_slices** out);
int ft_slice_values(ft_ctx*, const ft_lattice*, const float* values, int32_t axis, float iso, ft_slices** out);
int ft_slice_values_device(ft_ctx*, const ft_lattice*, const void* d_values, int32_t axis, float iso, ft_slices** out);
int ft_slices_get_info(const ft_slices*, ft_slices_info* out);
int ft_slices_device_buffers(const ft_slices*, void** d_points, void** d_polylines, void** d_normals, void** d_materials);
int ft_slices_read(const ft_slices*, ft_vec3* points, ft_polyline* polylines, ft_vec3* normals, int32_t* materials);
void ft_slices_destroy(ft_slices*);

/* Refinement: mesh and contour vertices moved onto the surface {distance = iso} by bisection of their lattice edge, on the device, and the same
 * machinery as a query of its own.  The mesher's vertex is the linear interpolation of the two end values of a lattice edge: it is off the surface by
 * whatever the field does between two lattice points.  The scene forms still hold the field when the vertices exist, so they can bisect the edge R
 * times and interpolate on the last bracket.  The topology does not change: only positions move.  This is the rule, every bit of it.
 *
 * Bracket: two points A, B (float32 x 3) with signed values sA, sB.  Both values are finite and exactly one of sA < 0, sB < 0 holds; inside is the
 *     mesher's s < 0.
 * Round, repeated R times:
 *         M = (A + B) * 0.5f per coordinate: one float32 sum, rounded, then one product, rounded;
 *         sM = D(M) - iso, with D(M) the bits ft_eval_distance / ft_sample_points give for M and one float32 subtraction.
 *     If sM is not finite the bracket stays as it is.  Otherwise, if (sM < 0) == (sA < 0) then (A, sA) = (M, sM), else (B, sB) = (M, sM).
 *     There is no other stopping rule: a bracket that can no longer shrink is a fixed point of this rule.
 * Finish: t = sA / (sA - sB), v = A + t * (B - A): the mesher's operations, rounded one by one, never fused, always from A towards B.
 * Mesh and contour vertices: edge (q, e) starts with A = p(q), the owner, B = p(q'), sA = s[q] and sB = s[q'], taken from the lattice.  With R = 0
 *     the finish is the mesher's formula on the mesher's operands: the result is bit-equal to the unrefined one.  A vertex is refined once and shared
 *     by every triangle or segment that uses it; a refined contour point is bit for bit the refined mesh vertex on the same edge.  Numbering,
 *     triangles, orientation, polylines, their order and n_skipped are those of the unrefined result, word for word.
 * Accuracy: the field is 1-Lipschitz and a zero of D - iso lies inside a bracket of length L * 2^-R (L: the lattice edge's length), so
 *     |D(v) - iso| <= L * 2^-R up to the evaluation's float32 noise, which takes over beyond R = 12 on scenes of unit size.
 *
 * ft_mesh_lattice_refined and ft_slice_lattice_refined are ft_mesh_lattice and ft_slice_lattice in every respect, with the refinement between the
 * vertex emit and whatever reads the vertices: for the mesher the normal / material launch, for the slicer the scatter into the point buffer and then
 * the normal / material launch.  Normals and materials are therefore taken at the refined positions.  refine_steps is R, 0 .. 32; outside that it is
 * FT_ERR_INVALID, checked right after the flag bits; every other refusal keeps the parent's place.  They add no synchronisation (the mesher still
 * synchronises once, the slicer twice): one launch forms the brackets from the values, and from the mask and vertex index the count and emit passes
 * left in the context's scratch; then per round one points-form field launch over the midpoints, distance only, and one launch of the round.  That
 * makes 1 + 2 R launches on the context's stream behind the emit.  Work memory: 48 B per vertex (eight bracket arrays, the midpoint, its
 * distance), in a buffer the context keeps, sized from the vertex total the constructor already reads.  There are no refined *_values forms: they
 * have no field.
 *
 * ft_refine_segments: where does the segment from a[r] to b[r] cross the level?  sA = D(a) - iso, sB = D(b) - iso.  out_status[r] is 1 where both are
 * finite and exactly one is inside: then out_point[r] is the finish after `steps` rounds.  Otherwise the status is 0 and the point is three NaN.
 * Bisection finds A crossing, not the first one: a segment that crosses the level three times has status 1 and gives any of the three; one that
 * crosses it twice has status 0.  Either output may be NULL, but not both; with out_point NULL no round runs.  Host and device forms follow the
 * contracts of ft_sample_points / ft_sample_points_device.  Refusals, all made before the device is asked for, in this order: FT_ERR_INVALID for a
 * NULL context or scene or a scene of another context, no output asked for, steps outside 0 .. 32, NULL ends or n < 0, a misaligned device buffer
 * (every one 4-byte aligned; points are 12 B apart), an output identical to an input or to the other output; FT_ERR_UNSUPPORTED for
 * n >= 0xFFFF0000; n = 0: FT_OK, nothing launched; then FT_ERR_NO_DEVICE on a host-only context.  The host form stages through the context's scratch
 * (24 B per segment up, 12 + 4 B down for the outputs asked for) and synchronises; the device form is launched on the context's stream and NOT
 * synchronised.  Work memory: 52 B per segment in the same buffer. */
int ft_mesh_lattice_refined(ft_ctx*, const ft_scene*, const ft_lattice*, float iso, float normal_epsilon, uint32_t flags, int32_t refine_steps,
                            ft_mesh** out);
int ft_slice_lattice_refined(ft_ctx*, const ft_scene*, const ft_lattice*, int32_t axis, float iso, float normal_epsilon, uint32_t flags,
                             int32_t refine_steps, ft_slices** out);
int ft_refine_segments(ft_ctx*, const ft_scene*, const ft_vec3* a, const ft_vec3* b, int64_t n, float iso, int32_t steps, ft_vec3* out_point,
                       int32_t* out_status);
int ft_refine_segments_device(ft_ctx*, const ft_scene*, const void* d_a, const void* d_b, int64_t n, float iso, int32_t steps, void* d_point,
                              void* d_status);

/* Shells: the connected pieces of an indexed triangle mesh, labelled on the device, with a record per piece, and the selection of some of them as a
 * mesh of its own.  Only connectivity is read, never a float; every output is an integer and a pure function of the triangle list; this is the rule,
 * every bit of it.
 *
 * Input: nV >= 0 vertices and nT >= 0 triangles of three int32 vertex indices each, 0 <= index < nV, the three indices of one triangle pairwise
 *     different.  The mesher guarantees both conditions; the generic entries check them.
 * Used vertex: a vertex named by at least one triangle.
 * Shell: a connected component of the graph whose nodes are the used vertices and whose edges are the triangles' sides.  Connectivity is by shared
 *     vertex: two triangles that share one vertex only are one shell.  Zero-area triangles connect like any other.
 * Numbering: shells are numbered 0 .. S - 1 in ascending order of their smallest vertex index.
 * Labels: vertex_shell[v] is the vertex's shell, or -1 for an unused vertex (for example one next to a non-finite value that no triangle
 *     references); triangle_shell[t] is the shell of the triangle's vertices.
 * Directed sides: triangle (t0, t1, t2) has the sides t0 -> t1, t1 -> t2, t2 -> t0.
 * Border edge: side a -> b is a border edge iff no triangle has the side b -> a.  Each side is judged on its own: a side that occurs twice is not a
 *     border edge if its reverse occurs once.
 * Record: ft_shell { first_vertex, n_vertices, n_triangles, n_border_edges }, 16 B.  first_vertex is the shell's smallest vertex, the key of the
 *     numbering.  A shell is closed iff n_border_edges == 0.
 * Info: ft_shells_info: the input's two counts, the shells, the closed ones, the unused vertices and the border edges of all shells together.
 * Limit: counts are int32.  n_triangles >= 715827883 (where 3 * nT no longer fits int32) is FT_ERR_UNSUPPORTED.
 * Empty input: nT == 0 gives zero shells and every vertex unused: FT_OK, no device needed, like the mesher's empty mesh.
 * Selection: given one byte per shell, shell s is kept iff keep[s] != 0.  The result is an ft_mesh that holds exactly the used vertices of the kept
 *     shells, in their old relative order (the new index is the rank among the kept), and the kept triangles in their old order with the indices
 *     remapped; normals and materials are gathered where the source has them; n_skipped is copied from the source.  The remap is monotone, so every
 *     triangle still starts with its smallest index and the kept shells keep their relative numbering: shells(select(m, keep)) equals the kept
 *     records with first_vertex remapped, in order.  No shell kept gives an empty mesh.
 *
 * ft_mesh_shells labels a mesh where it lies.  ft_shells_triangles labels any indexed mesh in host memory (staged through the context's scratch,
 * 12 B per triangle); ft_shells_triangles_device one in device memory (4-byte aligned, only read).  The shells own device memory of their context
 * and are independent of the mesh once built: they outlive it, but not their context.
 * Refusals, all made before the device is asked for, in this order: FT_ERR_INVALID for NULL where none is allowed (mesh, context, triangles unless
 * n_triangles is 0, out), a negative count or n_vertices >= 2^31, a misaligned device pointer; FT_ERR_UNSUPPORTED for the triangle limit;
 * FT_ERR_INVALID for triangles without vertices and, in ft_shells_triangles, for an index outside 0 .. n_vertices - 1 or twice in one triangle
 * (it validates its indices on the host before it uploads); empty input: FT_OK; then FT_ERR_NO_DEVICE on a host-only context; FT_ERR_HIP for a failed
 * allocation.  ft_shells_triangles_device validates the indices on the device in its first pass and reports FT_ERR_INVALID at the constructor's
 * first synchronisation; no kernel indexes anything with an unchecked value.  On any failure *out is NULL.
 * Synchronisations: the labelling iterates (hooking of roots plus shortcutting after Shiloach and Vishkin; at most floor(log_{3/2} nV) + 2
 * iterations, which the host loop carries as a hard cap: at the cap it returns an error, never a partial labelling) and the iterations needed depend
 * on the data.  A constructor synchronises the context's stream ceil(I / 4) + 1 times, I the iterations it ran: one read of a 4-byte flag per batch
 * of B = 4 iterations, written by a verify launch of its own, plus one for the totals; the labels and records are then complete
 * (ft_shells_device_buffers' addresses are ordered with whatever the context launches next).  Work memory, in a buffer the context keeps: 36 B per
 * vertex, 12 B per triangle, 16 B per three vertices, 4 B per tile of vertices and of triangles.
 * ft_shells_read copies to the caller's buffers (n_vertices x int32, n_triangles x int32, n_shells x ft_shell; host memory, or device memory: the
 * direction of each copy is taken from the address), synchronises the context's stream and accepts NULL for any part.
 * ft_mesh_select: keep is host memory, n_keep == n_shells.  FT_ERR_INVALID for NULL (mesh, shells, keep unless n_keep is 0, out), for shells that
 * were not built from that mesh (every mesh carries a serial number that its shells remember: equal counts alone do not pass; shells of a triangle
 * list select nothing), then for n_keep != n_shells; no shell kept: FT_OK and an empty mesh, no device needed; then FT_ERR_NO_DEVICE, FT_ERR_HIP.
 * It synchronises ONCE, for its two totals, then allocates exactly and scatters without synchronising again.  The result is a mesh like any other:
 * it outlives the source mesh and the shells. */
typedef struct ft_shells ft_shells;                   /* opaque; owns device memory of its context; independent of the mesh once built */
typedef struct ft_shell { int32_t first_vertex, n_vertices, n_triangles, n_border_edges; } ft_shell;   /* 16 B */
typedef struct ft_shells_info { int64_t n_vertices, n_triangles, n_shells, n_closed, n_unused_vertices, n_border_edges; } ft_shells_info;   /* 48 B */
int ft_mesh_shells(const ft_mesh*, ft_shells** out);
int ft_shells_triangles(ft_ctx*, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, ft_shells** out);
int ft_shells_triangles_device(ft_ctx*, const void* d_triangles, int64_t n_triangles, int64_t n_vertices, ft_shells** out);
int ft_shells_get_info(const ft_shells*, ft_shells_info* out);
int ft_shells_device_buffers(const ft_shells*, void** d_vertex_shell, void** d_triangle_shell, void** d_records);
int ft_shells_read(const ft_shells*, int32_t* vertex_shell, int32_t* triangle_shell, ft_shell* records);
void ft_shells_destroy(ft_shells*);
int ft_mesh_select(const ft_mesh*, const ft_shells*, const uint8_t* keep, int64_t n_keep, ft_mesh** out);

/* Measures: per shell of a labelled mesh its area, signed volume, first moment and box, computed on the device where the mesh lies.  Floating-point
 * sums are not associative, so the rule makes the sums exact: every triangle gives float64 terms by a fixed sequence of individually rounded
 * operations, every term is rounded ONCE to a multiple of a power of two that the call fixes in advance, and the quantised terms are added as
 * integers, where order cannot matter.  Every bit of every result is a pure function of the input; this is the rule, all of it.
 *
 * Input: vertices float32[nV][3], triangles int32[nT][3], a label per triangle and per vertex (ft_shells' triangle_shell and vertex_shell; in the
 *     whole-mesh form every triangle and every vertex has label 0 and there is one shell).
 * Extent: m is the largest |x| over all finite coordinates of all nV vertices, used by a triangle or not.  E = 0 if m == 0 (or no coordinate is
 *     finite), else ilogb(m) + 1, so that m < 2^E; denormals count by their true exponent.  Hence -148 <= E <= 128 (the smallest positive float32
 *     is 2^-149).
 * Measured triangles: a triangle is measured iff its three indices are in 0 .. nV - 1 (the mesher guarantees it) and all nine of its coordinates
 *     are finite.  Any other triangle adds nothing to any sum and 1 to its shell's n_unmeasured.  Zero-area triangles are measured.
 * Terms of a measured triangle (a, b, c): the nine float32 coordinates are widened to float64 (exact); then every -, *, + is one float64
 *     operation, never fused, operands in the order written:
 *         u = b - a,  v = c - a
 *         n = (u.y v.z - u.z v.y,  u.z v.x - u.x v.z,  u.x v.y - u.y v.x)
 *         A_t = 0.5 * sqrt((n.x n.x + n.y n.y) + n.z n.z)                    sqrt correctly rounded
 *         W_t = (a.x (b.y c.z - b.z c.y) + a.y (b.z c.x - b.x c.z)) + a.z (b.x c.y - b.y c.x)     six times the signed volume of (0, a, b, c)
 *         M_t,i = W_t * ((a_i + b_i) + c_i)                                    i = x, y, z
 * Bounds, from |coordinate| < 2^E (exact values first, then the roundings):
 *     area:    |u_i|, |v_i| < 2^(E+1), so |n_i| < 2 * 2^(2E+2) = 2^(2E+3), |n|^2 < 3 * 2^(4E+6) and A_t < 0.5 * sqrt(3) * 2^(2E+3) < 2^(2E+3).
 *              B_A = 2E + 3.
 *     volume:  each of the three brackets is below 2 * 2^(2E) in magnitude, each product with a coordinate below 2^(3E+1), their sum below
 *              3 * 2^(3E+1) < 2^(3E+3).  B_W = 3E + 3.
 *     moment:  |(a_i + b_i) + c_i| < 3 * 2^E, so |M_t,i| < 3 * 2^(3E+1) * 3 * 2^E = 18 * 2^(4E) < 2^(4E+5).  B_M = 4E + 5.
 *     Each term is reached by about a dozen roundings of relative size 2^-53 of intermediates that obey the same bounds, and each exact bound
 *     leaves a factor of at least 1.15 (area; 1.33 volume, 1.77 moment) to its power of two, so a rounded term stays below 2^B, let alone 2^(B+1).
 *     No intermediate leaves float64's normal range: the smallest non-zero product of four float32 values is 2^-596, the largest term 2^517.
 * Quantisation: for a kind K with bound exponent B_K, s_K = 90 - B_K and q = round-half-to-even(term * 2^s_K) as a mathematical integer, so
 *     |q| <= 2^91 (2^90 by the bounds above).  With nT < 2^31 every sum lies inside +-2^122: a 128-bit two's-complement accumulator never
 *     overflows.
 * Sums: per shell and kind Q_K = the sum of q over the shell's measured triangles, exactly.
 * Results: S_K = fl64(Q_K) * 2^(-s_K): the int128 -> float64 conversion rounds half to even, the scaling is exact (every exponent stays inside
 *     float64's normal range for -148 <= E <= 128).  area = S_A, volume = S_W / 6.0, moment[i] = S_M,i / 24.0, each one float64 division.
 *     moment is the integral of x over the enclosed volume; the centroid is moment / volume.
 * Sign: with the mesher's orientation (counter-clockwise seen from the outside) a closed body has volume > 0 and a closed cavity volume < 0.  The
 *     volume and moment of an open shell are the rule's numbers and mean nothing geometric.
 * Box: per shell, bbox_min[i] / bbox_max[i] over the finite values of coordinate i of the vertices labelled with that shell, compared by the
 *     ordered-integer key of the float32 bits (bits ^ 0x80000000 for a clear sign bit, ~bits for a set one, so -0 < +0): the result is one of the
 *     input bit patterns.  A shell without a finite value in a coordinate gets +inf / -inf there.
 * Record: ft_shell_measure, 72 B.  extent_exponent is E, the same in every record of a call.
 * Empty input: a mesh without vertices and triangles, or zero shells, gives FT_OK with nothing written and needs no device.
 *
 * ft_shells_measure writes n_shells records, ft_mesh_measure one record for the whole mesh.  out is host memory or device memory (8-byte aligned):
 * the direction is taken from the address, as in ft_shells_read.  The host form synchronises the context's stream once; the device form does not
 * synchronise: the records are ordered with whatever the context launches next.  A selected mesh (ft_mesh_select) measures like any other.
 * Refusals, all made before the device is asked for, in this order: FT_ERR_INVALID for NULL (mesh, shells; out unless nothing would be written),
 * for shells that were not built from that mesh (the serial number ft_mesh_select checks: shells of a triangle list measure nothing), for a
 * misaligned device pointer; empty input: FT_OK; then FT_ERR_NO_DEVICE on a host-only context; FT_ERR_HIP for a failed allocation.
 * Work memory, in a buffer the context keeps: 108 B per shell (five 128-bit sums, six box keys, one counter), 72 B per shell of staging for the
 * host form, and the 4-byte extent. */
typedef struct ft_shell_measure {
    double area, volume, moment[3];
    float bbox_min[3], bbox_max[3];
    int32_t n_unmeasured;         /* triangles of the shell that were not measured */
    int32_t extent_exponent;      /* E */
} ft_shell_measure;               /* 72 B */
int ft_shells_measure(const ft_mesh*, const ft_shells*, ft_shell_measure* out);
int ft_mesh_measure(const ft_mesh*, ft_shell_measure* out);

/* Contour measures: per polyline of a stack of contours its length, signed enclosed area, first moment and box in the plane, and the same per slice,
 * computed on the device where the points lie.  What "Measures" does for shells: float64 terms by a fixed sequence of individually rounded
 * operations, one quantisation per term, exact integer sums.  Every bit of every result is a pure function of the input; this is the rule, all of it.
 * What it shares with "Measures" is stated there.
 *
 * Input: points float32[nP][3]; nL polylines {first, count, slice, closed} (ft_polyline: the points [first, first + count)); an axis a in {0, 1, 2}
 *     and a slice count nW.  The in-plane coordinates are u = (a + 1) % 3 and v = (a + 2) % 3, as in "Slicing".  Nothing reads the coordinate along
 *     a, except the extent.
 * Extent: E is "Measures"' extent, taken over all finite coordinates (all three) of all nP points, part of a polyline or not.
 * Segments: polyline l with count = m has the segments (P_i, P_i+1), 0 <= i < m - 1, and, if closed != 0, the closing segment (P_m-1, P_0).  (A
 *     closed polyline of one point has the one segment (P_0, P_0); a polyline of no points has none.)
 * Measured segments: a segment is measured iff its four in-plane coordinates are finite.  Any other segment adds nothing to any sum and 1 to its
 *     polyline's n_unmeasured.  Zero-length segments are measured.
 * Terms of a measured segment (P, Q): the four float32 coordinates are widened to float64 (exact); then every -, *, + is one float64 operation,
 *     never fused, operands in the order written:
 *         du = Q.u - P.u,  dv = Q.v - P.v
 *         L_t   = sqrt(du du + dv dv)                                           sqrt correctly rounded
 *         C_t   = P.u Q.v - Q.u P.v                                             twice the signed area of (0, P, Q)
 *         M_t,u = C_t (P.u + Q.u)
 *         M_t,v = C_t (P.v + Q.v)
 * Bounds, from |coordinate| < 2^E (exact values first, then the roundings):
 *     length:  |du|, |dv| < 2^(E+1), so du^2 + dv^2 < 2 * 2^(2E+2) = 2^(2E+3) and L_t < sqrt(2) * 2^(E+1) < 2^(E+2).  B_L = E + 2.
 *     area:    each of the two products is below 2^(2E) in magnitude, their difference below 2 * 2^(2E) = 2^(2E+1) < 2^(2E+2).  B_C = 2E + 2.
 *     moment:  |P.u + Q.u| < 2^(E+1), so |M_t| < 2^(2E+1) * 2^(E+1) = 2^(3E+2) < 2^(3E+3).  B_M = 3E + 3.
 *     Each term is reached by at most six roundings of relative size 2^-53 of intermediates that obey the same bounds, and each exact bound leaves a
 *     factor of at least 1.41 (length; 2 area, 2 moment) to its power of two, so a rounded term stays below 2^B, let alone 2^(B+1).
 *     No intermediate leaves float64's normal range for -148 <= E <= 128: the smallest non-zero product of three float32 values (or of two float32
 *     differences) is at least 2^-447, the largest term below 2^387; the quantisation scales by 2^s with -297 <= s <= 531, so a scaled non-zero
 *     term is at least 2^-744, still normal, and none goes beyond 2^91.
 * Quantisation, sums, results: "Measures"' word for word.  s_K = 90 - B_K, q = round-half-to-even(term * 2^s_K) as a mathematical integer; the
 *     sums are 128-bit two's-complement integers; S_K = fl64(Q_K) * 2^(-s_K).  A polyline has fewer than 2^31 segments and a call fewer than 2^31
 *     points, so no sum, per polyline or per slice, leaves +-2^122.
 * Polyline record: ft_contour_measure, 56 B.  length = S_L; area = S_C / 2.0; moment[0] = S_M,u / 6.0 and moment[1] = S_M,v / 6.0, each one float64
 *     division.  moment is the integral of (u, v) over the enclosed area; the centroid is moment / area.  bbox_min[2] / bbox_max[2]: over the finite
 *     u and the finite v of the polyline's points, by "Measures"' ordered key, +inf / -inf without a finite value.  n_unmeasured.  extent_exponent is
 *     E, the same in every record of a call.
 * Sign: with positive steps along u and v a closed outer boundary has area > 0 and a closed hole area < 0: "Slicing"'s direction rule makes outer
 *     boundaries run counter-clockwise in the lattice's (u, v) indices, and a negative step along u or v (not both) mirrors the plane and flips the
 *     sign.  The area and moment of an open polyline are the rule's numbers over its m - 1 segments and mean nothing geometric.
 * Slice record: ft_slice_measure, 72 B, for each slice w, 0 <= w < nW.  Q_L(w) is the exact integer sum of Q_L over all polylines with slice == w;
 *     Q_C(w) and Q_M(w) are the exact integer sums over the closed ones only; they are converted and divided as above, so holes subtract and area is
 *     the section's enclosed area.  n_polylines, n_closed; n_outer counts the closed polylines with Q_C > 0, n_holes those with Q_C < 0;
 *     n_unmeasured is the sum of the polylines'; the box is over all of the slice's polylines' points; extent_exponent is E.  A slice without
 *     polylines has zeros and the +inf / -inf box.
 * Empty input: contours without polylines give FT_OK and need no device; the n_slices slice records (zeros, the +inf / -inf box, E = 0) are still
 *     written if asked for.
 *
 * ft_slices_measure writes n_polylines records to out_polylines and n_slices records to out_slices, in the contours' order.  Either output may be
 * NULL, but not both, unless nothing would be written.  Each is host memory or device memory (8-byte aligned): the direction is taken from the
 * address, as in ft_shells_measure.  A host output synchronises the context's stream once (once for both); with device outputs nothing is
 * synchronised: the records are ordered with whatever the context launches next.  The contours may have outlived their scene.
 * Refusals, all made before the device is asked for, in this order: FT_ERR_INVALID for NULL (the contours; both outputs although something would be
 * written), for a misaligned device pointer, for out_polylines identical to out_slices; empty contours: FT_OK; then FT_ERR_NO_DEVICE on a host-only
 * context; FT_ERR_HIP for a failed allocation.
 * Work memory, in a buffer the context keeps: 84 B per polyline (four 128-bit sums, four box keys, one counter), 100 B per slice (four 128-bit sums,
 * four box keys, five counters), the 4-byte extent, and 56 B per polyline and 72 B per slice of staging for the outputs that are host memory. */
typedef struct ft_contour_measure {
    double length, area, moment[2];
    float bbox_min[2], bbox_max[2];
    int32_t n_unmeasured;         /* segments of the polyline that were not measured */
    int32_t extent_exponent;      /* E */
} ft_contour_measure;             /* 56 B */
typedef struct ft_slice_measure {
    double length, area, moment[2];
    float bbox_min[2], bbox_max[2];
    int32_t n_polylines, n_closed, n_outer, n_holes, n_unmeasured;
    int32_t extent_exponent;      /* E */
} ft_slice_measure;               /* 72 B */
int ft_slices_measure(const ft_slices*, ft_contour_measure* out_polylines, ft_slice_measure* out_slices);

/* Single-process multi-GPU form (what an F# host would call): the flattened scene is
 * re-uploaded to each further device with ft_scene_clone, every device renders its column
 * stripes (stripe_rank = index in ctxs[], stripe_ranks = n) on its own host thread, and the
 * slabs are collected with ONE ncclGather to ctxs[0]'s device, de-interleaved
 * there and copied to `out` (full width x height x 3 host image).  full_frame's stripe_* and
 * x0/n_columns fields are ignored except stripe_width (0 = contiguous blocks of width/n). */
int ft_scene_clone(const ft_scene* src, ft_ctx* dst_ctx, ft_scene** out);
int ft_render_multi(ft_ctx* const* ctxs, const ft_scene* const* scenes, int32_t n,
                    const ft_camera*, const ft_render_params* full_frame, float* out, ft_stats* stats);

/* ---- introspection of the flattened scene (tests; not needed by a caller) ---------------- */
typedef struct ft_scene_info {
    int32_t n_instr, n_slots, n_consts, n_grids, n_children, n_cells, n_items, n_lights, n_materials;
    int32_t fast_path;            /* which specialised evaluator the scene selected: 0 general interpreter, 1 smooth union of spheres, 2 general with
                                   * on-demand sub-programs, 3 carved union (one union of primitives + at most two intersect / subtract steps) */
    int32_t cull_pc;              /* instruction of the program whose sphere run the child-culling pass serves; -1: none */
} ft_scene_info;
int ft_scene_info_get(const ft_scene*, ft_scene_info* out);
/* grid g: info = aabbMin[3], cellSizeInv[3]; counts[3]; arrays sized from ft_scene_info /
 * ft_scene_grid_shape: cell_start[ncells+1], centers[3*ncells], lower[nitems], child[nitems] */
int ft_scene_grid_shape(const ft_scene*, int32_t g, float info[6], int32_t counts[3], int32_t* n_cells, int32_t* n_items);
int ft_scene_grid_dump(const ft_scene*, int32_t g, uint32_t* cell_start, float* centers, float* lower, int32_t* child);
/* the scene's support sphere (centre xyz, radius): no point farther than epsilon from it can be a hit, which is what FT_OPT_ESCAPE relies on;
 * radius < 0: none is known for this scene (degenerate shapes, a unionSmooth of strength <= 0) and every ray marches to its end */
int ft_scene_support_sphere(const ft_scene*, float centre_radius[4]);
/* the constants of the smooth-union kernel's miss certificate (FT_OPT_CERT; margin < 0: the scene has none):
 * margin certM, clip padding certClip, squared start radius certRho2, Length factor certLenF, steps left certSteps */
int ft_scene_miss_certificate(const ft_scene*, float out[5]);
/* the constants of the smooth-union kernel's occlusion certificate (FT_OPT_OCCL; out[1] < 0: the scene has none): drift per step occE, the margin's
 * constant part occB, the smallest epsilon tried occEpsMin, the largest margin occCap, 1 / the Length padding occLenInv, the distance occNear
 * from a sphere beyond which the form is positive, the largest parameter occReach (up to it the float32 sum of the form cannot underflow).  A shadow ray ends as a hit where its line has a point at which the form is proved to be at most
 * -(occE (t / epsilon + 2) + occB), at a parameter t <= min(Length * occLenInv, occReach) */
int ft_scene_occlusion_certificate(const ft_scene*, float out[7]);
/* the departure certificate's constants (FT_OPT_DEPART): drift per step, constant part, kappa's factor, smallest epsilon, clip pad, Length factor, steps; out[1] < 0: none */
int ft_scene_departure_certificate(const ft_scene*, float out[7]);
/* the clusters of the certificate's bound (n_clusters = 0: the scene has none, and the certificate sums every child): n_clusters records of 8 floats
 * {centre xyz, radius, member count, first member} (the last two are int32 bits), then the n_children children (x, y, z, r) in cluster order.
 * out = NULL: only the counts; otherwise capacity >= 8 n_clusters + 4 n_children floats */
int ft_scene_miss_certificate_clusters(const ft_scene*, int32_t* n_clusters, int32_t* n_children, float* out, int32_t capacity);

/* math primitives of the device path, evaluated on the GPU: op 0 exp, 1 log, 2 sqrt, 3 a/b, 4 fast sqrt, 5 fast exp
 * (y = second operand, may be NULL otherwise).  Used by tests/test_math_parity.py. */
int ft_math_eval(ft_ctx*, int32_t op, const float* x, const float* y, int64_t n, float* out);
/* further ops of ft_math_eval: 6 / 7 glibc expf (FMA / SSE2 build), 8 / 9 glibc logf, 10 / 11 glibc powf(x, y), 12 the fixed pow(x, y),
 * 13 / 14 the branch-free MathF.Max(x, y) / MathF.Min(x, y) of the carved-union kernels (14: x never NaN).
 * ft_selftest_libm: checksums of the device restatement of glibc's expf (op 0), logf (1) or powf(x, y) (2) in `variant`
 * (FT_MATH_GLIBC_FMA / FT_MATH_GLIBC_SSE2) over n_chunks x 2^24 consecutive float bit patterns from lo_bits:
 * sums[c] = sum over the chunk of splitmix64((input bits << 32) | result bits) mod 2^64, every NaN result taken as 0x7fc00000.  A test forms
 * the same sums with the libm of the machine it runs on (256 chunks = every float). */
int ft_selftest_libm(ft_ctx*, int32_t op, int32_t variant, float y, uint32_t lo_bits, int32_t n_chunks, uint64_t* sums);
/* Exhaustive check, on the GPU, of the fast sqrt / exp forms used inside the smooth-union loop against
 * the exact forms, over EVERY float of the ranges they are used on; mismatches[0] = sqrt (both the five-instruction
 * form and the four-instruction form that runs with output modifiers enabled), [1] = exp (ldexp form, [-2.9e6, 88]),
 * [2] = exp (exponent-add form, [-87, 88], in the normal mode and under the near loop's mode); all must be 0. */
int ft_selftest_fastmath(ft_ctx*, uint64_t mismatches[3]);

#ifdef __cplusplus
}
#endif
#endif /* FRAYTRACER_HIP_H */
