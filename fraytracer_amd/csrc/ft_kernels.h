// ft_kernels.h — kernel argument block and host-callable launchers (implemented in kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/fraytracer_hip.h"
#include "ft_device.h"
#include "ft_libm.h"          // FT_LIBM_TAB_DOUBLES: the *_libm kernels' tables in LDS (ft_lds_layout)

#define FT_BLOCK 256          // 4 waves; every wave is an independent persistent worker
// dynamic LDS of a trace workgroup starts with a header: 64 words (per-wave statistics, the reporting wave's start clocks), in the diagnostic
// build 13 rows of per-lane union-walk counters (kernels.hip FT_UDBG: 12 + 1 scratch row), then FT_SH_ROWS rows of per-lane shading state
#define FT_LDS_CNT_WORDS 64
// the header's words: 0 .. 31 the per-wave statistics (kernels.hip FT_C_*: FT_BLOCK / 64 words per counter), 32 .. 35 the reporting wave's two start
// clocks, FT_LDS_REPORT_WORD the lean kernel's mark of the workgroup whose first thread reports them, FT_LDS_TILE_WORD .. + 2 * FT_BLOCK / 64 - 1 per wave the tile it took last and its round count at that grab (kernels.hip "Tile order"),
// FT_LDS_WAVE_WORD .. + 4 * FT_BLOCK / 64 - 1 per wave the lean kernel's four accumulate-only sums (kernels.hip ft_trace_body waveSt), the rest free
#define FT_LDS_TILE_WORD 40
#define FT_LDS_WAVE_WORD 48
#define FT_LDS_REPORT_WORD 36
static_assert(FT_LDS_WAVE_WORD >= FT_LDS_TILE_WORD + 2 * (256 / 64) && FT_LDS_WAVE_WORD + 4 * (256 / 64) <= FT_LDS_CNT_WORDS, "the wave sums lie behind the tile words, inside the header");
static_assert(FT_LDS_TILE_WORD >= 36 && FT_LDS_TILE_WORD + 2 * (256 / 64) <= FT_LDS_CNT_WORDS, "the tile words lie behind the clocks, inside the header");
// FT_LDS_HINT_WORD .. + 2 * FT_BLOCK / 64 - 1 per wave the try hint of the tile it works on and the rounds its bundles have held on (kernels.hip "Try hints"):
// the statistics' unused rows, zeroed with them
#define FT_LDS_HINT_WORD 24
static_assert(FT_LDS_HINT_WORD + 2 * (256 / 64) <= 32, "the hint words lie in the statistics' unused rows");

// Try hints (FT_OPT_TRY_HINT): one 32-bit word per 8x8 tile.  Bits 0-7: the earliest evaluation round of the tile, counted from the round its wave took it, on
// which the bundle certificate of its primary rays held; bits 8-15: the same for its shadow rays.  Rounds from 254 on are noted as 254; FT_HINT_NONE: on none.
// The schedule a hinted tile follows is kernels.hip ft_try_due.
#define FT_HINT_NONE 255u
#define FT_HINT_MAX 254u
#define FT_HINT_USED 0x10000u  // set on the word a wave keeps in LDS: the tile's tries follow it (clear: the launch's period)
#define FT_HINT_AFTER 2u       // a family's tries behind its first hold, or behind its hinted round while nothing has held: every 2nd round (the shipped period)
#define FT_HINT_IDLE 4u        // whatever the hint, and all a family is tried on where none of its bundles held: every 4th round of the tile, its first included
FT_HD uint32_t ft_hint_pack(uint32_t primary, uint32_t shadow) { return (primary & 255u) | (shadow & 255u) << 8; }
FT_HD uint32_t ft_hint_primary(uint32_t w) { return w & 255u; }
FT_HD uint32_t ft_hint_shadow(uint32_t w) { return (w >> 8) & 255u; }
// the word after a bundle of the primary (else the shadow) family held on round r of the tile: the smaller round stays
FT_HD uint32_t ft_hint_note(uint32_t w, bool primary, uint32_t r) {
    const uint32_t v = r < FT_HINT_MAX ? r : FT_HINT_MAX, p = ft_hint_primary(w), s = ft_hint_shadow(w);
    return primary ? ft_hint_pack(v < p ? v : p, s) : ft_hint_pack(p, v < s ? v : s);
}

#ifdef FT_UNION_PROFILE
#define FT_LDS_DBG_ROWS 13
#else
#define FT_LDS_DBG_ROWS 0
#endif
#define FT_SH_ROWS 10         // hit position, normal, accumulated light (3 each), the distance at the hit position
#define FT_LDS_SH_BASE (FT_LDS_CNT_WORDS + FT_LDS_DBG_ROWS * FT_BLOCK)
#define FT_LDS_HDR_FLOATS (FT_LDS_SH_BASE + FT_SH_ROWS * FT_BLOCK)
// lean kernel: every wave owns a row of FT_CULL_MAX float4 records behind everything else (kernels.hip "Exact child culling").  With 256 staged
// spheres a workgroup then needs 34 304 bytes of LDS: four per CU.  224 records would let a fifth in, and lose: the LAST children of a union
// are the ones dropped most often (the running sum is largest in front of them) — C3 4096^2 34.3 ms at 256, 36.5 at 224
#define FT_CULL_MAX 256
#define FT_CULL_ROW (4 * FT_CULL_MAX)

// Dynamic LDS of a trace or eval-points workgroup, in floats: the header above, nSlots x FT_BLOCK value slots (distance), as many
// (material index), the staged prefix of the constant pool (nStage floats), glibc's tables (*_libm kernels; 8-byte aligned) and one
// FT_CULL_ROW row per wave (16-byte aligned: written and read as float4).  The one definition of the layout: the kernels take their
// addresses from it, the host its footprint (4 x total bytes; capi.cpp planTrace).
struct FtLdsLayout { uint32_t slotD, slotL, consts, libmTab, rows, total; };
FT_HD FtLdsLayout ft_lds_layout(uint32_t nSlots, uint32_t nStage, bool libm, bool rows) {
    FtLdsLayout L;
    L.slotD = FT_LDS_HDR_FLOATS;
    L.slotL = FT_LDS_HDR_FLOATS + nSlots * FT_BLOCK;
    L.consts = FT_LDS_HDR_FLOATS + 2u * nSlots * FT_BLOCK;
    L.libmTab = (L.consts + nStage + 1u) & ~1u;
    const uint32_t end = libm ? L.libmTab + 2u * FT_LIBM_TAB_DOUBLES : L.consts + nStage;
    L.rows = (end + 3u) & ~3u;
    L.total = rows ? L.rows + FT_CULL_ROW * (FT_BLOCK / 64) : end;
    return L;
}

struct FtRenderArgs {
    FtSceneDev S;
    float cam[12];            // Position, Forward, UpScaled, RightScaled (Camera.fs:16-22)
    int32_t W, H, x0, nCols;
    uint32_t stripeW, stripeRanks, stripeRank, mode;    // mode 0: Image.render pixels, 1: explicit ray buffer (SdfScene.trace, hits below), 2: ray buffer, SdfForm.tryTrace
    float maxSize, eps, length, pad0;
    const ft_ray* rays;
    float* out;
    uint32_t* counter;        // global job cursor (zeroed before every launch)
    FtStatsDev* stats;
    uint32_t nJobs, chunk, tilesY;
    uint32_t cull;            // lean kernel: 1 = drop, per wave and round, the children whose terms are exact no-ops (kernels.hip "Exact child culling")
    // EXTENSIONS (spp = 1, aoSamples = 0 is the reference): sample plane s of the frame is written at
    // out + s * planeFloats and resolved by ft_resolve_kernel; ambient-occlusion rays per primary hit
    uint32_t spp, sppN, aoSamples, jobsPerPlane;
    float aoRadius; uint32_t planePixels;
    uint32_t ext;             // 1: launch the EXTENSION build of the kernel (set by the host, see capi.cpp)
    uint32_t maxBounces;      // EXTENSION glass: interactions per path; 0 = glass shades as a solid
    uint32_t spectral;        // EXTENSION: wavelength bins (0 = off)
    uint32_t lazy;            // 1: unions under an intersect stop at Items.[0] where the intersect's next child already decides (FT_OPT_LAZY_UNION; kernels.hip)
    uint32_t refillMin;       // idle lanes a wave waits for before it takes new rays (1 = refill at once; kernels.hip "Burst refill")
    uint32_t math;            // 0: the default kernels; 1: launch the *_libm build (FT_OPT_MATH = glibc and the scene has a unionSmooth)
    uint32_t shrink1, shrink2;   // guided hand-out: from job shrink1 on a wave takes chunk / 2 jobs at a time, from shrink2 on chunk / 4 (nJobs: never)
    uint32_t tailK;           // latency mode: a wave holding at most this many rays evaluates them one at a time with all 64 lanes (0 = off)
    const float* materialsExt;   // EXTENSION: 4 floats per material (glass flag, ior, dispersion, 0); kept out of
                                 // FtSceneDev so that the reference kernels' argument layout does not move
    float spec[16][4];        // per bin: RGB weight, Cauchy term (ft_spectral_table)
    uint32_t reuse;           // 1: a secondary ray's first evaluation — at the hit position — is the value the normal's centre probe computed there (FT_OPT_REUSE; kernels.hip FT_SH_D0)
    FtCarve carve;            // FtSceneDev.fastPath == 3: the union's tail and its terminated candidate lists (ft_device.h "Carved union")
    // EXTENSION ft_render_hits (EXTENSION builds only; appended so that no field above moves): per pixel, SdfObject.tryTrace of its sample-0 ray;
    // mode 1 (ft_trace_rays_hits, ft_object_try_trace): per ray of the buffer, at the ray's index
    float* hitsOut;           // 16 dwords per pixel (ft_object_trace_result) at cl * H + y (*_views builds: view * planePixels + cl * H + y); NULL: not asked
    int32_t* matOut;          // material handle per pixel (-1 on a miss); NULL: not asked
    const int32_t* matHandles;   // dense material index -> context handle (ft_material_*): the inverse of the flattener's remap
    uint32_t hits;            // 0: no hit buffers; 1: with the frame; 2: hits only (no lighting, nothing written to out)
    // miss certificate (lean kernel; kernels.hip ft_miss_certificate): a ray is due once its step count reaches certPrim (primary) / certShadow (shadow ray);
    // a wave runs the certificate when at least certMin of its lanes are due; a ray it fails on is due again certRepeat steps later (0: never)
    uint32_t cert, certPrim, certShadow, certMin, certRepeat;
    // ft_render_views (the *_views builds only; appended so that no field above moves): one launch over nViews cameras of one scene.  Job j is view
    // (j / jobsPerPlane) / spp, sample plane (j / jobsPerPlane) % spp; view k writes planes k * spp .. k * spp + spp - 1 (kernels.hip "Views")
    const float* views;       // nViews x 12 floats (ft_camera) in device memory; cam above is unused
    uint32_t nViews;          // 1 .. FT_MAX_VIEWS: PH_CAM evaluates camera l % nViews in lane l
    // ft_shade_hits (the *_shade builds only; appended so that no field above moves): job j is record j of hitsIn, shaded from SdfScene.fs:11 on
    // and written to out + 3 j; rays, cam and mode are unused (kernels.hip start_job SHADE)
    uint32_t shade;           // 1: launch the SHADE build of the kernel (set by the host, see capi.cpp launchRayBuffer); 2: its ft_light_visibility twin
    const float* hitsIn;      // nJobs x 16 dwords (ft_object_trace_result), 16-byte aligned: a lane loads its record as four 16-byte words
    // ft_light_visibility (the *_vis builds only; appended): job j writes visOut[j] = (visIn ? visIn[j] & visKeep : 0) | the bits of the lights in
    // visSel whose shadow ray from record j missed (kernels.hip settle VIS); out is unused
    uint32_t visSel, visKeep; // select & (2^nLights - 1); ~select & (2^nLights - 1)
    const uint32_t* visIn;    // NULL: nothing kept; may equal visOut (a lane reads its word before it writes it)
    uint32_t* visOut;
    // bundle certificate (lean kernel; kernels.hip ft_bundle_certificate; appended): tried every bundlePeriod-th evaluation round of a wave (0: never) for its
    // primary rays and for its shadow rays of at least bundleShadow steps, each where at least bundleMin (>= 1) lanes hold such a ray; needs cert
    uint32_t bundlePeriod, bundleMin, bundleShadow;
    // tile order (FRAME builds without EXTENSION; kernels.hip refill; appended; set only for mode 0, spp 1, chunk = refillMin = 64, no guided hand-out):
    // tileCost, where not NULL, receives per 8x8 tile the evaluation rounds its wave spent between taking it and taking its next one; tileOrder,
    // where not NULL, is a permutation of the tiles: the grab at cursor position 64 k works on tile tileOrder[k] (ft_launch_tile_order builds it)
    uint32_t* tileCost;
    const uint32_t* tileOrder;
    // occlusion certificate (lean kernel; kernels.hip ft_occlusion_certificate; appended; the constants are the scene's, scene.cpp
    // "Occlusion certificate"): tried every occPeriod-th evaluation round of a wave (0: never) for its shadow rays of occFrom .. occFrom + occPeriod - 1
    // steps — each ray meets exactly one such round — where at least occMin (>= 1) lanes hold such a ray
    uint32_t occPeriod, occFrom, occMin;
    FtOccl occ;
    // try hints (the launches that record tileCost; kernels.hip "Try hints"; appended): tileHint, where not NULL, holds one word per tile (above) and
    // receives what this launch's bundles did; tryHint = 1: the word a tile's last frame left schedules its bundle tries (needs tileHint)
    uint32_t* tileHint;
    uint32_t tryHint, pad1;
    // departure certificate (lean kernel; FT_OPT_DEPART; appended): the margin of the per-lane miss certificate's tries (ft_device.h FtCertMargin).  The flat
    // margin of the scene, slope 0, on every launch the option leaves alone: those count what they counted (capi.cpp departSchedule)
    FtCertMargin dep;
};
static_assert(offsetof(FtRenderArgs, occ) == 860 && offsetof(FtRenderArgs, tileHint) == 888 && offsetof(FtRenderArgs, dep) == 904 && sizeof(FtRenderArgs) == 936, "the kernels' argument block does not move");
#define FT_MAX_VIEWS 64       // views per launch (one PH_CAM value per lane); ft_render_views splits larger batches

// The forms of the trace kernel (kernels.hip FT_TRACE_FORMS builds every one of them from the same table of builds): what a job is and what it leaves.
// FRAME: a pixel or a ray of a ray buffer (no suffix); VIEWS: a pixel of one of nViews cameras (*_views); SHADE: a hit record, shaded (*_shade);
// VIS: a hit record, one visibility bit per light (*_vis).  NONE: what a launch asks for where no form exists (a shade form has no views build).
enum { FT_FORM_FRAME = 0, FT_FORM_VIEWS = 1, FT_FORM_SHADE = 2, FT_FORM_VIS = 3, FT_FORM_NONE = 4 };
FT_HD uint32_t ft_trace_form(bool views, unsigned shade) {
    if (shade) return (views || shade > 2u) ? FT_FORM_NONE : (shade == 2u ? FT_FORM_VIS : FT_FORM_SHADE);
    return views ? FT_FORM_VIEWS : FT_FORM_FRAME;
}
// Which trace kernel a launch runs: the one key that ft_launch_trace and ft_trace_occupancy look up (kernels.hip ft_trace_kernel_for).  variant: the
// kernel family (FtSceneDev.fastPath as capi.cpp planTrace decides it); carveKind: FtCarve.kind, read for variant 3 only.
struct FtTraceKey { uint32_t variant, carveKind, form; bool ext, libm; };
FT_HD FtTraceKey ft_trace_key(const FtRenderArgs& a) {
    return FtTraceKey{a.S.fastPath, a.carve.kind, ft_trace_form(a.views != nullptr, a.shade), a.ext != 0u, a.math != 0u};
}

// Field sampling (ft_sample_points / ft_sample_lattice; kernels.hip "Field sampling"): one point per lane, one job per wave.  A job is 64 consecutive
// points of a point buffer (pts != NULL) or one brick of 64 lattice points: 2^lgI x 2^lgJ x 2^lgK of them along i, j and k (lgI = 6 - lgJ - lgK), lane
// l at (l >> (lgJ + lgK), (l >> lgK) & (2^lgJ - 1), l & (2^lgK - 1)) in its brick; brick b lies at (b / (bricksJ * bricksK), (b / bricksK) % bricksJ,
// b % bricksK) bricks.  A block of its own, like FtGridBuildArgs: nothing in FtRenderArgs or FtSceneDev moves.
struct FtFieldArgs {
    FtSceneDev S;             // fastPath: the kernel family as capi.cpp planTrace decides it (1 lean, 3 carved, otherwise the general interpreter)
    FtCarve carve;            // fastPath == 3 only
    const float* pts;         // points form: n x 3 floats; NULL: the lattice below
    float origin[3], step[3];
    uint32_t ny, nz, nx;      // lattice counts (points form: unused)
    uint32_t bricksJ, bricksK;
    uint32_t lgJ, lgK;        // the brick's shape
    uint32_t nJobs;           // bricks, or ceil(n / 64)
    uint32_t n;               // points form: the number of points (< 0xFFFF0000)
    uint32_t cull;            // 1: ft_cull_children before every evaluation round (needs the wave rows in LDS)
    uint32_t math;            // 1: the *_libm build
    uint32_t bounded;         // FT_FIELD_BOUNDED: evaluate only where (dx dx + dy dy) + dz dz < br2, d = p - bc
    float bc[3], br2;
    float normalEps;          // read only with outN
    uint32_t nMaterials;      // entries of matHandles
    float* outD;              // any of the three may be NULL, not all
    float* outN;              // 3 floats per point
    int32_t* outM;
    const int32_t* matHandles;   // dense material index -> context handle, as in FtRenderArgs
};
// the brick shapes a launch may ask for: lgJ, lgK of 4x4x4, 2x4x8 and 2x2x16
#define FT_FIELD_BRICKS {{2u, 2u}, {2u, 3u}, {1u, 4u}}
#define FT_FIELD_BRICK_DEFAULT 1

#ifdef __cplusplus
extern "C" {
#endif
hipError_t ft_launch_field(const FtFieldArgs* a, unsigned blocks, size_t ldsBytes, hipStream_t st);
hipError_t ft_field_occupancy(unsigned variant, unsigned carveKind, bool libm, size_t ldsBytes, int* blocksPerCU);
hipError_t ft_launch_trace(const FtRenderArgs* a, unsigned blocks, size_t ldsBytes, hipStream_t st);
hipError_t ft_launch_eval_points(const FtSceneDev* S, int math, const float* pts, long long n, float* outD, int* outM,
                                 unsigned blocks, size_t ldsBytes, hipStream_t st);
hipError_t ft_launch_math(int op, const float* x, const float* y, long long n, float* out, hipStream_t st);
// ft_selftest_libm: per chunk of 2^24 consecutive float bit patterns starting at lo, the sum of splitmix64(input bits << 32 | result bits)
// of the device restatement of glibc's expf (op 0) / logf (1) / powf(x, y) (2); variant 1 = FMA build, 2 = SSE2 build
hipError_t ft_launch_libm_checksum(int op, int variant, float y, uint32_t lo, uint32_t nChunks, unsigned long long* d_sums, hipStream_t st);
// device-side buildSpatialLookup (SdfBoundary.fs:245-274): one workgroup per cell
struct FtGridBuildArgs {
    const float* bounds;      // n x (cx, cy, cz, r)
    uint32_t n, c;            // items, cells per axis
    float aabbMin[3], cellSize[3], halfDiag;
    float* centers;           // ncells x 3
    uint32_t* counts;         // ncells
    FtItem* tmp;              // ncells x n, each cell's candidates sorted by (LowerBound, index)
    uint32_t* flags;          // bit0: NaN LowerBound, bit1: empty cell
};
hipError_t ft_launch_grid_build(const FtGridBuildArgs* a, hipStream_t st);
hipError_t ft_launch_grid_compact(const FtItem* tmp, const uint32_t* cellStart, uint32_t ncells, uint32_t n, FtItem* items, hipStream_t st);
#define FT_GRID_BUILD_MAX_ITEMS 4096
hipError_t ft_launch_resolve(const float* planes, float* out, unsigned long long nFloats, unsigned spp, hipStream_t st);
// Image.toColors (+ toBitmap order) on the device: max pass + map pass on one stream; maxBits = 4 bytes of device scratch
hipError_t ft_launch_tonemap(const float* frame, uint32_t X, uint32_t Y, uint32_t* maxBits, float gammaInv, uint32_t dither, uint32_t seed,
                             int bmpOrder, unsigned char* out, unsigned numCUs, int math, hipStream_t st);   // math: FT_OPT_MATH (0 fixed pow, 1 / 2 glibc powf)
// ft_render_multi: gathered slabs [rank][stripe][...] -> frame [stripe][rank][...] on the device
hipError_t ft_launch_deinterleave(const float* recv, float* frame, unsigned long long stripeFloats, uint32_t nStripes, uint32_t nRanks, hipStream_t st);
hipError_t ft_launch_selftest(int op, uint32_t lo, uint32_t hi, unsigned long long* d_mismatches, hipStream_t st);
// Probes of the wave primitives and of the culling pass (kernels.hip "Probes"; capi.cpp ft_selftest_wave, ft_selftest_cull; the tests only).
// wave: nWaves x 64 inputs -> FT_WAVE_PROBE_PLANES planes of nWaves x 64 floats (op 1 writes the first four).  cull: nWaves x 64 points and nWaves
// masks -> two return words and two rows of FT_CULL_ROW floats per wave, the general wording first; rows no pass wrote hold FT_CULL_PROBE_FILL.
#define FT_WAVE_PROBE_PLANES 8
#define FT_CULL_PROBE_FILL 0xffc0deadu   // a NaN that no scene record holds
hipError_t ft_launch_selftest_wave(int op, const float* x, float scale, uint32_t nWaves, float* out, hipStream_t st);
size_t ft_selftest_cull_lds_bytes(uint32_t nStage);
hipError_t ft_launch_selftest_cull(const FtSceneDev* S, const float* pts, const unsigned long long* masks, uint32_t nWaves, uint32_t* words, float* rows,
                                   hipStream_t st);
// the kernel handle of a key given piecewise, nullptr where no such kernel exists (internal, like ft_trace_occupancy; tests/test_trace_kernel_table.py)
const void* ft_trace_kernel_for(unsigned variant, unsigned carveKind, bool ext, bool libm, bool views, unsigned shade);
hipError_t ft_trace_occupancy(const FtTraceKey& key, size_t ldsBytes, int* blocksPerCU);
// Tile order (kernels.hip "Tile order"): from the nTiles costs a trace launch recorded, the permutation `order` its next launch hands tiles out in: the
// tiles of cost >= num / den of the mean first, by non-increasing cost, the rest in ascending index.  Three small launches and one memset on st, no
// synchronisation.  work: ft_tile_order_work_bytes(nTiles) bytes of device memory that stay the launches' own until they have run.
#define FT_ORDER_TILES 1024   // tiles per workgroup of the order kernels
struct FtTileOrderWork { uint32_t hist[256], cursor[256]; unsigned long long sum; uint32_t ticketCount, ticketHeavy, nHeavy, pad; };
size_t ft_tile_order_work_bytes(uint32_t nTiles);
hipError_t ft_launch_tile_order(const uint32_t* cost, uint32_t nTiles, uint32_t num, uint32_t den, uint32_t* order, void* work, hipStream_t st);
// ft_shade_visible: n records + n masks -> n colours, no march (kernels.hip ft_shade_visible_kernel); lights: the scene's, in device memory
hipError_t ft_launch_shade_visible(const FtLight* lights, uint32_t nLights, const float bg[3], const float* hits, const uint32_t* vis, uint32_t n,
                                   float* out, hipStream_t st);
#ifdef __cplusplus
}
#endif
