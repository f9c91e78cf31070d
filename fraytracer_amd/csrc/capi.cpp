// capi.cpp — the C ABI of libfraytracer_hip.so (include/fraytracer_hip.h).  Plain host C++;
// device code and launchers live in kernels.hip.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/fraytracer_hip.h"
#include "build_hash.h"      // FT_SOURCE_HASH: written by the Makefile (source_hash.py)
#include "ft_kernels.h"
#include "ft_mesh.h"
#include "ft_slice.h"
#include "ft_refine.h"
#include "ft_shells.h"
#include "ft_measure.h"
#include "ft_contour_measure.h"
#include "scene.hpp"

#ifndef FT_BUILD_KIND
#define FT_BUILD_KIND "product"
#endif

namespace {

thread_local std::string g_err;
int setErr(int code, const std::string& m) { g_err = m; return code; }
int hipFail(hipError_t e, const char* what) {
    return setErr(FT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return hipFail(_e, #expr); } while (0)

inline f3 tof3(const float* p) { return mk3(p[0], p[1], p[2]); }
inline f3 tof3(const ft_vec3& v) { return mk3(v.x, v.y, v.z); }

}  // namespace

struct ft_ctx {
    int device = -1;
    bool hasDevice = false;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    int numCUs = 0;
    ft::Builder builder;
    ft::GridFiller* filler = nullptr;
    uint32_t* dCounter = nullptr;
    FtStatsDev* dStats = nullptr;
    void* scratch = nullptr; size_t scratchBytes = 0;     // staging for host-output entry points
    void* planes = nullptr; size_t planesBytes = 0;       // EXTENSION spp > 1: per-sample frames before the resolve
    void* aux = nullptr; size_t auxBytes = 0;             // tone map: [256 B: max bits | 8-bit image]
    void* cams = nullptr; size_t camsBytes = 0;           // ft_render_views: the batch's cameras (12 floats each)
    hipStream_t lane1 = nullptr, copyStream = nullptr;    // ft_render's host-output pipeline: second render lane, DMA stream (lazily created)
    std::vector<hipEvent_t> syncEvents;                   // untimed events of that pipeline
    std::vector<std::pair<void*, size_t>> hostRegs;       // ranges pinned through ft_host_register
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events; // one pair per kernel launch since last collect (at most FT_MAX_PENDING_EVENTS)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> eventPool;
    double foldedMs = 0.0;                                 // kernel time of launches whose event pair was already recycled
    // ft_ctx_set_option (kOptions; experiments / A-B runs: every setting renders the same bits)
    int optRefillMin = 64;                                 // idle lanes a wave waits for before it takes new rays (kernels.hip "Burst refill")
    int optMaxBlocksPerCU = 0;                             // 0: the occupancy limit
    int optHostChunks = 0;                                 // 0: automatic (4 for frames >= 16 MB)
    int optHostPin = 1;                                    // page-lock an unregistered ft_render destination for the call
    int optMath = FT_MATH_FIXED;                           // FT_OPT_MATH: arithmetic of MathF.Exp / Log / Pow
    int optTailK = -1;                                     // FT_OPT_TAIL_K: latency mode threshold (-1: per kernel default, 0: off)
    int optChunk = 64;                                     // FT_OPT_CHUNK: jobs per grab (experiments: 64 = one 8x8 tile, 32, 16)
    int optEscape = 1;                                     // FT_OPT_ESCAPE: rays that can no longer reach the scene's support sphere end as misses at once (kernels.hip ft_never_enters)
    int optLazyUnion = 1;                                  // FT_OPT_LAZY_UNION: a union under an intersect stops at Items.[0] where the intersect's next child decides (kernels.hip)
    int optCull = 1;                                       // FT_OPT_CULL: exact child culling in the lean kernel (kernels.hip); 0 = every child, every round
    int optReuse = 1;                                      // FT_OPT_REUSE: a secondary ray's first evaluation is taken from the normal's centre probe (kernels.hip FT_SH_D0); 0 = evaluated again, as the reference does
    int optCarved = 1;                                     // FT_OPT_CARVED: scenes of the "carved union" shape take their specialised kernel (kernels.hip ft_eval_carved); 0 = the general interpreter
    int optCert = 1;                                       // FT_OPT_CERT: the lean kernel's miss certificate (kernels.hip ft_miss_certificate); needs optEscape
    int optCertPolicy = 0;                                 // FT_OPT_CERT_POLICY: 0 = FT_CERT_POLICY_DEFAULT
    int optGuided = 0;                                     // FT_OPT_GUIDED: smaller chunks at the end of the job queue (lean kernel; measured: no gain)
    int optOccl = 1;                                       // FT_OPT_OCCL: the lean kernel's occlusion certificate (kernels.hip ft_occlusion_certificate); needs optEscape
    int optOcclPolicy = 0;                                 // FT_OPT_OCCL_POLICY: 0 = the shipped schedule (FT_OCCL_PERIOD ...)
    int optOrder = 1;                                      // FT_OPT_ORDER: 1 = frames hand their heavy tiles out first, from the costs the scene's last launch of the same grid recorded; 2 = record only; 0 = off
    int optTryHint = 1;                                    // FT_OPT_TRY_HINT: 1 = a frame's tiles schedule their bundle-certificate tries from what the scene's last launch of the same grid recorded per tile; 2 = record only; 0 = off
    int optDepart = 1;                                     // FT_OPT_DEPART: 1 = the launches that follow try hints try their shadow rays' miss certificate at birth under the margin that grows along the ray; 2 = every lean launch that passes the gate; 0 = off
    int fieldBrick = -1;                                   // brick shape of the lattice launches: -1 by kernel family (launchField), else an index into FT_FIELD_BRICKS (ft_ctx_field_brick: the probe's shapes)
    uint32_t meshTile = FT_MESH_TILE_DEFAULT;              // lattice points per workgroup of the mesher's kernels (ft_ctx_mesh_tile: the probe's tiles)
    uint32_t sliceTile = FT_SLICE_TILE_DEFAULT;            // items per workgroup of the slicer's tiled kernels (ft_ctx_slice_tile: the tests' and the probe's tiles)
    int sliceStop = 0;                                     // 0: whole extractions; 1 / 2: they end after the link kernel / the jump rounds, empty (ft_ctx_slice_probe: the probe's stages)
    int64_t sliceLast[2] = {0, 0};                         // vertices and jump rounds R of the context's last extraction (ft_ctx_slice_probe)
    void* sliceWork = nullptr; size_t sliceWorkBytes = 0;  // the slicer's per-vertex work (sized after its first totals, when the scratch still holds the lattice)
    void* refineWork = nullptr; size_t refineWorkBytes = 0; // the refinement's per-bracket work (FT_REFINE_ITEM_BYTES each; sized from the vertex total the constructor reads, or from a segment count)
    uint32_t shellsTile = FT_SHELLS_TILE_DEFAULT;          // items per workgroup of the shell labelling's tiled kernels (ft_ctx_shells_tile: the tests' and the probe's tiles)
    int shellsStop = 0;                                    // 0: whole labellings; 1 / 2 / 3: they end after the incidence lists / the iterations / the vertex labels, with no shell (ft_ctx_shells_probe: the probe's stages)
    int64_t shellsLast[2] = {0, 0};                        // iterations and synchronisations of the context's last labelling (ft_ctx_shells_last)
    void* shellsWork = nullptr; size_t shellsWorkBytes = 0; // the shell labelling's and the selection's work (ft_shells.h says how much per vertex and triangle)
    void* measureWork = nullptr; size_t measureWorkBytes = 0; // the measures' per-shell sums, box keys, counters and staged records (ft_measure.h says how much per shell)
    int measureStop = 0, measureEager = 0;                 // ft_ctx_measure_probe (the probe's stages): calls end after the extent kernel (1) or the terms kernel (2) and write no record; the terms kernel flushes at every iteration
    unsigned measureGrid = 0;                              // 0: the measures' kernels fill the device; else their workgroups (ft_ctx_measure_grid: the tests' and the probe's grids)
    void* contourWork = nullptr; size_t contourWorkBytes = 0; // the contour measures' per-polyline and per-slice sums, box keys, counters and staged records (ft_contour_measure.h says how much)
    int contourEager = 0;                                  // ft_ctx_contour_measure_probe: the terms kernel adds every lane's terms by itself
    unsigned contourGrid = 0;                              // 0: the contour measures' kernels fill the device; else their workgroups (ft_ctx_contour_measure_grid)
    int refineSkipField = 0;                               // 1: a refinement launches everything but its field rounds, and gives other positions (ft_ctx_refine_probe: the probe's stages)
    uint32_t orderNum = 1, orderDen = 1;                   // a tile is heavy from orderNum / orderDen of the mean cost on (ft_ctx_tile_order_rule: the probes' other rules)
};

// FT_OPT_ORDER: what a scene keeps per render lane between two frame launches (launchTrace; kernels.hip "Tile order").  cost, order and work are one
// allocation; key is everything that fixes the tile grid and the kernel of the launch that recorded cost — not the camera, epsilon, Length or lights:
// an order made for another view is only another permutation.
// FT_OPT_TRY_HINT: hint is the third array of that allocation, one word per tile (ft_kernels.h "Try hints"), under the same key: a hint made for another view only
// moves a tile's tries.
struct TileOrderKey {
    int32_t W, H, x0, nCols;
    uint32_t stripeW, stripeRanks, stripeRank, nJobs, variant, libm;
    bool operator==(const TileOrderKey& o) const {
        return W == o.W && H == o.H && x0 == o.x0 && nCols == o.nCols && stripeW == o.stripeW && stripeRanks == o.stripeRanks && stripeRank == o.stripeRank &&
               nJobs == o.nJobs && variant == o.variant && libm == o.libm;
    }
};
struct TileOrderSlot {
    uint32_t* cost = nullptr; uint32_t* order = nullptr; uint32_t* hint = nullptr; void* work = nullptr;
    uint32_t capTiles = 0;
    bool keyed = false, hasOrder = false;                  // key describes cost; order was built from cost
    float hintCam[12] = {};                                // the camera of the launch that filled hint: a launch follows the words only from a view close to it (tileOrder)
    bool hasHint = false, usedHint = false; TileOrderKey hintKey{};   // usedHint: that launch followed the words before it; a launch of hintKey's grid filled hint (its own flag and key: FT_OPT_ORDER = 0 clears keyed and records no costs)
    bool usedOrder = false;                                // the launch that recorded cost handed its tiles out in an order (ft_scene_tile_order_used)
    TileOrderKey key{};
};

struct ft_scene {
    ft_ctx* ctx = nullptr;
    ft::FlatScene flat;
    void* dBlob = nullptr;
    FtSceneDev dev{};
    const float* dMaterialsExt = nullptr;    // EXTENSION table, handed to the kernel through FtRenderArgs
    const int32_t* dMatHandles = nullptr;    // EXTENSION ft_render_hits: dense material index -> context handle (FlatScene::materialHandles)
    FtCarve carve{};                         // fastPath == 3: tail + device pointers of the terminated candidate lists
    bool usesExpLog = false;                 // the program has a unionSmooth (SdfForm.fs:80,82): the only place FT_OPT_MATH matters while tracing
    mutable TileOrderSlot orderSlots[2];     // FT_OPT_ORDER: per render lane (each lane has its own stream and job counter, so two launches in flight never share one)
};

namespace {

int requireDevice(ft_ctx* c) {
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (!c->hasDevice) return setErr(FT_ERR_NO_DEVICE, "context has no GPU: libfraytracer_hip has no CPU fallback");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hipFail(e, "hipSetDevice");
    return FT_OK;
}

// the context's device buffers (scratch, aux, planes, cams) only ever grow
int ensureBytes(void*& p, size_t& have, size_t need) {
    if (need <= have) return FT_OK;
    if (p) { HIP_TRY(hipFree(p)); p = nullptr; have = 0; }
    HIP_TRY(hipMalloc(&p, need));
    have = need;
    return FT_OK;
}
int ensureScratch(ft_ctx* c, size_t bytes) { return ensureBytes(c->scratch, c->scratchBytes, bytes); }
int ensureAux(ft_ctx* c, size_t bytes) { return ensureBytes(c->aux, c->auxBytes, bytes); }

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Device-side per-cell grid build (kernels.hip ft_grid_build_kernel).  Declines (host build) for tiny grids,
// more than FT_GRID_BUILD_MAX_ITEMS items or a scratch need above 512 MB.
struct DeviceGridFiller : ft::GridFiller {
    ft_ctx* c;
    explicit DeviceGridFiller(ft_ctx* ctx) : c(ctx) {}
    bool fill(ft::HostGrid& g, const std::vector<ft::Boundary>& bounds, float halfDiag, std::string& err) override {
        const size_t n = bounds.size(), ncells = g.centers.size();
        const size_t tmpBytes = ncells * n * sizeof(FtItem);
        if (n > FT_GRID_BUILD_MAX_ITEMS || ncells * n < 100000 || tmpBytes > ((size_t)512 << 20)) return false;
        if (hipSetDevice(c->device) != hipSuccess) return false;
        const size_t oB = 0, oC = align256(oB + n * 16), oN = align256(oC + ncells * 12), oS = align256(oN + ncells * 4),
                     oF = align256(oS + (ncells + 1) * 4), oT = align256(oF + 256), total = oT + tmpBytes;
        if (ensureScratch(c, total) != FT_OK) return false;
        unsigned char* base = static_cast<unsigned char*>(c->scratch);
        std::vector<float> hb(n * 4);
        for (size_t i = 0; i < n; ++i) { hb[4 * i] = bounds[i].center.x; hb[4 * i + 1] = bounds[i].center.y; hb[4 * i + 2] = bounds[i].center.z; hb[4 * i + 3] = bounds[i].radius; }
        auto ok = [](hipError_t e) { return e == hipSuccess; };
        if (!ok(hipMemcpyAsync(base + oB, hb.data(), n * 16, hipMemcpyHostToDevice, c->stream)) ||
            !ok(hipMemsetAsync(base + oF, 0, 4, c->stream))) return false;
        FtGridBuildArgs a{};
        a.bounds = reinterpret_cast<const float*>(base + oB); a.n = (uint32_t)n; a.c = (uint32_t)g.count[0];
        a.aabbMin[0] = g.aabbMin.x; a.aabbMin[1] = g.aabbMin.y; a.aabbMin[2] = g.aabbMin.z;
        a.cellSize[0] = g.cellSize.x; a.cellSize[1] = g.cellSize.y; a.cellSize[2] = g.cellSize.z; a.halfDiag = halfDiag;
        a.centers = reinterpret_cast<float*>(base + oC); a.counts = reinterpret_cast<uint32_t*>(base + oN);
        a.tmp = reinterpret_cast<FtItem*>(base + oT); a.flags = reinterpret_cast<uint32_t*>(base + oF);
        if (!ok(ft_launch_grid_build(&a, c->stream))) return false;
        std::vector<uint32_t> counts(ncells);
        uint32_t flags = 0;
        if (!ok(hipMemcpyAsync(counts.data(), base + oN, ncells * 4, hipMemcpyDeviceToHost, c->stream)) ||
            !ok(hipMemcpyAsync(&flags, base + oF, 4, hipMemcpyDeviceToHost, c->stream)) ||
            !ok(hipMemcpyAsync(g.centers.data(), base + oC, ncells * 12, hipMemcpyDeviceToHost, c->stream)) ||
            !ok(hipStreamSynchronize(c->stream))) return false;
        if (flags & 1u) { err = "union: NaN boundary"; return false; }
        if (flags & 2u) { err = "union: a lookup cell has no candidates (the reference would throw at Items.[0])"; return false; }
        uint32_t total_items = 0;
        for (size_t ci = 0; ci < ncells; ++ci) { g.cellStart[ci] = total_items; total_items += counts[ci]; }
        g.cellStart[ncells] = total_items;
        g.items.resize(total_items);
        FtItem* dItems = nullptr;                                       // CSR items, exact size
        if (!ok(hipMalloc((void**)&dItems, std::max<size_t>(16, (size_t)total_items * sizeof(FtItem))))) return false;
        const bool done =
            ok(hipMemcpyAsync(base + oS, g.cellStart.data(), (ncells + 1) * 4, hipMemcpyHostToDevice, c->stream)) &&
            ok(ft_launch_grid_compact(a.tmp, reinterpret_cast<const uint32_t*>(base + oS), (uint32_t)ncells, (uint32_t)n, dItems, c->stream)) &&
            ok(hipMemcpyAsync(g.items.data(), dItems, (size_t)total_items * sizeof(FtItem), hipMemcpyDeviceToHost, c->stream)) &&
            ok(hipStreamSynchronize(c->stream));
        (void)hipFree(dItems);
        return done;
    }
};

// One vector of a scene's blob: where it lies (256-byte aligned, never empty) and what is copied there
struct BlobPart { size_t at; const void* data; size_t bytes; };
template <class T> BlobPart placed(size_t& cursor, const std::vector<T>& v) {
    const BlobPart p{cursor, v.data(), v.size() * sizeof(T)};
    cursor = align256(cursor + std::max<size_t>(p.bytes, 16));
    return p;
}

int uploadScene(ft_ctx* c, ft_scene* s) {
    const ft::FlatScene& f = s->flat;
    size_t cur = 0;
    const BlobPart instr = placed(cur, f.instr), consts = placed(cur, f.consts), grids = placed(cur, f.grids),
                   kids = placed(cur, f.children), ctr = placed(cur, f.cellCenters), start = placed(cur, f.cellStart),
                   items = placed(cur, f.items), lights = placed(cur, f.lights), mats = placed(cur, f.materials),
                   matX = placed(cur, f.materialsExt), itemsT = placed(cur, f.itemsT), startT = placed(cur, f.cellStartT),
                   matH = placed(cur, f.materialHandles), certCl = placed(cur, f.certCl);
    std::vector<unsigned char> host(cur, 0);
    for (const BlobPart& p : {instr, consts, grids, kids, ctr, start, items, lights, mats, matX, itemsT, startT, matH, certCl})
        if (p.bytes) memcpy(host.data() + p.at, p.data, p.bytes);
    FtSceneDev& d = s->dev;
    d = f.hdr;                                             // every scalar as the flattener left it; what the blob holds follows: the lights' count, the pointers
    d.nLights = (uint32_t)f.lights.size();
    if (!c->hasDevice) return FT_OK;                       // host-only context: introspection only
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(&s->dBlob, cur));
    HIP_TRY(hipMemcpy(s->dBlob, host.data(), cur, hipMemcpyHostToDevice));
    unsigned char* b = static_cast<unsigned char*>(s->dBlob);
    d.instr = reinterpret_cast<const FtInstr*>(b + instr.at);
    d.consts = reinterpret_cast<const float*>(b + consts.at);
    d.grids = reinterpret_cast<const FtGrid*>(b + grids.at);
    d.children = reinterpret_cast<const FtChild*>(b + kids.at);
    d.cellCenters = reinterpret_cast<const float*>(b + ctr.at);
    d.cellStart = reinterpret_cast<const uint32_t*>(b + start.at);
    d.items = reinterpret_cast<const FtItemRec*>(b + items.at);
    d.lights = reinterpret_cast<const FtLight*>(b + lights.at);
    d.materials = reinterpret_cast<const float*>(b + mats.at);
    s->dMaterialsExt = reinterpret_cast<const float*>(b + matX.at);
    s->dMatHandles = reinterpret_cast<const int32_t*>(b + matH.at);
    d.certCl = reinterpret_cast<const float*>(b + certCl.at);
    s->carve = f.carve;
    s->carve.itemsT = reinterpret_cast<const FtItemRec*>(b + itemsT.at);
    s->carve.cellStartT = reinterpret_cast<const uint32_t*>(b + startT.at);
    return FT_OK;
}

// Latency-mode thresholds (rays per wave at or below which each ray is evaluated by all 64 lanes; measured)
// miss certificate (FT_OPT_CERT_POLICY layout): primary rays from their first evaluation, shadow rays from their 6th step, a wave runs the certificate
// once 16 of its lanes are due, and a ray it fails on is due again 6 steps later (DESIGN.md section 4 "Miss certificate": the policies measured)
constexpr int FT_CERT_POLICY_DEFAULT = 0 | (6 << 8) | (16 << 16) | (6 << 24);
// the bundle certificate's shipped schedule (bits 30-31 of the policy word = 0): every 2nd evaluation round of a wave, from one primary ray on, and from one
// shadow ray of 2 or more steps on (DESIGN.md section 5 "Bundle certificate on C3": the schedules measured)
constexpr uint32_t FT_BUNDLE_PERIOD = 2u, FT_BUNDLE_MIN = 1u, FT_BUNDLE_SHADOW = 2u;
// the occlusion certificate's shipped schedule (FT_OPT_OCCL_POLICY = 0): every 2nd evaluation round of a wave, for the shadow rays that have come into being
// since its last try, from one such ray on (DESIGN.md section 5 "Occlusion certificate on C3": the schedules measured)
constexpr uint32_t FT_OCCL_PERIOD = 2u, FT_OCCL_MIN = 1u;
constexpr int FT_TAIL_K_LEAN = 32, FT_TAIL_K_GENERAL = 2, FT_TAIL_K_CARVED = 1;      // carved: 1.26 ms at 0 / 1 against 1.29 at 2 on the 1000^2 Program.fs frame (profiles/r04_carved_variants.txt)
// does this launch take the glibc build of the kernels?
bool libmLaunch(const ft_ctx* c, const ft_scene* s) { return c->optMath != FT_MATH_FIXED && s->usesExpLog; }

// What a trace launch runs: the kernel family (FtSceneDev.fastPath of the launch; kernels.hip ft_trace_kernel_for), its arithmetic, its value slots,
// whether the wave rows for culled children are kept, and the LDS footprint (ft_lds_layout).  The only place these rules live:
//   * a carved union takes the general kernels for EXTENSION launches, with FT_OPT_CARVED = 0 and with glibc math: the carved kernels have no such builds;
//   * the lean and the carved kernels keep their values in registers and are launched with nSlots = 0 — for the lean kernel 2 KB per workgroup
//     that decide between 6 and 7 resident workgroups per CU (every other user of a lean scene, ft_eval_distance, runs the general interpreter);
//   * one row per wave behind everything: the lean kernel's latency mode and culled children; any other non-carved kernel's culled children where
//     the scene has a cull site.  Those are optional: without them the culling pass is off, so they are dropped where the footprint would exceed
//     the device's limit.  A scene too large even then is refused here, not by a launch failure.
//   * ft_shade_hits (shade) follows the same rules with the *_shade twins: no EXTENSION launch exists, so a carved union leaves the carved walk
//     only with FT_OPT_CARVED = 0 or glibc math, exactly where a ft_trace_rays of the scene does.  ft_light_visibility (shade = 2) is the same
//     marches with another result, so the same rules with the *_vis twins.
//   * a field launch (launchField: ft_sample_points, ft_sample_lattice) runs the same evaluators, so it plans like a plain trace launch (ext = false,
//     shade = 0) and looks its kernel up by the plan's variant and arithmetic (kernels.hip FT_FIELD_BUILDS, which has no EXTENSION build either).
struct KernelPlan { unsigned variant; bool libm, cullRows; uint32_t nSlots; size_t lds; };
int planTrace(const ft_ctx* c, const ft_scene* s, bool ext, unsigned shade, KernelPlan& p) {
    const bool hasCull = s->dev.cullPc != 0xffffffffu;
    if (shade && ext) return setErr(FT_ERR_INVALID, "internal: ft_shade_hits has no EXTENSION build");
    p.libm = libmLaunch(c, s);
    p.variant = (s->dev.fastPath == 3u && (ext || !c->optCarved || p.libm)) ? 0u : s->dev.fastPath;
    p.nSlots = (p.variant == 1u || p.variant == 3u) ? 0u : s->dev.nSlots;
    p.cullRows = p.variant == 1u || (p.variant != 3u && hasCull);
    int maxLds = 0;
    HIP_TRY(hipDeviceGetAttribute(&maxLds, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    p.lds = 4u * (size_t)ft_lds_layout(p.nSlots, s->dev.nStage, p.libm, p.cullRows).total;
    if (p.lds > (size_t)maxLds && p.variant != 1u && p.cullRows) {
        p.cullRows = false;
        p.lds = 4u * (size_t)ft_lds_layout(p.nSlots, s->dev.nStage, p.libm, false).total;
    }
    if (p.lds > (size_t)maxLds) return setErr(FT_ERR_UNSUPPORTED, "scene needs " + std::to_string(p.lds) + " bytes of LDS per workgroup; the device offers " + std::to_string(maxLds));
    return FT_OK;
}

// A frame loop that never calls ft_collect_stats must not grow the event list: beyond this many pending pairs the
// oldest one is folded into foldedMs (it has long completed: launches on one stream finish in order) and recycled.
constexpr size_t FT_MAX_PENDING_EVENTS = 64;
int foldOldestEvents(ft_ctx* c) {
    while (c->events.size() >= FT_MAX_PENDING_EVENTS) {
        auto p = c->events.front();
        HIP_TRY(hipEventSynchronize(p.second));
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, p.first, p.second));
        c->foldedMs += t;
        c->eventPool.push_back(p);
        c->events.erase(c->events.begin());
    }
    return FT_OK;
}

int acquireEvents(ft_ctx* c, hipEvent_t& a, hipEvent_t& b) {
    if (!c->eventPool.empty()) { a = c->eventPool.back().first; b = c->eventPool.back().second; c->eventPool.pop_back(); return FT_OK; }
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    return FT_OK;
}

// One timed launch on `stream`, stated once: the oldest pending pairs are folded, `launch` (a callable that returns the launch's hipError_t; `what`
// names it in a failure's message) runs between the two events of a pair, and the pair joins the pending ones that ft_collect_stats adds up.  Once
// the pair is acquired a failure returns it to the pool.
template <class Launch> int timedLaunch(ft_ctx* c, hipStream_t stream, const char* what, Launch launch) {
    int rc = foldOldestEvents(c); if (rc) return rc;
    hipEvent_t e0, e1;
    if ((rc = acquireEvents(c, e0, e1))) return rc;
    const char* at = "hipEventRecord";
    hipError_t e = hipEventRecord(e0, stream);
    if (e == hipSuccess && (e = launch()) != hipSuccess) at = what;
    if (e == hipSuccess) e = hipEventRecord(e1, stream);
    if (e != hipSuccess) { c->eventPool.emplace_back(e0, e1); return hipFail(e, at); }
    c->events.emplace_back(e0, e1);
    return FT_OK;
}

// The workgroups per CU a launch plans with, from what the occupancy query found for the kernel (`kernel` names it in the refusal): none is refused,
// more than 8 are not used, and FT_OPT_MAX_BLOCKS_PER_CU (experiments) caps them
int clampPerCU(const ft_ctx* c, const char* kernel, int& perCU) {
    if (perCU < 1) return setErr(FT_ERR_UNSUPPORTED, std::string("the ") + kernel + " kernel does not fit a compute unit with this scene's LDS footprint");
    perCU = std::min(perCU, 8);
    if (c->optMaxBlocksPerCU > 0) perCU = std::min(perCU, c->optMaxBlocksPerCU);
    return FT_OK;
}

// FT_OPT_ORDER: the slot of this launch with room for its tiles, nullptr where it cannot be had (the launch then runs in index order and records nothing)
TileOrderSlot* tileOrderSlot(const ft_scene* s, int lane, uint32_t nTiles) {
    TileOrderSlot& t = s->orderSlots[lane];
    if (t.capTiles >= nTiles) return &t;
    if (t.cost) (void)hipFree(t.cost);                    // waits for whatever still uses it
    t = TileOrderSlot{};
    const size_t words = 3 * (size_t)nTiles, bytes = align256(words * sizeof(uint32_t)) + ft_tile_order_work_bytes(nTiles);
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    t.cost = static_cast<uint32_t*>(p);
    t.order = t.cost + nTiles;
    t.hint = t.order + nTiles;
    t.work = static_cast<unsigned char*>(p) + align256(words * sizeof(uint32_t));
    t.capTiles = nTiles;
    return &t;
}

// ---- launchTrace's rules, one function each -------------------------------------------------------------------------------------------------

// Grid size: the workgroups of a launch of `key` over nJobs jobs — what the occupancy query allows per CU (clampPerCU), less on small frames, and
// never more than the jobs fill.
// Small frames: the job queue can only even out the load while there are several tiles per resident wave, and the grid-union kernels lose little
// throughput at half their occupancy (the 4000^2 Program.fs frame: 5.4 ms at 7 workgroups per CU, 6.0 at 4).  With about as many tiles as waves
// every tile is handed out at once, the heavy ones sit several deep on some SIMDs while others idle, and the frame lasts as long as the
// slowest of them at full contention.  So: about one resident wave per four tiles, at least two workgroups per CU (measured per size,
// profiles/r04_blocks_by_frame_size.jsonl: the reference's own 1000^2 frame 1.45 -> 1.27 ms, C2 at 1024^2 0.90 -> 0.61 ms).
int gridSize(const ft_ctx* c, const FtTraceKey& key, const KernelPlan& plan, uint32_t nJobs, unsigned& blocks) {
    int perCU = 0;
    HIP_TRY(ft_trace_occupancy(key, plan.lds, &perCU));
    int rc = clampPerCU(c, "trace", perCU); if (rc) return rc;
    if (c->optMaxBlocksPerCU <= 0 && key.variant != 1u) {
        const uint64_t tiles = ((uint64_t)nJobs + (uint64_t)c->optChunk - 1) / (uint64_t)c->optChunk;
        const uint64_t wavesPerLayer = (uint64_t)c->numCUs * (FT_BLOCK / 64);
        const uint64_t want = (tiles + 2 * wavesPerLayer) / (4 * wavesPerLayer);              // round(tiles / (4 x waves of one workgroup per CU))
        perCU = (int)std::min<uint64_t>((uint64_t)perCU, std::max<uint64_t>(2, want));
    }
    const uint64_t maxBlocks = (uint64_t)c->numCUs * perCU;
    const uint64_t wantBlocks = ((uint64_t)nJobs + FT_BLOCK - 1) / FT_BLOCK;
    blocks = (unsigned)std::max<uint64_t>(1, std::min(maxBlocks, wantBlocks));
    return FT_OK;
}

// Hand-out: how the waves of `blocks` workgroups take jobs from the queue.
//   chunk      one 8x8 tile per grab: measured faster than larger chunks (lanes of a wave stay on neighbouring
//              pixels) and 2.6e5 atomics per 4096^2 frame are far below the rate one counter sustains
//   refillMin  burst refill (kernels.hip): a wave takes new rays only when all 64 lanes are idle, i.e. it works through one 8x8 tile at a
//              time.  Measured (profiles/r02_refill_sweep.txt, kernel ms at refillMin = 1 / 32 / 64): 1000-torus scene 4000^2 22.5 /
//              15.8 / 12.1, at 1000^2 2.98 / 2.72 / 2.24, C2 4096^2 4.90 / 4.40 / 3.84, 300 on-demand combinators 24.6 / 14.8 / 10.3,
//              glass config 39.1 / 31.5 / 27.3, and even the VALU-bound C3 kernel 61.0 / 66.5 / 60.3: rays that start together stay in
//              step (march, the four normal probes, shadow rays), so a wave's lanes share lookup cells, list positions and branches.
//              64 unless FT_OPT_REFILL_MIN says otherwise (experiments)
//   tailK      the latency mode's threshold, per kernel family unless FT_OPT_TAIL_K sets it (FT_TAIL_K_*)
//   shrink1/2  guided hand-out of the last jobs (kernels.hip refill): one half tile, then one quarter tile per resident wave — only where the latency
//              mode makes a part-filled wave cheap (lean kernel, tailK >= 32) and only for the reference's sampling (tile-major job order)
void handOut(const ft_ctx* c, const ft_scene* s, unsigned variant, unsigned blocks, FtRenderArgs& a) {
    a.chunk = (uint32_t)c->optChunk;
    a.refillMin = (uint32_t)c->optRefillMin;
    a.tailK = (uint32_t)(c->optTailK >= 0 ? c->optTailK : (variant == 1u ? FT_TAIL_K_LEAN : variant == 3u ? FT_TAIL_K_CARVED : FT_TAIL_K_GENERAL));
    a.shrink1 = a.shrink2 = a.nJobs;
    if (s->dev.fastPath == 1u && a.tailK >= 32u && c->optGuided && a.mode == 0u) {
        const uint64_t waves = (uint64_t)blocks * (FT_BLOCK / 64);
        const uint64_t q = waves * (a.chunk / 4u), h = waves * (a.chunk / 2u);
        if ((uint64_t)a.nJobs > 4u * (q + h)) { a.shrink2 = (uint32_t)(a.nJobs - q); a.shrink1 = (uint32_t)(a.nJobs - q - h); }
    }
}

// FT_OPT_CERT_POLICY, the word's only decoder: bits 0-7 the step a primary ray is due from and 8-15 a shadow ray's (255: never), 16-23 the due lanes a
// wave waits for, 24-29 the steps after which a ray the certificate failed on is due again, 30-31 the bundle certificate's schedule — 0 shipped,
// 1 every round from one member on, 2 every second round, 3 off
struct CertPolicy { uint32_t prim, shadow, minLanes, repeat, bundle; };
CertPolicy decodeCertPolicy(uint32_t w) {
    return CertPolicy{(w & 255u) == 255u ? ~0u : (w & 255u), ((w >> 8) & 255u) == 255u ? ~0u : ((w >> 8) & 255u), (w >> 16) & 255u, (w >> 24) & 63u, w >> 30};
}

// FT_OPT_OCCL_POLICY, the word's only decoder: bits 0-7 the period in evaluation rounds (0: shipped, 255: off), 8-15 the steps a shadow ray takes before its
// try, 16-23 the candidates a try waits for (0: shipped)
struct OcclPolicy { uint32_t period, from, minLanes; };
OcclPolicy decodeOcclPolicy(uint32_t w) { return OcclPolicy{w & 255u, (w >> 8) & 255u, (w >> 16) & 255u}; }

// Miss certificate and bundle certificate: lean kernel (and its EXTENSION build: a render and its ft_render_hits twin count the same evaluations), only
// with the escape shortcut (it rests on the same support sphere and drift bound), on a scene that has one (certM >= 0).
// Tile-width rule: word 0 on a camera frame whose 8x8 tiles are narrower, at the far side of the support sphere, than the margin certM that every certificate concedes anyway:
// the bundle's width W stays below certM, so its bound loses next to nothing against its members' own and the per-lane tries only cost; they are left
// out (what 255 / 255 in an explicit word asks for).  Wider tiles (smaller frames, wider lenses), views and ray buffers keep both.  Measured on either
// side of the criterion, by frame size, lens and scene: DESIGN.md section 5 "Bundle certificate on C3", profiles/r06_bundle_certificate_tile_width.txt
void certSchedule(const ft_ctx* c, const ft::FlatScene& f, unsigned variant, FtRenderArgs& a) {
    const CertPolicy pol = decodeCertPolicy((uint32_t)(c->optCertPolicy != 0 ? c->optCertPolicy : FT_CERT_POLICY_DEFAULT));
    a.cert = (variant == 1u && c->optEscape && c->optCert && f.hdr.certM >= 0.0f) ? 1u : 0u;
    a.certPrim = pol.prim; a.certShadow = pol.shadow; a.certMin = pol.minLanes; a.certRepeat = pol.repeat;
    a.bundlePeriod = pol.bundle == 0u ? FT_BUNDLE_PERIOD : pol.bundle == 3u ? 0u : pol.bundle;
    a.bundleMin = pol.bundle == 0u ? FT_BUNDLE_MIN : 1u;
    a.bundleShadow = pol.bundle == 0u ? FT_BUNDLE_SHADOW : pol.bundle == 2u ? 2u : 0u;
    if (c->optCertPolicy == 0 && a.cert && a.mode == 0u && a.views == nullptr && a.maxSize > 0.0f) {
        const float* cm = a.cam;
        const double dx = (double)cm[0] - f.hdr.escC[0], dy = (double)cm[1] - f.hdr.escC[1], dz = (double)cm[2] - f.hdr.escC[2];
        auto len = [cm](int i) { return std::sqrt((double)cm[i] * cm[i] + (double)cm[i + 1] * cm[i + 1] + (double)cm[i + 2] * cm[i + 2]); };
        const double up = len(6), rt = len(9), fw = len(3);
        const double reach = std::sqrt(dx * dx + dy * dy + dz * dz) + (double)f.hdr.escR;
        const double tile = 8.0 * std::max(up, rt) / (double)a.maxSize * reach / fw;                // an 8x8 tile's side at distance `reach`
        if (fw > 0.0 && tile <= (double)f.hdr.certM) a.certPrim = a.certShadow = 0xffffffffu;
    }
}

// Occlusion certificate: where the miss certificate runs (a.cert: the lean kernel, the escape shortcut — the same support sphere and per-step drift — and
// FT_OPT_CERT, which switches every certificate: with it off a launch evaluates exactly what its rays' marches ask for), with FT_OPT_OCCL, on a scene
// that has one (occ.b >= 0).  A ray's first evaluation taken from the cache (FT_OPT_REUSE, a.reuse) is its step 0: it comes into being with one step taken.
void occlSchedule(const ft_ctx* c, const ft::FlatScene& f, FtRenderArgs& a) {
    const OcclPolicy pol = decodeOcclPolicy((uint32_t)c->optOcclPolicy);
    const bool on = a.cert && c->optOccl && f.occ.b >= 0.0f && pol.period != 255u;
    a.occPeriod = on ? (pol.period != 0u ? pol.period : FT_OCCL_PERIOD) : 0u;
    a.occFrom = pol.from + a.reuse;
    a.occMin = pol.minLanes != 0u ? pol.minLanes : FT_OCCL_MIN;
    a.occ = f.occ;
}

// FT_OPT_ORDER.  Eligible: a frame of whole tiles taken one at a time, on the kernel that keeps the bookkeeping (the lean kernel).
// An eligible launch records what each tile cost.  Where the slot's last launch had the same grid and kernel, it also hands the tiles out in
// the order built from that launch's costs.  A context with FT_OPT_GUIDED set is never eligible: the guided hand-out changes the grab size.
// A launch that is not eligible leaves the slot alone.  -> the slot the launch records into, nullptr: none
// (With FT_OPT_ORDER = 0 and FT_OPT_TRY_HINT on, the slot is still allocated and a.tileCost set — the kernel records hints where it records costs — so
// the kernel writes costs nobody reads: the slot stays unkeyed for the order and ft_scene_tile_costs reports none.)
// FT_OPT_TRY_HINT.  The same launches are eligible, and record per tile the rounds their bundle certificates held on (the kernel writes them where it writes
// the costs, so a.tileCost is set for them too).  A launch follows the words of the slot's last launch where that had the same grid and kernel AND its
// certificate schedule is word 0 of FT_OPT_CERT_POLICY with the per-lane tries left out (certSchedule's tile-width rule): an explicit word is taken as it
// stands, and a wide-tiled frame keeps the schedule its evaluation counts are known by.  A slot that cannot be had leaves the frame unhinted.
// The view must also be close to the one the words were recorded from: measured on C3 at 4096^2, a camera turned by 1 or 8 pixels a frame gains from
// its last frame's hints and one turned by 64 pixels a frame loses (+0.8 % sdf_evals, +2 % kernel time: holds found up to three rounds late), so a launch whose
// image moved by more than FT_HINT_MAX_SHIFT pixels, two tiles, records and does not follow.
constexpr double FT_HINT_MAX_SHIFT = 16.0;
// An upper estimate, in pixels, of how far the image of the scene moves between two cameras (12 floats each: position, forward, up, right as scaled):
// the turn of the forward direction, the change of the up and right vectors at the frame's edge, and the move of the position seen from the near side
// of the support sphere, each over one pixel's size at unit distance.  +inf where it cannot be told.
double cameraShiftPixels(const float* p, const float* q, float maxSize, const ft::FlatScene& f) {
    auto len = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    double d[4][3], fp[3], fq[3], ec[3];
    for (int v = 0; v < 4; ++v) for (int i = 0; i < 3; ++i) d[v][i] = (double)q[3 * v + i] - (double)p[3 * v + i];
    for (int i = 0; i < 3; ++i) { fp[i] = p[3 + i]; fq[i] = q[3 + i]; ec[i] = (double)q[i] - f.hdr.escC[i]; }
    const double lp = len(fp), lq = len(fq);
    const double up[3] = {q[6], q[7], q[8]}, rt[3] = {q[9], q[10], q[11]};
    const double side = std::max(len(up), len(rt));
    if (!(lp > 0.0) || !(lq > 0.0) || !(side > 0.0) || !(maxSize > 0.0f)) return INFINITY;
    const double pixel = side / (double)maxSize / lq;                                      // as certSchedule prices a tile
    const double turn[3] = {fq[0] / lq - fp[0] / lp, fq[1] / lq - fp[1] / lp, fq[2] / lq - fp[2] / lp};
    const double nearSide = std::max(len(ec) - (double)f.hdr.escR, 0.1 * (double)f.hdr.escR);
    const double moved = len(d[0]);
    if (moved > 0.0 && !(nearSide > 0.0)) return INFINITY;
    const double shift = len(turn) / pixel + (len(d[2]) + len(d[3])) / side * 0.5 * (double)maxSize + (moved > 0.0 ? moved / nearSide / pixel : 0.0);
    return shift == shift ? shift : INFINITY;
}
TileOrderSlot* tileOrder(const ft_ctx* c, const ft_scene* s, int lane, const FtTraceKey& key, FtRenderArgs& a) {
    a.tileCost = nullptr; a.tileOrder = nullptr; a.tileHint = nullptr; a.tryHint = 0u;
    TileOrderSlot* slot = nullptr;
    if (key.form == FT_FORM_FRAME && !key.ext && key.variant == 1u && a.mode == 0u && a.spp == 1u && a.chunk == 64u && a.refillMin == 64u && !c->optGuided && a.shrink1 == a.nJobs && a.nJobs >= 64u) {
        if (c->optOrder == 0) { s->orderSlots[lane].keyed = s->orderSlots[lane].hasOrder = s->orderSlots[lane].usedOrder = false; }
        if (c->optTryHint == 0) s->orderSlots[lane].hasHint = false;
        if (c->optOrder != 0 || c->optTryHint != 0) slot = tileOrderSlot(s, lane, a.nJobs >> 6);
    }
    if (slot) {
        const TileOrderKey k{a.W, a.H, a.x0, a.nCols, a.stripeW, a.stripeRanks, a.stripeRank, a.nJobs, key.variant, key.libm ? 1u : 0u};
        a.tileCost = slot->cost;
        if (c->optOrder != 0) {
            if (c->optOrder == 1 && slot->keyed && slot->hasOrder && slot->key == k) a.tileOrder = slot->order;
            slot->key = k; slot->keyed = true; slot->hasOrder = false; slot->usedOrder = a.tileOrder != nullptr;
        }
        if (c->optTryHint != 0) {
            const bool bundleAlone = c->optCertPolicy == 0 && a.cert != 0u && a.bundlePeriod != 0u && a.certPrim == 0xffffffffu && a.certShadow == 0xffffffffu;
            a.tileHint = slot->hint;
            if (c->optTryHint == 1 && bundleAlone && slot->hasHint && slot->hintKey == k && cameraShiftPixels(slot->hintCam, a.cam, a.maxSize, s->flat) <= FT_HINT_MAX_SHIFT) a.tryHint = 1u;
            slot->hintKey = k; slot->hasHint = true; slot->usedHint = a.tryHint != 0u;
            memcpy(slot->hintCam, a.cam, sizeof(slot->hintCam));
        }
    }
    return slot;
}

// Departure certificate (FT_OPT_DEPART; scene.cpp "Departure certificate"): the margin of the per-lane miss certificate's tries, and where it is tilted
// their schedule.  Every launch gets the scene's flat margin (slope 0: what the per-lane tries have always conceded).  The tilted one goes to
//   1  the launches that follow try hints (a.tryHint: same slot key, a camera within FT_HINT_MAX_SHIFT, word 0, narrow tiles, FT_OPT_TRY_HINT = 1) and no
//      other: first frames, wide-tiled frames, explicit words, views, ray buffers and EXTENSION launches count what they counted, to the last evaluation
//   2  every launch of the lean family (tests, fuzz),
// where certificates run at all (a.cert), the scene has the constants, and the launch has ONE epsilon no smaller than the scene's floor: a camera launch
// (mode 0, no hit records).  slope = depE / epsilon and base = 2 depE + depB + depK slope^2 are formed here in double; a lane of another epsilon (none
// in these launches) would be left out by epsMin.  Under word 0 the shadow rays are due at the step they are born with (1 with FT_OPT_REUSE, as
// occlSchedule counts).  Where certSchedule's tile-width rule left the per-lane tries out (every launch that follows hints), primary rays stay out and a
// wave tries once FT_DEPART_MIN lanes wait, and again FT_DEPART_REPEAT steps after a failure; a wide-tiled frame (option 2 only) keeps its primary
// tries, due lanes and repeat, under the tilted margin too.  An explicit word is taken as it stands and only the margin of its tries changes.
constexpr uint32_t FT_DEPART_MIN = 16u, FT_DEPART_REPEAT = 3u;   // measured: profiles/departure_certificate_policies.txt
void departSchedule(const ft_ctx* c, const ft::FlatScene& f, FtRenderArgs& a) {
    a.dep = FtCertMargin{0.0f, 0.0f, f.hdr.certM, f.hdr.certClip, f.hdr.certLenF, 0.0f, f.hdr.certSteps, 0u};
    const bool asked = c->optDepart == 2 || (c->optDepart == 1 && a.tryHint != 0u);
    if (!(asked && a.cert != 0u && f.dep.b >= 0.0f && a.mode == 0u && a.shade == 0u && a.eps >= f.dep.epsMin && a.eps <= f.hdr.escR)) return;
    const double slope = (double)f.dep.e / (double)a.eps * (1.0 + 1e-6);
    const double base = (2.0 * (double)f.dep.e + (double)f.dep.b + (double)f.dep.k * slope * slope) * (1.0 + 1e-6);
    a.dep = FtCertMargin{(float)slope, (float)(slope / 0.9 * (1.0 + 1e-6)), (float)base, f.dep.clip, f.dep.lenF, a.eps, f.dep.steps, 0u};
    if (c->optCertPolicy == 0) {
        if (a.certShadow == 0xffffffffu) { a.certMin = FT_DEPART_MIN; a.certRepeat = FT_DEPART_REPEAT; }   // narrow tiles: the tries are the shadow rays' alone
        a.certShadow = a.reuse;
    }
}

// launch the persistent trace kernel over nJobs jobs
// lane 0 = the context's stream; lane 1 = a second stream with its own job counter, so that two launches can be in flight
// (the drain of one overlaps the start of the next: DESIGN.md section 6)
int launchTrace(ft_ctx* c, const ft_scene* s, FtRenderArgs& a, int lane = 0) {
    hipStream_t stream = lane ? c->lane1 : c->stream;
    uint32_t* counter = c->dCounter + (lane ? 16 : 0);
    KernelPlan plan;
    int rc = planTrace(c, s, a.ext != 0u, a.shade, plan); if (rc) return rc;
    // what decides the kernel (ft_kernels.h ft_trace_key; a.ext, a.views and a.shade are the caller's), then the key: the occupancy query and the
    // launch look up the same one
    a.S = s->dev; a.S.fastPath = plan.variant; a.S.nSlots = plan.nSlots;
    a.S.mathFma = c->optMath == FT_MATH_GLIBC_FMA ? 1u : 0u;
    if (!c->optEscape) a.S.escR = -1.0f;
    a.carve = s->carve; a.materialsExt = s->dMaterialsExt;
    a.math = plan.libm ? 1u : 0u;
    a.counter = counter; a.stats = c->dStats;
    a.cull = (s->dev.cullPc != 0xffffffffu && plan.cullRows && c->optCull) ? 1u : 0u;
    a.lazy = c->optLazyUnion ? 1u : 0u;
    a.reuse = (c->optReuse && !a.shade) ? 1u : 0u;     // ft_shade_hits: no centre probe ran, nothing to reuse
    const FtTraceKey key = ft_trace_key(a);
    unsigned blocks = 0;
    if ((rc = gridSize(c, key, plan, a.nJobs, blocks))) return rc;
    handOut(c, s, plan.variant, blocks, a);
    certSchedule(c, s->flat, plan.variant, a);
    occlSchedule(c, s->flat, a);
    TileOrderSlot* slot = tileOrder(c, s, lane, key, a);
    departSchedule(c, s->flat, a);
    HIP_TRY(hipMemsetAsync(counter, 0, sizeof(uint32_t), stream));
    if ((rc = timedLaunch(c, stream, "ft_launch_trace", [&] { return ft_launch_trace(&a, blocks, plan.lds, stream); }))) return rc;
    if (slot && c->optOrder == 1) {                        // behind the frame on its own stream: no synchronisation, nothing comes back to the host
        // the frame is launched whatever becomes of its order: a failure here only leaves the next frame in index order
        if (ft_launch_tile_order(slot->cost, a.nJobs >> 6, c->orderNum, c->orderDen, slot->order, slot->work, stream) == hipSuccess) slot->hasOrder = true;
        else (void)hipGetLastError();
    }
    return FT_OK;
}

// ft_ctx_set_option / ft_ctx_get_option: every option's field on ft_ctx (which holds its default), the range it accepts and the message for a
// value outside it.  Two options accept less than their range: FT_OPT_CHUNK 64, 32 or 16 only, FT_OPT_CERT_POLICY 0 or due lanes in 1 .. 64.
struct OptionSpec { int32_t id; int ft_ctx::*field; int32_t lo, hi; const char* err; };
constexpr OptionSpec kOptions[] = {
    {FT_OPT_REFILL_MIN, &ft_ctx::optRefillMin, 1, 64, "FT_OPT_REFILL_MIN: 1 .. 64"},
    {FT_OPT_MAX_BLOCKS_PER_CU, &ft_ctx::optMaxBlocksPerCU, 0, 8, "FT_OPT_MAX_BLOCKS_PER_CU: 0 (no cap) .. 8"},
    {FT_OPT_HOST_CHUNKS, &ft_ctx::optHostChunks, 0, 16, "FT_OPT_HOST_CHUNKS: 0 (automatic) .. 16"},
    {FT_OPT_HOST_PIN, &ft_ctx::optHostPin, 0, 1, "FT_OPT_HOST_PIN: 0 or 1"},
    {FT_OPT_TAIL_K, &ft_ctx::optTailK, -1, 64, "FT_OPT_TAIL_K: -1 (default), 0 (off) .. 64"},
    {FT_OPT_MATH, &ft_ctx::optMath, FT_MATH_FIXED, FT_MATH_GLIBC_SSE2, "FT_OPT_MATH: 0 fixed, 1 glibc (FMA build), 2 glibc (SSE2 build)"},
    {FT_OPT_GUIDED, &ft_ctx::optGuided, 0, 1, "FT_OPT_GUIDED: 0 or 1"},
    {FT_OPT_CHUNK, &ft_ctx::optChunk, 16, 64, "FT_OPT_CHUNK: 64, 32 or 16"},
    {FT_OPT_CULL, &ft_ctx::optCull, 0, 1, "FT_OPT_CULL: 0 or 1"},
    {FT_OPT_ESCAPE, &ft_ctx::optEscape, 0, 1, "FT_OPT_ESCAPE: 0 or 1"},
    {FT_OPT_LAZY_UNION, &ft_ctx::optLazyUnion, 0, 1, "FT_OPT_LAZY_UNION: 0 or 1"},
    {FT_OPT_CARVED, &ft_ctx::optCarved, 0, 1, "FT_OPT_CARVED: 0 or 1"},
    {FT_OPT_REUSE, &ft_ctx::optReuse, 0, 1, "FT_OPT_REUSE: 0 or 1"},
    {FT_OPT_CERT, &ft_ctx::optCert, 0, 1, "FT_OPT_CERT: 0 or 1"},
    {FT_OPT_CERT_POLICY, &ft_ctx::optCertPolicy, INT32_MIN, INT32_MAX, "FT_OPT_CERT_POLICY: 0, or bits 16-23 (due lanes) in 1 .. 64"},
    {FT_OPT_ORDER, &ft_ctx::optOrder, 0, 2, "FT_OPT_ORDER: 0 off, 1 heavy tiles first, 2 record only"},
    {FT_OPT_OCCL, &ft_ctx::optOccl, 0, 1, "FT_OPT_OCCL: 0 or 1"},
    {FT_OPT_OCCL_POLICY, &ft_ctx::optOcclPolicy, 0, 0x40ffff, "FT_OPT_OCCL_POLICY: 0, or bits 0-7 period, 8-15 first step, 16-23 candidates (0 .. 64)"},
    {FT_OPT_TRY_HINT, &ft_ctx::optTryHint, 0, 2, "FT_OPT_TRY_HINT: 0 off, 1 tries scheduled from the last frame, 2 record only"},
    {FT_OPT_DEPART, &ft_ctx::optDepart, 0, 2, "FT_OPT_DEPART: 0 off, 1 on the launches that follow try hints, 2 on every launch that passes the gate"},
};
const OptionSpec* findOption(int32_t id) {
    for (const OptionSpec& o : kOptions) if (o.id == id) return &o;
    return nullptr;
}
bool optionAccepts(const OptionSpec& o, int32_t v) {
    if (v < o.lo || v > o.hi) return false;
    if (o.id == FT_OPT_CHUNK) return v == 64 || v == 32 || v == 16;
    if (o.id == FT_OPT_CERT_POLICY) { const uint32_t mn = decodeCertPolicy((uint32_t)v).minLanes; return v == 0 || (mn >= 1u && mn <= 64u); }
    return true;
}

// The job counter is 32 bits wide: `views` views of `samples` sample planes each, 64 jobs a tile.  The only place the limit is computed.
int checkJobCount(uint64_t views, uint64_t samples, const ft_render_params* p) {
    const uint64_t tiles = (uint64_t)((p->n_columns + 7) / 8) * (uint64_t)((p->height + 7) / 8);
    if (views * samples * tiles * 64 >= 0xFFFF0000ull) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 samples in one call");
    return FT_OK;
}

int checkParams(const ft_render_params* p) {
    if (!p) return setErr(FT_ERR_INVALID, "null render params");
    if (p->width <= 0 || p->height <= 0 || p->n_columns <= 0) return setErr(FT_ERR_INVALID, "empty image");
    if (p->stripe_width <= 0 || p->stripe_ranks <= 0 || p->stripe_rank < 0 || p->stripe_rank >= p->stripe_ranks)
        return setErr(FT_ERR_INVALID, "bad stripe description");
    int sn = 1; while (sn * sn < p->spp) ++sn;
    if (p->spp < 1 || p->spp > 64 || sn * sn != p->spp) return setErr(FT_ERR_INVALID, "spp (extension) must be a square number <= 64");
    if (p->ao_samples < 0 || p->ao_samples > 16) return setErr(FT_ERR_INVALID, "ao_samples (extension) must be in [0, 16]");
    if (p->max_bounces < 0 || p->max_bounces > 64) return setErr(FT_ERR_INVALID, "max_bounces (extension) must be in [0, 64]");
    if (p->spectral < 0 || p->spectral > 16 || (p->spectral > 0 && p->spp % p->spectral != 0))
        return setErr(FT_ERR_INVALID, "spectral (extension) must be in [0, 16] and divide spp");
    // last local column must map inside the image
    const int64_t c = (int64_t)p->n_columns - 1;
    const int64_t x = p->x0 + (c / p->stripe_width) * (int64_t)p->stripe_width * p->stripe_ranks + (int64_t)p->stripe_rank * p->stripe_width + c % p->stripe_width;
    if (p->x0 < 0 || x >= p->width) return setErr(FT_ERR_INVALID, "column range leaves the image");
    return checkJobCount(1, (uint64_t)p->spp, p);
}

}  // namespace

extern "C" {

int ft_abi_version(void) { return FT_ABI_VERSION; }
const char* ft_last_error(void) { return g_err.c_str(); }
const char* ft_build_info(void) { return "src=" FT_SOURCE_HASH ";kind=" FT_BUILD_KIND; }

int ft_ctx_set_option(ft_ctx* c, int32_t option, int32_t value) {
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    const OptionSpec* o = findOption(option);
    if (!o) return setErr(FT_ERR_INVALID, "unknown option");
    if (!optionAccepts(*o, value)) return setErr(FT_ERR_INVALID, o->err);
    c->*o->field = value;
    return FT_OK;
}
int ft_ctx_get_option(const ft_ctx* c, int32_t option, int32_t* value) {
    if (!c || !value) return setErr(FT_ERR_INVALID, "null argument");
    const OptionSpec* o = findOption(option);
    if (!o) return setErr(FT_ERR_INVALID, "unknown option");
    *value = c->*o->field;
    return FT_OK;
}

int ft_ctx_create(int device, ft_ctx** out) {
    if (!out) return setErr(FT_ERR_INVALID, "null out pointer");
    *out = nullptr;
    ft_ctx* c = new ft_ctx();
    c->device = device;
    if (device >= 0) {
        // every failure below leaves through ft_ctx_destroy, which releases whatever was created so far
        auto fail = [&](int rc) { c->hasDevice = c->stream != nullptr || c->dCounter != nullptr || c->dStats != nullptr; ft_ctx_destroy(c); return rc; };
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0) return fail(setErr(FT_ERR_NO_DEVICE, "no HIP device visible (libfraytracer_hip has no CPU fallback)"));
        if (device >= n) return fail(setErr(FT_ERR_INVALID, "device ordinal out of range"));
        if ((e = hipSetDevice(device)) != hipSuccess) return fail(hipFail(e, "hipSetDevice"));
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail(hipFail(e, "hipGetDeviceProperties"));
        c->numCUs = prop.multiProcessorCount;
        if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) { c->stream = nullptr; return fail(hipFail(e, "hipStreamCreate")); }
        c->ownStream = true;
        if ((e = hipMalloc((void**)&c->dCounter, 256)) != hipSuccess) { c->dCounter = nullptr; return fail(hipFail(e, "hipMalloc")); }
        if ((e = hipMalloc((void**)&c->dStats, sizeof(FtStatsDev))) != hipSuccess) { c->dStats = nullptr; return fail(hipFail(e, "hipMalloc")); }
        if ((e = hipMemsetAsync(c->dStats, 0, sizeof(FtStatsDev), c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(hipFail(e, "hipMemset"));
        c->hasDevice = true;
        c->filler = new DeviceGridFiller(c);
        c->builder.gridFiller = c->filler;
    }
    *out = c;
    return FT_OK;
}

void ft_ctx_destroy(ft_ctx* c) {
    if (!c) return;
    if (c->hasDevice) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        for (auto& p : c->events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        for (auto& p : c->eventPool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        if (c->scratch) (void)hipFree(c->scratch);
        if (c->planes) (void)hipFree(c->planes);
        if (c->aux) (void)hipFree(c->aux);
        if (c->cams) (void)hipFree(c->cams);
        if (c->sliceWork) (void)hipFree(c->sliceWork);
        if (c->refineWork) (void)hipFree(c->refineWork);
        if (c->shellsWork) (void)hipFree(c->shellsWork);
        if (c->measureWork) (void)hipFree(c->measureWork);
        if (c->contourWork) (void)hipFree(c->contourWork);
        for (auto& r : c->hostRegs) (void)hipHostUnregister(r.first);
        for (auto e : c->syncEvents) (void)hipEventDestroy(e);
        if (c->lane1) { (void)hipStreamSynchronize(c->lane1); (void)hipStreamDestroy(c->lane1); }
        if (c->copyStream) { (void)hipStreamSynchronize(c->copyStream); (void)hipStreamDestroy(c->copyStream); }
        if (c->dCounter) (void)hipFree(c->dCounter);
        if (c->dStats) (void)hipFree(c->dStats);
        if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
    }
    delete c->filler;
    delete c;
}

int ft_ctx_set_stream(ft_ctx* c, void* hip_stream) {
    int rc = requireDevice(c); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->ownStream && c->stream) { HIP_TRY(hipStreamDestroy(c->stream)); }
    if (hip_stream) { c->stream = static_cast<hipStream_t>(hip_stream); c->ownStream = false; }
    else { HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->ownStream = true; }
    return FT_OK;
}

// ---- scene construction ------------------------------------------------------------------------
#define CTX_OR_FAIL(c) do { if (!(c)) return setErr(FT_ERR_INVALID, "null context"); } while (0)
static int builderResult(ft_ctx* c, int h) { if (h < 0) g_err = c->builder.err; return h; }

ft_handle ft_form_sphere(ft_ctx* c, const ft_sphere* s) {
    CTX_OR_FAIL(c); if (!s) return setErr(FT_ERR_INVALID, "null primitive");
    return c->builder.sphere(tof3(s->center), s->radius);
}
ft_handle ft_form_capsule(ft_ctx* c, const ft_capsule* s) {
    CTX_OR_FAIL(c); if (!s) return setErr(FT_ERR_INVALID, "null primitive");
    return c->builder.capsule(tof3(s->from), tof3(s->to), s->radius);
}
ft_handle ft_form_torus(ft_ctx* c, const ft_torus* s) {
    CTX_OR_FAIL(c); if (!s) return setErr(FT_ERR_INVALID, "null primitive");
    return c->builder.torus(tof3(s->center), tof3(s->normal), s->major_radius, s->minor_radius);
}
ft_handle ft_form_triangle(ft_ctx* c, const ft_triangle* s) {
    CTX_OR_FAIL(c); if (!s) return setErr(FT_ERR_INVALID, "null primitive");
    return c->builder.triangle(tof3(s->v1), tof3(s->v2), tof3(s->v3), s->radius);
}
ft_handle ft_form_box(ft_ctx* c, const ft_box* s) {
    CTX_OR_FAIL(c); if (!s) return setErr(FT_ERR_INVALID, "null primitive");
    return c->builder.box(tof3(s->center), tof3(s->half_extent));
}
ft_handle ft_form_union(ft_ctx* c, const ft_handle* forms, int32_t n) { CTX_OR_FAIL(c); return builderResult(c, c->builder.formUnion(forms, n)); }
ft_handle ft_form_subtract(ft_ctx* c, ft_handle a, ft_handle b) { CTX_OR_FAIL(c); return builderResult(c, c->builder.formSubtract(a, b)); }
ft_handle ft_form_intersect(ft_ctx* c, const ft_handle* forms, int32_t n) { CTX_OR_FAIL(c); return builderResult(c, c->builder.formIntersect(forms, n)); }
ft_handle ft_form_union_smooth(ft_ctx* c, float strength, const ft_handle* forms, int32_t n) {
    CTX_OR_FAIL(c); return builderResult(c, c->builder.formUnionSmooth(strength, forms, n));
}
int ft_form_boundary(ft_ctx* c, ft_handle form, ft_boundary* out) {
    CTX_OR_FAIL(c);
    if (!c->builder.okForm(form) || !out) return setErr(FT_ERR_INVALID, "invalid form handle");
    const ft::Boundary& b = c->builder.forms[form].boundary;
    out->center.x = b.center.x; out->center.y = b.center.y; out->center.z = b.center.z; out->radius = b.radius;
    return FT_OK;
}
ft_handle ft_material_solid(ft_ctx* c, const float rgb[3]) { CTX_OR_FAIL(c); if (!rgb) return setErr(FT_ERR_INVALID, "null colour"); return c->builder.materialSolid(tof3(rgb)); }
ft_handle ft_material_glass(ft_ctx* c, const float tint[3], float ior, float dispersion) {
    CTX_OR_FAIL(c); if (!tint) return setErr(FT_ERR_INVALID, "null colour");
    return builderResult(c, c->builder.materialGlass(tof3(tint), ior, dispersion));
}
int ft_spectral_table(int32_t nw, float* out) {
    if (!out || nw < 1 || nw > 16) return setErr(FT_ERR_INVALID, "1 <= nw <= 16 and a buffer of nw x 4 floats");
    float t[16][4];
    ft::spectralTable(nw, t);
    memcpy(out, t, sizeof(float) * 4 * (size_t)nw);
    return FT_OK;
}
ft_handle ft_object_create(ft_ctx* c, ft_handle material, ft_handle form) { CTX_OR_FAIL(c); return builderResult(c, c->builder.objectCreate(material, form)); }
ft_handle ft_object_union(ft_ctx* c, const ft_handle* objs, int32_t n) { CTX_OR_FAIL(c); return builderResult(c, c->builder.objectUnion(objs, n)); }
ft_handle ft_object_subtract(ft_ctx* c, ft_handle obj, ft_handle form) { CTX_OR_FAIL(c); return builderResult(c, c->builder.objectSubtract(obj, form)); }
ft_handle ft_object_intersect(ft_ctx* c, ft_handle obj, const ft_handle* forms, int32_t n) {
    CTX_OR_FAIL(c); return builderResult(c, c->builder.objectIntersect(obj, forms, n));
}
ft_handle ft_object_form(ft_ctx* c, ft_handle obj) {
    CTX_OR_FAIL(c);
    if (!c->builder.okObject(obj)) return setErr(FT_ERR_INVALID, "invalid object handle");
    return c->builder.objects[obj].form;
}
ft_handle ft_light_directional(ft_ctx* c, const float d[3], const float rgb[3]) {
    CTX_OR_FAIL(c); if (!d || !rgb) return setErr(FT_ERR_INVALID, "null argument");
    return c->builder.lightDirectional(tof3(d), tof3(rgb));
}
ft_handle ft_light_point(ft_ctx* c, const float p[3], const float rgb[3]) {
    CTX_OR_FAIL(c); if (!p || !rgb) return setErr(FT_ERR_INVALID, "null argument");
    return c->builder.lightPoint(tof3(p), tof3(rgb));
}

int ft_scene_create(ft_ctx* c, ft_handle object, const float bg[3], const ft_handle* lights, int32_t n, ft_scene** out) {
    CTX_OR_FAIL(c);
    if (!out || !bg || n < 0 || (n > 0 && !lights)) return setErr(FT_ERR_INVALID, "bad argument");
    *out = nullptr;
    ft_scene* s = new ft_scene();
    s->ctx = c;
    std::string err;
    if (!ft::flatten(c->builder, object, bg, lights, n, s->flat, err)) { delete s; return setErr(FT_ERR_UNSUPPORTED, err); }
    // the union walk addresses candidate records and the constant pool with 32-bit byte offsets (kernels.hip ld_item_at / pool_at)
    if (s->flat.items.size() >= (1ull << 27) || s->flat.consts.size() >= (1ull << 30)) {
        delete s; return setErr(FT_ERR_UNSUPPORTED, "scene has 2^27 or more (cell, candidate) records or 2^30 or more constants");
    }
    for (const FtInstr& in : s->flat.instr)
        if (in.op == FT_OP_SMOOTH_RUN || in.op == FT_OP_SMOOTH_ADD || in.op == FT_OP_SMOOTH_FIN) s->usesExpLog = true;
    int rc = uploadScene(c, s);
    if (rc) { delete s; return rc; }
    *out = s;
    return FT_OK;
}

int ft_scene_clone(const ft_scene* src, ft_ctx* dst, ft_scene** out) {
    if (!src || !dst || !out) return setErr(FT_ERR_INVALID, "bad argument");
    ft_scene* s = new ft_scene();
    s->ctx = dst;
    s->flat = src->flat;
    s->usesExpLog = src->usesExpLog;
    int rc = uploadScene(dst, s);
    if (rc) { delete s; return rc; }
    *out = s;
    return FT_OK;
}

// src's flattened Object — program, constants, grids, support sphere, certificate clusters: copied, not rebuilt — under another background and other
// lights, which the flattener only appends (scene.cpp flatten: lights in the order given, the background as it stands), so the blob uploadScene
// lays out equals that of ft_scene_create(object, background, lights) byte for byte
int ft_scene_relight(const ft_scene* src, const float bg[3], const ft_handle* lights, int32_t n, ft_scene** out) {
    if (!src || !out || !bg || n < 0 || (n > 0 && !lights)) return setErr(FT_ERR_INVALID, "bad argument");
    *out = nullptr;
    ft_ctx* c = src->ctx;
    for (int32_t i = 0; i < n; ++i)
        if (lights[i] < 0 || (size_t)lights[i] >= c->builder.lights.size()) return setErr(FT_ERR_INVALID, "invalid light handle");
    ft_scene* s = new ft_scene();
    s->ctx = c;
    s->flat = src->flat;
    s->usesExpLog = src->usesExpLog;
    s->flat.lights.clear();
    for (int32_t i = 0; i < n; ++i) s->flat.lights.push_back(c->builder.lights[lights[i]].dev);
    s->flat.hdr.bg[0] = bg[0]; s->flat.hdr.bg[1] = bg[1]; s->flat.hdr.bg[2] = bg[2];
    int rc = uploadScene(c, s);
    if (rc) { delete s; return rc; }
    *out = s;
    return FT_OK;
}

void ft_scene_destroy(ft_scene* s) {
    if (!s) return;
    if (s->dBlob) { (void)hipSetDevice(s->ctx->device); (void)hipFree(s->dBlob); }
    for (TileOrderSlot& t : s->orderSlots) if (t.cost) { (void)hipSetDevice(s->ctx->device); (void)hipFree(t.cost); }
    delete s;
}

// Internal (not in the header, like ft_trace_kernel_for; tests/test_tile_order.py, tools/tile_order_probe.py): the costs the scene's last frame launch
// on lane 0 recorded per tile, and the order built from them, copied to `out` (room for cap values) once the context's stream has run dry.  Returns the
// tile count; 0 where the slot holds none (nothing recorded, FT_OPT_ORDER = 0; for the order also FT_OPT_ORDER = 2); a negative error code.
static long long readTileOrderSlot(const ft_scene* s, bool order, uint32_t* out, long long cap) {
    if (!s || !s->ctx || (!out && cap > 0) || cap < 0) return setErr(FT_ERR_INVALID, "bad argument");
    int rc = requireDevice(s->ctx); if (rc) return rc;
    const TileOrderSlot& t = s->orderSlots[0];
    if (!t.keyed || (order && !t.hasOrder)) return 0;
    const long long n = (long long)(t.key.nJobs >> 6);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    if (std::min(n, cap) > 0) HIP_TRY(hipMemcpy(out, order ? t.order : t.cost, (size_t)std::min(n, cap) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return n;
}
long long ft_scene_tile_costs(const ft_scene* s, uint32_t* out, long long cap) { return readTileOrderSlot(s, false, out, cap); }
long long ft_scene_tile_order(const ft_scene* s, uint32_t* out, long long cap) { return readTileOrderSlot(s, true, out, cap); }
// Internal (tests/test_try_hint.py, tools/try_hint_probe.py): the try hints of the scene's lane-0 slot (FT_OPT_TRY_HINT; ft_kernels.h "Try hints").
// ft_selftest_try_hints copies them to `out` as the tile costs are; ft_selftest_try_hints_fill overwrites them — mode 0: every word = value, mode 1: words
// from a generator seeded with value, every byte value possible — so that the next frame follows hints no frame could have left.
// Both return the tile count, 0 where the slot holds no hints, or a negative error code.
long long ft_selftest_try_hints(const ft_scene* s, uint32_t* out, long long cap) {
    if (!s || !s->ctx || (!out && cap > 0) || cap < 0) return setErr(FT_ERR_INVALID, "bad argument");
    int rc = requireDevice(s->ctx); if (rc) return rc;
    const TileOrderSlot& t = s->orderSlots[0];
    if (!t.hasHint) return 0;
    const long long n = (long long)(t.hintKey.nJobs >> 6);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    if (std::min(n, cap) > 0) HIP_TRY(hipMemcpy(out, t.hint, (size_t)std::min(n, cap) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return n;
}
long long ft_selftest_try_hints_fill(const ft_scene* s, int32_t mode, uint32_t value) {
    if (!s || !s->ctx || mode < 0 || mode > 1) return setErr(FT_ERR_INVALID, "bad argument");
    int rc = requireDevice(s->ctx); if (rc) return rc;
    const TileOrderSlot& t = s->orderSlots[0];
    if (!t.hasHint) return 0;
    const size_t n = t.hintKey.nJobs >> 6;
    std::vector<uint32_t> w(n, value);
    if (mode == 1) { uint64_t x = value * 2654435761ull + 88172645463325252ull; for (uint32_t& v : w) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (uint32_t)(x >> 24); } }
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy(t.hint, w.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    return (long long)n;
}
// Internal: the slot's words replaced by `words` (n = the slot's tile count): hints recorded from another view put under this one
long long ft_selftest_try_hints_write(const ft_scene* s, const uint32_t* words, long long n) {
    if (!s || !s->ctx || !words) return setErr(FT_ERR_INVALID, "bad argument");
    int rc = requireDevice(s->ctx); if (rc) return rc;
    const TileOrderSlot& t = s->orderSlots[0];
    if (!t.hasHint) return 0;
    if (n != (long long)(t.hintKey.nJobs >> 6)) return setErr(FT_ERR_INVALID, "not the slot's tile count");
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy(t.hint, words, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    return n;
}
// Internal: 1 where the scene's last frame launch on lane 0 that recorded try hints also followed the ones it found, else 0
int ft_selftest_try_hints_used(const ft_scene* s) { return s && s->orderSlots[0].hasHint && s->orderSlots[0].usedHint ? 1 : 0; }
// Internal: 1 where the scene's last recording frame launch on lane 0 handed its tiles out in a built order, 0 where it ran in index order
int ft_scene_tile_order_used(const ft_scene* s) { return s && s->orderSlots[0].keyed && s->orderSlots[0].usedOrder ? 1 : 0; }
// Internal (tools/tile_order_probe.py, tests/test_tile_order.py): tiles count as heavy from num / den of the mean cost on (the shipped rule is 1 / 1;
// 0 / 1 sorts every tile; 1000000 / 1 leaves none heavy: the identity).  ft_tile_is_heavy compares cost * n * den with sum * num in 64 bits: den <= 16
// keeps the left side below 2^62 for any frame, num <= 1000000 the right one for launches of fewer than 1.8e13 evaluation rounds (hours of kernel time)
int ft_ctx_tile_order_rule(ft_ctx* c, uint32_t num, uint32_t den) {
    if (!c || den == 0u || num > 1000000u || den > 16u) return setErr(FT_ERR_INVALID, "bad argument");
    c->orderNum = num; c->orderDen = den;
    return FT_OK;
}

float ft_lens_create(float fov) { return ft::lensCreate(fov); }
int ft_camera_look_at(const float pos[3], const float look[3], const float up[3], float nps, ft_camera* out) {
    if (!pos || !look || !up || !out) return setErr(FT_ERR_INVALID, "null argument");
    f3 o[4];
    ft::cameraLookAt(tof3(pos), tof3(look), tof3(up), nps, o);
    out->position = ft_vec3{o[0].x, o[0].y, o[0].z}; out->forward = ft_vec3{o[1].x, o[1].y, o[1].z};
    out->up_scaled = ft_vec3{o[2].x, o[2].y, o[2].z}; out->right_scaled = ft_vec3{o[3].x, o[3].y, o[3].z};
    return FT_OK;
}

// ---- hot path ------------------------------------------------------------------------------------
namespace {

// What a call writes per pixel or ray: colours (3 floats; SdfForm.tryTrace: its 10-dword results) and, in the EXTENSION builds, the 64-byte
// ft_object_trace_result records and the int32 material handles.  Any may be NULL: not asked for.
struct Outputs {
    void* rgb; void* hits; void* material;
    bool any() const { return rgb || hits || material; }
    bool extra() const { return hits || material; }                // something only the EXTENSION builds write
    Outputs at(size_t px) const {                                  // a frame's buffers `px` pixels further on
        auto step = [](void* p, size_t bytes) { return p ? static_cast<void*>(static_cast<unsigned char*>(p) + bytes) : nullptr; };
        return Outputs{step(rgb, px * 12), step(hits, px * 64), step(material, px * 4)};
    }
};

// What every form asks of its outputs, stated once: at least one of them and, in device memory, records on 16 bytes, the rest on 4.  The
// entry points differ in whether they ask for the device before or after this, and keep that order.
int checkOutputs(const Outputs& o, bool deviceMemory) {
    if (!o.any()) return setErr(FT_ERR_INVALID, "no output asked for");
    if (deviceMemory && ((reinterpret_cast<uintptr_t>(o.hits) & 15u) || (reinterpret_cast<uintptr_t>(o.material) & 3u) || (reinterpret_cast<uintptr_t>(o.rgb) & 3u)))
        return setErr(FT_ERR_INVALID, "the ft_object_trace_result records must be 16-byte aligned, every other output buffer 4-byte aligned");
    return FT_OK;
}

// nViews cameras (host memory), one set of parameters, outputs in device memory written view after view: every render entry point is a check
// plus one of these, and a new form (per-view parameters, a region of interest, a depth plane) is a field here
struct FrameRequest { const ft_camera* cams; int32_t nViews; const ft_render_params* p; Outputs dev; };

// The kernel arguments of one launch: nViews views (`views`: their cameras in device memory, 12 floats each; NULL: the single camera `cam`)
// with the parameters p.  No HIP call, no context: launchTrace adds what depends on those.
FtRenderArgs frameArgs(const ft_scene* s, const ft_render_params& p, const ft_camera* cam, const float* views, uint32_t nViews, const Outputs& o) {
    FtRenderArgs a{};
    if (views) { a.views = views; a.nViews = nViews; }
    else memcpy(a.cam, cam, sizeof(float) * 12);
    a.W = p.width; a.H = p.height; a.x0 = p.x0; a.nCols = p.n_columns;
    a.stripeW = (uint32_t)p.stripe_width; a.stripeRanks = (uint32_t)p.stripe_ranks; a.stripeRank = (uint32_t)p.stripe_rank;
    a.mode = 0;
    a.maxSize = (float)std::max(p.width, p.height);                // Image.fs:18
    a.eps = p.epsilon; a.length = p.length;
    a.tilesY = (uint32_t)((p.height + 7) / 8);
    a.jobsPerPlane = (uint32_t)((p.n_columns + 7) / 8) * a.tilesY * 64u;
    a.spp = (uint32_t)p.spp; a.sppN = 1; while (a.sppN * a.sppN < a.spp) ++a.sppN;
    a.aoSamples = (uint32_t)p.ao_samples; a.aoRadius = p.ao_radius;
    a.planePixels = (uint32_t)p.n_columns * (uint32_t)p.height;
    a.nJobs = a.jobsPerPlane * a.spp * nViews;                     // views: view after view, each its spp sample planes (kernels.hip start_job)
    // EXTENSION glass / wavelengths: without a glass material in the scene bounces change nothing
    a.maxBounces = s->dev.nGlass ? (uint32_t)p.max_bounces : 0u;
    a.spectral = (uint32_t)p.spectral;
    if (a.spectral) ft::spectralTable((int)a.spectral, a.spec);
    a.ext = (a.spp != 1u || a.aoSamples != 0u || a.maxBounces != 0u || a.spectral != 0u) ? 1u : 0u;
    if (o.extra()) {                                               // the hit buffers exist in the EXTENSION builds only
        a.ext = 1u;
        a.hits = o.rgb ? 1u : 2u;
        a.hitsOut = static_cast<float*>(o.hits); a.matOut = static_cast<int32_t*>(o.material);
        a.matHandles = s->dMatHandles;
    }
    return a;
}

// Launches `a` on a render lane, its colours to d_out.  EXTENSION spp > 1: one frame per sample into the context's planes, then a fixed-order
// resolve per view; the planes belong to lane 0.
int launchFrameArgs(ft_ctx* c, const ft_scene* s, FtRenderArgs& a, void* d_out, int lane) {
    if (a.spp == 1) { a.out = static_cast<float*>(d_out); return launchTrace(c, s, a, lane); }
    if (lane != 0) return setErr(FT_ERR_INVALID, "internal: the sample planes belong to lane 0");
    const uint32_t nViews = a.views ? a.nViews : 1u;
    const size_t planeFloats = (size_t)a.planePixels * 3;
    int rc = ensureBytes(c->planes, c->planesBytes, planeFloats * a.spp * nViews * sizeof(float)); if (rc) return rc;
    a.out = static_cast<float*>(c->planes);
    if ((rc = launchTrace(c, s, a, 0))) return rc;
    for (uint32_t k = 0; k < nViews; ++k)
        HIP_TRY(ft_launch_resolve(static_cast<const float*>(c->planes) + k * a.spp * planeFloats, static_cast<float*>(d_out) + k * planeFloats, planeFloats, a.spp, c->stream));
    return FT_OK;
}

// what every frame launch asks: a device, a scene of this context, cameras, an output, sound parameters — in this order
int checkFrame(ft_ctx* c, const ft_scene* s, const FrameRequest& r) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!s || s->ctx != c || !r.cams || !r.dev.any()) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    return checkParams(r.p);
}

// the batch's cameras into the context's device table (12 floats each)
int stageCameras(ft_ctx* c, const ft_camera* cameras, int32_t n) {
    static_assert(sizeof(ft_camera) == 12 * sizeof(float), "layout");
    const size_t bytes = (size_t)n * sizeof(ft_camera);
    int rc = ensureBytes(c->cams, c->camsBytes, bytes); if (rc) return rc;
    // on the context's stream, behind the launches that may still read the previous batch's table; from a pageable copy, so that the caller's
    // array is free when this returns (a pageable source is copied before hipMemcpyAsync returns)
    const std::vector<ft_camera> staged(cameras, cameras + n);
    HIP_TRY(hipMemcpyAsync(c->cams, staged.data(), bytes, hipMemcpyHostToDevice, c->stream));
    return FT_OK;
}

// The one path of every frame form, on the context's stream.  One view has its camera in the kernel arguments (ft_render_device's kernels);
// several go through the context's camera table in launches of at most FT_MAX_VIEWS views (one PH_CAM value per lane of a wave), each at its
// views' offsets into the outputs.  Without colours one ray per pixel is traced and the EXTENSION fields of p do not apply.
int launchFrame(ft_ctx* c, const ft_scene* s, const FrameRequest& r) {
    int rc = checkFrame(c, s, r); if (rc) return rc;
    ft_render_params p = *r.p;
    if (!r.dev.rgb) { p.spp = 1; p.ao_samples = 0; p.max_bounces = 0; p.spectral = 0; }
    if (r.nViews > 1 && (rc = stageCameras(c, r.cams, r.nViews))) return rc;
    const size_t px = (size_t)p.n_columns * (size_t)p.height;
    for (int32_t k0 = 0; k0 < r.nViews; k0 += FT_MAX_VIEWS) {
        const uint32_t m = (uint32_t)std::min<int32_t>(FT_MAX_VIEWS, r.nViews - k0);
        const Outputs part = r.dev.at((size_t)k0 * px);
        FtRenderArgs a = frameArgs(s, p, r.cams, r.nViews > 1 ? static_cast<const float*>(c->cams) + 12 * (size_t)k0 : nullptr, m, part);
        if ((rc = launchFrameArgs(c, s, a, part.rgb, 0))) return rc;
    }
    return FT_OK;
}

// everything a views form can refuse before any device work: arguments, parameters and the job count of the whole batch (without colours:
// one sample plane a view, whatever spp says); the device is asked for last
int checkViews(ft_ctx* c, const ft_camera* cameras, int32_t n, const ft_render_params* p, const Outputs& o) {
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (!cameras || !o.any()) return setErr(FT_ERR_INVALID, "null argument");
    if (n < 1) return setErr(FT_ERR_INVALID, "ft_render_views: n_views must be at least 1");
    int rc = checkParams(p); if (rc) return rc;
    if ((rc = checkJobCount((uint64_t)n, o.rgb ? (uint64_t)p->spp : 1u, p))) return rc;
    return requireDevice(c);
}

}  // namespace

// The four device forms: each a check, in the order it always had, and the one launch path.
int ft_render_device(ft_ctx* c, const ft_scene* s, const ft_camera* cam, const ft_render_params* p, void* d_out) {
    return launchFrame(c, s, FrameRequest{cam, 1, p, Outputs{d_out, nullptr, nullptr}});
}

int ft_render_hits_device(ft_ctx* c, const ft_scene* s, const ft_camera* cam, const ft_render_params* p, void* d_out_rgb, void* d_hits, void* d_material) {
    const Outputs o{d_out_rgb, d_hits, d_material};
    int rc = requireDevice(c); if (rc) return rc;                      // the device first, then the outputs
    if ((rc = checkOutputs(o, true))) return rc;
    return launchFrame(c, s, FrameRequest{cam, 1, p, o});
}

int ft_render_views_device(ft_ctx* c, const ft_scene* s, const ft_camera* cameras, int32_t n, const ft_render_params* p, void* d_out) {
    const Outputs o{d_out, nullptr, nullptr};
    int rc = checkViews(c, cameras, n, p, o); if (rc) return rc;
    return launchFrame(c, s, FrameRequest{cameras, n, p, o});
}

int ft_render_views_hits_device(ft_ctx* c, const ft_scene* s, const ft_camera* cameras, int32_t n, const ft_render_params* p, void* d_out_rgb,
                                void* d_hits, void* d_material) {
    const Outputs o{d_out_rgb, d_hits, d_material};
    int rc = checkOutputs(o, true); if (rc) return rc;                 // the outputs first, the device last (checkViews)
    if ((rc = checkViews(c, cameras, n, p, o))) return rc;
    return launchFrame(c, s, FrameRequest{cameras, n, p, o});
}

int ft_collect_stats(ft_ctx* c, ft_stats* st) {
    int rc = requireDevice(c); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    double ms = c->foldedMs;
    c->foldedMs = 0.0;
    for (auto& p : c->events) {
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, p.first, p.second));
        ms += t;
        c->eventPool.push_back(p);
    }
    c->events.clear();
    // Read and reset ON THE CONTEXT'S STREAM.  The stream is hipStreamNonBlocking, i.e. it does not synchronise with the legacy
    // null stream, and hipMemset of device memory returns before the fill has run: round 2 reset the block with a null-stream
    // hipMemset, which could still be pending when the next launch on c->stream began adding to it.
    FtStatsDev h{};
    HIP_TRY(hipMemcpyAsync(&h, c->dStats, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->dStats, 0, sizeof(FtStatsDev), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (st) {
        st->rays_primary = h.rays_primary; st->rays_shadow = h.rays_shadow; st->rays_ext = h.rays_ext;
        st->hits_primary = h.hits_primary; st->hits_shadow = h.hits_shadow; st->sdf_evals = h.sdf_evals;
        st->flags = h.flags; st->kernel_ms = (float)ms; st->wave_evals = h.wave_evals;
        st->shader_mhz = h.clk_ref ? (float)((double)h.clk_shader / (double)h.clk_ref * 100.0) : 0.0f;   // s_memrealtime: 100 MHz
        st->tail_fraction = h.sdf_evals ? (float)((double)h.coop_evals / (double)h.sdf_evals) : 0.0f;
        st->culled_fraction = h.cull_total ? (float)((double)h.cull_skipped / (double)h.cull_total) : 0.0f;
    }
    return FT_OK;
}

// ---- host output: Image.render returns a host FColor[,] (Image.fs:26-35) ------------------------------------------
// The frame (12 B / pixel) has to cross PCIe.  A pageable destination is copied by the runtime through its own staging
// at 4-8 GB/s (23-50 ms for a 4096^2 frame); a page-locked one is written by the DMA engines at link rate.  ft_render
// therefore (a) page-locks the caller's buffer for the duration of the call unless it already is (ft_host_register, or
// memory from hipHostMalloc) — the pinning runs on the calling thread while the GPU already renders — and (b) renders
// a large contiguous frame in four column chunks on two alternating streams (the drain of one chunk overlaps the start of
// the next) while a third stream copies every finished chunk, so that only the last chunk's copy is left at the end.
int ft_host_register(ft_ctx* c, void* p, uint64_t bytes) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!p || bytes == 0) return setErr(FT_ERR_INVALID, "bad argument");
    HIP_TRY(hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault));
    c->hostRegs.emplace_back(p, (size_t)bytes);
    return FT_OK;
}

int ft_host_unregister(ft_ctx* c, void* p) {
    int rc = requireDevice(c); if (rc) return rc;
    for (size_t i = 0; i < c->hostRegs.size(); ++i)
        if (c->hostRegs[i].first == p) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipHostUnregister(p));
            c->hostRegs.erase(c->hostRegs.begin() + (long)i);
            return FT_OK;
        }
    return setErr(FT_ERR_INVALID, "this pointer was not registered through ft_host_register");
}

namespace {

bool isPageLocked(ft_ctx* c, const void* p, size_t bytes) {
    const char* b = static_cast<const char*>(p);
    for (auto& r : c->hostRegs)
        if (b >= static_cast<const char*>(r.first) && b + bytes <= static_cast<const char*>(r.first) + r.second) return true;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain malloc memory: "invalid value"
    return attr.type == hipMemoryTypeHost;
}

int ensurePipeline(ft_ctx* c, size_t nEvents) {
    if (!c->lane1) HIP_TRY(hipStreamCreateWithFlags(&c->lane1, hipStreamNonBlocking));
    if (!c->copyStream) HIP_TRY(hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking));
    while (c->syncEvents.size() < nEvents) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->syncEvents.push_back(e);
    }
    return FT_OK;
}

// page-lock `p` unless it already is; true if this call pinned it (the caller unpins)
bool pinForCall(ft_ctx* c, void* p, size_t bytes) {
    if (bytes < ((size_t)1 << 20) || !c->optHostPin || isPageLocked(c, p, bytes)) return false;
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) return true;
    (void)hipGetLastError();                                   // not fatal: the runtime's pageable path still works
    return false;
}

// The host forms' staging ritual, once: [input | part 0 | part 1 | part 2] in the context's scratch, each part that is asked for on a 256-byte
// boundary; upload() brings the input up, the launch writes the parts, copyOut() queues every part to the caller's buffer behind it on the context's
// stream, finish() ends the call.  A part is a host destination (NULL: not asked for) and its bytes per item: the frame and ray-buffer forms have
// colours, records and the material plane (outputParts), the field forms distance, normal and material.
// A form that bounds its scratch plans one launch group and calls copyOut once per group.
// pin: page-lock the caller's buffers for the call while the GPU renders the first group, so that the copies run at link rate.  The views forms
// pin (like ft_render and ft_render_colors); ft_render_hits and the ray-buffer forms never did: whether they should is a measurement to make.
struct HostPart { void* host; size_t stride; };
using HostParts = std::array<HostPart, 3>;
class HostStaging {
public:
    HostStaging(ft_ctx* c, const char* what, const HostParts& parts, bool pin) : c_(c), what_(what), parts_(parts), pin_(pin) {}
    // scratch for `count` pixels, rays, records or points behind inputBytes of input
    int plan(size_t inputBytes, size_t count) {
        size_t end = inputBytes;
        for (int i = 0; i < 3; ++i) { off_[i] = align256(end); end = off_[i] + (parts_[i].host ? count * parts_[i].stride : 0); }
        return ensureScratch(c_, end);
    }
    void* input(size_t offset = 0) const { return static_cast<unsigned char*>(c_->scratch) + offset; }
    // `bytes` of the caller's input to the input area at `offset`, on the context's stream
    int upload(size_t offset, const void* src, size_t bytes) {
        HIP_TRY(hipMemcpyAsync(input(offset), src, bytes, hipMemcpyHostToDevice, c_->stream));
        return FT_OK;
    }
    void* part(int i) const { return parts_[i].host ? static_cast<unsigned char*>(c_->scratch) + off_[i] : nullptr; }
    Outputs dev() const { return Outputs{part(0), part(1), part(2)}; }
    bool ok() const { return !rc_ && err_ == hipSuccess; }
    // behind a launch that returned rc: `count` items from the scratch to the caller's buffers at item `first`; `total`: the items of the whole call
    void copyOut(int rc, size_t first, size_t count, size_t total) {
        rc_ = rc;
        if (!rc_ && pin_ && first == 0)                                // the GPU is rendering: page-lock the destinations meanwhile
            for (int i = 0; i < 3; ++i) if (parts_[i].host) pinned_[i] = pinForCall(c_, parts_[i].host, total * parts_[i].stride);
        for (int i = 0; i < 3 && ok(); ++i)
            if (parts_[i].host)
                err_ = hipMemcpyAsync(static_cast<unsigned char*>(parts_[i].host) + first * parts_[i].stride, part(i), count * parts_[i].stride, hipMemcpyDeviceToHost, c_->stream);
    }
    // nothing of the call is left in flight, whatever happened (the scratch and the caller's buffers are reused); what was pinned here is
    // released; then the launch's error, the copies', the synchronisation's.  The launches' event pairs stay pending: collecting is the next step
    // of a form that returns statistics (finish(st)), and not a step of one that does not (the field forms)
    int finish() {
        const hipError_t se = hipStreamSynchronize(c_->stream);
        for (int i = 0; i < 3; ++i) if (pinned_[i]) (void)hipHostUnregister(parts_[i].host);
        if (rc_) return rc_;
        if (err_ != hipSuccess) return hipFail(err_, (std::string(what_) + " host output").c_str());
        if (se != hipSuccess) return hipFail(se, what_);
        return FT_OK;
    }
    int finish(ft_stats* st) { const int rc = finish(); return rc ? rc : ft_collect_stats(c_, st); }
private:
    ft_ctx* c_; const char* what_;
    HostParts parts_; bool pin_;
    size_t off_[3] = {0, 0, 0};
    bool pinned_[3] = {false, false, false};
    int rc_ = FT_OK; hipError_t err_ = hipSuccess;
};
// the parts of a frame or ray-buffer form: colours (SdfForm.tryTrace: its 40-byte results), 64-byte records, the 4-byte material plane or masks
HostParts outputParts(const Outputs& host, size_t rgbStride = 12) { return HostParts{{{host.rgb, rgbStride}, {host.hits, 64}, {host.material, 4}}}; }

// The frame of `p` rendered into the context's scratch buffer in column chunks on the two render lanes (the drain of one chunk
// overlaps the start of the next); chunk i's completion is syncEvents[2 + i].  c0 receives the chunk boundaries (columns).
struct ChunkPlan { int n = 1; std::vector<int> c0; size_t colBytes = 0, bytes = 0; };

int launchChunks(ft_ctx* c, const ft_scene* s, const ft_camera* cam, const ft_render_params* p, ChunkPlan& plan) {
    int rc;
    plan.colBytes = (size_t)p->height * 3 * sizeof(float);
    plan.bytes = (size_t)p->n_columns * plan.colBytes;
    if ((rc = ensureScratch(c, plan.bytes))) return rc;
    // chunks: only the reference's sampling (spp = 1: no shared sample planes) of a contiguous column range that is worth it
    plan.n = (p->spp == 1 && p->stripe_ranks == 1 && p->n_columns >= 256 && plan.bytes >= ((size_t)16 << 20)) ? 4 : 1;
    if (const int v = c->optHostChunks; v >= 1 && p->spp == 1 && p->stripe_ranks == 1 && p->n_columns >= 8 * v) plan.n = v;   // FT_OPT_HOST_CHUNKS
    if ((rc = ensurePipeline(c, (size_t)plan.n + 2))) return rc;
    HIP_TRY(hipEventRecord(c->syncEvents[0], c->stream));      // whatever the caller queued on the context's stream comes first
    HIP_TRY(hipStreamWaitEvent(c->lane1, c->syncEvents[0], 0));
    HIP_TRY(hipStreamWaitEvent(c->copyStream, c->syncEvents[0], 0));
    plan.c0.assign(plan.n + 1, 0);
    for (int i = 0; i < plan.n; ++i) plan.c0[i] = (int)(((int64_t)p->n_columns * i / plan.n) & ~(int64_t)7);   // chunks start on a tile boundary
    plan.c0[plan.n] = p->n_columns;
    char* dFrame = static_cast<char*>(c->scratch);
    if ((rc = checkFrame(c, s, FrameRequest{cam, 1, p, Outputs{dFrame, nullptr, nullptr}}))) return rc;
    for (int i = 0; i < plan.n; ++i) {
        ft_render_params q = *p;
        q.x0 = p->x0 + plan.c0[i]; q.n_columns = plan.c0[i + 1] - plan.c0[i];
        if (p->stripe_ranks == 1) q.stripe_width = q.n_columns;
        const int lane = plan.n > 1 ? (i & 1) : 0;
        void* const dChunk = dFrame + (size_t)plan.c0[i] * plan.colBytes;
        FtRenderArgs a = frameArgs(s, q, cam, nullptr, 1, Outputs{dChunk, nullptr, nullptr});
        if ((rc = launchFrameArgs(c, s, a, dChunk, lane))) return rc;
        HIP_TRY(hipEventRecord(c->syncEvents[2 + i], lane ? c->lane1 : c->stream));
    }
    return FT_OK;
}

// The scope of a call that runs the chunk pipeline (ft_render, ft_render_colors).  Whatever goes wrong, nothing of the call may still be in
// flight when it returns (the scratch frame and the caller's buffer are reused), and a buffer pinned here is released.
struct ChunkedCall {
    ft_ctx* c; void* pinned = nullptr; bool waitedFor = false;     // waitedFor: the call synchronised everything itself
    void pin(void* p, size_t bytes) { if (pinForCall(c, p, bytes)) pinned = p; }
    ~ChunkedCall() {
        if (!waitedFor && c->copyStream) { (void)hipStreamSynchronize(c->copyStream); (void)hipStreamSynchronize(c->lane1); (void)hipStreamSynchronize(c->stream); }
        if (pinned) (void)hipHostUnregister(pinned);
    }
};

}  // namespace

int ft_render(ft_ctx* c, const ft_scene* s, const ft_camera* cam, const ft_render_params* p, float* out, ft_stats* st) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!out) return setErr(FT_ERR_INVALID, "null output");
    if ((rc = checkParams(p))) return rc;
    ChunkPlan plan;
    ChunkedCall call{c};
    if ((rc = launchChunks(c, s, cam, p, plan))) return rc;
    call.pin(out, plan.bytes);                                 // the GPU is rendering: page-lock the destination meanwhile
    char* dFrame = static_cast<char*>(c->scratch);
    hipError_t err = hipSuccess;
    for (int i = 0; i < plan.n && err == hipSuccess; ++i) {
        const size_t off = (size_t)plan.c0[i] * plan.colBytes, n = (size_t)(plan.c0[i + 1] - plan.c0[i]) * plan.colBytes;
        if ((err = hipStreamWaitEvent(c->copyStream, c->syncEvents[2 + i], 0)) != hipSuccess) break;
        err = hipMemcpyAsync(reinterpret_cast<char*>(out) + off, dFrame + off, n, hipMemcpyDeviceToHost, c->copyStream);
    }
    if (err == hipSuccess) err = hipEventRecord(c->syncEvents[1], c->copyStream);
    if (err == hipSuccess) err = hipStreamWaitEvent(c->stream, c->syncEvents[1], 0);   // join: the context's stream ends after the copies
    if (err == hipSuccess) err = hipStreamSynchronize(c->copyStream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->lane1);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) return hipFail(err, "ft_render host output");
    call.waitedFor = true;
    return ft_collect_stats(c, st);
}

// EXTENSION: the whole frame on lane 0 into the context's scratch, then copied out
int ft_render_hits(ft_ctx* c, const ft_scene* s, const ft_camera* cam, const ft_render_params* p, float* out_rgb, ft_object_trace_result* out_hits,
                   int32_t* out_material, ft_stats* st) {
    static_assert(sizeof(ft_object_trace_result) == 64, "layout");
    const Outputs host{out_rgb, out_hits, out_material};
    int rc = requireDevice(c); if (rc) return rc;
    if ((rc = checkOutputs(host, false))) return rc;
    if ((rc = checkParams(p))) return rc;
    const size_t px = (size_t)p->n_columns * (size_t)p->height;
    HostStaging stage(c, "ft_render_hits", outputParts(host), false);
    if ((rc = stage.plan(0, px))) return rc;
    stage.copyOut(launchFrame(c, s, FrameRequest{cam, 1, p, stage.dev()}), 0, px, px);
    return stage.finish(st);
}

// ---- ft_render_views: K cameras, one scene, one set of parameters ------------------------------------------------------
// the whole batch into the context's scratch, then one copy to the (page-locked for the call) destination
int ft_render_views(ft_ctx* c, const ft_scene* s, const ft_camera* cameras, int32_t n, const ft_render_params* p, float* out, ft_stats* st) {
    const Outputs host{out, nullptr, nullptr};
    int rc = checkViews(c, cameras, n, p, host); if (rc) return rc;
    if (n == 1) return ft_render(c, s, cameras, p, out, st);           // exactly ft_render (its column-chunk pipeline included)
    const size_t px = (size_t)p->n_columns * (size_t)p->height;
    HostStaging stage(c, "ft_render_views", outputParts(host), true);
    if ((rc = stage.plan(0, (size_t)n * px))) return rc;
    stage.copyOut(launchFrame(c, s, FrameRequest{cameras, n, p, stage.dev()}), 0, (size_t)n * px, (size_t)n * px);
    return stage.finish(st);
}

// ---- ft_render_views_hits: the hit buffers of K cameras, one scene, one set of parameters ------------------------------------------
// EXTENSION: one launch group (<= FT_MAX_VIEWS views) at a time into the context's scratch, each copied out behind its launch on the context's
// stream before the next group reuses the scratch: device memory stays bounded by one group.  The destinations are page-locked for the call
// while the first group renders (like ft_render_views'), so the copies run at link rate; a group's copy and the next group's render share the
// stream, one after the other.
int ft_render_views_hits(ft_ctx* c, const ft_scene* s, const ft_camera* cameras, int32_t n, const ft_render_params* p, float* out_rgb,
                         ft_object_trace_result* out_hits, int32_t* out_material, ft_stats* st) {
    const Outputs host{out_rgb, out_hits, out_material};
    int rc = checkOutputs(host, false); if (rc) return rc;
    if ((rc = checkViews(c, cameras, n, p, host))) return rc;
    if (!host.extra()) return ft_render_views(c, s, cameras, n, p, out_rgb, st);                      // the frames alone: staged as a whole batch
    if (n == 1) return ft_render_hits(c, s, cameras, p, out_rgb, out_hits, out_material, st);         // exactly ft_render_hits
    const size_t px = (size_t)p->n_columns * (size_t)p->height;
    HostStaging stage(c, "ft_render_views_hits", outputParts(host), true);
    if ((rc = stage.plan(0, (size_t)std::min<int32_t>(n, FT_MAX_VIEWS) * px))) return rc;
    for (int32_t k0 = 0; k0 < n && stage.ok(); k0 += FT_MAX_VIEWS) {
        const int32_t m = std::min<int32_t>(FT_MAX_VIEWS, n - k0);
        stage.copyOut(launchFrame(c, s, FrameRequest{cameras + k0, m, p, stage.dev()}), (size_t)k0 * px, (size_t)m * px, (size_t)n * px);
    }
    return stage.finish(st);
}

// ---- tone map: Image.toColors / toBitmap order on the device ---------------------------------
static int checkToneMap(const void* frame, int32_t X, int32_t Y, const ft_tonemap_params* p) {
    if (!frame || !p || X <= 0 || Y <= 0) return setErr(FT_ERR_INVALID, "bad argument");
    if (!(p->gamma > 0.0f)) return setErr(FT_ERR_INVALID, "gamma must be positive");
    if ((uint64_t)X * (uint64_t)Y >= (1ull << 31)) return setErr(FT_ERR_UNSUPPORTED, "more than 2^31 pixels");
    return FT_OK;
}

int ft_tone_map_device(ft_ctx* c, const void* d_frame, int32_t X, int32_t Y, const ft_tonemap_params* p, void* d_out) {
    int rc = requireDevice(c); if (rc) return rc;
    if ((rc = checkToneMap(d_frame, X, Y, p))) return rc;
    if (!d_out) return setErr(FT_ERR_INVALID, "null output");
    if (reinterpret_cast<uintptr_t>(d_frame) & 15u) return setErr(FT_ERR_INVALID, "the device frame must be 16-byte aligned");
    if ((rc = ensureAux(c, 256))) return rc;
    const float gammaInv = 1.0f / p->gamma;                            // Image.fs:38
    HIP_TRY(ft_launch_tonemap(static_cast<const float*>(d_frame), (uint32_t)X, (uint32_t)Y, static_cast<uint32_t*>(c->aux), gammaInv,
                              p->dither ? 1u : 0u, p->seed, p->bmp_order != 0, static_cast<unsigned char*>(d_out), (unsigned)c->numCUs, c->optMath, c->stream));
    return FT_OK;
}

int ft_tone_map(ft_ctx* c, const void* d_frame, int32_t X, int32_t Y, const ft_tonemap_params* p, uint8_t* out, float* max_out) {
    int rc = requireDevice(c); if (rc) return rc;
    if ((rc = checkToneMap(d_frame, X, Y, p))) return rc;
    if (!out) return setErr(FT_ERR_INVALID, "null output");
    const size_t bytes = (size_t)X * Y * 3;
    if ((rc = ensureAux(c, 256 + bytes))) return rc;
    unsigned char* dBytes = static_cast<unsigned char*>(c->aux) + 256;
    if ((rc = ft_tone_map_device(c, d_frame, X, Y, p, dBytes))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dBytes, bytes, hipMemcpyDeviceToHost, c->stream));
    if (max_out) HIP_TRY(hipMemcpyAsync(max_out, c->aux, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}

int ft_tone_map_host(ft_ctx* c, const float* frame, int32_t X, int32_t Y, const ft_tonemap_params* p, uint8_t* out, float* max_out) {
    int rc = requireDevice(c); if (rc) return rc;
    if ((rc = checkToneMap(frame, X, Y, p))) return rc;
    const size_t bytes = (size_t)X * Y * 12;
    if ((rc = ensureScratch(c, bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(c->scratch, frame, bytes, hipMemcpyHostToDevice, c->stream));
    return ft_tone_map(c, c->scratch, X, Y, p, out, max_out);
}

int ft_render_colors(ft_ctx* c, const ft_scene* s, const ft_camera* cam, const ft_render_params* p, const ft_tonemap_params* tm,
                     uint8_t* out, float* max_out, ft_stats* st) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!out || !tm) return setErr(FT_ERR_INVALID, "null argument");
    if ((rc = checkParams(p))) return rc;
    if (p->x0 != 0 || p->n_columns != p->width || p->stripe_ranks != 1)
        return setErr(FT_ERR_INVALID, "the tone map needs the whole frame (its normalisation is the global maximum, Image.fs:40-43)");
    if ((rc = checkToneMap(out, p->width, p->height, tm))) return rc;
    // the frame is rendered like ft_render's (column chunks on two lanes); the tone map follows on the context's stream once both
    // lanes are done — its normalisation needs every pixel — and only the bytes are copied out
    ChunkPlan plan;
    const size_t outBytes = (size_t)p->width * p->height * 3;
    ChunkedCall call{c};
    if ((rc = launchChunks(c, s, cam, p, plan))) return rc;
    call.pin(out, outBytes);
    hipError_t err = hipSuccess;
    for (int i = 0; i < plan.n && err == hipSuccess; ++i) err = hipStreamWaitEvent(c->stream, c->syncEvents[2 + i], 0);
    if (err != hipSuccess) return hipFail(err, "ft_render_colors");
    if ((rc = ft_tone_map(c, c->scratch, p->width, p->height, tm, out, max_out))) return rc;
    call.waitedFor = true;
    return ft_collect_stats(c, st);
}

// ---- ray buffers ------------------------------------------------------------------------------------
// The kernel knows two kinds of ray buffer: SdfScene.trace, which in the EXTENSION builds can also store every ray's SdfObject.tryTrace record and
// material handle, or only those, without shading; and SdfForm.tryTrace, whose 10-dword results take the colours' place.  SdfObject.tryTrace
// itself is the first kind asked for its records, which it cannot do without.  Shade is no ray buffer but runs through the same path: the input is
// n hit records (ft_object_trace_result, 64 B each), the output their colours under the scene's lights (the *_shade builds of the reference kernels).
// Visibility is Shade with one uint32 mask per record for a result (the *_vis builds): which lights' shadow rays missed.  The masks travel where the
// material plane does (Outputs::material: 4 B per record, 4-byte aligned); what else the call needs is its VisRequest.
enum class RayKind { Trace, Form, Object, Shade, Visibility };
static bool takesRecords(RayKind k) { return k == RayKind::Shade || k == RayKind::Visibility; }
static size_t inputStride(RayKind k) { return takesRecords(k) ? sizeof(ft_object_trace_result) : sizeof(ft_ray); }
struct VisRequest { uint32_t select; const void* in; };              // ft_light_visibility: the lights to march, the masks to keep the other bits of (NULL: none)
static uint32_t lightBits(const ft_scene* s) { return s->dev.nLights >= 32u ? 0xffffffffu : (1u << s->dev.nLights) - 1u; }

namespace {

// Everything is device memory: the kernel reads d_rays and writes the caller's buffers on the context's stream, with no scratch, no copy and
// no synchronisation.  The device is asked for first, then the arguments.
int launchRayBuffer(ft_ctx* c, const ft_scene* s, const void* d_rays, int64_t n, RayKind kind, const Outputs& o, const VisRequest* vis = nullptr) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!s || s->ctx != c || !d_rays || n < 0) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    if ((rc = checkOutputs(o, true))) return rc;
    if (kind == RayKind::Object && !o.hits) return setErr(FT_ERR_INVALID, "ray buffer: no output asked for");
    if (reinterpret_cast<uintptr_t>(d_rays) & 15u) return setErr(FT_ERR_INVALID, "ray buffer: the rays (hit records) must be 16-byte aligned");
    if (d_rays == o.rgb || d_rays == o.hits || d_rays == o.material) return setErr(FT_ERR_INVALID, "ray buffer: input and output must not overlap");
    if (n == 0) return FT_OK;
    if (n >= 0xFFFF0000ll) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 rays in one call");
    FtRenderArgs a{};
    a.mode = kind == RayKind::Form ? 2u : 1u; a.rays = static_cast<const ft_ray*>(d_rays);
    if (kind == RayKind::Shade) {                                      // records in, colours out: the SHADE builds read hitsIn and nothing of the ray fields
        if (!o.rgb || o.extra()) return setErr(FT_ERR_INVALID, "internal: ft_shade_hits writes colours only");
        a.mode = 3u; a.rays = nullptr; a.shade = 1u; a.hitsIn = static_cast<const float*>(d_rays);
    }
    if (kind == RayKind::Visibility) {                                 // records in, masks out: the same marches, no colour
        if (!vis || !o.material || o.rgb || o.hits) return setErr(FT_ERR_INVALID, "internal: ft_light_visibility writes masks only");
        a.mode = 3u; a.rays = nullptr; a.shade = 2u; a.hitsIn = static_cast<const float*>(d_rays);
        a.visSel = vis->select & lightBits(s); a.visKeep = ~vis->select & lightBits(s);
        a.visIn = static_cast<const uint32_t*>(vis->in); a.visOut = static_cast<uint32_t*>(o.material);
    }
    a.nJobs = (uint32_t)n; a.stripeW = 1; a.stripeRanks = 1; a.tilesY = 1; a.H = 1; a.W = 1; a.nCols = 1; a.maxSize = 1.0f;
    a.spp = 1; a.sppN = 1; a.jobsPerPlane = a.nJobs; a.planePixels = a.nJobs;
    // the same rules as a frame's (frameArgs): the hit buffers exist in the EXTENSION builds only, and plain SdfScene.trace stays on the
    // reference kernels (carved ones included)
    a.out = static_cast<float*>(o.rgb);
    if (kind == RayKind::Visibility) return launchTrace(c, s, a);     // its masks are no material plane: no EXTENSION build, no hit buffers
    a.ext = (kind == RayKind::Form || o.extra()) ? 1u : 0u;
    if (o.extra()) { a.hits = o.rgb ? 1u : 2u; a.hitsOut = static_cast<float*>(o.hits); }
    a.matOut = static_cast<int32_t*>(o.material); a.matHandles = s->dMatHandles;
    return launchTrace(c, s, a);
}

// The host forms: rays up into the context's scratch, the device form, every output asked for down again (HostStaging; the destinations are
// not pinned); nothing of the call is left in flight when it returns.
int traceRayBuffer(ft_ctx* c, const ft_scene* s, const void* rays, int64_t n, RayKind kind, const Outputs& host, ft_stats* st) {
    static_assert(sizeof(ft_ray) == 32 && sizeof(ft_form_trace_result) == 40 && sizeof(ft_object_trace_result) == 64, "layout");
    const size_t inBytes = (size_t)n * inputStride(kind);
    int rc = requireDevice(c); if (rc) return rc;
    if (!s || s->ctx != c || !rays || !host.any() || n < 0) return setErr(FT_ERR_INVALID, "bad argument");
    if (n == 0) { if (st) memset(st, 0, sizeof(*st)); return FT_OK; }
    if (n >= 0xFFFF0000ll) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 rays in one call");
    HostStaging stage(c, "ray buffer", outputParts(host, kind == RayKind::Form ? sizeof(ft_form_trace_result) : 12), false);
    if ((rc = stage.plan(inBytes, (size_t)n))) return rc;
    if ((rc = stage.upload(0, rays, inBytes))) return rc;
    stage.copyOut(launchRayBuffer(c, s, stage.input(), n, kind, stage.dev()), 0, (size_t)n, (size_t)n);
    return stage.finish(st);
}

}  // namespace

int ft_trace_rays_device(ft_ctx* c, const ft_scene* s, const void* d_rays, int64_t n, void* d_out_rgb) {
    return launchRayBuffer(c, s, d_rays, n, RayKind::Trace, Outputs{d_out_rgb, nullptr, nullptr});
}
int ft_form_try_trace_device(ft_ctx* c, const ft_scene* s, const void* d_rays, int64_t n, void* d_out) {
    return launchRayBuffer(c, s, d_rays, n, RayKind::Form, Outputs{d_out, nullptr, nullptr});
}
int ft_object_try_trace_device(ft_ctx* c, const ft_scene* s, const void* d_rays, int64_t n, void* d_out, void* d_material) {
    return launchRayBuffer(c, s, d_rays, n, RayKind::Object, Outputs{nullptr, d_out, d_material});
}
int ft_trace_rays_hits_device(ft_ctx* c, const ft_scene* s, const void* d_rays, int64_t n, void* d_out_rgb, void* d_hits, void* d_material) {
    return launchRayBuffer(c, s, d_rays, n, RayKind::Trace, Outputs{d_out_rgb, d_hits, d_material});
}

int ft_trace_rays(ft_ctx* c, const ft_scene* s, const ft_ray* rays, int64_t n, float* out, ft_stats* st) {
    return traceRayBuffer(c, s, rays, n, RayKind::Trace, Outputs{out, nullptr, nullptr}, st);
}
int ft_form_try_trace(ft_ctx* c, const ft_scene* s, const ft_ray* rays, int64_t n, ft_form_trace_result* out, ft_stats* st) {
    return traceRayBuffer(c, s, rays, n, RayKind::Form, Outputs{out, nullptr, nullptr}, st);
}
int ft_object_try_trace(ft_ctx* c, const ft_scene* s, const ft_ray* rays, int64_t n, ft_object_trace_result* out, ft_stats* st) {
    return traceRayBuffer(c, s, rays, n, RayKind::Object, Outputs{nullptr, out, nullptr}, st);
}
int ft_trace_rays_hits(ft_ctx* c, const ft_scene* s, const ft_ray* rays, int64_t n, float* out_rgb, ft_object_trace_result* out_hits,
                       int32_t* out_material, ft_stats* st) {
    return traceRayBuffer(c, s, rays, n, RayKind::Trace, Outputs{out_rgb, out_hits, out_material}, st);
}

// ---- ft_shade_hits: hit records shaded under the scene's lights (SdfScene.fs:11-28) ------------------------------------
// The one check of the three record forms (ft_shade_hits, ft_light_visibility, ft_shade_visible).  Everything that can be refused without a device
// is refused first, the device is asked for last (like the views forms): the statuses do not depend on the context having a GPU.
// `masks` and what they are to the call: ft_shade_hits has none; ft_light_visibility's vis_in may be NULL and may be its output vis_out (an update in
// place); ft_shade_visible needs its visibility and refuses to shade into it.  `out`: the colours, or vis_out.  A visibility mask has 32 bits: a scene
// with more lights is refused by the two calls that have masks.  *nothing: n = 0, FT_OK with nothing to do.
enum class Masks { None, Updated, Read };
static int checkRecords(const char* what, Masks use, const ft_ctx* c, const ft_scene* s, const void* hits, int64_t n, const void* masks, const void* out,
                        bool deviceMemory, bool* nothing) {
    *nothing = false;
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (!s || s->ctx != c || !hits || !out || (use == Masks::Read && !masks) || n < 0) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    if (deviceMemory) {
        if (reinterpret_cast<uintptr_t>(hits) & 15u) return setErr(FT_ERR_INVALID, std::string(what) + "_device: the hit records must be 16-byte aligned");
        if ((reinterpret_cast<uintptr_t>(masks) | reinterpret_cast<uintptr_t>(out)) & 3u)
            return setErr(FT_ERR_INVALID, std::string(what) + (use == Masks::None ? "_device: the colours must be 4-byte aligned" : "_device: the masks and the colours must be 4-byte aligned"));
    }
    if (hits == out || (use == Masks::Read && masks == out)) return setErr(FT_ERR_INVALID, std::string(what) + ": input and output must not overlap");
    if (n >= 0xFFFF0000ll) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 records in one call");
    if (use != Masks::None && s->dev.nLights > 32u) return setErr(FT_ERR_UNSUPPORTED, "a visibility mask holds 32 lights; the scene has " + std::to_string(s->dev.nLights));
    *nothing = n == 0;
    return FT_OK;
}
int ft_shade_hits_device(ft_ctx* c, const ft_scene* s, const void* d_hits, int64_t n, void* d_out_rgb) {
    bool nothing;
    int rc = checkRecords("ft_shade_hits", Masks::None, c, s, d_hits, n, nullptr, d_out_rgb, true, &nothing); if (rc || nothing) return rc;
    return launchRayBuffer(c, s, d_hits, n, RayKind::Shade, Outputs{d_out_rgb, nullptr, nullptr});
}
int ft_shade_hits(ft_ctx* c, const ft_scene* s, const ft_object_trace_result* hits, int64_t n, float* out_rgb, ft_stats* st) {
    bool nothing;
    int rc = checkRecords("ft_shade_hits", Masks::None, c, s, hits, n, nullptr, out_rgb, false, &nothing); if (rc) return rc;
    if (nothing) { if (st) memset(st, 0, sizeof(*st)); return FT_OK; }
    return traceRayBuffer(c, s, hits, n, RayKind::Shade, Outputs{out_rgb, nullptr, nullptr}, st);
}

// ---- ft_light_visibility / ft_shade_visible: the shadow marches kept as one bit per (record, light), and shading from those bits -------------
// Both go through checkRecords: refusals first, the device last.
int ft_light_visibility_device(ft_ctx* c, const ft_scene* s, const void* d_hits, int64_t n, uint32_t select, const void* d_vis_in, void* d_vis_out) {
    bool nothing;
    int rc = checkRecords("ft_light_visibility", Masks::Updated, c, s, d_hits, n, d_vis_in, d_vis_out, true, &nothing); if (rc || nothing) return rc;
    const VisRequest vis{select, d_vis_in};
    return launchRayBuffer(c, s, d_hits, n, RayKind::Visibility, Outputs{nullptr, nullptr, d_vis_out}, &vis);
}
// host form: [records | masks to keep] up into the scratch, the device form, the masks down (HostStaging's material plane: 4 B per record).  vis_in may
// be vis_out: it has gone up before anything comes down, on one stream.
int ft_light_visibility(ft_ctx* c, const ft_scene* s, const ft_object_trace_result* hits, int64_t n, uint32_t select, const uint32_t* vis_in,
                        uint32_t* vis_out, ft_stats* st) {
    bool nothing;
    int rc = checkRecords("ft_light_visibility", Masks::Updated, c, s, hits, n, vis_in, vis_out, false, &nothing); if (rc) return rc;
    if (nothing) { if (st) memset(st, 0, sizeof(*st)); return FT_OK; }
    if ((rc = requireDevice(c))) return rc;
    const size_t recBytes = (size_t)n * sizeof(ft_object_trace_result), keepAt = align256(recBytes);
    HostStaging stage(c, "light visibility", outputParts(Outputs{nullptr, nullptr, vis_out}), false);
    if ((rc = stage.plan(keepAt + (vis_in ? (size_t)n * 4 : 0), (size_t)n))) return rc;
    if ((rc = stage.upload(0, hits, recBytes))) return rc;
    if (vis_in && (rc = stage.upload(keepAt, vis_in, (size_t)n * 4))) return rc;
    const VisRequest vis{select, vis_in ? stage.input(keepAt) : nullptr};
    stage.copyOut(launchRayBuffer(c, s, stage.input(), n, RayKind::Visibility, stage.dev(), &vis), 0, (size_t)n, (size_t)n);
    return stage.finish(st);
}

// its own kernel, not a trace launch: no job queue, no LDS, no counters; timed like one (ft_collect_stats adds the pair up)
static int launchShadeVisible(ft_ctx* c, const ft_scene* s, const void* d_hits, const void* d_vis, int64_t n, void* d_out) {
    int rc = requireDevice(c); if (rc) return rc;
    return timedLaunch(c, c->stream, "ft_launch_shade_visible", [&] {
        return ft_launch_shade_visible(s->dev.lights, s->dev.nLights, s->dev.bg, static_cast<const float*>(d_hits), static_cast<const uint32_t*>(d_vis),
                                       (uint32_t)n, static_cast<float*>(d_out), c->stream);
    });
}
int ft_shade_visible_device(ft_ctx* c, const ft_scene* s, const void* d_hits, const void* d_visibility, int64_t n, void* d_out_rgb) {
    bool nothing;
    int rc = checkRecords("ft_shade_visible", Masks::Read, c, s, d_hits, n, d_visibility, d_out_rgb, true, &nothing); if (rc || nothing) return rc;
    return launchShadeVisible(c, s, d_hits, d_visibility, n, d_out_rgb);
}
int ft_shade_visible(ft_ctx* c, const ft_scene* s, const ft_object_trace_result* hits, const uint32_t* visibility, int64_t n, float* out_rgb,
                     ft_stats* st) {
    bool nothing;
    int rc = checkRecords("ft_shade_visible", Masks::Read, c, s, hits, n, visibility, out_rgb, false, &nothing); if (rc) return rc;
    if (nothing) { if (st) memset(st, 0, sizeof(*st)); return FT_OK; }
    if ((rc = requireDevice(c))) return rc;
    const size_t recBytes = (size_t)n * sizeof(ft_object_trace_result), visAt = align256(recBytes);
    HostStaging stage(c, "shade visible", outputParts(Outputs{out_rgb, nullptr, nullptr}), false);
    if ((rc = stage.plan(visAt + (size_t)n * 4, (size_t)n))) return rc;
    if ((rc = stage.upload(0, hits, recBytes))) return rc;
    if ((rc = stage.upload(visAt, visibility, (size_t)n * 4))) return rc;
    stage.copyOut(launchShadeVisible(c, s, stage.input(), stage.input(visAt), n, stage.part(0)), 0, (size_t)n, (size_t)n);
    return stage.finish(st);
}

int ft_eval_distance(ft_ctx* c, const ft_scene* s, const ft_vec3* pts, int64_t n, float* outD, int32_t* outM) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!s || s->ctx != c || !pts || !outD || n < 0) return setErr(FT_ERR_INVALID, "bad argument");
    if (n == 0) return FT_OK;
    const size_t pBytes = align256((size_t)n * 12), dBytes = align256((size_t)n * 4), mBytes = (size_t)n * 4;
    if ((rc = ensureScratch(c, pBytes + dBytes + mBytes))) return rc;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    HIP_TRY(hipMemcpyAsync(base, pts, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    const unsigned blocks = (unsigned)std::min<int64_t>((n + FT_BLOCK - 1) / FT_BLOCK, (int64_t)c->numCUs * 8);
    const bool libm = libmLaunch(c, s);
    FtSceneDev dev = s->dev;
    dev.mathFma = c->optMath == FT_MATH_GLIBC_FMA ? 1u : 0u;
    const size_t lds = 4u * (size_t)ft_lds_layout(dev.nSlots, dev.nStage, libm, dev.fastPath == 1u).total;    // all slots: the general interpreter
    HIP_TRY(ft_launch_eval_points(&dev, libm ? 1 : 0, reinterpret_cast<const float*>(base), n, reinterpret_cast<float*>(base + pBytes),
                                  reinterpret_cast<int*>(base + pBytes + dBytes), blocks, lds, c->stream));
    HIP_TRY(hipMemcpyAsync(outD, base + pBytes, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (outM) HIP_TRY(hipMemcpyAsync(outM, base + pBytes + dBytes, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}

// ---- field sampling: ft_sample_points, ft_sample_lattice and their *_device forms (kernels.hip "Field sampling") -----------------
namespace {

// points (n of them) or a lattice, and where the results go: every address is host or device memory as the entry point says
struct FieldRequest { const void* points; int64_t n; const ft_lattice* lat; float eps; uint32_t flags; void* dist; void* normal; void* material; };
int64_t fieldCount(const FieldRequest& r) { return r.lat ? (int64_t)r.lat->nx * r.lat->ny * r.lat->nz : r.n; }

// Everything that can be refused without a device, in the header's order.  *nothing: FT_OK with nothing to launch.
int checkField(const ft_ctx* c, const ft_scene* s, const FieldRequest& r, bool deviceMemory, bool* nothing) {
    static_assert(sizeof(ft_lattice) == 36, "layout");
    *nothing = false;
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (!s || s->ctx != c) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    if (!r.dist && !r.normal && !r.material) return setErr(FT_ERR_INVALID, "field: no output asked for");
    if (r.flags & ~(uint32_t)FT_FIELD_BOUNDED) return setErr(FT_ERR_INVALID, "field: unknown flag bits");
    if (r.lat) {
        const int32_t cnt[3] = {r.lat->nx, r.lat->ny, r.lat->nz};
        for (int32_t v : cnt) if (v < 1 || v > 16777216) return setErr(FT_ERR_INVALID, "lattice: every count must be 1 .. 16777216");
    } else if (!r.points || r.n < 0) return setErr(FT_ERR_INVALID, "field: null points or a negative count");
    if (deviceMemory) {
        const void* all[4] = {r.points, r.dist, r.normal, r.material};
        for (const void* p : all) if (reinterpret_cast<uintptr_t>(p) & 3u) return setErr(FT_ERR_INVALID, "field: every device buffer must be 4-byte aligned");
    }
    if (r.points && (r.points == r.dist || r.points == r.normal || r.points == r.material)) return setErr(FT_ERR_INVALID, "field: input and output must not overlap");
    if ((r.dist && (r.dist == r.normal || r.dist == r.material)) || (r.normal && r.normal == r.material)) return setErr(FT_ERR_INVALID, "field: outputs must not overlap");
    // three counts of at most 2^24: the product of two fits 2^48, and the third is applied only below the limit
    const uint64_t total = r.lat ? (uint64_t)r.lat->nx * (uint64_t)r.lat->ny : (uint64_t)r.n;
    if (total >= 0xFFFF0000ull || (r.lat && total * (uint64_t)r.lat->nz >= 0xFFFF0000ull)) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 points in one call");
    *nothing = !r.lat && r.n == 0;
    return FT_OK;
}

// the launch: device memory throughout, the context's stream, not synchronised; the arguments have passed checkField and the context has a device
int launchField(ft_ctx* c, const ft_scene* s, const FieldRequest& r) {
    KernelPlan plan;
    int rc = planTrace(c, s, false, 0u, plan); if (rc) return rc;
    FtFieldArgs a{};
    a.S = s->dev;
    a.S.fastPath = plan.variant;
    a.S.nSlots = plan.nSlots;
    a.S.mathFma = c->optMath == FT_MATH_GLIBC_FMA ? 1u : 0u;
    a.carve = s->carve;
    a.math = plan.libm ? 1u : 0u;
    a.cull = (s->dev.cullPc != 0xffffffffu && plan.cullRows && c->optCull) ? 1u : 0u;
    // The brick of a wave, by measurement (256^3 lattices, kernel ms for 4x4x4 / 2x4x8 / 2x2x16, profiles/field_probe.jsonl): the lean kernel gains from the
    // tightest culling ball, C3 1.78 / 1.86 / 1.91; the grid-union kernels from longer runs along k, whose lanes share lookup cells and whose stores are
    // contiguous — 1000 tori 0.395 / 0.378 / 0.403, combinator crowd (128^3) 0.393 / 0.357 / 0.363
    static const uint32_t bricks[3][2] = FT_FIELD_BRICKS;
    const int brick = c->fieldBrick >= 0 ? c->fieldBrick : (plan.variant == 1u ? 0 : FT_FIELD_BRICK_DEFAULT);
    a.lgJ = bricks[brick][0]; a.lgK = bricks[brick][1];
    if (r.lat) {
        const ft_lattice& l = *r.lat;
        a.origin[0] = l.origin.x; a.origin[1] = l.origin.y; a.origin[2] = l.origin.z;
        a.step[0] = l.step.x; a.step[1] = l.step.y; a.step[2] = l.step.z;
        a.nx = (uint32_t)l.nx; a.ny = (uint32_t)l.ny; a.nz = (uint32_t)l.nz;
        const uint32_t lgI = 6u - a.lgJ - a.lgK;
        const uint64_t bi = ((uint64_t)a.nx + (1u << lgI) - 1u) >> lgI, bj = ((uint64_t)a.ny + (1u << a.lgJ) - 1u) >> a.lgJ, bk = ((uint64_t)a.nz + (1u << a.lgK) - 1u) >> a.lgK;
        a.bricksJ = (uint32_t)bj; a.bricksK = (uint32_t)bk;
        a.nJobs = (uint32_t)(bi * bj * bk);                            // a brick count is at most its axis' point count: the product stays below 2^32
    } else {
        a.pts = static_cast<const float*>(r.points);
        a.n = (uint32_t)r.n;
        a.nJobs = (uint32_t)(((uint64_t)r.n + 63u) >> 6);
    }
    a.bounded = (r.flags & FT_FIELD_BOUNDED) ? 1u : 0u;
    const ft::Boundary& b = s->flat.boundary;
    a.bc[0] = b.center.x; a.bc[1] = b.center.y; a.bc[2] = b.center.z; a.br2 = b.radius * b.radius;
    a.normalEps = r.normal ? r.eps : 0.0f;
    a.outD = static_cast<float*>(r.dist); a.outN = static_cast<float*>(r.normal); a.outM = static_cast<int32_t*>(r.material);
    a.matHandles = s->dMatHandles; a.nMaterials = (uint32_t)s->flat.materialHandles.size();
    int perCU = 0;
    HIP_TRY(ft_field_occupancy(plan.variant, a.carve.kind, plan.libm, plan.lds, &perCU));
    if ((rc = clampPerCU(c, "field", perCU))) return rc;
    const uint64_t wantBlocks = ((uint64_t)a.nJobs + (FT_BLOCK / 64) - 1) / (FT_BLOCK / 64);
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->numCUs * perCU, wantBlocks));
    return timedLaunch(c, c->stream, "ft_launch_field", [&] { return ft_launch_field(&a, blocks, plan.lds, c->stream); });
}

int sampleDevice(ft_ctx* c, const ft_scene* s, const FieldRequest& r) {
    bool nothing;
    int rc = checkField(c, s, r, true, &nothing); if (rc || nothing) return rc;
    if ((rc = requireDevice(c))) return rc;
    return launchField(c, s, r);
}

// the host forms: [points | distance | normal | material] in the context's scratch (HostStaging); the lattice form uploads nothing.  They return no
// statistics, so nothing is collected: the launch's event pair stays pending for the caller's next ft_collect_stats
int sampleHost(ft_ctx* c, const ft_scene* s, const FieldRequest& r) {
    bool nothing;
    int rc = checkField(c, s, r, false, &nothing); if (rc || nothing) return rc;
    if ((rc = requireDevice(c))) return rc;
    const size_t n = (size_t)fieldCount(r), inBytes = r.points ? n * 12 : 0;
    HostStaging stage(c, "field", HostParts{{{r.dist, 4}, {r.normal, 12}, {r.material, 4}}}, false);
    if ((rc = stage.plan(inBytes, n))) return rc;
    if (r.points && (rc = stage.upload(0, r.points, inBytes))) return rc;
    FieldRequest d = r;
    d.points = r.points ? stage.input() : nullptr;
    d.dist = stage.part(0); d.normal = stage.part(1); d.material = stage.part(2);
    stage.copyOut(launchField(c, s, d), 0, n, n);
    return stage.finish();
}

}  // namespace

int ft_sample_points(ft_ctx* c, const ft_scene* s, const ft_vec3* points, int64_t n, float normal_epsilon, uint32_t flags,
                     float* out_distance, ft_vec3* out_normal, int32_t* out_material) {
    return sampleHost(c, s, FieldRequest{points, n, nullptr, normal_epsilon, flags, out_distance, out_normal, out_material});
}
int ft_sample_points_device(ft_ctx* c, const ft_scene* s, const void* d_points, int64_t n, float normal_epsilon, uint32_t flags,
                            void* d_distance, void* d_normal, void* d_material) {
    return sampleDevice(c, s, FieldRequest{d_points, n, nullptr, normal_epsilon, flags, d_distance, d_normal, d_material});
}
int ft_sample_lattice(ft_ctx* c, const ft_scene* s, const ft_lattice* lattice, float normal_epsilon, uint32_t flags,
                      float* out_distance, ft_vec3* out_normal, int32_t* out_material) {
    if (!lattice) return setErr(FT_ERR_INVALID, "null lattice");
    return sampleHost(c, s, FieldRequest{nullptr, 0, lattice, normal_epsilon, flags, out_distance, out_normal, out_material});
}
int ft_sample_lattice_device(ft_ctx* c, const ft_scene* s, const ft_lattice* lattice, float normal_epsilon, uint32_t flags,
                             void* d_distance, void* d_normal, void* d_material) {
    if (!lattice) return setErr(FT_ERR_INVALID, "null lattice");
    return sampleDevice(c, s, FieldRequest{nullptr, 0, lattice, normal_epsilon, flags, d_distance, d_normal, d_material});
}
// Internal (not in the header, like ft_ctx_tile_order_rule; tools/field_probe.py): the brick shape of this context's lattice launches, an index into
// FT_FIELD_BRICKS (0: 4x4x4, 1: 2x4x8, 2: 2x2x16), or -1 for the shipped rule (launchField: by kernel family).  Every shape gives the same bits.
int ft_ctx_field_brick(ft_ctx* c, int32_t shape) {
    if (!c || shape < -1 || shape > 2) return setErr(FT_ERR_INVALID, "bad argument");
    c->fieldBrick = shape;
    return FT_OK;
}

// ---- refinement: brackets bisected onto the surface (refine.hip; the rule is the header's "Refinement").  What the refined constructors and
// ft_refine_segments share ----
namespace {

// the context's refinement work for n brackets: [A x y z | B x y z | sA | sB | M (n x 3) | D(M) | D(b) for segments], every array on a 256-byte boundary
struct RefineWork { size_t arr[8], mid, dist, distB, end; };
RefineWork refineWork(size_t n, bool segments) {
    RefineWork w{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    for (size_t& o : w.arr) o = take(n * 4);
    w.mid = take(n * 12); w.dist = take(n * 4); w.distB = segments ? take(n * 4) : 0;
    w.end = at;
    return w;
}
// the argument block over the context's work (already ensured): everything but what says where the brackets come from
FtRefineArgs refineArgs(ft_ctx* c, const RefineWork& w, size_t n, float iso) {
    FtRefineArgs g{};
    unsigned char* wk = static_cast<unsigned char*>(c->refineWork);
    auto floats = [&](size_t o) { return reinterpret_cast<float*>(wk + o); };
    for (int ax = 0; ax < 3; ++ax) { g.br.a[ax] = floats(w.arr[ax]); g.br.b[ax] = floats(w.arr[3 + ax]); }
    g.br.sa = floats(w.arr[6]); g.br.sb = floats(w.arr[7]);
    g.mid = floats(w.mid); g.dist = floats(w.dist);
    g.iso = iso; g.nV = (uint32_t)n;
    return g;
}
int launchRefine(ft_ctx* c, int kernel, const FtRefineArgs& g, uint64_t items) {
    static const char* const names[FT_REFINE_KERNELS] = {"refine lattice", "refine segments", "refine round"};
    int perCU = 0;
    const hipError_t e = ft_refine_occupancy(kernel, &perCU);
    if (e != hipSuccess) return hipFail(e, (std::string("occupancy of the ") + names[kernel] + " kernel").c_str());
    int rc = clampPerCU(c, names[kernel], perCU); if (rc) return rc;
    const uint64_t want = (items + FT_REFINE_BLOCK - 1) / FT_REFINE_BLOCK;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->numCUs * perCU, want));
    return timedLaunch(c, c->stream, "ft_launch_refine", [&] { return ft_launch_refine(kernel, &g, blocks, c->stream); });
}
// `first` (lattice or segments: it forms the brackets and, with no round, finishes them), then per round one points-form field launch over the midpoint
// buffer, distance only, and the round kernel; the last round writes the finish into `out` (n x 3).  1 + 2 * steps launches on the context's stream,
// none synchronised.
int launchRefinement(ft_ctx* c, const ft_scene* s, int first, uint64_t firstItems, FtRefineArgs g, int32_t steps, float* out) {
    g.out = out;
    g.last = steps == 0 ? 1u : 0u;
    int rc = launchRefine(c, first, g, firstItems); if (rc) return rc;
    for (int32_t r = 0; r < steps; ++r) {
        if (!c->refineSkipField && (rc = launchField(c, s, FieldRequest{g.mid, (int64_t)g.nV, nullptr, 0.0f, 0u, const_cast<float*>(g.dist), nullptr, nullptr}))) return rc;
        g.last = r + 1 == steps ? 1u : 0u;
        if ((rc = launchRefine(c, FT_REFINE_K_ROUND, g, g.nV))) return rc;
    }
    return FT_OK;
}
// the brackets of a lattice's owned edges (mask and vbase: what the count and emit passes left in the context's scratch), refined into `out` (nV x 3)
int refineLattice(ft_ctx* c, const ft_scene* s, const ft_lattice& l, const float* dValues, const uint8_t* mask, const uint32_t* vbase, uint32_t edges,
                  float iso, size_t nV, int32_t steps, float* out) {
    FtRefineArgs g = refineArgs(c, refineWork(nV, false), nV, iso);
    g.values = dValues;
    g.nx = (uint32_t)l.nx; g.ny = (uint32_t)l.ny; g.nz = (uint32_t)l.nz;
    g.n = g.nx * g.ny * g.nz;
    g.origin[0] = l.origin.x; g.origin[1] = l.origin.y; g.origin[2] = l.origin.z;
    g.step[0] = l.step.x; g.step[1] = l.step.y; g.step[2] = l.step.z;
    g.mask = mask; g.vbase = vbase; g.edges = edges;
    return launchRefinement(c, s, FT_REFINE_K_LATTICE, g.n, g, steps, out);
}

struct SegmentsRequest { const void* a; const void* b; int64_t n; float iso; int32_t steps; void* point; void* status; };

// Everything that can be refused without a device, in ft_sample_points' order.  *nothing: FT_OK with nothing to launch.
int checkSegments(const ft_ctx* c, const ft_scene* s, const SegmentsRequest& r, bool deviceMemory, bool* nothing) {
    *nothing = false;
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (!s || s->ctx != c) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    if (!r.point && !r.status) return setErr(FT_ERR_INVALID, "refine: no output asked for");
    if (r.steps < 0 || r.steps > FT_REFINE_MAX_STEPS) return setErr(FT_ERR_INVALID, "refine: the steps must be 0 .. 32");
    if (!r.a || !r.b || r.n < 0) return setErr(FT_ERR_INVALID, "refine: null segment ends or a negative count");
    const void* all[4] = {r.a, r.b, r.point, r.status};
    if (deviceMemory)
        for (const void* p : all) if (reinterpret_cast<uintptr_t>(p) & 3u) return setErr(FT_ERR_INVALID, "refine: every device buffer must be 4-byte aligned");
    for (int i = 0; i < 2; ++i) if (all[i] == r.point || all[i] == r.status) return setErr(FT_ERR_INVALID, "refine: input and output must not overlap");
    if (r.point && r.point == r.status) return setErr(FT_ERR_INVALID, "refine: outputs must not overlap");
    if ((uint64_t)r.n >= 0xFFFF0000ull) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 points in one call");
    *nothing = r.n == 0;
    return FT_OK;
}
// the launches: device memory throughout, the context's stream, not synchronised; the arguments have passed checkSegments, the context has a device
int launchSegments(ft_ctx* c, const ft_scene* s, const SegmentsRequest& r) {
    const size_t n = (size_t)r.n;
    const RefineWork w = refineWork(n, true);
    int rc = ensureBytes(c->refineWork, c->refineWorkBytes, w.end); if (rc) return rc;
    FtRefineArgs g = refineArgs(c, w, n, r.iso);
    float* distB = reinterpret_cast<float*>(static_cast<unsigned char*>(c->refineWork) + w.distB);
    g.segA = static_cast<const float*>(r.a); g.segB = static_cast<const float*>(r.b);
    g.distA = g.dist; g.distB = distB;
    g.status = static_cast<int32_t*>(r.status);
    if ((rc = launchField(c, s, FieldRequest{r.a, r.n, nullptr, 0.0f, 0u, const_cast<float*>(g.dist), nullptr, nullptr}))) return rc;
    if ((rc = launchField(c, s, FieldRequest{r.b, r.n, nullptr, 0.0f, 0u, distB, nullptr, nullptr}))) return rc;
    if (!r.point) g.mid = nullptr;                                     // only the status: no bracket is kept, no round runs
    return launchRefinement(c, s, FT_REFINE_K_SEGMENTS, n, g, r.point ? r.steps : 0, static_cast<float*>(r.point));
}

}  // namespace

int ft_refine_segments_device(ft_ctx* c, const ft_scene* s, const void* d_a, const void* d_b, int64_t n, float iso, int32_t steps, void* d_point, void* d_status) {
    const SegmentsRequest r{d_a, d_b, n, iso, steps, d_point, d_status};
    bool nothing;
    int rc = checkSegments(c, s, r, true, &nothing); if (rc || nothing) return rc;
    if ((rc = requireDevice(c))) return rc;
    return launchSegments(c, s, r);
}
// host form: [a | b | point | status] in the context's scratch (HostStaging), the device form, the outputs down; synchronises
int ft_refine_segments(ft_ctx* c, const ft_scene* s, const ft_vec3* a, const ft_vec3* b, int64_t n, float iso, int32_t steps, ft_vec3* out_point, int32_t* out_status) {
    SegmentsRequest r{a, b, n, iso, steps, out_point, out_status};
    bool nothing;
    int rc = checkSegments(c, s, r, false, &nothing); if (rc || nothing) return rc;
    if ((rc = requireDevice(c))) return rc;
    const size_t count = (size_t)n, bAt = align256(count * 12);
    HostStaging stage(c, "refine", HostParts{{{out_point, 12}, {out_status, 4}, {nullptr, 0}}}, false);
    if ((rc = stage.plan(bAt + count * 12, count))) return rc;
    if ((rc = stage.upload(0, a, count * 12)) || (rc = stage.upload(bAt, b, count * 12))) return rc;
    r.a = stage.input(0); r.b = stage.input(bAt); r.point = stage.part(0); r.status = stage.part(1);
    stage.copyOut(launchSegments(c, s, r), 0, count, count);
    return stage.finish();
}
// Internal (not in the header, like ft_ctx_mesh_tile; the tests): one round of the rule over n caller-given brackets in device memory — eight arrays of n
// floats, `stride` floats apart, in the order A.x A.y A.z B.x B.y B.z sA sB — with their midpoints d_mid (n x 3) and the midpoints' distances d_dist (n).
// last = 0: the brackets are updated in place and d_mid receives the next midpoints; last = 1: d_out (n x 3) receives the finish.  Synchronises.
int ft_ctx_refine_round(ft_ctx* c, void* d_bracket, int64_t stride, void* d_mid, const void* d_dist, int64_t n, float iso, int32_t last, void* d_out) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!d_bracket || !d_mid || !d_dist || n < 1 || stride < n || (uint64_t)n >= 0xFFFF0000ull || (last && !d_out)) return setErr(FT_ERR_INVALID, "bad argument");
    FtRefineArgs g{};
    float* base = static_cast<float*>(d_bracket);
    for (int ax = 0; ax < 3; ++ax) { g.br.a[ax] = base + (size_t)ax * stride; g.br.b[ax] = base + (size_t)(3 + ax) * stride; }
    g.br.sa = base + (size_t)6 * stride; g.br.sb = base + (size_t)7 * stride;
    g.mid = static_cast<float*>(d_mid); g.dist = static_cast<const float*>(d_dist);
    g.iso = iso; g.nV = (uint32_t)n; g.last = last ? 1u : 0u; g.out = static_cast<float*>(d_out);
    if ((rc = launchRefine(c, FT_REFINE_K_ROUND, g, (uint64_t)n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}
// Internal (tools/refine_probe.py): skip_field = 1 this context's refinements launch everything but their field rounds (the midpoints' distances are
// whatever the work buffer holds, so the positions are not the rule's), so that the field rounds' kernel time is a difference of two figures
int ft_ctx_refine_probe(ft_ctx* c, int32_t skip_field) {
    if (!c || skip_field < 0 || skip_field > 1) return setErr(FT_ERR_INVALID, "bad argument");
    c->refineSkipField = skip_field;
    return FT_OK;
}

// ---- meshing: ft_mesh_lattice, ft_mesh_values, ft_mesh_values_device and what reads a mesh (mesh.hip; the rule is the header's "Meshing") ----------
struct ft_mesh {
    ft_ctx* ctx = nullptr;
    int64_t nV = 0, nT = 0, nSkipped = 0;
    uint64_t serial = 0;                                   // unique per mesh of the process: what an ft_shells remembers of the mesh it was built from
    bool hasNormal = false, hasMaterial = false;
    void* dVertices = nullptr; void* dTriangles = nullptr; void* dNormals = nullptr; void* dMaterials = nullptr;
};

namespace {

// the scene (scene form only), the lattice, its values (values forms only; host or device memory as the entry point says) and where the mesh goes
// refine: the bisection rounds of ft_mesh_lattice_refined, -1 for the unrefined forms
struct MeshRequest { const ft_scene* s; const ft_lattice* lat; const void* values; float iso, eps; uint32_t flags; ft_mesh** out; int32_t refine = -1; bool refined = false; };
enum class MeshForm { Scene, HostValues, DeviceValues };

ft_mesh* newMesh(ft_ctx* c) {
    static std::atomic<uint64_t> serial{0};
    ft_mesh* m = new ft_mesh();
    m->ctx = c;
    m->serial = ++serial;                                              // never 0: that is "built from no mesh"
    return m;
}

// Everything that can be refused without a device, in the header's order.  *nothing: a count of 1, FT_OK with an empty mesh and nothing to launch.
int checkMesh(const ft_ctx* c, const MeshRequest& r, MeshForm form, bool* nothing) {
    *nothing = false;
    if (r.out) *r.out = nullptr;
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (form == MeshForm::Scene && (!r.s || r.s->ctx != c)) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    if (!r.lat) return setErr(FT_ERR_INVALID, "null lattice");
    if (form != MeshForm::Scene && !r.values) return setErr(FT_ERR_INVALID, "mesh: null values");
    if (!r.out) return setErr(FT_ERR_INVALID, "null out pointer");
    const int32_t cnt[3] = {r.lat->nx, r.lat->ny, r.lat->nz};
    for (int32_t v : cnt) if (v < 1 || v > 16777216) return setErr(FT_ERR_INVALID, "lattice: every count must be 1 .. 16777216");
    if (r.flags & ~(uint32_t)(FT_MESH_NORMAL | FT_MESH_MATERIAL)) return setErr(FT_ERR_INVALID, "mesh: unknown flag bits");
    if (r.refined && (r.refine < 0 || r.refine > FT_REFINE_MAX_STEPS)) return setErr(FT_ERR_INVALID, "mesh: refine_steps must be 0 .. 32");
    if (form == MeshForm::DeviceValues && (reinterpret_cast<uintptr_t>(r.values) & 3u)) return setErr(FT_ERR_INVALID, "mesh: the device values must be 4-byte aligned");
    // three counts of at most 2^24: the product of two fits 2^48, and the third is applied only below the limit
    const uint64_t two = (uint64_t)r.lat->nx * (uint64_t)r.lat->ny;
    if (two >= 0xFFFF0000ull || two * (uint64_t)r.lat->nz >= 0xFFFF0000ull) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 points in one call");
    *nothing = r.lat->nx == 1 || r.lat->ny == 1 || r.lat->nz == 1;
    return FT_OK;
}

// The extraction: values (device memory, n floats) -> m's vertices and triangles.  work: 5 B per point and 12 B per tile behind `workAt` bytes of
// the context's scratch (already ensured).  Synchronises the context's stream once, between the scan and the allocations.
struct MeshWork { size_t mask, vbase, tileV, tileT, tileS, totals, end; };
MeshWork meshWork(size_t at, size_t n, size_t nTiles) {
    MeshWork w{};
    w.mask = align256(at); w.vbase = align256(w.mask + n); w.tileV = align256(w.vbase + 4 * n); w.tileT = align256(w.tileV + 4 * nTiles);
    w.tileS = align256(w.tileT + 4 * nTiles); w.totals = align256(w.tileS + 4 * nTiles); w.end = w.totals + 256;
    return w;
}
int launchMesh(ft_ctx* c, int kernel, const FtMeshArgs& a) {
    int perCU = 0;
    HIP_TRY(ft_mesh_occupancy(kernel, a.tile, &perCU));
    static const char* const names[4] = {"mesh count", "mesh scan", "mesh vertices", "mesh triangles"};
    int rc = clampPerCU(c, names[kernel], perCU); if (rc) return rc;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->numCUs * perCU, a.nTiles));
    return timedLaunch(c, c->stream, "ft_launch_mesh", [&] { return ft_launch_mesh(kernel, &a, blocks, c->stream); });
}
int extractMesh(ft_ctx* c, const ft_lattice& l, const float* dValues, float iso, const MeshWork& w, ft_mesh* m, bool refined) {
    FtMeshArgs a{};
    a.values = dValues; a.iso = iso;
    a.nx = (uint32_t)l.nx; a.ny = (uint32_t)l.ny; a.nz = (uint32_t)l.nz;
    a.n = a.nx * a.ny * a.nz;                                          // below 0xFFFF0000 (checkMesh)
    a.tile = c->meshTile;
    a.nTiles = (uint32_t)(((uint64_t)a.n + a.tile - 1u) / a.tile);
    a.origin[0] = l.origin.x; a.origin[1] = l.origin.y; a.origin[2] = l.origin.z;
    a.step[0] = l.step.x; a.step[1] = l.step.y; a.step[2] = l.step.z;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    a.mask = base + w.mask; a.vbase = reinterpret_cast<uint32_t*>(base + w.vbase);
    a.tileV = reinterpret_cast<uint32_t*>(base + w.tileV); a.tileT = reinterpret_cast<uint32_t*>(base + w.tileT); a.tileS = reinterpret_cast<uint32_t*>(base + w.tileS);
    a.totals = reinterpret_cast<unsigned long long*>(base + w.totals);
    int rc;
    if ((rc = launchMesh(c, FT_MESH_K_COUNT, a)) || (rc = launchMesh(c, FT_MESH_K_SCAN, a))) return rc;
    unsigned long long totals[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                          // the one synchronisation: the outputs cannot be sized before the count
    if (totals[0] >= (1ull << 31) || totals[1] >= (1ull << 31)) return setErr(FT_ERR_UNSUPPORTED, "mesh: 2^31 or more vertices or triangles (the index type is int32)");
    m->nV = (int64_t)totals[0]; m->nT = (int64_t)totals[1]; m->nSkipped = (int64_t)totals[2];
    if (m->nV) HIP_TRY(hipMalloc(&m->dVertices, (size_t)m->nV * 12));
    if (m->nT) HIP_TRY(hipMalloc(&m->dTriangles, (size_t)m->nT * 12));
    if (refined && m->nV && (rc = ensureBytes(c->refineWork, c->refineWorkBytes, refineWork((size_t)m->nV, false).end))) return rc;
    a.vertices = static_cast<float*>(m->dVertices); a.triangles = static_cast<int32_t*>(m->dTriangles);
    a.nV = (uint32_t)m->nV; a.nT = (uint32_t)m->nT;
    if (m->nV && (rc = launchMesh(c, FT_MESH_K_VERTICES, a))) return rc;              // triangles only join vertices: none without them
    if (m->nT && (rc = launchMesh(c, FT_MESH_K_TRIANGLES, a))) return rc;
    return FT_OK;
}

int buildMesh(ft_ctx* c, const MeshRequest& r, MeshForm form) {
    bool nothing;
    int rc = checkMesh(c, r, form, &nothing); if (rc) return rc;
    ft_mesh* m = newMesh(c);
    m->hasNormal = (r.flags & FT_MESH_NORMAL) != 0u; m->hasMaterial = (r.flags & FT_MESH_MATERIAL) != 0u;
    if (nothing) { *r.out = m; return FT_OK; }
    auto fail = [&](int code) { if (c->hasDevice) (void)hipStreamSynchronize(c->stream); ft_mesh_destroy(m); return code; };
    if ((rc = requireDevice(c))) return fail(rc);
    const ft_lattice& l = *r.lat;
    const size_t n = (size_t)l.nx * l.ny * l.nz, tile = c->meshTile, nTiles = (n + tile - 1) / tile;
    const MeshWork w = meshWork(form == MeshForm::DeviceValues ? 0 : n * 4, n, nTiles);
    if ((rc = ensureScratch(c, w.end))) return fail(rc);
    const float* dValues = form == MeshForm::DeviceValues ? static_cast<const float*>(r.values) : static_cast<const float*>(c->scratch);
    if (form == MeshForm::HostValues) {
        const hipError_t e = hipMemcpyAsync(c->scratch, r.values, n * 4, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(hipFail(e, "mesh: upload"));
    } else if (form == MeshForm::Scene) {
        if ((rc = launchField(c, r.s, FieldRequest{nullptr, 0, r.lat, 0.0f, 0u, c->scratch, nullptr, nullptr}))) return fail(rc);
    }
    if ((rc = extractMesh(c, l, dValues, r.iso, w, m, r.refined))) return fail(rc);
    // behind the vertex emit, before anything reads the vertices: the mask and vbase of the extraction are still in the scratch
    if (r.refined && m->nV) {
        const unsigned char* base = static_cast<const unsigned char*>(c->scratch);
        if ((rc = refineLattice(c, r.s, l, dValues, base + w.mask, reinterpret_cast<const uint32_t*>(base + w.vbase), FT_REFINE_EDGES_MESH, r.iso, (size_t)m->nV,
                                r.refine, static_cast<float*>(m->dVertices)))) return fail(rc);
    }
    if (form == MeshForm::Scene && m->nV && (m->hasNormal || m->hasMaterial)) {
        hipError_t e = hipSuccess;
        if (m->hasNormal) e = hipMalloc(&m->dNormals, (size_t)m->nV * 12);
        if (e == hipSuccess && m->hasMaterial) e = hipMalloc(&m->dMaterials, (size_t)m->nV * 4);
        if (e != hipSuccess) return fail(hipFail(e, "hipMalloc"));
        // one points-form launch over the vertex buffer: what ft_sample_points_device gives for those points
        if ((rc = launchField(c, r.s, FieldRequest{m->dVertices, m->nV, nullptr, r.eps, 0u, nullptr, m->dNormals, m->dMaterials}))) return fail(rc);
    }
    *r.out = m;
    return FT_OK;
}

}  // namespace

int ft_mesh_lattice(ft_ctx* c, const ft_scene* s, const ft_lattice* lattice, float iso, float normal_epsilon, uint32_t flags, ft_mesh** out) {
    return buildMesh(c, MeshRequest{s, lattice, nullptr, iso, normal_epsilon, flags, out}, MeshForm::Scene);
}
int ft_mesh_lattice_refined(ft_ctx* c, const ft_scene* s, const ft_lattice* lattice, float iso, float normal_epsilon, uint32_t flags, int32_t refine_steps, ft_mesh** out) {
    return buildMesh(c, MeshRequest{s, lattice, nullptr, iso, normal_epsilon, flags, out, refine_steps, true}, MeshForm::Scene);
}
int ft_mesh_values_device(ft_ctx* c, const ft_lattice* lattice, const void* d_values, float iso, ft_mesh** out) {
    return buildMesh(c, MeshRequest{nullptr, lattice, d_values, iso, 0.0f, 0u, out}, MeshForm::DeviceValues);
}
int ft_mesh_values(ft_ctx* c, const ft_lattice* lattice, const float* values, float iso, ft_mesh** out) {
    return buildMesh(c, MeshRequest{nullptr, lattice, values, iso, 0.0f, 0u, out}, MeshForm::HostValues);
}
int ft_mesh_get_info(const ft_mesh* m, ft_mesh_info* o) {
    if (!m || !o) return setErr(FT_ERR_INVALID, "null argument");
    o->n_vertices = m->nV; o->n_triangles = m->nT; o->n_skipped = m->nSkipped;
    o->has_normal = m->hasNormal ? 1 : 0; o->has_material = m->hasMaterial ? 1 : 0;
    return FT_OK;
}
int ft_mesh_device_buffers(const ft_mesh* m, void** d_vertices, void** d_triangles, void** d_normals, void** d_materials) {
    if (!m) return setErr(FT_ERR_INVALID, "null mesh");
    if (d_vertices) *d_vertices = m->dVertices;
    if (d_triangles) *d_triangles = m->dTriangles;
    if (d_normals) *d_normals = m->dNormals;
    if (d_materials) *d_materials = m->dMaterials;
    return FT_OK;
}
int ft_mesh_read(const ft_mesh* m, ft_vec3* vertices, int32_t* triangles, ft_vec3* normals, int32_t* materials) {
    if (!m) return setErr(FT_ERR_INVALID, "null mesh");
    if ((normals && !m->hasNormal) || (materials && !m->hasMaterial)) return setErr(FT_ERR_INVALID, "mesh: built without the normals or materials asked for");
    if (!m->ctx->hasDevice) return FT_OK;                              // an empty mesh of a host-only context: nothing to copy
    int rc = requireDevice(m->ctx); if (rc) return rc;
    const struct { void* host; const void* dev; size_t bytes; } parts[4] = {
        {vertices, m->dVertices, (size_t)m->nV * 12}, {triangles, m->dTriangles, (size_t)m->nT * 12},
        {normals, m->dNormals, (size_t)m->nV * 12}, {materials, m->dMaterials, (size_t)m->nV * 4}};
    hipError_t e = hipSuccess;
    for (const auto& p : parts)
        if (e == hipSuccess && p.host && p.dev && p.bytes) e = hipMemcpyAsync(p.host, p.dev, p.bytes, hipMemcpyDefault, m->ctx->stream);      // host or device destination
    const hipError_t se = hipStreamSynchronize(m->ctx->stream);        // nothing of the call is left in flight, whatever happened
    if (e != hipSuccess) return hipFail(e, "ft_mesh_read");
    if (se != hipSuccess) return hipFail(se, "ft_mesh_read");
    return FT_OK;
}
void ft_mesh_destroy(ft_mesh* m) {
    if (!m) return;
    if (m->ctx->hasDevice && (m->dVertices || m->dTriangles || m->dNormals || m->dMaterials)) {
        (void)hipSetDevice(m->ctx->device);
        for (void* p : {m->dVertices, m->dTriangles, m->dNormals, m->dMaterials}) if (p) (void)hipFree(p);      // waits for whatever still uses it
    }
    delete m;
}
// Internal (not in the header, like ft_ctx_field_brick; tools/mesh_probe.py): the lattice points per workgroup of this context's mesher launches, one
// of 128, 256, 512, 1024.  Every tile gives the same mesh.
int ft_ctx_mesh_tile(ft_ctx* c, int32_t tile) {
    if (!c || (tile != 128 && tile != 256 && tile != 512 && tile != 1024)) return setErr(FT_ERR_INVALID, "bad argument");
    c->meshTile = (uint32_t)tile;
    return FT_OK;
}

// ---- slicing: ft_slice_lattice, ft_slice_values, ft_slice_values_device and what reads the contours (slice.hip; the rule is the header's "Slicing") ----
struct ft_slices {
    ft_ctx* ctx = nullptr;
    int64_t nP = 0, nL = 0, nClosed = 0, nSkipped = 0;
    int32_t axis = 0, nSlices = 0;
    bool hasNormal = false, hasMaterial = false;
    void* dPoints = nullptr; void* dPolylines = nullptr; void* dNormals = nullptr; void* dMaterials = nullptr;
};

namespace {

// refine: the bisection rounds of ft_slice_lattice_refined, -1 for the unrefined forms
struct SliceRequest { const ft_scene* s; const ft_lattice* lat; const void* values; int32_t axis; float iso, eps; uint32_t flags; ft_slices** out; int32_t refine = -1; bool refined = false; };

// Everything that can be refused without a device, in the header's order (the mesher's, with the axis between the counts and the flag bits).  *nothing: a
// count of 1 in the plane, FT_OK with an empty result and nothing to launch.
int checkSlice(const ft_ctx* c, const SliceRequest& r, MeshForm form, bool* nothing) {
    static_assert(sizeof(ft_polyline) == 16 && sizeof(ft_slices_info) == 48, "layout");
    *nothing = false;
    if (r.out) *r.out = nullptr;
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (form == MeshForm::Scene && (!r.s || r.s->ctx != c)) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    if (!r.lat) return setErr(FT_ERR_INVALID, "null lattice");
    if (form != MeshForm::Scene && !r.values) return setErr(FT_ERR_INVALID, "slice: null values");
    if (!r.out) return setErr(FT_ERR_INVALID, "null out pointer");
    const int32_t cnt[3] = {r.lat->nx, r.lat->ny, r.lat->nz};
    for (int32_t v : cnt) if (v < 1 || v > 16777216) return setErr(FT_ERR_INVALID, "lattice: every count must be 1 .. 16777216");
    if (r.axis < 0 || r.axis > 2) return setErr(FT_ERR_INVALID, "slice: the axis must be 0, 1 or 2");
    if (r.flags & ~(uint32_t)(FT_SLICE_NORMAL | FT_SLICE_MATERIAL)) return setErr(FT_ERR_INVALID, "slice: unknown flag bits");
    if (r.refined && (r.refine < 0 || r.refine > FT_REFINE_MAX_STEPS)) return setErr(FT_ERR_INVALID, "slice: refine_steps must be 0 .. 32");
    if (form == MeshForm::DeviceValues && (reinterpret_cast<uintptr_t>(r.values) & 3u)) return setErr(FT_ERR_INVALID, "slice: the device values must be 4-byte aligned");
    // three counts of at most 2^24: the product of two fits 2^48, and the third is applied only below the limit
    const uint64_t two = (uint64_t)r.lat->nx * (uint64_t)r.lat->ny;
    if (two >= 0xFFFF0000ull || two * (uint64_t)r.lat->nz >= 0xFFFF0000ull) return setErr(FT_ERR_UNSUPPORTED, "more than 2^32 points in one call");
    *nothing = cnt[(r.axis + 1) % 3] == 1 || cnt[(r.axis + 2) % 3] == 1;
    return FT_OK;
}

// the lattice passes' work behind `at` bytes of the context's scratch: 5 B per point and 12 B per tile, as the mesher's
struct SliceWork { size_t mask, vbase, tileA, tileB, tileC, totals, end; };
SliceWork sliceWork(size_t at, size_t n, size_t nTiles) {
    SliceWork w{};
    w.mask = align256(at); w.vbase = align256(w.mask + n); w.tileA = align256(w.vbase + 4 * n); w.tileB = align256(w.tileA + 4 * nTiles);
    w.tileC = align256(w.tileB + 4 * nTiles); w.totals = align256(w.tileC + 4 * nTiles); w.end = w.totals + 256;
    return w;
}

const char* const kSliceKernels[FT_SLICE_KERNELS] = {"slice count", "slice scan", "slice emit", "slice link", "slice lead", "slice jump", "slice cut", "slice tail",
                                                     "slice heads", "slice vertex scan", "slice records", "slice scatter"};
// the workgroups of one launch: `items` tiles, or vertices in the untiled kernels
int sliceBlocks(ft_ctx* c, int kernel, const FtSliceArgs& a, uint64_t items, unsigned* blocks) {
    int perCU = 0;
    const hipError_t e = ft_slice_occupancy(kernel, a.tile, &perCU);
    if (e != hipSuccess) return hipFail(e, (std::string("occupancy of the ") + kSliceKernels[kernel] + " kernel").c_str());
    int rc = clampPerCU(c, kSliceKernels[kernel], perCU); if (rc) return rc;
    const unsigned flat = ft_slice_block(kernel, 0u);                  // 0 for the tiled kernels: their workgroup is the tile
    const uint64_t want = flat ? (items + flat - 1) / flat : items;
    *blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->numCUs * perCU, want));
    return FT_OK;
}
int launchSlice(ft_ctx* c, int kernel, const FtSliceArgs& a, uint64_t items) {
    unsigned blocks = 1;
    int rc = sliceBlocks(c, kernel, a, items, &blocks); if (rc) return rc;
    return timedLaunch(c, c->stream, "ft_launch_slice", [&] { return ft_launch_slice(kernel, &a, blocks, c->stream); });
}
// `first` (lead or cut) and the jump rounds behind it, under one event pair; a's from / to end up swapped where the rounds are odd
int launchSliceRounds(ft_ctx* c, int first, FtSliceArgs& a, unsigned rounds) {
    unsigned b0 = 1, b1 = 1;
    int rc;
    if ((rc = sliceBlocks(c, first, a, a.nV, &b0)) || (rc = sliceBlocks(c, FT_SLICE_K_JUMP, a, a.nV, &b1))) return rc;
    rc = timedLaunch(c, c->stream, "ft_launch_slice_jumps", [&] {
        const hipError_t e = ft_launch_slice(first, &a, b0, c->stream);
        return e != hipSuccess ? e : ft_launch_slice_jumps(&a, rounds, b1, c->stream);
    });
    if (rc == FT_OK && (rounds & 1u)) std::swap(a.from, a.to);
    return rc;
}

// The extraction: values (device memory, n floats) -> m's points and polylines.  Synchronises the context's stream twice: for the vertex and segment
// totals (the per-vertex work is sized from them) and for the point and polyline totals (the outputs are).
// refineScene: NULL, or the scene whose field refines the vertices (refineSteps rounds) between the emit and the scatter.
int extractSlices(ft_ctx* c, const ft_lattice& l, const float* dValues, int32_t axis, float iso, const SliceWork& w, ft_slices* m, const ft_scene* refineScene,
                  int32_t refineSteps) {
    FtSliceArgs a{};
    a.values = dValues; a.iso = iso; a.axis = (uint32_t)axis;
    a.nx = (uint32_t)l.nx; a.ny = (uint32_t)l.ny; a.nz = (uint32_t)l.nz;
    a.n = a.nx * a.ny * a.nz;                                          // below 0xFFFF0000 (checkSlice)
    a.tile = c->sliceTile;
    a.nTiles = (uint32_t)(((uint64_t)a.n + a.tile - 1u) / a.tile);
    a.origin[0] = l.origin.x; a.origin[1] = l.origin.y; a.origin[2] = l.origin.z;
    a.step[0] = l.step.x; a.step[1] = l.step.y; a.step[2] = l.step.z;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    a.mask = base + w.mask; a.vbase = reinterpret_cast<uint32_t*>(base + w.vbase);
    a.tileA = reinterpret_cast<uint32_t*>(base + w.tileA); a.tileB = reinterpret_cast<uint32_t*>(base + w.tileB); a.tileC = reinterpret_cast<uint32_t*>(base + w.tileC);
    a.totals = reinterpret_cast<unsigned long long*>(base + w.totals);
    int rc;
    if ((rc = launchSlice(c, FT_SLICE_K_COUNT, a, a.nTiles)) || (rc = launchSlice(c, FT_SLICE_K_SCAN, a, 1))) return rc;
    unsigned long long totals[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                          // the first synchronisation: vertices, segments, skipped triangles
    m->nSkipped = (int64_t)totals[2];
    if (totals[0] >= (1ull << 31)) return setErr(FT_ERR_UNSUPPORTED, "slice: 2^31 or more points or polylines (the index type is int32)");
    if (!totals[0] || !totals[1]) return FT_OK;                        // no segment: no polyline
    const size_t nV = (size_t)totals[0], nVT = (nV + a.tile - 1) / a.tile;
    a.nV = (uint32_t)nV; a.nVTiles = (uint32_t)nVT;
    // the per-vertex work: 12 + 11 * 4 + 1 B per vertex, 12 B per tile of vertices
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    const size_t oPos = take(nV * 12), oSlice = take(nV * 4), oNext = take(nV * 4), oPrev = take(nV * 4), oLen = take(nV * 4), oOff = take(nV * 4);
    size_t oState[6];
    for (size_t& o : oState) o = take(nV * 4);
    const size_t oCyc = take(nV), oA = take(nVT * 4), oB = take(nVT * 4), oC = take(nVT * 4), oTotals = take(256);
    if ((rc = ensureBytes(c->sliceWork, c->sliceWorkBytes, at))) return rc;
    if (refineScene && (rc = ensureBytes(c->refineWork, c->refineWorkBytes, refineWork(nV, false).end))) return rc;
    unsigned char* wk = static_cast<unsigned char*>(c->sliceWork);
    auto words = [&](size_t o) { return reinterpret_cast<uint32_t*>(wk + o); };
    a.vpos = reinterpret_cast<float*>(wk + oPos); a.vslice = words(oSlice); a.next = words(oNext); a.prev = words(oPrev); a.len = words(oLen); a.off = words(oOff);
    a.from = FtSliceState{words(oState[0]), words(oState[1]), words(oState[2])};
    a.to = FtSliceState{words(oState[3]), words(oState[4]), words(oState[5])};
    a.cyc = wk + oCyc; a.vtA = words(oA); a.vtB = words(oB); a.vtC = words(oC);
    a.vtotals = reinterpret_cast<unsigned long long*>(wk + oTotals);
    HIP_TRY(hipMemsetAsync(a.next, 0xff, oLen - oNext, c->stream));     // next and prev, adjacent: FT_SLICE_NONE
    HIP_TRY(hipMemsetAsync(a.len, 0, nV * 4, c->stream));
    if ((rc = launchSlice(c, FT_SLICE_K_EMIT, a, a.nTiles)) || (rc = launchSlice(c, FT_SLICE_K_LINK, a, a.nTiles))) return rc;
    if (refineScene) {                                                 // behind the emit, long before the scatter reads vpos; the chaining never reads positions
        static const uint32_t edges[3] = FT_REFINE_EDGES_SLICE;
        if ((rc = refineLattice(c, refineScene, l, dValues, a.mask, a.vbase, edges[axis], iso, nV, refineSteps, a.vpos))) return rc;
    }
    unsigned rounds = 0;
    while (((uint64_t)1 << rounds) < (uint64_t)nV) ++rounds;          // 2^rounds >= the vertex total: a window of that many hops covers any cycle
    c->sliceLast[0] = (int64_t)nV; c->sliceLast[1] = (int64_t)rounds;
    if (c->sliceStop == 1) return FT_OK;
    if ((rc = launchSliceRounds(c, FT_SLICE_K_LEAD, a, rounds)) || (rc = launchSliceRounds(c, FT_SLICE_K_CUT, a, rounds))) return rc;
    if (c->sliceStop == 2) return FT_OK;
    if ((rc = launchSlice(c, FT_SLICE_K_TAIL, a, nV)) || (rc = launchSlice(c, FT_SLICE_K_HEADS, a, nVT)) || (rc = launchSlice(c, FT_SLICE_K_VSCAN, a, 1))) return rc;
    HIP_TRY(hipMemcpyAsync(totals, a.vtotals, sizeof totals, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                          // the second synchronisation: polylines, points, closed polylines
    if (totals[0] >= (1ull << 31) || totals[1] >= (1ull << 31)) return setErr(FT_ERR_UNSUPPORTED, "slice: 2^31 or more points or polylines (the index type is int32)");
    m->nL = (int64_t)totals[0]; m->nP = (int64_t)totals[1]; m->nClosed = (int64_t)totals[2];
    if (!m->nL) return FT_OK;
    HIP_TRY(hipMalloc(&m->dPoints, (size_t)m->nP * 12));
    HIP_TRY(hipMalloc(&m->dPolylines, (size_t)m->nL * sizeof(ft_polyline)));
    a.points = static_cast<float*>(m->dPoints); a.polylines = static_cast<int32_t*>(m->dPolylines);
    a.nP = (uint32_t)m->nP; a.nL = (uint32_t)m->nL;
    if ((rc = launchSlice(c, FT_SLICE_K_RECORDS, a, nVT)) || (rc = launchSlice(c, FT_SLICE_K_SCATTER, a, nV))) return rc;
    return FT_OK;
}

int buildSlices(ft_ctx* c, const SliceRequest& r, MeshForm form) {
    bool nothing;
    int rc = checkSlice(c, r, form, &nothing); if (rc) return rc;
    ft_slices* m = new ft_slices();
    m->ctx = c;
    m->axis = r.axis;
    m->nSlices = r.axis == 0 ? r.lat->nx : (r.axis == 1 ? r.lat->ny : r.lat->nz);
    m->hasNormal = (r.flags & FT_SLICE_NORMAL) != 0u; m->hasMaterial = (r.flags & FT_SLICE_MATERIAL) != 0u;
    if (nothing) { *r.out = m; return FT_OK; }
    auto fail = [&](int code) { if (c->hasDevice) (void)hipStreamSynchronize(c->stream); ft_slices_destroy(m); return code; };
    if ((rc = requireDevice(c))) return fail(rc);
    const ft_lattice& l = *r.lat;
    const size_t n = (size_t)l.nx * l.ny * l.nz, tile = c->sliceTile, nTiles = (n + tile - 1) / tile;
    const SliceWork w = sliceWork(form == MeshForm::DeviceValues ? 0 : n * 4, n, nTiles);
    if ((rc = ensureScratch(c, w.end))) return fail(rc);
    const float* dValues = form == MeshForm::DeviceValues ? static_cast<const float*>(r.values) : static_cast<const float*>(c->scratch);
    if (form == MeshForm::HostValues) {
        const hipError_t e = hipMemcpyAsync(c->scratch, r.values, n * 4, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(hipFail(e, "slice: upload"));
    } else if (form == MeshForm::Scene) {
        if ((rc = launchField(c, r.s, FieldRequest{nullptr, 0, r.lat, 0.0f, 0u, c->scratch, nullptr, nullptr}))) return fail(rc);
    }
    if ((rc = extractSlices(c, l, dValues, r.axis, r.iso, w, m, r.refined ? r.s : nullptr, r.refine))) return fail(rc);
    if (form == MeshForm::Scene && m->nP && (m->hasNormal || m->hasMaterial)) {
        hipError_t e = hipSuccess;
        if (m->hasNormal) e = hipMalloc(&m->dNormals, (size_t)m->nP * 12);
        if (e == hipSuccess && m->hasMaterial) e = hipMalloc(&m->dMaterials, (size_t)m->nP * 4);
        if (e != hipSuccess) return fail(hipFail(e, "hipMalloc"));
        // one points-form launch over the finished point buffer: what ft_sample_points_device gives for those points
        if ((rc = launchField(c, r.s, FieldRequest{m->dPoints, m->nP, nullptr, r.eps, 0u, nullptr, m->dNormals, m->dMaterials}))) return fail(rc);
    }
    *r.out = m;
    return FT_OK;
}

}  // namespace

int ft_slice_lattice(ft_ctx* c, const ft_scene* s, const ft_lattice* lattice, int32_t axis, float iso, float normal_epsilon, uint32_t flags, ft_slices** out) {
    return buildSlices(c, SliceRequest{s, lattice, nullptr, axis, iso, normal_epsilon, flags, out}, MeshForm::Scene);
}
int ft_slice_lattice_refined(ft_ctx* c, const ft_scene* s, const ft_lattice* lattice, int32_t axis, float iso, float normal_epsilon, uint32_t flags, int32_t refine_steps,
                             ft_slices** out) {
    return buildSlices(c, SliceRequest{s, lattice, nullptr, axis, iso, normal_epsilon, flags, out, refine_steps, true}, MeshForm::Scene);
}
int ft_slice_values_device(ft_ctx* c, const ft_lattice* lattice, const void* d_values, int32_t axis, float iso, ft_slices** out) {
    return buildSlices(c, SliceRequest{nullptr, lattice, d_values, axis, iso, 0.0f, 0u, out}, MeshForm::DeviceValues);
}
int ft_slice_values(ft_ctx* c, const ft_lattice* lattice, const float* values, int32_t axis, float iso, ft_slices** out) {
    return buildSlices(c, SliceRequest{nullptr, lattice, values, axis, iso, 0.0f, 0u, out}, MeshForm::HostValues);
}
int ft_slices_get_info(const ft_slices* m, ft_slices_info* o) {
    if (!m || !o) return setErr(FT_ERR_INVALID, "null argument");
    o->n_points = m->nP; o->n_polylines = m->nL; o->n_closed = m->nClosed; o->n_skipped = m->nSkipped;
    o->axis = m->axis; o->n_slices = m->nSlices;
    o->has_normal = m->hasNormal ? 1 : 0; o->has_material = m->hasMaterial ? 1 : 0;
    return FT_OK;
}
int ft_slices_device_buffers(const ft_slices* m, void** d_points, void** d_polylines, void** d_normals, void** d_materials) {
    if (!m) return setErr(FT_ERR_INVALID, "null slices");
    if (d_points) *d_points = m->dPoints;
    if (d_polylines) *d_polylines = m->dPolylines;
    if (d_normals) *d_normals = m->dNormals;
    if (d_materials) *d_materials = m->dMaterials;
    return FT_OK;
}
int ft_slices_read(const ft_slices* m, ft_vec3* points, ft_polyline* polylines, ft_vec3* normals, int32_t* materials) {
    if (!m) return setErr(FT_ERR_INVALID, "null slices");
    if ((normals && !m->hasNormal) || (materials && !m->hasMaterial)) return setErr(FT_ERR_INVALID, "slice: built without the normals or materials asked for");
    if (!m->ctx->hasDevice) return FT_OK;                              // an empty result of a host-only context: nothing to copy
    int rc = requireDevice(m->ctx); if (rc) return rc;
    const struct { void* host; const void* dev; size_t bytes; } parts[4] = {
        {points, m->dPoints, (size_t)m->nP * 12}, {polylines, m->dPolylines, (size_t)m->nL * sizeof(ft_polyline)},
        {normals, m->dNormals, (size_t)m->nP * 12}, {materials, m->dMaterials, (size_t)m->nP * 4}};
    hipError_t e = hipSuccess;
    for (const auto& p : parts)
        if (e == hipSuccess && p.host && p.dev && p.bytes) e = hipMemcpyAsync(p.host, p.dev, p.bytes, hipMemcpyDefault, m->ctx->stream);      // host or device destination
    const hipError_t se = hipStreamSynchronize(m->ctx->stream);        // nothing of the call is left in flight, whatever happened
    if (e != hipSuccess) return hipFail(e, "ft_slices_read");
    if (se != hipSuccess) return hipFail(se, "ft_slices_read");
    return FT_OK;
}
void ft_slices_destroy(ft_slices* m) {
    if (!m) return;
    if (m->ctx->hasDevice && (m->dPoints || m->dPolylines || m->dNormals || m->dMaterials)) {
        (void)hipSetDevice(m->ctx->device);
        for (void* p : {m->dPoints, m->dPolylines, m->dNormals, m->dMaterials}) if (p) (void)hipFree(p);      // waits for whatever still uses it
    }
    delete m;
}
// Internal (not in the header, like ft_ctx_mesh_tile; tools/slice_probe.py and the tests): the items per workgroup of this context's slicer launches, one
// of 128, 256, 512, 1024.  Every tile gives the same contours.
int ft_ctx_slice_tile(ft_ctx* c, int32_t tile) {
    if (!c || (tile != 128 && tile != 256 && tile != 512 && tile != 1024)) return setErr(FT_ERR_INVALID, "bad argument");
    c->sliceTile = (uint32_t)tile;
    return FT_OK;
}
// Internal (tools/slice_probe.py): stop = 0 whole extractions, 1 / 2 this context's extractions end after the link kernel / after the jump rounds and
// give an empty result, so that a stage's kernel time is a difference of two figures; last (may be NULL): the vertices and the jump rounds R of the
// context's last extraction.
int ft_ctx_slice_probe(ft_ctx* c, int32_t stop, int64_t* last) {
    if (!c || stop < 0 || stop > 2) return setErr(FT_ERR_INVALID, "bad argument");
    c->sliceStop = stop;
    if (last) { last[0] = c->sliceLast[0]; last[1] = c->sliceLast[1]; }
    return FT_OK;
}

// ---- shells: ft_mesh_shells, ft_shells_triangles, ft_shells_triangles_device, what reads them, and ft_mesh_select (shells.hip; the rule is the header's "Shells") ----
struct ft_shells {
    ft_ctx* ctx = nullptr;
    int64_t nV = 0, nT = 0, nS = 0, nClosed = 0, nUnused = 0, nBorder = 0;
    uint64_t meshSerial = 0;                               // ft_mesh::serial of the mesh they were built from; 0: from a triangle list
    void* dVertexShell = nullptr; void* dTriangleShell = nullptr; void* dRecords = nullptr;
};

namespace {

enum class ShellsForm { Mesh, HostTriangles, DeviceTriangles };
constexpr int64_t FT_SHELLS_MAX_TRIANGLES = 715827883;     // 3 * nT no longer fits int32 from here on

// Everything that can be refused without a device, in the header's order.  *nothing: no triangle, FT_OK with every vertex unused and nothing to launch.
int checkShells(const ft_ctx* c, ShellsForm form, const void* triangles, int64_t nT, int64_t nV, ft_shells** out, bool* nothing) {
    static_assert(sizeof(ft_shell) == 16 && sizeof(ft_shells_info) == 48, "layout");
    *nothing = false;
    if (out) *out = nullptr;
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (!triangles && nT != 0) return setErr(FT_ERR_INVALID, "shells: null triangles");
    if (!out) return setErr(FT_ERR_INVALID, "null out pointer");
    if (nT < 0 || nV < 0 || nV >= ((int64_t)1 << 31)) return setErr(FT_ERR_INVALID, "shells: the counts must be >= 0 and n_vertices below 2^31");
    if (form == ShellsForm::DeviceTriangles && (reinterpret_cast<uintptr_t>(triangles) & 3u)) return setErr(FT_ERR_INVALID, "shells: the device triangles must be 4-byte aligned");
    if (nT >= FT_SHELLS_MAX_TRIANGLES) return setErr(FT_ERR_UNSUPPORTED, "shells: 715827883 or more triangles (3 * n_triangles must fit int32)");
    if (nT > 0 && nV == 0) return setErr(FT_ERR_INVALID, "shells: triangles without vertices");
    if (form == ShellsForm::HostTriangles) {
        const int32_t* t = static_cast<const int32_t*>(triangles);
        for (int64_t i = 0; i < nT; ++i, t += 3) {
            const bool ok = t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[0] < nV && t[1] < nV && t[2] < nV && t[0] != t[1] && t[1] != t[2] && t[0] != t[2];
            if (!ok) return setErr(FT_ERR_INVALID, "shells: triangle " + std::to_string(i) + " has an index outside 0 .. n_vertices - 1, or one twice");
        }
    }
    *nothing = nT == 0;
    return FT_OK;
}

const char* const kShellsKernels[FT_SHELLS_KERNELS] = {
    "shells init", "shells degree", "shells degree sums", "shells scan", "shells offsets", "shells fill", "shells shortcut", "shells hook", "shells apply",
    "shells stagnant hook", "shells second shortcut", "shells verify", "shells first", "shells leader sums", "shells number", "shells label vertices",
    "shells label triangles", "shells summary", "shells keep vertex sums", "shells keep triangle sums", "shells keep vertices", "shells keep triangles"};

// the workgroups of one launch, by the kernel's domain: vertices, triangles or shells; tiles of them in the tiled kernels
int shellsBlocks(ft_ctx* c, int kernel, const FtShellsArgs& a, unsigned* blocks) {
    int perCU = 0;
    const hipError_t e = ft_shells_occupancy(kernel, a.tile, &perCU);
    if (e != hipSuccess) return hipFail(e, (std::string("occupancy of the ") + kShellsKernels[kernel] + " kernel").c_str());
    int rc = clampPerCU(c, kShellsKernels[kernel], perCU); if (rc) return rc;
    const int domain = ft_shells_domain(kernel);
    const uint64_t items = domain == 0 ? a.nV : (domain == 1 ? a.nT : (domain == 2 ? a.nS : 1));
    const unsigned per = ft_shells_block(kernel, a.tile);
    *blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->numCUs * perCU, (items + per - 1) / per));
    return FT_OK;
}
int launchShells(ft_ctx* c, int kernel, const FtShellsArgs& a) {
    unsigned blocks = 1;
    int rc = shellsBlocks(c, kernel, a, &blocks); if (rc) return rc;
    return timedLaunch(c, c->stream, "ft_launch_shells", [&] { return ft_launch_shells(kernel, &a, blocks, c->stream); });
}

// The labelling of nT > 0 triangles over nV > 0 vertices in device memory -> s's labels, records and totals.  Synchronises the context's stream once
// per batch of FT_SHELLS_BATCH iterations (the 4-byte stop flag) and once for the totals.
int labelShells(ft_ctx* c, const int32_t* dTriangles, ft_shells* s) {
    const size_t nV = (size_t)s->nV, nT = (size_t)s->nT, tile = c->shellsTile;
    const size_t nVT = (nV + tile - 1) / tile, nTT = (nT + tile - 1) / tile, room = nV / 3 + 1;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    size_t oWord[8];
    for (size_t& o : oWord) o = take(nV * 4);
    const size_t oInc = take(nT * 12), oA = take(std::max(nVT, nTT) * 4), oC = take(std::max(nVT, nTT) * 4), oRec = take(room * sizeof(ft_shell)), oTotals = take(256),
                 oFlags = take(768);
    int rc;
    if ((rc = ensureBytes(c->shellsWork, c->shellsWorkBytes, at))) return rc;
    HIP_TRY(hipMalloc(&s->dVertexShell, nV * 4));
    HIP_TRY(hipMalloc(&s->dTriangleShell, nT * 4));
    unsigned char* wk = static_cast<unsigned char*>(c->shellsWork);
    auto words = [&](size_t o) { return reinterpret_cast<uint32_t*>(wk + o); };
    FtShellsArgs a{};
    a.triangles = dTriangles;
    a.nV = (uint32_t)nV; a.nT = (uint32_t)nT; a.tile = (uint32_t)tile; a.nVTiles = (uint32_t)nVT; a.nTTiles = (uint32_t)nTT; a.scanTiles = a.nVTiles;
    a.parent = words(oWord[0]); a.parent2 = words(oWord[1]); a.stamp = words(oWord[2]); a.hook = words(oWord[3]); a.first = words(oWord[4]);
    a.degree = words(oWord[5]); a.offset = words(oWord[6]); a.cursor = words(oWord[7]);
    a.incidence = words(oInc); a.tileA = words(oA); a.tileC = words(oC);
    a.totals = reinterpret_cast<unsigned long long*>(wk + oTotals); a.flags = words(oFlags);
    a.nS = (uint32_t)room; a.records = reinterpret_cast<int32_t*>(wk + oRec);
    a.vertexShell = static_cast<int32_t*>(s->dVertexShell); a.triangleShell = static_cast<int32_t*>(s->dTriangleShell);
    HIP_TRY(hipMemsetAsync(wk + oTotals, 0, 256 + 768, c->stream));     // totals and flags, adjacent
    for (int k : {FT_SHELLS_K_INIT, FT_SHELLS_K_DEGREE, FT_SHELLS_K_DEGREE_SUMS, FT_SHELLS_K_SCAN, FT_SHELLS_K_OFFSETS, FT_SHELLS_K_FILL})
        if ((rc = launchShells(c, k, a))) return rc;
    if (c->shellsStop == 1) return FT_OK;
    unsigned blocksV = 1, blocksT = 1;
    if ((rc = shellsBlocks(c, FT_SHELLS_K_SHORTCUT, a, &blocksV)) || (rc = shellsBlocks(c, FT_SHELLS_K_HOOK, a, &blocksT))) return rc;
    for (int k : {FT_SHELLS_K_APPLY, FT_SHELLS_K_STAGNANT, FT_SHELLS_K_SHORTCUT2, FT_SHELLS_K_VERIFY}) {      // a failed query names its kernel
        unsigned unused = 1;
        if ((rc = shellsBlocks(c, k, a, &unused))) return rc;
    }
    const unsigned cap = ft_shells_iteration_cap(nV);
    unsigned done = 0, batch = 0;
    c->shellsLast[0] = c->shellsLast[1] = 0;
    for (bool open = true; open; ++batch) {
        if (done >= cap)
            return setErr(FT_ERR_UNSUPPORTED, "shells: the labelling has not finished after its proven bound of " + std::to_string(cap) + " iterations (internal error)");
        const unsigned count = std::min<unsigned>(FT_SHELLS_BATCH, cap - done);
        a.iteration = done + 1u; a.flagWord = batch;
        if ((rc = timedLaunch(c, c->stream, "ft_launch_shells_iterations", [&] { return ft_launch_shells_iterations(&a, count, blocksV, blocksT, c->stream); }))) return rc;
        done += count;
        uint32_t flag = 0;
        HIP_TRY(hipMemcpyAsync(&flag, a.flags + batch, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                      // one 4-byte flag per batch
        c->shellsLast[0] = (int64_t)done; c->shellsLast[1] += 1;
        if (batch == 0 && (flag & FT_SHELLS_FLAG_INVALID))             // the first pass' verdict (flag word 0), at the first synchronisation
            return setErr(FT_ERR_INVALID, "shells: a triangle has an index outside 0 .. n_vertices - 1, or one twice");
        open = (flag & FT_SHELLS_FLAG_OPEN) != 0u;
    }
    if (c->shellsStop == 2) return FT_OK;
    for (int k : {FT_SHELLS_K_FIRST, FT_SHELLS_K_LEADER_SUMS, FT_SHELLS_K_SCAN, FT_SHELLS_K_NUMBER, FT_SHELLS_K_LABEL_VERTICES, FT_SHELLS_K_LABEL_TRIANGLES,
                  FT_SHELLS_K_SUMMARY}) {
        if (c->shellsStop == 3 && k == FT_SHELLS_K_LABEL_TRIANGLES) return FT_OK;
        if ((rc = launchShells(c, k, a))) return rc;
    }
    unsigned long long totals[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                          // the one for the totals: shells, used vertices, closed shells, border edges
    c->shellsLast[1] += 1;
    if (totals[0] > room || totals[1] > nV) return setErr(FT_ERR_HIP, "shells: impossible totals (internal error)");
    s->nS = (int64_t)totals[0]; s->nUnused = (int64_t)(nV - totals[1]); s->nClosed = (int64_t)totals[2]; s->nBorder = (int64_t)totals[3];
    if (s->nS) {
        HIP_TRY(hipMalloc(&s->dRecords, (size_t)s->nS * sizeof(ft_shell)));
        HIP_TRY(hipMemcpyAsync(s->dRecords, a.records, (size_t)s->nS * sizeof(ft_shell), hipMemcpyDeviceToDevice, c->stream));
    }
    return FT_OK;
}

int buildShells(ft_ctx* c, ShellsForm form, const void* triangles, int64_t nT, int64_t nV, uint64_t meshSerial, ft_shells** out) {
    bool nothing;
    int rc = checkShells(c, form, triangles, nT, nV, out, &nothing); if (rc) return rc;
    ft_shells* s = new ft_shells();
    s->ctx = c; s->nV = nV; s->nT = nT; s->meshSerial = meshSerial;
    auto fail = [&](int code) { if (c->hasDevice) (void)hipStreamSynchronize(c->stream); ft_shells_destroy(s); return code; };
    if (nothing) {                                                     // every vertex unused; on a host-only context ft_shells_read writes the -1 itself
        s->nUnused = nV;
        if (c->hasDevice && nV) {
            if ((rc = requireDevice(c))) return fail(rc);
            hipError_t e = hipMalloc(&s->dVertexShell, (size_t)nV * 4);
            if (e == hipSuccess) e = hipMemsetAsync(s->dVertexShell, 0xff, (size_t)nV * 4, c->stream);
            if (e != hipSuccess) return fail(hipFail(e, "shells: empty labels"));
        }
        *out = s;
        return FT_OK;
    }
    if ((rc = requireDevice(c))) return fail(rc);
    const int32_t* dTriangles = static_cast<const int32_t*>(triangles);
    if (form == ShellsForm::HostTriangles) {                           // staged through the context's scratch
        if ((rc = ensureScratch(c, (size_t)nT * 12))) return fail(rc);
        const hipError_t e = hipMemcpyAsync(c->scratch, triangles, (size_t)nT * 12, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(hipFail(e, "shells: upload"));
        dTriangles = static_cast<const int32_t*>(c->scratch);
    }
    if ((rc = labelShells(c, dTriangles, s))) return fail(rc);
    *out = s;
    return FT_OK;
}

}  // namespace

int ft_mesh_shells(const ft_mesh* m, ft_shells** out) {
    if (out) *out = nullptr;
    if (!m) return setErr(FT_ERR_INVALID, "null mesh");
    return buildShells(m->ctx, ShellsForm::Mesh, m->dTriangles, m->nT, m->nV, m->serial, out);
}
int ft_shells_triangles(ft_ctx* c, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, ft_shells** out) {
    return buildShells(c, ShellsForm::HostTriangles, triangles, n_triangles, n_vertices, 0, out);
}
int ft_shells_triangles_device(ft_ctx* c, const void* d_triangles, int64_t n_triangles, int64_t n_vertices, ft_shells** out) {
    return buildShells(c, ShellsForm::DeviceTriangles, d_triangles, n_triangles, n_vertices, 0, out);
}
int ft_shells_get_info(const ft_shells* s, ft_shells_info* o) {
    if (!s || !o) return setErr(FT_ERR_INVALID, "null argument");
    o->n_vertices = s->nV; o->n_triangles = s->nT; o->n_shells = s->nS; o->n_closed = s->nClosed; o->n_unused_vertices = s->nUnused; o->n_border_edges = s->nBorder;
    return FT_OK;
}
int ft_shells_device_buffers(const ft_shells* s, void** d_vertex_shell, void** d_triangle_shell, void** d_records) {
    if (!s) return setErr(FT_ERR_INVALID, "null shells");
    if (d_vertex_shell) *d_vertex_shell = s->dVertexShell;
    if (d_triangle_shell) *d_triangle_shell = s->dTriangleShell;
    if (d_records) *d_records = s->dRecords;
    return FT_OK;
}
int ft_shells_read(const ft_shells* s, int32_t* vertex_shell, int32_t* triangle_shell, ft_shell* records) {
    if (!s) return setErr(FT_ERR_INVALID, "null shells");
    if (!s->ctx->hasDevice) {                                          // empty shells of a host-only context: every vertex is unused
        if (vertex_shell && s->nV) std::memset(vertex_shell, 0xff, (size_t)s->nV * 4);
        return FT_OK;
    }
    int rc = requireDevice(s->ctx); if (rc) return rc;
    const struct { void* host; const void* dev; size_t bytes; } parts[3] = {
        {vertex_shell, s->dVertexShell, (size_t)s->nV * 4}, {triangle_shell, s->dTriangleShell, (size_t)s->nT * 4}, {records, s->dRecords, (size_t)s->nS * sizeof(ft_shell)}};
    hipError_t e = hipSuccess;
    for (const auto& p : parts)
        if (e == hipSuccess && p.host && p.dev && p.bytes) e = hipMemcpyAsync(p.host, p.dev, p.bytes, hipMemcpyDefault, s->ctx->stream);      // host or device destination
    const hipError_t se = hipStreamSynchronize(s->ctx->stream);        // nothing of the call is left in flight, whatever happened
    if (e != hipSuccess) return hipFail(e, "ft_shells_read");
    if (se != hipSuccess) return hipFail(se, "ft_shells_read");
    return FT_OK;
}
void ft_shells_destroy(ft_shells* s) {
    if (!s) return;
    if (s->ctx->hasDevice && (s->dVertexShell || s->dTriangleShell || s->dRecords)) {
        (void)hipSetDevice(s->ctx->device);
        for (void* p : {s->dVertexShell, s->dTriangleShell, s->dRecords}) if (p) (void)hipFree(p);      // waits for whatever still uses it
    }
    delete s;
}

// The selection.  Synchronises the context's stream once, for the kept vertices and triangles; then allocates exactly and scatters.
int ft_mesh_select(const ft_mesh* m, const ft_shells* s, const uint8_t* keep, int64_t n_keep, ft_mesh** out) {
    if (out) *out = nullptr;
    if (!m) return setErr(FT_ERR_INVALID, "null mesh");
    if (!s) return setErr(FT_ERR_INVALID, "null shells");
    if (!keep && n_keep != 0) return setErr(FT_ERR_INVALID, "select: null keep");
    if (!out) return setErr(FT_ERR_INVALID, "null out pointer");
    if (s->ctx != m->ctx || s->meshSerial != m->serial) return setErr(FT_ERR_INVALID, "select: the shells were not built from this mesh");
    if (n_keep != s->nS) return setErr(FT_ERR_INVALID, "select: n_keep must be the number of shells");
    ft_ctx* c = m->ctx;
    ft_mesh* r = newMesh(c);
    r->hasNormal = m->hasNormal; r->hasMaterial = m->hasMaterial; r->nSkipped = m->nSkipped;
    bool any = false;
    for (int64_t i = 0; i < n_keep; ++i) any = any || keep[i] != 0;
    if (!any) { *out = r; return FT_OK; }                              // no shell kept (or none there): an empty mesh, no device needed
    auto fail = [&](int code) { if (c->hasDevice) (void)hipStreamSynchronize(c->stream); ft_mesh_destroy(r); return code; };
    int rc;
    if ((rc = requireDevice(c))) return fail(rc);
    const size_t nV = (size_t)m->nV, nT = (size_t)m->nT, nS = (size_t)s->nS, tile = c->shellsTile;
    const size_t nVT = (nV + tile - 1) / tile, nTT = (nT + tile - 1) / tile;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    const size_t oRemap = take(nV * 4), oAV = take(nVT * 4), oAT = take(nTT * 4), oC = take(std::max(nVT, nTT) * 4), oKeep = take(nS), oTotals = take(256);
    if ((rc = ensureBytes(c->shellsWork, c->shellsWorkBytes, at))) return fail(rc);
    unsigned char* wk = static_cast<unsigned char*>(c->shellsWork);
    auto words = [&](size_t o) { return reinterpret_cast<uint32_t*>(wk + o); };
    FtShellsArgs av{};
    av.triangles = static_cast<const int32_t*>(m->dTriangles);
    av.nV = (uint32_t)nV; av.nT = (uint32_t)nT; av.tile = (uint32_t)tile; av.nVTiles = (uint32_t)nVT; av.nTTiles = (uint32_t)nTT; av.nS = (uint32_t)nS;
    av.vertexShell = static_cast<int32_t*>(s->dVertexShell); av.triangleShell = static_cast<int32_t*>(s->dTriangleShell);
    av.keep = wk + oKeep; av.remap = words(oRemap); av.tileC = words(oC);
    av.srcVertices = static_cast<const uint32_t*>(m->dVertices); av.srcNormals = static_cast<const uint32_t*>(m->dNormals); av.srcMaterials = static_cast<const uint32_t*>(m->dMaterials);
    FtShellsArgs at_ = av;                                             // the triangles' pass: sums, prefixes and total of its own
    av.tileA = words(oAV); av.scanTiles = av.nVTiles; av.totals = reinterpret_cast<unsigned long long*>(wk + oTotals);
    at_.tileA = words(oAT); at_.scanTiles = at_.nTTiles; at_.totals = av.totals + 2;
    hipError_t e = hipMemcpyAsync(wk + oKeep, keep, nS, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(hipFail(e, "select: upload"));
    if ((rc = launchShells(c, FT_SHELLS_K_KEEP_VERTEX_SUMS, av)) || (rc = launchShells(c, FT_SHELLS_K_SCAN, av)) ||
        (rc = launchShells(c, FT_SHELLS_K_KEEP_TRIANGLE_SUMS, at_)) || (rc = launchShells(c, FT_SHELLS_K_SCAN, at_))) return fail(rc);
    unsigned long long totals[4] = {0, 0, 0, 0};
    e = hipMemcpyAsync(totals, av.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);          // the one synchronisation: the kept vertices and triangles
    if (e != hipSuccess) return fail(hipFail(e, "select: totals"));
    if (totals[0] > nV || totals[2] > nT) return fail(setErr(FT_ERR_HIP, "select: impossible totals (internal error)"));
    r->nV = (int64_t)totals[0]; r->nT = (int64_t)totals[2];
    if (r->nV) e = hipMalloc(&r->dVertices, (size_t)r->nV * 12);
    if (e == hipSuccess && r->nT) e = hipMalloc(&r->dTriangles, (size_t)r->nT * 12);
    if (e == hipSuccess && r->nV && m->dNormals) e = hipMalloc(&r->dNormals, (size_t)r->nV * 12);
    if (e == hipSuccess && r->nV && m->dMaterials) e = hipMalloc(&r->dMaterials, (size_t)r->nV * 4);
    if (e != hipSuccess) return fail(hipFail(e, "hipMalloc"));
    av.nVOut = at_.nVOut = (uint32_t)r->nV; av.nTOut = at_.nTOut = (uint32_t)r->nT;
    av.dstVertices = static_cast<uint32_t*>(r->dVertices); av.dstNormals = static_cast<uint32_t*>(r->dNormals); av.dstMaterials = static_cast<uint32_t*>(r->dMaterials);
    at_.dstTriangles = static_cast<int32_t*>(r->dTriangles);
    if (!r->dNormals) av.srcNormals = nullptr;
    if (!r->dMaterials) av.srcMaterials = nullptr;
    if (r->nV && (rc = launchShells(c, FT_SHELLS_K_KEEP_VERTICES, av))) return fail(rc);
    if (r->nT && (rc = launchShells(c, FT_SHELLS_K_KEEP_TRIANGLES, at_))) return fail(rc);
    *out = r;
    return FT_OK;
}
// Internal (not in the header, like ft_ctx_mesh_tile; tools/shells_probe.py and the tests): the items per workgroup of this context's tiled shell
// kernels, one of 128, 256, 512, 1024.  Every tile gives the same result.
int ft_ctx_shells_tile(ft_ctx* c, int32_t tile) {
    if (!c || (tile != 128 && tile != 256 && tile != 512 && tile != 1024)) return setErr(FT_ERR_INVALID, "bad argument");
    c->shellsTile = (uint32_t)tile;
    return FT_OK;
}
// Internal (the tests and the probe): the iterations and the synchronisations of the context's last labelling
int ft_ctx_shells_last(ft_ctx* c, int64_t* last) {
    if (!c || !last) return setErr(FT_ERR_INVALID, "bad argument");
    last[0] = c->shellsLast[0]; last[1] = c->shellsLast[1];
    return FT_OK;
}

// Internal (tools/shells_probe.py): stop = 0 whole labellings; 1 / 2 / 3: this context's labellings end after the incidence lists / after the
// iterations / after the vertex labels and give shells that are not the rule's (no shell, labels unwritten), so that a stage's kernel time is a
// difference of two figures
int ft_ctx_shells_probe(ft_ctx* c, int32_t stop) {
    if (!c || stop < 0 || stop > 3) return setErr(FT_ERR_INVALID, "bad argument");
    c->shellsStop = stop;
    return FT_OK;
}

// ---- measures: ft_shells_measure, ft_mesh_measure (measure.hip; the rule is the header's "Measures") ------------------------------------------------
namespace {

const char* const kMeasureKernels[FT_MEASURE_KERNELS] = {"measure extent and box", "measure terms", "measure finish", "measure convert"};

int launchMeasure(ft_ctx* c, int kernel, const FtMeasureArgs& a) {
    int perCU = 0;
    const hipError_t e = ft_measure_occupancy(kernel, &perCU);
    if (e != hipSuccess) return hipFail(e, (std::string("occupancy of the ") + kMeasureKernels[kernel] + " kernel").c_str());
    int rc = clampPerCU(c, kMeasureKernels[kernel], perCU); if (rc) return rc;
    const int domain = ft_measure_domain(kernel);
    const uint64_t items = domain == 0 ? a.nV : (domain == 1 ? a.nT : a.nS);
    unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->numCUs * perCU, (items + FT_MEASURE_BLOCK - 1) / FT_MEASURE_BLOCK));
    if (c->measureGrid) blocks = c->measureGrid;
    return timedLaunch(c, c->stream, "ft_launch_measure", [&] { return ft_launch_measure(kernel, &a, blocks, c->stream); });
}

// is `p` device memory of this process (a host-only context never asks the runtime: everything is host memory to it)
bool measureOutOnDevice(const ft_ctx* c, const void* p) {
    if (!c->hasDevice || !p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }      // plain malloc memory: "invalid value"
    return attr.type == hipMemoryTypeDevice;
}

// The work memory of a call over nS shells, and the three launches.  Labels NULL: every vertex and triangle has label 0.  `out`: nS records in host
// or device memory (toDevice); the host form stages them in the work memory and synchronises the stream once.
int runMeasure(ft_ctx* c, const void* dVertices, size_t nV, const void* dTriangles, size_t nT, const void* dVertexShell, const void* dTriangleShell, size_t nS,
               ft_shell_measure* out, bool toDevice) {
    static_assert(sizeof(ft_shell_measure) == FT_MEASURE_RECORD_BYTES, "layout");
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    // zeroed: sums, maximum keys, counters, extent (adjacent); set to 0xff: minimum keys
    const size_t oSums = take(nS * 2 * FT_MEASURE_SUMS * 8), oMax = take(nS * 12), oBad = take(nS * 4), oExtent = take(4), oMin = take(nS * 12), zeroed = oMin;
    const size_t oStage = take(nS * sizeof(ft_shell_measure));
    int rc;
    if ((rc = ensureBytes(c->measureWork, c->measureWorkBytes, at))) return rc;
    unsigned char* wk = static_cast<unsigned char*>(c->measureWork);
    FtMeasureArgs a{};
    a.vertices = static_cast<const uint32_t*>(dVertices); a.triangles = static_cast<const int32_t*>(dTriangles);
    a.vertexShell = static_cast<const int32_t*>(dVertexShell); a.triangleShell = static_cast<const int32_t*>(dTriangleShell);
    a.nV = (uint32_t)nV; a.nT = (uint32_t)nT; a.nS = (uint32_t)nS;
    a.sums = reinterpret_cast<unsigned long long*>(wk + oSums);
    a.boxMax = reinterpret_cast<uint32_t*>(wk + oMax); a.unmeasured = reinterpret_cast<uint32_t*>(wk + oBad); a.extent = reinterpret_cast<uint32_t*>(wk + oExtent);
    a.boxMin = reinterpret_cast<uint32_t*>(wk + oMin);
    a.out = toDevice ? static_cast<void*>(out) : static_cast<void*>(wk + oStage);
    a.eager = c->measureEager;
    HIP_TRY(hipMemsetAsync(wk, 0, zeroed, c->stream));
    HIP_TRY(hipMemsetAsync(wk + oMin, 0xff, nS * 12, c->stream));
    if (nV && (rc = launchMeasure(c, FT_MEASURE_K_EXTENT, a))) return rc;
    if (c->measureStop == 1) return FT_OK;
    if (nT && (rc = launchMeasure(c, FT_MEASURE_K_TERMS, a))) return rc;
    if (c->measureStop == 2) return FT_OK;
    if ((rc = launchMeasure(c, FT_MEASURE_K_FINISH, a))) return rc;
    if (toDevice) return FT_OK;
    hipError_t e = hipMemcpyAsync(out, wk + oStage, nS * sizeof(ft_shell_measure), hipMemcpyDeviceToHost, c->stream);
    const hipError_t se = hipStreamSynchronize(c->stream);             // the one synchronisation of the host form
    if (e == hipSuccess) e = se;
    return e == hipSuccess ? FT_OK : hipFail(e, "measure: records");
}

// what both public entries share once their own NULL checks are done: alignment, empty input, device, run
int measureMesh(const ft_mesh* m, const ft_shells* s, size_t nS, ft_shell_measure* out) {
    ft_ctx* c = m->ctx;
    const bool nothing = nS == 0 || (m->nV == 0 && m->nT == 0);
    if (!out && !nothing) return setErr(FT_ERR_INVALID, "null out pointer");
    const bool toDevice = measureOutOnDevice(c, out);
    if (toDevice && (reinterpret_cast<uintptr_t>(out) & 7u)) return setErr(FT_ERR_INVALID, "measure: the device records must be 8-byte aligned");
    if (nothing) return FT_OK;
    int rc = requireDevice(c); if (rc) return rc;
    return runMeasure(c, m->dVertices, (size_t)m->nV, m->dTriangles, (size_t)m->nT, s ? s->dVertexShell : nullptr, s ? s->dTriangleShell : nullptr, nS, out, toDevice);
}

}  // namespace

int ft_shells_measure(const ft_mesh* m, const ft_shells* s, ft_shell_measure* out) {
    if (!m) return setErr(FT_ERR_INVALID, "null mesh");
    if (!s) return setErr(FT_ERR_INVALID, "null shells");
    if (!out && s->nS != 0 && (m->nV != 0 || m->nT != 0)) return setErr(FT_ERR_INVALID, "null out pointer");
    if (s->ctx != m->ctx || s->meshSerial != m->serial) return setErr(FT_ERR_INVALID, "measure: the shells were not built from this mesh");
    return measureMesh(m, s, (size_t)s->nS, out);
}
int ft_mesh_measure(const ft_mesh* m, ft_shell_measure* out) {
    if (!m) return setErr(FT_ERR_INVALID, "null mesh");
    return measureMesh(m, nullptr, 1, out);
}

// Internal (not in the header, like ft_ctx_shells_tile; the tests and tools/measure_probe.py): the measures of host arrays with arbitrary labels —
// vertices float32 [nV][3], triangles int32 [nT][3], vertex_label int32 [nV] and triangle_label int32 [nT] (either may be NULL: label 0), nS shells ->
// nS records in host memory.  Nothing is validated on the host: the kernels check every index and label (an index outside 0 .. nV - 1 makes the
// triangle unmeasured, a label outside 0 .. nS - 1 leaves the triangle or vertex out).
int ft_ctx_measure_triangles(ft_ctx* c, const float* vertices, int64_t nV, const int32_t* triangles, int64_t nT, const int32_t* vertex_label,
                             const int32_t* triangle_label, int64_t nS, ft_shell_measure* out) {
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if ((!vertices && nV) || (!triangles && nT) || (!out && nS)) return setErr(FT_ERR_INVALID, "null argument");
    if (nV < 0 || nT < 0 || nS < 0 || nV >= ((int64_t)1 << 31) || nT >= ((int64_t)1 << 31) || nS >= ((int64_t)1 << 31)) return setErr(FT_ERR_INVALID, "measure: counts must be in 0 .. 2^31 - 1");
    if (nS == 0) return FT_OK;
    int rc = requireDevice(c); if (rc) return rc;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    const size_t oV = take((size_t)nV * 12), oT = take((size_t)nT * 12), oVL = take((size_t)nV * 4), oTL = take((size_t)nT * 4);
    if ((rc = ensureScratch(c, std::max<size_t>(at, 256)))) return rc;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    const struct { size_t at; const void* host; size_t bytes; } parts[4] = {
        {oV, vertices, (size_t)nV * 12}, {oT, triangles, (size_t)nT * 12}, {oVL, vertex_label, (size_t)nV * 4}, {oTL, triangle_label, (size_t)nT * 4}};
    for (const auto& p : parts)
        if (p.host && p.bytes) HIP_TRY(hipMemcpyAsync(base + p.at, p.host, p.bytes, hipMemcpyHostToDevice, c->stream));
    return runMeasure(c, base + oV, (size_t)nV, base + oT, (size_t)nT, vertex_label ? base + oVL : nullptr, triangle_label ? base + oTL : nullptr, (size_t)nS, out, false);
}
// Internal (the tests): the finish kernel's conversion alone — sums: n pairs {low, high} of 64-bit words (two's complement) in host memory ->
// out[i] = fl64(sums[i]) * 2^-s as a double, in host memory
int ft_ctx_measure_finish(ft_ctx* c, const uint64_t* sums, int64_t n, int32_t s, double* out) {
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if (n < 0 || n >= ((int64_t)1 << 31) || ((!sums || !out) && n)) return setErr(FT_ERR_INVALID, "bad argument");
    if (n == 0) return FT_OK;
    int rc = requireDevice(c); if (rc) return rc;
    const size_t in = align256((size_t)n * 16);
    if ((rc = ensureScratch(c, in + (size_t)n * 8))) return rc;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    HIP_TRY(hipMemcpyAsync(base, sums, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    FtMeasureArgs a{};
    a.nS = (uint32_t)n; a.sums = reinterpret_cast<unsigned long long*>(base); a.out = base + in; a.scale = s;
    if ((rc = launchMeasure(c, FT_MEASURE_K_CONVERT, a))) return rc;
    HIP_TRY(hipMemcpyAsync(out, base + in, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}
// Internal (the tests and the probe): the workgroups of this context's measure launches; 0: as many as fill the device.  Every grid gives the same bytes.
int ft_ctx_measure_grid(ft_ctx* c, int32_t workgroups) {
    if (!c || workgroups < 0 || workgroups > 65536) return setErr(FT_ERR_INVALID, "bad argument");
    c->measureGrid = (unsigned)workgroups;
    return FT_OK;
}

// Internal (tools/measure_probe.py): stop = 0 whole calls; 1 / 2: this context's measure calls end after the extent kernel / after the terms kernel and
// write no record, so that a stage's kernel time is a difference of two figures.  eager = 1: the terms kernel flushes every lane's partial sums at
// every iteration — the form without the accumulation in registers, which gives the same bytes
int ft_ctx_measure_probe(ft_ctx* c, int32_t stop, int32_t eager) {
    if (!c || stop < 0 || stop > 2 || eager < 0 || eager > 1) return setErr(FT_ERR_INVALID, "bad argument");
    c->measureStop = stop; c->measureEager = eager;
    return FT_OK;
}

// ---- contour measures: ft_slices_measure (contour_measure.hip; the rule is the header's "Contour measures") -------------------------------------------
namespace {

const char* const kContourKernels[FT_CONTOUR_KERNELS] = {"contour extent and box", "contour terms", "contour polylines", "contour slices"};

int launchContour(ft_ctx* c, int kernel, const FtContourArgs& a) {
    int perCU = 0;
    const hipError_t e = ft_contour_occupancy(kernel, &perCU);
    if (e != hipSuccess) return hipFail(e, (std::string("occupancy of the ") + kContourKernels[kernel] + " kernel").c_str());
    int rc = clampPerCU(c, kContourKernels[kernel], perCU); if (rc) return rc;
    const int domain = ft_contour_domain(kernel);
    const uint64_t items = domain == 0 ? a.nP : (domain == 1 ? a.nL : a.nW);
    unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->numCUs * perCU, (items + FT_CONTOUR_BLOCK - 1) / FT_CONTOUR_BLOCK));
    if (c->contourGrid) blocks = c->contourGrid;
    return timedLaunch(c, c->stream, "ft_launch_contour", [&] { return ft_launch_contour(kernel, &a, blocks, c->stream); });
}

// What can be refused about the two outputs without a device, in the header's order: both NULL although something would be written, a misaligned device
// pointer, one address for both.  *pDev / *sDev: the output is device memory.
int checkContourOuts(const ft_ctx* c, const void* outP, const void* outS, size_t nL, size_t nW, bool* pDev, bool* sDev) {
    static_assert(sizeof(ft_contour_measure) == FT_CONTOUR_RECORD_BYTES && sizeof(ft_slice_measure) == FT_CONTOUR_SLICE_RECORD_BYTES, "layout");
    *pDev = *sDev = false;
    if (!outP && !outS && (nL || nW)) return setErr(FT_ERR_INVALID, "contour measures: null out pointers");
    *pDev = measureOutOnDevice(c, outP); *sDev = measureOutOnDevice(c, outS);
    if ((*pDev && (reinterpret_cast<uintptr_t>(outP) & 7u)) || (*sDev && (reinterpret_cast<uintptr_t>(outS) & 7u)))
        return setErr(FT_ERR_INVALID, "contour measures: the device records must be 8-byte aligned");
    if (outP && outP == outS) return setErr(FT_ERR_INVALID, "contour measures: the two outputs must not be the same address");
    return FT_OK;
}

// the slice records of contours without points and polylines: zeros and the +inf / -inf box, E = 0
void emptySliceRecords(ft_slice_measure* out, size_t nW) {
    ft_slice_measure r;
    std::memset(&r, 0, sizeof r);
    for (int x = 0; x < 2; ++x) { r.bbox_min[x] = std::numeric_limits<float>::infinity(); r.bbox_max[x] = -std::numeric_limits<float>::infinity(); }
    for (size_t w = 0; w < nW; ++w) out[w] = r;
}

// The work memory of a call over nL polylines and nW slices, and the four launches.  Points and polylines are device memory.  Each output is NULL, host
// memory (staged in the work memory; the stream is synchronised once, after both copies are queued) or device memory (written in place, nothing synchronised).
int runContour(ft_ctx* c, const void* dPoints, size_t nP, const void* dPolylines, size_t nL, int32_t axis, size_t nW, ft_contour_measure* outP, bool pDev,
               ft_slice_measure* outS, bool sDev) {
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    // zeroed: sums, maximum keys, counters, extent (adjacent); set to 0xff: minimum keys (adjacent)
    const size_t oSums = take(nL * 2 * FT_CONTOUR_SUMS * 8), oMax = take(nL * 8), oBad = take(nL * 4), oSSums = take(nW * 2 * FT_CONTOUR_SUMS * 8), oSMax = take(nW * 8),
                 oCount = take(nW * 4 * FT_CONTOUR_COUNTERS), oExtent = take(4), oMin = take(nL * 8), zeroed = oMin, oSMin = take(nW * 8), ones = at - oMin;
    const size_t oStageP = take(outP && !pDev ? nL * sizeof(ft_contour_measure) : 0), oStageS = take(outS && !sDev ? nW * sizeof(ft_slice_measure) : 0);
    int rc;
    if ((rc = ensureBytes(c->contourWork, c->contourWorkBytes, std::max<size_t>(at, 256)))) return rc;
    unsigned char* wk = static_cast<unsigned char*>(c->contourWork);
    auto words = [&](size_t o) { return reinterpret_cast<uint32_t*>(wk + o); };
    FtContourArgs a{};
    a.points = static_cast<const uint32_t*>(dPoints); a.polylines = static_cast<const int32_t*>(dPolylines);
    a.nP = (uint32_t)nP; a.nL = (uint32_t)nL; a.nW = (uint32_t)nW; a.axis = (uint32_t)axis;
    a.sums = reinterpret_cast<unsigned long long*>(wk + oSums); a.boxMin = words(oMin); a.boxMax = words(oMax); a.unmeasured = words(oBad);
    a.sliceSums = reinterpret_cast<unsigned long long*>(wk + oSSums); a.sliceBoxMin = words(oSMin); a.sliceBoxMax = words(oSMax); a.sliceCounters = words(oCount);
    a.extent = words(oExtent);
    a.outPolylines = !outP ? nullptr : (pDev ? static_cast<void*>(outP) : static_cast<void*>(wk + oStageP));
    a.outSlices = !outS ? nullptr : (sDev ? static_cast<void*>(outS) : static_cast<void*>(wk + oStageS));
    a.eager = c->contourEager;
    HIP_TRY(hipMemsetAsync(wk, 0, zeroed, c->stream));
    if (ones) HIP_TRY(hipMemsetAsync(wk + oMin, 0xff, ones, c->stream));
    if (nP && (rc = launchContour(c, FT_CONTOUR_K_EXTENT, a))) return rc;
    if (nP && nL && (rc = launchContour(c, FT_CONTOUR_K_TERMS, a))) return rc;
    if (nL && (outP || outS) && (rc = launchContour(c, FT_CONTOUR_K_POLYLINES, a))) return rc;
    if (nW && outS && (rc = launchContour(c, FT_CONTOUR_K_SLICES, a))) return rc;
    const bool pHost = outP && !pDev && nL, sHost = outS && !sDev && nW;
    if (!pHost && !sHost) return FT_OK;
    hipError_t e = hipSuccess;
    if (pHost) e = hipMemcpyAsync(outP, wk + oStageP, nL * sizeof(ft_contour_measure), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && sHost) e = hipMemcpyAsync(outS, wk + oStageS, nW * sizeof(ft_slice_measure), hipMemcpyDeviceToHost, c->stream);
    const hipError_t se = hipStreamSynchronize(c->stream);             // the one synchronisation of a call with a host output
    if (e == hipSuccess) e = se;
    return e == hipSuccess ? FT_OK : hipFail(e, "contour measures: records");
}

}  // namespace

int ft_slices_measure(const ft_slices* m, ft_contour_measure* out_polylines, ft_slice_measure* out_slices) {
    if (!m) return setErr(FT_ERR_INVALID, "null slices");
    ft_ctx* c = m->ctx;
    const size_t nL = (size_t)m->nL, nW = (size_t)m->nSlices;
    bool pDev, sDev;
    int rc = checkContourOuts(c, out_polylines, out_slices, nL, nW, &pDev, &sDev); if (rc) return rc;
    if (nL == 0 && !sDev) {                                            // empty contours: no device needed; a device output only exists where a device does
        if (out_slices) emptySliceRecords(out_slices, nW);
        return FT_OK;
    }
    if ((rc = requireDevice(c))) return rc;
    return runContour(c, m->dPoints, (size_t)m->nP, m->dPolylines, nL, m->axis, nW, out_polylines, pDev, out_slices, sDev);
}

// Internal (not in the header, like ft_ctx_measure_triangles; the tests and tools/contour_measure_probe.py): the contour measures of host arrays —
// points float32 [nP][3], polylines ft_polyline [nL], an axis and nW slices -> nL and nW records (either output may be NULL; host or device memory).
// Validated on the host before anything is uploaded: every [first, first + count) lies in 0 .. nP, every slice in 0 .. nW - 1, and `first` ascends
// without overlap (first[l + 1] >= first[l] + count[l]: what the slicer writes and the kernels' search relies on).  The kernels check every word again.
int ft_ctx_measure_polylines(ft_ctx* c, const float* points, int64_t nP, const ft_polyline* polylines, int64_t nL, int32_t axis, int64_t nW,
                             ft_contour_measure* out_polylines, ft_slice_measure* out_slices) {
    if (!c) return setErr(FT_ERR_INVALID, "null context");
    if ((!points && nP) || (!polylines && nL)) return setErr(FT_ERR_INVALID, "null argument");
    if (nP < 0 || nL < 0 || nW < 0 || nP >= ((int64_t)1 << 31) || nL >= ((int64_t)1 << 31) || nW >= ((int64_t)1 << 31))
        return setErr(FT_ERR_INVALID, "contour measures: counts must be in 0 .. 2^31 - 1");
    if (axis < 0 || axis > 2) return setErr(FT_ERR_INVALID, "contour measures: the axis must be 0, 1 or 2");
    bool pDev, sDev;
    int rc = checkContourOuts(c, out_polylines, out_slices, (size_t)nL, (size_t)nW, &pDev, &sDev); if (rc) return rc;
    int64_t end = 0;
    for (int64_t l = 0; l < nL; ++l) {
        const ft_polyline& p = polylines[l];
        if (p.first < 0 || p.count < 0 || (int64_t)p.first + p.count > nP) return setErr(FT_ERR_INVALID, "contour measures: a polyline's points lie outside 0 .. n_points");
        if (p.slice < 0 || p.slice >= nW) return setErr(FT_ERR_INVALID, "contour measures: a polyline's slice lies outside 0 .. n_slices - 1");
        if (p.first < end) return setErr(FT_ERR_INVALID, "contour measures: the polylines' points must ascend without overlap");
        end = (int64_t)p.first + p.count;
    }
    if (nL == 0 && nP == 0 && !sDev) {
        if (out_slices) emptySliceRecords(out_slices, (size_t)nW);
        return FT_OK;
    }
    if ((rc = requireDevice(c))) return rc;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; };
    const size_t oP = take((size_t)nP * 12), oL = take((size_t)nL * sizeof(ft_polyline));
    if ((rc = ensureScratch(c, std::max<size_t>(at, 256)))) return rc;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    if (nP) HIP_TRY(hipMemcpyAsync(base + oP, points, (size_t)nP * 12, hipMemcpyHostToDevice, c->stream));
    if (nL) HIP_TRY(hipMemcpyAsync(base + oL, polylines, (size_t)nL * sizeof(ft_polyline), hipMemcpyHostToDevice, c->stream));
    return runContour(c, base + oP, (size_t)nP, base + oL, (size_t)nL, axis, (size_t)nW, out_polylines, pDev, out_slices, sDev);
}
// Internal (the tests and the probe): the workgroups of this context's contour-measure launches; 0: as many as fill the device.  Every grid gives the same bytes.
int ft_ctx_contour_measure_grid(ft_ctx* c, int32_t workgroups) {
    if (!c || workgroups < 0 || workgroups > 65536) return setErr(FT_ERR_INVALID, "bad argument");
    c->contourGrid = (unsigned)workgroups;
    return FT_OK;
}
// Internal (tools/contour_measure_probe.py and the tests): eager = 1: the terms kernel adds every lane's terms by itself — the form without the
// segmented reduction across the wave, which gives the same bytes
int ft_ctx_contour_measure_probe(ft_ctx* c, int32_t eager) {
    if (!c || eager < 0 || eager > 1) return setErr(FT_ERR_INVALID, "bad argument");
    c->contourEager = eager;
    return FT_OK;
}

int ft_math_eval(ft_ctx* c, int32_t op, const float* x, const float* y, int64_t n, float* out) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!x || !out || n < 0 || op < 0 || op > 14 || ((op == 3 || op >= 10) && !y)) return setErr(FT_ERR_INVALID, "bad argument");
    if (n == 0) return FT_OK;
    const size_t b = align256((size_t)n * 4);
    if ((rc = ensureScratch(c, 3 * b))) return rc;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    HIP_TRY(hipMemcpyAsync(base, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (y) HIP_TRY(hipMemcpyAsync(base + b, y, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(ft_launch_math(op, reinterpret_cast<const float*>(base), reinterpret_cast<const float*>(base + b), n,
                           reinterpret_cast<float*>(base + 2 * b), c->stream));
    HIP_TRY(hipMemcpyAsync(out, base + 2 * b, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}

int ft_selftest_fastmath(ft_ctx* c, uint64_t mismatches[3]) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!mismatches) return setErr(FT_ERR_INVALID, "null output");
    if ((rc = ensureScratch(c, 256))) return rc;
    unsigned long long* d = static_cast<unsigned long long*>(c->scratch);
    HIP_TRY(hipMemsetAsync(d, 0, 24, c->stream));
    // sqrt: every float in [2^-96, 2^100]; exp: every float in [-2.9e6, -0] and [+0, 88]
    HIP_TRY(ft_launch_selftest(0, 0x0F800000u, 0x71800000u, d, c->stream));
    HIP_TRY(ft_launch_selftest(5, 0x27800000u, 0x48000000u, d, c->stream));    // strength -2 / -4 / -1/2 through the subtraction's output modifier: every root in [2^-48, 2^17] x four radii
    HIP_TRY(ft_launch_selftest(3, 0x0F800000u, 0x71800000u, d, c->stream));    // the 4-instruction form (output modifiers) under the NEAR loop's mode: same range, same counter
    HIP_TRY(ft_launch_selftest(1, 0x80000000u, 0xCA310080u, d + 1, c->stream));
    HIP_TRY(ft_launch_selftest(1, 0x00000000u, 0x42B00000u, d + 1, c->stream));
    // exponent-add form of exp ("near" regime): every float in [-87, -0] and [+0, 88]
    HIP_TRY(ft_launch_selftest(2, 0x80000000u, 0xC2AE0000u, d + 2, c->stream));
    HIP_TRY(ft_launch_selftest(2, 0x00000000u, 0x42B00000u, d + 2, c->stream));
    HIP_TRY(ft_launch_selftest(4, 0x80000000u, 0xC2AE0000u, d + 2, c->stream));  // the same form under the NEAR loop's mode (IEEE off, f32 denormals flushed)
    HIP_TRY(ft_launch_selftest(4, 0x00000000u, 0x42B00000u, d + 2, c->stream));
    unsigned long long h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, d, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    mismatches[0] = h[0]; mismatches[1] = h[1]; mismatches[2] = h[2];
    return FT_OK;
}

int ft_selftest_libm(ft_ctx* c, int32_t op, int32_t variant, float y, uint32_t lo_bits, int32_t n_chunks, uint64_t* sums) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!sums || op < 0 || op > 2 || (variant != FT_MATH_GLIBC_FMA && variant != FT_MATH_GLIBC_SSE2) || n_chunks < 1 || n_chunks > 256 ||
        (uint64_t)lo_bits + ((uint64_t)n_chunks << 24) > (1ull << 32)) return setErr(FT_ERR_INVALID, "bad argument");
    if ((rc = ensureScratch(c, (size_t)n_chunks * 8))) return rc;
    unsigned long long* d = static_cast<unsigned long long*>(c->scratch);
    HIP_TRY(hipMemsetAsync(d, 0, (size_t)n_chunks * 8, c->stream));
    HIP_TRY(ft_launch_libm_checksum(op, variant, y, lo_bits, (uint32_t)n_chunks, d, c->stream));
    HIP_TRY(hipMemcpyAsync(sums, d, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}

// Internal (not in the header, like ft_ctx_mesh_tile; tests/test_gpu_wave_primitives.py): the wave primitives of kernels.hip on n_waves x 64 host floats,
// every wave with all 64 lanes live.  op 0: out receives FT_WAVE_PROBE_PLANES planes of n_waves x 64 floats (both maxima, both prefix sums with their
// totals, both exclusive prefixes); op 1: four planes, four lean maxima back to back (kernels.hip ft_selftest_wave_kernel).  scale multiplies every
// input in front of a maximum; the tests pass 1.
int ft_selftest_wave(ft_ctx* c, int32_t op, const float* x, float scale, int32_t n_waves, float* out) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!x || !out || op < 0 || op > 1 || n_waves < 1 || n_waves > 65536) return setErr(FT_ERR_INVALID, "bad argument");
    const size_t plane = (size_t)n_waves * 64 * 4, outBytes = (op == 0 ? FT_WAVE_PROBE_PLANES : 4) * plane;
    if ((rc = ensureScratch(c, align256(plane) + outBytes))) return rc;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    HIP_TRY(hipMemcpyAsync(base, x, plane, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(ft_launch_selftest_wave(op, reinterpret_cast<const float*>(base), scale, (uint32_t)n_waves, reinterpret_cast<float*>(base + align256(plane)), c->stream));
    HIP_TRY(hipMemcpyAsync(out, base + align256(plane), outBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}

// Internal (tests/test_gpu_cull_pass.py): both wordings of the culling pass (kernels.hip ft_cull_children<false>, <true>) on n_waves x 64 host points,
// wave w under the lane mask masks[w] (never 0).  words: 2 per wave, the general wording's return first; rows: 2 x FT_CULL_ROW floats per wave in the
// same order, FT_CULL_PROBE_FILL where no pass wrote.  A scene without a cull site gives FT_CULL_NONE twice and untouched rows.
int ft_selftest_cull(ft_ctx* c, const ft_scene* s, const ft_vec3* pts, const uint64_t* masks, int32_t n_waves, uint32_t* words, float* rows) {
    int rc = requireDevice(c); if (rc) return rc;
    if (!s || s->ctx != c) return setErr(FT_ERR_INVALID, "bad argument (scene must belong to this context)");
    if (!pts || !masks || !words || !rows || n_waves < 1 || n_waves > 4096) return setErr(FT_ERR_INVALID, "bad argument");
    for (int32_t w = 0; w < n_waves; ++w) if (masks[w] == 0) return setErr(FT_ERR_INVALID, "a wave's lane mask must not be empty");
    int maxLds = 0;
    HIP_TRY(hipDeviceGetAttribute(&maxLds, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    const size_t lds = ft_selftest_cull_lds_bytes(s->dev.nStage);
    if (lds > (size_t)maxLds) return setErr(FT_ERR_UNSUPPORTED, "scene needs " + std::to_string(lds) + " bytes of LDS per workgroup; the device offers " + std::to_string(maxLds));
    const size_t pBytes = align256((size_t)n_waves * 64 * 12), mBytes = align256((size_t)n_waves * 8), wBytes = align256((size_t)n_waves * 8),
                 rBytes = (size_t)n_waves * 2 * FT_CULL_ROW * 4;
    if ((rc = ensureScratch(c, pBytes + mBytes + wBytes + rBytes))) return rc;
    unsigned char* base = static_cast<unsigned char*>(c->scratch);
    HIP_TRY(hipMemcpyAsync(base, pts, (size_t)n_waves * 64 * 12, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(base + pBytes, masks, (size_t)n_waves * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(ft_launch_selftest_cull(&s->dev, reinterpret_cast<const float*>(base), reinterpret_cast<const unsigned long long*>(base + pBytes), (uint32_t)n_waves,
                                    reinterpret_cast<uint32_t*>(base + pBytes + mBytes), reinterpret_cast<float*>(base + pBytes + mBytes + wBytes), c->stream));
    HIP_TRY(hipMemcpyAsync(words, base + pBytes + mBytes, (size_t)n_waves * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(rows, base + pBytes + mBytes + wBytes, rBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FT_OK;
}
// Internal (the same test): the scene's cull site as flattened — site[0] the run's child count (0: no site), site[1] its flags (FT_FLAG_INIT: the run
// starts its accumulator), site[2] the bits of its strength's negative inverse; records (may be NULL): the first min(count, capacity) children, 4 floats each
int ft_scene_cull_site(const ft_scene* s, uint32_t site[3], float* records, int32_t capacity) {
    if (!s || !site || capacity < 0 || (capacity > 0 && !records)) return setErr(FT_ERR_INVALID, "bad argument");
    const ft::FlatScene& f = s->flat;
    site[0] = site[1] = site[2] = 0u;
    if (f.hdr.cullPc == 0xffffffffu) return FT_OK;
    const FtInstr& in = f.instr[f.hdr.cullPc];
    site[0] = in.count; site[1] = in.flags; memcpy(&site[2], &in.f0, 4);
    const size_t n = std::min<size_t>(in.count, (size_t)capacity);
    if (n) memcpy(records, f.consts.data() + in.data, n * 16);
    return FT_OK;
}

// ---- internal hooks for multi.cpp (not part of the public ABI) ------------------------------------------
int ft_ctx_device_(const ft_ctx* c) { return (c && c->hasDevice) ? c->device : -1; }
void* ft_ctx_stream_(const ft_ctx* c) { return c ? (void*)c->stream : nullptr; }
void ft_set_error_(int, const char* msg) { g_err = msg ? msg : ""; }

// ---- introspection ---------------------------------------------------------------------------------
int ft_scene_info_get(const ft_scene* s, ft_scene_info* o) {
    if (!s || !o) return setErr(FT_ERR_INVALID, "null argument");
    const ft::FlatScene& f = s->flat;
    o->n_instr = (int32_t)f.instr.size(); o->n_slots = (int32_t)f.hdr.nSlots; o->n_consts = (int32_t)f.consts.size();
    o->n_grids = (int32_t)f.grids.size(); o->n_children = (int32_t)f.children.size(); o->n_cells = (int32_t)(f.cellCenters.size() / 3);
    o->n_items = (int32_t)f.items.size(); o->n_lights = (int32_t)f.lights.size(); o->n_materials = (int32_t)(f.materials.size() / 3);
    o->fast_path = (int32_t)f.hdr.fastPath;
    o->cull_pc = (int32_t)f.hdr.cullPc;
    return FT_OK;
}

int ft_scene_grid_shape(const ft_scene* s, int32_t g, float info[6], int32_t counts[3], int32_t* nCells, int32_t* nItems) {
    if (!s || g < 0 || (size_t)g >= s->flat.grids.size()) return setErr(FT_ERR_INVALID, "bad grid index");
    if (!info || !counts) return setErr(FT_ERR_INVALID, "null output");
    const FtGrid& G = s->flat.grids[g];
    for (int i = 0; i < 3; ++i) { info[i] = G.aabbMin[i]; info[3 + i] = G.cellSizeInv[i]; counts[i] = G.count[i]; }
    const int32_t nc = G.count[0] * G.count[1] * G.count[2];
    if (nCells) *nCells = nc;
    if (nItems) *nItems = (int32_t)(s->flat.cellStart[G.cellBase + nc] - s->flat.cellStart[G.cellBase]);
    return FT_OK;
}

int ft_scene_support_sphere(const ft_scene* s, float cr[4]) {
    if (!s || !cr) return setErr(FT_ERR_INVALID, "null argument");
    memcpy(cr, s->flat.hdr.escC, 3 * sizeof(float)); cr[3] = s->flat.hdr.escR;
    return FT_OK;
}
int ft_scene_miss_certificate(const ft_scene* s, float out[5]) {
    if (!s || !out) return setErr(FT_ERR_INVALID, "null argument");
    const FtSceneDev& h = s->flat.hdr;
    out[0] = h.certM; out[1] = h.certClip; out[2] = h.certRho2; out[3] = h.certLenF; out[4] = (float)h.certSteps;
    return FT_OK;
}
int ft_scene_occlusion_certificate(const ft_scene* s, float out[7]) {
    if (!s || !out) return setErr(FT_ERR_INVALID, "null argument");
    static_assert(sizeof(FtOccl) == 7 * sizeof(float), "out[7] is FtOccl, field by field");
    memcpy(out, &s->flat.occ, sizeof(FtOccl));
    return FT_OK;
}
int ft_scene_departure_certificate(const ft_scene* s, float out[7]) {
    if (!s || !out) return setErr(FT_ERR_INVALID, "null argument");
    const FtDepart& d = s->flat.dep;
    out[0] = d.e; out[1] = d.b; out[2] = d.k; out[3] = d.epsMin; out[4] = d.clip; out[5] = d.lenF; out[6] = (float)d.steps;
    return FT_OK;
}
int ft_scene_miss_certificate_clusters(const ft_scene* s, int32_t* nClusters, int32_t* nChildren, float* out, int32_t capacity) {
    if (!s || !nClusters || !nChildren) return setErr(FT_ERR_INVALID, "null argument");
    const ft::FlatScene& f = s->flat;
    *nClusters = (int32_t)f.hdr.certK;
    *nChildren = (int32_t)((f.certCl.size() - 8u * f.hdr.certK) / 4u);
    if (!out) return FT_OK;
    if (capacity < 0 || (size_t)capacity < f.certCl.size()) return setErr(FT_ERR_INVALID, "capacity below 8 n_clusters + 4 n_children floats");
    if (!f.certCl.empty()) memcpy(out, f.certCl.data(), f.certCl.size() * 4);
    return FT_OK;
}

int ft_scene_grid_dump(const ft_scene* s, int32_t g, uint32_t* cellStart, float* centers, float* lower, int32_t* child) {
    if (!s || g < 0 || (size_t)g >= s->flat.grids.size()) return setErr(FT_ERR_INVALID, "bad grid index");
    if (!cellStart || !centers || !lower || !child) return setErr(FT_ERR_INVALID, "null output");
    const ft::FlatScene& f = s->flat;
    const FtGrid& G = f.grids[g];
    const uint32_t nc = (uint32_t)(G.count[0] * G.count[1] * G.count[2]);
    const uint32_t first = f.cellStart[G.cellBase];
    for (uint32_t c = 0; c <= nc; ++c) cellStart[c] = f.cellStart[G.cellBase + c] - first;
    memcpy(centers, f.cellCenters.data() + 3 * (size_t)G.cellBase, (size_t)nc * 12);
    const uint32_t ni = f.cellStart[G.cellBase + nc] - first;
    for (uint32_t i = 0; i < ni; ++i) { lower[i] = f.items[first + i].lowerBound; child[i] = (int32_t)f.items[first + i].child; }
    return FT_OK;
}

}  // extern "C"
