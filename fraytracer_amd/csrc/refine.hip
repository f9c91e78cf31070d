// refine.hip — mesh and contour vertices moved onto the surface by bisection of their lattice edge, and the same machinery for caller-given segments
// (include/fraytracer_hip.h "Refinement" is the rule; this file is its device side).  Three kernels, one lane per item, grid-stride, no atomics:
//   lattice    one lane per lattice point q: the brackets of the edges q owns, in key order, from the mask and vbase the count and emit passes left
//   segments   one lane per segment: status and bracket from the two end distances
//   round      one lane per bracket: D(M) read, the rule applied
// Each ends with the next midpoint M, or on the last round (with no round: at once) with the finish.  The field evaluations between two rounds are
// the library's points-form field launch over the midpoint buffer; nothing here evaluates a distance.
// Built with -ffp-contract=off like every other object: each sum, product and quotient of the rule is rounded on its own.
#include <hip/hip_runtime.h>

#include "ft_refine.h"

namespace {

constexpr uint32_t ft_refine_codes(uint32_t c0, uint32_t c1, uint32_t c2) { return c0 | (c1 << 3) | (c2 << 6); }
constexpr uint32_t FT_REFINE_SLICE_CODES[3] = FT_REFINE_EDGES_SLICE;
static_assert(FT_REFINE_EDGES_MESH == (ft_refine_codes(1, 2, 3) | (ft_refine_codes(4, 5, 6) << 9) | (7u << 18)), "the mesher's seven directions");
// axis a: +v, +u, +u+v with u = (a + 1) % 3, v = (a + 2) % 3 and the codes 4, 2, 1 of the axes 0, 1, 2, ascending
static_assert(FT_REFINE_SLICE_CODES[0] == ft_refine_codes(1, 2, 3) && FT_REFINE_SLICE_CODES[1] == ft_refine_codes(1, 4, 5) &&
              FT_REFINE_SLICE_CODES[2] == ft_refine_codes(2, 4, 6), "the slicer's three directions per axis");

__device__ __forceinline__ bool ft_refine_finite(float s) { return __builtin_fabsf(s) < __builtin_inff(); }        // false for NaN

struct FtRefineItem { float a[3], b[3], sa, sb; };

__device__ __forceinline__ void ft_refine_store(const FtRefineBracket& br, uint32_t v, const FtRefineItem& x) {
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) { br.a[ax][v] = x.a[ax]; br.b[ax][v] = x.b[ax]; }
    br.sa[v] = x.sa; br.sb[v] = x.sb;
}

// how every kernel ends: the next midpoint, or the finish — the mesher's operations, from A towards B
__device__ __forceinline__ void ft_refine_end(const FtRefineArgs& g, uint32_t v, const FtRefineItem& x) {
    if (!g.last) {
        float* m = g.mid + 3 * (size_t)v;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) m[ax] = (x.a[ax] + x.b[ax]) * 0.5f;
        return;
    }
    const float t = x.sa / (x.sa - x.sb);
    float* out = g.out + 3 * (size_t)v;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) out[ax] = x.a[ax] + t * (x.b[ax] - x.a[ax]);
}

// no bracket: three NaN at the end, and until then a midpoint the field has already been asked at (`at`)
__device__ __forceinline__ void ft_refine_end_dead(const FtRefineArgs& g, uint32_t v, const float* at) {
    const float nan = __builtin_nanf("");
    if (g.last) { float* out = g.out + 3 * (size_t)v; out[0] = nan; out[1] = nan; out[2] = nan; }
    else if (at) { float* m = g.mid + 3 * (size_t)v; m[0] = at[0]; m[1] = at[1]; m[2] = at[2]; }
}

__global__ __launch_bounds__(FT_REFINE_BLOCK) void ft_refine_lattice_kernel(FtRefineArgs g) {
    const unsigned long long stride = (unsigned long long)gridDim.x * FT_REFINE_BLOCK;
    for (unsigned long long q64 = (unsigned long long)blockIdx.x * FT_REFINE_BLOCK + threadIdx.x; q64 < g.n; q64 += stride) {
        const uint32_t q = (uint32_t)q64, own = g.mask[q];
        if (!own) continue;
        const uint32_t at = g.vbase[q];
        const uint32_t k = q % g.nz, ij = q / g.nz, j = ij % g.ny, i = ij / g.ny;
        const uint32_t idx[3] = {i, j, k};
        FtRefineItem x;
        x.sa = g.values[q] - g.iso;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) x.a[ax] = g.origin[ax] + (float)idx[ax] * g.step[ax];
        uint32_t rank = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 7u; ++b) {                            // ascending e; a slicer's mask has three bits
            if (!((own >> b) & 1u)) continue;
            const uint32_t c = (g.edges >> (3u * b)) & 7u;
            const uint32_t d[3] = {(c >> 2) & 1u, (c >> 1) & 1u, c & 1u};
            const uint32_t v = at + rank;
            ++rank;
            if (v >= g.nV) continue;
            x.sb = g.values[(size_t)q + (size_t)d[0] * g.ny * g.nz + (size_t)d[1] * g.nz + d[2]] - g.iso;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) x.b[ax] = g.origin[ax] + (float)(idx[ax] + d[ax]) * g.step[ax];
            ft_refine_store(g.br, v, x);
            ft_refine_end(g, v, x);
        }
    }
}

__global__ __launch_bounds__(FT_REFINE_BLOCK) void ft_refine_segments_kernel(FtRefineArgs g) {
    const unsigned long long stride = (unsigned long long)gridDim.x * FT_REFINE_BLOCK;
    for (unsigned long long v64 = (unsigned long long)blockIdx.x * FT_REFINE_BLOCK + threadIdx.x; v64 < g.nV; v64 += stride) {
        const uint32_t v = (uint32_t)v64;
        const float* pa = g.segA + 3 * (size_t)v;
        const float* pb = g.segB + 3 * (size_t)v;
        FtRefineItem x;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { x.a[ax] = pa[ax]; x.b[ax] = pb[ax]; }
        x.sa = g.distA[v] - g.iso; x.sb = g.distB[v] - g.iso;
        const bool crosses = ft_refine_finite(x.sa) && ft_refine_finite(x.sb) && ((x.sa < 0.0f) != (x.sb < 0.0f));
        if (g.status) g.status[v] = crosses ? 1 : 0;
        if (!g.mid && !g.out) continue;                                // only the status was asked for
        if (!crosses) x.sa = __builtin_nanf("");
        ft_refine_store(g.br, v, x);
        if (crosses) ft_refine_end(g, v, x); else ft_refine_end_dead(g, v, x.a);
    }
}

__global__ __launch_bounds__(FT_REFINE_BLOCK) void ft_refine_round_kernel(FtRefineArgs g) {
    const unsigned long long stride = (unsigned long long)gridDim.x * FT_REFINE_BLOCK;
    for (unsigned long long v64 = (unsigned long long)blockIdx.x * FT_REFINE_BLOCK + threadIdx.x; v64 < g.nV; v64 += stride) {
        const uint32_t v = (uint32_t)v64;
        FtRefineItem x;
        x.sa = g.br.sa[v];
        if (x.sa != x.sa) { ft_refine_end_dead(g, v, nullptr); continue; }
        x.sb = g.br.sb[v];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { x.a[ax] = g.br.a[ax][v]; x.b[ax] = g.br.b[ax][v]; }
        const float* m = g.mid + 3 * (size_t)v;
        const float sm = g.dist[v] - g.iso;
        if (ft_refine_finite(sm)) {                                    // otherwise the bracket stays as it is
            if ((sm < 0.0f) == (x.sa < 0.0f)) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { x.a[ax] = m[ax]; g.br.a[ax][v] = x.a[ax]; }
                x.sa = sm; g.br.sa[v] = sm;
            } else {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { x.b[ax] = m[ax]; g.br.b[ax][v] = x.b[ax]; }
                x.sb = sm; g.br.sb[v] = sm;
            }
        }
        ft_refine_end(g, v, x);
    }
}

const void* ft_refine_kernel(int kernel) {
    switch (kernel) {
        case FT_REFINE_K_LATTICE: return (const void*)ft_refine_lattice_kernel;
        case FT_REFINE_K_SEGMENTS: return (const void*)ft_refine_segments_kernel;
        case FT_REFINE_K_ROUND: return (const void*)ft_refine_round_kernel;
    }
    return nullptr;
}

}  // namespace

extern "C" hipError_t ft_launch_refine(int kernel, const FtRefineArgs* a, unsigned blocks, hipStream_t st) {
    const void* k = ft_refine_kernel(kernel);
    if (!k) return hipErrorInvalidDeviceFunction;
    FtRefineArgs args = *a;
    void* kp[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(FT_REFINE_BLOCK), kp, 0, st);
}
extern "C" hipError_t ft_refine_occupancy(int kernel, int* blocksPerCU) {
    const void* k = ft_refine_kernel(kernel);
    if (!k) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocksPerCU, k, FT_REFINE_BLOCK, 0);
}
