// slice.hip — ordered contour loops from a lattice of distances: per lattice plane the section of the mesher's surface (include/fraytracer_hip.h
// "Slicing" is the rule; this file is its device side).  No atomics, so that vertex, point and polyline order are the rule's:
//   count, scan, emit   as the mesher's: per point the 3-bit mask of the vertices it owns in its plane, tile sums, their prefix sums, the vertices in
//                       key order
//   link                per cell its at most two segments: next[start] = end, prev[end] = start; every word has one writer
//   lead, jump x R      pointer doubling along prev with (ancestor, hops, smallest index seen), double-buffered: 2^R >= the vertex total, so a vertex that
//                       has not reached a head by then is on a cycle and has seen all of it
//   cut, jump x R       the same with every cycle cut in front of its smallest vertex: every vertex then knows (head, rank)
//   tail, heads, scan, records, scatter   the last vertex of a polyline gives its head the length; polyline numbers and point offsets are prefix sums
//                       over the vertices, in key order by construction
// Built with -ffp-contract=off like every other object: each product, sum and quotient of the vertex rule is rounded on its own.
#include <hip/hip_runtime.h>

#include "ft_slice.h"

namespace {

// ---- the direction table, from the integer corner offsets ----------------------------------------------------------------------------------------
// Corner code c = 2 du + dv in the plane's (u, v).  Triangle 0 is {c0, c0 + u, c0 + u + v}, triangle 1 {c0, c0 + v, c0 + u + v}.
__host__ __device__ constexpr uint32_t ft_slice_corner(int t, int x) { return x == 0 ? 0u : (x == 2 ? 3u : (t == 0 ? 2u : 1u)); }

struct FtSliceTable { uint32_t e[2][8]; };

constexpr uint32_t ft_slice_slot(uint32_t x, uint32_t y) {             // the edge between corners x and y: owned by the one nearer c0
    const uint32_t wx = (x >> 1) + (x & 1u), wy = (y >> 1) + (y & 1u);
    const uint32_t lo = wx < wy ? x : y, hi = wx < wy ? y : x;
    return (lo << 2) | (2u * ((hi >> 1) - (lo >> 1)) + ((hi & 1u) - (lo & 1u)));
}

constexpr FtSliceTable ft_slice_make_table() {
    FtSliceTable T{};
    for (int t = 0; t < 2; ++t) {
        for (int m = 1; m < 7; ++m) {                                  // bit x of m: corner x of the triangle is inside
            const int inside = (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1);
            const bool lIn = inside == 1;
            int l = 0;
            for (int x = 0; x < 3; ++x) if ((((m >> x) & 1) == 1) == lIn) l = x;
            const int m1 = l == 0 ? 1 : 0, m2 = l == 2 ? 1 : 2;
            const int cl = (int)ft_slice_corner(t, l), c1 = (int)ft_slice_corner(t, m1), c2 = (int)ft_slice_corner(t, m2);
            const int ax = (c2 >> 1) - (c1 >> 1), ay = (c2 & 1) - (c1 & 1), bx = (cl >> 1) - (c1 >> 1), by = (cl & 1) - (c1 & 1);
            const int det = ax * by - ay * bx;                         // det(M2 - M1, L - M1)
            const bool forward = (det > 0) == lIn;                     // from the vertex on (L, M1) to the one on (L, M2): the inside lies to the left
            const uint32_t s1 = ft_slice_slot((uint32_t)cl, (uint32_t)c1), s2 = ft_slice_slot((uint32_t)cl, (uint32_t)c2);
            T.e[t][m] = 1u | ((forward ? s1 : s2) << 1) | ((forward ? s2 : s1) << 5);
        }
    }
    return T;
}

constexpr FtSliceTable FT_SLICE_TABLE_HOST = ft_slice_make_table();
__constant__ FtSliceTable FT_SLICE_TABLE = ft_slice_make_table();

// ---- what a lane knows about its point --------------------------------------------------------------------------------------------------------
struct FtSlicePlane { uint32_t su, sv; bool swapUV; };                 // strides of the in-plane axes in the points' indexing; axis 1: +u is the lower e
struct FtSliceCorners { uint32_t in4, fin4; bool cell; };              // bit c: corner c of cell q is inside / is a lattice point with a finite value

// x[i] of three values without an indexed array (a runtime index would put the array into scratch)
__device__ __forceinline__ uint32_t ft_slice_pick(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t i) { return i == 0u ? x0 : (i == 1u ? x1 : x2); }
__device__ __forceinline__ FtSlicePlane ft_slice_plane(const FtSliceArgs& a) {
    const uint32_t u = (a.axis + 1u) % 3u, v = (a.axis + 2u) % 3u, s0 = a.ny * a.nz;
    return FtSlicePlane{ft_slice_pick(s0, a.nz, 1u, u), ft_slice_pick(s0, a.nz, 1u, v), a.axis == 1u};
}
__device__ __forceinline__ float ft_slice_signed(const FtSliceArgs& a, size_t q) { return a.values[q] - a.iso; }
__device__ __forceinline__ bool ft_slice_finite(float s) { return __builtin_fabsf(s) < __builtin_inff(); }      // false for NaN
__device__ __forceinline__ size_t ft_slice_corner_at(const FtSlicePlane& p, size_t q, uint32_t c) { return q + (size_t)(c >> 1) * p.su + (size_t)(c & 1u) * p.sv; }
// the bit of the owner's mask for the edge of direction code dd (1: +v, 2: +u, 3: +u+v): the three in ascending e
__device__ __forceinline__ uint32_t ft_slice_bit(const FtSlicePlane& p, uint32_t dd) { return dd == 3u ? 2u : ((dd == 2u) != p.swapUV ? 1u : 0u); }

__device__ __forceinline__ FtSliceCorners ft_slice_classify(const FtSliceArgs& a, const FtSlicePlane& p, uint32_t q) {
    const uint32_t k = q % a.nz, ij = q / a.nz, j = ij % a.ny, i = ij / a.ny;
    const uint32_t u = (a.axis + 1u) % 3u, v = (a.axis + 2u) % 3u;
    const bool eu = ft_slice_pick(i, j, k, u) + 1u < ft_slice_pick(a.nx, a.ny, a.nz, u), ev = ft_slice_pick(i, j, k, v) + 1u < ft_slice_pick(a.nx, a.ny, a.nz, v);
    FtSliceCorners r{0u, 0u, eu && ev};
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) {
        const bool exists = (!(c & 2u) || eu) && (!(c & 1u) || ev);
        if (!exists) continue;
        const float s = ft_slice_signed(a, ft_slice_corner_at(p, q, c));
        if (ft_slice_finite(s)) r.fin4 |= 1u << c;
        if (s < 0.0f) r.in4 |= 1u << c;
    }
    return r;
}

// the vertices q owns, as mask bits: the edge of direction dd ends at corner dd
__device__ __forceinline__ uint32_t ft_slice_owned(const FtSlicePlane& p, const FtSliceCorners& r) {
    if (!(r.fin4 & 1u)) return 0u;
    const uint32_t differs = ((r.in4 & 1u) ? ~r.in4 : r.in4) & r.fin4;
    uint32_t own = 0u;
#pragma unroll
    for (uint32_t dd = 1; dd < 4u; ++dd) if ((differs >> dd) & 1u) own |= 1u << ft_slice_bit(p, dd);
    return own;
}

// triangle t of cell q: its inside mask, or 8 where a corner is not finite
__device__ __forceinline__ uint32_t ft_slice_case(const FtSliceCorners& r, int t) {
    const uint32_t c1 = ft_slice_corner(t, 1), need = 1u | (1u << c1) | 8u;
    if ((r.fin4 & need) != need) return 8u;
    return (r.in4 & 1u) | (((r.in4 >> c1) & 1u) << 1) | (((r.in4 >> 3) & 1u) << 2);
}
__device__ __forceinline__ uint32_t ft_slice_case_segments(uint32_t m) { return (m >= 1u && m <= 6u) ? 1u : 0u; }

// ---- sums and scans across a workgroup ------------------------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup's threads; every thread calls it.  lds: one word per wave, reusable after the call's last barrier
__device__ __forceinline__ uint32_t ft_slice_block_exclusive(uint32_t v, uint32_t* lds) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(inc, off, 64); if (lane >= (uint32_t)off) inc += t; }
    __syncthreads();                                                   // the previous user of lds is done
    if (lane == 63u) lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t w = 0; w < wave; ++w) before += lds[w];
    return before + inc - v;
}

// the workgroup's sums of x, y, z into out[tile]; every thread calls it.  red: three words per wave
template <int TILE> __device__ __forceinline__ void ft_slice_tile_sums(uint32_t x, uint32_t y, uint32_t z, uint32_t* red, uint32_t tile, uint32_t* ox, uint32_t* oy,
                                                                        uint32_t* oz) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { x += __shfl_down(x, off, 64); y += __shfl_down(y, off, 64); z += __shfl_down(z, off, 64); }
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) { const uint32_t w = threadIdx.x >> 6; red[3u * w] = x; red[3u * w + 1u] = y; red[3u * w + 2u] = z; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sx = 0u, sy = 0u, sz = 0u;
        for (int w = 0; w < TILE / 64; ++w) { sx += red[3 * w]; sy += red[3 * w + 1]; sz += red[3 * w + 2]; }
        ox[tile] = sx; oy[tile] = sy; oz[tile] = sz;
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_slice_count_kernel(FtSliceArgs a) {
    __shared__ uint32_t red[3 * (TILE / 64)];
    const FtSlicePlane p = ft_slice_plane(a);
    for (uint32_t tile = blockIdx.x; tile < a.nTiles; tile += gridDim.x) {
        const unsigned long long q64 = (unsigned long long)tile * TILE + threadIdx.x;
        uint32_t verts = 0u, segs = 0u, skipped = 0u;
        if (q64 < a.n) {
            const uint32_t q = (uint32_t)q64;
            const FtSliceCorners r = ft_slice_classify(a, p, q);
            const uint32_t own = ft_slice_owned(p, r);
            a.mask[q] = (uint8_t)own;
            verts = (uint32_t)__popc(own);
            if (r.cell) {
#pragma unroll
                for (int t = 0; t < 2; ++t) { const uint32_t m = ft_slice_case(r, t); segs += ft_slice_case_segments(m); skipped += m >= 8u ? 1u : 0u; }
            }
        }
        ft_slice_tile_sums<TILE>(verts, segs, skipped, red, tile, a.tileA, a.tileB, a.tileC);
    }
}

// One workgroup.  Levels as in the mesher's scan: FT_SLICE_SCAN_ITEMS tile sums in a thread, 64 threads in a wave, the waves through LDS, and a carry from
// each round of FT_SLICE_SCAN_BLOCK * FT_SLICE_SCAN_ITEMS tiles to the next.  The prefixes are kept mod 2^32 (2^31 or more is refused from the 64-bit
// totals before anything reads them).  x, y: scanned in place; z: only summed.
__device__ __forceinline__ void ft_slice_scan(uint32_t* x, uint32_t* y, const uint32_t* z, uint32_t nTiles, unsigned long long* totals) {
    constexpr int WAVES = FT_SLICE_SCAN_BLOCK / 64;
    __shared__ unsigned long long wx[WAVES], wy[WAVES], wz[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carryX = 0ull, carryY = 0ull, carryZ = 0ull;
    for (unsigned long long base = 0ull; base < nTiles; base += (unsigned long long)FT_SLICE_SCAN_BLOCK * FT_SLICE_SCAN_ITEMS) {
        const unsigned long long first = base + (unsigned long long)threadIdx.x * FT_SLICE_SCAN_ITEMS;
        uint32_t vx[FT_SLICE_SCAN_ITEMS], vy[FT_SLICE_SCAN_ITEMS];
        unsigned long long sx = 0ull, sy = 0ull, sz = 0ull;
#pragma unroll
        for (int r = 0; r < FT_SLICE_SCAN_ITEMS; ++r) {
            const bool in = first + r < nTiles;
            vx[r] = in ? x[first + r] : 0u; vy[r] = in ? y[first + r] : 0u;
            sx += vx[r]; sy += vy[r]; sz += in ? z[first + r] : 0u;
        }
        unsigned long long ix = sx, iy = sy;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long px = __shfl_up(ix, off, 64), py = __shfl_up(iy, off, 64);
            if (lane >= (uint32_t)off) { ix += px; iy += py; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sz += __shfl_down(sz, off, 64);
        __syncthreads();                                               // the previous round's readers of wx / wy / wz are done
        if (lane == 63u) { wx[wave] = ix; wy[wave] = iy; }
        if (lane == 0u) wz[wave] = sz;
        __syncthreads();
        unsigned long long beforeX = carryX, beforeY = carryY;
        for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
            if (w < wave) { beforeX += wx[w]; beforeY += wy[w]; }
            carryX += wx[w]; carryY += wy[w]; carryZ += wz[w];
        }
        unsigned long long ex = beforeX + ix - sx, ey = beforeY + iy - sy;
#pragma unroll
        for (int r = 0; r < FT_SLICE_SCAN_ITEMS; ++r) {
            if (first + r < nTiles) { x[first + r] = (uint32_t)ex; y[first + r] = (uint32_t)ey; }
            ex += vx[r]; ey += vy[r];
        }
    }
    if (threadIdx.x == 0u) { totals[0] = carryX; totals[1] = carryY; totals[2] = carryZ; }
}
__global__ __launch_bounds__(FT_SLICE_SCAN_BLOCK) void ft_slice_scan_kernel(FtSliceArgs a) { ft_slice_scan(a.tileA, a.tileB, a.tileC, a.nTiles, a.totals); }
__global__ __launch_bounds__(FT_SLICE_SCAN_BLOCK) void ft_slice_vscan_kernel(FtSliceArgs a) { ft_slice_scan(a.vtA, a.vtB, a.vtC, a.nVTiles, a.vtotals); }

// the sum of tile `tile` from the scanned prefixes
__device__ __forceinline__ uint32_t ft_slice_tile_sum(const uint32_t* prefix, uint32_t tile, uint32_t nTiles, uint32_t total) {
    return (tile + 1u < nTiles ? prefix[tile + 1u] : total) - prefix[tile];
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_slice_emit_kernel(FtSliceArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    const FtSlicePlane p = ft_slice_plane(a);
    const uint32_t u = (a.axis + 1u) % 3u, v = (a.axis + 2u) % 3u;
    for (uint32_t tile = blockIdx.x; tile < a.nTiles; tile += gridDim.x) {
        const unsigned long long q64 = (unsigned long long)tile * TILE + threadIdx.x;
        const bool live = q64 < a.n;
        const uint32_t q = (uint32_t)q64, tileBase = a.tileA[tile];
        if (ft_slice_tile_sum(a.tileA, tile, a.nTiles, a.nV) == 0u) {   // nothing owned here (the whole workgroup agrees): only the index
            if (live) a.vbase[q] = tileBase;
            continue;
        }
        const uint32_t own = live ? a.mask[q] : 0u;
        const uint32_t at = tileBase + ft_slice_block_exclusive((uint32_t)__popc(own), lds);
        if (!live) continue;
        a.vbase[q] = at;
        if (!own) continue;
        const uint32_t k = q % a.nz, ij = q / a.nz, j = ij % a.ny, i = ij / a.ny;
        const uint32_t idx[3] = {i, j, k};
        const float s0 = ft_slice_signed(a, q);
        float p0[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) p0[ax] = a.origin[ax] + (float)idx[ax] * a.step[ax];
        uint32_t rank = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 3u; ++b) {                            // ascending e
            if (!((own >> b) & 1u)) continue;
            const uint32_t dd = b == 2u ? 3u : ((b == 1u) != p.swapUV ? 2u : 1u);
            const float s1 = ft_slice_signed(a, ft_slice_corner_at(p, q, dd));
            const float t = s0 / (s0 - s1);                            // from the owner towards the far end
            uint32_t d[3];
#pragma unroll
            for (uint32_t ax = 0; ax < 3u; ++ax) d[ax] = (ax == u ? dd >> 1 : 0u) + (ax == v ? dd & 1u : 0u);
            const uint32_t vtx = at + rank;
            ++rank;
            if (vtx >= a.nV) continue;
            float* out = a.vpos + 3 * (size_t)vtx;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float p1 = a.origin[ax] + (float)(idx[ax] + d[ax]) * a.step[ax];
                out[ax] = p0[ax] + t * (p1 - p0[ax]);
            }
            a.vslice[vtx] = ft_slice_pick(i, j, k, a.axis);
        }
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_slice_link_kernel(FtSliceArgs a) {
    const FtSlicePlane p = ft_slice_plane(a);
    for (uint32_t tile = blockIdx.x; tile < a.nTiles; tile += gridDim.x) {
        if (ft_slice_tile_sum(a.tileB, tile, a.nTiles, (uint32_t)a.totals[1]) == 0u) continue;
        const unsigned long long q64 = (unsigned long long)tile * TILE + threadIdx.x;
        if (q64 >= a.n) continue;
        const uint32_t q = (uint32_t)q64;
        const FtSliceCorners r = ft_slice_classify(a, p, q);
        if (!r.cell) continue;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t m = ft_slice_case(r, t);
            if (!ft_slice_case_segments(m)) continue;
            const uint32_t word = FT_SLICE_TABLE.e[t][m];
            uint32_t end[2];
#pragma unroll
            for (uint32_t side = 0; side < 2u; ++side) {
                const uint32_t slot = (word >> (1u + 4u * side)) & 15u, bit = ft_slice_bit(p, slot & 3u);
                const size_t owner = ft_slice_corner_at(p, q, slot >> 2);
                end[side] = a.vbase[owner] + (uint32_t)__popc((uint32_t)a.mask[owner] & ((1u << bit) - 1u));
            }
            if (end[0] >= a.nV || end[1] >= a.nV) continue;
            a.next[end[0]] = end[1];
            a.prev[end[1]] = end[0];
        }
    }
}

// ---- the chains: one lane per vertex, grid-stride -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT_SLICE_FLAT_BLOCK) void ft_slice_lead_kernel(FtSliceArgs a) {
    for (unsigned long long v64 = (unsigned long long)blockIdx.x * FT_SLICE_FLAT_BLOCK + threadIdx.x; v64 < a.nV; v64 += (unsigned long long)gridDim.x * FT_SLICE_FLAT_BLOCK) {
        const uint32_t v = (uint32_t)v64, pv = a.prev[v];
        const bool head = pv == FT_SLICE_NONE;
        a.from.anc[v] = head ? (v | FT_SLICE_DONE) : pv;
        a.from.hops[v] = head ? 0u : 1u;
        a.from.low[v] = v;
    }
}

__global__ __launch_bounds__(FT_SLICE_FLAT_BLOCK) void ft_slice_jump_kernel(FtSliceArgs a) {
    for (unsigned long long v64 = (unsigned long long)blockIdx.x * FT_SLICE_FLAT_BLOCK + threadIdx.x; v64 < a.nV; v64 += (unsigned long long)gridDim.x * FT_SLICE_FLAT_BLOCK) {
        const uint32_t v = (uint32_t)v64;
        uint32_t anc = a.from.anc[v], hops = a.from.hops[v], low = a.from.low[v];
        if (!(anc & FT_SLICE_DONE) && anc < a.nV) {
            const uint32_t low2 = a.from.low[anc];
            hops += a.from.hops[anc];
            low = low2 < low ? low2 : low;
            anc = a.from.anc[anc];
        }
        a.to.anc[v] = anc; a.to.hops[v] = hops; a.to.low[v] = low;
    }
}

__global__ __launch_bounds__(FT_SLICE_FLAT_BLOCK) void ft_slice_cut_kernel(FtSliceArgs a) {
    for (unsigned long long v64 = (unsigned long long)blockIdx.x * FT_SLICE_FLAT_BLOCK + threadIdx.x; v64 < a.nV; v64 += (unsigned long long)gridDim.x * FT_SLICE_FLAT_BLOCK) {
        const uint32_t v = (uint32_t)v64;
        const bool open = (a.from.anc[v] & FT_SLICE_DONE) != 0u;
        a.cyc[v] = open ? 0u : 1u;
        if (open) continue;                                            // (head, rank) already
        const bool leader = a.from.low[v] == v;                        // the smallest vertex of its cycle: the cut is in front of it
        a.from.anc[v] = leader ? (v | FT_SLICE_DONE) : a.prev[v];
        a.from.hops[v] = leader ? 0u : 1u;
    }
}

__global__ __launch_bounds__(FT_SLICE_FLAT_BLOCK) void ft_slice_tail_kernel(FtSliceArgs a) {
    for (unsigned long long v64 = (unsigned long long)blockIdx.x * FT_SLICE_FLAT_BLOCK + threadIdx.x; v64 < a.nV; v64 += (unsigned long long)gridDim.x * FT_SLICE_FLAT_BLOCK) {
        const uint32_t v = (uint32_t)v64, nv = a.next[v];
        if (nv == FT_SLICE_NONE && a.prev[v] == FT_SLICE_NONE) continue;        // no segment uses it
        const uint32_t head = a.from.anc[v] & ~FT_SLICE_DONE;
        if ((nv == FT_SLICE_NONE || nv == head) && head < a.nV) a.len[head] = a.from.hops[v] + 1u;
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_slice_heads_kernel(FtSliceArgs a) {
    __shared__ uint32_t red[3 * (TILE / 64)];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x) {
        const unsigned long long v64 = (unsigned long long)tile * TILE + threadIdx.x;
        uint32_t heads = 0u, points = 0u, closed = 0u;
        if (v64 < a.nV) {
            points = a.len[v64];
            heads = points ? 1u : 0u;
            closed = (points && a.cyc[v64]) ? 1u : 0u;
        }
        ft_slice_tile_sums<TILE>(heads, points, closed, red, tile, a.vtA, a.vtB, a.vtC);
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_slice_records_kernel(FtSliceArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x) {
        if (ft_slice_tile_sum(a.vtA, tile, a.nVTiles, a.nL) == 0u) continue;       // the whole workgroup agrees
        const unsigned long long v64 = (unsigned long long)tile * TILE + threadIdx.x;
        const uint32_t points = v64 < a.nV ? a.len[v64] : 0u;
        const uint32_t line = a.vtA[tile] + ft_slice_block_exclusive(points ? 1u : 0u, lds);
        const uint32_t first = a.vtB[tile] + ft_slice_block_exclusive(points, lds);
        if (!points) continue;
        a.off[v64] = first;
        if (line >= a.nL) continue;
        int32_t* out = a.polylines + 4 * (size_t)line;
        out[0] = (int32_t)first; out[1] = (int32_t)points; out[2] = (int32_t)a.vslice[v64]; out[3] = a.cyc[v64] ? 1 : 0;
    }
}

__global__ __launch_bounds__(FT_SLICE_FLAT_BLOCK) void ft_slice_scatter_kernel(FtSliceArgs a) {
    for (unsigned long long v64 = (unsigned long long)blockIdx.x * FT_SLICE_FLAT_BLOCK + threadIdx.x; v64 < a.nV; v64 += (unsigned long long)gridDim.x * FT_SLICE_FLAT_BLOCK) {
        const uint32_t v = (uint32_t)v64;
        if (a.next[v] == FT_SLICE_NONE && a.prev[v] == FT_SLICE_NONE) continue;
        const uint32_t head = a.from.anc[v] & ~FT_SLICE_DONE;
        if (head >= a.nV) continue;
        const unsigned long long at = (unsigned long long)a.off[head] + a.from.hops[v];
        if (at >= a.nP) continue;
        const float* in = a.vpos + 3 * (size_t)v;
        float* out = a.points + 3 * (size_t)at;
        out[0] = in[0]; out[1] = in[1]; out[2] = in[2];
    }
}

template <int TILE> const void* ft_slice_kernel_of(int kernel) {
    switch (kernel) {
        case FT_SLICE_K_COUNT: return (const void*)ft_slice_count_kernel<TILE>;
        case FT_SLICE_K_EMIT: return (const void*)ft_slice_emit_kernel<TILE>;
        case FT_SLICE_K_LINK: return (const void*)ft_slice_link_kernel<TILE>;
        case FT_SLICE_K_HEADS: return (const void*)ft_slice_heads_kernel<TILE>;
        case FT_SLICE_K_RECORDS: return (const void*)ft_slice_records_kernel<TILE>;
    }
    return nullptr;
}
const void* ft_slice_kernel(int kernel, uint32_t tile) {
    switch (kernel) {
        case FT_SLICE_K_SCAN: return (const void*)ft_slice_scan_kernel;
        case FT_SLICE_K_VSCAN: return (const void*)ft_slice_vscan_kernel;
        case FT_SLICE_K_LEAD: return (const void*)ft_slice_lead_kernel;
        case FT_SLICE_K_JUMP: return (const void*)ft_slice_jump_kernel;
        case FT_SLICE_K_CUT: return (const void*)ft_slice_cut_kernel;
        case FT_SLICE_K_TAIL: return (const void*)ft_slice_tail_kernel;
        case FT_SLICE_K_SCATTER: return (const void*)ft_slice_scatter_kernel;
    }
    switch (tile) {
        case 128u: return ft_slice_kernel_of<128>(kernel);
        case 256u: return ft_slice_kernel_of<256>(kernel);
        case 512u: return ft_slice_kernel_of<512>(kernel);
        case 1024u: return ft_slice_kernel_of<1024>(kernel);
    }
    return nullptr;
}

}  // namespace

extern "C" unsigned ft_slice_block(int kernel, uint32_t tile) {
    switch (kernel) {
        case FT_SLICE_K_SCAN: case FT_SLICE_K_VSCAN: return FT_SLICE_SCAN_BLOCK;
        case FT_SLICE_K_LEAD: case FT_SLICE_K_JUMP: case FT_SLICE_K_CUT: case FT_SLICE_K_TAIL: case FT_SLICE_K_SCATTER: return FT_SLICE_FLAT_BLOCK;
    }
    return tile;
}
extern "C" hipError_t ft_launch_slice(int kernel, const FtSliceArgs* a, unsigned blocks, hipStream_t st) {
    const void* k = ft_slice_kernel(kernel, a->tile);
    if (!k) return hipErrorInvalidDeviceFunction;
    FtSliceArgs args = *a;
    void* kp[] = {&args};
    const bool scan = kernel == FT_SLICE_K_SCAN || kernel == FT_SLICE_K_VSCAN;
    return hipLaunchKernel(k, dim3(scan ? 1u : blocks), dim3(ft_slice_block(kernel, a->tile)), kp, 0, st);
}
extern "C" hipError_t ft_launch_slice_jumps(const FtSliceArgs* a, unsigned rounds, unsigned blocks, hipStream_t st) {
    FtSliceArgs args = *a;
    for (unsigned r = 0; r < rounds; ++r) {
        void* kp[] = {&args};
        const hipError_t e = hipLaunchKernel((const void*)ft_slice_jump_kernel, dim3(blocks), dim3(FT_SLICE_FLAT_BLOCK), kp, 0, st);
        if (e != hipSuccess) return e;
        const FtSliceState t = args.from; args.from = args.to; args.to = t;
    }
    return hipSuccess;
}
extern "C" hipError_t ft_slice_occupancy(int kernel, uint32_t tile, int* blocksPerCU) {
    const void* k = ft_slice_kernel(kernel, tile);
    if (!k) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocksPerCU, k, (int)ft_slice_block(kernel, tile), 0);
}
extern "C" const uint32_t* ft_slice_table(void) { return &FT_SLICE_TABLE_HOST.e[0][0]; }
