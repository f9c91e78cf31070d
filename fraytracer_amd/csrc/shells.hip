// shells.hip — the shells (connected components) of an indexed triangle mesh, their records and the selection of some of them, on the device
// (include/fraytracer_hip.h "Shells" is the rule; this file is its device side; ft_shells.h says which algorithm and why it ends).  Integers only.
//   init, degree, sums, scan, offsets, fill      the vertex -> triangle incidence lists: count, scan, fill (the fill order is arbitrary: only the
//                                                existence of a reverse side is ever asked of a list)
//   shortcut, hook, apply, stagnant, apply, shortcut   one iteration of the labelling; every launch reads only what earlier launches wrote
//   verify                                       the stop decision, a launch of its own
//   first, sums, scan, number                    per root its smallest member; the members that are one, counted in vertex order: the rule's numbering
//   label vertices, label triangles, summary     labels, the records' counts (one atomicAdd per wave and shell), border edges, totals
//   keep sums, scan, keep vertices / triangles   the selection: ranks among the kept by prefix sums, so old order is kept
// Atomics: atomicMin, atomicAdd and atomicOr on integers at agent scope; every result is independent of the order they arrive in.  No kernel waits
// for another workgroup.  Every index read back from an array is checked against its bound before it is used.
#include <hip/hip_runtime.h>

#include "ft_shells.h"

namespace {

// ---- what a lane knows about its triangle ----------------------------------------------------------------------------------------------------------
struct FtShellsTri { uint32_t i0, i1, i2; bool ok; };                  // ok: the three indices are below nV and pairwise different
__device__ __forceinline__ FtShellsTri ft_shells_tri(const FtShellsArgs& a, uint32_t t) {
    const int32_t* p = a.triangles + 3 * (size_t)t;
    FtShellsTri r{(uint32_t)p[0], (uint32_t)p[1], (uint32_t)p[2], false};       // a negative index is a large one
    r.ok = r.i0 < a.nV && r.i1 < a.nV && r.i2 < a.nV && r.i0 != r.i1 && r.i1 != r.i2 && r.i0 != r.i2;
    return r;
}
// does the triangle have the directed side x -> y
__device__ __forceinline__ bool ft_shells_has_side(const FtShellsTri& u, uint32_t x, uint32_t y) {
    return (u.i0 == x && u.i1 == y) || (u.i1 == x && u.i2 == y) || (u.i2 == x && u.i0 == y);
}

// the grid-stride loop of the untiled kernels, whole waves at a time: `item` may be at or beyond n (the lane then only takes part in the wave's shuffles)
#define FT_SHELLS_FOR(item, n)                                                                                                               \
    for (unsigned long long item##Base = (unsigned long long)blockIdx.x * FT_SHELLS_FLAT_BLOCK; item##Base < (n);                            \
         item##Base += (unsigned long long)gridDim.x * FT_SHELLS_FLAT_BLOCK)                                                                 \
        for (unsigned long long item = item##Base + threadIdx.x, item##Once = 1; item##Once; item##Once = 0)

// records[4 * key + field] += the wave's sum of `amount` over the lanes with that key: one atomicAdd per wave and key.  Every lane of the wave calls it
__device__ __forceinline__ void ft_shells_add(const FtShellsArgs& a, uint32_t field, uint32_t key, uint32_t amount) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(amount != 0u && key < a.nS);
    while (todo) {                                                     // the same for the whole wave
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t k0 = (uint32_t)__shfl((int)key, leader, 64);
        const bool mine = amount != 0u && key == k0;
        uint32_t sum = mine ? amount : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += (uint32_t)__shfl_xor((int)sum, off, 64);
        if (lane == (uint32_t)leader) atomicAdd(reinterpret_cast<unsigned int*>(a.records) + 4 * (size_t)k0 + field, sum);
        todo &= ~__ballot(mine);
    }
}

// ---- sums and scans across a workgroup (the slicer's pattern) ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ft_shells_block_exclusive(uint32_t v, uint32_t* lds) {
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
template <int TILE> __device__ __forceinline__ void ft_shells_tile_sums(uint32_t x, uint32_t z, uint32_t* red, uint32_t tile, uint32_t* ox, uint32_t* oz) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { x += __shfl_down(x, off, 64); z += __shfl_down(z, off, 64); }
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) { const uint32_t w = threadIdx.x >> 6; red[2u * w] = x; red[2u * w + 1u] = z; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sx = 0u, sz = 0u;
        for (int w = 0; w < TILE / 64; ++w) { sx += red[2 * w]; sz += red[2 * w + 1]; }
        ox[tile] = sx; oz[tile] = sz;
    }
}
__device__ __forceinline__ uint32_t ft_shells_tile_sum(const uint32_t* prefix, uint32_t tile, uint32_t nTiles, uint32_t total) {
    return (tile + 1u < nTiles ? prefix[tile + 1u] : total) - prefix[tile];
}

// One workgroup: the first a.scanTiles words of tileA scanned in place (mod 2^32: the totals are below 2^31 by the entry's checks), tileC only summed.
__global__ __launch_bounds__(FT_SHELLS_SCAN_BLOCK) void ft_shells_scan_kernel(FtShellsArgs a) {
    constexpr int WAVES = FT_SHELLS_SCAN_BLOCK / 64;
    __shared__ unsigned long long wx[WAVES], wz[WAVES];
    const uint32_t nTiles = a.scanTiles;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carryX = 0ull, carryZ = 0ull;
    for (unsigned long long base = 0ull; base < nTiles; base += (unsigned long long)FT_SHELLS_SCAN_BLOCK * FT_SHELLS_SCAN_ITEMS) {
        const unsigned long long first = base + (unsigned long long)threadIdx.x * FT_SHELLS_SCAN_ITEMS;
        uint32_t vx[FT_SHELLS_SCAN_ITEMS];
        unsigned long long sx = 0ull, sz = 0ull;
#pragma unroll
        for (int r = 0; r < FT_SHELLS_SCAN_ITEMS; ++r) {
            const bool in = first + r < nTiles;
            vx[r] = in ? a.tileA[first + r] : 0u;
            sx += vx[r]; sz += in ? a.tileC[first + r] : 0u;
        }
        unsigned long long ix = sx;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned long long px = __shfl_up(ix, off, 64); if (lane >= (uint32_t)off) ix += px; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sz += __shfl_down(sz, off, 64);
        __syncthreads();                                               // the previous round's readers of wx / wz are done
        if (lane == 63u) wx[wave] = ix;
        if (lane == 0u) wz[wave] = sz;
        __syncthreads();
        unsigned long long beforeX = carryX;
        for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
            if (w < wave) beforeX += wx[w];
            carryX += wx[w]; carryZ += wz[w];
        }
        unsigned long long ex = beforeX + ix - sx;
#pragma unroll
        for (int r = 0; r < FT_SHELLS_SCAN_ITEMS; ++r) {
            if (first + r < nTiles) a.tileA[first + r] = (uint32_t)ex;
            ex += vx[r];
        }
    }
    if (threadIdx.x == 0u) { a.totals[0] = carryX; a.totals[1] = carryZ; }
}

// ---- the incidence lists ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_init_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(v, a.nV) {
        if (v >= a.nV) continue;
        a.parent[v] = (uint32_t)v; a.parent2[v] = (uint32_t)v; a.stamp[v] = 0u; a.hook[v] = FT_SHELLS_NONE; a.first[v] = FT_SHELLS_NONE;
        a.degree[v] = 0u; a.cursor[v] = 0u;
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_degree_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(t, a.nT) {
        if (t >= a.nT) continue;
        const FtShellsTri r = ft_shells_tri(a, (uint32_t)t);
        if (!r.ok) { atomicOr(a.flags, FT_SHELLS_FLAG_INVALID); continue; }     // nothing is indexed with it, here or later
        atomicAdd(a.degree + r.i0, 1u); atomicAdd(a.degree + r.i1, 1u); atomicAdd(a.degree + r.i2, 1u);
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_degree_sums_kernel(FtShellsArgs a) {
    __shared__ uint32_t red[2 * (TILE / 64)];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x) {
        const unsigned long long v = (unsigned long long)tile * TILE + threadIdx.x;
        const uint32_t d = v < a.nV ? a.degree[v] : 0u;
        ft_shells_tile_sums<TILE>(d, d ? 1u : 0u, red, tile, a.tileA, a.tileC);
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_offsets_kernel(FtShellsArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x) {
        const unsigned long long v = (unsigned long long)tile * TILE + threadIdx.x;
        const uint32_t at = a.tileA[tile] + ft_shells_block_exclusive(v < a.nV ? a.degree[v] : 0u, lds);
        if (v < a.nV) a.offset[v] = at;
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_fill_kernel(FtShellsArgs a) {
    const unsigned long long room = 3ull * a.nT;
    FT_SHELLS_FOR(t, a.nT) {
        if (t >= a.nT) continue;
        const FtShellsTri r = ft_shells_tri(a, (uint32_t)t);
        if (!r.ok) continue;
        const uint32_t idx[3] = {r.i0, r.i1, r.i2};
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const uint32_t rank = atomicAdd(a.cursor + idx[x], 1u);
            const unsigned long long slot = (unsigned long long)a.offset[idx[x]] + rank;
            if (rank < a.degree[idx[x]] && slot < room) a.incidence[slot] = (uint32_t)t;
        }
    }
}

// ---- one iteration --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_shortcut_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(v, a.nV) {
        if (v >= a.nV) continue;
        const uint32_t p = a.parent[v];
        const uint32_t g = p < a.nV ? a.parent[p] : p;
        a.parent2[v] = g;
        if (g != p && g < a.nV) a.stamp[g] = a.iteration;             // every writer of a word writes the same value
    }
}

__device__ __forceinline__ void ft_shells_hook_side(const FtShellsArgs& a, uint32_t i, uint32_t j) {
    const uint32_t pi = a.parent2[i], pj = a.parent2[j];
    if (pi == a.parent[i] && pj < pi && pi < a.nV) { atomicMin(a.hook + pi, pj); a.stamp[pj] = a.iteration; }
}
__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_hook_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(t, a.nT) {
        if (t >= a.nT) continue;
        const FtShellsTri r = ft_shells_tri(a, (uint32_t)t);
        if (!r.ok) continue;
        ft_shells_hook_side(a, r.i0, r.i1); ft_shells_hook_side(a, r.i1, r.i0);
        ft_shells_hook_side(a, r.i1, r.i2); ft_shells_hook_side(a, r.i2, r.i1);
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_apply_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(v, a.nV) {
        if (v >= a.nV) continue;
        const uint32_t h = a.hook[v];
        if (h == FT_SHELLS_NONE) continue;
        a.hook[v] = FT_SHELLS_NONE;
        if (h < a.nV) a.parent2[v] = h;
    }
}

__device__ __forceinline__ void ft_shells_stagnant_side(const FtShellsArgs& a, uint32_t i, uint32_t j) {
    const uint32_t r = a.parent2[i];
    if (r >= a.nV || a.parent2[r] != r || a.stamp[r] >= a.iteration) return;
    const uint32_t pj = a.parent2[j];
    if (pj != r) atomicMin(a.hook + r, pj);
}
__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_stagnant_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(t, a.nT) {
        if (t >= a.nT) continue;
        const FtShellsTri r = ft_shells_tri(a, (uint32_t)t);
        if (!r.ok) continue;
        ft_shells_stagnant_side(a, r.i0, r.i1); ft_shells_stagnant_side(a, r.i1, r.i0);
        ft_shells_stagnant_side(a, r.i1, r.i2); ft_shells_stagnant_side(a, r.i2, r.i1);
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_shortcut2_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(v, a.nV) {
        if (v >= a.nV) continue;
        const uint32_t p = a.parent2[v];
        a.parent[v] = p < a.nV ? a.parent2[p] : p;
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_verify_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(t, a.nT) {
        if (t >= a.nT) continue;
        const FtShellsTri r = ft_shells_tri(a, (uint32_t)t);
        if (!r.ok) continue;
        const uint32_t l0 = a.parent[r.i0], l1 = a.parent[r.i1], l2 = a.parent[r.i2];
        const bool done = l0 == l1 && l1 == l2 && l0 < a.nV && a.parent[l0] == l0;
        if (!done) atomicOr(a.flags + a.flagWord, FT_SHELLS_FLAG_OPEN);
    }
}

// ---- numbering, labels, records -----------------------------------------------------------------------------------------------------------------
// One atomicMin per wave and root instead of one per vertex (a shell of a million vertices would queue them all on one word): the wave's lanes are
// consecutive vertices, so the first lane with a root holds the wave's smallest member of it.  A lane whose plain load of first[root] is already at or
// below its vertex has nothing to add: a stale load only shows a larger value than the word holds, never a smaller one.
__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_first_kernel(FtShellsArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    FT_SHELLS_FOR(v, a.nV) {
        uint32_t root = FT_SHELLS_NONE;
        if (v < a.nV && a.degree[v]) { root = a.parent[v]; if (root >= a.nV || a.first[root] <= (uint32_t)v) root = FT_SHELLS_NONE; }
        unsigned long long todo = __ballot(root != FT_SHELLS_NONE);
        while (todo) {                                                 // the same for the whole wave
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t r0 = (uint32_t)__shfl((int)root, leader, 64);
            if (lane == (uint32_t)leader) atomicMin(a.first + r0, (uint32_t)v);
            todo &= ~__ballot(root == r0);
        }
    }
}

// is v its shell's smallest vertex
__device__ __forceinline__ bool ft_shells_leader(const FtShellsArgs& a, unsigned long long v) {
    if (v >= a.nV || !a.degree[v]) return false;
    const uint32_t root = a.parent[v];
    return root < a.nV && a.first[root] == (uint32_t)v;
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_leader_sums_kernel(FtShellsArgs a) {
    __shared__ uint32_t red[2 * (TILE / 64)];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x) {
        const unsigned long long v = (unsigned long long)tile * TILE + threadIdx.x;
        ft_shells_tile_sums<TILE>(ft_shells_leader(a, v) ? 1u : 0u, (v < a.nV && a.degree[v]) ? 1u : 0u, red, tile, a.tileA, a.tileC);      // leaders; used vertices
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_number_kernel(FtShellsArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x) {
        if (ft_shells_tile_sum(a.tileA, tile, a.nVTiles, (uint32_t)a.totals[0]) == 0u) continue;      // the whole workgroup agrees; the scan's total: the shells
        const unsigned long long v = (unsigned long long)tile * TILE + threadIdx.x;
        const bool leader = ft_shells_leader(a, v);
        const uint32_t shell = a.tileA[tile] + ft_shells_block_exclusive(leader ? 1u : 0u, lds);
        if (!leader || shell >= a.nS) continue;
        a.hook[a.parent[v]] = shell;                                   // ft_shells_leader checked the root
        int32_t* out = a.records + 4 * (size_t)shell;
        out[0] = (int32_t)v; out[1] = 0; out[2] = 0; out[3] = 0;
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_label_vertices_kernel(FtShellsArgs a) {
    FT_SHELLS_FOR(v, a.nV) {
        uint32_t shell = FT_SHELLS_NONE;
        if (v < a.nV) {
            if (a.degree[v]) { const uint32_t root = a.parent[v]; if (root < a.nV) shell = a.hook[root]; }
            if (shell >= a.nS) shell = FT_SHELLS_NONE;
            a.vertexShell[v] = (int32_t)shell;                         // FT_SHELLS_NONE is -1
        }
        ft_shells_add(a, 1u, shell, shell != FT_SHELLS_NONE ? 1u : 0u);
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_label_triangles_kernel(FtShellsArgs a) {
    const unsigned long long room = 3ull * a.nT;
    FT_SHELLS_FOR(t, a.nT) {
        uint32_t shell = FT_SHELLS_NONE, border = 0u;
        if (t < a.nT) {
            const FtShellsTri r = ft_shells_tri(a, (uint32_t)t);
            if (r.ok) {
                shell = (uint32_t)a.vertexShell[r.i0];
                if (shell >= a.nS) shell = FT_SHELLS_NONE;
                const uint32_t idx[4] = {r.i0, r.i1, r.i2, r.i0};
#pragma unroll
                for (int x = 0; x < 3; ++x) {                          // side from -> to: a border edge iff no triangle has to -> from
                    const uint32_t from = idx[x], to = idx[x + 1];
                    const uint32_t dFrom = a.degree[from], dTo = a.degree[to];
                    const uint32_t at = dFrom <= dTo ? from : to;      // such a triangle is in both lists: the shorter one is read
                    const uint32_t n = dFrom <= dTo ? dFrom : dTo;
                    const unsigned long long begin = a.offset[at];
                    bool found = false;
                    for (uint32_t k = 0; k < n && !found && begin + k < room; ++k) {
                        const uint32_t u = a.incidence[begin + k];
                        if (u >= a.nT) continue;
                        const FtShellsTri o = ft_shells_tri(a, u);
                        found = o.ok && ft_shells_has_side(o, to, from);
                    }
                    border += found ? 0u : 1u;
                }
            }
            a.triangleShell[t] = (int32_t)shell;
        }
        const bool live = shell != FT_SHELLS_NONE;
        ft_shells_add(a, 2u, shell, live ? 1u : 0u);
        ft_shells_add(a, 3u, shell, live ? border : 0u);
    }
}

__global__ __launch_bounds__(FT_SHELLS_FLAT_BLOCK) void ft_shells_summary_kernel(FtShellsArgs a) {
    const unsigned long long nS = a.totals[0] < a.nS ? a.totals[0] : a.nS;      // the shells the scan counted; a.nS is the room
    FT_SHELLS_FOR(s, nS) {
        unsigned long long closed = 0ull, border = 0ull;
        if (s < nS) { const uint32_t b = (uint32_t)a.records[4 * (size_t)s + 3]; border = b; closed = b ? 0ull : 1ull; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { closed += __shfl_down(closed, off, 64); border += __shfl_down(border, off, 64); }
        if ((threadIdx.x & 63u) == 0u) {
            if (closed) atomicAdd(a.totals + 2, closed);
            if (border) atomicAdd(a.totals + 3, border);
        }
    }
}

// ---- the selection --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ft_shells_kept(const FtShellsArgs& a, const int32_t* shellOf, unsigned long long item, unsigned long long n) {
    if (item >= n) return false;
    const uint32_t s = (uint32_t)shellOf[item];
    return s < a.nS && a.keep[s] != 0;
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_keep_vertex_sums_kernel(FtShellsArgs a) {
    __shared__ uint32_t red[2 * (TILE / 64)];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x)
        ft_shells_tile_sums<TILE>(ft_shells_kept(a, a.vertexShell, (unsigned long long)tile * TILE + threadIdx.x, a.nV) ? 1u : 0u, 0u, red, tile, a.tileA, a.tileC);
}
template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_keep_triangle_sums_kernel(FtShellsArgs a) {
    __shared__ uint32_t red[2 * (TILE / 64)];
    for (uint32_t tile = blockIdx.x; tile < a.nTTiles; tile += gridDim.x)
        ft_shells_tile_sums<TILE>(ft_shells_kept(a, a.triangleShell, (unsigned long long)tile * TILE + threadIdx.x, a.nT) ? 1u : 0u, 0u, red, tile, a.tileA, a.tileC);
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_keep_vertices_kernel(FtShellsArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nVTiles; tile += gridDim.x) {
        const unsigned long long v = (unsigned long long)tile * TILE + threadIdx.x;
        const bool kept = ft_shells_kept(a, a.vertexShell, v, a.nV);
        const uint32_t at = a.tileA[tile] + ft_shells_block_exclusive(kept ? 1u : 0u, lds);
        if (v >= a.nV) continue;
        a.remap[v] = kept ? at : FT_SHELLS_NONE;
        if (!kept || at >= a.nVOut) continue;
#pragma unroll
        for (int x = 0; x < 3; ++x) a.dstVertices[3 * (size_t)at + x] = a.srcVertices[3 * (size_t)v + x];
        if (a.srcNormals) {
#pragma unroll
            for (int x = 0; x < 3; ++x) a.dstNormals[3 * (size_t)at + x] = a.srcNormals[3 * (size_t)v + x];
        }
        if (a.srcMaterials) a.dstMaterials[at] = a.srcMaterials[v];
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_shells_keep_triangles_kernel(FtShellsArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nTTiles; tile += gridDim.x) {
        const unsigned long long t = (unsigned long long)tile * TILE + threadIdx.x;
        const bool kept = ft_shells_kept(a, a.triangleShell, t, a.nT);
        const uint32_t at = a.tileA[tile] + ft_shells_block_exclusive(kept ? 1u : 0u, lds);
        if (!kept || at >= a.nTOut) continue;
        const FtShellsTri r = ft_shells_tri(a, (uint32_t)t);
        if (!r.ok) continue;
        const uint32_t n0 = a.remap[r.i0], n1 = a.remap[r.i1], n2 = a.remap[r.i2];
        if (n0 >= a.nVOut || n1 >= a.nVOut || n2 >= a.nVOut) continue;
        int32_t* out = a.dstTriangles + 3 * (size_t)at;
        out[0] = (int32_t)n0; out[1] = (int32_t)n1; out[2] = (int32_t)n2;
    }
}

template <int TILE> const void* ft_shells_kernel_of(int kernel) {
    switch (kernel) {
        case FT_SHELLS_K_DEGREE_SUMS: return (const void*)ft_shells_degree_sums_kernel<TILE>;
        case FT_SHELLS_K_OFFSETS: return (const void*)ft_shells_offsets_kernel<TILE>;
        case FT_SHELLS_K_LEADER_SUMS: return (const void*)ft_shells_leader_sums_kernel<TILE>;
        case FT_SHELLS_K_NUMBER: return (const void*)ft_shells_number_kernel<TILE>;
        case FT_SHELLS_K_KEEP_VERTEX_SUMS: return (const void*)ft_shells_keep_vertex_sums_kernel<TILE>;
        case FT_SHELLS_K_KEEP_TRIANGLE_SUMS: return (const void*)ft_shells_keep_triangle_sums_kernel<TILE>;
        case FT_SHELLS_K_KEEP_VERTICES: return (const void*)ft_shells_keep_vertices_kernel<TILE>;
        case FT_SHELLS_K_KEEP_TRIANGLES: return (const void*)ft_shells_keep_triangles_kernel<TILE>;
    }
    return nullptr;
}
const void* ft_shells_kernel(int kernel, uint32_t tile) {
    switch (kernel) {
        case FT_SHELLS_K_INIT: return (const void*)ft_shells_init_kernel;
        case FT_SHELLS_K_DEGREE: return (const void*)ft_shells_degree_kernel;
        case FT_SHELLS_K_SCAN: return (const void*)ft_shells_scan_kernel;
        case FT_SHELLS_K_FILL: return (const void*)ft_shells_fill_kernel;
        case FT_SHELLS_K_SHORTCUT: return (const void*)ft_shells_shortcut_kernel;
        case FT_SHELLS_K_HOOK: return (const void*)ft_shells_hook_kernel;
        case FT_SHELLS_K_APPLY: return (const void*)ft_shells_apply_kernel;
        case FT_SHELLS_K_STAGNANT: return (const void*)ft_shells_stagnant_kernel;
        case FT_SHELLS_K_SHORTCUT2: return (const void*)ft_shells_shortcut2_kernel;
        case FT_SHELLS_K_VERIFY: return (const void*)ft_shells_verify_kernel;
        case FT_SHELLS_K_FIRST: return (const void*)ft_shells_first_kernel;
        case FT_SHELLS_K_LABEL_VERTICES: return (const void*)ft_shells_label_vertices_kernel;
        case FT_SHELLS_K_LABEL_TRIANGLES: return (const void*)ft_shells_label_triangles_kernel;
        case FT_SHELLS_K_SUMMARY: return (const void*)ft_shells_summary_kernel;
    }
    switch (tile) {
        case 128u: return ft_shells_kernel_of<128>(kernel);
        case 256u: return ft_shells_kernel_of<256>(kernel);
        case 512u: return ft_shells_kernel_of<512>(kernel);
        case 1024u: return ft_shells_kernel_of<1024>(kernel);
    }
    return nullptr;
}

bool ft_shells_tiled(int kernel) {
    switch (kernel) {
        case FT_SHELLS_K_DEGREE_SUMS: case FT_SHELLS_K_OFFSETS: case FT_SHELLS_K_LEADER_SUMS: case FT_SHELLS_K_NUMBER: case FT_SHELLS_K_KEEP_VERTEX_SUMS:
        case FT_SHELLS_K_KEEP_TRIANGLE_SUMS: case FT_SHELLS_K_KEEP_VERTICES: case FT_SHELLS_K_KEEP_TRIANGLES: return true;
    }
    return false;
}

hipError_t ft_shells_launch_one(int kernel, const FtShellsArgs& args, unsigned blocks, hipStream_t st) {
    const void* k = ft_shells_kernel(kernel, args.tile);
    if (!k) return hipErrorInvalidDeviceFunction;
    FtShellsArgs copy = args;
    void* kp[] = {&copy};
    return hipLaunchKernel(k, dim3(kernel == FT_SHELLS_K_SCAN ? 1u : blocks), dim3(ft_shells_block(kernel, args.tile)), kp, 0, st);
}

}  // namespace

extern "C" int ft_shells_domain(int kernel) {
    switch (kernel) {
        case FT_SHELLS_K_SCAN: return 3;
        case FT_SHELLS_K_SUMMARY: return 2;
        case FT_SHELLS_K_DEGREE: case FT_SHELLS_K_FILL: case FT_SHELLS_K_HOOK: case FT_SHELLS_K_STAGNANT: case FT_SHELLS_K_VERIFY: case FT_SHELLS_K_LABEL_TRIANGLES:
        case FT_SHELLS_K_KEEP_TRIANGLE_SUMS: case FT_SHELLS_K_KEEP_TRIANGLES: return 1;
    }
    return 0;
}
extern "C" unsigned ft_shells_block(int kernel, uint32_t tile) {
    if (kernel == FT_SHELLS_K_SCAN) return FT_SHELLS_SCAN_BLOCK;
    return ft_shells_tiled(kernel) ? tile : FT_SHELLS_FLAT_BLOCK;
}
extern "C" hipError_t ft_launch_shells(int kernel, const FtShellsArgs* a, unsigned blocks, hipStream_t st) { return ft_shells_launch_one(kernel, *a, blocks, st); }
extern "C" hipError_t ft_launch_shells_iterations(const FtShellsArgs* a, unsigned count, unsigned blocksV, unsigned blocksT, hipStream_t st) {
    static const int steps[6] = {FT_SHELLS_K_SHORTCUT, FT_SHELLS_K_HOOK, FT_SHELLS_K_APPLY, FT_SHELLS_K_STAGNANT, FT_SHELLS_K_APPLY, FT_SHELLS_K_SHORTCUT2};
    FtShellsArgs args = *a;
    for (unsigned r = 0; r < count; ++r, ++args.iteration) {
        for (int k : steps) {
            const hipError_t e = ft_shells_launch_one(k, args, ft_shells_domain(k) == 1 ? blocksT : blocksV, st);
            if (e != hipSuccess) return e;
        }
    }
    return ft_shells_launch_one(FT_SHELLS_K_VERIFY, args, blocksT, st);
}
extern "C" hipError_t ft_shells_occupancy(int kernel, uint32_t tile, int* blocksPerCU) {
    const void* k = ft_shells_kernel(kernel, tile);
    if (!k) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocksPerCU, k, (int)ft_shells_block(kernel, tile), 0);
}
extern "C" unsigned ft_shells_iteration_cap(uint64_t n) {
    unsigned k = 0;
    unsigned __int128 pow3 = 1, scaled = n < 1 ? 1 : n;               // the largest k with 3^k <= n 2^k
    while (pow3 * 3 <= scaled * 2) { pow3 *= 3; scaled *= 2; ++k; }
    return k + 2;
}
