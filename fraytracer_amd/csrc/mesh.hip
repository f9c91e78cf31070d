// mesh.hip — triangle meshes from a lattice of distances: marching tetrahedra on the Kuhn subdivision (include/fraytracer_hip.h "Meshing" is the
// rule; this file is its device side).  Four kernels, no atomics, so that vertex and triangle order are the rule's:
//   count      one lane per lattice point q (k contiguous across a wave): the 7-bit mask of the vertices q owns, the triangles and the skipped
//              tetrahedra of cell q; per tile of consecutive points (one workgroup's worth: FtMeshArgs.tile) the three sums
//   scan       one workgroup: exclusive prefix sums of the tile sums, the 64-bit totals the host reads after its one synchronisation
//   vertices   per point the index of its first vertex (vbase), and the vertices
//   triangles  per cell its triangles; the vertex on edge (q, e) is vbase[q] + popcount(mask[q] & ((1 << e) - 1))
// Built with -ffp-contract=off like every other object: each product, sum and quotient of the vertex rule is rounded on its own.
#include <hip/hip_runtime.h>

#include "ft_mesh.h"

namespace {

// ---- the orientation table, from the integer corner offsets -----------------------------------------------------------------------------------
// Corner code c = 4 di + 2 dj + dk.  Tetrahedron t (the permutations of the axes in lexicographic order) has the corners 0, c1(t), c2(t), 7.
__host__ __device__ constexpr uint32_t ft_mesh_c1(int t) { return (0x112244u >> (4 * t)) & 7u; }      // 4, 4, 2, 2, 1, 1
__host__ __device__ constexpr uint32_t ft_mesh_c2(int t) { return (0x353656u >> (4 * t)) & 7u; }      // 6, 5, 6, 3, 5, 3

struct FtMeshTable { unsigned long long e[6][16]; };

constexpr int ft_mesh_det(const int a[3], const int b[3], const int c[3]) {
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

constexpr FtMeshTable ft_mesh_make_table() {
    FtMeshTable T{};
    for (int t = 0; t < 6; ++t) {
        const int C[4] = {0, (int)ft_mesh_c1(t), (int)ft_mesh_c2(t), 7};
        int P[4][3] = {};
        for (int x = 0; x < 4; ++x) { P[x][0] = (C[x] >> 2) & 1; P[x][1] = (C[x] >> 1) & 1; P[x][2] = C[x] & 1; }
        for (int m = 0; m < 16; ++m) {                                 // bit x of m: corner x is inside
            int A[4] = {}, B[4] = {}, na = 0, nb = 0;
            for (int x = 0; x < 4; ++x) { if ((m >> x) & 1) A[na++] = x; else B[nb++] = x; }
            int cyc[4][2] = {}, n = 0;                                 // crossing edges as corner pairs, counter-clockwise seen from the outside
            if (na == 1 || na == 3) {
                const int apex = na == 1 ? A[0] : B[0];
                const int* base = na == 1 ? B : A;
                int d[3][3] = {};
                for (int r = 0; r < 3; ++r) for (int ax = 0; ax < 3; ++ax) d[r][ax] = P[base[r]][ax] - P[apex][ax];
                const int det = ft_mesh_det(d[0], d[1], d[2]);
                // vertices at apex + t_r d[r], t_r > 0: the normal of (v0, v1, v2) has the sign of det along v0 - apex; it points away from an inside
                // apex and towards an outside one
                const bool swap = na == 1 ? det < 0 : det > 0;
                const int order[3] = {0, swap ? 2 : 1, swap ? 1 : 2};
                for (int r = 0; r < 3; ++r) { cyc[r][0] = apex; cyc[r][1] = base[order[r]]; }
                n = 3;
            } else if (na == 2) {
                const int a1 = A[0], a2 = A[1], b1 = B[0], b2 = B[1];
                int u[3] = {}, v[3] = {}, out[3] = {};
                for (int ax = 0; ax < 3; ++ax) { u[ax] = P[b2][ax] - P[b1][ax]; v[ax] = P[a2][ax] - P[a1][ax]; out[ax] = P[b1][ax] + P[b2][ax] - P[a1][ax] - P[a2][ax]; }
                // the cycle (a1 b1, a1 b2, a2 b2, a2 b1) at the edges' midpoints is a parallelogram with normal u x v
                const bool rev = ft_mesh_det(u, v, out) < 0;
                const int q[4][2] = {{a1, b1}, {a1, b2}, {a2, b2}, {a2, b1}};
                for (int r = 0; r < 4; ++r) { cyc[r][0] = q[rev ? 3 - r : r][0]; cyc[r][1] = q[rev ? 3 - r : r][1]; }
                n = 4;
            }
            if (n == 0) continue;
            // slot (owner corner << 3) | e; in a lattice with every count >= 2 the corners' linear indices are ordered like their codes, so the slot
            // orders the vertices of one cell as their indices do
            int slot[4] = {}, first = 0;
            for (int r = 0; r < n; ++r) {
                const int lo = cyc[r][0] < cyc[r][1] ? cyc[r][0] : cyc[r][1], hi = cyc[r][0] < cyc[r][1] ? cyc[r][1] : cyc[r][0];
                slot[r] = (C[lo] << 3) | ((C[hi] ^ C[lo]) - 1);
                if (slot[r] < slot[first]) first = r;
            }
            int s[4] = {};
            for (int r = 0; r < n; ++r) s[r] = slot[(first + r) % n];
            const int tri[6] = {s[0], s[1], s[2], s[0], s[2], s[3]};
            unsigned long long word = n == 3 ? 1ull : 2ull;
            for (int r = 0; r < (n == 3 ? 3 : 6); ++r) word |= (unsigned long long)tri[r] << (2 + 6 * r);
            T.e[t][m] = word;
        }
    }
    return T;
}

constexpr FtMeshTable FT_MESH_TABLE_HOST = ft_mesh_make_table();
__constant__ FtMeshTable FT_MESH_TABLE = ft_mesh_make_table();

// ---- what a lane knows about its point ------------------------------------------------------------------------------------------------------
struct FtMeshCorners { uint32_t in8, fin8; bool cell; };               // bit c: corner c of cell q is inside / is a lattice point with a finite value

__device__ __forceinline__ float ft_mesh_signed(const FtMeshArgs& a, size_t q) { return a.values[q] - a.iso; }
__device__ __forceinline__ bool ft_mesh_finite(float s) { return __builtin_fabsf(s) < __builtin_inff(); }       // false for NaN
__device__ __forceinline__ size_t ft_mesh_corner_at(const FtMeshArgs& a, size_t q, uint32_t c) {
    return q + (size_t)((c >> 2) & 1u) * a.ny * a.nz + (size_t)((c >> 1) & 1u) * a.nz + (c & 1u);
}

__device__ __forceinline__ FtMeshCorners ft_mesh_classify(const FtMeshArgs& a, uint32_t q) {
    const uint32_t k = q % a.nz, ij = q / a.nz, j = ij % a.ny, i = ij / a.ny;
    const bool ei = i + 1u < a.nx, ej = j + 1u < a.ny, ek = k + 1u < a.nz;
    FtMeshCorners r{0u, 0u, ei && ej && ek};
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) {
        const bool exists = (!(c & 4u) || ei) && (!(c & 2u) || ej) && (!(c & 1u) || ek);
        if (!exists) continue;
        const float s = ft_mesh_signed(a, ft_mesh_corner_at(a, q, c));
        if (ft_mesh_finite(s)) r.fin8 |= 1u << c;
        if (s < 0.0f) r.in8 |= 1u << c;
    }
    return r;
}

// the vertices q owns: edge (q, e) ends at corner e + 1
__device__ __forceinline__ uint32_t ft_mesh_owned(const FtMeshCorners& r) {
    if (!(r.fin8 & 1u)) return 0u;
    const uint32_t differs = ((r.in8 & 1u) ? ~r.in8 : r.in8) & r.fin8;
    return (differs >> 1) & 0x7fu;
}

// per tetrahedron of cell q its inside mask, or 16 where a corner is not finite; triangles and skipped tetrahedra of the cell
__device__ __forceinline__ uint32_t ft_mesh_case(const FtMeshCorners& r, int t) {
    const uint32_t need = 1u | (1u << ft_mesh_c1(t)) | (1u << ft_mesh_c2(t)) | 128u;
    if ((r.fin8 & need) != need) return 16u;
    return (r.in8 & 1u) | (((r.in8 >> ft_mesh_c1(t)) & 1u) << 1) | (((r.in8 >> ft_mesh_c2(t)) & 1u) << 2) | (((r.in8 >> 7) & 1u) << 3);
}
__device__ __forceinline__ uint32_t ft_mesh_case_triangles(uint32_t m) {
    const uint32_t inside = (uint32_t)__popc(m & 15u);
    return m >= 16u ? 0u : (inside == 2u ? 2u : ((inside == 1u || inside == 3u) ? 1u : 0u));
}

// ---- sums and scans across a workgroup ------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup's threads; every thread calls it.  lds: one word per wave, reusable after the call's last barrier
__device__ __forceinline__ uint32_t ft_mesh_block_exclusive(uint32_t v, uint32_t* lds) {                // any workgroup of whole waves
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

template <int TILE> __global__ __launch_bounds__(TILE) void ft_mesh_count_kernel(FtMeshArgs a) {
    __shared__ unsigned long long red[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nTiles; tile += gridDim.x) {
        const unsigned long long q64 = (unsigned long long)tile * TILE + threadIdx.x;
        unsigned long long packed = 0ull;                              // vertices | triangles << 20 | skipped << 40: a tile's sums stay below 2^20
        if (q64 < a.n) {
            const uint32_t q = (uint32_t)q64;
            const FtMeshCorners r = ft_mesh_classify(a, q);
            const uint32_t own = ft_mesh_owned(r);
            a.mask[q] = (uint8_t)own;
            uint32_t tris = 0u, skipped = 0u;
            if (r.cell) {
#pragma unroll
                for (int t = 0; t < 6; ++t) { const uint32_t m = ft_mesh_case(r, t); tris += ft_mesh_case_triangles(m); skipped += m >= 16u ? 1u : 0u; }
            }
            packed = (unsigned long long)__popc(own) | ((unsigned long long)tris << 20) | ((unsigned long long)skipped << 40);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) packed += __shfl_down(packed, off, 64);
        __syncthreads();
        if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = packed;
        __syncthreads();
        if (threadIdx.x == 0u) {
            unsigned long long s = 0ull;
            for (int w = 0; w < TILE / 64; ++w) s += red[w];
            a.tileV[tile] = (uint32_t)(s & 0xfffffull);
            a.tileT[tile] = (uint32_t)((s >> 20) & 0xfffffull);
            a.tileS[tile] = (uint32_t)(s >> 40);
        }
    }
}

// One workgroup.  Levels: FT_MESH_SCAN_ITEMS tile sums in a thread, 64 threads in a wave, the waves of the workgroup through LDS, and a carry from
// each round of FT_MESH_SCAN_BLOCK * FT_MESH_SCAN_ITEMS tiles to the next.  The prefixes are kept mod 2^32 (a mesh of 2^31 or more is refused from the
// 64-bit totals before anything reads them).
__global__ __launch_bounds__(FT_MESH_SCAN_BLOCK) void ft_mesh_scan_kernel(FtMeshArgs a) {
    constexpr int WAVES = FT_MESH_SCAN_BLOCK / 64;
    __shared__ unsigned long long wv[WAVES], wt[WAVES], ws[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carryV = 0ull, carryT = 0ull, carryS = 0ull;
    for (unsigned long long base = 0ull; base < a.nTiles; base += (unsigned long long)FT_MESH_SCAN_BLOCK * FT_MESH_SCAN_ITEMS) {
        const unsigned long long first = base + (unsigned long long)threadIdx.x * FT_MESH_SCAN_ITEMS;
        uint32_t v[FT_MESH_SCAN_ITEMS], t[FT_MESH_SCAN_ITEMS];
        unsigned long long sv = 0ull, st = 0ull, ss = 0ull;
#pragma unroll
        for (int r = 0; r < FT_MESH_SCAN_ITEMS; ++r) {
            const bool in = first + r < a.nTiles;
            v[r] = in ? a.tileV[first + r] : 0u; t[r] = in ? a.tileT[first + r] : 0u;
            sv += v[r]; st += t[r]; ss += in ? a.tileS[first + r] : 0u;
        }
        unsigned long long iv = sv, it = st;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long pv = __shfl_up(iv, off, 64), pt = __shfl_up(it, off, 64);
            if (lane >= (uint32_t)off) { iv += pv; it += pt; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_down(ss, off, 64);
        __syncthreads();                                               // the previous round's readers of wv / wt / ws are done
        if (lane == 63u) { wv[wave] = iv; wt[wave] = it; }
        if (lane == 0u) ws[wave] = ss;
        __syncthreads();
        unsigned long long beforeV = carryV, beforeT = carryT;
        for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
            if (w < wave) { beforeV += wv[w]; beforeT += wt[w]; }
            carryV += wv[w]; carryT += wt[w]; carryS += ws[w];
        }
        unsigned long long ev = beforeV + iv - sv, et = beforeT + it - st;
#pragma unroll
        for (int r = 0; r < FT_MESH_SCAN_ITEMS; ++r) {
            if (first + r < a.nTiles) { a.tileV[first + r] = (uint32_t)ev; a.tileT[first + r] = (uint32_t)et; }
            ev += v[r]; et += t[r];
        }
    }
    if (threadIdx.x == 0u) { a.totals[0] = carryV; a.totals[1] = carryT; a.totals[2] = carryS; }
}

// the sum of tile `tile` from the scanned prefixes
__device__ __forceinline__ uint32_t ft_mesh_tile_sum(const uint32_t* prefix, uint32_t tile, uint32_t nTiles, uint32_t total) {
    return (tile + 1u < nTiles ? prefix[tile + 1u] : total) - prefix[tile];
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_mesh_vertices_kernel(FtMeshArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nTiles; tile += gridDim.x) {
        const unsigned long long q64 = (unsigned long long)tile * TILE + threadIdx.x;
        const bool live = q64 < a.n;
        const uint32_t q = (uint32_t)q64, tileBase = a.tileV[tile];
        if (ft_mesh_tile_sum(a.tileV, tile, a.nTiles, a.nV) == 0u) {   // nothing owned here (the whole workgroup agrees): only the index
            if (live) a.vbase[q] = tileBase;
            continue;
        }
        const uint32_t own = live ? a.mask[q] : 0u;
        const uint32_t at = tileBase + ft_mesh_block_exclusive((uint32_t)__popc(own), lds);
        if (!live) continue;
        a.vbase[q] = at;
        if (!own) continue;
        const uint32_t k = q % a.nz, ij = q / a.nz, j = ij % a.ny, i = ij / a.ny;
        const uint32_t idx[3] = {i, j, k};
        const float s0 = ft_mesh_signed(a, q);
        float p0[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) p0[ax] = a.origin[ax] + (float)idx[ax] * a.step[ax];
        uint32_t rank = 0u;
#pragma unroll
        for (uint32_t e = 0; e < 7u; ++e) {
            if (!((own >> e) & 1u)) continue;
            const uint32_t c = e + 1u;
            const float s1 = ft_mesh_signed(a, ft_mesh_corner_at(a, q, c));
            const float t = s0 / (s0 - s1);                            // from the owner towards the far end
            const uint32_t d[3] = {(c >> 2) & 1u, (c >> 1) & 1u, c & 1u};
            const uint32_t v = at + rank;
            ++rank;
            if (v >= a.nV) continue;
            float* out = a.vertices + 3 * (size_t)v;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float p1 = a.origin[ax] + (float)(idx[ax] + d[ax]) * a.step[ax];
                out[ax] = p0[ax] + t * (p1 - p0[ax]);
            }
        }
    }
}

template <int TILE> __global__ __launch_bounds__(TILE) void ft_mesh_triangles_kernel(FtMeshArgs a) {
    __shared__ uint32_t lds[TILE / 64];
    for (uint32_t tile = blockIdx.x; tile < a.nTiles; tile += gridDim.x) {
        if (ft_mesh_tile_sum(a.tileT, tile, a.nTiles, a.nT) == 0u) continue;      // the whole workgroup agrees
        const unsigned long long q64 = (unsigned long long)tile * TILE + threadIdx.x;
        const bool live = q64 < a.n;
        const uint32_t q = (uint32_t)q64;
        FtMeshCorners r{0u, 0u, false};
        if (live) r = ft_mesh_classify(a, q);
        uint32_t cases[6], tris = 0u;
#pragma unroll
        for (int t = 0; t < 6; ++t) { cases[t] = r.cell ? ft_mesh_case(r, t) : 16u; tris += ft_mesh_case_triangles(cases[t]); }
        uint32_t at = a.tileT[tile] + ft_mesh_block_exclusive(tris, lds);
        if (!tris) continue;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const uint32_t n = ft_mesh_case_triangles(cases[t]);
            if (!n) continue;
            const unsigned long long word = FT_MESH_TABLE.e[t][cases[t]];
            for (uint32_t tri = 0; tri < n; ++tri, ++at) {
                if (at >= a.nT) continue;
                int32_t* out = a.triangles + 3 * (size_t)at;
#pragma unroll
                for (uint32_t c = 0; c < 3u; ++c) {
                    const uint32_t slot = (uint32_t)(word >> (2u + 6u * (3u * tri + c))) & 63u, e = slot & 7u;
                    const size_t owner = ft_mesh_corner_at(a, q, slot >> 3);
                    out[c] = (int32_t)(a.vbase[owner] + (uint32_t)__popc((uint32_t)a.mask[owner] & ((1u << e) - 1u)));
                }
            }
        }
    }
}

template <int TILE> const void* ft_mesh_kernel_of(int kernel) {
    switch (kernel) {
        case FT_MESH_K_COUNT: return (const void*)ft_mesh_count_kernel<TILE>;
        case FT_MESH_K_SCAN: return (const void*)ft_mesh_scan_kernel;
        case FT_MESH_K_VERTICES: return (const void*)ft_mesh_vertices_kernel<TILE>;
        case FT_MESH_K_TRIANGLES: return (const void*)ft_mesh_triangles_kernel<TILE>;
    }
    return nullptr;
}
const void* ft_mesh_kernel(int kernel, uint32_t tile) {
    switch (tile) {
        case 128u: return ft_mesh_kernel_of<128>(kernel);
        case 256u: return ft_mesh_kernel_of<256>(kernel);
        case 512u: return ft_mesh_kernel_of<512>(kernel);
        case 1024u: return ft_mesh_kernel_of<1024>(kernel);
    }
    return nullptr;
}

}  // namespace

extern "C" hipError_t ft_launch_mesh(int kernel, const FtMeshArgs* a, unsigned blocks, hipStream_t st) {
    const void* k = ft_mesh_kernel(kernel, a->tile);
    if (!k) return hipErrorInvalidDeviceFunction;
    FtMeshArgs args = *a;
    void* kp[] = {&args};
    const bool scan = kernel == FT_MESH_K_SCAN;
    return hipLaunchKernel(k, dim3(scan ? 1u : blocks), dim3(scan ? FT_MESH_SCAN_BLOCK : a->tile), kp, 0, st);
}
extern "C" hipError_t ft_mesh_occupancy(int kernel, uint32_t tile, int* blocksPerCU) {
    const void* k = ft_mesh_kernel(kernel, tile);
    if (!k) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocksPerCU, k, kernel == FT_MESH_K_SCAN ? FT_MESH_SCAN_BLOCK : (int)tile, 0);
}
extern "C" const unsigned long long* ft_mesh_table(void) { return &FT_MESH_TABLE_HOST.e[0][0]; }
