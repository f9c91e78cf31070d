// ft_slice.h — argument block and host-callable launchers of the slicer (implemented in slice.hip; the rule: include/fraytracer_hip.h "Slicing").
// A header of its own: nothing kernels.hip or mesh.hip includes changes with it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

// items per tile = threads per workgroup of the tiled kernels, one lane per lattice point (k contiguous) or per vertex: 128, 256, 512 or 1024.  Every
// tile gives the same contours
#define FT_SLICE_TILE_DEFAULT 512
#define FT_SLICE_SCAN_BLOCK 512   // threads of the scan kernel's single workgroup
// consecutive tile sums per thread and round of the scan: FT_SLICE_SCAN_BLOCK * FT_SLICE_SCAN_ITEMS tiles per round.  4, not the mesher's 8: with 8 the
// scan kernels took 144 VGPRs, and in a run of the whole GPU suite the occupancy query answered 0 for them (alone they had passed); with 4 they take 98,
// below the mesher's 120, which that query has always placed
#define FT_SLICE_SCAN_ITEMS 4
#define FT_SLICE_FLAT_BLOCK 256   // threads per workgroup of the untiled kernels (one lane per vertex, grid-stride)
#define FT_SLICE_NONE 0xffffffffu // "no vertex" in next / prev
#define FT_SLICE_DONE 0x80000000u // in a jump state's ancestor word: the ancestor is the chain's head (vertex totals stay below 2^31)

// One jump state per vertex, as three words: anc (the vertex `hops` segments back along prev, FT_SLICE_DONE set once that is the chain's head), hops,
// and low (the smallest vertex index from the vertex back to anc: anc itself only once it is the head).
struct FtSliceState { uint32_t* anc; uint32_t* hops; uint32_t* low; };

// One extraction over a lattice of n = nx * ny * nz < 0xFFFF0000 points, planes normal to `axis`, counts >= 2 along the two in-plane axes.  All pointers
// are device memory.  Lattice passes (nTiles tiles of `tile` points):
//   count    values -> mask (per point the 3 bits of the vertices it owns on its in-plane edges, ascending e), tileA / tileB / tileC = per tile
//            the vertices, the segments and the skipped triangles
//   scan     tileA, tileB -> exclusive prefix sums in place (mod 2^32), totals = the three sums in 64 bits (tileC is only summed)
//   emit     mask, tileA -> vbase (per point the index of its first vertex), vpos (nV x 3 floats), vslice (per vertex its plane)
//   link     values, mask, vbase -> next[start] = end, prev[end] = start per segment (both initialised to FT_SLICE_NONE by the host)
// Vertex passes (nV vertices; nVTiles tiles of `tile` vertices):
//   lead     prev -> state `from`: one hop
//   jump     state `from` -> state `to`: pointer doubling, one round; reads only `from`
//   cut      state `from` in place after the lead rounds: cyc (1: on a cycle), every cycle cut in front of its smallest vertex, open chains kept
//   tail     state `from` (every vertex done), next, prev -> len[head] = points of the polyline (len zeroed by the host)
//   heads    len, cyc -> vtA / vtB / vtC = per tile of vertices the polylines, their points, the closed ones
//   (scan over vtA, vtB, vtC with nTiles = nVTiles)
//   records  len, cyc, vslice, vtA, vtB -> off (per head its first point), polylines (nL records of 4 int32)
//   scatter  state `from`, off, vpos -> points (nP x 3 floats)
struct FtSliceArgs {
    const float* values;
    float iso;
    uint32_t axis;
    uint32_t nx, ny, nz;
    uint32_t n, nTiles, tile;     // nTiles = ceil(n / tile)
    float origin[3], step[3];
    uint8_t* mask;                // n bytes
    uint32_t* vbase;              // n words
    uint32_t* tileA;              // nTiles words each
    uint32_t* tileB;
    uint32_t* tileC;
    unsigned long long* totals;   // 3 x 64 bits
    uint32_t nV, nVTiles;         // from here on: after the first totals are known
    float* vpos;                  // nV x 3
    uint32_t* vslice;             // nV words each
    uint32_t* next;
    uint32_t* prev;
    FtSliceState from, to;
    uint8_t* cyc;                 // nV bytes
    uint32_t* len;
    uint32_t* off;
    uint32_t* vtA;                // nVTiles words each
    uint32_t* vtB;
    uint32_t* vtC;
    unsigned long long* vtotals;  // 3 x 64 bits
    uint32_t nP, nL;              // after the second totals are known; nothing is written at or beyond nP points / nL polylines
    float* points;
    int32_t* polylines;
};

#ifdef __cplusplus
extern "C" {
#endif
enum { FT_SLICE_K_COUNT = 0, FT_SLICE_K_SCAN = 1, FT_SLICE_K_EMIT = 2, FT_SLICE_K_LINK = 3, FT_SLICE_K_LEAD = 4, FT_SLICE_K_JUMP = 5, FT_SLICE_K_CUT = 6,
       FT_SLICE_K_TAIL = 7, FT_SLICE_K_HEADS = 8, FT_SLICE_K_VSCAN = 9, FT_SLICE_K_RECORDS = 10, FT_SLICE_K_SCATTER = 11, FT_SLICE_KERNELS = 12 };
// blocks: workgroups, each taking tiles (or, in the untiled kernels lead .. tail and scatter, FT_SLICE_FLAT_BLOCK vertices) blockIdx.x, blockIdx.x +
// blocks, ...; the scan kernels are always one workgroup
hipError_t ft_launch_slice(int kernel, const FtSliceArgs* a, unsigned blocks, hipStream_t st);
// `rounds` jump rounds from a->from, alternating between a->from and a->to, launched back to back: the result is in a->from if rounds is even
hipError_t ft_launch_slice_jumps(const FtSliceArgs* a, unsigned rounds, unsigned blocks, hipStream_t st);
hipError_t ft_slice_occupancy(int kernel, uint32_t tile, int* blocksPerCU);
unsigned ft_slice_block(int kernel, uint32_t tile);
// the direction table the link kernel reads, built at compile time from the integer corner offsets (slice.hip ft_slice_make_table): entry
// [triangle 0 / 1][inside mask of its three corners in the rule's order] = 0 where there is no segment, else 1 | start slot << 1 | end slot << 5 with
// slot = (owner corner 2 du + dv) << 2 | (edge direction 2 du + dv)
const uint32_t* ft_slice_table(void);
#ifdef __cplusplus
}
#endif
