// ft_refine.h — argument block and host-callable launchers of the vertex refinement (implemented in refine.hip; the rule: include/fraytracer_hip.h
// "Refinement").  A header of its own: nothing kernels.hip, mesh.hip or slice.hip includes changes with it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#define FT_REFINE_BLOCK 256            // threads per workgroup of all three kernels: one lane per item, grid-stride
#define FT_REFINE_MAX_STEPS 32
// the 3-bit corner codes (4 di + 2 dj + dk) of the edges behind the bits of a lattice point's mask, bit b at 3 b: the mesher's seven directions, and per
// slice axis the three without a component along it, ascending e (the header's "Slicing": e 0, 1, 2 / 0, 3, 4 / 1, 3, 5)
#define FT_REFINE_EDGES_MESH 0x1f58d1u                                  // 1, 2, 3, 4, 5, 6, 7
#define FT_REFINE_EDGES_SLICE {0x0d1u, 0x161u, 0x1a2u}                  // 1, 2, 3 / 1, 4, 5 / 2, 4, 6
// work the context keeps per bracket: the eight bracket arrays, the midpoint and its distance (FT_REFINE_ITEM_BYTES); a segment query adds the second
// end's distance
#define FT_REFINE_ITEM_BYTES 48
#define FT_REFINE_SEGMENT_BYTES 52

// The state of n brackets as separate arrays, so that a wave's loads and stores are contiguous: ends A and B per coordinate, their signed values.
// A bracket whose sa is NaN is no bracket (a segment that does not cross): the rounds leave it alone and the finish writes three NaN.
struct FtRefineBracket { float* a[3]; float* b[3]; float* sa; float* sb; };

// All pointers are device memory.  nV brackets; nothing is written at or beyond nV items of any array.
//   lattice   values, mask, vbase (what the mesher's or slicer's count and emit passes left) -> the brackets of the owned edges in key order
//   segments  segA, segB (nV x 3), distA, distB -> status (may be NULL), the brackets
//   round     dist = D(mid) -> one round of the rule on every bracket
// Every kernel ends alike: last = 0 writes the next midpoint into mid (nV x 3: the point buffer of the next field launch), last = 1 writes the finish
// into out (nV x 3) instead.
struct FtRefineArgs {
    FtRefineBracket br;
    float* mid;
    const float* dist;
    float iso;
    uint32_t nV;
    uint32_t last;
    float* out;
    // lattice: n = nx * ny * nz < 0xFFFF0000 points; edges: the corner codes of the mask's bits (FT_REFINE_EDGES_*)
    const float* values;
    uint32_t nx, ny, nz, n;
    float origin[3], step[3];
    const uint8_t* mask;
    const uint32_t* vbase;
    uint32_t edges;
    // segments
    const float* segA;
    const float* segB;
    const float* distA;
    const float* distB;
    int32_t* status;
};

#ifdef __cplusplus
extern "C" {
#endif
enum { FT_REFINE_K_LATTICE = 0, FT_REFINE_K_SEGMENTS = 1, FT_REFINE_K_ROUND = 2, FT_REFINE_KERNELS = 3 };
// blocks: workgroups of FT_REFINE_BLOCK threads, each taking items blockIdx.x * FT_REFINE_BLOCK + threadIdx.x, + blocks * FT_REFINE_BLOCK, ...
hipError_t ft_launch_refine(int kernel, const FtRefineArgs* a, unsigned blocks, hipStream_t st);
hipError_t ft_refine_occupancy(int kernel, int* blocksPerCU);
#ifdef __cplusplus
}
#endif
