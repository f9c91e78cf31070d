// ft_mesh.h — argument block and host-callable launchers of the mesher (implemented in mesh.hip; the rule: include/fraytracer_hip.h "Meshing").
// A header of its own: nothing kernels.hip includes changes with it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

// lattice points per tile = threads per workgroup of the count and emit kernels, one lane per point, k contiguous: 128, 256, 512 or 1024.  The shipped
// one by measurement (256^3 lattices, kernel ms of count + scan + emit for 128 / 256 / 512 / 1024, profiles/mesh_probe.jsonl): C3 0.925 / 0.628 /
// 0.576 / 0.585, 1000 tori 1.093 / 0.729 / 0.686 / 0.695, combinator crowd (128^3) 0.146 / 0.107 / 0.101 / 0.100.  Every tile gives the same mesh
#define FT_MESH_TILE_DEFAULT 512
#define FT_MESH_SCAN_BLOCK 512    // threads of the scan kernel's single workgroup: two waves per SIMD, resident whatever its registers
#define FT_MESH_SCAN_ITEMS 8      // consecutive tile sums per thread and round of the scan: FT_MESH_SCAN_BLOCK * FT_MESH_SCAN_ITEMS tiles per round

// One extraction over a lattice of n = nx * ny * nz < 0xFFFF0000 points, every count >= 2.  All pointers are device memory.
//   count:     values -> mask (per point the 7 bits of the vertices it owns), tileV / tileT / tileS (per tile of `tile` consecutive points
//              the vertices its points own, the triangles and the skipped tetrahedra of the cells at its points)
//   scan:      tileV, tileT -> their exclusive prefix sums in place (mod 2^32); totals = {vertices, triangles, skipped} in 64 bits
//   vertices:  mask, tileV -> vbase (per point the index of its first vertex), vertices (nV x 3 floats)
//   triangles: values, mask, vbase, tileT -> triangles (nT x 3 int32)
struct FtMeshArgs {
    const float* values;
    float iso;
    uint32_t nx, ny, nz;
    uint32_t n, nTiles, tile;     // nTiles = ceil(n / tile)
    float origin[3], step[3];
    uint8_t* mask;                // n bytes
    uint32_t* vbase;              // n words
    uint32_t* tileV;              // nTiles words each
    uint32_t* tileT;
    uint32_t* tileS;
    unsigned long long* totals;   // 3 x 64 bits
    float* vertices;              // emit only; nothing is written at or beyond nV vertices / nT triangles
    int32_t* triangles;
    uint32_t nV, nT;
};

#ifdef __cplusplus
extern "C" {
#endif
enum { FT_MESH_K_COUNT = 0, FT_MESH_K_SCAN = 1, FT_MESH_K_VERTICES = 2, FT_MESH_K_TRIANGLES = 3 };
// blocks: workgroups of a->tile threads, each taking tiles blockIdx.x, blockIdx.x + blocks, ...; the scan kernel is always one workgroup
hipError_t ft_launch_mesh(int kernel, const FtMeshArgs* a, unsigned blocks, hipStream_t st);
hipError_t ft_mesh_occupancy(int kernel, uint32_t tile, int* blocksPerCU);
// the orientation table the triangle kernel reads, built at compile time from the integer corner offsets (mesh.hip ft_mesh_make_table): entry
// [tetrahedron][inside mask of its corners c0 .. c3] = triangle count in bits 0-1, then six 6-bit slots (owner corner 4 di + 2 dj + dk) << 3 | e
const unsigned long long* ft_mesh_table(void);
#ifdef __cplusplus
}
#endif
