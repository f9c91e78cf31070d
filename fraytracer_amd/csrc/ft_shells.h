// ft_shells.h — argument block and host-callable launchers of the shell labelling and the selection (implemented in shells.hip; the rule:
// include/fraytracer_hip.h "Shells").  A header of its own: nothing kernels.hip, mesh.hip, slice.hip or refine.hip includes changes with it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

// items per tile = threads per workgroup of the tiled kernels (the ones in front of and behind a scan), one lane per vertex or triangle: 128, 256,
// 512 or 1024.  Every tile gives the same result
#define FT_SHELLS_TILE_DEFAULT 512
#define FT_SHELLS_SCAN_BLOCK 512   // threads of the scan kernel's single workgroup
#define FT_SHELLS_SCAN_ITEMS 4     // consecutive tile sums per thread and round of the scan (the slicer's 4: its scan has always been placed)
#define FT_SHELLS_FLAT_BLOCK 256   // threads per workgroup of the untiled kernels (one lane per vertex or triangle, grid-stride)
#define FT_SHELLS_NONE 0xffffffffu // "no candidate" in hook, "no vertex yet" in first
#define FT_SHELLS_BATCH 4          // iterations launched between two reads of the stop flag
#define FT_SHELLS_FLAG_OPEN 1u     // in a flag word: the verify launch found a triangle with two labels or a label that is no root
#define FT_SHELLS_FLAG_INVALID 2u  // in flag word 0: the first pass found an index outside 0 .. nV - 1 or twice in one triangle

// The labelling is Shiloach and Vishkin's algorithm (Y. Shiloach, U. Vishkin, "An O(log n) parallel connectivity algorithm", Journal of Algorithms 3
// (1982) 57-67), its five steps launched one kernel boundary apart so that every launch reads only what earlier launches wrote — exactly a run of
// the synchronous CRCW machine the paper's proof is about, with atomicMin as the machine's arbitrary winner of a concurrent write:
//   shortcut    parent2[v] = parent[parent[v]]; where that moved v, stamp[parent2[v]] = s
//   hook        side (i, j), both ways: parent2[i] == parent[i] and parent2[j] < parent2[i]: hook[parent2[i]] min= parent2[j], stamp[parent2[j]] = s
//   apply       parent2[r] = hook[r] where there is one; hook[r] = none
//   stagnant    side (i, j), both ways: r = parent2[i] is a root, stamp[r] < s and parent2[j] != r: hook[r] min= parent2[j]
//   apply
//   shortcut    parent[v] = parent2[parent2[v]]
// Bound (the paper's theorem): the sum of the heights of the trees that are not yet whole components shrinks to 2/3 or less per iteration, so after
// at most floor(log_{3/2} n) + 2 iterations every component is one star.  ft_shells_iteration_cap(n) is that number; the host loop stops there with
// an error, never with a partial labelling.  Roots are not the smallest vertices (the stagnant hook goes either way): the rule's numbering comes
// from `first` (atomicMin of the members per root) and a scan over the vertices in order.
// The stop decision is a launch of its own (verify): it reads parent as the iteration's last launch left it and ORs FT_SHELLS_FLAG_OPEN into the
// batch's flag word unless every triangle's three labels are equal and a root.
// Two of a triangle's three sides carry the hooks (they connect its three vertices); all three are sides for the border edges.
//
// Work memory: 9 words per vertex (parent, parent2, stamp, hook, first, degree, offset, cursor, remap: 36 B), 3 words per triangle (the
// vertex -> triangle incidence lists: 12 B), 16 B per three vertices for the records before their number is known, 4 B per tile of vertices and per
// tile of triangles, and 1 KB of flags and totals.
struct FtShellsArgs {
    const int32_t* triangles;     // nT x 3, only read; every kernel checks the three indices before it uses them
    uint32_t nV, nT, tile;
    uint32_t nVTiles, nTTiles;    // ceil(nV / tile), ceil(nT / tile)
    uint32_t scanTiles;           // the tiles of the next scan launch: nVTiles or nTTiles, whichever the sums in front of it were over
    uint32_t* parent;             // nV words each
    uint32_t* parent2;
    uint32_t* stamp;
    uint32_t* hook;               // between the iterations FT_SHELLS_NONE everywhere; after the numbering: per root its shell
    uint32_t* first;
    uint32_t* degree;             // triangles per vertex; 0: unused
    uint32_t* offset;             // exclusive prefix of degree
    uint32_t* cursor;
    uint32_t* incidence;          // 3 nT words
    uint32_t* tileA;              // max(nVTiles, nTTiles) words each: tile sums, then their exclusive prefix
    uint32_t* tileC;              // only summed
    unsigned long long* totals;   // [0] sum of tileA, [1] sum of tileC (the scan); [2] closed shells, [3] border edges (summary)
    uint32_t* flags;              // one word per batch
    uint32_t iteration;           // s of the iteration kernels, from 1
    uint32_t flagWord;            // the word the verify launch ORs into
    uint32_t nS;                  // the labelling: room in `records` (the shells' number is totals[0] once the leaders are scanned); the selection: shells
    int32_t* records;             // nS x 4 int32 (ft_shell)
    int32_t* vertexShell;         // nV
    int32_t* triangleShell;       // nT
    // selection
    const uint8_t* keep;          // nS bytes
    uint32_t* remap;              // nV words
    const uint32_t* srcVertices;  // nV x 3 words (float32 bits: copied, never computed with)
    const uint32_t* srcNormals;   // or NULL
    const uint32_t* srcMaterials; // or NULL
    uint32_t* dstVertices; uint32_t* dstNormals; uint32_t* dstMaterials; int32_t* dstTriangles;
    uint32_t nVOut, nTOut;        // nothing is written at or beyond them
};

#ifdef __cplusplus
extern "C" {
#endif
enum { FT_SHELLS_K_INIT = 0, FT_SHELLS_K_DEGREE = 1, FT_SHELLS_K_DEGREE_SUMS = 2, FT_SHELLS_K_SCAN = 3, FT_SHELLS_K_OFFSETS = 4, FT_SHELLS_K_FILL = 5,
       FT_SHELLS_K_SHORTCUT = 6, FT_SHELLS_K_HOOK = 7, FT_SHELLS_K_APPLY = 8, FT_SHELLS_K_STAGNANT = 9, FT_SHELLS_K_SHORTCUT2 = 10, FT_SHELLS_K_VERIFY = 11,
       FT_SHELLS_K_FIRST = 12, FT_SHELLS_K_LEADER_SUMS = 13, FT_SHELLS_K_NUMBER = 14, FT_SHELLS_K_LABEL_VERTICES = 15, FT_SHELLS_K_LABEL_TRIANGLES = 16,
       FT_SHELLS_K_SUMMARY = 17, FT_SHELLS_K_KEEP_VERTEX_SUMS = 18, FT_SHELLS_K_KEEP_TRIANGLE_SUMS = 19, FT_SHELLS_K_KEEP_VERTICES = 20,
       FT_SHELLS_K_KEEP_TRIANGLES = 21, FT_SHELLS_KERNELS = 22 };
// 0: one lane per vertex, 1: per triangle, 2: per shell, 3: the scan's single workgroup
int ft_shells_domain(int kernel);
// threads per workgroup: the tile for the tiled kernels, FT_SHELLS_SCAN_BLOCK for the scan, else FT_SHELLS_FLAT_BLOCK
unsigned ft_shells_block(int kernel, uint32_t tile);
// blocks: workgroups, each taking tiles (or, in the untiled kernels, FT_SHELLS_FLAT_BLOCK items) blockIdx.x, blockIdx.x + blocks, ...
hipError_t ft_launch_shells(int kernel, const FtShellsArgs* a, unsigned blocks, hipStream_t st);
// `count` iterations from a->iteration on (six launches each) and one verify launch, back to back
hipError_t ft_launch_shells_iterations(const FtShellsArgs* a, unsigned count, unsigned blocksV, unsigned blocksT, hipStream_t st);
hipError_t ft_shells_occupancy(int kernel, uint32_t tile, int* blocksPerCU);
// floor(log_{3/2} n) + 2 in integers: the iterations after which Shiloach and Vishkin's algorithm has finished on n vertices
unsigned ft_shells_iteration_cap(uint64_t n);
#ifdef __cplusplus
}
#endif
