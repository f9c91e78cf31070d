// ft_contour_measure.h — argument block and host-callable launchers of the contour measures (implemented in contour_measure.hip; the rule:
// include/fraytracer_hip.h "Contour measures").  A header of its own: nothing kernels.hip, mesh.hip, slice.hip, refine.hip, shells.hip or measure.hip
// includes changes with it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#define FT_CONTOUR_BLOCK 256            // threads per workgroup of the four kernels (one lane per point, polyline or slice, grid-stride in whole chunks)
#define FT_CONTOUR_NONE 0xffffffffu     // "no polyline": a point that no record covers, a lane without a point
#define FT_CONTOUR_SUMS 4               // the 128-bit sums per polyline and per slice: length, twice the area, six times the two moments
#define FT_CONTOUR_SHIFT 90             // "Measures"' quantisation: a term of bound exponent B is quantised to multiples of 2^(B - 90)
#define FT_CONTOUR_RECORD_BYTES 56      // sizeof(ft_contour_measure)
#define FT_CONTOUR_SLICE_RECORD_BYTES 72 // sizeof(ft_slice_measure)
#define FT_CONTOUR_COUNTERS 5           // per slice: polylines, closed, outer, holes, unmeasured segments

// The four launches of a call, each reading only what earlier launches (and two memsets) wrote:
//   extent + box   per point: the wave's largest |bits| of a finite coordinate (all three) -> one atomicMax per wave at the end of its loop; the point's
//                  polyline by binary search over the records' `first` (ascending with the polyline index: slice.hip's records kernel takes `first`
//                  from a prefix sum over the chain heads in the order it numbers the polylines in; the internal entry refuses anything else); lanes
//                  hold consecutive points, so a wave sees its polylines as runs: a segmented reduction gives each run's smallest and largest ordered
//                  key of the finite u and of the finite v -> atomicMin / atomicMax by the run's first lane
//   terms          per point the segment that starts there (the last point of a closed polyline owns the closing segment, the last point of an open
//                  one owns nothing): four float64 terms, each quantised once to a 128-bit integer (two 64-bit words); a segmented reduction sums
//                  each run (128-bit adds with carry) and the run's first lane adds the result with 64-bit atomics: the low word with a returning
//                  atomicAdd, whose old value tells this adder, and no other, whether the word wrapped; the high word gets the sum's high word plus
//                  that carry.  Integer additions commute: the sums are exact whatever the order
//   polylines      per polyline: int128 -> float64 by hand (round half to even), the scaling, the divisions, the box keys back to bits, the record;
//                  and the polyline's integer sums, box keys and counters into its slice's accumulators with the same atomics (the length always, the
//                  area and the moments of closed polylines only).  A slice's polylines need not be contiguous
//   slices         per slice: the same conversion, the record
// No kernel waits for another workgroup; every first, count and slice read from memory is checked against its bound before it indexes anything.
//
// Work memory per polyline: 64 B of sums (4 x {low, high}), 8 B of box minimum keys, 8 B of box maximum keys, 4 B of unmeasured segments = 84 B;
// per slice: 64 B of sums, 16 B of box keys, 20 B of counters = 100 B; 4 B of extent per call.  The minimum keys start at 0xffffffff, everything else at
// 0 (an ordered key of a finite float is in 0x00800000 .. 0xff7fffff, so a maximum key of 0 says "no finite value").
struct FtContourArgs {
    const uint32_t* points;          // nP x 3 float32 bits, only read
    const int32_t* polylines;        // nL x {first, count, slice, closed}, only read; first ascends with the index
    uint32_t nP, nL, nW, axis;       // axis 0 .. 2: u = (axis + 1) % 3, v = (axis + 2) % 3
    unsigned long long* sums;        // nL x 8: per kind {low, high}, two's complement
    uint32_t* boxMin;                // nL x 2 ordered keys (u, v)
    uint32_t* boxMax;                // nL x 2
    uint32_t* unmeasured;            // nL
    unsigned long long* sliceSums;   // nW x 8
    uint32_t* sliceBoxMin;           // nW x 2
    uint32_t* sliceBoxMax;           // nW x 2
    uint32_t* sliceCounters;         // nW x FT_CONTOUR_COUNTERS
    uint32_t* extent;                // 1 word: the largest |bits| of a finite coordinate
    void* outPolylines;              // nL records of FT_CONTOUR_RECORD_BYTES, 8-byte aligned, or NULL
    void* outSlices;                 // nW records of FT_CONTOUR_SLICE_RECORD_BYTES, 8-byte aligned, or NULL
    int32_t eager;                   // terms, the probe only: 1 = every lane adds its own segment's terms (the form without the reduction across the wave)
};

#ifdef __cplusplus
extern "C" {
#endif
enum { FT_CONTOUR_K_EXTENT = 0, FT_CONTOUR_K_TERMS = 1, FT_CONTOUR_K_POLYLINES = 2, FT_CONTOUR_K_SLICES = 3, FT_CONTOUR_KERNELS = 4 };
// 0: one lane per point, 1: per polyline, 2: per slice
int ft_contour_domain(int kernel);
// blocks: workgroups of FT_CONTOUR_BLOCK threads, each taking items blockIdx.x * FT_CONTOUR_BLOCK + threadIdx.x, + blocks * FT_CONTOUR_BLOCK, ...
hipError_t ft_launch_contour(int kernel, const FtContourArgs* a, unsigned blocks, hipStream_t st);
hipError_t ft_contour_occupancy(int kernel, int* blocksPerCU);
#ifdef __cplusplus
}
#endif
