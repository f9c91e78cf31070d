// ft_measure.h — argument block and host-callable launchers of the per-shell measures (implemented in measure.hip; the rule:
// include/fraytracer_hip.h "Measures").  A header of its own: nothing kernels.hip, mesh.hip, slice.hip, refine.hip or shells.hip includes changes with it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#define FT_MEASURE_BLOCK 256           // threads per workgroup of the three kernels (one lane per vertex, triangle or shell, grid-stride)
#define FT_MEASURE_NONE 0xffffffffu    // "no shell": a label outside 0 .. nS - 1, a lane without a triangle, a lane that holds no partial sums
#define FT_MEASURE_SUMS 5              // the 128-bit sums per shell: area, six volumes, three times twenty-four moments
#define FT_MEASURE_SHIFT 90            // a term of bound exponent B is quantised to multiples of 2^(B - 90)
#define FT_MEASURE_RECORD_BYTES 72     // sizeof(ft_shell_measure)

// The three launches of a call, each reading only what earlier launches (and two memsets) wrote:
//   extent + box   per vertex: the wave's largest |bits| of a finite coordinate -> one atomicMax per wave at the end of its loop; per wave and distinct
//                  shell the smallest and largest ordered key of the finite values of each coordinate -> atomicMin / atomicMax
//   terms          per triangle: five float64 terms, each quantised once to a 128-bit integer (two 64-bit words), summed per lane while the lane's
//                  shell stays the same; a flush sums the lanes of one shell across the wave (128-bit adds with carry) and adds the result with 64-bit
//                  atomics: the low word with a returning atomicAdd, whose old value tells this adder, and no other, whether the word wrapped; the
//                  high word gets the sum's high word plus that carry.  Integer additions commute: the sums are exact whatever the order
//   finish         per shell: int128 -> float64 by hand (round half to even), the scaling, the three divisions, the box keys back to bits, the record
// No kernel waits for another workgroup; every index and label read from memory is checked against its bound before it is used.
//
// Work memory per shell: 80 B of sums (5 x {low, high}), 12 B of box minimum keys, 12 B of box maximum keys, 4 B of unmeasured triangles; 4 B of
// extent per call.  The minimum keys start at 0xffffffff, everything else at 0 (an ordered key of a finite float is in 0x00800000 .. 0xff7fffff, so
// a maximum key of 0 says "no finite value").
struct FtMeasureArgs {
    const uint32_t* vertices;      // nV x 3 float32 bits, only read
    const int32_t* triangles;      // nT x 3, only read; the three indices are checked before they are used
    const int32_t* vertexShell;    // nV labels, or NULL: every vertex has label 0
    const int32_t* triangleShell;  // nT labels, or NULL: every triangle has label 0
    uint32_t nV, nT, nS;
    unsigned long long* sums;      // nS x 10: per kind {low, high}, two's complement
    uint32_t* boxMin;              // nS x 3 ordered keys
    uint32_t* boxMax;              // nS x 3
    uint32_t* unmeasured;          // nS
    uint32_t* extent;              // 1 word: the largest |bits| of a finite coordinate
    void* out;                     // nS records of FT_MEASURE_RECORD_BYTES, 8-byte aligned (finish)
    int32_t scale;                 // convert only: out[i] = fl64(sums[i]) * 2^-scale as a double, i < nS
    int32_t eager;                 // terms, the probe only: 1 = a lane flushes its partial sums at every iteration (the form without the accumulation in registers)
};

#ifdef __cplusplus
extern "C" {
#endif
enum { FT_MEASURE_K_EXTENT = 0, FT_MEASURE_K_TERMS = 1, FT_MEASURE_K_FINISH = 2, FT_MEASURE_K_CONVERT = 3, FT_MEASURE_KERNELS = 4 };
// 0: one lane per vertex, 1: per triangle, 2: per shell
int ft_measure_domain(int kernel);
// blocks: workgroups of FT_MEASURE_BLOCK threads, each taking items blockIdx.x * FT_MEASURE_BLOCK + threadIdx.x, + blocks * FT_MEASURE_BLOCK, ...
hipError_t ft_launch_measure(int kernel, const FtMeasureArgs* a, unsigned blocks, hipStream_t st);
hipError_t ft_measure_occupancy(int kernel, int* blocksPerCU);
#ifdef __cplusplus
}
#endif
