// contour_measure.hip — per-polyline and per-slice measures of contours on the device: length, enclosed area, first moment, box
// (include/fraytracer_hip.h "Contour measures" is the rule; this file is its device side; ft_contour_measure.h says what the four launches do and what
// the work memory holds).
//   extent + box   the call's extent (largest |coordinate|) and each polyline's box in the plane, as integer maxima and minima of float32 bit patterns
//   terms          per segment four float64 terms, each rounded once to a 128-bit integer; exact integer sums per run of a wave and per polyline
//   polylines      int128 -> float64 (round half to even, by hand), scaling, divisions, the record; the polyline's integers into its slice's
//   slices         the same conversion per slice, the record
// Float64 arithmetic: every -, *, + below is one IEEE operation (the Makefile's -ffp-contract=off and the pragma here), sqrt and / are the correctly
// rounded ones; ldexp and rint are exact operations.  Atomics: atomicMin, atomicMax and atomicAdd on integers at agent scope; every result is
// independent of the order they arrive in.  No kernel waits for another workgroup.
// The quantisation (ft_contour_add), the 128-bit add with carry through two 64-bit atomics (ft_contour_atomic_add), the conversion
// (ft_contour_to_double), the extent's exponent and the ordered keys are measure.hip's, restated here word for word rather than moved into a shared
// header: measure.hip and what it compiles to stay untouched.
#include <hip/hip_runtime.h>

#include "ft_contour_measure.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

struct FtContourRecord { double length, area, moment[2]; uint32_t boxMin[2], boxMax[2]; int32_t nUnmeasured, extentExponent; };                 // ft_contour_measure
struct FtContourSliceRecord { double length, area, moment[2]; uint32_t boxMin[2], boxMax[2]; int32_t nPolylines, nClosed, nOuter, nHoles, nUnmeasured, extentExponent; };      // ft_slice_measure
static_assert(sizeof(FtContourRecord) == FT_CONTOUR_RECORD_BYTES && sizeof(FtContourSliceRecord) == FT_CONTOUR_SLICE_RECORD_BYTES, "layout");

// the grid-stride loop, whole waves at a time and a contiguous chunk of FT_CONTOUR_BLOCK items per workgroup iteration: lanes hold consecutive items;
// `item` may be at or beyond n (the lane then only takes part in the wave's shuffles)
#define FT_CONTOUR_FOR(item, n)                                                                                                              \
    for (u64 item##Base = (u64)blockIdx.x * FT_CONTOUR_BLOCK; item##Base < (n); item##Base += (u64)gridDim.x * FT_CONTOUR_BLOCK)             \
        for (u64 item = item##Base + threadIdx.x, item##Once = 1; item##Once; item##Once = 0)

// E of the rule from the largest |bits| of a finite coordinate: 0 for 0, else ilogb + 1, denormals by their true exponent
__device__ __forceinline__ int ft_contour_exponent(uint32_t maxBits) {
    if (maxBits == 0u) return 0;
    if (maxBits >= 0x00800000u) return (int)(maxBits >> 23) - 126;
    return -148 + (31 - __clz((int)maxBits));
}
// the bound exponent B of a kind: length E + 2, twice the area 2E + 2, the moments 3E + 3
__device__ __forceinline__ int ft_contour_bound(int kind, int E) { return kind == 0 ? E + 2 : (kind == 1 ? 2 * E + 2 : 3 * E + 3); }

__device__ __forceinline__ bool ft_contour_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
// the ordered key of a float32 bit pattern: unsigned order of the keys = numeric order of the floats, -0 below +0
__device__ __forceinline__ uint32_t ft_contour_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u); }
__device__ __forceinline__ uint32_t ft_contour_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

struct FtContourLine { uint32_t first, count, slice; bool closed; };

// The polyline of point i: the last record whose `first` is at or below i (binary search: `first` ascends with the index), then every word of it against
// its bound: the point lies in [first, first + count), that range in 0 .. nP, the slice in 0 .. nW - 1.  FT_CONTOUR_NONE: no record covers the point.
__device__ __forceinline__ uint32_t ft_contour_find(const FtContourArgs& a, uint32_t i, FtContourLine& line) {
    uint32_t lo = 0u, hi = a.nL;
    while (lo < hi) {                                                  // mid < nL throughout
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)a.polylines[4 * (size_t)mid] <= i) lo = mid + 1u; else hi = mid;      // a negative first is a large one
    }
    if (lo == 0u) return FT_CONTOUR_NONE;
    const uint32_t l = lo - 1u;
    const int32_t* r = a.polylines + 4 * (size_t)l;
    line.first = (uint32_t)r[0]; line.count = (uint32_t)r[1]; line.slice = (uint32_t)r[2]; line.closed = r[3] != 0;
    const bool ok = line.first <= i && i - line.first < line.count && (u64)line.first + (u64)line.count <= (u64)a.nP && line.slice < a.nW;
    return ok ? l : FT_CONTOUR_NONE;
}

// does the lane `off` lanes up hold the same key (and is there such a lane): the partner of one step of a segmented reduction.  Lanes hold consecutive
// points and `first` ascends, so equal keys are neighbours: after the steps off = 1, 2, .. 32 the first lane of a run holds the run's result
__device__ __forceinline__ bool ft_contour_partner(uint32_t key, uint32_t lane, int off) {
    const uint32_t other = (uint32_t)__shfl_down((int)key, off, 64);
    return key != FT_CONTOUR_NONE && lane + (uint32_t)off < 64u && other == key;
}
__device__ __forceinline__ bool ft_contour_head(uint32_t key, uint32_t lane) {
    const uint32_t before = (uint32_t)__shfl_up((int)key, 1, 64);
    return key != FT_CONTOUR_NONE && (lane == 0u || before != key);
}

// ---- extent + box ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT_CONTOUR_BLOCK) void ft_contour_extent_kernel(FtContourArgs a) {
    const uint32_t lane = threadIdx.x & 63u, cu = (a.axis + 1u) % 3u, cv = (a.axis + 2u) % 3u;
    uint32_t most = 0u;
    FT_CONTOUR_FOR(i, a.nP) {
        uint32_t key = FT_CONTOUR_NONE, lo[2] = {0xffffffffu, 0xffffffffu}, hi[2] = {0u, 0u};
        if (i < a.nP) {
            uint32_t w[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                w[x] = a.points[3 * (size_t)i + x];
                if (ft_contour_finite(w[x])) most = max(most, w[x] & 0x7fffffffu);
            }
            FtContourLine line;
            key = ft_contour_find(a, (uint32_t)i, line);
            const uint32_t bu = cu == 0u ? w[0] : (cu == 1u ? w[1] : w[2]), bv = cv == 0u ? w[0] : (cv == 1u ? w[1] : w[2]);
            if (ft_contour_finite(bu)) lo[0] = hi[0] = ft_contour_key(bu);
            if (ft_contour_finite(bv)) lo[1] = hi[1] = ft_contour_key(bv);
        }
        if (!__any(key != FT_CONTOUR_NONE)) continue;                 // the same for the whole wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const bool take = ft_contour_partner(key, lane, off);
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const uint32_t ol = (uint32_t)__shfl_down((int)lo[x], off, 64), oh = (uint32_t)__shfl_down((int)hi[x], off, 64);
                if (take) { lo[x] = min(lo[x], ol); hi[x] = max(hi[x], oh); }
            }
        }
        if (ft_contour_head(key, lane)) {                              // key < nL: ft_contour_find checked it; hi == 0: no finite value, nothing to say
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                if (hi[x] == 0u) continue;
                atomicMin(a.boxMin + 2 * (size_t)key + x, lo[x]);
                atomicMax(a.boxMax + 2 * (size_t)key + x, hi[x]);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) most = max(most, (uint32_t)__shfl_xor((int)most, off, 64));
    if (lane == 0u && most != 0u) atomicMax(a.extent, most);
}

// ---- terms -----------------------------------------------------------------------------------------------------------------------------------------
// acc += round-half-to-even(term * 2^shift) as a 128-bit two's-complement integer.  ldexp is exact (the product stays far inside float64's range,
// or underflows towards a value below 1/2 that rounds to 0 either way), rint rounds once, and what it gives is an integer of at most 2^92: its 53
// significant bits are shifted into place
__device__ __forceinline__ void ft_contour_add(double term, int shift, u64& accLo, u64& accHi) {
    const u64 bits = (u64)__double_as_longlong(rint(ldexp(term, shift)));
    const int e = (int)((bits >> 52) & 0x7ffu);
    const u64 m = e ? ((bits & 0x000fffffffffffffull) | 0x0010000000000000ull) : 0ull;      // an integer: exponent field 0 only for 0
    const int sh = e - 1075;
    u64 lo, hi;
    if (sh >= 0) { const int s = sh < 63 ? sh : 63; lo = m << s; hi = s ? m >> (64 - s) : 0ull; }
    else { const int s = -sh < 63 ? -sh : 63; lo = m >> s; hi = 0ull; }                      // an integer: nothing is shifted out
    if (bits >> 63) { lo = ~lo + 1ull; hi = ~hi + (lo == 0ull ? 1ull : 0ull); }
    accLo += lo;
    accHi += hi + (accLo < lo ? 1ull : 0ull);
}

// *p (two words: low, high) += the 128-bit integer (lo, hi), in any order with other adders
__device__ __forceinline__ void ft_contour_atomic_add(u64* p, u64 lo, u64 hi) {
    if ((lo | hi) == 0ull) return;
    const u64 old = atomicAdd(p, lo);                                  // this adder, and no other, sees whether its own addition wrapped the low word
    const u64 up = hi + ((u64)(old + lo) < old ? 1ull : 0ull);
    if (up != 0ull) atomicAdd(p + 1, up);
}

__global__ __launch_bounds__(FT_CONTOUR_BLOCK) void ft_contour_terms_kernel(FtContourArgs a) {
    const uint32_t lane = threadIdx.x & 63u, cu = (a.axis + 1u) % 3u, cv = (a.axis + 2u) % 3u;
    const int E = ft_contour_exponent(*a.extent);
    const int shiftL = FT_CONTOUR_SHIFT - ft_contour_bound(0, E), shiftC = FT_CONTOUR_SHIFT - ft_contour_bound(1, E), shiftM = FT_CONTOUR_SHIFT - ft_contour_bound(2, E);
    FT_CONTOUR_FOR(i, a.nP) {
        uint32_t key = FT_CONTOUR_NONE, bad = 0u;
        u64 lo[FT_CONTOUR_SUMS] = {0ull, 0ull, 0ull, 0ull}, hi[FT_CONTOUR_SUMS] = {0ull, 0ull, 0ull, 0ull};
        if (i < a.nP) {
            FtContourLine line;
            key = ft_contour_find(a, (uint32_t)i, line);
            if (key != FT_CONTOUR_NONE) {
                // the segment that starts at this point: to the next point, or from the last point of a closed polyline back to the first
                const uint32_t at = (uint32_t)i - line.first;
                uint32_t j = FT_CONTOUR_NONE;
                if (at + 1u < line.count) j = (uint32_t)i + 1u; else if (line.closed) j = line.first;
                if (j != FT_CONTOUR_NONE) {                            // j < first + count <= nP
                    const uint32_t pu = a.points[3 * (size_t)i + cu], pv = a.points[3 * (size_t)i + cv];
                    const uint32_t qu = a.points[3 * (size_t)j + cu], qv = a.points[3 * (size_t)j + cv];
                    if (ft_contour_finite(pu) && ft_contour_finite(pv) && ft_contour_finite(qu) && ft_contour_finite(qv)) {
                        const double Pu = (double)__uint_as_float(pu), Pv = (double)__uint_as_float(pv);
                        const double Qu = (double)__uint_as_float(qu), Qv = (double)__uint_as_float(qv);
                        const double du = Qu - Pu, dv = Qv - Pv;
                        const double L = sqrt(du * du + dv * dv);
                        const double C = Pu * Qv - Qu * Pv;
                        ft_contour_add(L, shiftL, lo[0], hi[0]);
                        ft_contour_add(C, shiftC, lo[1], hi[1]);
                        ft_contour_add(C * (Pu + Qu), shiftM, lo[2], hi[2]);
                        ft_contour_add(C * (Pv + Qv), shiftM, lo[3], hi[3]);
                    } else {
                        bad = 1u;
                    }
                }
            }
        }
        if (!__any(key != FT_CONTOUR_NONE)) continue;                 // the same for the whole wave
        bool head = key != FT_CONTOUR_NONE;                            // eager: every lane for itself
        if (!a.eager) {
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const bool take = ft_contour_partner(key, lane, off);
#pragma unroll
                for (int k = 0; k < FT_CONTOUR_SUMS; ++k) {
                    u64 ol = __shfl_down(lo[k], off, 64), oh = __shfl_down(hi[k], off, 64);
                    if (!take) { ol = 0ull; oh = 0ull; }
                    lo[k] += ol;
                    hi[k] += oh + (lo[k] < ol ? 1ull : 0ull);
                }
                const uint32_t ob = (uint32_t)__shfl_down((int)bad, off, 64);
                bad += take ? ob : 0u;
            }
            head = ft_contour_head(key, lane);
        }
        if (head) {                                                    // once per wave and polyline; key < nL: ft_contour_find checked it
#pragma unroll
            for (int k = 0; k < FT_CONTOUR_SUMS; ++k) ft_contour_atomic_add(a.sums + 2 * FT_CONTOUR_SUMS * (size_t)key + 2 * k, lo[k], hi[k]);
            if (bad != 0u) atomicAdd(a.unmeasured + key, bad);
        }
    }
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------------------------
// a 128-bit two's-complement integer as the nearest float64, ties to even: the magnitude's leading one goes to bit 127, the top 53 bits are the
// significand, bit 10 of the high word is the guard and everything below it the sticky bit; a significand that rounds up to 2^53 carries into the
// exponent by itself
__device__ __forceinline__ double ft_contour_to_double(u64 lo, u64 hi) {
    const bool negative = (hi >> 63) != 0ull;
    if (negative) { lo = ~lo + 1ull; hi = ~hi + (lo == 0ull ? 1ull : 0ull); }
    if ((lo | hi) == 0ull) return 0.0;
    const int lz = hi ? __clzll((long long)hi) : 64 + __clzll((long long)lo);
    u64 nh, nl;
    if (lz >= 64) { nh = lo << (lz - 64); nl = 0ull; }
    else if (lz == 0) { nh = hi; nl = lo; }
    else { nh = (hi << lz) | (lo >> (64 - lz)); nl = lo << lz; }
    u64 significand = nh >> 11;
    const bool guard = ((nh >> 10) & 1ull) != 0ull, sticky = ((nh & 0x3ffull) | nl) != 0ull;
    if (guard && (sticky || (significand & 1ull))) significand += 1ull;
    const u64 bits = ((u64)(1023 + 127 - lz) << 52) + (significand - 0x0010000000000000ull) + (negative ? 0x8000000000000000ull : 0ull);
    return __longlong_as_double((long long)bits);
}

// the four results of four sums {low, high}: length, area, the two moments
__device__ __forceinline__ void ft_contour_results(const u64* sums, int E, double& length, double& area, double (&moment)[2]) {
    double S[FT_CONTOUR_SUMS];
#pragma unroll
    for (int k = 0; k < FT_CONTOUR_SUMS; ++k) S[k] = ldexp(ft_contour_to_double(sums[2 * k], sums[2 * k + 1]), ft_contour_bound(k < 2 ? k : 2, E) - FT_CONTOUR_SHIFT);      // exact
    length = S[0];
    area = S[1] / 2.0;
    moment[0] = S[2] / 6.0;
    moment[1] = S[3] / 6.0;
}

__global__ __launch_bounds__(FT_CONTOUR_BLOCK) void ft_contour_polylines_kernel(FtContourArgs a) {
    const int E = ft_contour_exponent(*a.extent);
    FT_CONTOUR_FOR(l, a.nL) {
        if (l >= a.nL) continue;
        const int32_t* rec = a.polylines + 4 * (size_t)l;
        const uint32_t slice = (uint32_t)rec[2];
        const bool closed = rec[3] != 0;
        const u64* sums = a.sums + 2 * FT_CONTOUR_SUMS * (size_t)l;
        u64 q[2 * FT_CONTOUR_SUMS];
#pragma unroll
        for (int k = 0; k < 2 * FT_CONTOUR_SUMS; ++k) q[k] = sums[k];
        uint32_t kmin[2], kmax[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) { kmin[x] = a.boxMin[2 * (size_t)l + x]; kmax[x] = a.boxMax[2 * (size_t)l + x]; }
        const uint32_t bad = a.unmeasured[l];
        if (a.outPolylines) {
            FtContourRecord r;
            ft_contour_results(q, E, r.length, r.area, r.moment);
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                r.boxMin[x] = kmax[x] ? ft_contour_unkey(kmin[x]) : 0x7f800000u;       // no finite value: +inf / -inf
                r.boxMax[x] = kmax[x] ? ft_contour_unkey(kmax[x]) : 0xff800000u;
            }
            r.nUnmeasured = (int32_t)bad;
            r.extentExponent = E;
            static_cast<FtContourRecord*>(a.outPolylines)[l] = r;
        }
        if (!a.outSlices || slice >= a.nW) continue;                   // a slice outside 0 .. nW - 1 indexes nothing
        u64* ss = a.sliceSums + 2 * FT_CONTOUR_SUMS * (size_t)slice;
        ft_contour_atomic_add(ss, q[0], q[1]);                         // the length always; the area and the moments of closed polylines only
        if (closed) {
#pragma unroll
            for (int k = 1; k < FT_CONTOUR_SUMS; ++k) ft_contour_atomic_add(ss + 2 * k, q[2 * k], q[2 * k + 1]);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            if (kmax[x] == 0u) continue;
            atomicMin(a.sliceBoxMin + 2 * (size_t)slice + x, kmin[x]);
            atomicMax(a.sliceBoxMax + 2 * (size_t)slice + x, kmax[x]);
        }
        uint32_t* n = a.sliceCounters + FT_CONTOUR_COUNTERS * (size_t)slice;
        atomicAdd(n + 0, 1u);
        if (closed) {
            atomicAdd(n + 1, 1u);
            const bool negative = (q[3] >> 63) != 0ull, zero = (q[2] | q[3]) == 0ull;       // the sign of Q_C
            if (!zero) atomicAdd(n + (negative ? 3 : 2), 1u);
        }
        if (bad != 0u) atomicAdd(n + 4, bad);
    }
}

__global__ __launch_bounds__(FT_CONTOUR_BLOCK) void ft_contour_slices_kernel(FtContourArgs a) {
    const int E = ft_contour_exponent(*a.extent);
    FT_CONTOUR_FOR(w, a.nW) {
        if (w >= a.nW || !a.outSlices) continue;
        FtContourSliceRecord r;
        ft_contour_results(a.sliceSums + 2 * FT_CONTOUR_SUMS * (size_t)w, E, r.length, r.area, r.moment);
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const uint32_t top = a.sliceBoxMax[2 * (size_t)w + x];
            r.boxMin[x] = top ? ft_contour_unkey(a.sliceBoxMin[2 * (size_t)w + x]) : 0x7f800000u;
            r.boxMax[x] = top ? ft_contour_unkey(top) : 0xff800000u;
        }
        const uint32_t* n = a.sliceCounters + FT_CONTOUR_COUNTERS * (size_t)w;
        r.nPolylines = (int32_t)n[0]; r.nClosed = (int32_t)n[1]; r.nOuter = (int32_t)n[2]; r.nHoles = (int32_t)n[3]; r.nUnmeasured = (int32_t)n[4];
        r.extentExponent = E;
        static_cast<FtContourSliceRecord*>(a.outSlices)[w] = r;
    }
}

const void* ft_contour_kernel(int kernel) {
    switch (kernel) {
        case FT_CONTOUR_K_EXTENT: return (const void*)ft_contour_extent_kernel;
        case FT_CONTOUR_K_TERMS: return (const void*)ft_contour_terms_kernel;
        case FT_CONTOUR_K_POLYLINES: return (const void*)ft_contour_polylines_kernel;
        case FT_CONTOUR_K_SLICES: return (const void*)ft_contour_slices_kernel;
    }
    return nullptr;
}

}  // namespace

extern "C" int ft_contour_domain(int kernel) { return kernel <= FT_CONTOUR_K_TERMS ? 0 : (kernel == FT_CONTOUR_K_POLYLINES ? 1 : 2); }
extern "C" hipError_t ft_launch_contour(int kernel, const FtContourArgs* a, unsigned blocks, hipStream_t st) {
    const void* k = ft_contour_kernel(kernel);
    if (!k) return hipErrorInvalidDeviceFunction;
    FtContourArgs copy = *a;
    void* kp[] = {&copy};
    return hipLaunchKernel(k, dim3(blocks), dim3(FT_CONTOUR_BLOCK), kp, 0, st);
}
extern "C" hipError_t ft_contour_occupancy(int kernel, int* blocksPerCU) {
    const void* k = ft_contour_kernel(kernel);
    if (!k) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocksPerCU, k, FT_CONTOUR_BLOCK, 0);
}
