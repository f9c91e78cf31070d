// measure.hip — per-shell measures of an indexed triangle mesh on the device: area, volume, first moment, box (include/fraytracer_hip.h "Measures"
// is the rule; this file is its device side; ft_measure.h says what the three launches do and what the work memory holds).
//   extent + box   the call's extent (largest |coordinate|) and each shell's box, both as integer maxima and minima of float32 bit patterns
//   terms          per triangle five float64 terms, each rounded once to a 128-bit integer; exact integer sums per lane, wave and shell
//   finish         int128 -> float64 (round half to even, by hand), scaling, divisions, the record;  convert: the same conversion on given sums
// Float64 arithmetic: every -, *, + below is one IEEE operation (the Makefile's -ffp-contract=off and the pragma here), sqrt and / are the
// correctly rounded ones; ldexp and rint are exact operations.  Atomics: atomicMin, atomicMax and atomicAdd on integers at agent scope; every result
// is independent of the order they arrive in.  No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "ft_measure.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

struct FtMeasureRecord { double area, volume, moment[3]; uint32_t boxMin[3], boxMax[3]; int32_t nUnmeasured, extentExponent; };     // ft_shell_measure
static_assert(sizeof(FtMeasureRecord) == FT_MEASURE_RECORD_BYTES, "layout");

// the grid-stride loop, whole waves at a time: `item` may be at or beyond n (the lane then only takes part in the wave's shuffles)
#define FT_MEASURE_FOR(item, n)                                                                                                              \
    for (u64 item##Base = (u64)blockIdx.x * FT_MEASURE_BLOCK; item##Base < (n); item##Base += (u64)gridDim.x * FT_MEASURE_BLOCK)             \
        for (u64 item = item##Base + threadIdx.x, item##Once = 1; item##Once; item##Once = 0)

// E of the rule from the largest |bits| of a finite coordinate: 0 for 0, else ilogb + 1, denormals by their true exponent
__device__ __forceinline__ int ft_measure_exponent(uint32_t maxBits) {
    if (maxBits == 0u) return 0;
    if (maxBits >= 0x00800000u) return (int)(maxBits >> 23) - 126;
    return -148 + (31 - __clz((int)maxBits));
}
// the bound exponent B of a kind: area 2E + 3, volume 3E + 3, moments 4E + 5
__device__ __forceinline__ int ft_measure_bound(int kind, int E) { return kind == 0 ? 2 * E + 3 : (kind == 1 ? 3 * E + 3 : 4 * E + 5); }

__device__ __forceinline__ bool ft_measure_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
// the ordered key of a float32 bit pattern: unsigned order of the keys = numeric order of the floats, -0 below +0
__device__ __forceinline__ uint32_t ft_measure_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u); }
__device__ __forceinline__ uint32_t ft_measure_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

// ---- extent + box ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT_MEASURE_BLOCK) void ft_measure_extent_kernel(FtMeasureArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t most = 0u;
    FT_MEASURE_FOR(v, a.nV) {
        uint32_t shell = FT_MEASURE_NONE, lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
        if (v < a.nV) {
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const uint32_t bits = a.vertices[3 * (size_t)v + x];
                if (!ft_measure_finite(bits)) continue;
                most = max(most, bits & 0x7fffffffu);
                lo[x] = hi[x] = ft_measure_key(bits);
            }
            shell = a.vertexShell ? (uint32_t)a.vertexShell[v] : 0u;
            if (shell >= a.nS) shell = FT_MEASURE_NONE;                // -1 (a vertex no triangle names) or anything else outside: in no box
        }
        u64 todo = __ballot(shell != FT_MEASURE_NONE);
        while (todo) {                                                 // the same for the whole wave: once per distinct shell
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t s0 = (uint32_t)__shfl((int)shell, leader, 64);
            const bool mine = shell == s0;
            uint32_t l[3], h[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) { l[x] = mine ? lo[x] : 0xffffffffu; h[x] = mine ? hi[x] : 0u; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    l[x] = min(l[x], (uint32_t)__shfl_xor((int)l[x], off, 64));
                    h[x] = max(h[x], (uint32_t)__shfl_xor((int)h[x], off, 64));
                }
            }
            // every lane holds the six results: lanes 0 .. 2 take the minima, 3 .. 5 the maxima; h == 0: no finite value, nothing to say
            const uint32_t myLo = lane == 0u ? l[0] : (lane == 1u ? l[1] : l[2]);
            const uint32_t myHi = lane == 3u ? h[0] : (lane == 4u ? h[1] : h[2]);
            if (lane < 3u && myLo != 0xffffffffu) atomicMin(a.boxMin + 3 * (size_t)s0 + lane, myLo);
            if (lane >= 3u && lane < 6u && myHi != 0u) atomicMax(a.boxMax + 3 * (size_t)s0 + (lane - 3u), myHi);
            todo &= ~__ballot(mine);
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
__device__ __forceinline__ void ft_measure_add(double term, int shift, u64& accLo, u64& accHi) {
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

// The partial sums of the lanes with key != FT_MEASURE_NONE go to their shells: per distinct key the wave's 128-bit sums (every lane ends with all
// of them), then lane k < 5 adds kind k and lane 5 the unmeasured triangles.  Every lane of the wave calls it.
__device__ __forceinline__ void ft_measure_flush(const FtMeasureArgs& a, uint32_t key, const u64 (&accLo)[FT_MEASURE_SUMS], const u64 (&accHi)[FT_MEASURE_SUMS],
                                                 uint32_t bad) {
    const uint32_t lane = threadIdx.x & 63u;
    u64 todo = __ballot(key != FT_MEASURE_NONE);
    while (todo) {                                                     // the same for the whole wave
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t s0 = (uint32_t)__shfl((int)key, leader, 64);    // below nS: the caller checked it
        const bool mine = key == s0;
        u64 lo[FT_MEASURE_SUMS], hi[FT_MEASURE_SUMS];
        uint32_t b = mine ? bad : 0u;
#pragma unroll
        for (int k = 0; k < FT_MEASURE_SUMS; ++k) { lo[k] = mine ? accLo[k] : 0ull; hi[k] = mine ? accHi[k] : 0ull; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < FT_MEASURE_SUMS; ++k) {
                const u64 ol = __shfl_xor(lo[k], off, 64), oh = __shfl_xor(hi[k], off, 64);
                lo[k] += ol;
                hi[k] += oh + (lo[k] < ol ? 1ull : 0ull);
            }
            b += (uint32_t)__shfl_xor((int)b, off, 64);
        }
        u64 myLo = lo[0], myHi = hi[0];
#pragma unroll
        for (int k = 1; k < FT_MEASURE_SUMS; ++k) if (lane == (uint32_t)k) { myLo = lo[k]; myHi = hi[k]; }
        if (lane < (uint32_t)FT_MEASURE_SUMS && (myLo | myHi) != 0ull) {
            u64* p = a.sums + 2 * FT_MEASURE_SUMS * (size_t)s0 + 2 * lane;
            const u64 old = atomicAdd(p, myLo);                        // this adder, and no other, sees whether its own addition wrapped the low word
            const u64 up = myHi + ((u64)(old + myLo) < old ? 1ull : 0ull);
            if (up != 0ull) atomicAdd(p + 1, up);
        }
        if (lane == (uint32_t)FT_MEASURE_SUMS && b != 0u) atomicAdd(a.unmeasured + s0, b);
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(FT_MEASURE_BLOCK) void ft_measure_terms_kernel(FtMeasureArgs a) {
    const int E = ft_measure_exponent(*a.extent);
    const int shiftA = FT_MEASURE_SHIFT - ft_measure_bound(0, E), shiftW = FT_MEASURE_SHIFT - ft_measure_bound(1, E), shiftM = FT_MEASURE_SHIFT - ft_measure_bound(2, E);
    uint32_t held = FT_MEASURE_NONE, bad = 0u;                         // the shell of this lane's partial sums
    u64 accLo[FT_MEASURE_SUMS] = {0ull, 0ull, 0ull, 0ull, 0ull}, accHi[FT_MEASURE_SUMS] = {0ull, 0ull, 0ull, 0ull, 0ull};
    FT_MEASURE_FOR(t, a.nT) {
        uint32_t shell = FT_MEASURE_NONE;
        if (t < a.nT) {
            shell = a.triangleShell ? (uint32_t)a.triangleShell[t] : 0u;
            if (shell >= a.nS) shell = FT_MEASURE_NONE;                // a triangle of no shell: in no sum and no count
        }
        const bool leave = held != FT_MEASURE_NONE && (a.eager != 0 || (shell != FT_MEASURE_NONE && shell != held));
        if (__any(leave)) {                                            // the same for the whole wave
            ft_measure_flush(a, leave ? held : FT_MEASURE_NONE, accLo, accHi, bad);
            if (leave) {
                held = FT_MEASURE_NONE; bad = 0u;
#pragma unroll
                for (int k = 0; k < FT_MEASURE_SUMS; ++k) { accLo[k] = 0ull; accHi[k] = 0ull; }
            }
        }
        if (shell == FT_MEASURE_NONE) continue;
        held = shell;
        const int32_t* p = a.triangles + 3 * (size_t)t;
        const uint32_t i0 = (uint32_t)p[0], i1 = (uint32_t)p[1], i2 = (uint32_t)p[2];       // a negative index is a large one
        bool ok = i0 < a.nV && i1 < a.nV && i2 < a.nV;
        uint32_t w[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (ok) {
#pragma unroll
            for (int x = 0; x < 3; ++x) { w[x] = a.vertices[3 * (size_t)i0 + x]; w[3 + x] = a.vertices[3 * (size_t)i1 + x]; w[6 + x] = a.vertices[3 * (size_t)i2 + x]; }
#pragma unroll
            for (int x = 0; x < 9; ++x) ok = ok && ft_measure_finite(w[x]);
        }
        if (!ok) { bad += 1u; continue; }
        const double ax = (double)__uint_as_float(w[0]), ay = (double)__uint_as_float(w[1]), az = (double)__uint_as_float(w[2]);
        const double bx = (double)__uint_as_float(w[3]), by = (double)__uint_as_float(w[4]), bz = (double)__uint_as_float(w[5]);
        const double cx = (double)__uint_as_float(w[6]), cy = (double)__uint_as_float(w[7]), cz = (double)__uint_as_float(w[8]);
        const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
        const double six = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
        ft_measure_add(area, shiftA, accLo[0], accHi[0]);
        ft_measure_add(six, shiftW, accLo[1], accHi[1]);
        ft_measure_add(six * ((ax + bx) + cx), shiftM, accLo[2], accHi[2]);
        ft_measure_add(six * ((ay + by) + cy), shiftM, accLo[3], accHi[3]);
        ft_measure_add(six * ((az + bz) + cz), shiftM, accLo[4], accHi[4]);
    }
    if (__any(held != FT_MEASURE_NONE)) ft_measure_flush(a, held, accLo, accHi, bad);
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------------------------
// a 128-bit two's-complement integer as the nearest float64, ties to even: the magnitude's leading one goes to bit 127, the top 53 bits are the
// significand, bit 10 of the high word is the guard and everything below it the sticky bit; a significand that rounds up to 2^53 carries into the
// exponent by itself
__device__ __forceinline__ double ft_measure_to_double(u64 lo, u64 hi) {
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

__global__ __launch_bounds__(FT_MEASURE_BLOCK) void ft_measure_finish_kernel(FtMeasureArgs a) {
    const int E = ft_measure_exponent(*a.extent);
    FT_MEASURE_FOR(s, a.nS) {
        if (s >= a.nS) continue;
        double S[FT_MEASURE_SUMS];
#pragma unroll
        for (int k = 0; k < FT_MEASURE_SUMS; ++k) {
            const u64* p = a.sums + 2 * FT_MEASURE_SUMS * (size_t)s + 2 * k;
            S[k] = ldexp(ft_measure_to_double(p[0], p[1]), ft_measure_bound(k, E) - FT_MEASURE_SHIFT);      // exact
        }
        FtMeasureRecord r;
        r.area = S[0];
        r.volume = S[1] / 6.0;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            r.moment[x] = S[2 + x] / 24.0;
            const uint32_t top = a.boxMax[3 * (size_t)s + x];
            r.boxMin[x] = top ? ft_measure_unkey(a.boxMin[3 * (size_t)s + x]) : 0x7f800000u;      // no finite value: +inf / -inf
            r.boxMax[x] = top ? ft_measure_unkey(top) : 0xff800000u;
        }
        r.nUnmeasured = (int32_t)a.unmeasured[s];
        r.extentExponent = E;
        static_cast<FtMeasureRecord*>(a.out)[s] = r;
    }
}

// the conversion alone, on given sums: out[i] = fl64(sums[i]) * 2^-scale
__global__ __launch_bounds__(FT_MEASURE_BLOCK) void ft_measure_convert_kernel(FtMeasureArgs a) {
    FT_MEASURE_FOR(i, a.nS) {
        if (i >= a.nS) continue;
        static_cast<double*>(a.out)[i] = ldexp(ft_measure_to_double(a.sums[2 * (size_t)i], a.sums[2 * (size_t)i + 1]), -a.scale);
    }
}

const void* ft_measure_kernel(int kernel) {
    switch (kernel) {
        case FT_MEASURE_K_EXTENT: return (const void*)ft_measure_extent_kernel;
        case FT_MEASURE_K_TERMS: return (const void*)ft_measure_terms_kernel;
        case FT_MEASURE_K_FINISH: return (const void*)ft_measure_finish_kernel;
        case FT_MEASURE_K_CONVERT: return (const void*)ft_measure_convert_kernel;
    }
    return nullptr;
}

}  // namespace

extern "C" int ft_measure_domain(int kernel) { return kernel == FT_MEASURE_K_EXTENT ? 0 : (kernel == FT_MEASURE_K_TERMS ? 1 : 2); }
extern "C" hipError_t ft_launch_measure(int kernel, const FtMeasureArgs* a, unsigned blocks, hipStream_t st) {
    const void* k = ft_measure_kernel(kernel);
    if (!k) return hipErrorInvalidDeviceFunction;
    FtMeasureArgs copy = *a;
    void* kp[] = {&copy};
    return hipLaunchKernel(k, dim3(blocks), dim3(FT_MEASURE_BLOCK), kp, 0, st);
}
extern "C" hipError_t ft_measure_occupancy(int kernel, int* blocksPerCU) {
    const void* k = ft_measure_kernel(kernel);
    if (!k) return hipErrorInvalidDeviceFunction;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocksPerCU, k, FT_MEASURE_BLOCK, 0);
}
