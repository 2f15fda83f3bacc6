// qm_block.hpp -- the wavefront and workgroup primitives of the front-end stage kernels (conditioning, picks,
// amplitudes, trigger, day files), each written once.  Every result is the same in every thread that gets it and in
// every run: the order of every combination is fixed.
//   wave level   wave_sum / wave_max / wave_first: f(i) over i < n by one wavefront -- lane l takes l, l + 64, ... in
//                that order, a butterfly 32..1 closes.  Nothing crosses wavefronts
//   order_key    doubles of either sign order like these 64-bit keys
//   BlockReduce  N 64-bit values per thread combined over the workgroup: butterfly 32..1 over the lanes, then the
//                wavefronts in ascending order.  One barrier per call
//   scans        wave_scan: inclusive over the lanes with an operator; block_scan: prefix sum over the workgroup
//   block_median exact median of up to 2^32 - 1 keyed values, NumPy's mean of the two middle ones for an even count
// The pragma that switches contraction off is lexical and device code is otherwise compiled with contraction allowed
// (qm_condition.hpp says what depends on it): every function here that adds or subtracts doubles has it in its body.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qm {

// ---- wave level: 64 lanes, the result identical in every lane -------------------------------------------------------
// sum over i < n of f(i), the same bits in every lane of the wavefront and in every run
template <typename F>
__device__ __forceinline__ double wave_sum(int n, F f) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int i = lane; i < n; i += 64) acc += f(i);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    return acc;
}

// max over i < n of f(i), the same in every lane
template <typename F>
__device__ __forceinline__ double wave_max(int n, F f) {
    const int lane = threadIdx.x & 63;
    double acc = -__builtin_inf();
    for (int i = lane; i < n; i += 64) {
        const double v = f(i);
        acc = v > acc ? v : acc;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(acc, m, 64);
        acc = o > acc ? o : acc;
    }
    return acc;
}

// smallest i < n with p(i), n where there is none
template <typename P>
__device__ __forceinline__ int wave_first(int n, P p) {
    const int lane = threadIdx.x & 63;
    int acc = n;
    for (int i = lane; i < n; i += 64)
        if (p(i) && i < acc) acc = i;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = __shfl_xor(acc, m, 64);
        acc = o < acc ? o : acc;
    }
    return acc;
}

// ---- keys -----------------------------------------------------------------------------------------------------------
// doubles of either sign order like these keys (-0.0 just below +0.0)
__device__ __forceinline__ unsigned long long order_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double order_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k ^ (1ull << 63)) : ~k;
    return __longlong_as_double((long long)u);
}

// ---- workgroup reduction --------------------------------------------------------------------------------------------
struct BlockAdd {
    __device__ __forceinline__ double operator()(double a, double b) const {
#pragma clang fp contract(off)
        return a + b;
    }
    __device__ __forceinline__ long long operator()(long long a, long long b) const { return a + b; }
    __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const {
        return a + b;
    }
};
struct BlockMax {
    __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; }
    __device__ __forceinline__ long long operator()(long long a, long long b) const { return a > b ? a : b; }
    __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const {
        return a > b ? a : b;
    }
};
struct BlockMin {
    __device__ __forceinline__ long long operator()(long long a, long long b) const { return a < b ? a : b; }
};

// v[0..N) of every thread combined with `op` -- lanes by butterfly, then the workgroup's `waves` <= kWaves wavefronts
// in ascending order -- and handed back to every thread.  One barrier per call: the slots alternate between two sets,
// and a set is written again only after the barrier of the call in between.  Every thread of the workgroup calls.
template <int kSlots, int kWaves>
struct BlockReduce {
    static_assert(kWaves >= 1 && kWaves <= 16, "a workgroup has at most 16 wavefronts");
    static constexpr int kWords = 2 * kWaves * kSlots;
    unsigned long long *slots;      // [2][kWaves][kSlots]
    int waves, phase;

    template <typename T, int N, typename Op>
    __device__ __forceinline__ void run(T (&v)[N], Op op) {
        static_assert(sizeof(T) == 8 && N <= kSlots, "64-bit values, at most kSlots of them");
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        unsigned long long *set = slots + (phase & 1) * kWaves * kSlots;
#pragma unroll
        for (int k = 0; k < N; ++k) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v[k] = op(v[k], __shfl_xor(v[k], m, 64));
            if (lane == 0) __builtin_memcpy(&set[wave * kSlots + k], &v[k], 8);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < N; ++k) {
            __builtin_memcpy(&v[k], &set[k], 8);
#pragma unroll
            for (int q = 1; q < kWaves; ++q) {
                if (q >= waves) break;
                T w;
                __builtin_memcpy(&w, &set[q * kSlots + k], 8);
                v[k] = op(v[k], w);
            }
        }
        ++phase;
    }
};

// ---- scans ----------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T lane_up(T v, int d) {              // lane l <- lane l - d; aggregates overload it
    return __shfl_up(v, d, 64);
}
struct ScanAdd {
    template <typename T>
    __device__ __forceinline__ T operator()(T before, T v) const { return before + v; }
};

// inclusive scan over the wavefront's lanes in lane order: op(before, v) joins what stands before a lane to its own
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, Op op) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = lane_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    return v;
}

// inclusive prefix sum over the workgroup's threads; `wsum`: one value per wavefront, free again after the call.
// Every thread of the workgroup calls.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T *wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_scan(v, ScanAdd());
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    for (int q = 0; q < wave; ++q) v += wsum[q];
    __syncthreads();
    return v;
}

// ---- median ---------------------------------------------------------------------------------------------------------
struct MedianLds {
    alignas(16) unsigned hist[256];
    unsigned sel[2];
};

// The median of the n > 0 elements t < m for which key_at(t, key) is true (it then gives the element's order_key), as
// a double: NumPy's mean of the two middle values for an even count.  Exact selection of the middle order statistic by
// eight radix passes over the elements (8-bit digits, histogram in LDS); equal keys are the normal case, and a
// wavefront whose keys all fall into one bin adds once.  An even count takes the largest key below the selected one as
// well, or the same value where it repeats.  Every thread of a workgroup of 256 threads or more calls, behind a
// barrier where key_at reads LDS.
template <typename KeyAt, typename Reduce>
__device__ __forceinline__ double block_median(int m, unsigned n, KeyAt key_at, MedianLds &s, Reduce &red) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, threads = blockDim.x;
    unsigned long long prefix = 0;
    unsigned k = n / 2;                                         // (from 0) among the keys that match the prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) s.hist[tid] = 0;
        __syncthreads();
        const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        for (int t0 = 0; t0 < m; t0 += threads) {               // (the same trips for every thread: the ballots)
            const int t = t0 + tid;
            unsigned long long q = 0;
            const bool act = t < m && key_at(t, q) && (q & himask) == prefix;
            const unsigned bin = (unsigned)(q >> shift) & 255u;
            const unsigned long long mask = __ballot(act);
            if (mask) {
                const int leader = __builtin_ctzll(mask);
                const unsigned b0 = (unsigned)__shfl((int)bin, leader, 64);
                if (__all(!act || bin == b0)) {
                    if (lane == leader) atomicAdd(&s.hist[b0], (unsigned)__popcll(mask));
                } else if (act) {
                    atomicAdd(&s.hist[bin], 1u);
                }
            }
        }
        __syncthreads();
        // the bin that holds the k-th key: exclusive prefix <= k < inclusive prefix.  Wavefront 0, four bins a lane
        if (tid < 64) {
            unsigned c[4], own = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) own += c[j] = s.hist[4 * lane + j];
            unsigned excl = wave_scan(own, ScanAdd()) - own;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (excl <= k && k < excl + c[j]) {
                    s.sel[0] = 4u * lane + j;
                    s.sel[1] = excl;
                }
                excl += c[j];
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)s.sel[0] << shift;
        k -= s.sel[1];
    }
    const unsigned long long hi = prefix;
    if (n & 1) return order_unkey(hi);
    // the element below it: the largest key under `hi`, or `hi` itself where the value repeats
    unsigned long long below[1] = {0}, best[1] = {0};
    for (int t = tid; t < m; t += threads) {
        unsigned long long q = 0;
        if (key_at(t, q) && q < hi) {
            ++below[0];
            best[0] = q > best[0] ? q : best[0];
        }
    }
    red.run(below, BlockAdd());
    red.run(best, BlockMax());
    const unsigned long long lo = below[0] < (unsigned long long)(n / 2) ? hi : best[0];
    return (order_unkey(lo) + order_unkey(hi)) / 2.0;
}

}  // namespace qm
