// qm_trigger.hpp -- the trigger stage on the device: what the reference's Trigger does to a day's coalescence series
// (quakemigrate/signal/trigger.py:318-638): optional Gaussian smoothing of COA and COA_N, a static or per-chunk
// median / MAD threshold on the trigger series, the maximal runs at or above it (candidates) with the first maximum of
// COA in each, the MinTime / MaxTime rule, and the pairwise merge of candidates into events.  The rules, on arrays:
// tests/trigger_ref.py.  Every output value is a copied sample or an integer: there is no tolerance in this stage.
//
// Seven plain kernels, each its own launch; NO workgroup waits on another one inside a kernel (the per-workgroup run
// counts are scanned by a launch of their own, between the launch that counts and the launch that compacts):
//   trig_smooth_kernel   tiles of kTrigSmoothTile outputs with a 2r halo and the r + 1 weights in LDS, both series in
//                        one launch (blockIdx.y); halo indices by the periodic reflect rule d c b a | a b c d | d c b a
//                        (period 2n: also right for n <= r); SciPy's symmetric summation order, no contraction: its bits
//   trig_stat_kernel     one workgroup per chunk: block_median (qm_block.hpp: eight radix passes over order-preserving
//                        64-bit keys of the samples' bit patterns) with the chunk re-read from global memory (L2) on
//                        every pass; the MAD passes form |x - med| on the fly.  Equal keys are the normal case
//                        (.scanmseed data are quantised to 1e-5)
//   trig_count_kernel    flag[i] = trig[i] >= thr[i / chunk]; run starts (flag[i] and not flag[i - 1]) and ends (flag[i]
//                        and not flag[i + 1]) counted per workgroup of kTrigRunBlock samples, with the non-finite
//                        samples of the two input series
//   trig_scan_kernel     one workgroup: exclusive prefix of the counts with a carried total
//   trig_compact_kernel  the starts and ends in index order: the k-th start pairs with the k-th end
//   trig_peak_kernel     one wavefront per candidate: first maximum of COA over the run (per-lane strict >, butterfly
//                        that keeps the lower index on equal values), then MinTime / MaxTime in int64 nanoseconds
//   trig_merge_kernel    one workgroup looping over the candidates kTrigMergeThreads at a time with a carried prefix:
//                        separation flags, their prefix sum (the event number) and a segmented scan of (first largest
//                        TRIG_COA, smallest MinTime, largest MaxTime, members).  The scan's operator is exact and
//                        associative, so the result does not depend on how the scan is laid out over the wavefronts
//
// Tunables of this stage (compile-time; read-outs of qm_engine_get under the names on the right):
//   kTrigMaxRadius      4096   largest smoothing radius taken ("trigger_max_radius"): halo + weights + tile = 104 KB LDS
//   kTrigSmoothTile     1024   outputs per smoothing workgroup ("trigger_smooth_tile")
//   kTrigRunBlock       2048   samples per workgroup of the run kernels ("trigger_run_block")
//   kTrigMergeThreads    256   candidates per pass of the merge loop ("trigger_merge_stride")
//   kTrigMaxSamples     2^30   longest series taken (indices are 32-bit inside the kernels)
#pragma once
#include "qm_block.hpp"

namespace qm {

constexpr int kTrigMaxRadius = 4096;
constexpr int kTrigSmoothTile = 1024;
constexpr int kTrigSmoothThreads = 256;
constexpr int kTrigStatThreads = 1024;          // (256 for chunks of at most kTrigStatSmall samples)
constexpr int kTrigStatSmall = 8192;
constexpr int kTrigRunThreads = 256;
constexpr int kTrigRunItems = 8;                // consecutive samples per thread
constexpr int kTrigRunBlock = kTrigRunThreads * kTrigRunItems;
constexpr int kTrigMergeThreads = 256;
constexpr int64_t kTrigMaxSamples = (int64_t)1 << 30;
constexpr int kTrigCandColumns = 5;             // f, l, p, MinTime, MaxTime
constexpr int kTrigEventInts = 4;               // p, MinTime, MaxTime, members
constexpr int kTrigEventValues = 3;             // TRIG_COA, COA, COA_NORM
// the stages of a call, as "trigger_timing" times them: smoothing, chunk statistics, run count + scan, compaction,
// peaks, merge
enum TrigStage : int { kTrigSmooth = 0, kTrigStats, kTrigRuns, kTrigCompact, kTrigPeaks, kTrigMerge, kTrigStages };
inline constexpr const char *const kTrigStageNames[kTrigStages] = {"smooth", "stats", "runs", "compact", "peaks", "merge"};

inline size_t trig_smooth_lds_bytes(int r) { return ((size_t)kTrigSmoothTile + 3 * (size_t)r + 1) * sizeof(double); }

struct TrigSmoothArgs {
    const double *x;                // [2][n]
    const double *w;                // [r + 1]: the kernel's first half, w[r] the centre
    double *y;                      // [2][n]
    int n, r;
};

struct TrigStatArgs {
    const double *trig;             // [n]
    double *thr;                    // [chunks]
    int n, chunk, method;           // 1: median + 1.4826 MAD x value, 2: median x value
    double value;
};

struct TrigRunArgs {
    const double *raw;              // [2][n]: the call's input, for the count of non-finite samples
    const double *trig;             // [n]
    const double *thr;              // [chunks]
    int n, chunk, nblocks;
    int32_t *counts;                // [3][nblocks]: starts, ends, non-finite
    int32_t *offsets;               // [2][nblocks]: exclusive prefixes of starts and ends
    int64_t *totals;                // starts, ends, non-finite, events
    int32_t *first, *last;          // [candidates]
};

struct TrigPeakArgs {
    const double *coa, *coa_n, *trig;
    const int32_t *first, *last;
    int64_t *cand;                  // [nc][5]
    double *cval;                   // [nc]: trig[p]
    int64_t *ev_i;                  // [events][4]
    double *ev_f;                   // [events][3]
    int64_t *totals;
    int nc;
    int64_t period, mw, mei;
};

// ---- device helpers (the workgroup's sums, scans and the median: qm_block.hpp) --------------------------------------
using TrigRunReduce = BlockReduce<3, kTrigRunThreads / 64>;    // the run kernels' sums: three counts at most

__device__ __forceinline__ bool trig_flag(const TrigRunArgs &a, int i) {
    return a.trig[i] >= a.thr[(unsigned)i / (unsigned)a.chunk];
}

#ifdef QM_TU_TRIGGER
// ---- smoothing ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrigSmoothThreads) void trig_smooth_kernel(TrigSmoothArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char trig_lds[];
    const int n = a.n, r = a.r, tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kTrigSmoothTile;
    const int outs = (int)(n - base < kTrigSmoothTile ? n - base : kTrigSmoothTile);
    double *tile = reinterpret_cast<double *>(trig_lds);            // [outs + 2r], tile[k] = x(base - r + k)
    double *w = tile + kTrigSmoothTile + 2 * (size_t)r;             // [r + 1]
    const double *x = a.x + (int64_t)blockIdx.y * n;
    const int64_t period = 2 * (int64_t)n;
    for (int k = tid; k < outs + 2 * r; k += kTrigSmoothThreads) {
        int64_t m = (base - r + k) % period;
        if (m < 0) m += period;
        tile[k] = x[m < n ? m : period - 1 - m];
    }
    for (int k = tid; k <= r; k += kTrigSmoothThreads) w[k] = a.w[k];
    __syncthreads();
    double *y = a.y + (int64_t)blockIdx.y * n + base;
    for (int o = tid; o < outs; o += kTrigSmoothThreads) {
        const double *c = tile + o + r;
        double out = c[0] * w[r];
        for (int j = r; j >= 1; --j) out += (c[-j] + c[j]) * w[r - j];
        y[o] = out;
    }
}

// ---- chunk statistics -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrigStatThreads) void trig_stat_kernel(TrigStatArgs a) {
#pragma clang fp contract(off)
    using Reduce = BlockReduce<1, kTrigStatThreads / 64>;
    __shared__ MedianLds s;
    __shared__ unsigned long long slots[Reduce::kWords];
    Reduce red{slots, (int)(blockDim.x >> 6), 0};
    const int64_t c0 = (int64_t)blockIdx.x * a.chunk;
    const int m = (int)(a.n - c0 < a.chunk ? a.n - c0 : a.chunk);
    const double *x = a.trig + c0;
    const double med = block_median(m, (unsigned)m, [&](int t, unsigned long long &q) {
        q = order_key(x[t]);
        return true;
    }, s, red);
    double thr;
    if (a.method == 1) {
        const double mad = 1.4826 * block_median(m, (unsigned)m, [&](int t, unsigned long long &q) {
            q = order_key(fabs(x[t] - med));
            return true;
        }, s, red);
        thr = med + mad * a.value;
    } else {
        thr = med * a.value;
    }
    if (threadIdx.x == 0) a.thr[blockIdx.x] = thr;
}

// ---- runs -----------------------------------------------------------------------------------------------------------
// the flags of a thread's kTrigRunItems samples and of the two samples beside them, as starts and ends
__device__ __forceinline__ void trig_edges(const TrigRunArgs &a, int i0, unsigned &starts, unsigned &ends) {
    starts = ends = 0;
    if (i0 >= a.n) return;
    bool prev = i0 > 0 && trig_flag(a, i0 - 1);
    bool cur = trig_flag(a, i0);
#pragma unroll
    for (int j = 0; j < kTrigRunItems; ++j) {
        const int i = i0 + j;
        if (i >= a.n) break;
        const bool next = i + 1 < a.n && trig_flag(a, i + 1);
        if (cur && !prev) starts |= 1u << j;
        if (cur && !next) ends |= 1u << j;
        prev = cur;
        cur = next;
    }
}

__global__ __launch_bounds__(kTrigRunThreads) void trig_count_kernel(TrigRunArgs a) {
    __shared__ unsigned long long slots[TrigRunReduce::kWords];
    TrigRunReduce red{slots, kTrigRunThreads / 64, 0};
    const int i0 = blockIdx.x * kTrigRunBlock + threadIdx.x * kTrigRunItems;
    unsigned starts, ends;
    trig_edges(a, i0, starts, ends);
    unsigned long long c[3] = {(unsigned long long)__popc(starts), (unsigned long long)__popc(ends), 0ull};
    for (int j = 0; j < kTrigRunItems; ++j) {
        const int i = i0 + j;
        if (i < a.n) c[2] += (isfinite(a.raw[i]) ? 0 : 1) + (isfinite(a.raw[(int64_t)a.n + i]) ? 0 : 1);
    }
    red.run(c, BlockAdd());
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) a.counts[k * a.nblocks + blockIdx.x] = (int32_t)c[k];
}

__global__ __launch_bounds__(kTrigRunThreads) void trig_scan_kernel(TrigRunArgs a) {
    __shared__ unsigned wsum[kTrigRunThreads / 64];
    __shared__ unsigned long long slots[TrigRunReduce::kWords];
    TrigRunReduce red{slots, kTrigRunThreads / 64, 0};
    unsigned carry_s = 0, carry_e = 0;
    unsigned long long bad[1] = {0};
    for (int b0 = 0; b0 < a.nblocks; b0 += kTrigRunThreads) {
        const int b = b0 + threadIdx.x;
        const unsigned cs = b < a.nblocks ? (unsigned)a.counts[b] : 0u;
        const unsigned ce = b < a.nblocks ? (unsigned)a.counts[a.nblocks + b] : 0u;
        bad[0] += b < a.nblocks ? (unsigned long long)a.counts[2 * a.nblocks + b] : 0ull;
        const unsigned is = block_scan(cs, wsum), ie = block_scan(ce, wsum);
        if (b < a.nblocks) {
            a.offsets[b] = (int32_t)(carry_s + is - cs);
            a.offsets[a.nblocks + b] = (int32_t)(carry_e + ie - ce);
        }
        // the tile's totals: the last thread's inclusive sums
        const bool last = threadIdx.x == kTrigRunThreads - 1;
        unsigned long long total[2] = {last ? is : 0u, last ? ie : 0u};
        red.run(total, BlockAdd());
        carry_s += (unsigned)total[0];
        carry_e += (unsigned)total[1];
    }
    red.run(bad, BlockAdd());
    if (threadIdx.x == 0) {
        a.totals[0] = carry_s;
        a.totals[1] = carry_e;
        a.totals[2] = (int64_t)bad[0];
        a.totals[3] = 0;
    }
}

__global__ __launch_bounds__(kTrigRunThreads) void trig_compact_kernel(TrigRunArgs a) {
    __shared__ unsigned wsum[kTrigRunThreads / 64];
    const int i0 = blockIdx.x * kTrigRunBlock + threadIdx.x * kTrigRunItems;
    unsigned starts, ends;
    trig_edges(a, i0, starts, ends);
    const unsigned cs = __popc(starts), ce = __popc(ends);
    unsigned ps = a.offsets[blockIdx.x] + block_scan(cs, wsum) - cs;
    unsigned pe = a.offsets[a.nblocks + blockIdx.x] + block_scan(ce, wsum) - ce;
#pragma unroll
    for (int j = 0; j < kTrigRunItems; ++j) {
        if (starts & (1u << j)) a.first[ps++] = i0 + j;
        if (ends & (1u << j)) a.last[pe++] = i0 + j;
    }
}

// ---- candidates -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trig_peak_kernel(TrigPeakArgs a) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= a.nc) return;                                      // (the whole wavefront)
    const int64_t f = a.first[k], l = a.last[k];
    double best = -__builtin_inf();
    long long at = 0x7fffffffffffffffll;
    for (int64_t i = f + lane; i <= l; i += 64) {               // (a run may be the whole series)
        const double v = a.coa[i];
        if (v > best) {
            best = v;
            at = i;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double v = __shfl_xor(best, m, 64);
        const long long i = __shfl_xor(at, m, 64);
        if (v > best || (v == best && i < at)) {
            best = v;
            at = i;
        }
    }
    if (lane == 0) {
        const int64_t tp = at * a.period, tf = f * a.period, tl = l * a.period, gap = a.mei - a.mw;
        int64_t *row = a.cand + (int64_t)k * kTrigCandColumns;
        row[0] = f;
        row[1] = l;
        row[2] = at;
        row[3] = tp - tf < a.mw ? tp - a.mei : tf - gap;
        row[4] = tl - tp < a.mw ? tp + a.mei : tl + gap;
        a.cval[k] = a.trig[at];
    }
}

// ---- merge ----------------------------------------------------------------------------------------------------------
struct TrigSeg {
    int ev, cnt;
    double val;
    long long p, mn, mx;
};
// `a` stands before `b`; equal values keep the earlier member
__device__ __forceinline__ TrigSeg trig_join(const TrigSeg &a, const TrigSeg &b) {
    if (a.ev != b.ev) return b;
    TrigSeg r = a;
    if (b.val > a.val) {
        r.val = b.val;
        r.p = b.p;
    }
    r.mn = b.mn < a.mn ? b.mn : a.mn;
    r.mx = b.mx > a.mx ? b.mx : a.mx;
    r.cnt = a.cnt + b.cnt;
    return r;
}
struct TrigJoin {
    __device__ __forceinline__ TrigSeg operator()(const TrigSeg &a, const TrigSeg &b) const { return trig_join(a, b); }
};
__device__ __forceinline__ TrigSeg lane_up(const TrigSeg &v, int d) {      // (wave_scan's shuffle, per member)
    return TrigSeg{lane_up(v.ev, d), lane_up(v.cnt, d), lane_up(v.val, d), lane_up(v.p, d), lane_up(v.mn, d),
                   lane_up(v.mx, d)};
}

__global__ __launch_bounds__(kTrigMergeThreads) void trig_merge_kernel(TrigPeakArgs a) {
    __shared__ unsigned wsum[kTrigMergeThreads / 64];
    __shared__ TrigSeg wseg[kTrigMergeThreads / 64];
    __shared__ TrigSeg carry_slot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto peak_time = [&](int k) { return a.cand[(int64_t)k * kTrigCandColumns + 2] * a.period; };
    // candidates k - 1 and k are separate events (trigger.py:602-608)
    auto separate = [&](int k) {
        const int64_t *c0 = a.cand + (int64_t)(k - 1) * kTrigCandColumns, *c1 = c0 + kTrigCandColumns;
        return c0[4] < peak_time(k) - a.mw && c1[3] > peak_time(k - 1) + a.mw;
    };
    TrigSeg carry{};
    for (int k0 = 0; k0 < a.nc; k0 += kTrigMergeThreads) {
        const int k = k0 + tid;
        const bool valid = k < a.nc;
        const unsigned sep = valid && k > 0 && separate(k) ? 1u : 0u;
        const bool ends = valid && (k == a.nc - 1 || separate(k + 1));
        TrigSeg v{};
        v.ev = (k0 > 0 ? carry.ev : 0) + (int)block_scan(sep, wsum);
        if (valid) {
            const int64_t *c = a.cand + (int64_t)k * kTrigCandColumns;
            v.cnt = 1;
            v.val = a.cval[k];
            v.p = c[2];
            v.mn = c[3];
            v.mx = c[4];
        } else {
            v.ev = 0x7fffffff;
        }
        v = wave_scan(v, TrigJoin());
        if (lane == 63) wseg[wave] = v;
        __syncthreads();
        TrigSeg acc = carry;
        bool have = k0 > 0;
        for (int q = 0; q < wave; ++q) {
            acc = have ? trig_join(acc, wseg[q]) : wseg[q];
            have = true;
        }
        if (have) v = trig_join(acc, v);
        if (ends) {
            int64_t *ei = a.ev_i + (int64_t)v.ev * kTrigEventInts;
            double *ef = a.ev_f + (int64_t)v.ev * kTrigEventValues;
            ei[0] = v.p;
            ei[1] = v.mn;
            ei[2] = v.mx;
            ei[3] = v.cnt;
            ef[0] = v.val;
            ef[1] = a.coa[v.p];
            ef[2] = a.coa_n[v.p];
            if (k == a.nc - 1) a.totals[3] = (int64_t)v.ev + 1;
        }
        if (tid == kTrigMergeThreads - 1) carry_slot = v;
        __syncthreads();
        carry = carry_slot;
        __syncthreads();
    }
}
#endif  // QM_TU_TRIGGER

}  // namespace qm
