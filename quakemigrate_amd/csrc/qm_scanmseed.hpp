// qm_scanmseed.hpp -- the day file's codec on the device: the STEIM2 payloads of the .scanmseed records that
// quakemigrate_amd/scanmseed.py writes and reads (miniSEED 2, 4096-byte records, 64 header bytes + 63 frames of 16
// big-endian words; word 0 of a frame holds fifteen 2-bit codes, words 1 and 2 of frame 0 the record's first and last
// sample: 943 data words per record).  The rules, on arrays: tests/scanmseed_ref.py.  Every value is an integer or a
// copied bit pattern: there is no tolerance in this stage.
//
// What makes the greedy packer parallel:
//   - the differences are global: d[0] = 0, d[p] = x[p] - x[p - 1] otherwise, across record boundaries too (64-bit:
//     two int32 samples can differ by more than int32 holds);
//   - count(p), the differences the word that STARTS at p takes, is the first of 7x4, 6x5, 5x6, 4x8, 3x10, 2x15, 1x30
//     bits whose count is <= n - p (the end of the TRACE, not of the record) and whose differences all fit: it depends
//     on the widths of d[p .. p + 6] and on n - p only;
//   - so the words of a trace are ONE chain p -> p + count(p) from p = 0, cut into records every 943 words.
//
// Encode, five launches, NO workgroup waits on another one inside a kernel, no lane walks more than a tile:
//   sms_quantise_kernel  (float64 input only) min(x, clip) * factor, round half to even, int32 -- NumPy's
//                        np.round(np.minimum(x, clip) * factor).astype(int32) wherever that is defined.  A NaN, or a
//                        scaled value outside int32, is REFUSED: NumPy's cast there is platform-defined
//   sms_scan_kernel      per tile of kSmsTile positions: width classes of the tile and a 6-position halo in LDS,
//                        count(p) of every position (kept: one byte each), then seven lanes walk the tile's chain from
//                        the seven possible entry offsets: exit offset into the next tile and words on the way.  A
//                        difference outside 30 bits is refused (the Python raises OverflowError)
//   sms_compose_kernel   one workgroup per channel composes the tiles' 7-entry maps in order, kSmsComposeChunk tiles at
//                        a time through LDS: every tile's true entry offset and first word index, the channel's words
//                        and records
//   -- the counts and the refusals come back to the host here; the output is sized and zeroed --
//   sms_pack_kernel      per tile: one lane walks the tile's chain from the true entry and lists the word starts, then
//                        every lane packs words: word w of the channel goes to record w / 943, slot w % 943 + 2,
//                        byte-swapped; its 2-bit code to a side array; the words that open a record note their position
//   sms_frame_kernel     one lane per frame: word 0 from its fifteen codes; frame 0 also the two integration constants
//                        and the record's sample count.  Unused words and frames of a trace's last record stay zero
// The bytes depend on the input alone: the only atomics are minima of error positions.
//
// Decode, one launch, one workgroup per record (records are independent): codes of word 0 -> per-word counts -> prefix
// sum -> the first n differences -> 64-bit prefix sum from the forward constant -> samples; checked against the
// reverse constant.  An invalid code / dnib pair before the n-th difference, fewer differences than samples or a
// constant mismatch is an error naming the smallest such record (the Python's three ValueErrors, in its order).
//
// Compile-time constants (read-outs of qm_engine_get under the names on the right):
//   kSmsTile          2048   positions per workgroup of the scan and pack kernels ("scanmseed_tile")
//   kSmsComposeChunk  1024   tiles per LDS pass of the compose kernel ("scanmseed_compose_chunk")
//   kSmsMaxSamples    2^28   longest channel taken (5 n positions are indexed in 32 bits by the side arrays' rows)
#pragma once
#include "qm_block.hpp"

namespace qm {

constexpr int kSmsChannels = 5;
constexpr int kSmsRecLen = 4096, kSmsDataOffset = 64;
constexpr int kSmsRecU32 = kSmsRecLen / 4, kSmsHeadU32 = kSmsDataOffset / 4;
constexpr int kSmsFrames = 63;                                  // frames per record
constexpr int kSmsPayloadWords = kSmsFrames * 16;               // 1008
constexpr int kSmsRecWords = kSmsFrames * 15 - 2;               // 943 data words per record
constexpr int kSmsMaxCount = 7;                                 // differences in a word, at most
constexpr int kSmsRecMaxSamples = kSmsRecWords * kSmsMaxCount;  // 6601
constexpr int kSmsTile = 2048;
constexpr int kSmsThreads = 256;
constexpr int kSmsComposeChunk = 1024;
constexpr int64_t kSmsMaxSamples = (int64_t)1 << 28;
// error slots (unsigned 64-bit minima, all ones: none): the first three hold channel * n + position, the last
// record * 4 + kind
enum SmsErr : int { kSmsErrNaN = 0, kSmsErrRange, kSmsErrDiff, kSmsErrDecode, kSmsErrSlots };
enum SmsDecodeKind : int { kSmsBadCode = 0, kSmsShort = 1, kSmsMismatch = 2 };
// the stages "scanmseed_ns_<stage>" times: encode's five launches, the decode launch
enum SmsStage : int { kSmsQuantise = 0, kSmsScan, kSmsCompose, kSmsPack, kSmsFrame, kSmsDecode, kSmsStages };
inline constexpr const char *const kSmsStageNames[kSmsStages] = {"quantise", "scan", "compose", "pack", "frame", "decode"};

struct SmsQuantArgs {
    const double *in;               // [5][n]
    int32_t *out;                   // [5][n]
    int n;
    double factor[kSmsChannels], clip[kSmsChannels];            // clip +inf: none
    unsigned long long *err;
};

struct SmsEncodeArgs {
    const int32_t *x;               // [5][n]
    int n, tiles;
    uint8_t *count;                 // [5][n]: count(p)
    uint8_t *codes;                 // [5][n]: the 2-bit code of word w of the channel (words <= n)
    uint32_t *map;                  // [5][tiles][7]: exit offset << 16 | words, per entry offset
    int32_t *entry, *word0;         // [5][tiles]
    unsigned long long *totals;     // [5] words, [5] records
    unsigned long long *err;
    // from the pack launch on
    uint32_t *out;                  // [records][1024]
    int32_t *rec_first, *rec_count; // [records]
    int rec_off[kSmsChannels + 1];  // the channels' first records
    int words[kSmsChannels];
};

struct SmsDecodeArgs {
    const uint32_t *rec;            // [n_rec][1024]
    const int32_t *rec_n;           // [n_rec]
    const int64_t *rec_out;         // [n_rec]: where the record's samples go
    const double *rec_factor;       // [n_rec] or nullptr
    int32_t *out;                   // [n_total]
    double *outf;                   // [n_total] or nullptr
    unsigned long long *err;
};

// width class of a difference: 0..6 for 4, 5, 6, 8, 10, 15, 30 bits, 7: outside 30 bits
__host__ __device__ __forceinline__ int sms_class(int64_t d) {
    const int64_t m = d < 0 ? ~d : d;                           // d fits b bits iff m < 2^(b - 1)
    return m < 8 ? 0 : m < 16 ? 1 : m < 32 ? 2 : m < 128 ? 3 : m < 512 ? 4 : m < 16384 ? 5 : m < ((int64_t)1 << 29) ? 6 : 7;
}
// the layout of a word of `count` differences: bits per difference, 2-bit code, dnib (top two bits; code 1 has none)
__host__ __device__ __forceinline__ void sms_layout(int count, int &bits, unsigned &code, unsigned &dnib) {
    switch (count) {
        case 7: bits = 4; code = 3; dnib = 2; break;
        case 6: bits = 5; code = 3; dnib = 1; break;
        case 5: bits = 6; code = 3; dnib = 0; break;
        case 4: bits = 8; code = 1; dnib = 0; break;
        case 3: bits = 10; code = 2; dnib = 3; break;
        case 2: bits = 15; code = 2; dnib = 2; break;
        default: bits = 30; code = 2; dnib = 1; break;
    }
}
// slot s of a record's non-code words (0 and 1: the constants, 2..944: data) -> index among the payload's words
__host__ __device__ __forceinline__ int sms_slot_word(int s) { return (s / 15) * 16 + s % 15 + 1; }

#ifdef QM_TU_SCANMSEED
__device__ __forceinline__ uint32_t sms_bswap(uint32_t v) { return __builtin_bswap32(v); }

// ---- encode ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSmsThreads) void sms_quantise_kernel(SmsQuantArgs a) {
#pragma clang fp contract(off)
    const int c = blockIdx.y;
    const double f = a.factor[c], clip = a.clip[c];
    const int64_t row = (int64_t)c * a.n;
    for (int64_t i = (int64_t)blockIdx.x * kSmsThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kSmsThreads) {
        double v = a.in[row + i];
        v = v != v ? v : (clip < v ? clip : v);                 // np.minimum: NaN stays NaN
        v = rint(v * f);                                        // round half to even
        int32_t q = 0;
        if (v != v) atomicMin(&a.err[kSmsErrNaN], (unsigned long long)(row + i));
        else if (v < -2147483648.0 || v > 2147483647.0) atomicMin(&a.err[kSmsErrRange], (unsigned long long)(row + i));
        else q = (int32_t)v;
        a.out[row + i] = q;
    }
}

__global__ __launch_bounds__(kSmsThreads) void sms_scan_kernel(SmsEncodeArgs a) {
    __shared__ uint8_t cls[kSmsTile + 8];
    __shared__ uint8_t cnt[kSmsTile];
    const int c = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, n = a.n;
    const int start = t * kSmsTile;
    const int end = n - start < kSmsTile ? n : start + kSmsTile;
    const int64_t row = (int64_t)c * n;
    const int32_t *x = a.x + row;
    for (int k = tid; k < kSmsTile + kSmsMaxCount - 1; k += kSmsThreads) {
        const int p = start + k;
        int w = 0;
        if (p < n) {
            w = sms_class(p ? (int64_t)x[p] - (int64_t)x[p - 1] : 0);
            if (w == 7 && p < end) atomicMin(&a.err[kSmsErrDiff], (unsigned long long)(row + p));
        }
        cls[k] = (uint8_t)w;
    }
    __syncthreads();
    for (int k = tid; k < end - start; k += kSmsThreads) {
        const int left = n - (start + k);
        int mx[kSmsMaxCount];
        mx[0] = cls[k];
#pragma unroll
        for (int j = 1; j < kSmsMaxCount; ++j) mx[j] = mx[j - 1] > cls[k + j] ? mx[j - 1] : (int)cls[k + j];
        int res = 1;                                            // (a refused difference: the chain still moves on)
#pragma unroll
        for (int i = 0; i < kSmsMaxCount; ++i) {                // layout i: 7 - i differences of class <= i
            const int need = kSmsMaxCount - i;
            if (need <= left && mx[need - 1] <= i) {
                res = need;
                break;
            }
        }
        cnt[k] = (uint8_t)res;
        a.count[row + start + k] = (uint8_t)res;
    }
    __syncthreads();
    if (tid < kSmsMaxCount) {
        int p = start + tid, words = 0;
        while (p < end) {
            p += cnt[p - start];
            ++words;
        }
        const int exit_off = p >= end ? p - end : 0;            // (an entry past a short last tile: never on the chain)
        a.map[((size_t)c * a.tiles + t) * kSmsMaxCount + tid] = ((uint32_t)exit_off << 16) | (uint32_t)words;
    }
}

__global__ __launch_bounds__(kSmsThreads) void sms_compose_kernel(SmsEncodeArgs a) {
    __shared__ uint32_t m[kSmsComposeChunk * kSmsMaxCount];
    __shared__ int32_t ent[kSmsComposeChunk], w0[kSmsComposeChunk];
    const int c = blockIdx.x, tid = threadIdx.x;
    const uint32_t *map = a.map + (size_t)c * a.tiles * kSmsMaxCount;
    int e = 0, w = 0;                                           // (thread 0's: the chain's state between chunks)
    for (int t0 = 0; t0 < a.tiles; t0 += kSmsComposeChunk) {
        const int cnt = a.tiles - t0 < kSmsComposeChunk ? a.tiles - t0 : kSmsComposeChunk;
        for (int k = tid; k < cnt * kSmsMaxCount; k += kSmsThreads) m[k] = map[(size_t)t0 * kSmsMaxCount + k];
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < cnt; ++k) {
                ent[k] = e;
                w0[k] = w;
                const uint32_t u = m[k * kSmsMaxCount + e];
                w += (int)(u & 0xffffu);
                e = (int)(u >> 16);
            }
        }
        __syncthreads();
        for (int k = tid; k < cnt; k += kSmsThreads) {
            a.entry[(size_t)c * a.tiles + t0 + k] = ent[k];
            a.word0[(size_t)c * a.tiles + t0 + k] = w0[k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.totals[c] = (unsigned long long)w;
        a.totals[kSmsChannels + c] = (unsigned long long)((w + kSmsRecWords - 1) / kSmsRecWords);
    }
}

__global__ __launch_bounds__(kSmsThreads) void sms_pack_kernel(SmsEncodeArgs a) {
    __shared__ uint8_t cnt[kSmsTile];
    __shared__ uint16_t starts[kSmsTile];
    __shared__ int n_words;
    const int c = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, n = a.n;
    const int start = t * kSmsTile;
    const int end = n - start < kSmsTile ? n : start + kSmsTile;
    const int64_t row = (int64_t)c * n;
    const int32_t *x = a.x + row;
    for (int k = tid; k < end - start; k += kSmsThreads) cnt[k] = a.count[row + start + k];
    __syncthreads();
    if (tid == 0) {
        int q = a.entry[(size_t)c * a.tiles + t], k = 0;
        while (q < end - start) {
            starts[k++] = (uint16_t)q;
            q += cnt[q];
        }
        n_words = k;
    }
    __syncthreads();
    const int first_word = a.word0[(size_t)c * a.tiles + t];
    for (int k = tid; k < n_words; k += kSmsThreads) {
        const int q = starts[k], p = start + q, cn = cnt[q];
        int bits;
        unsigned code, dnib;
        sms_layout(cn, bits, code, dnib);
        const uint32_t mask = (1u << bits) - 1u;
        uint32_t word = 0;
        for (int i = 0; i < cn; ++i) {                          // (the masked low bits of the 64-bit difference)
            const int pi = p + i;
            const uint32_t d = pi ? (uint32_t)x[pi] - (uint32_t)x[pi - 1] : 0u;
            word = (word << bits) | (d & mask);
        }
        word |= dnib << 30;
        const int w = first_word + k;
        const int r = w / kSmsRecWords, s = w % kSmsRecWords + 2;
        const size_t rec = (size_t)a.rec_off[c] + r;
        a.out[rec * kSmsRecU32 + kSmsHeadU32 + sms_slot_word(s)] = sms_bswap(word);
        a.codes[row + w] = (uint8_t)code;
        if (s == 2) a.rec_first[rec] = p;
    }
}

__global__ __launch_bounds__(64) void sms_frame_kernel(SmsEncodeArgs a) {
    const int rec = blockIdx.x, f = threadIdx.x;
    if (f >= kSmsFrames) return;
    int c = 0;
    while (c < kSmsChannels - 1 && rec >= a.rec_off[c + 1]) ++c;
    const int r = rec - a.rec_off[c];
    const int64_t row = (int64_t)c * a.n;
    uint32_t w0 = 0;
#pragma unroll
    for (int k = 1; k <= 15; ++k) {
        const int s = f * 15 + k - 1;
        if (s < 2) continue;
        const int64_t w = (int64_t)r * kSmsRecWords + s - 2;
        if (w < a.words[c]) w0 |= (uint32_t)a.codes[row + w] << (30 - 2 * k);
    }
    uint32_t *frame = a.out + (size_t)rec * kSmsRecU32 + kSmsHeadU32 + f * 16;
    frame[0] = sms_bswap(w0);
    if (f == 0) {
        const int first = a.rec_first[rec];
        const int next = rec + 1 < a.rec_off[c + 1] ? a.rec_first[rec + 1] : a.n;
        frame[1] = sms_bswap((uint32_t)a.x[row + first]);
        frame[2] = sms_bswap((uint32_t)a.x[row + next - 1]);
        a.rec_count[rec] = next - first;
    }
}

// ---- decode ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSmsThreads) void sms_decode_kernel(SmsDecodeArgs a) {
#pragma clang fp contract(off)
    __shared__ uint32_t w[kSmsPayloadWords];
    __shared__ int32_t diffs[kSmsRecMaxSamples + 7];
    __shared__ int wsum[4];
    __shared__ long long wsum64[4];
    __shared__ int bad, total;
    constexpr int kPer = 4;                                     // data words per thread: 4 x 256 >= 943
    const int rec = blockIdx.x, tid = threadIdx.x, n = a.rec_n[rec];
    const uint32_t *src = a.rec + (size_t)rec * kSmsRecU32 + kSmsHeadU32;
    for (int k = tid; k < kSmsPayloadWords; k += kSmsThreads) w[k] = sms_bswap(src[k]);
    if (tid == 0) bad = 0;
    __syncthreads();
    const long long x0 = (int32_t)w[1], xn = (int32_t)w[2];
    int cn[kPer], bits[kPer], invalid = 0, mine = 0;
    uint32_t v[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int j = tid * kPer + i;
        cn[i] = 0;
        bits[i] = 0;
        v[i] = 0;
        if (j >= kSmsRecWords) continue;
        const int s = j + 2, fw = (s / 15) * 16, k = s % 15 + 1;
        const unsigned code = (w[fw] >> (30 - 2 * k)) & 3u;
        v[i] = w[fw + k];
        const unsigned dnib = v[i] >> 30;
        if (code == 1) { cn[i] = 4; bits[i] = 8; }
        else if (code == 2 && dnib == 1) { cn[i] = 1; bits[i] = 30; }
        else if (code == 2 && dnib == 2) { cn[i] = 2; bits[i] = 15; }
        else if (code == 2 && dnib == 3) { cn[i] = 3; bits[i] = 10; }
        else if (code == 3 && dnib == 0) { cn[i] = 5; bits[i] = 6; }
        else if (code == 3 && dnib == 1) { cn[i] = 6; bits[i] = 5; }
        else if (code == 3 && dnib == 2) { cn[i] = 7; bits[i] = 4; }
        else if (code != 0) invalid |= 1 << i;
        mine += cn[i];
    }
    const int incl = block_scan(mine, wsum);
    int at = incl - mine;                                       // differences before this thread's words
    if (tid == kSmsThreads - 1) total = incl;
    // the Python stops reading at the n-th difference: an invalid pair behind it is not looked at
#pragma unroll
    for (int i = 0, b = at; i < kPer; ++i) {
        if ((invalid >> i & 1) && b < n) bad = 1;
        b += cn[i];
    }
    __syncthreads();
    if (bad || total < n) {                                     // (the whole workgroup)
        if (tid == 0)
            atomicMin(&a.err[kSmsErrDecode], (unsigned long long)rec * 4 + (bad ? kSmsBadCode : kSmsShort));
        return;
    }
    // here n <= total <= kSmsRecMaxSamples: the writes below stay inside diffs[] and inside the record's n outputs
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        for (int q = 0; q < cn[i]; ++q) {
            if (at + q >= n) break;
            const uint32_t field = (v[i] >> ((cn[i] - 1 - q) * bits[i])) & ((1u << bits[i]) - 1u);
            diffs[at + q] = (int32_t)(field << (32 - bits[i])) >> (32 - bits[i]);     // sign extension
        }
        at += cn[i];
    }
    __syncthreads();
    const int per = (n + kSmsThreads - 1) / kSmsThreads;
    const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += i ? diffs[i] : 0;      // (difference 0 is not used: sample 0 is x0)
    long long run = x0 + block_scan(sum, wsum64) - sum;
    const int64_t base = a.rec_out[rec];
    const double factor = a.rec_factor ? a.rec_factor[rec] : 1.0;
    for (int i = lo; i < hi; ++i) {
        run += i ? diffs[i] : 0;
        const int32_t smp = (int32_t)run;
        a.out[base + i] = smp;
        if (a.outf) a.outf[base + i] = (double)smp / factor;
        if (i == n - 1 && run != xn) atomicMin(&a.err[kSmsErrDecode], (unsigned long long)rec * 4 + kSmsMismatch);
    }
}
#endif  // QM_TU_SCANMSEED

}  // namespace qm
