// leaf_resample.hpp -- windowed-sinc (Hann, polyphase) resampling of leaf_resample_f32 as plain functions, for the device and for the
// host: csrc/inst_resample.hip builds its kernel on them, and tools/resample_check.cpp runs them on the CPU (the host test compares
// its table and outputs with a NumPy oracle; under -fsanitize=undefined,address it walks hostile records).  No HIP header is needed.
//
// The definition is in include/leaf_hip.h (leaf_resample_f32); this file IS that definition in code: the integer plan (gcd, width,
// the span k0 / cnt of a phase, the output length), the clamps of one record, the table (host only, evaluated in double and rounded
// once), and one output -- the span loop as ONE chain acc = fmaf(h, x, acc) from +0.0f, taps ascending, and the int16 quantiser.  The
// chain is generic over where the taps and the samples come from (LDS, global memory, a std::vector): the order is the same
// everywhere, so the bits are.
#pragma once
#include <cstddef>
#include "leaf_segments_view.hpp"

#if !defined(__HIPCC__) && !defined(__CUDACC__)
#include <math.h>
#endif
#if defined(__clang__)
#define LEAF_RESAMPLE_UNROLL _Pragma("unroll")
#else
#define LEAF_RESAMPLE_UNROLL
#endif

constexpr int kResampleTile = 1024;                   // output samples per tile (one workgroup of 256 lanes, four outputs per lane)
constexpr int kResampleMaxRatio = 65535;              // reduced o and n stay at or below this
constexpr long long kResampleMaxTableBytes = 1ll << 26;
constexpr int kResampleHeaderInts = 8;                // magic, o, n, width, stride, taps_in_lds, 0, 0
constexpr int kResampleMagic = 0x3153524c;            // "LRS1"
constexpr int kResampleLdsBudget = 64 * 1024;         // bytes of LDS per workgroup: two workgroups per CU and room to spare (a starting
                                                      // point from the CU's 160 KB, not a measurement)

struct ResamplePlan {
    int o, n;                     // orig_freq / g, new_freq / g
    int W;                        // lowpass_filter_width
    int width;                    // ceil(W o / base); 0 for o == n
    int K;                        // taps per phase before the span: 2 width + o
    double base;                  // min(o, n) rolloff
};

LEAF_HOST_DEVICE inline long long resample_gcd(long long a, long long b) {
    while (b != 0) {
        const long long r = a % b;
        a = b;
        b = r;
    }
    return a;
}

// The plan of (orig_freq, new_freq, W, rolloff), all valid (> 0, > 0, >= 1, in (0, 1]).  False: the reduced ratio or the width is
// beyond what the library takes (LEAF_ERR_UNSUPPORTED).
LEAF_HOST_DEVICE inline bool resample_plan(int orig_freq, int new_freq, int W, double rolloff, ResamplePlan& p) {
    const long long g = resample_gcd(orig_freq, new_freq);
    const long long o = orig_freq / g, n = new_freq / g;
    if (o > kResampleMaxRatio || n > kResampleMaxRatio) return false;
    p.o = (int)o; p.n = (int)n; p.W = W;
    p.base = (double)(o < n ? o : n) * rolloff;
    if (o == n) {                                                         // one phase whose only tap is 1: the identity
        p.width = 0; p.K = 1;
        return true;
    }
    const double w = ceil((double)((long long)W * o) / p.base);
    if (!(w < (double)(kResampleMaxTableBytes / 8))) return false;        // (2 width + o) floats per phase could not fit
    p.width = (int)w;
    p.K = 2 * p.width + p.o;
    return true;
}

// t of tap k of phase p, and whether the tap belongs to the span: |t| < W.  (o == n: tap 0 alone.)
LEAF_HOST_DEVICE inline double resample_tap_time(const ResamplePlan& q, int p, long long k) {
    const long long num = (k - (long long)q.width) * (long long)q.n - (long long)p * (long long)q.o;
    return (double)num * q.base / (double)((long long)q.o * (long long)q.n);
}
LEAF_HOST_DEVICE inline bool resample_in_span(const ResamplePlan& q, int p, long long k) {
    if (k < 0 || k >= q.K) return false;
    if (q.o == q.n) return true;
    const double t = resample_tap_time(q, p, k);
    return (t < 0 ? -t : t) < (double)q.W;
}

// The span of phase p, 0 <= p < n: its first tap k0 and its size cnt >= 1.  The tap nearest to t = 0 is inside (|t| <= 1 / 2 < W) and
// t rises with k, so the span is the run around it: two bisections on the predicate above, nothing else decides a tap.
LEAF_HOST_DEVICE inline void resample_span(const ResamplePlan& q, int p, int& k0, int& cnt) {
    if (q.o == q.n) { k0 = 0; cnt = 1; return; }
    long long c = (long long)q.width + ((long long)p * q.o + q.n / 2) / q.n;   // (k - width) n nearest to p o
    if (c > q.K - 1) c = q.K - 1;
    long long lo = -1, hi = c;                                            // lo outside (or before tap 0), hi inside
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (resample_in_span(q, p, mid)) hi = mid; else lo = mid;
    }
    const long long first = hi;
    lo = c; hi = q.K;                                                     // lo inside, hi outside (or behind the last tap)
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (resample_in_span(q, p, mid)) lo = mid; else hi = mid;
    }
    k0 = (int)first;
    cnt = (int)(lo - first + 1);
}

// ceil(n L / o) for a recording of L samples (L < 0 counts as 0); o, n >= 1.  Saturates instead of overflowing.
LEAF_HOST_DEVICE inline long long resample_length(long long L, long long o, long long n) {
    if (L <= 0) return 0;
    const long long q = L / o, r = L % o, most = 0x7fffffffffffffffll;
    const long long tail = r == 0 ? 0 : (r <= (most - (o - 1)) / n ? (n * r + o - 1) / o : most);   // r < o: n r / o < n + 1 when it fits
    if (q > (most - tail) / n) return most;
    return n * q + tail;
}

// ---- one record, clamped (the header's MEMORY SAFETY rule) ---------------------------------------------------------------------------
struct ResampleRecord {
    long long off;                // first sample in the store, in [0, store_len]
    int L;                        // samples, in [0, store_len - off]
    long long out_off;            // first output sample, in [0, out_total]
    long long out_len;            // min(resample_length(L), out_total - out_off)
};

// store_len, out_total >= 0; o, n in [1, kResampleMaxRatio]
LEAF_HOST_DEVICE inline ResampleRecord resample_record(long long in_off, int in_len, long long store_len, long long out_off,
                                                       long long out_total, int o, int n) {
    const SegmentView v = recording_view(in_off, in_len, store_len);
    ResampleRecord r;
    r.off = v.off;
    r.L = v.L;
    r.out_off = out_off < 0 ? 0 : (out_off > out_total ? out_total : out_off);
    const long long len = resample_length(v.L, o, n), room = out_total - r.out_off;    // len <= 2^31 * 65535: no overflow
    r.out_len = len < room ? len : room;
    return r;
}

// a span read from a table that cannot be trusted, into [0, K): cnt into [0, min(stride, K)], k0 into [0, K - cnt]
LEAF_HOST_DEVICE inline void resample_clamp_span(int& k0, int& cnt, int K, int stride) {
    const int most = stride < K ? stride : K;
    cnt = cnt < 0 ? 0 : (cnt > most ? most : cnt);
    k0 = k0 < 0 ? 0 : (k0 > K - cnt ? K - cnt : k0);
}

// ---- one output ----------------------------------------------------------------------------------------------------------------------
// y = sum over the span, k ascending, of h[k0 + i] x[k0 + i]: one fmaf chain from +0.0f.  h(i): tap k0 + i of the phase; x(k): the
// sample behind tap k (+0.0f outside the recording).  Every tap of the span is applied, zeros included.
template <class Taps, class Samples>
LEAF_HOST_DEVICE inline float resample_output(int k0, int cnt, const Taps& h, const Samples& x) {
    float acc = 0.0f;
    int i = 0;
    for (; i + 8 <= cnt; i += 8) {                                        // the operands of eight taps first, so that their loads are in
        float hv[8], xv[8];                                               // flight together; then the chain, in the same order
        LEAF_RESAMPLE_UNROLL
        for (int e = 0; e < 8; ++e) {
            hv[e] = h(i + e);
            xv[e] = x(k0 + i + e);
        }
        LEAF_RESAMPLE_UNROLL
        for (int e = 0; e < 8; ++e) acc = fmaf(hv[e], xv[e], acc);
    }
    for (; i < cnt; ++i) acc = fmaf(h(i), x(k0 + i), acc);
    return acc;
}

// int16 output: rint(y 32768) to nearest even, saturated to [-32768, 32767]; NaN gives 0
LEAF_HOST_DEVICE inline short resample_quantize(float y) {
    const float s = y * 32768.0f;
    if (!(s == s)) return 0;
    const float q = rintf(s);
    return (short)(int)(q < -32768.0f ? -32768.0f : (q > 32767.0f ? 32767.0f : q));
}

// an int16 sample as the library reads it everywhere: v 2^-15, exact
LEAF_HOST_DEVICE inline float resample_widen(short v) { return (float)(int)v * 0x1p-15f; }

// ---- the table: host only, in double --------------------------------------------------------------------------------------------------
// Layout (int32 / float32 words): kResampleHeaderInts header words, k0[n], cnt[n], then n rows of `stride` taps -- row p holds the
// span's taps h[p][k0 .. k0 + cnt) and zeros behind them.  stride is the largest cnt made odd, so that consecutive phases start in
// different LDS banks.
struct ResampleTableShape {
    int stride;
    long long bytes;              // 0: beyond kResampleMaxTableBytes
};

inline ResampleTableShape resample_table_shape(const ResamplePlan& q) {
    int most = 1;
    for (int p = 0; p < q.n; ++p) {
        int k0, cnt;
        resample_span(q, p, k0, cnt);
        if (cnt > most) most = cnt;
    }
    ResampleTableShape s;
    s.stride = most | 1;
    s.bytes = 4ll * (kResampleHeaderInts + 2ll * q.n + (long long)q.n * s.stride);
    if (s.bytes > kResampleMaxTableBytes) s.bytes = 0;
    return s;
}

// the window the tiles of this plan stage, in samples: a tile of kResampleTile outputs touches at most (tile - 1) / n + 2 input
// strides of o samples (its first output may be any phase) plus the 2 width taps around them
inline long long resample_window_samples(const ResamplePlan& q) {
    return ((long long)(kResampleTile - 1) / q.n + 2) * q.o + 2ll * q.width;
}

// where the tiles read from: the window in LDS when it fits the budget beside the tile's outputs, the taps too when they fit as well
inline void resample_paths(const ResamplePlan& q, const ResampleTableShape& s, bool& window_in_lds, bool& taps_in_lds) {
    const long long win = 4 * (resample_window_samples(q) + kResampleTile);
    window_in_lds = win <= kResampleLdsBudget;
    taps_in_lds = window_in_lds && win + (s.bytes - 4 * kResampleHeaderInts) <= kResampleLdsBudget;
}

// tap k of phase p, inside the span: fp32(sinc(t) cos^2(pi t / (2 W)) base / o)
inline float resample_tap(const ResamplePlan& q, int p, int k) {
    if (q.o == q.n) return 1.0f;
    const double pi = 3.14159265358979323846;
    const double t = resample_tap_time(q, p, k);
    const double s = t == 0.0 ? 1.0 : sin(pi * t) / (pi * t);
    const double c = cos(pi * t / (2.0 * (double)q.W));
    return (float)(s * c * c * q.base / (double)q.o);
}

// the whole table into `words` (s.bytes / 4 of them)
inline void resample_table_fill(const ResamplePlan& q, const ResampleTableShape& s, void* words) {
    int* hdr = static_cast<int*>(words);
    bool win, taps;
    resample_paths(q, s, win, taps);
    hdr[0] = kResampleMagic; hdr[1] = q.o; hdr[2] = q.n; hdr[3] = q.width; hdr[4] = s.stride; hdr[5] = taps ? 1 : 0; hdr[6] = 0; hdr[7] = 0;
    int* k0s = hdr + kResampleHeaderInts;
    int* cnts = k0s + q.n;
    float* h = reinterpret_cast<float*>(cnts + q.n);
    for (int p = 0; p < q.n; ++p) {
        int k0, cnt;
        resample_span(q, p, k0, cnt);
        k0s[p] = k0;
        cnts[p] = cnt;
        float* row = h + (size_t)p * s.stride;
        for (int i = 0; i < s.stride; ++i) row[i] = i < cnt ? resample_tap(q, p, k0 + i) : 0.0f;
    }
}
