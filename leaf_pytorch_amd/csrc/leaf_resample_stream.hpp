// leaf_resample_stream.hpp -- where a CHUNKED resampler stands, on integers alone (leaf_resample_stream_plan, the checks of
// leaf_resample_stream_step_f32), for the host and the device: csrc/inst_resample.hip calls these functions, and
// tools/resample_stream_check.cpp runs them on the CPU chunk by chunk (tests/test_host_resample_stream.py compares them with a Python
// oracle and the chunked outputs with the whole-signal tool's).  No HIP header is needed.
//
// The definition is in include/leaf_hip.h (leaf_resample_stream_step_f32).  An output of leaf_resample_f32 is a pure function of the
// recording -- one fmaf chain over its span -- so a stream only has to know WHICH samples an output reads.  In a step the stream's
// signal is the virtual buffer V = [history (hist_len samples) | chunk (Tc samples)], Lv = hist_len + Tc.  WINDOW COORDINATE c means
// "tap c of group 0", group 0 being the group (the o input samples and n outputs of one period of the ratio) of the next output to
// emit; `shift` virtual +0.0f samples stand in front of V[0] (width of them when a stream begins: the recording starts at its first
// sample), so coordinate c is V[c - shift], and E = shift + Lv is one past the last sample that has arrived.  Output t, counted from
// phase 0 of group 0 (t = g n + p), reads the coordinates g o + k0[p] .. g o + klast[p].
#pragma once
#include "leaf_resample.hpp"

constexpr int kResampleStreamMaxChunk = 1 << 20;      // samples one slot takes in one step

// the last tap of phase p's span; non-decreasing in p, and klast[n - 1] - klast[0] <= o: the last sample an output reads never falls
// with t
LEAF_HOST_DEVICE inline int resample_klast(const ResamplePlan& q, int p) {
    int k0, cnt;
    resample_span(q, p, k0, cnt);
    return k0 + cnt - 1;
}

// has every sample of output t (t >= 0) arrived?
LEAF_HOST_DEVICE inline bool resample_stream_complete(const ResamplePlan& q, long long t, long long E) {
    const long long g = t / q.n;
    return g * q.o + resample_klast(q, (int)(t - g * q.n)) <= E - 1;
}

// The outputs a step emits, from t = phase on.  Running: every output whose whole span has arrived -- per output, not per group; the
// predicate falls once and stays down, so the count is found by bisection below the first group that begins at or behind E.  At the
// end of a stream: every remaining output of the recording, (g n + p) o < n (E - width) -- ceil(n T / o) in relative terms; samples
// at or behind E count as +0.0f.  0 <= shift, 0 <= Lv, 0 <= phase < n.
LEAF_HOST_DEVICE inline long long resample_stream_count(const ResamplePlan& q, int shift, long long Lv, int phase, bool end) {
    const long long E = (long long)shift + Lv;
    if (end) {
        const long long all = resample_length(E - q.width, q.o, q.n);
        return all > phase ? all - phase : 0;
    }
    if (E <= 0) return 0;
    long long lo = (long long)phase - 1, hi = ((E - 1) / q.o + 1) * q.n;   // every t <= lo is complete (none is), t = hi is not
    if (hi <= phase) return 0;
    // A guess first -- klast[p] is about width + p o / n + W o / base, so the last complete t is about (E - 1 - that) n / o -- and a
    // gallop away from it: the bracket is narrow before the bisection begins.  The guess decides nothing: the predicate does.
    const double reach = (double)q.width + (q.o == q.n ? 0.0 : (double)((long long)q.W * q.o) / q.base);
    const double at = ((double)(E - 1) - reach) * (double)q.n / (double)q.o;
    long long t = at < (double)(lo + 1) ? lo + 1 : (at > (double)(hi - 1) ? hi - 1 : (long long)at);
    if (resample_stream_complete(q, t, E)) {
        lo = t;
        for (long long step = 1; lo + step < hi; step *= 2) {
            if (!resample_stream_complete(q, lo + step, E)) { hi = lo + step; break; }
            lo += step;
        }
    } else {
        hi = t;
        for (long long step = 1; hi - step > lo; step *= 2) {
            if (resample_stream_complete(q, hi - step, E)) { lo = hi - step; break; }
            hi -= step;
        }
    }
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (resample_stream_complete(q, mid, E)) lo = mid; else hi = mid;
    }
    return hi - phase;
}

// where a stream stands between two steps
struct ResampleStreamPos {
    int hist_len, shift, phase;
};
inline ResampleStreamPos resample_stream_begin(const ResamplePlan& q) { return ResampleStreamPos{0, q.width, 0}; }

// one step: what it emits, what it drops, and where the stream stands behind it
struct ResampleStreamMove {
    long long n;                  // outputs emitted
    long long drop;               // V[drop, Lv) is the next step's history (end: drop = Lv, nothing is kept)
    ResampleStreamPos next;
};

// The hand-over: the next output is (G, p'), and the new origin is window coordinate G o.  G is the group of the last output emitted
// or the one behind it, and G o <= E (the last phase's span ends at or behind tap o - 1), so drop <= Lv.
LEAF_HOST_DEVICE inline ResampleStreamMove resample_stream_move(const ResamplePlan& q, const ResampleStreamPos& at, int Tc, bool end) {
    const long long Lv = (long long)at.hist_len + Tc;
    ResampleStreamMove m;
    m.n = resample_stream_count(q, at.shift, Lv, at.phase, end);
    if (end) {
        m.drop = Lv;
        m.next = ResampleStreamPos{0, q.width, 0};
        return m;
    }
    const long long t = at.phase + m.n, G = t / q.n, Go = G * q.o;
    long long drop = Go > at.shift ? Go - at.shift : 0;
    if (drop > Lv) drop = Lv;
    m.drop = drop;
    m.next.hist_len = (int)(Lv - drop);
    m.next.shift = Go < at.shift ? (int)(at.shift - Go) : 0;
    m.next.phase = (int)(t - G * q.n);
    return m;
}

// One slot's record as leaf_resample_stream_step_f32 checks it, in the header's order.  0: fine; otherwise the number of the first
// check that fails: 1 hist_len <= H = K - 1, 2 shift <= width, 3 phase < n, 4 Tc, parity and end in range, 5 drop_samples <= Lv and
// what is kept fits the history, 6 n <= n_max, 7 n is what the rule gives.  Everything an address is derived from passes here.
LEAF_HOST_DEVICE inline int resample_stream_slot_bad(const ResamplePlan& q, int hist_len, int Tc, int parity, int shift, int phase, int n,
                                                     int drop_samples, int end, int n_max) {
    const int H = q.K - 1;
    if (hist_len < 0 || hist_len > H) return 1;
    if (shift < 0 || shift > q.width) return 2;
    if (phase < 0 || phase >= q.n) return 3;
    if (Tc < 0 || Tc > kResampleStreamMaxChunk || (parity & ~1) || (end & ~1)) return 4;
    const long long Lv = (long long)hist_len + Tc;
    if (drop_samples < 0 || drop_samples > Lv || (!end && Lv - drop_samples > H)) return 5;
    if (n < 0 || n > n_max) return 6;
    if (resample_stream_count(q, shift, Lv, phase, end != 0) != n) return 7;
    return 0;
}

// ---- the window of a step ------------------------------------------------------------------------------------------------------------
// Window coordinate c (any value) as the place of its sample: -1 for +0.0f (in front of the stream or behind what has arrived),
// v in [0, hist_len) for history sample v, hist_len + u for chunk sample u in [0, Tc).
LEAF_HOST_DEVICE inline long long resample_stream_source(long long c, int shift, int hist_len, int Tc) {
    const long long v = c - shift;
    return v < 0 || v >= (long long)hist_len + Tc ? -1 : v;
}
