// leaf_segments_view.hpp -- the clamped plan of one row of leaf_assemble_segments_f32 (and of one recording of leaf_clip_peaks_f32)
// as plain integer functions, for the device and for the host: csrc/leaf_clips.hpp builds its kernels on them, and
// tools/segment_view_check.cpp runs them over hostile plans on the CPU under -fsanitize=undefined.  No HIP header is needed.
//
// Every operand is brought into a range where the next operation cannot overflow BEFORE that operation: nothing here adds or
// subtracts two unclamped values.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEAF_HOST_DEVICE __host__ __device__
#else
#define LEAF_HOST_DEVICE
#endif

struct SegmentView {
    long long off;                // first sample of the recording in the store, in [0, store_len]
    int L;                        // its samples, in [0, store_len - off]
    int left;                     // -win, win clamped into [-S, L]: row element t is the recording's sample t - left
};

// the recording alone (the header's MEMORY SAFETY rule, the clamps of leaf_assemble_clips_f32); store_len >= 0
LEAF_HOST_DEVICE inline SegmentView recording_view(long long rec_off, int rec_len, long long store_len) {
    SegmentView v;
    v.off = rec_off < 0 ? 0 : (rec_off > store_len ? store_len : rec_off);
    const long long len = rec_len, most = store_len - v.off;              // 0 <= most <= store_len
    v.L = (int)(len < 0 ? 0 : (len > most ? most : len));                 // <= rec_len: it fits an int
    v.left = 0;
    return v;
}

// ... and the window of S >= 1 samples that starts at the recording's sample `win` (before it, inside it or behind it)
LEAF_HOST_DEVICE inline SegmentView segment_view(long long rec_off, int rec_len, long long win, long long store_len, int S) {
    SegmentView v = recording_view(rec_off, rec_len, store_len);
    const long long lo = -(long long)S, hi = v.L;
    const long long w = win < lo ? lo : (win > hi ? hi : win);            // a window beyond either end reads what this one reads
    v.left = (int)-w;                                                     // in [-L, S]
    return v;
}

// the recording's sample behind row element t, 0 <= t < S, by the 'replicate' rule: clamp(win + t, 0, L - 1); needs L >= 1
LEAF_HOST_DEVICE inline long long segment_source(const SegmentView& v, long long t) {
    const long long j = t - (long long)v.left, last = (long long)v.L - 1;
    return j < 0 ? 0 : (j > last ? last : j);
}

// the entry of peaks[0, R) a row scales by (and of moments[0, R) a clip or a row is standardised by); R >= 1
LEAF_HOST_DEVICE inline int segment_peak_index(int rec, int R) {
    return rec < 0 ? 0 : (rec > R - 1 ? R - 1 : rec);
}

// leaf_clip_moments_f32: the fixed split of a recording's reductions.  A recording of L samples is ceil(L / 1024) tiles; its tiles
// are dealt to kMomentSpans spans of `per` = ceil(tiles / kMomentSpans) consecutive tiles each (the last ones may be empty).  The
// split depends on L alone -- not on the grid, the store or the other recordings -- so the order of every addition is fixed by it.
constexpr int kMomentTile = 1024;
constexpr int kMomentSpans = 32;

struct MomentSpan {
    long long begin, end;         // the recording's samples [begin, end), 0 <= begin, end <= L; begin >= end: an empty span
};

// span k, 0 <= k < kMomentSpans, of a recording of L >= 0 samples (k and L outside are clamped)
LEAF_HOST_DEVICE inline MomentSpan moment_span(int L, int k) {
    const long long len = L < 0 ? 0 : L, kk = k < 0 ? 0 : (k > kMomentSpans - 1 ? kMomentSpans - 1 : k);
    const long long tiles = (len + kMomentTile - 1) / kMomentTile;        // <= 2^21
    const long long per = (tiles + kMomentSpans - 1) / kMomentSpans;      // <= 2^16
    MomentSpan s;
    s.begin = kk * per * kMomentTile;                                     // <= 2^31: 64 bits hold it
    s.end = s.begin + per * kMomentTile;
    if (s.begin > len) s.begin = len;
    if (s.end > len) s.end = len;
    return s;
}
