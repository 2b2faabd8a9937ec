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

// the entry of peaks[0, R) a row scales by; R >= 1
LEAF_HOST_DEVICE inline int segment_peak_index(int rec, int R) {
    return rec < 0 ? 0 : (rec > R - 1 ? R - 1 : rec);
}
