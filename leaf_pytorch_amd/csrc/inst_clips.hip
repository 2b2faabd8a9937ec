// inst_clips.hip -- batch assembly from a packed sample store: the kernels of leaf_clips.hpp and their C-ABI entries.
// One of the translation units of libleaf_hip.so; it shares nothing with the others but the header's declarations.
#include "leaf_clips.hpp"

// include/leaf_hip.h: the argument checks come first (status only, nothing launched), one launch of B workgroups follows
int leaf_assemble_clips_f32(const void* store, long long store_len, int flags, int B, int size,
                            const long long* rec_off, const int* rec_len, const int* start, const int* pad_mode,
                            const float* gain, int normalize, const int* masks, int M, float* out, void* stream) {
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;          // fp32 or 16-bit PCM in, fp32 out
    if (!store || !rec_off || !rec_len || !start || !pad_mode || !out) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || size < 1 || store_len < 0 || M < 0 || (M > 0 && !masks)) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) || misaligned(start, 3u) ||
        misaligned(pad_mode, 3u) || misaligned(gain, 3u) || misaligned(masks, 3u) || misaligned(out, 3u))
        return LEAF_ERR_ALIGNMENT;
    ClipParams p{};
    p.store = store; p.store_len = store_len;
    p.rec_off = rec_off; p.rec_len = rec_len; p.start = start; p.pad_mode = pad_mode;
    p.gain = gain; p.masks = M > 0 ? masks : nullptr; p.out = out;
    p.S = size; p.M = M; p.normalize = normalize != 0;
    if (pcm) hipLaunchKernelGGL(assemble_clips_kernel<true>, dim3(B), dim3(kClipThreads), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(assemble_clips_kernel<false>, dim3(B), dim3(kClipThreads), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// ... with background noise at an SNR and / or Gaussian noise in the same launch.  Each group is there or NULL as a whole (a
// partly given group is LEAF_ERR_NULL_POINTER); without both the call is the entry above.
int leaf_assemble_clips_noise_f32(const void* store, long long store_len, int flags, int B, int size,
                                  const long long* rec_off, const int* rec_len, const int* start, const int* pad_mode,
                                  const float* gain, int normalize, const int* masks, int M, float* out,
                                  const void* noise_store, long long noise_store_len, const long long* noise_off, const int* noise_len,
                                  const int* noise_start, const int* noise_pad_mode, const float* noise_coeff,
                                  const float* gauss_amp, unsigned long long gauss_seed, const long long* gauss_stream, void* stream) {
    const bool any_noise = noise_store || noise_off || noise_len || noise_start || noise_pad_mode || noise_coeff;
    const bool any_gauss = gauss_amp || gauss_stream;
    if (!any_noise && !any_gauss)
        return leaf_assemble_clips_f32(store, store_len, flags, B, size, rec_off, rec_len, start, pad_mode, gain, normalize, masks, M, out, stream);
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;
    if (!store || !rec_off || !rec_len || !start || !pad_mode || !out) return LEAF_ERR_NULL_POINTER;
    if (any_noise && !(noise_store && noise_off && noise_len && noise_start && noise_pad_mode && noise_coeff)) return LEAF_ERR_NULL_POINTER;
    if (any_gauss && !(gauss_amp && gauss_stream)) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || size < 1 || store_len < 0 || M < 0 || (M > 0 && !masks) || (any_noise && noise_store_len < 0)) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) || misaligned(start, 3u) ||
        misaligned(pad_mode, 3u) || misaligned(gain, 3u) || misaligned(masks, 3u) || misaligned(out, 3u) ||
        misaligned(noise_store, pcm ? 1u : 3u) || misaligned(noise_off, 7u) || misaligned(noise_len, 3u) || misaligned(noise_start, 3u) ||
        misaligned(noise_pad_mode, 3u) || misaligned(noise_coeff, 3u) || misaligned(gauss_amp, 3u) || misaligned(gauss_stream, 7u))
        return LEAF_ERR_ALIGNMENT;
    ClipParams p{};
    p.store = store; p.store_len = store_len;
    p.rec_off = rec_off; p.rec_len = rec_len; p.start = start; p.pad_mode = pad_mode;
    p.gain = gain; p.masks = M > 0 ? masks : nullptr; p.out = out;
    p.S = size; p.M = M; p.normalize = normalize != 0;
    ClipNoiseParams np{};
    np.store = noise_store; np.store_len = noise_store_len;
    np.rec_off = noise_off; np.rec_len = noise_len; np.start = noise_start; np.pad_mode = noise_pad_mode; np.coeff = noise_coeff;
    np.amp = gauss_amp; np.stream = gauss_stream; np.seed = gauss_seed;
    const dim3 grid(B), block(kClipThreads);
    const hipStream_t st = (hipStream_t)stream;
    switch ((pcm ? 4 : 0) | (any_noise ? 2 : 0) | (any_gauss ? 1 : 0)) {
        case 1: hipLaunchKernelGGL((assemble_clips_noise_kernel<false, false, true>), grid, block, 0, st, p, np); break;
        case 2: hipLaunchKernelGGL((assemble_clips_noise_kernel<false, true, false>), grid, block, 0, st, p, np); break;
        case 3: hipLaunchKernelGGL((assemble_clips_noise_kernel<false, true, true>), grid, block, 0, st, p, np); break;
        case 5: hipLaunchKernelGGL((assemble_clips_noise_kernel<true, false, true>), grid, block, 0, st, p, np); break;
        case 6: hipLaunchKernelGGL((assemble_clips_noise_kernel<true, true, false>), grid, block, 0, st, p, np); break;
        default: hipLaunchKernelGGL((assemble_clips_noise_kernel<true, true, true>), grid, block, 0, st, p, np); break;
    }
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// ... on the standardised recording.  The group (moments, moments_rec) is there or NULL as a whole; without it the call is the
// entry above (which, without its own groups, is the plain one).
int leaf_assemble_clips_std_f32(const void* store, long long store_len, int flags, int B, int size,
                                const long long* rec_off, const int* rec_len, const int* start, const int* pad_mode,
                                const float* gain, int normalize, const int* masks, int M, float* out,
                                const void* noise_store, long long noise_store_len, const long long* noise_off, const int* noise_len,
                                const int* noise_start, const int* noise_pad_mode, const float* noise_coeff,
                                const float* gauss_amp, unsigned long long gauss_seed, const long long* gauss_stream,
                                const float* moments, const int* moments_rec, int R, void* stream) {
    if (!moments && !moments_rec)
        return leaf_assemble_clips_noise_f32(store, store_len, flags, B, size, rec_off, rec_len, start, pad_mode, gain, normalize, masks, M, out,
                                             noise_store, noise_store_len, noise_off, noise_len, noise_start, noise_pad_mode, noise_coeff,
                                             gauss_amp, gauss_seed, gauss_stream, stream);
    const bool any_noise = noise_store || noise_off || noise_len || noise_start || noise_pad_mode || noise_coeff;
    const bool any_gauss = gauss_amp || gauss_stream;
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;
    if (!store || !rec_off || !rec_len || !start || !pad_mode || !out) return LEAF_ERR_NULL_POINTER;
    if (any_noise && !(noise_store && noise_off && noise_len && noise_start && noise_pad_mode && noise_coeff)) return LEAF_ERR_NULL_POINTER;
    if (any_gauss && !(gauss_amp && gauss_stream)) return LEAF_ERR_NULL_POINTER;
    if (!moments || !moments_rec) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || size < 1 || store_len < 0 || M < 0 || (M > 0 && !masks) || (any_noise && noise_store_len < 0) || R < 1) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) || misaligned(start, 3u) ||
        misaligned(pad_mode, 3u) || misaligned(gain, 3u) || misaligned(masks, 3u) || misaligned(out, 3u) ||
        misaligned(noise_store, pcm ? 1u : 3u) || misaligned(noise_off, 7u) || misaligned(noise_len, 3u) || misaligned(noise_start, 3u) ||
        misaligned(noise_pad_mode, 3u) || misaligned(noise_coeff, 3u) || misaligned(gauss_amp, 3u) || misaligned(gauss_stream, 7u) ||
        misaligned(moments, 3u) || misaligned(moments_rec, 3u))
        return LEAF_ERR_ALIGNMENT;
    ClipParams p{};
    p.store = store; p.store_len = store_len;
    p.rec_off = rec_off; p.rec_len = rec_len; p.start = start; p.pad_mode = pad_mode;
    p.gain = gain; p.masks = M > 0 ? masks : nullptr; p.out = out;
    p.S = size; p.M = M; p.normalize = normalize != 0;
    ClipNoiseParams np{};
    np.store = noise_store; np.store_len = noise_store_len;
    np.rec_off = noise_off; np.rec_len = noise_len; np.start = noise_start; np.pad_mode = noise_pad_mode; np.coeff = noise_coeff;
    np.amp = gauss_amp; np.stream = gauss_stream; np.seed = gauss_seed;
    ClipStdParams sp{};
    sp.moments = moments; sp.rec = moments_rec; sp.R = R;
    const dim3 grid(B), block(kClipThreads);
    const hipStream_t st = (hipStream_t)stream;
    switch ((pcm ? 4 : 0) | (any_noise ? 2 : 0) | (any_gauss ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((assemble_clips_std_kernel<false, false, false>), grid, block, 0, st, p, np, sp); break;
        case 1: hipLaunchKernelGGL((assemble_clips_std_kernel<false, false, true>), grid, block, 0, st, p, np, sp); break;
        case 2: hipLaunchKernelGGL((assemble_clips_std_kernel<false, true, false>), grid, block, 0, st, p, np, sp); break;
        case 3: hipLaunchKernelGGL((assemble_clips_std_kernel<false, true, true>), grid, block, 0, st, p, np, sp); break;
        case 4: hipLaunchKernelGGL((assemble_clips_std_kernel<true, false, false>), grid, block, 0, st, p, np, sp); break;
        case 5: hipLaunchKernelGGL((assemble_clips_std_kernel<true, false, true>), grid, block, 0, st, p, np, sp); break;
        case 6: hipLaunchKernelGGL((assemble_clips_std_kernel<true, true, false>), grid, block, 0, st, p, np, sp); break;
        default: hipLaunchKernelGGL((assemble_clips_std_kernel<true, true, true>), grid, block, 0, st, p, np, sp); break;
    }
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// the stream on its own: z[b][t] for t in [0, size), the values the entry above adds (times gauss_amp[b])
int leaf_gaussian_noise_f32(int B, int size, unsigned long long seed, const long long* stream_ids, float* out, void* stream) {
    if (!stream_ids || !out) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || size < 1) return LEAF_ERR_BAD_SHAPE;
    const int tiles = (int)((((long long)size + 3) / 4 + 255) / 256);
    if ((long long)B * tiles > 0x7fffffffll) return LEAF_ERR_BAD_SHAPE;
    if ((reinterpret_cast<uintptr_t>(stream_ids) & 7u) || (reinterpret_cast<uintptr_t>(out) & 3u)) return LEAF_ERR_ALIGNMENT;
    hipLaunchKernelGGL(gaussian_noise_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, (hipStream_t)stream, size, tiles, seed, stream_ids, out);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// max |r_i| per recording: the tile prefix (one workgroup), then the tiles (two launches, one call per dataset)
size_t leaf_clip_peaks_workspace_bytes(int R) { return R < 1 ? 0 : sizeof(long long) * ((size_t)R + 1); }

int leaf_clip_peaks_f32(const void* store, long long store_len, int flags, int R, const long long* rec_off, const int* rec_len,
                        float* peaks, void* workspace, size_t workspace_bytes, void* stream) {
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;
    if (!store || !rec_off || !rec_len || !peaks) return LEAF_ERR_NULL_POINTER;
    if (R < 1 || store_len < 0) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) || misaligned(peaks, 3u) || misaligned(workspace, 15u))
        return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < leaf_clip_peaks_workspace_bytes(R)) return LEAF_ERR_WORKSPACE;
    PeakParams p{};
    p.store = store; p.store_len = store_len; p.rec_off = rec_off; p.rec_len = rec_len; p.peaks = peaks;
    p.tile_start = static_cast<long long*>(workspace); p.R = R;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(clip_peaks_plan_kernel, dim3(1), dim3(kClipThreads), 0, st, p);
    // the host does not see the plan: recordings that do not overlap have at most R + store_len / tile tiles, and a plan with more
    // is walked by the same waves
    const long long tiles = (long long)R + store_len / kPeakTile, per_block = kPeakThreads / 64;
    const long long blocks = std::min<long long>((tiles + per_block - 1) / per_block, kPeakMaxBlocks);
    if (pcm) hipLaunchKernelGGL(clip_peaks_kernel<true>, dim3((unsigned)blocks), dim3(kPeakThreads), 0, st, p);
    else hipLaunchKernelGGL(clip_peaks_kernel<false>, dim3((unsigned)blocks), dim3(kPeakThreads), 0, st, p);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// the rows of whole recordings, test.py's pad_input: one launch of rows x tiles workgroups
int leaf_assemble_segments_f32(const void* store, long long store_len, int flags, int rows, int size, const long long* rec_off,
                               const int* rec_len, const long long* win, const float* peaks, const int* rec, int R, float* out,
                               void* stream) {
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;
    if (!store || !rec_off || !rec_len || !win || !out || (peaks && !rec)) return LEAF_ERR_NULL_POINTER;
    if (rows < 1 || size < 1 || store_len < 0 || (peaks && R < 1)) return LEAF_ERR_BAD_SHAPE;
    const long long chunks = ((long long)size + 3 + 3) >> 2;              // at the worst row shift
    const long long tiles = (chunks + kClipChunks * kClipThreads - 1) / (kClipChunks * kClipThreads);
    if ((long long)rows * tiles > 0x7fffffffll) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) || misaligned(win, 7u) ||
        misaligned(peaks, 3u) || misaligned(rec, 3u) || misaligned(out, 3u))
        return LEAF_ERR_ALIGNMENT;
    SegmentParams p{};
    p.store = store; p.store_len = store_len; p.rec_off = rec_off; p.rec_len = rec_len; p.win = win;
    p.peaks = peaks; p.rec = rec; p.out = out; p.R = R; p.S = size; p.tiles = (int)tiles;
    const dim3 grid((unsigned)(rows * tiles)), block(kClipThreads);
    if (pcm) hipLaunchKernelGGL(assemble_segments_kernel<true>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(assemble_segments_kernel<false>, grid, block, 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// ... of the standardised recordings.  moments == NULL: the call is the entry above.
int leaf_assemble_segments_std_f32(const void* store, long long store_len, int flags, int rows, int size, const long long* rec_off,
                                   const int* rec_len, const long long* win, const float* peaks, const int* rec, int R, float* out,
                                   const float* moments, int normalize, void* stream) {
    if (!moments) return leaf_assemble_segments_f32(store, store_len, flags, rows, size, rec_off, rec_len, win, peaks, rec, R, out, stream);
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;
    if (peaks) return LEAF_ERR_UNSUPPORTED;                               // the raw recording's peak has no place behind the map
    if (!store || !rec_off || !rec_len || !win || !out || !rec) return LEAF_ERR_NULL_POINTER;
    if (rows < 1 || size < 1 || store_len < 0 || R < 1) return LEAF_ERR_BAD_SHAPE;
    const long long chunks = ((long long)size + 3 + 3) >> 2;              // at the worst row shift
    const long long tiles = (chunks + kClipChunks * kClipThreads - 1) / (kClipChunks * kClipThreads);
    if ((long long)rows * tiles > 0x7fffffffll) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) || misaligned(win, 7u) ||
        misaligned(rec, 3u) || misaligned(out, 3u) || misaligned(moments, 3u))
        return LEAF_ERR_ALIGNMENT;
    SegmentParams p{};
    p.store = store; p.store_len = store_len; p.rec_off = rec_off; p.rec_len = rec_len; p.win = win;
    p.peaks = nullptr; p.rec = rec; p.out = out; p.R = R; p.S = size; p.tiles = (int)tiles;
    ClipStdParams sp{};
    sp.moments = moments; sp.rec = rec; sp.R = R; sp.normalize = normalize != 0;
    const dim3 grid((unsigned)(rows * tiles)), block(kClipThreads);
    if (pcm) hipLaunchKernelGGL(assemble_segments_std_kernel<true>, grid, block, 0, (hipStream_t)stream, p, sp);
    else hipLaunchKernelGGL(assemble_segments_std_kernel<false>, grid, block, 0, (hipStream_t)stream, p, sp);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// mean, std, min, max per recording: two passes over the samples (sum; squared deviations from the float64 mean), each a launch of
// span partials and a launch that folds them -- four launches, one call per dataset
size_t leaf_clip_moments_workspace_bytes(int R) {
    return R < 1 ? 0 : (sizeof(MomentPartial) * kMomentSpans + sizeof(double)) * (size_t)R;
}

int leaf_clip_moments_f32(const void* store, long long store_len, int flags, int R, const long long* rec_off, const int* rec_len,
                          float* moments, void* workspace, size_t workspace_bytes, void* stream) {
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;
    if (!store || !rec_off || !rec_len || !moments) return LEAF_ERR_NULL_POINTER;
    if (R < 1 || store_len < 0) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) || misaligned(moments, 3u) || misaligned(workspace, 15u))
        return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < leaf_clip_moments_workspace_bytes(R)) return LEAF_ERR_WORKSPACE;
    static_assert(sizeof(MomentPartial) == 16, "the workspace layout of include/leaf_hip.h");
    MomentParams p{};
    p.store = store; p.store_len = store_len; p.rec_off = rec_off; p.rec_len = rec_len; p.moments = moments;
    p.part = static_cast<MomentPartial*>(workspace);
    p.mean = reinterpret_cast<double*>(p.part + (size_t)R * kMomentSpans);
    p.R = R;
    const hipStream_t st = (hipStream_t)stream;
    // a unit (one span of one recording) is one wave's; the units beyond the grid are walked by the same waves, and which wave takes
    // a unit does not enter its partial
    const long long units = (long long)R * kMomentSpans, per_block = kPeakThreads / 64;
    const dim3 pass((unsigned)std::min<long long>((units + per_block - 1) / per_block, kPeakMaxBlocks)), block(kPeakThreads);
    const dim3 fold((unsigned)(((long long)R + kPeakThreads - 1) / kPeakThreads));
    if (pcm) hipLaunchKernelGGL((clip_moments_pass_kernel<true, false>), pass, block, 0, st, p);
    else hipLaunchKernelGGL((clip_moments_pass_kernel<false, false>), pass, block, 0, st, p);
    hipLaunchKernelGGL(clip_moments_fold_kernel<false>, fold, block, 0, st, p);
    if (pcm) hipLaunchKernelGGL((clip_moments_pass_kernel<true, true>), pass, block, 0, st, p);
    else hipLaunchKernelGGL((clip_moments_pass_kernel<false, true>), pass, block, 0, st, p);
    hipLaunchKernelGGL(clip_moments_fold_kernel<true>, fold, block, 0, st, p);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// the plan of the entries above, drawn on the device: one launch of one workgroup, no workspace, nothing read back.  Each output group
// is there or NULL as a whole; the noise group brings the noise store's two arrays with it.
int leaf_draw_clip_plan(int B, int size, int train, const long long* offsets, const int* lengths, int R,
                        const long long* noise_offsets, const int* noise_lengths, int Rn,
                        const long long* index, const long long* order, long long N,
                        unsigned long long* state, int advance, unsigned long long seed, unsigned long long stream_base,
                        int pad_mode_a, int pad_mode_b, double wrap_pad_prob, double gain_prob, double gain_db_lo, double gain_db_hi,
                        int M, double time_perc, double noise_prob, double snr_lo, double snr_hi,
                        double gauss_prob, double gauss_amp_lo, double gauss_amp_hi,
                        long long* rec_off, int* rec_len, int* start, int* pad_mode, float* gain, int* masks, int* rec,
                        long long* noise_off, int* noise_len, int* noise_start, int* noise_pad_mode, float* noise_coeff,
                        float* gauss_amp, long long* gauss_stream, long long* index_out, void* stream) {
    const bool any_noise = noise_offsets || noise_lengths || noise_off || noise_len || noise_start || noise_pad_mode || noise_coeff;
    const bool any_gauss = gauss_amp || gauss_stream;
    if (!offsets || !lengths || !state || !rec_off || !rec_len || !start || !pad_mode) return LEAF_ERR_NULL_POINTER;
    if (!index == !order) return LEAF_ERR_NULL_POINTER;                   // exactly one names the recordings
    if (any_noise && !(noise_offsets && noise_lengths && noise_off && noise_len && noise_start && noise_pad_mode && noise_coeff))
        return LEAF_ERR_NULL_POINTER;
    if (any_gauss && !(gauss_amp && gauss_stream)) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || size < 1 || R < 1 || M < 0 || M > kDrawMaxMasks || (M > 0 && !masks) || (order && N < 1) || (any_noise && Rn < 1) ||
        pad_mode_a < 0 || pad_mode_a > 3 || pad_mode_b < 0 || pad_mode_b > 3)
        return LEAF_ERR_BAD_SHAPE;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(offsets, 7u) || misaligned(lengths, 3u) || misaligned(noise_offsets, 7u) || misaligned(noise_lengths, 3u) ||
        misaligned(index, 7u) || misaligned(order, 7u) || misaligned(state, 7u) || misaligned(rec_off, 7u) || misaligned(rec_len, 3u) ||
        misaligned(start, 3u) || misaligned(pad_mode, 3u) || misaligned(gain, 3u) || misaligned(masks, 3u) || misaligned(rec, 3u) ||
        misaligned(noise_off, 7u) || misaligned(noise_len, 3u) || misaligned(noise_start, 3u) || misaligned(noise_pad_mode, 3u) ||
        misaligned(noise_coeff, 3u) || misaligned(gauss_amp, 3u) || misaligned(gauss_stream, 7u) || misaligned(index_out, 7u))
        return LEAF_ERR_ALIGNMENT;
    DrawParams p{};
    p.offsets = offsets; p.lengths = lengths; p.noise_offsets = noise_offsets; p.noise_lengths = noise_lengths;
    p.index = index; p.order = order; p.N = N; p.state = state; p.seed = seed; p.stream_base = stream_base;
    p.k.S = size; p.k.train = train != 0; p.k.mode0 = pad_mode_a; p.k.mode1 = pad_mode_b; p.k.M = M;
    p.k.wrap_pad_prob = wrap_pad_prob; p.k.gain_prob = gain_prob; p.k.gain_lo = gain_db_lo; p.k.gain_hi = gain_db_hi; p.k.time_perc = time_perc;
    p.k.noise_prob = noise_prob; p.k.snr_lo = snr_lo; p.k.snr_hi = snr_hi;
    p.k.gauss_prob = gauss_prob; p.k.amp_lo = gauss_amp_lo; p.k.amp_hi = gauss_amp_hi;
    p.B = B; p.R = R; p.Rn = Rn; p.advance = advance != 0;
    p.rec_off = rec_off; p.rec_len = rec_len; p.start = start; p.pad_mode = pad_mode; p.gain = gain; p.masks = M > 0 ? masks : nullptr; p.rec = rec;
    p.noise_off = noise_off; p.noise_len = noise_len; p.noise_start = noise_start; p.noise_pad_mode = noise_pad_mode; p.noise_coeff = noise_coeff;
    p.gauss_amp = gauss_amp; p.gauss_stream = gauss_stream; p.index_out = index_out;
    hipLaunchKernelGGL(draw_clip_plan_kernel, dim3(1), dim3(kDrawThreads), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// mixup's permutation and weights, drawn on the device: one launch of one workgroup, no workspace, nothing read back
int leaf_draw_mixup(int B, double alpha, unsigned long long* state, int advance, unsigned long long seed, unsigned long long stream_base,
                    int* perm, float* lam, void* stream) {
    if (!state || !perm || !lam) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || B > kMixMaxBatch || !(alpha > 0.0 && std::isfinite(alpha))) return LEAF_ERR_BAD_SHAPE;   // a NaN is not > 0
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(state, 7u) || misaligned(perm, 3u) || misaligned(lam, 3u)) return LEAF_ERR_ALIGNMENT;
    MixDrawParams p{};
    p.state = state; p.seed = seed; p.stream_base = stream_base; p.alpha = alpha; p.perm = perm; p.lam = lam;
    p.B = B; p.advance = advance != 0;
    p.N = 1;
    while (p.N < B) p.N <<= 1;                                            // the sort's size: the power of two at or above B
    hipLaunchKernelGGL(draw_mixup_kernel, dim3(1), dim3(mix_draw_threads(p.N)), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}
