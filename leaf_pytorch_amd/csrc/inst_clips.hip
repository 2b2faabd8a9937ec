// inst_clips.hip -- batch assembly from a packed sample store: the kernel of leaf_clips.hpp and its C-ABI entry.
// One of the translation units of libleaf_hip.so; it shares nothing with the others but the header's declarations.
#define LEAF_INST_TU 1
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
