// inst_fft_wg.hip -- instantiations of the static-geometry workgroup forward kernels (leaf_fft_wg.hpp, leaf_fft_wg4k.hpp).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_wg4k.hpp"
#include "leaf_inst.hpp"

// fp32 waveform, tail finalize (the STREAM variant: inst_fft_wg_streamfin.hip; 16-bit and mixed waveforms: inst_fft_wg_x16.hip,
// inst_fft_wg_mix.hip, inst_fft_wg_mix16.hip).  tailc: the tile form of the tail, 128 (rows of <= 128 frames) or 64 (longer rows)
FftKernel leaf_inst_fft_wg(int sk, int nw, int tailc) {
    if (FftKernel fn = wg_tail_instance<kWgXF32>(sk, nw, tailc)) return fn;
    FftKernel fn = nullptr;
    const bool t128 = tailc == 128, t64 = tailc == 64;
    (void)t128; (void)t64;
#ifdef LEAF_WG_NW                   // A/B builds (tools/compare_builds.py name:-DLEAF_WG_NW=8): another workgroup size for 401/160
    if (sk == 401 && nw == LEAF_WG_NW) fn = t128 ? wg_tail_kernel<401, 160, LEAF_WG_NW, kWgXF32, 128>() : t64 ? wg_tail_kernel<401, 160, LEAF_WG_NW, kWgXF32, 64>() : nullptr;
#endif
#if LEAF_TOOLS                      // LEAF_WG_WAVES=16: the column-half transposition form (A/B measurements)
    if (sk == 401 && nw == 16) fn = t128 ? wg_tail_kernel<401, 160, 16, kWgXF32, 128>() : t64 ? wg_tail_kernel<401, 160, 16, kWgXF32, 64>() : nullptr;
    else if (sk == 801 && nw == 14) fn = t128 ? wg_tail_kernel<801, 320, 14, kWgXF32, 128>() : t64 ? wg_tail_kernel<801, 320, 14, kWgXF32, 64>() : nullptr;
    else if (sk == 201 && nw == 16) fn = t128 ? wg_tail_kernel<201, 80, 16, kWgXF32, 128>() : t64 ? wg_tail_kernel<201, 80, 16, kWgXF32, 64>() : nullptr;
#endif
    return fn;
}

FftKernel leaf_inst_fft_wg4k() {
    FftKernel fn = leaf_fft_wg4k_kernel<801, 320, LEAF_4K_FWD_NW>;
    return fn;
}

unsigned leaf_layout_fft_wg() { return leaf_params_layout(); }                // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
