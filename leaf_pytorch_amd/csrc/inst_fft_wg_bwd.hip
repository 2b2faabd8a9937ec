// inst_fft_wg_bwd.hip -- instantiations of the static-geometry workgroup backward kernels (leaf_fft_wg_bwd.hpp).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_wg_bwd.hpp"
#include "leaf_inst.hpp"

FftKernel leaf_inst_fft_wg_bwd(int sk) {
    FftKernel fn = nullptr;
    if (sk == 401) fn = leaf_fft_wg_bwd_kernel<401, 160, 12>;
    else if (sk == 801) fn = leaf_fft_wg_bwd_kernel<801, 320, 12>;
    else if (sk == 201) fn = leaf_fft_wg_bwd_kernel<201, 80, 12>;
    return fn;
}

// ... for a mixed call (waveform mixup in the block load)
FftKernel leaf_inst_fft_wg_bwd_mix(int sk) {
    FftKernel fn = nullptr;
    if (sk == 401) fn = leaf_fft_wg_bwd_kernel<401, 160, 12, false, true>;
    else if (sk == 801) fn = leaf_fft_wg_bwd_kernel<801, 320, 12, false, true>;
    else if (sk == 201) fn = leaf_fft_wg_bwd_kernel<201, 80, 12, false, true>;
    return fn;
}

FftKernel leaf_inst_fft_blk_bwd_dx(int sk) {
    FftKernel fn = nullptr;
    if (sk == 401) fn = leaf_fft_blk_bwd_dx_kernel<401, 160>;
    else if (sk == 801) fn = leaf_fft_blk_bwd_dx_kernel<801, 320>;
    else if (sk == 201) fn = leaf_fft_blk_bwd_dx_kernel<201, 80>;
    return fn;
}

FftKernel leaf_inst_fft_blk_bwd_dx_bf16(int sk) {
    FftKernel fn = nullptr;
    if (sk == 401) fn = leaf_fft_blk_bwd_dx_kernel<401, 160, true>;
    else if (sk == 801) fn = leaf_fft_blk_bwd_dx_kernel<801, 320, true>;
    else if (sk == 201) fn = leaf_fft_blk_bwd_dx_kernel<201, 80, true>;
    return fn;
}

unsigned leaf_layout_fft_wg_bwd() { return leaf_params_layout(); }                // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
