// inst_fft_wgg4k_bwd.hip -- instantiations of the 4096-sample run-time-geometry backward kernel (leaf_fft_wgg4k_bwd.hpp).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_wgg4k_bwd.hpp"
#include "leaf_inst.hpp"

FftKernel leaf_inst_fft_wgg4k_bwd(int ni2) {
    FftKernel fn = nullptr;
    switch (ni2) {
        case 10: fn = leaf_fft_wgg4k_bwd_kernel<12, 10>; break;
        case 13: fn = leaf_fft_wgg4k_bwd_kernel<12, 13>; break;
        case 17: fn = leaf_fft_wgg4k_bwd_kernel<12, 17>; break;
    }
    return fn;
}

// ... for a mixed call (waveform mixup in the block load)
FftKernel leaf_inst_fft_wgg4k_bwd_mix(int ni2) {
    FftKernel fn = nullptr;
    switch (ni2) {
        case 10: fn = leaf_fft_wgg4k_bwd_kernel<12, 10, false, false, true>; break;
        case 13: fn = leaf_fft_wgg4k_bwd_kernel<12, 13, false, false, true>; break;
        case 17: fn = leaf_fft_wgg4k_bwd_kernel<12, 17, false, false, true>; break;
    }
    return fn;
}
FftKernel leaf_inst_fft_wg4k_bwd_mix() {
    FftKernel fn = leaf_fft_wgg4k_bwd_kernel<LEAF_4K_BWD_NW, 7, true, false, true>;
    return fn;
}

// the static 32 kHz geometry (K = 801, hop = 320)
FftKernel leaf_inst_fft_wg4k_bwd() {
    FftKernel fn = leaf_fft_wgg4k_bwd_kernel<LEAF_4K_BWD_NW, 7, true>;
    return fn;
}

// ... with dL/dx: nine waves, the block's gradient spectra in LDS
FftKernel leaf_inst_fft_wg4k_bwd_dx() {
    FftKernel fn = leaf_fft_wgg4k_bwd_kernel<kWg4BwdDxWaves, 7, true, true>;
    return fn;
}

unsigned leaf_layout_fft_wgg4k_bwd() { return leaf_params_layout(); }                // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
