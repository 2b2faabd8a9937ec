// inst_fft_small.hip -- instantiations of the single-launch small-batch forward (leaf_fft_small.hpp).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_small.hpp"
#include "leaf_inst.hpp"

// split: two workgroups per (clip, filter), seven waves each (grid (F, B, 2))
SmallKernel leaf_inst_fft_small(int sk, bool split) {
    SmallKernel fn = nullptr;
    if (sk == 401) fn = split ? leaf_fft_small_kernel<401, 160, true> : leaf_fft_small_kernel<401, 160>;
    else if (sk == 201) fn = split ? leaf_fft_small_kernel<201, 80, true> : leaf_fft_small_kernel<201, 80>;
    return fn;
}

// ... for a mixed call (waveform mixup in the block load)
SmallKernel leaf_inst_fft_small_mix(int sk, bool split) {
    SmallKernel fn = nullptr;
    if (sk == 401) fn = split ? leaf_fft_small_kernel<401, 160, true, true> : leaf_fft_small_kernel<401, 160, false, true>;
    else if (sk == 201) fn = split ? leaf_fft_small_kernel<201, 80, true, true> : leaf_fft_small_kernel<201, 80, false, true>;
    return fn;
}

unsigned leaf_layout_fft_small() { return leaf_params_layout(); }                // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
