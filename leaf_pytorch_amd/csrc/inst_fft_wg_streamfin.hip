// inst_fft_wg_streamfin.hip -- the static workgroup forward kernels that finalize in the kernel (STREAM: whole clips per workgroup,
// frame sums in an LDS ring; leaf_fft_wg.hpp), every sample kind (the loader is chosen at run time).  One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_wg.hpp"
#include "leaf_inst.hpp"

FftKernel leaf_inst_fft_wg_streamfin(int sk, int nw) {
    FftKernel fn = nullptr;
    if (sk == 401 && nw == 12) fn = leaf_fft_wg_kernel<401, 160, 12, true>;
    else if (sk == 801 && nw == 10) fn = leaf_fft_wg_kernel<801, 320, 10, true>;
    else if (sk == 201 && nw == 12) fn = leaf_fft_wg_kernel<201, 80, 12, true>;
    return fn;
}

unsigned leaf_layout_fft_wg_streamfin() { return leaf_params_layout(); }      // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
