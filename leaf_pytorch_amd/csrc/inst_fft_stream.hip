// inst_fft_stream.hip -- instantiations of the one-launch streaming step (leaf_fft_stream.hpp).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_stream.hpp"
#include "leaf_inst.hpp"

StreamKernel leaf_inst_fft_stream(int sk) {
    StreamKernel fn = nullptr;
    if (sk == 401) fn = leaf_fft_stream_kernel<401, 160>;
    else if (sk == 201) fn = leaf_fft_stream_kernel<201, 80>;
    return fn;
}

StreamBankKernel leaf_inst_fft_stream_bank(int sk) {
    StreamBankKernel fn = nullptr;
    if (sk == 401) fn = leaf_fft_stream_bank_kernel<401, 160>;
    else if (sk == 201) fn = leaf_fft_stream_bank_kernel<201, 80>;
    return fn;
}

unsigned leaf_layout_fft_stream() { return leaf_params_layout(); }              // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
