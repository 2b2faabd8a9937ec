// inst_fft_stream.hip -- instantiations of the one-launch streaming step (leaf_fft_stream.hpp).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#define LEAF_INST_TU 1
#include "leaf_fft_stream.hpp"
#include "leaf_inst.hpp"

const void* leaf_inst_fft_stream(int sk) {
    void (*fn)(const StreamParams) = nullptr;
    if (sk == 401) fn = leaf_fft_stream_kernel<401, 160>;
    else if (sk == 201) fn = leaf_fft_stream_kernel<201, 80>;
    return reinterpret_cast<const void*>(fn);
}

const void* leaf_inst_fft_stream_bank(int sk) {
    void (*fn)(const StreamBankParams) = nullptr;
    if (sk == 401) fn = leaf_fft_stream_bank_kernel<401, 160>;
    else if (sk == 201) fn = leaf_fft_stream_bank_kernel<201, 80>;
    return reinterpret_cast<const void*>(fn);
}

unsigned leaf_layout_fft_stream() { return leaf_layout_hash_stream(); }              // parameter-struct layout this unit was compiled with (leaf_inst.hpp)
