// inst_fft_wg_mix.hip -- the tail-finalize instances of the static workgroup forward kernel (leaf_fft_wg.hpp) for mixed calls on an fp32 waveform (waveform mixup in the block load).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_wg.hpp"
#include "leaf_inst.hpp"

FftKernel leaf_inst_fft_wg_mix(int sk, int nw, int tailc) { return wg_tail_instance<kWgXMix>(sk, nw, tailc); }

unsigned leaf_layout_fft_wg_mix() { return leaf_params_layout(); }      // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
