// inst_fft_wg_x16.hip -- the tail-finalize instances of the static workgroup forward kernel (leaf_fft_wg.hpp) for 16-bit waveforms (bfloat16 and PCM16 share the load loop).
// One of the translation units of libleaf_hip.so; see leaf_inst.hpp.
#include "leaf_fft_wg.hpp"
#include "leaf_inst.hpp"

FftKernel leaf_inst_fft_wg_x16(int sk, int nw, int tailc) { return wg_tail_instance<kWgX16>(sk, nw, tailc); }

unsigned leaf_layout_fft_wg_x16() { return leaf_params_layout(); }      // the launch structs' layout this unit was compiled with (leaf_inst.hpp)
