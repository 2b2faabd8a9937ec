// leaf_inst.hpp -- handles of the big kernel-template instantiations, one getter per kernel family.
// Included by every unit: declarations only.
//
// libleaf_hip.so is built from several translation units compiled in parallel (leaf_pytorch_amd/_native.py): leaf_kernels.hip
// holds the C ABI, the host logic and the small kernels; each inst_*.hip instantiates one family of the big templates and
// hands out their host-side handles through the getters below.  A getter returns nullptr for a combination that is not
// instantiated (the callers treat that as "this kernel does not exist for the geometry").  The handles are typed: a kernel
// takes its parameter struct by value, the structs are defined once (leaf_params.hpp, namespace leaf), and the unit that
// launches a kernel passes the type the kernel was compiled for -- the compiler checks it.
//
// LEAF_TOOLS (compile-time, default 0): measurement builds additionally instantiate the A/B variants the tools/ scripts
// select through environment variables (16-wave static kernels, wide NOFF = 6 register tiles of the MFMA kernel).
#pragma once
#include "leaf_params.hpp"
#ifndef LEAF_TOOLS
#define LEAF_TOOLS 0
#endif

namespace leaf {
using FusedKernel = void (*)(const FusedParams);
using DtapsKernel = void (*)(const DtapsParams);
using FftKernel = void (*)(const FftParams);
using SmallKernel = void (*)(const SmallParams);
using StreamKernel = void (*)(const StreamParams);
using StreamBankKernel = void (*)(const StreamBankParams);
using HeadBwdKernel = void (*)(const HeadBwdParams);
}  // namespace leaf

leaf::FusedKernel leaf_inst_fused(int rt, int noff, bool even_k, bool bwd);          // leaf_fused_kernel<RT, NOFF, EVENK, BWD>
leaf::DtapsKernel leaf_inst_dtaps(int rt, int tpw, bool even_k);                     // dtaps_mfma_kernel<RT, TPW, EVENK>
leaf::FftKernel leaf_inst_fft(int sk, int g2, int rs, int bwd);                      // leaf_fft_kernel<SK, SHOP, G2, RS, BWD>; sk = 0 | 201 | 401 | 801
leaf::FftKernel leaf_inst_fft_wg(int sk, int nw, int tailc);                         // fp32 waveform: leaf_fft_wg_kernel<SK, SHOP, NW> (tailc = 128), leaf_fft_wg_kernel_var<.., kWgXF32, 64>
leaf::FftKernel leaf_inst_fft_wg_streamfin(int sk, int nw);                          // leaf_fft_wg_kernel<SK, SHOP, NW, true>: every sample kind
leaf::FftKernel leaf_inst_fft_wg_x16(int sk, int nw, int tailc);                     // leaf_fft_wg_kernel_var<SK, SHOP, NW, kWgX16, TAILC>: bfloat16 / PCM16 waveform
leaf::SmallKernel leaf_inst_fft_small(int sk, bool split);                          // leaf_fft_small_kernel<SK, SHOP, SPLIT>: sk = 401 | 201
leaf::StreamKernel leaf_inst_fft_stream(int sk);                                     // leaf_fft_stream_kernel<SK, SHOP>: sk = 401 | 201
leaf::StreamBankKernel leaf_inst_fft_stream_bank(int sk);                            // leaf_fft_stream_bank_kernel<SK, SHOP>: sk = 401 | 201
leaf::FftKernel leaf_inst_fft_wg4k();                                                // leaf_fft_wg4k_kernel<801, 320, 12>
leaf::FftKernel leaf_inst_fft_wgg(int ni, bool half_scratch);                        // leaf_fft_wgg_kernel<12, NI, HALF>
leaf::FftKernel leaf_inst_fft_wgg4k(int ni2);                                        // leaf_fft_wgg4k_kernel<12, NI2>
leaf::FftKernel leaf_inst_fft_wg_bwd(int sk);                                        // leaf_fft_wg_bwd_kernel<SK, SHOP, 12>
leaf::FftKernel leaf_inst_fft_wg_bwd_dx(int sk);                                     // leaf_fft_wg_bwd_kernel<SK, SHOP, 12, true>: + dL/dx (K = 401, 201)
leaf::FftKernel leaf_inst_fft_blk_bwd_dx(int sk);                                    // leaf_fft_blk_bwd_dx_kernel<SK, SHOP>
leaf::FftKernel leaf_inst_fft_blk_bwd_dx_bf16(int sk);                               // leaf_fft_blk_bwd_dx_kernel<SK, SHOP, true>: bfloat16 waveform
leaf::FftKernel leaf_inst_fft_wgg_bwd(int ni, bool half_scratch);                    // leaf_fft_wgg_bwd_kernel<12, NI, HALF>
leaf::FftKernel leaf_inst_fft_wgg_bwd_dx(int ni);                                    // leaf_fft_wgg_bwd_kernel<12, NI, true, true>: + dL/dx
leaf::FftKernel leaf_inst_fft_wgg4k_bwd(int ni2);                                    // leaf_fft_wgg4k_bwd_kernel<12, NI2>
leaf::FftKernel leaf_inst_fft_wg4k_bwd();                                            // leaf_fft_wgg4k_bwd_kernel<12, 7, true>: K = 801, hop = 320
leaf::FftKernel leaf_inst_fft_wg4k_bwd_dx();                                         // leaf_fft_wgg4k_bwd_kernel<9, 7, true, true>: the same with dL/dx
leaf::HeadBwdKernel leaf_inst_head_bwd();                                            // leaf_head_bwd_kernel: pool_b and PCEN gradients from pooled_raw, one launch
// the split of the batch that kernel's grid (F, S) follows -- slices of L rows, a function of B, F and the CU count alone
// (leaf_head_bwd.hpp: head_plan)
void leaf_head_bwd_plan(int B, int F, int cus, int* S, int* L);

// the instances for a mixed call (waveform mixup in the block load, leaf_common.hpp); nullptr where there is none
leaf::FftKernel leaf_inst_fft_mix(int sk, int bwd);                                  // leaf_fft_kernel<SK, SHOP, 1, 1, BWD, true>: sk = 401 | 801 | 201
leaf::FftKernel leaf_inst_fft_wg_mix(int sk, int nw, int tailc);                     // leaf_fft_wg_kernel_var<SK, SHOP, NW, kWgXMix, TAILC>: fp32 waveform
leaf::FftKernel leaf_inst_fft_wg_mix16(int sk, int nw, int tailc);                   // leaf_fft_wg_kernel_var<SK, SHOP, NW, kWgXMix16, TAILC>: PCM16 waveform
leaf::SmallKernel leaf_inst_fft_small_mix(int sk, bool split);                       // leaf_fft_small_kernel<SK, SHOP, SPLIT, true>
leaf::FftKernel leaf_inst_fft_wg_bwd_mix(int sk);                                    // leaf_fft_wg_bwd_kernel<SK, SHOP, 12, false, true>
leaf::FftKernel leaf_inst_fft_wgg4k_bwd_mix(int ni2);                                // leaf_fft_wgg4k_bwd_kernel<12, NI2, false, false, true>
leaf::FftKernel leaf_inst_fft_wg4k_bwd_mix();                                        // leaf_fft_wgg4k_bwd_kernel<12, 7, true, false, true>

// leaf::leaf_params_layout() as each unit was compiled with it (leaf_params.hpp): compared by leaf_kernels.hip with its own
// value before the first launch (inst_layouts_ok) -- what catches a stale object file of an incremental build.
unsigned leaf_layout_fft();
unsigned leaf_layout_fft_small();
unsigned leaf_layout_fft_stream();
unsigned leaf_layout_fft_wg();
unsigned leaf_layout_fft_wg_streamfin();
unsigned leaf_layout_fft_wg_x16();
unsigned leaf_layout_fft_wg_mix();
unsigned leaf_layout_fft_wg_mix16();
unsigned leaf_layout_fft_wg_bwd();
unsigned leaf_layout_fft_wg_bwd_dx();
unsigned leaf_layout_fft_wgg();
unsigned leaf_layout_fft_wgg4k_bwd();
unsigned leaf_layout_fft_wgg_bwd();
unsigned leaf_layout_fft_wgg_bwd_dx();
unsigned leaf_layout_fused();
unsigned leaf_layout_head_bwd();
