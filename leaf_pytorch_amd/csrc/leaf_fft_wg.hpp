// leaf_fft_wg.hpp -- overlap-save forward, second generation: one WORKGROUP per block, spectrum shared through LDS
// Included by every unit: templates, device functions, constexpr sizes (gfx950 only).
//
// Why (round-1 profile of leaf_fft_kernel, profiles/r01): the kernel is fp32-VALU-issue-bound but issues only ~0.49 of
// the SIMD's slots: a wave issues at most one VALU instruction per ~4.6 cycles, so two waves per SIMD cannot fill a
// 2-cycle pipe, and each wave-level FFT has four dependent LDS phases.  Two waves per SIMD was forced by registers: the
// block's spectrum A' (64 VGPRs) stayed resident across the wave's filters next to the 64 registers of the transform.
//
// Here A' lives in LDS instead, computed ONCE per block and read by every wave of the workgroup at the spectral
// multiply, which (i) frees 64 + 32 VGPRs -> three waves per SIMD (12-wave workgroups, <= 168 VGPRs), (ii) removes the
// repeated forward transforms (one per block instead of one per (block, filter group)), and (iii) needs only half the
// spectrum: the (rotated) block is real, so A'[N - k] = conj(A'[k]) and bins 0..1024 are stored (8.2 KB per block);
// the upper half is read back mirrored (a descending ds_read_b64, conflict-free like the ascending one).
//
// Scheduling: no barriers.  A workgroup walks its blocks (blockIdx.x, + gridDim.x, ...) through a task queue in LDS:
//     fwd(0), [fwd(1), inv(0,0) .. inv(0,F-1)], [fwd(2), inv(1,0) ..], ...
// pulled in order with one LDS atomic per task.  fwd(i) = load + forward transform of set i's block into ring slot i & 1;
// inv(i,f) = spectral multiply with filter f + inverse transform + |.|^2 + pooling (the arithmetic of
// leaf_fft_kernel's static-geometry path; results differ from it only by the rounding of the mirrored upper half-spectrum,
// ~1e-7 relative, so a clip is bit-identical across batches served by THIS kernel, not across the two kernels).  Dependencies are two monotonic counters per slot:
//     inv(i,f) waits for  spectrum_cnt[slot] >= (i >> 1) + 1     (the spectrum is there: wg_acquire_block)
//     fwd(i)   waits for  readers_cnt[slot] >= (i >> 1) * F      (every reader of the slot's previous occupant is done)
// (the queue's ints, the protocol's operations and the loads every workgroup kernel shares: leaf_wg_queue.hpp)
// Because fwd(i+1) is queued BEFORE set i's inverse tasks, one wave computes the next spectrum while the other eleven
// work on the current block, and nobody waits for it.  Deadlock-free: a task only ever waits for tasks queued before it.
#pragma once
#include <type_traits>
#include "leaf_fft.hpp"
#include "leaf_inst.hpp"            // leaf::FftKernel: what the instance ladder at the end of this header hands out
#include "leaf_wg_queue.hpp"       // the task queue, its protocol, the block and spectrum-row loads: shared by all workgroup kernels

namespace {

constexpr int kWgRingFloat2 = 1032;            // bins 0..1024 of a block's spectrum, padded
constexpr int kWgFwdBins = 1152;               // static FORWARD kernel (leaf_fft_wg_kernel) and the first-block spectra of the table launch: bins 0..1151 -- the
constexpr int kWgRingFwdFloat2 = kWgFwdBins + 8;   // transform yields all 2048 bins, and band tasks whose window crosses Nyquist (leaf_band.hpp, round 6) read bins
                                               // kb .. kb + M - 1 < 1152 as they lie (bins above 1024 are the conjugate mirror of a real block's spectrum).  128 bins
                                               // beyond Nyquist, not 256: with 2 x 2 KB more the streaming-finalize instance would fall from a 64-frame ring to 32
                                               // (lag 6 -> 2, +5 % on BASELINE configs[3] / [4]); the default bank's top filter needs 111

// ---- wave-level 2048-point FFT, LDS-lean variant of fft2048 (same arithmetic, same register conventions) ----------
// At three waves per SIMD the LDS pipe (one per CU) is as busy as the VALUs (profiles/r02), so the transposes and table
// reads are re-shaped around the LDS cycle table of MI355X_MICROARCH.md:
//   * transposition writes: ds_write_addtid_b32 (address = M0 + offset + 4 lane, no address VGPR): 2 LDS cycles per
//     wave-instruction instead of ds_write_b32's 4 -- the write IS "row brev5(i), column lane", exactly the add-tid form;
//   * transposition reads: a lane's 32 values are contiguous in its row, so with a row stride of 68 floats (16-byte
//     aligned rows; the four 16-lane groups of a ds_read_b128 then cover all 64 banks exactly once) they are 8
//     ds_read_b128 (4 cycles per 16 bytes/lane) instead of 32 ds_read_b32 (2 cycles per 4 bytes/lane): half the cycles;
//   * twiddle / ring reads: ds_read_b64 issued from inline asm in chunks of 8 with counted lgkmcnt waits, because the
//     compiler pairs its own 8-byte LDS loads into ds_read2(st64)_b64, which the LDS serves at half the bytes per clock
//     of two ds_read_b64 (a volatile load is no way out: it becomes a flat load with a full wait behind each).
typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int kWgScrStride = 68;
constexpr int kWgScrFloats = 32 * kWgScrStride;

__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}
// One ds_read_b64 the compiler does not see as a memory operation (so it cannot pair it); the destination is only
// valid after a lds_wait8<N>() naming it.  LDS returns in issue order, so lgkmcnt(N) completes everything but the
// youngest N DS operations of this wave, whoever issued them.
template <int OFF>
__device__ __forceinline__ void lds_rd8(v2f& dst, unsigned addr) {
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
template <int N>
__device__ __forceinline__ void lds_wait8(v2f (&a)[8]) {
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])
                 : "i"(N));
}
// Eight-at-a-time streaming of 32 table entries: body(k, value) for k = 0..31, entry k read from addr + OFF(k).
template <typename OffFn, typename Body>
__device__ __forceinline__ void lds_stream32(unsigned addr, OffFn, Body body) {
    v2f buf[2][8];
    auto issue = [&](auto cc) {
        constexpr int c = decltype(cc)::value;
        lds_rd8<OffFn::off(8 * c + 0)>(buf[c & 1][0], addr); lds_rd8<OffFn::off(8 * c + 1)>(buf[c & 1][1], addr);
        lds_rd8<OffFn::off(8 * c + 2)>(buf[c & 1][2], addr); lds_rd8<OffFn::off(8 * c + 3)>(buf[c & 1][3], addr);
        lds_rd8<OffFn::off(8 * c + 4)>(buf[c & 1][4], addr); lds_rd8<OffFn::off(8 * c + 5)>(buf[c & 1][5], addr);
        lds_rd8<OffFn::off(8 * c + 6)>(buf[c & 1][6], addr); lds_rd8<OffFn::off(8 * c + 7)>(buf[c & 1][7], addr);
    };
    issue(std::integral_constant<int, 0>{});
    issue(std::integral_constant<int, 1>{});
    lds_wait8<8>(buf[0]);
#pragma unroll
    for (int j = 0; j < 8; ++j) body(j, buf[0][j]);
    issue(std::integral_constant<int, 2>{});
    lds_wait8<8>(buf[1]);
#pragma unroll
    for (int j = 0; j < 8; ++j) body(8 + j, buf[1][j]);
    issue(std::integral_constant<int, 3>{});
    lds_wait8<8>(buf[0]);
#pragma unroll
    for (int j = 0; j < 8; ++j) body(16 + j, buf[0][j]);
    lds_wait8<0>(buf[1]);
#pragma unroll
    for (int j = 0; j < 8; ++j) body(24 + j, buf[1][j]);
}
struct OffTwl { static constexpr int off(int i) { return 512 * brev5(i); } };      // twl[brev5(i)][lane], register order
struct OffRow { static constexpr int off(int k) { return 512 * (k & 15); } };      // 16 consecutive 64-entry rows

// scr[brev5(i) * 68 + lane] = v[i], i = 0..31, through M0-relative add-tid stores (M0 saved and restored: the compiler
// owns it for the LDS-DMA builtin).  scr_lds = the wave's scr as an LDS byte address (wave-uniform).
__device__ __forceinline__ void wg_transpose_store(const float (&v)[32], unsigned scr_lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %17\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %1 offset:0\n\t"
                 "ds_write_addtid_b32 %2 offset:4352\n\t"
                 "ds_write_addtid_b32 %3 offset:2176\n\t"
                 "ds_write_addtid_b32 %4 offset:6528\n\t"
                 "ds_write_addtid_b32 %5 offset:1088\n\t"
                 "ds_write_addtid_b32 %6 offset:5440\n\t"
                 "ds_write_addtid_b32 %7 offset:3264\n\t"
                 "ds_write_addtid_b32 %8 offset:7616\n\t"
                 "ds_write_addtid_b32 %9 offset:544\n\t"
                 "ds_write_addtid_b32 %10 offset:4896\n\t"
                 "ds_write_addtid_b32 %11 offset:2720\n\t"
                 "ds_write_addtid_b32 %12 offset:7072\n\t"
                 "ds_write_addtid_b32 %13 offset:1632\n\t"
                 "ds_write_addtid_b32 %14 offset:5984\n\t"
                 "ds_write_addtid_b32 %15 offset:3808\n\t"
                 "ds_write_addtid_b32 %16 offset:8160\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(v[8]), "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]), "s"(scr_lds)
                 : "memory");
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %17\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %1 offset:272\n\t"
                 "ds_write_addtid_b32 %2 offset:4624\n\t"
                 "ds_write_addtid_b32 %3 offset:2448\n\t"
                 "ds_write_addtid_b32 %4 offset:6800\n\t"
                 "ds_write_addtid_b32 %5 offset:1360\n\t"
                 "ds_write_addtid_b32 %6 offset:5712\n\t"
                 "ds_write_addtid_b32 %7 offset:3536\n\t"
                 "ds_write_addtid_b32 %8 offset:7888\n\t"
                 "ds_write_addtid_b32 %9 offset:816\n\t"
                 "ds_write_addtid_b32 %10 offset:5168\n\t"
                 "ds_write_addtid_b32 %11 offset:2992\n\t"
                 "ds_write_addtid_b32 %12 offset:7344\n\t"
                 "ds_write_addtid_b32 %13 offset:1904\n\t"
                 "ds_write_addtid_b32 %14 offset:6256\n\t"
                 "ds_write_addtid_b32 %15 offset:4080\n\t"
                 "ds_write_addtid_b32 %16 offset:8432\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(v[16]), "v"(v[17]), "v"(v[18]), "v"(v[19]), "v"(v[20]), "v"(v[21]), "v"(v[22]), "v"(v[23]), "v"(v[24]), "v"(v[25]), "v"(v[26]), "v"(v[27]), "v"(v[28]), "v"(v[29]), "v"(v[30]), "v"(v[31]), "s"(scr_lds)
                 : "memory");
}

// Column-half transposition (swap-free cross stage, below): the 32 lanes of one half-wave store their 32 registers as
// rows brev5(i) of a [32][36] scratch (columns = their 32 lane positions); every lane of the wave then reads row
// lane & 31 -- once after the lower half-wave's stores, once after the upper's.  M0-relative add-tid stores under an exec
// mask set inside the statement; the upper half-wave's base is 128 bytes lower so that lane 32 lands in column 0.
constexpr int kWgColStride = 36;
constexpr int kWgScrHalfFloats = 32 * kWgColStride;                      // 4608 bytes per wave
template <int UPPER>
__device__ __forceinline__ void wg_transpose_store_cols(const float (&v)[32], unsigned scr_lds) {
    unsigned keep;
    unsigned long long save;
    const unsigned base = scr_lds - (UPPER ? 128u : 0u);
    const unsigned long long mask = UPPER ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b64 %1, exec\n\ts_mov_b32 m0, %18\n\ts_mov_b64 exec, %19\n\t"
                 "ds_write_addtid_b32 %2 offset:0\n\t"
                 "ds_write_addtid_b32 %3 offset:2304\n\t"
                 "ds_write_addtid_b32 %4 offset:1152\n\t"
                 "ds_write_addtid_b32 %5 offset:3456\n\t"
                 "ds_write_addtid_b32 %6 offset:576\n\t"
                 "ds_write_addtid_b32 %7 offset:2880\n\t"
                 "ds_write_addtid_b32 %8 offset:1728\n\t"
                 "ds_write_addtid_b32 %9 offset:4032\n\t"
                 "ds_write_addtid_b32 %10 offset:288\n\t"
                 "ds_write_addtid_b32 %11 offset:2592\n\t"
                 "ds_write_addtid_b32 %12 offset:1440\n\t"
                 "ds_write_addtid_b32 %13 offset:3744\n\t"
                 "ds_write_addtid_b32 %14 offset:864\n\t"
                 "ds_write_addtid_b32 %15 offset:3168\n\t"
                 "ds_write_addtid_b32 %16 offset:2016\n\t"
                 "ds_write_addtid_b32 %17 offset:4320\n\t"
                 "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "=&s"(save)
                 : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(v[8]), "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]), "s"(base), "s"(mask)
                 : "memory");
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b64 %1, exec\n\ts_mov_b32 m0, %18\n\ts_mov_b64 exec, %19\n\t"
                 "ds_write_addtid_b32 %2 offset:144\n\t"
                 "ds_write_addtid_b32 %3 offset:2448\n\t"
                 "ds_write_addtid_b32 %4 offset:1296\n\t"
                 "ds_write_addtid_b32 %5 offset:3600\n\t"
                 "ds_write_addtid_b32 %6 offset:720\n\t"
                 "ds_write_addtid_b32 %7 offset:3024\n\t"
                 "ds_write_addtid_b32 %8 offset:1872\n\t"
                 "ds_write_addtid_b32 %9 offset:4176\n\t"
                 "ds_write_addtid_b32 %10 offset:432\n\t"
                 "ds_write_addtid_b32 %11 offset:2736\n\t"
                 "ds_write_addtid_b32 %12 offset:1584\n\t"
                 "ds_write_addtid_b32 %13 offset:3888\n\t"
                 "ds_write_addtid_b32 %14 offset:1008\n\t"
                 "ds_write_addtid_b32 %15 offset:3312\n\t"
                 "ds_write_addtid_b32 %16 offset:2160\n\t"
                 "ds_write_addtid_b32 %17 offset:4464\n\t"
                 "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "=&s"(save)
                 : "v"(v[16]), "v"(v[17]), "v"(v[18]), "v"(v[19]), "v"(v[20]), "v"(v[21]), "v"(v[22]), "v"(v[23]), "v"(v[24]), "v"(v[25]), "v"(v[26]), "v"(v[27]), "v"(v[28]), "v"(v[29]), "v"(v[30]), "v"(v[31]), "s"(base), "s"(mask)
                 : "memory");
}

// Twiddle tables of the workgroup kernels: twl as fft_build_twiddles; the half-wave twiddles in PAIR order,
//   twp[h][j][w]  = h ? W_64^(j + 16 w) : 1,  j < 16, w < 2   (float2; same 64 entries as twh[j][h]),
// so that the fused first stage of the second 32-point transform gets both twiddles of a register pair (j, j + 16) with one
// ds_read_b128 (16 LDS instructions per transform instead of 32).
__device__ __forceinline__ void fft_build_twiddles_wg(float2* twl, float2* twp, int tid, int nthreads) {
    for (int i = tid; i < 32 * 64; i += nthreads) {
        const int k1 = i >> 6, l = i & 63;                                       // twl[k1][l]
        float s, c;
        sincospif(2.0f * (float)((l * k1) & (kFftN - 1)) / (float)kFftN, &s, &c);
        twl[i] = make_float2(c, -s);
    }
    for (int i = tid; i < 64; i += nthreads) {
        const int h = i >> 5, e = i & 31, j = (e >> 1) + 16 * (e & 1);
        float s, c;
        sincospif(2.0f * (float)j / 64.0f, &s, &c);
        twp[i] = h ? make_float2(c, -s) : make_float2(1.0f, 0.0f);
    }
}
// sixteen 16-byte table entries at addr + 16 k, four at a time, two groups in flight: body(k, value)
template <int OFF>
__device__ __forceinline__ void lds_rd16(f32x4& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
template <int N>
__device__ __forceinline__ void lds_wait16x4(f32x4 (&a)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : "i"(N));
}
template <typename Body>
__device__ __forceinline__ void lds_stream16q(unsigned addr, Body body) {
    f32x4 buf[2][4];
    auto issue = [&](auto cc) {
        constexpr int c = decltype(cc)::value;
        lds_rd16<16 * (4 * c + 0)>(buf[c & 1][0], addr); lds_rd16<16 * (4 * c + 1)>(buf[c & 1][1], addr);
        lds_rd16<16 * (4 * c + 2)>(buf[c & 1][2], addr); lds_rd16<16 * (4 * c + 3)>(buf[c & 1][3], addr);
    };
    issue(std::integral_constant<int, 0>{});
    issue(std::integral_constant<int, 1>{});
    lds_wait16x4<4>(buf[0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) body(j, buf[0][j]);
    issue(std::integral_constant<int, 2>{});
    lds_wait16x4<4>(buf[1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) body(4 + j, buf[1][j]);
    issue(std::integral_constant<int, 3>{});
    lds_wait16x4<4>(buf[0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) body(8 + j, buf[0][j]);
    lds_wait16x4<0>(buf[1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) body(12 + j, buf[1][j]);
}

}  // namespace
#include "leaf_band.hpp"           // band-limited filter tasks (uses the LDS helpers above)
namespace {

// The spectral multiply Z = conj(A' R_f) of a filter task, fused with the first decimation-in-time stage of the transform that follows
// (pairs of rows (k, k + 16), unit twiddles; the transform is then called with SKIP1).  A = the block's spectrum in the ring, bins
// 0..1024; rq[k] = R_f[64 k + lane].  Rows 0..15 come straight from the ring, rows 16..31 mirrored (A'[N - e] = conj(A'[e])): two streams
// of 16 rows, ascending from A[lane], and the mirror A[2048 - 64 k - lane], k = 16..31, read as rows 15..0 of the base A[64 - lane], so
// row k + 16 is hi[k].  With za = conj(A'[k]) R[k] and zb = the mirrored row's product,
//     out[k] = za + zb,  out[k + 16] = za - zb   as one product and two FMAs per component -- 6 instructions per pair of rows
// instead of 4 products + 4 additions.  8-row chunks with counted waits: all 32 ring reads in flight at once would need 64 registers
// next to rq and Z.  (The counted waits are exact when no older LDS operation of the wave is outstanding; an older one only makes
// them wait longer.)
// Called by the backward kernels (wg_bwd_filter).  leaf_fft_wg_body and leaf_fft_wgg_kernel keep their written-out copies: with the call
// in its place the compiler allocated their registers differently and the STREAM instances and the run-time-geometry forward measured
// 0.6-0.9 % slower (profiles/wg_shared_protocol.txt).
__device__ __forceinline__ void wg_multiply_stage1(const float2* A, int lane, const float (&rq)[32], float (&zre)[32], float (&zim)[32]) {
    const unsigned a_lo = lds_addr(A + lane), a_hi = lds_addr(A + (kFftN - 64 * 31) - lane);
    v2f lo[16], hi[16];
    auto rd = [&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if constexpr (k < 16) lds_rd8<512 * k>(lo[k], a_lo);
        else lds_rd8<512 * (31 - k)>(hi[k - 16], a_hi);
    };
    // chunk 0: rows 0..7, chunk 1: rows 8..15, chunk 2: rows 16..23, chunk 3: rows 24..31
#define LEAF_RD8(B) rd(std::integral_constant<int, B + 0>{}); rd(std::integral_constant<int, B + 1>{}); \
                    rd(std::integral_constant<int, B + 2>{}); rd(std::integral_constant<int, B + 3>{}); \
                    rd(std::integral_constant<int, B + 4>{}); rd(std::integral_constant<int, B + 5>{}); \
                    rd(std::integral_constant<int, B + 6>{}); rd(std::integral_constant<int, B + 7>{});
    v2f(&lo0)[8] = *reinterpret_cast<v2f(*)[8]>(&lo[0]);
    v2f(&lo1)[8] = *reinterpret_cast<v2f(*)[8]>(&lo[8]);
    v2f(&hi0)[8] = *reinterpret_cast<v2f(*)[8]>(&hi[0]);
    v2f(&hi1)[8] = *reinterpret_cast<v2f(*)[8]>(&hi[8]);
    auto pair = [&](int k) {
        const float ra = rq[k], rb = rq[k + 16];
        const float tr_ = lo[k].x * ra, ti_ = -(lo[k].y * ra);
        zre[k] = fmaf(hi[k].x, rb, tr_);
        zim[k] = fmaf(hi[k].y, rb, ti_);
        zre[k + 16] = fmaf(-hi[k].x, rb, tr_);
        zim[k + 16] = fmaf(-hi[k].y, rb, ti_);
    };
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // the counted waits below see only these reads
    LEAF_RD8(0) LEAF_RD8(16) LEAF_RD8(8)
    lds_wait8<8>(lo0);
    lds_wait8<8>(hi0);
#pragma unroll
    for (int k = 0; k < 8; ++k) pair(k);
    LEAF_RD8(24)
    lds_wait8<0>(lo1);
    lds_wait8<0>(hi1);
#pragma unroll
    for (int k = 8; k < 16; ++k) pair(k);
#undef LEAF_RD8
}

// SKIP1: the caller has already run the first decimation-in-time stage (registers (k, k + 16), unit twiddles) -- fused with the
// spectral multiply that produced the input (wg_multiply_stage1, above, in the backward kernels; the two forward kernels of the
// 2048-sample plan carry the same sequence written out in their task loops)
template <bool HALF, bool SKIP1 = false>
__device__ __forceinline__ void fft2048w(float (&re)[32], float (&im)[32], float* scr, unsigned scr_lds, const float2* twl,
                                         const float2* twh, int lane) {
    if constexpr (SKIP1) {
        fft32_dit_stage<2>(re, im);
        fft32_dit_stage<4>(re, im);
        fft32_dit_stage<8>(re, im);
        fft32_dit_stage<16>(re, im);
    } else {
        fft32_dif(re, im);                               // register i <-> k1 = brev5(i), lane = n2
    }
    lds_stream32(lds_addr(twl + lane), OffTwl{}, [&](int i, v2f w) {
        if (i == 0) return;                               // W^0 = 1
        const float r = re[i] * w.x - im[i] * w.y;
        im[i] = re[i] * w.y + im[i] * w.x;
        re[i] = r;
    });
    const int k1r = lane & 31, h = lane >> 5;
    float tr[32], ti[32];
    // 64-point DFT over n2 = j + 32 hh, first radix-2 step WITHOUT a cross-lane exchange: every lane reads both halves of
    // its transposed row (its own 32 columns and the other half-wave's) and forms a + b (lower half-wave) or a - b (upper)
    // itself -- one FMA per value.  v_permlane32_swap issues at ~8 cycles (profiles/r01/ubench_valu.txt), the 64 swaps
    // per transform of the exchange form were a sixth of its issue time; the price is 16 more ds_read_b128 per transform.
    const float sg = h ? -1.0f : 1.0f;                    // t = a + sg b: a = x[j] (lower half-wave's), b = x[j + 32] (upper's)
    if constexpr (HALF) {
        const f32x4* row = reinterpret_cast<const f32x4*>(scr + k1r * kWgColStride);
        auto plane = [&](const float (&src)[32], float (&t)[32]) {
            f32x4 a[8], b[8];
            wg_transpose_store_cols<0>(src, scr_lds);
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = row[q];
            wg_transpose_store_cols<1>(src, scr_lds);     // LDS executes in order: the reads above are served first
#pragma unroll
            for (int q = 0; q < 8; ++q) b[q] = row[q];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                t[4 * q] = fmaf(b[q].x, sg, a[q].x); t[4 * q + 1] = fmaf(b[q].y, sg, a[q].y);
                t[4 * q + 2] = fmaf(b[q].z, sg, a[q].z); t[4 * q + 3] = fmaf(b[q].w, sg, a[q].w);
            }
            asm volatile("" ::: "memory");
        };
        pin32(re);                                        // the twiddle products are complete before the first store
        pin32(im);
        plane(re, tr);
        pin32(tr);
        plane(im, ti);
        pin32(ti);
    } else {
        const f32x4* lo = reinterpret_cast<const f32x4*>(scr + k1r * kWgScrStride);
        auto plane = [&](const float (&src)[32], float (&t)[32]) {
            wg_transpose_store(src, scr_lds);
#pragma unroll
            for (int q0 = 0; q0 < 8; q0 += 4) {           // 32 values in flight at a time
#pragma unroll
                for (int q = q0; q < q0 + 4; ++q) {
                    const f32x4 a = lo[q], b = lo[q + 8];
                    t[4 * q] = fmaf(b.x, sg, a.x); t[4 * q + 1] = fmaf(b.y, sg, a.y);
                    t[4 * q + 2] = fmaf(b.z, sg, a.z); t[4 * q + 3] = fmaf(b.w, sg, a.w);
                }
                asm volatile("" ::: "memory");
            }
        };
        pin32(re);
        pin32(im);
        plane(re, tr);
        pin32(tr);
        plane(im, ti);
        pin32(ti);
    }
    // The half-wave twiddle fused into the first decimation-in-time stage of the 32-point transform over j: that stage
    // pairs registers (j, j + 16) with unit twiddles, so with a = t[j] w[j] and b = t[j + 16] w[j + 16]
    //     out[j] = a + b = a + w_b t_b  (four FMAs on top of a),   out[j + 16] = a - b = 2 a - out[j]  (two FMAs):
    // 10 instructions per pair instead of 8 (two complex products) + 4 (the butterfly) -- 32 fewer per transform.  The table
    // is streamed in pair order (w[j], w[j + 16]).
    lds_stream16q(lds_addr(twh + 32 * h), [&](int j, f32x4 w) {             // w = (w[j], w[j + 16]) of this half-wave
        float ar, ai;
        if (j == 0) {
            ar = tr[0];
            ai = ti[0];
        } else {
            ar = tr[j] * w.x - ti[j] * w.y;
            ai = tr[j] * w.y + ti[j] * w.x;
        }
        const float br = tr[j + 16], bi = ti[j + 16];
        const float pr = fmaf(-bi, w.w, fmaf(br, w.z, ar));
        const float pi = fmaf(bi, w.z, fmaf(br, w.w, ai));
        re[j] = pr;
        im[j] = pi;
        re[j + 16] = fmaf(2.0f, ar, -pr);
        im[j + 16] = fmaf(2.0f, ai, -pi);
    });
    fft32_dit_stage<2>(re, im);
    fft32_dit_stage<4>(re, im);
    fft32_dit_stage<8>(re, im);
    fft32_dit_stage<16>(re, im);                         // register i <-> k' = brev5(i): element 64 k' + lane
}

// floats of dynamic LDS for NW waves
constexpr int fft_wg_scr_floats(int NW) { return NW > 12 ? kWgScrHalfFloats : kWgScrFloats; }   // > 12 waves: half buffer
constexpr size_t fft_wg_lds_bytes(int NW, int SK) {
    return ((size_t)kTwFloats + 2 * 2 * kWgRingFwdFloat2 + kWgQueueInts +
            (size_t)NW * fft_wg_scr_floats(NW)) * 4;
}
// Static pooling with the weights in REGISTERS.  A 64-sample row r of |y|^2 meets frame fi's window at window index
// j0 + lane with j0 = 64 r - is(fi), is(fi) = (DMIN + fi) hop - padL: every j0 is congruent to padL modulo g = gcd(64, hop),
// so the ~80 (row, frame) pairs of a block share only NJ = (K + 62 - jmin) / g + 1 distinct weight vectors
// w_k[lane] = g_f[jmin + g k + lane] (15 at 401/160, 14 at 801/320, 17 at 201/80; zero outside the window: the table row has
// kGPad zeros in front and a zero tail).  They are read from the filter's table row once per task (NJ coalesced loads) and
// replace the wave-private LDS copy of the row, its DMA and one ds_read_b32 per pair.
constexpr int wg_gcd(int a, int b) { return b == 0 ? a : wg_gcd(b, a % b); }
constexpr int wg_pool_step(int SHOP) { return wg_gcd(64, SHOP); }
constexpr int wg_pool_jmin(int SK, int SHOP) {       // smallest j0 >= -63 congruent to padL modulo the step
    const int g = wg_pool_step(SHOP), padl = SK / 2 + SK % 2 - 1;
    return -63 + (((padl + 63) % g) + g) % g;
}
constexpr int wg_pool_nj(int SK, int SHOP) { return (SK - 1 - wg_pool_jmin(SK, SHOP)) / wg_pool_step(SHOP) + 1; }

// ---- streaming finalize (STREAM = true) -------------------------------------------------------------------------------
// When the dealing gives every workgroup whole clips, the per-frame partial sums never leave the CU: an inverse task drops
// its (at most NFR) frame sums into a small LDS ring, fr[frame mod RING][filter] (ONE accumulator per frame and filter since
// round 5: the two blocks a window meets add their sums with ds_add_f32 -- a + b either way round, the rounding of `part`'s
// slot 0 + slot 1 -- and the finalize puts the zero back; the ring is twice as long in the same LDS, which the band tasks'
// shorter blocks need: with a lag of 2 the forward task waited ~25 k cycles per 20 k-cycle block), and once every filter of
// block c is through, the frames that block completed are finalized
// by ONE wave, lane = filter: sums -> bias -> floor -> the EMA recurrence, continued from the state kept in LDS -> PCEN ->
// the output rows (fin_* of leaf_fft.hpp: the same arithmetic as the row kernel, so a clip's bits do not depend on which
// of the two finalizes it).  That wave is whichever finishes the block's LAST filter (the completion counter tells it), so
// nobody waits for stragglers; blocks are finalized in order (a done-counter per ring-slot parity), and the forward task of
// block c + 2 publishes its spectrum only after block c's frames are out, so that no inverse task of block c + 2 -- whose
// frames wrap onto them in the ring -- starts earlier.  No partial sums in HBM, no second kernel, no tail.  Frames are numbered through the workgroup's clips (clip ordinal x
// T' + m), so that the last frames of one clip and the first of the next sit side by side in the ring.
// The ring length (a power of two, FftParams::stream_ring, chosen by the host as large as the LDS allows) sets how far ahead
// the forward tasks may run: block s may publish its spectrum once block s - D is out, D = wg_stream_lag(ring) (even, so
// that both sit on the same ring-slot parity).  The smallest ring gives D = 2 -- the forward wave then idles until the
// block two behind is finalized, ~0.8 task per block, measured +5 % on the kernel; twice that ring gives D >= 4 and
// nobody waits.
constexpr int wg_pow2_ceil(int v) { int r = 1; while (r < v) r <<= 1; return r; }
// filters-done counters: one per block modulo 8 (sq[set & 7], behind the ring; target ((set >> 3) + 1) F).  Blocks 8 apart share one, so
// the forward lag is capped at 6: block s + 8 cannot start before block s + 2 is finalized, i.e. long after block s.
constexpr int kWgStreamMaxLag = 6;
constexpr int wg_stream_lag(int SK, int SHOP, int ring) {
    const int padl = SK / 2 + SK % 2 - 1, ls = fft_block_len(SK, SHOP, true);
    const int dmax = (ls - 1 + padl) / SHOP, mf = (ls - SK + padl) / SHOP, fb = ls / SHOP;
    // frames written by block s reach s fb + dmax; block j is final through j fb + mf: (s fb + dmax) - ring <= j fb + mf
    const int lag = ((ring + mf - dmax) / fb) & ~1;
    return lag > kWgStreamMaxLag ? kWgStreamMaxLag : lag;
}
constexpr int wg_stream_ring_min(int SK, int SHOP) {                      // smallest ring with a lag of 2
    int r = 8;
    while (wg_stream_lag(SK, SHOP, r) < 2) r <<= 1;
    return r;
}
constexpr int wg_stream_fp(int F) { return F | 1; }                       // filters padded to an odd count (bank spread)
// Output staging of the streaming finalize: a block completes ~10 frames of every filter's row, which written as they come
// are 4-byte stores at stride T' (measured 2.4x the output's bytes at the memory side, round 3).  The finished values are
// parked in LDS instead, [F][kWgOutRow] (two chunks of 32 frames, by chunk parity, + 1 pad), and a 32-frame chunk of every
// row goes out together once its last frame is final (or the clip ends): 128 contiguous bytes per row and store
// instruction.  A block completes fewer than 32 frames, so it touches at most two consecutive chunks, and the older of the
// two slots it may write held a chunk that an earlier block completed and flushed.
constexpr int kWgOutChunk = 32;
constexpr int kWgOutRow = 2 * kWgOutChunk + 1;
// Round 5: the finalizing wave raises its issue priority for the duration.  With the band tasks a block is ~19 tasks, and the
// blocks' finalizes are ONE dependent chain through the launch (in order: the EMA state) of ~900 latency-bound instructions per
// block on a wave that shares its SIMD with two transform waves: traced at 7-30 k cycles of a ~21 k-cycle block period, each
// starting 11-35 k cycles late -- 13-16 % of the kernel.  s_setprio 3: BASELINE configs[4] 1.0605 -> 0.8946 ms, configs[3]'s shape
// 0.2390 -> 0.2073 ms, same box (profiles/r05/ab_stream_finalize.txt; now ahead of the partial-sum path it replaces).  Also
// measured there: five frames interleaved instead of four (nothing) and every filter task finalizing its own row with lane =
// frame (8-10 % slower: bookkeeping on every task, a point function per 30 frames of one filter instead of per 400 of forty).
constexpr size_t fft_wg_stream_lds_bytes(int NW, int SK, int ring, int F) {      // + frame ring, EMA state, per-filter coefficients, output staging
    return fft_wg_lds_bytes(NW, SK) + ((size_t)ring * wg_stream_fp(F) + wg_stream_fp(F) + 8 * (size_t)F + 8 +
                                       (size_t)F * kWgOutRow) * 4;
}

// ---- one loader and one tail tile per instance ------------------------------------------------------------------------------
// The sample kind of the waveform (XK) and the tile form of the tail (TAILC, wg_tail_finalize) are compile-time: the host knows both
// (FwdIo::xtype, the call's mix, T') and every launch ran exactly one of the three load loops and one of the two tiles, with the
// others' code -- ~19 KB of an 80 KB kernel -- around the task loop in a 64 KB instruction cache.  fp32; 16-bit (bfloat16 and PCM16
// share a loop: a wave-uniform select of the conversion); mixed fp32; mixed PCM16 (leaf_common.hpp; a mixed load is ~3 KB of code
// and the kernel has two load sites, so the two mixed sample types are an instance each).  Since the row-owned tail (wg_tail_rows,
// below) TAILC only selects the chunk length of a row, 128 or 64 frames; the instance set and the host's choice by T' are as they were.
// The STREAM instances keep the choice at run time (kWgXAny: the three loops of one load site, as before the split): they do not take the
// early path, so they have one load site, and with a single loader they measured 0.6-1.3 % slower at the shapes that run them
// (profiles/early_forward.txt) -- the split stays where the second load site needs it.
constexpr int kWgXF32 = 0, kWgX16 = 1, kWgXMix = 2, kWgXMix16 = 3;
constexpr int kWgXAny = 4;
// The block gb of the launch, rotated left by padL samples, into the wave's registers: are[r] = sample 64 r + lane of the rotated
// block, zero outside [0, T) (both partners, mixed); (b, c) = the block's clip and its index in the clip.  The one load site of the
// forward transforms: the queue's forward task and the two early first blocks (below).
template <int SK, int SHOP, int XK>
__device__ __forceinline__ void wg_load_block(const FftParams& p, int gb, int lane, float (&are)[32], int& b, int& c) {
    constexpr int PADL = SK / 2 + SK % 2 - 1;
    constexpr int LS = fft_block_len(SK, SHOP, true);
    // which load loop: compile-time constants in the instances of one kind, the call's own (wave-uniform) for kWgXAny
    constexpr bool ANY = XK == kWgXAny;
    b = gb / p.nblk;                                                      // the only division per block
    c = gb - b * p.nblk;
    const int n_c = c * LS;
    const float* xb = static_cast<const float*>(p.x) + (size_t)b * p.T;
    const unsigned short* xh = static_cast<const unsigned short*>(p.x) + (size_t)b * p.T;
    if (ANY ? p.mix_lam != nullptr : (XK == kWgXMix || XK == kWgXMix16)) {
        // waveform mixup in the load (leaf_common.hpp): the block's clip mixed with its partner, weights and partner row
        // read once per block; a loop per sample type (fp32 / 16-bit PCM)
        const MixClip mc = mix_clip(p.mix_perm, p.mix_lam, b, p.B, p.T);
        const size_t row = (size_t)b * p.T;
        if constexpr (ANY) {
            // (one loop for both sample types, a wave-uniform select of the load as in the 16-bit loop below: the instance that keeps
            // every loader stays inside the size of the kernel it replaces)
            const int st = p.io_bf16 == kSamplePcm16 ? kSamplePcm16 : kSampleF32;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = 64 * r + lane;
                const int n = n_c - PADL + ((i + PADL) & (kFftN - 1));
                const float w = mix_load(p.x, row, mc.partner, (size_t)min(max(n, 0), p.T - 1), mc.lam, mc.om, st);
                are[r] = (n >= 0 && n < p.T) ? w : 0.0f;
            }
        } else if (XK == kWgXMix16) {
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = 64 * r + lane;
                are[r] = mix_sample<kSamplePcm16>(p.x, row, mc, n_c - PADL + ((i + PADL) & (kFftN - 1)), p.T);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = 64 * r + lane;
                are[r] = mix_sample<kSampleF32>(p.x, row, mc, n_c - PADL + ((i + PADL) & (kFftN - 1)), p.T);
            }
        }
    } else if (ANY ? p.io_bf16 != 0 : XK == kWgX16) {
        const bool pcm = p.io_bf16 == kSamplePcm16;     // 16-bit PCM shares the loop: a wave-uniform select of the conversion
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const int i = 64 * r + lane;                      // block rotated left by padL samples
            const int n = n_c - PADL + ((i + PADL) & (kFftN - 1));
            const unsigned v = xh[min(max(n, 0), p.T - 1)];
            const float w = pcm ? pcm16_widen((short)v) : __uint_as_float(v << 16);
            are[r] = (n >= 0 && n < p.T) ? w : 0.0f;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const int i = 64 * r + lane;
            const int n = n_c - PADL + ((i + PADL) & (kFftN - 1));
            are[r] = (n >= 0 && n < p.T) ? xb[n] : 0.0f;
        }
    }
}

// ---- the tail: every wave finalizes the rows it owns ---------------------------------------------------------------------------
// After the drain barrier (release fence + __syncthreads at the end of the task loop: every frame sum of the clips this workgroup owns
// is in its LDS, or in L2) the rows [b_lo F, b_hi F) are dealt to the NW waves -- row counts differ by at most one: 3 or 4 of the
// default forward's 40 -- and a wave takes its rows end to end in its OWN transposition scratch, kWgTailRows rows at a time, CH frames
// per chunk.  No barrier and no other wave's data behind the drain barrier: a wave's LDS operations execute in order, so the
// wavefront-scope fences below (compiler ordering; s_waitcnt lgkmcnt is all the hardware needs) are the only synchronisation.
//   (1) lane = live frame of the chunk, the rows side by side: the sums (LDS, or `part` past the vector cache with relaxed
//       agent-scope loads, see fft_finalize_tile; a pass's loads are issued together) -> fin_pooled -> raw_out -> floor -> P;
//   (2) lane r < rows: the smoother's recurrence of row r down the frames (fin_ema_step, state from p_0, frame 0 through the step
//       too, the carry in a register between chunks) -> M;
//   (3) lane = (row, frame of a 16-frame group): the point function and the store.
// (2) of group g + 1 is issued with (3) of group g: the recurrence's dependent operations on a few lanes beside 64 lanes of log2 /
// exp2 chains, and beside the two other waves of the SIMD, which are in their own rows.  What the tail costs is instruction issue --
// 4 cycles per wave instruction, 8 for log2 / exp2 / rcp -- so each stage is written for few instructions per row.  The arithmetic is fin_*'s, in
// the order fft_finalize_tile and the streaming finalize apply it: the row kernel stays an independent implementation of the same bits.
// PCEN off and filters with delta <= 0 (the reference's literal powf) take a compact rolled form beside the hot loop.
constexpr int kWgTailRows = 4, kWgTailGroup = 16;                         // 4 rows x 16 frames: the 64 lanes of the point stage
constexpr int wg_tail_stride(int CH) { return CH + kWgTailGroup; }        // rows 16 banks apart: a group of the four rows meets every bank once
constexpr int wg_tail_floats(int CH) { return 2 * kWgTailRows * wg_tail_stride(CH); }
template <int NW, int CH>
__device__ __forceinline__ void wg_tail_rows(const FinParams& q, int b_lo, int b_hi, float* scr, int wave, int lane) {
    static_assert(CH == 64 || CH == 128, "chunk lengths of the tail");
    constexpr int RB = kWgTailRows, GF = kWgTailGroup, S = wg_tail_stride(CH);
    float* P = scr;                                                       // [RB][S] floored pooled values of the chunk
    float* Mt = scr + RB * S;                                             // [RB][S] smoothed values
    const int TP = q.TP, mode = q.mode;
    const SlotGeom geo = q.geo;
    const bool scaled = q.clip_scale2 != nullptr, pcen = (mode & 1) != 0;
    auto ld = [](const float* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto wave_fence = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); };
    const int nrows_all = (b_hi - b_lo) * q.F;
    if (nrows_all <= 0) return;
    const int per = nrows_all / NW, rem = nrows_all - per * NW;
    const int my0 = b_lo * q.F + wave * per + min(wave, rem), mycnt = per + (wave < rem ? 1 : 0);
    for (int r0 = 0; r0 < mycnt; r0 += RB) {
        const int row0 = my0 + r0, nr = min(RB, mycnt - r0);
        // lane -> its row of the point stage (lanes past the last row repeat it and store nothing), that row's coefficients and scale
        const int rl = min(lane >> 4, nr - 1), jl = lane & (GF - 1);
        const int rowl = row0 + rl, bl = rowl / q.F, fl = rowl - bl * q.F;
        const FinCoef c = q.lds_coef ? static_cast<const FinCoef*>(q.lds_coef)[fl] : fin_coef(q, fl);
        const float s2l = scaled ? q.clip_scale2[bl] : 1.0f;
        const bool mine = (lane >> 4) < nr;
        // lane -> its row of the recurrence (lanes past the last row repeat it: the same values to the same addresses)
        const int re = min(lane, nr - 1);
        FinCoef ce{};
        ce.w = __shfl(c.w, GF * re);
        ce.omw = __shfl(c.omw, GF * re);
        const bool fast = pcen && __all(c.dl > 0.0f);                     // every row on the cancellation-free PCEN form
        const float* prow = P + re * S;
        float* mrow = Mt + re * S;
        auto ema_group = [&](int g, float M) {                            // the GF frames from g GF on, of row `re`
            float pv[GF];
#pragma unroll
            for (int k = 0; k < GF; ++k) pv[k] = prow[g * GF + k];
#pragma unroll
            for (int k = 0; k < GF; ++k) {
                M = fin_ema_step(ce, pv[k], M);
                mrow[g * GF + k] = M;
            }
            return M;
        };
        float carry = 0.0f;
        for (int m0 = 0; m0 < TP; m0 += CH) {
            const int nfr = min(CH, TP - m0);
            wave_fence();                                                 // the previous chunk's reads of P and M are issued
            // ---- (1) lane = frame, the batch's rows side by side: their loads are issued together from clamped, always valid
            // addresses; a row's base address, bias and scale are wave-uniform (the coefficients sit in lane 16 r)
            for (int j0 = 0; j0 < nfr; j0 += 64) {
                const bool on = j0 + lane < nfr;
                const int j = min(j0 + lane, nfr - 1), m = m0 + j;
                float a[RB], b2[RB], c3[RB];
                int ns = 1;
                if (q.lds_sums) {                                         // the slots were added up in LDS (a + b: the same rounding)
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        a[r] = q.lds_sums[(size_t)(row0 + min(r, nr - 1) - q.lds_row0) * TP + m];
                        b2[r] = c3[r] = 0.0f;
                    }
                } else {
                    ns = fin_slots(geo, m);
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        const float* pr = q.part + (size_t)(row0 + min(r, nr - 1)) * geo.nslot * TP + m;
                        a[r] = ld(pr);
                        b2[r] = ld(pr + (ns > 1 ? TP : 0));
                        c3[r] = geo.nslot > 2 ? ld(pr + (ns > 2 ? 2 * TP : 0)) : 0.0f;
                    }
                }
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const float bias = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.bias), GF * r));
                    const float s2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s2l), GF * r));
                    float v = fin_pooled(a[r], b2[r], c3[r], ns, scaled, s2, bias);
                    if (on && r < nr) {
                        if (q.raw_out) q.raw_out[(size_t)(row0 + r) * TP + m] = v;
                        if (!(mode & 8)) v = pooled_floor(v);
                        P[r * S + j] = v;
                    }
                }
            }
            wave_fence();                                                 // P is written
            const int ng = (nfr + GF - 1) / GF;
            const size_t orow = (size_t)rowl * TP + m0;
            if (fast) {
                // ---- (2) + (3): the recurrence runs one group ahead of the point stage.  In the chunk's last group it walks past the
                // last frame over stale scratch: values nothing reads (a chunk that is cut short is the row's last, so its carry is
                // not used either).
                float M = ema_group(0, m0 == 0 ? prow[0] : carry);        // state starts at p_0 (postprocessing.py:15)
                for (int g = 0; g < ng; ++g) {
                    wave_fence();                                         // M of group g is written
                    const int j = g * GF + jl;
                    const float pv = P[rl * S + j], mv = Mt[rl * S + j];
                    if (g + 1 < ng) M = ema_group(g + 1, M);
                    const float o = fin_point_pcen_pos(c, q.floor_, pv, mv);
                    if (mine && j < nfr) fin_store(q, orow + j, o);
                }
                carry = M;
            } else {
                if (pcen) {
                    float M = m0 == 0 ? prow[0] : carry;
#pragma nounroll
                    for (int j = 0; j < nfr; ++j) {
                        M = fin_ema_step(ce, prow[j], M);
                        mrow[j] = M;
                    }
                    carry = M;
                    wave_fence();
                }
#pragma nounroll
                for (int g = 0; g < ng; ++g) {
                    const int j = g * GF + jl;
                    const float o = fin_point(c, mode, q.floor_, P[rl * S + j], pcen ? Mt[rl * S + j] : 0.0f);
                    if (mine && j < nfr) fin_store(q, orow + j, o);
                }
            }
        }
    }
}

// The kernel's body; the two __global__ templates below name its instances (leaf_fft_wg_kernel: fp32 samples, rows of <= 128
// frames -- what the default forward runs; leaf_fft_wg_kernel_var: every other (sample kind, tail) pair).
template <int SK, int SHOP, int NW, bool STREAM, int XK, int TAILC>
__device__ __forceinline__ void leaf_fft_wg_body(const FftParams& p) {
    constexpr bool HALF = NW > 12;                                        // 16 rows of transposition scratch per wave
    constexpr int SCRF = fft_wg_scr_floats(NW);
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    float2* twl = reinterpret_cast<float2*>(wsm);                        // [32][64]
    float2* twh = twl + 32 * 64;                                          // [32][2]
    float2* ring = twh + 64;                                              // [2][kWgRingFwdFloat2]
    int* q = reinterpret_cast<int*>(ring + 2 * kWgRingFwdFloat2);         // the task queue (leaf_wg_queue.hpp)
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane0 = tid & 63;
#if LEAF_TRACE
    const unsigned long long tr_entry = __builtin_amdgcn_s_memtime();    // kernel entry (written behind the first barrier: WG_STAMP_AT)
    const unsigned long long tr_entry_rt = __builtin_amdgcn_s_memrealtime();   // ... on the 100 MHz clock too: the shader clock follows from the pair
#endif
    float* scr = reinterpret_cast<float*>(q + kWgQueueInts) + (size_t)wave * SCRF;
    // STREAM: frame ring [RING][FPS] (one accumulator per frame and filter: the blocks a window meets ADD their sums, the
    // finalize reads it and puts the zero back) and the EMA state [FPS] behind the waves' scratch
    const int RING = p.stream_ring;                                       // power of two (host: fft_forward)
    const int FPS = wg_stream_fp(p.F);
    float* fr = reinterpret_cast<float*>(q + kWgQueueInts) + (size_t)NW * SCRF;
    float* ema_st = fr + (size_t)RING * FPS;
    FinCoef* coefT = reinterpret_cast<FinCoef*>(ema_st + FPS);             // [F]: the filters' finalize coefficients, once per launch
    static_assert(sizeof(FinCoef) == 32, "8 floats per filter");
    int* sq = reinterpret_cast<int*>(coefT + p.F);                        // [8]: filters done per block (modulo 8)
    float* ost = reinterpret_cast<float*>(sq + 8);                        // [F][kWgOutRow]: finished outputs, two chunks by parity
    (void)fr; (void)ema_st; (void)coefT; (void)sq; (void)ost;
    // fin_fused == 3 (not STREAM): the per-frame sums of the clips this workgroup owns, [clip][filter][T'] floats behind the
    // waves' scratch -- every workgroup gets whole clips and they fit (cfg1: one clip, 40 x 100 x 4 B = 16 KB).  The two
    // blocks a window meets add their sums with ds_add_f32 (a + b either way round: the rounding of `part`'s slot 0 + slot 1),
    // the tail reads them from LDS: no partial sums in HBM for these clips.
    float* lsum = reinterpret_cast<float*>(q + kWgQueueInts) + (size_t)NW * SCRF;
    const bool lds_sums = !STREAM && p.fin_fused == 3;
    const unsigned scr_lds = __builtin_amdgcn_readfirstlane(
        (unsigned)(size_t)(__attribute__((address_space(3))) float*)scr);   // LDS byte address of this wave's scr
    // band-limited filter tasks (leaf_band.hpp): the plan sits behind everything else
    constexpr bool BANDK = !HALF && band_geometry_ok(SK, SHOP);
    const bool band_on = BANDK && p.band.rec != nullptr;
    int* bl = reinterpret_cast<int*>(wsm + p.band.lds_off);
    (void)bl;
    if constexpr (BANDK) {
        if (band_on && wave == 0) band_build_plan(p.band.rec, p.band.elist, p.band.n_edge, p.F, bl, lane0, p.band.bias, p.band.smax);
    }

    // The workgroup's first block: its spectrum was computed by the table launch on otherwise idle waves (p.spec0; this transform is
    // the one task nothing here could overlap with: eleven waves waited ~12 k cycles for it).  Wave 1 requests it before the tables
    // are built and publishes it right after the barrier; the task queue then starts behind fwd(0).
    const bool spec_pre = p.spec0 != nullptr && !HALF && p.B * p.nblk > 0;
    float2 sv[kWgFwdBins / 64];                                           // bins 0..1151 (kWgFwdBins)
    if (spec_pre && wave == 1) {
        const float2* src = p.spec0 + (size_t)blockIdx.x * kWgRingFwdFloat2;
#pragma unroll
        for (int k = 0; k < kWgFwdBins / 64; ++k) sv[k] = src[64 * k + lane0];
    }
    // Without p.spec0 (the table cache validated and returned; 16-bit PCM; a mixed call; prepared tables) the workgroup's first TWO
    // blocks are requested here, at the kernel's first instructions: nothing in a forward transform's loads depends on the tables or the
    // plan, and left to the task queue they started only after the barrier -- 32 loads per lane, cold from HBM, with eleven waves
    // waiting behind them.  Wave NW - 1 takes block 0, wave NW - 2 block 1 (wave 0 has the plan); both still build twiddles below (the
    // loads are in flight meanwhile), transform right after the barrier and publish as fwd(0) / fwd(1) do; the queue starts behind them.
    // The waves that leave the barrier beside them request their first tasks' table rows meanwhile.  Not in the STREAM instances
    // (whole clips per workgroup, 20+ blocks each at the shapes that run them: the start is amortised, and the second transform's
    // 9.5 KB of code would put them above the size of the kernel they replace).
    constexpr bool EARLYK = !HALF && !STREAM;
    const bool early = EARLYK && p.spec0 == nullptr;
    const int eset = NW - 1 - wave;                                       // the set an early wave transforms: 0 or 1
    bool early_me = false;
    float ex[32];
    int eb = 0, ec = 0;
    if constexpr (EARLYK) {
        const OwnedClips deal0{p.B * p.nblk, (int)gridDim.x, p.nblk};    // (the dealing, as below)
        early_me = early && eset < 2 && eset < deal0.count((int)blockIdx.x);
        if (early_me) wg_load_block<SK, SHOP, XK>(p, deal0.start((int)blockIdx.x) + eset, lane0, ex, eb, ec);
    }
    // (while wave 0 builds the plan -- one global round trip -- the other waves build the twiddle tables)
    if (BANDK && band_on) { if (wave > 0) fft_build_twiddles_wg(twl, twh, tid - 64, (NW - 1) * 64); }
    else fft_build_twiddles_wg(twl, twh, tid, NW * 64);
    // (early: tasks 0 and 1 are fwd(0) and fwd(1) -- task 1 the skipped slot when nset == 1)
    if (tid < kWgQueueInts) q[tid] = (tid == 0 && spec_pre) ? 1 : (tid == 0 && early) ? 2 : 0;
    if constexpr (STREAM) {
        for (int f = tid; f < p.F; f += NW * 64) coefT[f] = fin_coef(p.fin, f);
        if (tid < 8) sq[tid] = 0;
        for (int i = tid; i < RING * FPS; i += NW * 64) fr[i] = 0.0f;
    }
    FinCoef* lcoef = nullptr;                                             // (lds_sums) the filters' finalize coefficients, for the tail
    if (lds_sums) {
        const int n = (int)((long long)p.B * p.nblk / (int)gridDim.x / p.nblk) * p.F * p.TP;    // clips per workgroup x F x T'
        for (int i = tid; i < n; i += NW * 64) lsum[i] = 0.0f;
        lcoef = reinterpret_cast<FinCoef*>(lsum + (n + 7) / 8 * 8);
        // (from wave NW - 3 downwards: wave 0 builds the plan, and the last two hold their first blocks' loads -- memory returns in
        // order, so a coefficient load behind those would wait for them before the barrier)
        constexpr int NC = NW > 2 ? (NW - 2) * 64 : NW * 64;
        if (tid < NC)
            for (int f = NC - 1 - tid; f < p.F; f += NC) lcoef[f] = fin_coef(p.fin, f);
    }
    __syncthreads();
#if LEAF_TRACE
    // phase stamps of workgroup 0, waves 0..7 (tools/trace_wg.py): tag << 56 | s_memtime
    int tr_n = 0;
#define WG_STAMP(tag)                                                                                           \
    do {                                                                                                        \
        if (LEAF_TRACE == 2 && (tag) != 1 && (tag) != 2 && (tag) < 8) break;   /* 2: task starts and finalize stamps only */ \
        if (blockIdx.x == 0 && wave < 16 && lane0 == 0 && tr_n < 56)                                            \
            p.trace[wave * 64 + tr_n] = ((unsigned long long)(tag) << 56) | (__builtin_amdgcn_s_memtime() & 0x00FFFFFFFFFFFFFFull); \
        ++tr_n;                                                                                                 \
    } while (0)
    // the launch's fixed costs -- start, drain, tail -- at fixed slots behind the 56 running stamps of a wave (every trace level):
    // slot 56 kernel entry (tag 14), 57 out of the first barrier (15), 58 the workgroup's first spectrum published (16: the wave
    // that published it), 59 the wave's last task done (17), 60 out of the drain barrier (18), 61 the wave's rows finalized (19)
    // 62 / 63: the 100 MHz clock (s_memrealtime) at kernel entry and beside slot 61 (tags 20 / 21)
#define WG_STAMP_AT(slot, tag, when)                                                                            \
    do {                                                                                                        \
        if (blockIdx.x == 0 && wave < 16 && lane0 == 0)                                                         \
            p.trace[wave * 64 + (slot)] = ((unsigned long long)(tag) << 56) | ((when) & 0x00FFFFFFFFFFFFFFull); \
    } while (0)
#define WG_STAMP_NOW(slot, tag) WG_STAMP_AT(slot, tag, __builtin_amdgcn_s_memtime())
    WG_STAMP_NOW(57, 15);
    WG_STAMP_AT(56, 14, tr_entry);
    WG_STAMP_AT(62, 20, tr_entry_rt);
#else
#define WG_STAMP(tag) do { } while (0)
#define WG_STAMP_AT(slot, tag, when) do { } while (0)
#define WG_STAMP_NOW(slot, tag) do { } while (0)
#endif

    constexpr int PADL = SK / 2 + SK % 2 - 1;
    constexpr int LS = fft_block_len(SK, SHOP, true);
    constexpr int DMIN = -((SK - 1 - PADL) / SHOP);
    constexpr int DMAX = (LS - 1 + PADL) / SHOP;
    constexpr int NFR = DMAX - DMIN + 1;
    constexpr int NROW = LS / 64;
    constexpr int NGRP = (NFR + 15) / 16;
    static_assert(LS % SHOP == 0 && LS % 64 == 0 && LS > 0 && NFR <= 32 && (SK & 1), "static odd-window geometry");
    static_assert(!STREAM || (LS + SK - PADL) / SHOP + 2 <= kWgOutChunk, "a block completes fewer frames than one output chunk");

    // Task ids: F + 1 slots per set (wg_task_decode); slot 0 of set i is fwd(i + 1), slots 1..F are the set's filters.
    // blocks are dealt CONTIGUOUSLY (workgroup w: blocks [first_gb, first_gb + nset)): a clip's blocks stay on one CU (the
    // overlap-save halo is re-read from this CU's cache) and a clip all of whose blocks this workgroup ran is finalized in
    // the tail below without another kernel
    const OwnedClips deal{p.B * p.nblk, (int)gridDim.x, p.nblk};
    if (spec_pre && wave == 1) {                                          // fwd(0): ring slot 0, generation 0
        const int gb0 = deal.start((int)blockIdx.x);
#pragma unroll
        for (int k = 0; k < kWgFwdBins / 64; ++k) ring[64 * k + lane0] = sv[k];
        wg_publish(q, 0, gb0 / p.nblk, gb0 % p.nblk, lane0);
        WG_STAMP_NOW(58, 16);
    }
    if (early_me) {
        // fwd(eset): ring slot eset, generation 0 -- no reader of an earlier occupant to wait for; published as the queue's forward task does
        WG_STAMP(1);
        float eim[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) eim[r] = 0.0f;
        fft2048w<HALF>(ex, eim, scr, scr_lds, twl, twh, lane0);           // register i <-> bin 64 brev5(i) + lane
        float2* A = ring + eset * kWgRingFwdFloat2;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int k = brev5(i);
            if (k < kWgFwdBins / 64) A[64 * k + lane0] = make_float2(ex[i], eim[i]);
        }
        wg_publish(q, eset, eb, ec, lane0);
        if (eset == 0) WG_STAMP_NOW(58, 16);
    }
    const int first_gb = deal.start((int)blockIdx.x);
    const int nset = deal.count((int)blockIdx.x);                         // blocks of this workgroup
    const int NT = band_on ? __builtin_amdgcn_readfirstlane(bl[0]) : p.F;   // filter tasks per block
    const int* tdesc = bl + kBandPlanHead;
    const int* bmem = tdesc + p.F + 4;
    (void)tdesc; (void)bmem;
    const WgTaskCursor cur = wg_task_cursor(q, lane0, NT, nset);          // NT + 1 slots per set
    // descriptor of a filter task: class (0: one filter on 2048 points, 1 / 2: band task) | index << 2 (filter / first member)
    auto desc_of = [&](int role) {
        if (role <= 0 || role > NT) return 0;
        return band_on ? __builtin_amdgcn_readfirstlane(tdesc[role - 1]) : (role - 1) << 2;
    };
    float rq[32];                                                         // R_f[64 k + lane], natural row order
    // the 32 table values the task `role` starts with: a spectrum row, or the bins of a band task's windows (row 0 as a dummy
    // when there is no filter task)
    auto prefetch_task = [&](int role, int lane) {
        const int d = desc_of(role);
        if constexpr (BANDK) {
            if ((d & 3) == 1) { band_load_spectrum<16>(rq, reinterpret_cast<const float*>(p.H), bmem[(d >> 2) + lane / band_lpf(16)], lane); return; }
            if ((d & 3) == 2) { band_load_spectrum<32>(rq, reinterpret_cast<const float*>(p.H), bmem[(d >> 2) + lane / band_lpf(32)], lane); return; }
        }
        wg_load_real_spectrum(rq, p.H, d >> 2, lane);
    };

    // ---- STREAM: finalize the frames that set j's block completed (see the comment above the kernel); one wave, lane = filter
    auto stream_finalize = [&](int j) {
        // called by the wave that completed set j's last filter; blocks go out in order (EMA state, and set j - 1's sums)
        WG_STAMP(10);                                                     // finalize: waiting for the previous block's
        if (j > 0) wg_wait_ge(wgq_stream_out_cnt(q, (j - 1) & 1), ((j - 1) >> 1) + 1);
        WG_STAMP(8);                                                      // finalize: start
        __builtin_amdgcn_s_setprio(3);                                    // (see above: the launch's one dependent chain goes first)
        const int gb = first_gb + j;
        const int b = gb / p.nblk, c = gb - b * p.nblk;
        const int gbase = ((gb - first_gb) / p.nblk) * p.TP;              // ring numbering: clip ordinal x T' + m
        // frames final once block c is through: window end m hop - padL + K - 1 <= (c + 1) L - 1; the clip's last block
        // completes all that remain
        const int mf_prev = c == 0 ? -1 : min(p.TP - 1, (c * LS - SK + PADL) / SHOP);
        const int mf = c == p.nblk - 1 ? p.TP - 1 : min(p.TP - 1, ((c + 1) * LS - SK + PADL) / SHOP);
        const int mode = p.fin.mode;
        const bool scaled = p.fin.clip_scale2 != nullptr;
        const float s2 = scaled ? p.fin.clip_scale2[b] : 1.0f;
#ifndef LEAF_STREAM_ABLATE
#define LEAF_STREAM_ABLATE 0       // measurement only (results wrong): 1 = the finalize loop is skipped, 2 = only its stores are
#endif
        // Four frames at a time: (A) the slots, the pooled values and the EMA recurrence -- the only sequential part, three
        // operations per frame -- into registers; (B) four INDEPENDENT point functions, straight-line, so that the scheduler
        // interleaves their dependent chains (log2 / exp2 / rcp at 16+ cycles each): finalized one frame after the other, a
        // lone wave on a SIMD shared with two transform waves took ~25 cycles per instruction, 4 task-times per block.
        constexpr int G = 4;
        for (int f0 = 0; f0 < p.F && LEAF_STREAM_ABLATE != 1; f0 += 64) {
            const int f = f0 + lane0;
            const bool on = f < p.F;
            const FinCoef cf = coefT[on ? f : 0];
            const bool fast = __all(!on || cf.dl > 0.0f);                 // every filter on the cancellation-free PCEN form
            float M = (c == 0 || !on) ? 0.0f : ema_st[f];
            const size_t orow = ((size_t)b * p.F + (on ? f : 0)) * p.TP;
            for (int base = mf_prev + 1; base <= mf; base += G) {
                const int cnt = min(G, mf - base + 1);
                float sa[G], sb[G], v[G], Mv[G];
                int ns[G];
#pragma unroll
                for (int k = 0; k < G; ++k) {                            // (A) loads first
                    const int m = min(base + k, mf);
                    // the frame's accumulator: a (+ b when the window meets two blocks: added in LDS, a + b either way round -- the
                    // rounding of `part`'s slot 0 + slot 1); read, and zero for the frame that wraps onto it
                    float* e = fr + (size_t)((gbase + m) & (RING - 1)) * FPS + (on ? f : 0);
                    ns[k] = 1;
                    sa[k] = e[0];
                    sb[k] = 0.0f;
                    if (on && k < cnt) e[0] = 0.0f;
                }
#pragma unroll
                for (int k = 0; k < G; ++k) {                            // ... then the recurrence, in frame order
                    const int m = base + k;
                    float x = fin_pooled(sa[k], sb[k], 0.0f, ns[k], scaled, s2, cf.bias);
                    if (k < cnt && on && p.fin.raw_out) p.fin.raw_out[orow + m] = x;
                    if (!(mode & 8)) x = pooled_floor(x);
                    v[k] = x;
                    if ((mode & 1) && k < cnt) {
                        if (m == 0) M = x;                                // state starts at p_0 (postprocessing.py:15)
                        M = fin_ema_step(cf, x, M);
                    }
                    Mv[k] = M;
                }
                if (fast && (mode & 1)) {                                 // (B) branch-free: the chains of the eight frames interleave
                    float o[G];
#pragma unroll
                    for (int k = 0; k < G; ++k) o[k] = fin_point_pcen_pos(cf, p.fin.floor_, v[k], Mv[k]);
#pragma unroll
                    for (int k = 0; k < G; ++k)
                        if (k < cnt && on && (LEAF_STREAM_ABLATE != 2 || o[k] == 12345.678f))
                            ost[f * kWgOutRow + ((base + k) & (2 * kWgOutChunk - 1))] = o[k];
                } else {
                    // PCEN off, or a filter with delta <= 0 (the reference's literal powf form): one compact out-of-line
                    // point function, frame after frame -- rare, and the code of this kernel has to stay inside the
                    // instruction cache next to the transforms (87 KB with this path unrolled: the whole kernel ran 15 % slower)
#pragma unroll
                    for (int k = 0; k < G; ++k) {
                        const float ov = fin_point_outofline(cf, mode, p.fin.floor_, v[k], Mv[k]);
                        if (k < cnt && on) ost[f * kWgOutRow + ((base + k) & (2 * kWgOutChunk - 1))] = ov;
                    }
                }
            }
            if (on) ema_st[f] = M;
        }
        // ---- flush: every 32-frame chunk of the clip's rows whose last frame is now final (the clip's last block: also the
        // partial chunk at its end).  Chunks q with (q + 1) 32 - 1 <= mf_prev went out with an earlier block.
        if (LEAF_STREAM_ABLATE != 1) {
            const int q0 = (mf_prev + 1) / kWgOutChunk;
            const int q1 = c == p.nblk - 1 ? (p.TP - 1) / kWgOutChunk : (mf + 1) / kWgOutChunk - 1;   // last chunk that is complete
            for (int qc = q0; qc <= q1; ++qc) {
                const int m = qc * kWgOutChunk + (lane0 & (kWgOutChunk - 1));
                for (int r0 = 0; r0 < p.F; r0 += 64 / kWgOutChunk) {
                    const int row = r0 + lane0 / kWgOutChunk;
                    if (row < p.F && m < p.TP)
                        fin_store(p.fin, ((size_t)b * p.F + row) * p.TP + m, ost[row * kWgOutRow + (m & (2 * kWgOutChunk - 1))]);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        WG_STAMP(9);                                                      // finalize: done
        wg_release();                // ring entries read, EMA state written: block j is out
        wg_bump(wgq_stream_out_cnt(q, j & 1), lane0);
    };
    (void)stream_finalize;

    // Invariant at the loop head: (set, role) is the decoded current task, and when it is an inverse task its filter's
    // spectrum row has already been requested into rq (by the previous task, under its pooling).
    int seen_set = -1, seen_b = 0, seen_c = 0, seen_base = 0, seen_clip = 0;   // block coordinates of the set this wave last worked on
    int set = 0, role = 0;
    int t = cur.next(set, role);
    prefetch_task(role, lane0);
    while (cur.has(t)) {
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const int slot = set & 1, gen = set >> 1;
        float2* A = ring + slot * kWgRingFwdFloat2;
        WG_STAMP(role == 0 ? 1 : 2);                                      // task taken: 1 forward transform, 2 filter
        if (role == 0) {
            // ---- forward transform of block gb into ring slot `slot` (skipped past the last set)
            if (set < nset) {
                float are[32], aim[32];
                int fb, fc;                                               // the block's clip and its index in the clip
                wg_load_block<SK, SHOP, XK>(p, first_gb + set, lane, are, fb, fc);
#pragma unroll
                for (int r = 0; r < 32; ++r) aim[r] = 0.0f;
                fft2048w<HALF>(are, aim, scr, scr_lds, twl, twh, lane);        // register i <-> bin 64 brev5(i) + lane
                wg_wait_ge(wgq_readers_cnt(q, slot), gen * NT);           // the slot's previous readers are done
                if constexpr (STREAM) {                                   // ... and the frames ours wrap onto in the ring are out
                    const int lag = wg_stream_lag(SK, SHOP, RING);        // (block set - lag: same parity, (lag / 2) generations back)
                    if (set >= lag) wg_wait_ge(wgq_stream_out_cnt(q, slot), gen - lag / 2 + 1);
                }
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int k = brev5(i);
                    if (k < kWgFwdBins / 64) A[64 * k + lane] = make_float2(are[i], aim[i]);     // bins 0..1151: 1025.. for band windows that cross Nyquist
                }
                wg_publish(q, slot, fb, fc, lane);
                if (set == 0) WG_STAMP_NOW(58, 16);
            }
            // rq is redefined UNCONDITIONALLY here (row 0 when the next task is not an inverse one), so that the previous
            // row is dead throughout this branch -- carried through the forward transform it would be spilled every task
            t = cur.next(set, role);
            prefetch_task(role, lane);
            continue;
        }
        // ---- filter task `role` of the block in ring slot `slot`
        const int tdsc = desc_of(role);
        const int f = tdsc >> 2;
        if (set != seen_set) {                                            // this wave's first filter of the block
            wg_acquire_block(q, slot, gen, seen_b, seen_c);
            if constexpr (STREAM) seen_base = ((set - seen_c) / p.nblk) * p.TP;   // clip ordinal in this workgroup x T' (aligned dealing)
            seen_clip = lds_sums ? (set - seen_c) / p.nblk : 0;           // clip ordinal in this workgroup (whole clips per workgroup)
            seen_set = set;
        }
        WG_STAMP(3);                                                      // spectrum available
        const int b = seen_b, c = seen_c;
        const int n_c = c * LS;
        const int Lv = min(LS, p.T - n_c);
        int mlo = n_c + PADL - SK + 1;                                    // first frame whose window reaches the block
        mlo = mlo <= 0 ? 0 : (mlo + SHOP - 1) / SHOP;
        const int mhi = min(p.TP - 1, (n_c + Lv - 1 + PADL) / SHOP);
        if constexpr (BANDK) {
            if (tdsc & 3) {
                // ---- band task: eight (four) narrow-band filters on 256- (512-) point transforms (leaf_band.hpp)
                int tn_b = 0, nset_b = 0, nrole_b = 0;
                auto mid = [&]() {
                    tn_b = cur.next(nset_b, nrole_b);
                    prefetch_task(nrole_b, lane);
                    return std::integral_constant<int, 32>{};             // 32 loads issued
                };
                auto stamp = [&](int tag) { (void)tag; WG_STAMP(tag); };
                // the block's share of frame m of filter `fid`: where the 2048-point task puts it
                auto bout = [&](int fid, int m, float v) {
                    const int first_block = max(0, m * SHOP - PADL) / LS;
                    if constexpr (STREAM)
                        __hip_atomic_fetch_add(&fr[(size_t)((seen_base + m) & (RING - 1)) * FPS + fid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else if (lds_sums)
                        __hip_atomic_fetch_add(&lsum[((size_t)seen_clip * p.F + fid) * p.TP + m], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else
                        p.part[(((size_t)b * p.F + fid) * p.nslot + (c - first_block)) * p.TP + m] = v;
                };
                if ((tdsc & 3) == 1)
                    band_task<16, SK, SHOP>(p, rq, A, bmem + (tdsc >> 2), bl + 4, twl, scr, scr_lds, q, slot, c, mlo, mhi, lane, mid, bout, stamp);
                else
                    band_task<32, SK, SHOP>(p, rq, A, bmem + (tdsc >> 2), bl + 4, twl, scr, scr_lds, q, slot, c, mlo, mhi, lane, mid, bout, stamp);
                if constexpr (STREAM) {                                   // as below: the block's last task sends its frames out
                    const int done = wg_count(&sq[set & 7], lane);
                    if (done + 1 == ((set >> 3) + 1) * NT) stream_finalize(set);
                }
                WG_STAMP(7);
                t = tn_b;
                set = nset_b;
                role = nrole_b;
                continue;
            }
        }
        // Z = conj(A' R_f): rows 0..15 straight from the ring, rows 16..31 mirrored (A'[N - e] = conj(A'[e]))
        // (8-row chunks, fenced: all 32 ring reads in flight at once would need 64 registers next to rq and Z)
        float zre[32], zim[32];
        {
            // two streams of 16 rows: ascending from A[lane], and the mirror A[2048 - 64 k - lane], k = 16..31, read as
            // rows 15..0 of the base A[1088 - lane] (= k = 31 first); lds_stream32 walks 2 x 16 rows
            const unsigned a_lo = lds_addr(A + lane), a_hi = lds_addr(A + (kFftN - 64 * 31) - lane);
            v2f lo[16], hi[16];
            auto rd = [&](auto kk) {
                constexpr int k = decltype(kk)::value;
                if constexpr (k < 16) lds_rd8<512 * k>(lo[k], a_lo);
                else lds_rd8<512 * (31 - k)>(hi[k - 16], a_hi);
            };
            (void)rd;
            // chunk 0: rows 0..7, chunk 1: rows 8..15, chunk 2: rows 16..23, chunk 3: rows 24..31
#define LEAF_RD8(B) rd(std::integral_constant<int, B + 0>{}); rd(std::integral_constant<int, B + 1>{}); \
                    rd(std::integral_constant<int, B + 2>{}); rd(std::integral_constant<int, B + 3>{}); \
                    rd(std::integral_constant<int, B + 4>{}); rd(std::integral_constant<int, B + 5>{}); \
                    rd(std::integral_constant<int, B + 6>{}); rd(std::integral_constant<int, B + 7>{});
            v2f(&lo0)[8] = *reinterpret_cast<v2f(*)[8]>(&lo[0]);
            v2f(&lo1)[8] = *reinterpret_cast<v2f(*)[8]>(&lo[8]);
            v2f(&hi0)[8] = *reinterpret_cast<v2f(*)[8]>(&hi[0]);
            v2f(&hi1)[8] = *reinterpret_cast<v2f(*)[8]>(&hi[8]);
            // the spectral multiply fused with the first decimation-in-time stage of the transform (pairs of rows (k, k + 16),
            // unit twiddles): with za = conj(A'[k]) R[k] and zb = the mirrored row's product,
            //     out[k] = za + zb,  out[k + 16] = za - zb   as one product and two FMAs per component -- 6 instructions per pair
            // instead of 4 products + 4 additions.  Mirrored rows are read as rows 15..0 of a_hi: row k + 16 is hi[k].
            auto pair = [&](int k) {
                const float ra = rq[k], rb = rq[k + 16];
                const float tr_ = lo[k].x * ra, ti_ = -(lo[k].y * ra);
                zre[k] = fmaf(hi[k].x, rb, tr_);
                zim[k] = fmaf(hi[k].y, rb, ti_);
                zre[k + 16] = fmaf(-hi[k].x, rb, tr_);
                zim[k + 16] = fmaf(-hi[k].y, rb, ti_);
            };
            LEAF_RD8(0) LEAF_RD8(16) LEAF_RD8(8)
            lds_wait8<8>(lo0);
            lds_wait8<8>(hi0);
#pragma unroll
            for (int k = 0; k < 8; ++k) pair(k);
            LEAF_RD8(24)
            lds_wait8<0>(lo1);
            lds_wait8<0>(hi1);
#pragma unroll
            for (int k = 8; k < 16; ++k) pair(k);
#undef LEAF_RD8
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::"v"(zre[31]), "v"(zim[31]) : "memory");
        wg_reader_done(q, slot, lane);
        WG_STAMP(4);                                                      // spectral multiply done
        fft2048w<HALF, true>(zre, zim, scr, scr_lds, twl, twh, lane);   // register i <-> samples 64 brev5(i) + lane
        WG_STAMP(5);                                                      // inverse transform done
        // the filter's pooling weights, NJ vectors (see wg_pool_nj): requested now, consumed after the energies
        constexpr int PG = wg_pool_step(SHOP), PJ0 = wg_pool_jmin(SK, SHOP), NJ = wg_pool_nj(SK, SHOP);
        float pw[NJ];
        {
            const float* gsrc = p.Gz + (size_t)f * p.GZ + (kGPad + PJ0) + lane;
            asm volatile("" ::: "memory");
#pragma unroll
            for (int k = 0; k < NJ; ++k) pw[k] = gsrc[PG * k];
            asm volatile("" ::: "memory");
        }
        float er[NROW];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int r = brev5(i);
            if (r < NROW) er[r] = zre[i] * zre[i] + zim[i] * zim[i];
        }
        if (Lv < LS) {                                                    // a clip's last block: outputs past the clip's end
#pragma unroll
            for (int r = 0; r < NROW; ++r) er[r] = 64 * r + lane < Lv ? er[r] : 0.0f;
        }
        // next task: reserved now so that its filter's spectrum row streams in under the pooling
        int nset_i = 0, nrole = 0;
        const int tn = cur.next(nset_i, nrole);
        asm volatile("" ::"v"(er[0]), "v"(er[NROW - 1]));
        prefetch_task(nrole, lane);                                      // (row 0 as a dummy when there is no next filter)
        asm volatile("s_waitcnt vmcnt(32)" ::: "memory");                 // the pooling weights (issued before the 32 loads) have landed
        WG_STAMP(6);                                                      // energies, next task reserved, pooling row landed
        float acc[NGRP][16];
#pragma unroll
        for (int g = 0; g < NGRP; ++g)
#pragma unroll
            for (int fi = 0; fi < 16; ++fi) acc[g][fi] = 0.0f;
#pragma unroll
        for (int r = 0; r < NROW; ++r) {
#pragma unroll
            for (int fi = 0; fi < NFR; ++fi) {
                const int is = (DMIN + fi) * SHOP - PADL;
                if (is <= 64 * r + 63 && is + SK > 64 * r) {
                    static_assert((PADL - PJ0) % PG == 0, "window offsets are congruent to padL modulo gcd(64, hop)");
                    acc[fi / 16][fi % 16] = fmaf(er[r], pw[(64 * r - is - PJ0) / PG], acc[fi / 16][fi % 16]);
                }
            }
        }
        asm volatile("" : "+v"(acc[0][0]));
#pragma unroll
        for (int g = 0; g < NGRP; ++g) {
            const float v = frame_butterfly16(acc[g], lane);
            const int fi = 16 * g + ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
            const int m = n_c / SHOP + DMIN + fi;
            if ((lane & 3) == 0 && fi < NFR && m >= mlo && m <= mhi) {
                const int first_block = max(0, m * SHOP - PADL) / LS;
                if constexpr (STREAM)
                    __hip_atomic_fetch_add(&fr[(size_t)((seen_base + m) & (RING - 1)) * FPS + f], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else if (lds_sums)
                    __hip_atomic_fetch_add(&lsum[((size_t)seen_clip * p.F + f) * p.TP + m], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    p.part[(((size_t)b * p.F + f) * p.nslot + (c - first_block)) * p.TP + m] = v;
            }
        }
        if constexpr (STREAM) {
            // This filter's frame sums are in the ring (LDS operations of a wave execute in order, so the count below lands
            // after them); the count's return value says whether this was the block's last filter, and if so the block's
            // frames go out NOW, before this wave can block on anything else.  (Looking at the count a task later saves the LDS
            // round trip per task, but a pending finalize on a wave that then waits for a spectrum whose forward task waits
            // for that very finalize is a deadlock -- it happened at F = 3, where a wave's next task is several blocks ahead.)
            const int done = wg_count(&sq[set & 7], lane);
            if (done + 1 == ((set >> 3) + 1) * NT) stream_finalize(set);
        }
        WG_STAMP(7);                                                      // pooling, reduction and stores issued
        t = tn;
        set = nset_i;
        role = nrole;
    }
    WG_STAMP_NOW(59, 17);                                                 // this wave's last task is done
    // ---- clip-resident finalize: every partial sum of a clip this workgroup owns outright was written by its own waves.
    // Release (the stores have reached L2) - barrier - then every wave finalizes the rows dealt to it in its own scratch
    // (wg_tail_rows: bias, floor, EMA, PCEN; the partial sums are read past the vector cache); no barrier behind this one.
    // Clips that straddle two workgroups are left to fft_finalize_kernel.
    if constexpr (!STREAM) {
        if (p.fin_fused) {
            const int b_lo = (first_gb + p.nblk - 1) / p.nblk, b_hi = (first_gb + nset) / p.nblk;
            static_assert(SCRF >= wg_tail_floats(TAILC), "a wave's transposition scratch holds its rows of a chunk");
            FinParams fin = p.fin;
            if (lds_sums) {
                fin.lds_sums = lsum;
                fin.lds_row0 = b_lo * p.F;
                fin.lds_coef = lcoef;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();                                              // every task is done: the scratch is free
            WG_STAMP_NOW(60, 18);
            wg_tail_rows<NW, TAILC>(fin, b_lo, b_hi, scr, wave, lane0);
            WG_STAMP_NOW(61, 19);
            WG_STAMP_AT(63, 21, __builtin_amdgcn_s_memrealtime());
        }
    }
}

template <int SK, int SHOP, int NW, bool STREAM = false>
__global__ __launch_bounds__(NW * 64, (NW + 3) / 4) void leaf_fft_wg_kernel(const FftParams p) {
    leaf_fft_wg_body<SK, SHOP, NW, STREAM, STREAM ? kWgXAny : kWgXF32, STREAM ? 0 : 128>(p);
}
// the other tail-finalize instances.  XK: kWgXF32 / kWgX16 / kWgXMix / kWgXMix16; TAILC: 128 (T' <= 128) or 64 (longer rows)
template <int SK, int SHOP, int NW, int XK, int TAILC>
__global__ __launch_bounds__(NW * 64, (NW + 3) / 4) void leaf_fft_wg_kernel_var(const FftParams p) {
    static_assert(XK != kWgXAny && (XK != kWgXF32 || TAILC != 128) && (TAILC == 64 || TAILC == 128), "that pair is leaf_fft_wg_kernel");
    leaf_fft_wg_body<SK, SHOP, NW, false, XK, TAILC>(p);
}
// The instance ladder of the translation units (inst_fft_wg*.hip): the tail-finalize kernel of sample kind XK for a geometry and a
// tail tile, nullptr where there is none.  NWX: a further workgroup size for 401/160, 801/320, 201/80 (tools builds), 0 = none.
template <int SK, int SHOP, int NW, int XK, int TAILC>
constexpr FftKernel wg_tail_kernel() {
    if constexpr (XK == kWgXF32 && TAILC == 128) return leaf_fft_wg_kernel<SK, SHOP, NW, false>;
    else return leaf_fft_wg_kernel_var<SK, SHOP, NW, XK, TAILC>;
}
template <int XK, int TAILC>
inline FftKernel wg_tail_instance_of(int sk, int nw) {
    if (sk == 401 && nw == 12) return wg_tail_kernel<401, 160, 12, XK, TAILC>();
    if (sk == 801 && nw == 10) return wg_tail_kernel<801, 320, 10, XK, TAILC>();
    if (sk == 201 && nw == 12) return wg_tail_kernel<201, 80, 12, XK, TAILC>();
    return nullptr;
}
template <int XK>
inline FftKernel wg_tail_instance(int sk, int nw, int tailc) {
    return tailc == 128 ? wg_tail_instance_of<XK, 128>(sk, nw) : tailc == 64 ? wg_tail_instance_of<XK, 64>(sk, nw) : nullptr;
}

}  // namespace
