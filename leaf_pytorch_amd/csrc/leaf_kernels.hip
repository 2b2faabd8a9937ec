// leaf_kernels.hip -- MI355X (gfx950 / CDNA4) kernels for the LEAF frontend forward path, and the
// C ABI declared in include/leaf_hip.h.  Written for gfx950 only: 64-lane wavefronts, fp32 MFMA
// (v_mfma_f32_16x16x4_f32), 160 KiB LDS per CU.  No torch types anywhere in this file.
//
// One of the translation units of libleaf_hip.so: the C ABI, the host logic and every plain (non-template) kernel -- the headers
// this unit alone includes (leaf_kernels_*.hpp, leaf_staged.hpp, leaf_stage_backward.hpp).  The big kernel templates are
// instantiated in the inst_*.hip units and reached through the typed getters of leaf_inst.hpp; what a launch passes is defined
// once, in leaf_params.hpp.  Every other header is safe in any unit: templates, device functions, constexpr sizes.
//
// Reference arithmetic being replaced (file:line under the reference repository):
//   leaf_pytorch/frontend.py:78-89        Leaf.forward
//   leaf_pytorch/convolution.py:15-22     GaborConstraint            -> constrain() below
//   leaf_pytorch/impulse_responses.py:5-16,66-71  Gabor taps         -> gabor_tap()
//   leaf_pytorch/convolution.py:71-99     GaborConv1d.forward        -> fused kernel / conv_staged
//   leaf_pytorch/frontend.py:15-19        SquaredModulus             -> fused kernel / sqmod
//   leaf_pytorch/impulse_responses.py:74-80 + pooling.py:31-42       -> fused kernel / pool_staged
//   leaf_pytorch/postprocessing.py:13-28,62-69  EMA + PCEN           -> finalize kernel
//
// Design (the derivations and the measured ladders of rounds 1-3 are in NOTES.md).  Three interchangeable formulations of the same arithmetic, chosen
// per call (LEAF_ALGO_AUTO):
//   * leaf_fft*.hpp -- overlap-save FFT (default for windows from 224 taps): a wave-level 2048-point FFT (32 x 64
//     four-step: register butterflies, LDS transposition, a swap-free half-wave step), the block's spectrum shared by the
//     filters; per filter a spectral multiply (real spectrum; an even window's unpaired tap in the time domain), one
//     inverse transform, |.|^2 and the Gaussian pooling to per-frame partial sums; a row kernel sums the partials, floors
//     at 1e-5 and runs the EMA/PCEN scan.  With a backward epilogue the same structure is the backward (tap gradient = two
//     spectral dot products per block and filter; dL/dx = one more transform per block).
//       leaf_fft.hpp              one wave per block (small batches; round 1's kernel)
//       leaf_fft_wg.hpp / _bwd    one workgroup per block, spectrum ring in LDS, task queue: static LEAF geometries
//       leaf_fft_wg4k.hpp         4096-sample blocks for K = 801 / hop 320 (two half transforms per filter)
//       leaf_fft_wgg.hpp / _bwd   the same with window, hop and block length at run time (64..1216 taps, odd or even)
//       leaf_fft_wgg4k.hpp / _bwd 4096-sample blocks with run-time geometry (odd windows 833..2049)
//   * leaf_fused.hpp -- direct form on the fp32 MFMA (short windows, and the backward for even / short windows):
//     the Gabor taps are Hermitian in t (Re even, Im odd), so with s_k[n] = x[n+k] + x[n-k] and
//     d_k[n] = x[n+k] - x[n-k] the complex filterbank is two real GEMMs with HALF the K extent,
//         Re y[n,f] = sum_k s_k[n] * hr_f[k],   Im y[n,f] = sum_k d_k[n] * hi_f[k],  k = 0..K/2,
//     exact fp32 fmaf chains at the fp32 vector rate with operands delivered from LDS; one wave owns one hop-block,
//     squares its accumulator tiles, applies the pooling weights and reduces to per-frame partial sums.
//   * leaf_staged.hpp -- one kernel per reference module, every intermediate materialised: the sub-modules' own
//     forwards, the on-device cross-check of the fused kernels, and the fallback for geometries nothing else covers.
//   In the fused paths the 80x-inflated (B,2F,T) tensor of the reference never exists.
#include <atomic>
#include <random>
#include <cstdlib>
#include "leaf_common.hpp"
#include "leaf_staged.hpp"
#include "leaf_fused.hpp"
#include "leaf_backward.hpp"
#include "leaf_stage_backward.hpp"
#include "leaf_fft.hpp"
#include "leaf_fft_wg.hpp"
#include "leaf_fft_small.hpp"
#include "leaf_fft_stream.hpp"
#include "leaf_fft_wg_bwd.hpp"
#include "leaf_fft_wg4k.hpp"
#include "leaf_fft_wgg.hpp"
#include "leaf_fft_wgg_bwd.hpp"
#include "leaf_fft_wgg4k.hpp"
#include "leaf_fft_wgg4k_bwd.hpp"
#include "leaf_inst.hpp"            // the big kernel templates are instantiated in the inst_*.hip units: typed handles
// the plain kernels, compiled in this unit alone
#include "leaf_kernels_tables.hpp"
#include "leaf_kernels_rows.hpp"
#include "leaf_kernels_misc.hpp"
#include "leaf_kernels_backward.hpp"
namespace {

// Tools-only environment switches (A/B measurements of tools/*.py): compiled in only with -DLEAF_TOOLS=1
// (LEAF_HIPCC_EXTRA="-DLEAF_TOOLS=1"); the product library reads no environment variable except LEAF_NO_4K.
inline const char* tools_env(const char* name) { return LEAF_TOOLS ? getenv(name) : nullptr; }

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Waveform mixup of a call (leaf_forward_mix_f32 / leaf_backward_mix_f32), set only where a kernel family that mixes in its
// loads serves the call (the other families get a mixed copy, mixup_kernel); lam == NULL: off
struct MixArgs { const int* perm; const float* lam; };
// The per-call options of one ABI call: built once at the entry point (forward_ctx / backward_ctx) and passed down by const
// reference, so that every decision names what it depends on.  Nothing is kept between calls: the library stays re-entrant.
struct CallCtx {
    int cus;                 // CUs this call may fill: the device's count minus LEAF_ALGO_RESERVE_CUS(k), at least one
    bool stream_finalize;    // LEAF_ALGO_STREAM_FINALIZE
    bool band_off;           // LEAF_ALGO_FULL_TRANSFORMS / LEAF_FLAG_BWD_FULL_TRANSFORMS
    bool band_strict;        // LEAF_ALGO_STRICT_BAND_CLASSES / LEAF_FLAG_BWD_STRICT_BAND_CLASSES
    bool no_table_cache;     // LEAF_ALGO_NO_TABLE_CACHE: leaf_forward_cached_f32 runs as leaf_forward_f32
    int desync;              // LEAF_ALGO_TUNE_DESYNC(n); -1 = automatic
    int sel;                 // the selector (low byte of `algo`); resolve_selector() turns LEAF_ALGO_AUTO into what runs
    MixArgs mix;
};
// the host-only bundles of what every internal function of a full forward / backward repeats (nothing to do with the kernels'
// parameter structs, whose layouts are hashed): the shape, and with it the seven parameter pointers and the stream
struct Shape { int B, T, F, K, hop; };
struct LeafArgs {
    Shape s;
    const float *kernel, *pool_w, *pool_b, *alpha, *delta, *root, *ema_w;
    hipStream_t st;
};
// CU count of the CURRENT device (cached per device ordinal; plans are sized for the device the call runs on)
int device_cus() {
    constexpr int kMaxDev = 64;
    static std::atomic<int> cached[kMaxDev];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < kMaxDev) {
        n = cached[dev].load(std::memory_order_relaxed);
        if (n > 0) return n;
    }
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    if (dev >= 0 && dev < kMaxDev) cached[dev].store(n, std::memory_order_relaxed);
    return n;
}
// the one place that unpacks the forward's `algo` word
CallCtx forward_ctx(int algo) {
    CallCtx c{};
    c.cus = std::max(1, device_cus() - ((algo >> 16) & 0xff));           // LEAF_ALGO_RESERVE_CUS(k): grids of this call leave k CUs free
    c.stream_finalize = (algo & LEAF_ALGO_STREAM_FINALIZE) != 0;
    c.band_off = (algo & LEAF_ALGO_FULL_TRANSFORMS) != 0;
    c.band_strict = (algo & LEAF_ALGO_STRICT_BAND_CLASSES) != 0;
    c.no_table_cache = (algo & LEAF_ALGO_NO_TABLE_CACHE) != 0;
    c.desync = ((algo >> 8) & 0xff) - 1;
    c.sel = algo & 0xff;
    return c;
}
// ... and the backward's, whose options travel in `flags` (no reservation, no selector: bwd_path() decides)
CallCtx backward_ctx(int flags, MixArgs mix) {
    CallCtx c{};
    c.cus = device_cus();
    c.band_off = (flags & LEAF_FLAG_BWD_FULL_TRANSFORMS) != 0;
    c.band_strict = (flags & LEAF_FLAG_BWD_STRICT_BAND_CLASSES) != 0;
    c.desync = -1;
    c.sel = LEAF_ALGO_AUTO;
    c.mix = mix;
    return c;
}
// Tools-only switch LEAF_WG_GENERIC=1: the static geometries through the run-time-geometry workgroup kernel (A/B measurements)
inline bool wg_force_generic() {
    static const bool on = [] { const char* e = tools_env("LEAF_WG_GENERIC"); return e && atoi(e) != 0; }();
    return on;
}

struct FusedPlan {
    bool ok;
    int FP, ntiles, KS, R, Hf, xshift, NBH, NU, HP, XS, q_lo, q_hi, nq, noff, noff_t, padL, TP;
    int rt_main, groups_main, rt_rem;
    int GJ;
    size_t w_floats, g_floats, part_floats, meta_ints;
};

// +4 tap rows and +16 window floats per wave: the k-loop prefetches one step past its last k-step
inline size_t fused_lds_bytes(int R, int rt, int XS) {
    return ((size_t)(R + 4) * 32 * rt + (size_t)kWavesPerWG * (XS + 16)) * 4;
}

FusedPlan make_plan(const Shape& s, int cus) {
    const auto [B, T, F, K, hop] = s;
    FusedPlan pl{};
    pl.padL = K / 2 + K % 2 - 1;
    pl.TP = (T + (K - 1) - K) / hop + 1;
    pl.FP = 16 * ceil_div(F, 16);
    pl.ntiles = pl.FP / 16;
    pl.KS = ceil_div(K / 2 + 1, 4);
    pl.R = 4 * pl.KS;
    pl.Hf = (K - 1) / 2;
    pl.xshift = K / 2 - pl.padL;
    pl.NBH = ceil_div(hop, 16);
    pl.NU = ceil_div(pl.NBH, kUB);
    pl.HP = 4 * pl.KS;
    pl.XS = 16 * kUB * pl.NU + 2 * pl.HP;
    pl.q_lo = pl.padL / hop;
    pl.q_hi = (T - 1 + pl.padL) / hop;
    pl.nq = pl.q_hi - pl.q_lo + 1;
    pl.noff = (K - 1) / hop + 1;
    pl.noff_t = pl.noff <= 1 ? 1 : (pl.noff <= 3 ? 3 : (pl.noff <= 6 ? 6 : 0));
    pl.w_floats = (size_t)pl.R * 2 * pl.FP;
    pl.GJ = ((std::max(pl.noff_t, 1) - 1) * hop + 16 * kUB * pl.NU + 3) / 4 * 4;
    pl.g_floats = (size_t)pl.FP * pl.GJ;
    pl.part_floats = (size_t)B * pl.TP * pl.noff * pl.FP;
    pl.meta_ints = (size_t)2 * pl.FP + pl.ntiles;          // perm[FP], col_of[FP], tile_ks[ntiles]
    pl.rt_main = 0;
    // Widest register tile whose taps fit LDS -- unless the batch is so small that (tasks x filter groups) would not
    // even give every wave slot of the chip one task: then narrower tiles (more filter groups, shorter per-wave
    // dependency chains) cut the latency of a small forward.
    const long long wave_slots = (long long)cus * kWavesPerWG;
    // NOFF = 6 instances (4..6 overlapping frames per hop-block): the widest register tiles spill (720 B/lane at RT = 3,
    // 188 B at RT = 2, -Rpass-analysis=kernel-resource-usage), so the tile is capped where it stays in registers;
    // LEAF_FUSED_RT_CAP (environment, tools only) overrides the cap for measurements.
    static const int rt_cap_env = [] { const char* e = tools_env("LEAF_FUSED_RT_CAP"); return e ? atoi(e) : 0; }();
    const int rt_cap = rt_cap_env > 0 ? rt_cap_env : (pl.noff_t == 6 ? 1 : 3);
    for (int rt = 3; rt >= 1; --rt) {
        if (rt > rt_cap && rt > 1) continue;
        if (rt > pl.ntiles || fused_lds_bytes(pl.R, rt, pl.XS) > (size_t)kMaxLds) continue;
        if (pl.rt_main == 0) pl.rt_main = rt;
        if ((long long)B * pl.nq * ceil_div(pl.ntiles, rt) >= wave_slots) break;
        pl.rt_main = rt;
    }
    pl.ok = pl.rt_main > 0 && pl.noff_t > 0 && pl.FP <= kMaxFP && (long long)B * pl.nq < (1ll << 30) &&
            (double)pl.part_floats < 2.0e9;
    if (pl.ok) {
        pl.groups_main = pl.ntiles / pl.rt_main;
        pl.rt_rem = pl.ntiles % pl.rt_main;
    }
    return pl;
}

hipError_t launch_fused(const FusedParams& prm, int rt, int noff_t, int groups, size_t lds, int grid_x, hipStream_t st) {
    const FusedKernel kfn = leaf_inst_fused(rt, noff_t, (prm.K % 2) == 0, prm.dY != nullptr);
    if (!kfn) return hipErrorInvalidValue;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kfn, dim3(grid_x, groups), dim3(kWavesPerWG * 64), lds, st, prm);
    return hipGetLastError();
}

struct BwdPlan {
    bool ok;
    int NKT, NW, TPW, NS, HPc, XSC, LD, nch;
    size_t lds;
};

BwdPlan make_bwd_plan(const FusedPlan& pl, int T) {
    BwdPlan bp{};
    if (!pl.ok) return bp;
    bp.NKT = ceil_div(pl.R, 16);
    bp.NW = 16;                                        // 4 waves per SIMD; k-tiles are dealt to them SIMD-balanced in-kernel
    bp.TPW = ceil_div(bp.NKT, bp.NW);
    bp.HPc = 16 * bp.NKT;
    bp.LD = 2 * pl.FP + 16;
    bp.NS = 0;
    for (int ns = 64; ns >= 16; ns >>= 1)
        if (ns * (2 * pl.FP) / 4 <= kDtPF * bp.NW * 64) { bp.NS = ns; break; }
    if (bp.NS == 0 || bp.TPW > 3) return bp;
    bp.XSC = bp.NS + 2 * bp.HPc;
    if (bp.XSC > 2 * bp.NW * 64) return bp;
    bp.lds = (size_t)2 * ((bp.XSC + 3) / 4 * 4 + (size_t)bp.NS * bp.LD) * 4;
    if (bp.lds > (size_t)kMaxLds) return bp;
    bp.nch = ceil_div(T, bp.NS);
    bp.ok = true;
    return bp;
}

hipError_t launch_dtaps(const DtapsParams& prm, int rt, int tpw, int groups, size_t lds, int grid_x, hipStream_t st) {
    const DtapsKernel kfn = leaf_inst_dtaps(rt, tpw, (prm.K % 2) == 0);
    if (!kfn) return hipErrorInvalidValue;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kfn, dim3(grid_x, groups), dim3(prm.NW * 64), lds, st, prm);
    return hipGetLastError();
}

// the fused kernel over all filter groups: full groups of rt_main tiles, then the remainder group
hipError_t launch_fused_groups(FusedParams prm, const FusedPlan& pl, int cus, hipStream_t st) {
    const int wg_needed = ceil_div(prm.total_tasks, kWavesPerWG);
    if (pl.groups_main > 0) {
        prm.tile_base = 0;
        const int gx = std::max(1, std::min(wg_needed, std::max(1, cus / pl.groups_main)));
        hipError_t e = launch_fused(prm, pl.rt_main, pl.noff_t, pl.groups_main, fused_lds_bytes(pl.R, pl.rt_main, pl.XS), gx, st);
        if (e != hipSuccess) return e;
    }
    if (pl.rt_rem > 0) {
        prm.tile_base = pl.groups_main * pl.rt_main;
        const int gx = std::max(1, std::min(wg_needed, cus));
        hipError_t e = launch_fused(prm, pl.rt_rem, pl.noff_t, 1, fused_lds_bytes(pl.R, pl.rt_rem, pl.XS), gx, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

FusedParams base_fused_params(const FusedPlan& pl, const Shape& s, int tuning_desync) {
    const auto [B, T, F, K, hop] = s;
    FusedParams prm{};
    prm.B = B; prm.T = T; prm.TP = pl.TP; prm.F = F; prm.FP = pl.FP; prm.K = K; prm.hop = hop; prm.padL = pl.padL;
    prm.KS = pl.KS; prm.Hf = pl.Hf; prm.xshift = pl.xshift; prm.NU = pl.NU; prm.HP = pl.HP; prm.XS = pl.XS;
    prm.q_lo = pl.q_lo; prm.nq = pl.nq; prm.noff = pl.noff; prm.total_tasks = B * pl.nq; prm.GJ = pl.GJ;
    // half a unit of MFMA work is ~ 16*kUB samples x 2*RT tiles x KS k-steps x 32 cycles; s_sleep(127) ~ 8.1k cycles
    prm.desync_sleeps = tuning_desync >= 0 ? tuning_desync
                                           : std::max(1, (int)((long long)kUB * 2 * pl.rt_main * pl.KS * 32 / 2 / 8128));
    return prm;
}

// workspace layout of the fused backward (floats)
struct BwdLayout {
    size_t W, G, Gs, meta, part, raw, ema, gpre, gcols, rowsum, dwpart, dHpart, dY, total;
};

BwdLayout bwd_layout(const FusedPlan& pl, const BwdPlan& bp, int B, int T, int F, int cus) {
    BwdLayout L{};
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += align_up(n, 64); return at; };
    L.W = take(pl.w_floats);
    L.G = take(pl.g_floats);
    L.Gs = take(pl.g_floats);
    L.meta = take(pl.meta_ints);
    L.part = take(pl.part_floats);
    L.raw = take((size_t)B * F * pl.TP);
    L.ema = take((size_t)B * F * pl.TP);
    L.gpre = take((size_t)B * F * pl.TP);
    L.gcols = take((size_t)B * pl.TP * pl.FP);
    L.rowsum = take((size_t)B * F * 4);
    L.dwpart = take((size_t)cus * kWavesPerWG * pl.FP);
    L.dHpart = take((size_t)(cus + 1) * 16 * bp.NKT * 2 * pl.FP);     // + 1 slab for the reduced sum
    L.dY = take((size_t)B * T * 2 * pl.FP);
    L.total = o;
    return L;
}

// ---- FFT (overlap-save) forward plan
struct FftPlan {
    bool ok;
    int L, nblk, NT, GZ, g_bufs, fq, nfq, TP, padL, scr_floats, nslot;
    size_t lds, h_floats, gz_floats, part_floats;
    size_t band_stat, band_dyn;   // tables of the band-limited filter tasks (leaf_band.hpp), 0 where they do not apply
};
// ---- band-limited filter tasks: table layout (float offsets).  The per-filter records and the decimated pooling windows depend
// on the parameters only and sit behind the overlap-save tables (also in the frozen-parameter tables of
// leaf_fft_prepare_tables_f32); the edge tables and the edge list depend on the clip length as well and follow them in a
// forward call's workspace (leaf_forward_prepared_f32: behind the partial sums).
constexpr int kMaxCusForSpec0 = 512;                     // workgroups whose first-block spectrum the table launch computes (>= #CUs)
struct BandLayout {
    size_t rec, gz, stat;          // parameter-only part
    size_t edge, elist, spec0, dyn;   // per-call part (offsets from its own base); spec0: the workgroups' first-block spectra
};
inline BandLayout band_layout(int F, int K, int hop) {
    BandLayout bl{};
    if (!band_geometry_ok(K, hop) || F > kBandMaxFilters) return bl;
    size_t o = 0;
    bl.rec = o; o += align_up((size_t)4 * F, 64);
    bl.gz = o; o += align_up((size_t)F * band_gz_floats(K, hop), 64);
    bl.stat = o;
    o = 0;
    bl.edge = o; o += align_up((size_t)F * 2 * kBandMaxEdge * 512, 64);
    bl.elist = o; o += align_up((size_t)4 * kBandMaxEdge, 64);
    bl.spec0 = o; o += align_up((size_t)kMaxCusForSpec0 * kWgRingFwdFloat2 * 2, 64);
    bl.dyn = o;
    return bl;
}
// Frames reg_lo .. reg_hi take the shift-invariant decimated window (its tails stay inside the clip); every other frame is an
// edge frame with one table per block its (cut) window meets.  false: more edge entries than the tables hold (tiny clips).
inline bool band_edges(int T, int K, int hop, int L, int padL, BandParams& bp, BandEdge (&e)[kBandMaxEdge]) {
    const int TP = (T - 1) / hop + 1, lphi = band_lphi(16);
    int lo = ceil_div(padL + lphi, hop), hi = (T - K - lphi + padL) >= 0 ? (T - K - lphi + padL) / hop : -1;
    hi = std::min(hi, TP - 1);
    if (hi < lo) { lo = TP; hi = TP - 1; }                  // every frame is an edge frame
    bp.reg_lo = lo;
    bp.reg_hi = hi;
    int n = 0;
    for (int m = 0; m < TP; ++m) {
        if (m >= lo && m <= hi) continue;
        const int ws = m * hop - padL;
        for (int c = std::max(0, ws) / L; c * L < std::min(T, ws + K); ++c) {
            const int a = std::max({c * L, 0, ws}), b = std::min({(c + 1) * L, T, ws + K});
            if (a >= b) continue;
            if (n == kBandMaxEdge) return false;
            e[n++] = BandEdge{c, m, a, b};
        }
    }
    bp.n_edge = n;
    return true;
}

FftPlan make_fft_plan(const Shape& s, int cus) {
    const auto [B, T, F, K, hop] = s;
    FftPlan fp{};
    if (K < 2 || K > 64 * kPoolRowsMax - 63) return fp;         // pooling rows per window <= kPoolRowsMax (K <= 1217)
    fp.padL = K / 2 + K % 2 - 1;
    fp.TP = (T - 1) / hop + 1;
    fp.L = fft_block_len(K, hop, fft_static_geometry(K, hop));
    fp.nblk = ceil_div(T, fp.L);
    fp.NT = ceil_div(K + 63, 64);
    fp.GZ = (kGPad + K + 256 + 3) / 4 * 4;                   // pooling reads run up to 3 rows + 63 lanes past the window
    // filters per task: as many as keeps one wave slot per SIMD pair busy everywhere -- fewer filters per task means the
    // block's forward transform is repeated more often, which only matters once the chip is full
    fp.fq = (int)std::min<long long>(kFftFQ, std::max<long long>(1, (long long)B * fp.nblk * F / ((long long)cus * kFftWaves)));
    fp.nfq = ceil_div(F, fp.fq);
    fp.scr_floats = 32 * 65;                                 // transposes only: the energies stay in registers
    const size_t scr = (size_t)fp.scr_floats;
    for (fp.g_bufs = 2; fp.g_bufs >= 1; --fp.g_bufs) {          // double-buffer the pooling row when LDS allows
        fp.lds = ((size_t)kTwFloats + kFftWaves * (scr + fp.g_bufs * (size_t)fp.GZ)) * 4;
        if (fp.lds <= (size_t)kMaxLds) break;
    }
    if (fp.g_bufs < 1) return fp;
    if ((long long)B * fp.nblk >= (1ll << 30) || F > 65535) return fp;
    fp.h_floats = (size_t)F * kFftN * 2;
    fp.gz_floats = (size_t)F * fp.GZ;
    fp.nslot = (K - 1 > fp.L) ? 3 : 2;                       // blocks a frame's window can meet
    if (K - 1 > 2 * fp.L) return fp;
    fp.part_floats = (size_t)B * fp.TP * fp.nslot * F;
    fp.band_stat = band_layout(F, K, hop).stat;
    fp.band_dyn = band_layout(F, K, hop).dyn;
    fp.ok = true;
    return fp;
}

// ---- 4096-sample plan (leaf_fft_wg4k.hpp): the 32 kHz LEAF geometry.  LEAF_ALGO_FFT_WG means THIS kernel for that geometry
// at every batch size (so that a clip is bit-identical across batch compositions); the frozen-parameter entry points
// (leaf_fft_prepare_tables_f32 / leaf_forward_prepared_f32) keep the 2048-sample tables and kernels.
struct Fft4kPlan {
    bool ok;
    bool generic;          // run-time-geometry kernel (leaf_fft_wgg4k.hpp); false: the static K = 801 / hop = 320 instance
    int L, nblk, nslot, TP, padL, RG, nw;
    size_t lds;
    size_t tab_floats, grow_floats, part_floats;
    size_t band_floats;    // tables of the band tasks (static instance only): records | decimated pooling windows | edge tables | edge list
};
// band tables of the 4096-sample plan (float offsets from their base)
struct Band4kLayout { size_t rec, gz, edge, elist, total; };
inline Band4kLayout band4k_layout(int F, int K, int hop) {
    Band4kLayout bl{};
    size_t o = 0;
    bl.rec = o; o += align_up((size_t)4 * F, 64);
    bl.gz = o; o += align_up((size_t)F * band4k_gz_floats(K, hop), 64);
    bl.edge = o; o += align_up((size_t)F * kBandMaxEdge * 512, 64);
    bl.elist = o; o += align_up((size_t)4 * kBandMaxEdge, 64);
    bl.total = o;
    return bl;
}
// LEAF_NO_4K=1 (environment, tools / tests only): keep every window on the 2048-sample plan
inline bool fft4k_disabled() {
    static const bool off = [] { const char* e = getenv("LEAF_NO_4K"); return e && atoi(e) != 0; }();
    return off;
}
FftKernel pick_fft_wgg4k_kernel(int K) { return leaf_inst_fft_wgg4k(fft_wgg4k_taps_per_lane(K)); }
Fft4kPlan make_fft4k_plan(const Shape& s) {
    const auto [B, T, F, K, hop] = s;
    Fft4kPlan fp{};
    if (fft4k_disabled()) return fp;
    fp.padL = K / 2 + K % 2 - 1;
    fp.TP = (T - 1) / hop + 1;
    if ((long long)B * ceil_div(T, 2048) >= (1ll << 30) || F > 65535) return fp;
    if (K == 801 && hop == 320) {
        fp.L = 3200;
        fp.RG = kWg4RowFloats;
        fp.nw = LEAF_4K_FWD_NW;
        fp.lds = fft_wg4k_lds_bytes(LEAF_4K_FWD_NW);
        if (F <= kBandMaxFilters) fp.band_floats = band4k_layout(F, K, hop).total;
    } else {
        // any other odd window from K = 833 (where the 2048-sample plan drops below half valid outputs) to 2049
        if (!(K & 1) || K < 833 || K > 2049) return fp;
        fp.generic = true;
        fp.L = (kFft4N - K + 1) & ~1;
        if ((fp.L + K - 2) / hop + 2 > kWgg4MaxFrames) return fp;       // frames a block meets: parked in LDS between the halves
        fp.RG = fft_wgg4k_row_floats(K);
        fp.nw = 12;
        const int fbn = fft_wgg4k_frame_floats(K, hop);
        while (fp.nw > 6 && fft_wgg4k_lds_bytes(fp.nw, K, fbn) > (size_t)kMaxLds) --fp.nw;
        fp.lds = fft_wgg4k_lds_bytes(fp.nw, K, fbn);
        if (fp.lds > (size_t)kMaxLds) return fp;
    }
    fp.nblk = ceil_div(T, fp.L);
    fp.nslot = 2;                                                        // K - 1 <= 2048 <= L: a window meets at most two blocks
    fp.tab_floats = (size_t)F * kFft4TabFloats;
    fp.grow_floats = (size_t)F * 2 * fp.RG + kFft4WtFloats;            // + the shared twiddle table w^e of the static kernel's odd half
    fp.part_floats = (size_t)B * fp.TP * fp.nslot * F;
    fp.ok = true;
    return fp;
}
size_t fft4k_workspace_floats(const Fft4kPlan& fp, int B) {
    return align_up(fp.tab_floats, 64) + align_up(fp.grow_floats, 64) + align_up(fp.part_floats, 64) + fp.band_floats + align_up((size_t)B, 64);
}
static_assert(fft_wg4k_bwd_dx_lds_bytes(kWg4BwdDxWaves) <= (size_t)kMaxLds, "LDS budget");
static_assert(fft_wg4k_lds_bytes(12) <= (size_t)kMaxLds && fft_wgg4k_lds_bytes(6, 2049, kWgg4MaxFrames) <= (size_t)kMaxLds, "LDS budget");

// ---- which instantiation of leaf_fft_kernel serves a geometry.  Odd K: real-spectrum kernels (the taps are Hermitian
// about the centre tap); even K: complex spectrum.  The backward instances exist for the real-spectrum form only.

// ---- workgroup-per-block variant (leaf_fft_wg.hpp): static odd-window geometries; worth it once every CU gets blocks
struct FftWgLaunch {
    FftKernel fn;
    int nw;
    size_t lds;
    bool fused_finalize = false;   // the kernel deals blocks contiguously and finalizes the clips it owns (FftParams::fin)
    FftKernel fn_stream = nullptr; // the STREAM variant (whole clips per workgroup: finalizes as the blocks complete), if any
    int sk = 0, shop = 0;          // its compile-time geometry (for the LDS size, which grows with F)
    bool lds_sums = false;         // the kernel can keep the per-frame sums of whole clips in LDS (fin_fused = 3)
};
// 12 waves (3 per SIMD, full transposition scratch) by default: with the swap-free cross stage the column-half transposition
// of the 16-wave form (twice the store instructions) costs more than the fourth wave per SIMD brings (cfg1 0.223 vs 0.227 ms,
// cfg3 0.4215 vs 0.428, cfg4 2.03 vs 2.05: tools/bench_configs.py, interleaved).  LEAF_WG_WAVES=16|12 (environment, tools
// only) overrides the choice for A/B measurements.
// Every instance holds ONE loader and one tile form of the tail (leaf_fft_wg.hpp): xk = the waveform's sample kind
// (wg_sample_kind), long_rows = T' > 128.
inline int wg_sample_kind(int xtype, const float* mix_lam) {
    return mix_lam ? (xtype == kSamplePcm16 ? kWgXMix16 : kWgXMix) : xtype ? kWgX16 : kWgXF32;
}
FftWgLaunch pick_fft_wg_kernel(int K, int hop, int xk, bool long_rows) {
    static const int forced = [] { const char* e = tools_env("LEAF_WG_WAVES"); return e ? atoi(e) : 0; }();
    const bool w16 = forced == 16 || forced == 14;
    int nw = 0;
#ifdef LEAF_WG_NW
    if (K == 401 && hop == 160) nw = LEAF_WG_NW;                          // A/B builds only
    else
#endif
    if (K == 401 && hop == 160) nw = w16 ? 16 : 12;
    else if (K == 801 && hop == 320) nw = w16 ? 14 : 10;               // 16 do not fit the LDS
    else if (K == 201 && hop == 80) nw = w16 ? 16 : 12;
    else return {nullptr, 0, 0};
    const int tailc = long_rows ? 64 : 128;
    const FftKernel fn = xk == kWgXMix ? leaf_inst_fft_wg_mix(K, nw, tailc) : xk == kWgXMix16 ? leaf_inst_fft_wg_mix16(K, nw, tailc)
                         : xk == kWgX16 ? leaf_inst_fft_wg_x16(K, nw, tailc) : leaf_inst_fft_wg(K, nw, tailc);
    const FftKernel fn_stream = leaf_inst_fft_wg_streamfin(K, nw);        // (the loader chosen at run time: one load site)
    return {fn, nw, fft_wg_lds_bytes(nw, K), true, fn_stream, K, hop, true};
}
// is there a static instance for the geometry (every sample kind and tail has one where one has)?  Not for launching.
inline bool fft_wg_static_exists(int K, int hop) { return pick_fft_wg_kernel(K, hop, kWgXF32, false).fn != nullptr; }
// Any other window the 2048-sample plan covers -- odd or even -- takes the run-time-geometry workgroup kernel
// (leaf_fft_wgg.hpp): one instantiation per bucket of taps-per-lane and window parity, as many waves (<= 12: three per
// SIMD's registers) as the LDS holds energy rows for.
FftWgLaunch pick_fft_wgg_kernel(const FftPlan& fp, int K, int hop) {
    (void)hop;
    if (!fp.ok || K < 64 || K > 64 * 19) return {nullptr, 0, 0};          // 19 taps per lane at most
    // the full transposition scratch (fewer LDS store instructions per transform) where the LDS holds it for at least
    // `full_min` = 11 waves (instantiated for the buckets up to 10 taps per lane: 11.025 kHz 0.227 -> 0.209 ms at 12 waves,
    // 22.05 / 24 kHz -1..2 % at 11); LEAF_WGG_FULL=0|12|11 (environment, tools only)
    static const int full_min = [] { const char* e = tools_env("LEAF_WGG_FULL"); return e ? atoi(e) : 11; }();
    const int ni = fft_wgg_taps_per_lane(K);
    if (full_min > 0 && ni <= 10) {
        int nwf = 12;
        while (nwf > full_min && fft_wgg_lds_bytes_full(nwf, K) > (size_t)kMaxLds) --nwf;
        if (fft_wgg_lds_bytes_full(nwf, K) <= (size_t)kMaxLds)
            return {leaf_inst_fft_wgg(ni, false), nwf, fft_wgg_lds_bytes_full(nwf, K), true};
    }
    int nw = 12;
    while (nw > 6 && fft_wgg_lds_bytes(nw, K) > (size_t)kMaxLds) --nw;
    const size_t lds = fft_wgg_lds_bytes(nw, K);
    if (lds > (size_t)kMaxLds) return {nullptr, 0, 0};
    return {leaf_inst_fft_wgg(ni, true), nw, lds, true};
}
static_assert(fft_wg_lds_bytes(12, 401) <= (size_t)kMaxLds && fft_wg_lds_bytes(10, 801) <= (size_t)kMaxLds &&
              fft_wg_lds_bytes(16, 401) <= (size_t)kMaxLds && fft_wg_lds_bytes(14, 801) <= (size_t)kMaxLds, "LDS budget");
// AUTO takes the workgroup variant when the batch gives every CU at least one block; below that the per-wave kernel
// (one task per wave, filters-per-task adapted to the batch) has the shorter critical path.
bool fft_wg_available(const FftPlan& fp, int K, int hop) {
    return fp.ok && (fft_wg_static_exists(K, hop) || pick_fft_wgg_kernel(fp, K, hop).fn != nullptr);
}
// Blocks from which the workgroup kernels beat the per-wave kernel: a little under half a block per CU (measured crossover,
// tools/sweep_batch_wg.py: 80 -> 160 blocks at 16 kHz, 60 -> 120 at 22.05 kHz, 80 -> 120 at 8 kHz, 68 -> 136 4096-sample
// blocks at 48 kHz; one block per workgroup costs the same 42 / 53 / 104 us from 1 to 256 blocks)
inline long long fft_wg_min_blocks(int cus) { return (long long)cus * 7 / 16; }
// the same question for the backward kernels, in sixteenths of a block per CU (measured, tools/sweep_batch_wg_bwd.py: the static
// kernel against the per-wave backward crosses between 320 and 480 blocks at 16 kHz, the run-time-geometry one between 120
// and 180 at 22.05 kHz, the 4096-sample one between 68 and 136 at 48 kHz); LEAF_WG_BWD_MIN_BLOCKS (environment, tools only)
// overrides it for the sweep
inline long long fft_wg_bwd_min_blocks(int cus, int sixteenths) {
    static const long long forced = [] { const char* e = tools_env("LEAF_WG_BWD_MIN_BLOCKS"); return e ? atoll(e) : -1ll; }();
    return forced >= 0 ? forced : (long long)cus * sixteenths / 16;
}
bool fft_wg_auto(const FftPlan& fp, int B, int K, int hop, int cus) {
    return fft_wg_available(fp, K, hop) && (long long)B * fp.nblk >= fft_wg_min_blocks(cus) &&
           (K >= 224 || fft_static_geometry(K, hop));
}
FftKernel pick_fft_kernel(const FftPlan& fp, int K, int hop, bool bwd) {
    const bool stat = fft_static_geometry(K, hop) && fp.g_bufs == 2;
    // odd and even windows alike: real-spectrum kernels (even K: Hermitian K - 1 taps + the unpaired tap in the time domain)
    if (stat && (K & 1)) return (leaf_inst_fft(K, 1, 1, bwd ? 1 : 0));
    return (leaf_inst_fft(0, fp.g_bufs == 2 ? 1 : 0, (K & 1) ? 1 : 2, bwd ? 1 : 0));
}

// the MIX instances (waveform mixup in the block load): the static odd windows only; nullptr elsewhere
FftKernel pick_fft_kernel_mix(const FftPlan& fp, int K, int hop, bool bwd) {
    const bool stat = fp.ok && fft_static_geometry(K, hop) && fp.g_bufs == 2;
    return stat && (K & 1) ? (leaf_inst_fft_mix(K, bwd ? 1 : 0)) : nullptr;
}

// Even K (real-spectrum form): the unpaired taps live behind the real spectra, in the second half of the float2 slab that
// the (retired) complex-spectrum layout sized: [F][2048] floats of spectra, then [F][2] floats.  Odd K: none.
float* fft_lone_taps(float* tables, int F, int K) { return (K & 1) ? nullptr : tables + (size_t)F * kFftN; }

// Floats of the parameter-derived tables of the FFT path: filter spectra, pooling rows, identity column map.
// (`band_dyn`: + the per-call tables of the band-limited filter tasks -- the workspace of a forward call has them, the
// frozen-parameter tables of leaf_fft_prepare_tables_f32 do not: the edge tables depend on the clip length)
size_t fft_table_floats(const FftPlan& fp, int F, bool band_dyn = true) {
    return align_up(fp.h_floats, 64) + align_up(fp.gz_floats, 64) + align_up((size_t)F, 64) + fp.band_stat + (band_dyn ? fp.band_dyn : 0);
}
// (+ B floats behind the partial sums: the per-clip scales of LEAF_FLAG_PEAKNORM)
size_t fft_workspace_floats(const FftPlan& fp, int F, int B) {
    return fft_table_floats(fp, F) + align_up(fp.part_floats, 64) + (LEAF_TRACE ? 16 * 64 * 2 : 0) + align_up((size_t)B, 64);
}

// ---- the self-validating table cache of leaf_forward_cached_f32 (stamps: leaf_fft.hpp).  One caller-owned buffer holds the tables of
// the 2048-sample plan as a forward call's workspace does -- [spectra | pooling rows | col_of | band records, G~ | edge tables | edge
// list] -- and, where the workspace has the first-block spectra, the stamps [roles][F][kStampWords]: roles = 2 + the edge entries of
// this clip length where the geometry has band tasks, else 1.
struct TableCache { float* p; size_t bytes; };
int cache_edge_entries(const FftPlan& fp, const Shape& s) {
    BandParams bp{};
    BandEdge e[kBandMaxEdge];
    return band_edges(s.T, s.K, s.hop, fp.L, fp.padL, bp, e) ? bp.n_edge : 0;
}
size_t table_cache_floats(const FftPlan& fp, const Shape& s) {
    const BandLayout bl = band_layout(s.F, s.K, s.hop);
    const int roles = bl.stat ? 2 + cache_edge_entries(fp, s) : 1;
    return fft_table_floats(fp, s.F, false) + bl.spec0 + (size_t)roles * s.F * kStampWords;
}
unsigned* table_cache_stamps(const FftPlan& fp, float* cache, const Shape& s) {
    return reinterpret_cast<unsigned*>(cache + fft_table_floats(fp, s.F, false) + band_layout(s.F, s.K, s.hop).spec0);
}

// ---- single-launch small-batch forward (leaf_fft_small.hpp): one workgroup per (clip, filter)
struct SmallPlan {
    bool ok;
    bool split;            // two workgroups of seven waves per (clip, filter) (leaf_fft_small.hpp, SPLIT): while 2 B F workgroups get a CU each
    int nblk, ring, TP;
    size_t lds;
    size_t carry_floats;   // SPLIT: the seam's EMA states, [B][F] (ticket, value) pairs, behind the per-clip scales in the workspace
};
#ifndef LEAF_SMALL_ROUNDS
#define LEAF_SMALL_ROUNDS 2            // rounds of (clip, filter) workgroups over the CUs up to which a batch takes the one-launch kernel (2: 7 .. 12 clips of the default front end 41 -> 30 us; 4: slower than three launches from 16 clips)
#endif
SmallPlan make_small_plan(const Shape& s, int cus) {
    const auto [B, T, F, K, hop] = s;
    SmallPlan sp{};
    if (!((K == 401 && hop == 160) || (K == 201 && hop == 80))) return sp;
    const int L = fft_block_len(K, hop, true);
    sp.nblk = ceil_div(T, L);
    sp.TP = (T - 1) / hop + 1;
    sp.ring = std::min(sp.nblk, kSmallRing);
    sp.lds = fft_small_lds_bytes(kSmallWaves, sp.TP);
    // every (clip, filter) pair gets a CU of its own in one round (LEAF_SMALL_ROUNDS = 2: or in two); clips of up to two ring passes
    sp.ok = (long long)B * F <= (long long)LEAF_SMALL_ROUNDS * cus && F <= 65535 && B <= 65535 && sp.nblk <= kSmallMaxBlocks && sp.lds <= (size_t)kMaxLds;
    static const bool split_off = [] { const char* e = tools_env("LEAF_SMALL_SPLIT"); return e && atoi(e) == 0; }();   // tools only: A/B
    if (sp.ok && !split_off && 2ll * B * F <= cus && sp.nblk >= 2 && sp.nblk <= 2 * (kSmallSplitRing - 1) &&
        fft_small_split_lds_bytes(sp.TP) <= (size_t)kMaxLds) {
        sp.split = true;
        sp.lds = fft_small_split_lds_bytes(sp.TP);
        sp.carry_floats = align_up((size_t)B * F * 4, 64);
    }
    return sp;
}

// AUTO: the overlap-save FFT kernel whenever its plan fits and the window is long enough to pay for the transforms --
// its cost per block does not depend on K, the direct MFMA kernel's grows with K.  Measured on MI355X
// (tools/sweep_window.py, B = 256 x 1 s): K = 101/151/201: 338/289/415 us FFT vs 249/317/382 us MFMA (a tie);
// K = 251: 389 vs 841 us; K = 401: 386 vs 1122 us; K = 801: 1.43 vs 4.24 ms.  Batch size does not enter: with the
// filters-per-task adaptation the FFT path also wins at B = 1 (37 vs 58 us, tools/sweep_small_batch.py).
// Short windows / geometries the FFT plan rejects -> MFMA; staged as the last resort.
int auto_algo(const Shape& s, int cus, bool allow_small = true) {
    const int B = s.B, K = s.K, hop = s.hop;
    if (allow_small && make_small_plan(s, cus).ok) return LEAF_ALGO_FFT_SMALL;  // a handful of clips: tables, transforms and PCEN in one launch
    const FftPlan fp = make_fft_plan(s, cus);
    const Fft4kPlan f4 = make_fft4k_plan(s);                             // long windows: 4096-sample blocks from ~half a block per CU
    if (f4.ok && (long long)B * f4.nblk >= fft_wg_min_blocks(cus)) return LEAF_ALGO_FFT_WG;
    if (f4.ok) {                                                          // ... below that the 2048-sample per-wave kernel, if it fits
        // (also for the static K = 801 geometry: LEAF_ALGO_FFT_WG always means the 4096-sample kernel there, which the
        // threshold above just ruled out)
        if (fp.ok) return LEAF_ALGO_FFT;
        return make_plan(s, cus).ok ? LEAF_ALGO_MFMA : LEAF_ALGO_STAGED;
    }
    if (fft_wg_auto(fp, B, K, hop, cus)) return LEAF_ALGO_FFT_WG;
    if (fp.ok && (K >= 224 || fft_static_geometry(K, hop))) return LEAF_ALGO_FFT;
    return make_plan(s, cus).ok ? LEAF_ALGO_MFMA : LEAF_ALGO_STAGED;
}
// The one selector resolver: validates the low byte of `algo` and resolves LEAF_ALGO_AUTO; the selector that runs, or
// LEAF_ERR_BAD_ALGO.  (valid_selector alone where the answer is due before the shape is known to be usable: the empty batch)
inline bool valid_selector(int sel) { return sel >= LEAF_ALGO_AUTO && sel <= LEAF_ALGO_FFT_SMALL; }
int resolve_selector(int sel, const Shape& s, int cus) {
    if (!valid_selector(sel)) return LEAF_ERR_BAD_ALGO;
    return sel == LEAF_ALGO_AUTO ? auto_algo(s, cus) : sel;
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
// float32 / int32 buffers the kernels reach with one-element accesses only (parameters, their gradients, pooled_raw, stage
// inputs and outputs): 4-byte aligned; NULL (an optional argument left out) passes
template <class... P> inline bool any_misaligned(const P*... p) { return (misaligned(p) || ...); }
// `workspace` and `tables`: the kernels read their regions (each a multiple of 256 bytes behind the base) with 8- and 16-byte
// accesses -- float2 / float4 / int4 rows, 16-byte direct-to-LDS loads, the 64-bit seam tickets: 16-byte aligned
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
// sample type of the waveform buffer (leaf_common.hpp kSample*), the value the kernels' `io_bf16` field carries
// is the feature side (out of the forward, grad_out of the backward) bfloat16?  LEAF_FLAG_OUT_BF16 says so for that side alone,
// LEAF_FLAG_IO_BF16 for both sides; the kernels carry it as bit 2 of their `mode`
inline bool feat_bf16(int flags) { return (flags & (LEAF_FLAG_IO_BF16 | LEAF_FLAG_OUT_BF16)) != 0; }
inline int x_sample_type(int flags) {
    return (flags & LEAF_FLAG_IO_BF16) ? kSampleBf16 : (flags & LEAF_FLAG_X_PCM16) ? kSamplePcm16 : kSampleF32;
}

// Every inst_*.hip was compiled with the launch structs' layout this unit has (leaf_params.hpp: the types are shared, the object
// files of an incremental build are not).  Checked once; a mismatch fails every entry point with LEAF_ERR_LAUNCH.
bool inst_layouts_ok() {
    static const bool ok = [] {
        for (unsigned (*unit)() : {leaf_layout_fft, leaf_layout_fft_small, leaf_layout_fft_stream, leaf_layout_fft_wg, leaf_layout_fft_wg_streamfin,
                                   leaf_layout_fft_wg_x16, leaf_layout_fft_wg_mix, leaf_layout_fft_wg_mix16, leaf_layout_fft_wg_bwd,
                                   leaf_layout_fft_wg_bwd_dx, leaf_layout_fft_wgg, leaf_layout_fft_wgg4k_bwd, leaf_layout_fft_wgg_bwd,
                                   leaf_layout_fft_wgg_bwd_dx, leaf_layout_fused, leaf_layout_head_bwd})
            if (unit() != leaf_params_layout()) return false;
        return true;
    }();
    return ok;
}

int check_shape(int B, int T, int F, int K, int hop) {
    if (B < 1 || T < 1 || F < 1 || K < 1 || hop < 1) return LEAF_ERR_BAD_SHAPE;
    if ((long long)B * T >= (1ll << 31)) return LEAF_ERR_BAD_SHAPE;
    if (!inst_layouts_ok()) return LEAF_ERR_LAUNCH;                       // a build whose units disagree about the kernel arguments
    return LEAF_OK;
}

// B == 0 is the EMPTY BATCH, not an error: the reference returns a (0, F, T') tensor for it (frontend.py:78-89 ->
// convolution.py:97 on a zero-size batch) and autograd gives zero parameter gradients.  Entry points that take a batch
// accept it, launch nothing (the backward zero-fills the parameter gradients) and return LEAF_OK; the data pointers of an
// empty batch may be NULL.  Every other extent must still be valid.
inline bool empty_batch(int B, int T, int F, int K, int hop) { return B == 0 && T >= 1 && F >= 1 && K >= 1 && hop >= 1; }

size_t staged_workspace_floats(const Shape& s) {
    const auto [B, T, F, K, hop] = s;
    const int TP = (T + (K - 1) - K) / hop + 1;
    return align_up((size_t)2 * F * K, 64) + align_up((size_t)F * K, 64) + align_up((size_t)B * 2 * F * T, 64) +
           align_up((size_t)B * F * T, 64) + align_up((size_t)B * F * TP, 64);
}

// the row kernel of the overlap-save paths; `own` = the dealing of the main kernel when that kernel finalized the clips it
// owned outright (OwnedClips{} = none: every row is finalized here)
inline void launch_fft_finalize(const FinParams& fin, int B, const OwnedClips& own, int cus, hipStream_t st) {
    const int tiles = ceil_div(B * fin.F, kFinKernelRows);
    if (tiles > 2 * cus)
        hipLaunchKernelGGL(fft_finalize_kernel<512>, dim3(tiles), dim3(512), 0, st, fin, B, own);
    else
        hipLaunchKernelGGL(fft_finalize_kernel<1024>, dim3(tiles), dim3(1024), 0, st, fin, B, own);
}
// does the contiguous dealing give every clip to a single workgroup?  (then the row kernel has nothing left to do)
inline bool all_clips_owned(const OwnedClips& own) {
    if (own.nblocks <= 0) return false;
    for (int w = 0; w < own.G; ++w)
        if (own.start(w) % own.nblk != 0) return false;
    return true;
}

#define LEAF_LAUNCH_CHECK()                                  \
    do {                                                     \
        if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH; \
    } while (0)

// workspace of the forward behind a RESOLVED selector (bytes); 0: the selector does not apply to the shape
size_t forward_workspace_bytes(const Shape& s, int sel, int cus) {
    switch (sel) {
        case LEAF_ALGO_FFT_SMALL: {                           // nothing but the per-clip scales of LEAF_FLAG_PEAKNORM
            const SmallPlan sp = make_small_plan(s, cus);
            return sp.ok ? (align_up((size_t)s.B, 64) + sp.carry_floats) * 4 : 0;
        }
        case LEAF_ALGO_FFT:
        case LEAF_ALGO_FFT_WG: {
            const FftPlan fp = make_fft_plan(s, cus);
            const Fft4kPlan f4 = make_fft4k_plan(s);
            if (sel == LEAF_ALGO_FFT_WG && f4.ok) return fft4k_workspace_floats(f4, s.B) * 4;
            if (sel == LEAF_ALGO_FFT_WG && !fft_wg_available(fp, s.K, s.hop)) return 0;
            return fp.ok ? fft_workspace_floats(fp, s.F, s.B) * 4 : 0;
        }
        case LEAF_ALGO_MFMA: {
            const FusedPlan pl = make_plan(s, cus);
            return pl.ok ? (align_up(pl.w_floats, 64) + align_up(pl.g_floats, 64) + align_up(pl.meta_ints, 64) +
                            align_up(pl.part_floats, 64) + (LEAF_TRACE ? 16 * 64 * 2 : 0)) * 4
                         : 0;
        }
        case LEAF_ALGO_STAGED: return staged_workspace_floats(s) * 4;
    }
    return 0;
}

// a kernel with dynamic LDS: raise the function's limit (the attribute is per function and device: set on every call -- a
// host-side table lookup), launch, report a launch error
template <class Params>
int launch_lds(void (*fn)(const Params), dim3 grid, int waves, size_t lds, hipStream_t st, const Params& prm) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(fn, grid, dim3(waves * 64), lds, st, prm);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}
inline int cu_grid(int work, int cus) { return std::max(1, std::min(work, cus)); }   // persistent workgroups: one per CU at most

// the FftParams fields that an FftPlan decides (the 2048-sample kernels, forward and backward)
void fill_fft_params(FftParams& q, const FftPlan& fp, const Shape& s) {
    q.B = s.B; q.T = s.T; q.TP = fp.TP; q.F = s.F; q.K = s.K; q.hop = s.hop; q.padL = fp.padL;
    q.L = fp.L; q.nblk = fp.nblk; q.GZ = fp.GZ; q.nslot = fp.nslot; q.g_bufs = fp.g_bufs; q.NT = fp.NT; q.fq = fp.fq; q.nfq = fp.nfq;
    q.scr_floats = fp.scr_floats;
    q.total_tasks = s.B * fp.nblk * fp.nfq;
    q.rot = s.K / 2;
}

// Band-limited filter tasks (leaf_band.hpp, leaf_band_bwd.hpp): where a call's tables live, and the wiring of the table launch's
// arguments (`ba`) and the main kernel's (`band`) that the four sites share -- the 2048- and 4096-sample forwards and backwards.
// What differs between them is explicit: the backward's derivative slabs (`bwd_slabs`, with gz2 / edge2 in `t`) and where the
// bias-aware energy bound applies (`bias`, `smax`: the forward always, the backward unless it is asked for round 5's rule);
// `cross`, `edge_only` and the tools' `force` belong to single sites and are set there.
struct BandTabs { int* rec; float* gz; float* gz2; float* edge; float* edge2; int* elist; };
void wire_band(BandTabArgs& ba, BandParams& band, const BandTabs& t, const Shape& s, int L, int padL, bool strict, int bwd_slabs,
               const float* bias, float smax) {
    ba.T = s.T; ba.L = L; ba.hop = s.hop; ba.padL = padL;
    ba.eps2 = kBandEps2; ba.eta = strict ? kBandEta : kBandEtaFree;      // (leaf_band.hpp: round 6's aliasing bound)
    ba.bwd_slabs = bwd_slabs;
    ba.rec = t.rec; ba.gz = t.gz; ba.gz2 = t.gz2; ba.edge = t.edge; ba.edge2 = t.edge2; ba.elist = t.elist; ba.n_edge = band.n_edge;
    band.rec = t.rec; band.gz = t.gz; band.gz2 = t.gz2; band.edge = t.edge; band.edge2 = t.edge2; band.elist = t.elist;
    band.bias = bias; band.smax = smax;                                   // the energy bound follows this call's bias (leaf_band.hpp)
}
// tools only (LEAF_BAND): 0 switches the forward's band tasks off, 1 / 2 force a class
inline int band_env() {
    static const int v = [] { const char* e = tools_env("LEAF_BAND"); return e ? atoi(e) : -1; }();
    return v;
}
// tools only (LEAF_FIN_FUSED=0): no finalize in the workgroup kernels' tails (A/B)
inline bool fin_fused_off() {
    static const bool off = [] { const char* e = tools_env("LEAF_FIN_FUSED"); return e && atoi(e) == 0; }();
    return off;
}

// the pre-floor pooled energies from the overlap-save partial sums (mode 8), where the caller of the backward saved none
void finalize_pooled_raw(const LeafArgs& a, const float* part, const SlotGeom& geom, float* raw, int cus) {
    const int TP = (a.s.T - 1) / a.s.hop + 1;
    launch_fft_finalize(FinParams{part, a.s.F, TP, geom, a.pool_b, a.alpha, a.delta, a.root, a.ema_w, 1e-12f, 8, raw, raw, nullptr},
                        a.s.B, OwnedClips{}, cus, a.st);
}
// dL/dx from the per-block input gradients: `planes` planes of `N` samples per block
int launch_dx_gather(bool bf16, const float* dxblk, const Shape& s, int nblk, int planes, int L, int padL, float* g_x, int N, hipStream_t st) {
    hipLaunchKernelGGL(bf16 ? fft_dx_gather_kernel<true> : fft_dx_gather_kernel<false>, dim3(ceil_div(s.T, 1024), s.B), dim3(256), 0, st,
                       dxblk, s.T, nblk, planes, L, padL, g_x, N);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

}  // namespace

extern "C" {

int leaf_abi_version(void) { return LEAF_ABI_VERSION; }

const char* leaf_status_string(int status) {
    switch (status) {
        case LEAF_OK: return "ok";
        case LEAF_ERR_NULL_POINTER: return "null pointer argument";
        case LEAF_ERR_BAD_SHAPE: return "bad shape (T,F,K,hop must be >= 1, B >= 0 and B*T < 2^31)";
        case LEAF_ERR_WORKSPACE: return "workspace missing or too small (see leaf_workspace_bytes)";
        case LEAF_ERR_BAD_ALGO: return "unknown or inapplicable algorithm selector";
        case LEAF_ERR_LAUNCH: return "HIP kernel launch failed";
        case LEAF_ERR_NO_DEVICE: return "no usable gfx950 device";
        case LEAF_ERR_ALIGNMENT: return "buffer not 4-byte aligned (2-byte for bfloat16 and 16-bit PCM buffers; 16-byte for workspace and tables)";
        case LEAF_ERR_UNSUPPORTED: return "combination not supported (bfloat16 I/O and 16-bit PCM input (LEAF_FLAG_X_PCM16) and bfloat16 features (LEAF_FLAG_OUT_BF16) have no staged forward: use float32 buffers; LEAF_FLAG_X_PCM16 excludes LEAF_FLAG_IO_BF16 and has no dL/dx (g_x must be NULL); the waveform-mixup entries (leaf_*_mix_f32) take neither LEAF_FLAG_IO_BF16 nor LEAF_FLAG_PEAKNORM nor g_x; LEAF_FLAG_PEAKNORM needs an overlap-save path and has no backward)";
    }
    return "unknown status";
}

int leaf_auto_algo(int B, int T, int F, int K, int hop) {
    if (check_shape(B, T, F, K, hop) != LEAF_OK) return LEAF_ERR_BAD_SHAPE;
    return auto_algo(Shape{B, T, F, K, hop}, device_cus());
}

int leaf_fft_plan_info(int B, int T, int F, int K, int hop, int* info) {
    if (!info) return LEAF_ERR_NULL_POINTER;
    if (check_shape(B, T, F, K, hop) != LEAF_OK) return LEAF_ERR_BAD_SHAPE;
    const Shape s{B, T, F, K, hop};
    const FftPlan fp = make_fft_plan(s, device_cus());
    const Fft4kPlan f4 = make_fft4k_plan(s);
    if (f4.ok && auto_algo(s, device_cus()) == LEAF_ALGO_FFT_WG) {        // what AUTO runs is the 4096-sample plan
        info[0] = kFft4N; info[1] = f4.L; info[2] = f4.nblk; info[3] = F; info[4] = 1; info[5] = f4.nslot;
        info[6] = 0; info[7] = (int)f4.lds;
        return LEAF_OK;
    }
    if (!fp.ok) return LEAF_ERR_BAD_ALGO;
    info[0] = kFftN; info[1] = fp.L; info[2] = fp.nblk; info[3] = fp.fq; info[4] = fp.nfq; info[5] = fp.nslot;
    info[6] = fp.g_bufs; info[7] = (int)fp.lds;
    return LEAF_OK;
}

int leaf_num_frames(int T, int K, int hop) {
    if (T < 1 || K < 1 || hop < 1) return LEAF_ERR_BAD_SHAPE;
    const int padL = K / 2 + K % 2 - 1, padR = K / 2;
    return (T + padL + padR - K) / hop + 1;
}

size_t leaf_workspace_bytes(int B, int T, int F, int K, int hop, int algo) {
    if (check_shape(B, T, F, K, hop) != LEAF_OK) return 0;
    const CallCtx ctx = forward_ctx(algo);                   // LEAF_ALGO_RESERVE_CUS(k): AUTO resolves as the forward call will
    const Shape s{B, T, F, K, hop};
    const int sel = resolve_selector(ctx.sel, s, ctx.cus);
    return sel < 0 ? 0 : forward_workspace_bytes(s, sel, ctx.cus);
}

int leaf_gabor_taps_f32(const float* kernel, int F, int K, float* taps, void* stream) {
    if (!kernel || !taps) return LEAF_ERR_NULL_POINTER;
    if (F < 1 || K < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(kernel, taps)) return LEAF_ERR_ALIGNMENT;
    hipLaunchKernelGGL(taps_direct_kernel, dim3(ceil_div(F * K, 256)), dim3(256), 0, (hipStream_t)stream, kernel, F, K,
                       gabor_bounds(K), taps);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_lowpass_window_f32(const float* pool_w, int F, int K, float* window, void* stream) {
    if (!pool_w || !window) return LEAF_ERR_NULL_POINTER;
    if (F < 1 || K < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(pool_w, window)) return LEAF_ERR_ALIGNMENT;
    hipLaunchKernelGGL(lowpass_window_kernel, dim3(ceil_div(F * K, 256)), dim3(256), 0, (hipStream_t)stream, pool_w, F, K,
                       window);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_gabor_conv_f32(const float* x, int B, int T, const float* kernel, int F, int K, float* y, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!x || !kernel || !y) return LEAF_ERR_NULL_POINTER;
    if (check_shape(B, T, F, K, 1) != LEAF_OK || 2 * F > 65535 || B > 65535) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(x, kernel, y) || misaligned16(workspace)) return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < (size_t)2 * F * K * 4) return LEAF_ERR_WORKSPACE;
    float* taps = static_cast<float*>(workspace);
    int rc = leaf_gabor_taps_f32(kernel, F, K, taps, stream);
    if (rc != LEAF_OK) return rc;
    const int padL = K / 2 + K % 2 - 1;
    hipLaunchKernelGGL(conv_staged_kernel, dim3(ceil_div(T, 256), 2 * F, B), dim3(256), 0, (hipStream_t)stream, x, taps, B,
                       T, 2 * F, K, padL, y);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_squared_modulus_f32(const float* y, int B, int F, int T, float* e, void* stream) {
    if (!y || !e) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || T < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(y, e)) return LEAF_ERR_ALIGNMENT;
    const size_t n = (size_t)B * F * T;
    hipLaunchKernelGGL(sqmod_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y,
                       (size_t)B * F, T, e);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_gaussian_lowpass_f32(const float* e, int B, int F, int T, const float* pool_w, const float* pool_b, int K,
                              int hop, float* pooled, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || !pool_w || !pooled) return LEAF_ERR_NULL_POINTER;
    if (check_shape(B, T, F, K, hop) != LEAF_OK || F > 65535 || B > 65535) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(e, pool_w, pool_b, pooled) || misaligned16(workspace)) return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < (size_t)F * K * 4) return LEAF_ERR_WORKSPACE;
    float* g = static_cast<float*>(workspace);
    int rc = leaf_lowpass_window_f32(pool_w, F, K, g, stream);
    if (rc != LEAF_OK) return rc;
    const int TP = leaf_num_frames(T, K, hop);
    const int padL = K / 2 + K % 2 - 1;
    hipLaunchKernelGGL(pool_staged_kernel, dim3(ceil_div(TP, 64), F, B), dim3(64), 0, (hipStream_t)stream, e, g, pool_b, F,
                       T, TP, K, hop, padL, pooled);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_ema_f32(const float* p, int B, int F, int TP, const float* ema_w, float* ema, void* stream) {
    if (!p || !ema_w || !ema) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || TP < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(p, ema_w, ema)) return LEAF_ERR_ALIGNMENT;
    hipLaunchKernelGGL(pcen_rows_kernel, dim3(ceil_div(B * F, 64)), dim3(64), 0, (hipStream_t)stream, p, B * F, F, TP,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, ema_w, 0.0f, 0, ema);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_pcen_f32(const float* p, int B, int F, int TP, const float* alpha, const float* delta, const float* root,
                  const float* ema_w, float floor_, float* out, void* stream) {
    if (!p || !alpha || !delta || !root || !ema_w || !out) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || TP < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(p, alpha, delta, root, ema_w, out)) return LEAF_ERR_ALIGNMENT;
    hipLaunchKernelGGL(pcen_rows_kernel, dim3(ceil_div(B * F, 64)), dim3(64), 0, (hipStream_t)stream, p, B * F, F, TP,
                       alpha, delta, root, ema_w, floor_, 1, out);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_pcen_stream_f32(const float* p, int B, int F, int n, const float* alpha, const float* delta, const float* root,
                         const float* ema_w, float floor_, int log1p_, const float* ema_in, float* ema_out, float* out,
                         void* stream) {
    if (!p || !out) return LEAF_ERR_NULL_POINTER;
    if (alpha && (!delta || !root || !ema_w)) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || n < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(p, alpha, delta, root, ema_w, ema_in, ema_out, out)) return LEAF_ERR_ALIGNMENT;
    FinParams q{};
    q.F = F; q.TP = n; q.alpha = alpha; q.delta = delta; q.root = root; q.ema_w = ema_w; q.floor_ = floor_;
    q.mode = alpha ? 1 : (log1p_ ? 2 : 0);
    q.out = out;
    hipLaunchKernelGGL(pcen_stream_kernel, dim3(ceil_div(B * F, 64)), dim3(64), 0, (hipStream_t)stream, p, B * F, n, q, ema_in,
                       ema_out);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

// ---- stage backwards: what autograd derives for each reference module called on its own ---------------------

size_t leaf_stage_backward_workspace_bytes(int stage, int B, int T, int F, int K, int hop) {
    if (B < 1 || T < 1 || F < 1) return 0;
    const size_t TP = K >= 1 && hop >= 1 ? (size_t)leaf_num_frames(T, K, hop) : 0;
    switch (stage) {
        case LEAF_STAGE_GABOR_CONV: return (align_up((size_t)2 * F * K, 64) + align_up((size_t)B * 2 * F * K, 64)) * 4;
        case LEAF_STAGE_LOWPASS: return (align_up((size_t)F * K, 64) * 2 + align_up((size_t)F, 64)) * 4;
        case LEAF_STAGE_EMA: return (align_up((size_t)B * F * T, 64) + align_up((size_t)B * F, 64)) * 4;      // T = frames here
        case LEAF_STAGE_PCEN: return (align_up((size_t)B * F * T, 64) + align_up((size_t)B * F * 4, 64)) * 4; // T = frames here
    }
    (void)TP;
    return 0;
}

int leaf_gabor_conv_backward_f32(const float* x, int B, int T, const float* kernel, int F, int K, const float* grad_y,
                                 float* g_kernel, float* g_x, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !kernel || !grad_y) return LEAF_ERR_NULL_POINTER;
    if (check_shape(B, T, F, K, 1) != LEAF_OK || 2 * F > 65535 || B > 65535) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(x, kernel, grad_y, g_kernel, g_x) || misaligned16(workspace)) return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < leaf_stage_backward_workspace_bytes(LEAF_STAGE_GABOR_CONV, B, T, F, K, 1))
        return LEAF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* taps = static_cast<float*>(workspace);
    float* tpart = taps + align_up((size_t)2 * F * K, 64);
    const int padL = K / 2 + K % 2 - 1;
    int rc = leaf_gabor_taps_f32(kernel, F, K, taps, stream);
    if (rc != LEAF_OK) return rc;
    if (g_kernel) {
        hipLaunchKernelGGL(dtaps_partial_kernel, dim3(ceil_div(K, 128), 2 * F, B), dim3(128), 0, st, grad_y, x, T, 2 * F, K,
                           padL, tpart);
        LEAF_LAUNCH_CHECK();
        hipLaunchKernelGGL(dkernel_kernel, dim3(F), dim3(256), 0, st, tpart, taps, kernel, B, F, K, gabor_bounds(K), g_kernel);
        LEAF_LAUNCH_CHECK();
    }
    if (g_x) {
        hipLaunchKernelGGL(dx_kernel, dim3(ceil_div(T, 256), B), dim3(256), 0, st, grad_y, taps, T, 2 * F, K, padL, g_x);
        LEAF_LAUNCH_CHECK();
    }
    return LEAF_OK;
}

int leaf_squared_modulus_backward_f32(const float* y, const float* grad_e, int B, int F, int T, float* grad_y, void* stream) {
    if (!y || !grad_e || !grad_y) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || T < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(y, grad_e, grad_y)) return LEAF_ERR_ALIGNMENT;
    const size_t n = (size_t)B * F * T;
    hipLaunchKernelGGL(sqmod_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, grad_e,
                       (size_t)B * F, T, grad_y);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_gaussian_lowpass_backward_f32(const float* e, const float* grad_pooled, int B, int F, int T, const float* pool_w,
                                       int K, int hop, float* g_e, float* g_pool_w, float* g_pool_b, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!e || !grad_pooled || !pool_w) return LEAF_ERR_NULL_POINTER;
    if (check_shape(B, T, F, K, hop) != LEAF_OK || F > 65535 || B > 65535) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(e, grad_pooled, pool_w, g_e, g_pool_w, g_pool_b) || misaligned16(workspace)) return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < leaf_stage_backward_workspace_bytes(LEAF_STAGE_LOWPASS, B, T, F, K, hop))
        return LEAF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* g = static_cast<float*>(workspace);
    float* dg = g + align_up((size_t)F * K, 64);
    float* gw_tmp = dg + align_up((size_t)F * K, 64);
    const int TP = leaf_num_frames(T, K, hop);
    const int padL = K / 2 + K % 2 - 1;
    int rc = leaf_lowpass_window_f32(pool_w, F, K, g, stream);
    if (rc != LEAF_OK) return rc;
    if (g_e) {
        hipLaunchKernelGGL(pool_bwd_de_kernel, dim3(ceil_div(T, 256), F, B), dim3(256), 0, st, g, grad_pooled, F, T, TP, K, hop,
                           padL, g_e);
        LEAF_LAUNCH_CHECK();
    }
    if (g_pool_w || g_pool_b) {
        hipLaunchKernelGGL(pool_bwd_dg_kernel, dim3(ceil_div(K, 128), F), dim3(128), 0, st, e, grad_pooled, B, F, T, TP, K, hop,
                           padL, dg);
        LEAF_LAUNCH_CHECK();
        hipLaunchKernelGGL(param_reduce_kernel, dim3(F), dim3(kParamRedThreads), 0, st, grad_pooled, dg, g, (const float*)nullptr,
                           pool_w, B, F, TP, K, 0, (const float*)nullptr, 0, 0, (const int*)nullptr,
                           g_pool_w ? g_pool_w : gw_tmp, g_pool_b, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                           (float*)nullptr);
        LEAF_LAUNCH_CHECK();
    }
    return LEAF_OK;
}

int leaf_ema_backward_f32(const float* p, const float* grad_ema, int B, int F, int TP, const float* ema_w, float* g_p,
                          float* g_ema_w, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !grad_ema || !ema_w || !g_p || !g_ema_w) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || TP < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(p, grad_ema, ema_w, g_p, g_ema_w) || misaligned16(workspace)) return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < leaf_stage_backward_workspace_bytes(LEAF_STAGE_EMA, B, TP, F, 1, 1))
        return LEAF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* M = static_cast<float*>(workspace);
    float* rowsum = M + align_up((size_t)B * F * TP, 64);
    hipLaunchKernelGGL(ema_bwd_rows_kernel, dim3(ceil_div(B * F, 64)), dim3(64), 0, st, p, grad_ema, B * F, F, TP, ema_w, M, g_p,
                       rowsum);
    LEAF_LAUNCH_CHECK();
    hipLaunchKernelGGL(rows_to_filter_sum_kernel, dim3(F), dim3(256), 0, st, rowsum, B, F, 1, 1, g_ema_w, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_pcen_backward_f32(const float* p, const float* grad_out, int B, int F, int TP, const float* alpha,
                           const float* delta, const float* root, const float* ema_w, float floor_, float* g_p,
                           float* g_alpha, float* g_delta, float* g_root, float* g_ema_w, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!p || !grad_out || !alpha || !delta || !root || !ema_w || !g_p || !g_alpha || !g_delta || !g_root || !g_ema_w)
        return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || TP < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(p, grad_out, alpha, delta, root, ema_w, g_p, g_alpha, g_delta, g_root, g_ema_w) || misaligned16(workspace))
        return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < leaf_stage_backward_workspace_bytes(LEAF_STAGE_PCEN, B, TP, F, 1, 1))
        return LEAF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* M = static_cast<float*>(workspace);
    float* rowsum = M + align_up((size_t)B * F * TP, 64);
    hipLaunchKernelGGL(pcen_bwd_rows_kernel, dim3(ceil_div(B * F, 64)), dim3(64), 0, st, p, grad_out, B * F, F, TP, alpha, delta,
                       root, ema_w, floor_, 1 | 16, M, g_p, rowsum, (const int*)nullptr, 0, (float*)nullptr);
    LEAF_LAUNCH_CHECK();
    hipLaunchKernelGGL(rows_to_filter_sum_kernel, dim3(F), dim3(256), 0, st, rowsum, B, F, 4, 4, g_alpha, g_delta, g_root,
                       g_ema_w);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

// what a forward path reads and writes besides the parameters
struct FwdIo {
    const void* x;
    int xtype;                       // sample type of x (leaf_common.hpp kSample*)
    int mode;                        // finalize mode: bit0 PCEN, bit1 log1p compression, bit2 bfloat16 features
    void* out;
    float* pooled_raw;               // leaf_forward_save_f32: the pre-floor pooled energies, else NULL
    const float* clip_scale2;        // LEAF_FLAG_PEAKNORM: the per-clip scales, else NULL
    hipEvent_t* ev;                  // leaf_forward_profiled_f32: the four stage events, else NULL
};
static inline FinParams fwd_fin_params(const LeafArgs& a, const FwdIo& io, const float* part, int TP, const SlotGeom& geom) {
    return FinParams{part, a.s.F, TP, geom, a.pool_b, a.alpha, a.delta, a.root, a.ema_w, 1e-12f, io.mode, io.out, io.pooled_raw, io.clip_scale2};
}
static inline void record(hipEvent_t* ev, int i, hipStream_t st) { if (ev) (void)hipEventRecord(ev[i], st); }

// the tables of the 2048-sample plan inside one buffer: [spectra | pooling rows | col_of | band tables]
struct FftTabPtrs { float2* H; float* Gz; int* col_of; float* band; };
static inline FftTabPtrs fft_tab_ptrs(const FftPlan& fp, float* tables, int F) {
    float* Gz = tables + align_up(fp.h_floats, 64);
    int* col_of = reinterpret_cast<int*>(Gz + align_up(fp.gz_floats, 64));
    return {reinterpret_cast<float2*>(tables), Gz, col_of, reinterpret_cast<float*>(col_of) + align_up((size_t)F, 64)};
}

// the band tasks of one 2048-sample forward call: band.rec == NULL when it runs none
struct FwdBand { BandParams band; size_t lds; const float2* spec0; };

// The table launch of the overlap-save forward, and with it the decision whether this call runs band-limited filter tasks
// (leaf_band.hpp): narrow-band filters on 256- / 512-point inverse transforms.  They need the static
// workgroup kernel of a geometry they are built for (the training forward takes them too: the pooled tensor it saves for
// the backward differs from the full-transform one by ~1e-6, the backward recomputes with full transforms).  The tables are
// built by the prep launch itself (fft_prep_band_kernel); with frozen-parameter tables
// (tables_ready) the parameter-only part is in them and only the edge tables of this clip length are built here, into
// band_scratch.  The plan takes fb.lds bytes of LDS behind everything else.
static int fft_forward_tables(const CallCtx& ctx, const FftPlan& fp, const LeafArgs& a, const FwdIo& io, float* tables,
                              bool tables_ready, bool use_wg, float* band_scratch, unsigned* stamps, FwdBand& fb) {
    const auto [B, T, F, K, hop] = a.s;
    const FftTabPtrs tp = fft_tab_ptrs(fp, tables, F);
    if (use_wg && !ctx.band_off && (!tables_ready || band_scratch)) {
        const FftWgLaunch wl = pick_fft_wg_kernel(K, hop, wg_sample_kind(io.xtype, ctx.mix.lam), fp.TP > 128);
        const BandLayout bl = band_layout(F, K, hop);
        BandTabArgs ba{};
        if (bl.stat && wl.fn && wl.nw <= 12 && !wg_force_generic() && band_env() != 0 && fp.nslot == 2 &&
            wl.lds + band_lds_bytes(F) <= (size_t)kMaxLds && band_edges(T, K, hop, fp.L, fp.padL, fb.band, ba.e)) {
            float* dyn = tables_ready ? band_scratch : tp.band + bl.stat;
            wire_band(ba, fb.band, BandTabs{reinterpret_cast<int*>(tp.band + bl.rec), tp.band + bl.gz, nullptr, dyn + bl.edge, nullptr,
                                            reinterpret_cast<int*>(dyn + bl.elist)},
                      a.s, fp.L, fp.padL, ctx.band_strict, /*bwd_slabs=*/0, a.pool_b, ctx.band_strict ? 1.0f : 2.0f);
            ba.cross = ctx.band_strict ? 0 : 1;                   // (windows across Nyquist)
            ba.force = band_env() > 0 ? band_env() : 0;
            ba.edge_only = tables_ready ? 1 : 0;
            ba.stamps = stamps; ba.strict = ctx.band_strict ? 1 : 0;   // (the table cache: validate or build)
            fb.lds = band_lds_bytes(F);
            // the main kernel's workgroups' FIRST blocks are transformed by this launch too (waves 1..7 of the workgroups (f, 0),
            // idle while wave 0 transforms the taps): the one forward transform nothing in the main kernel overlaps with (eleven
            // waves waited ~12 k cycles for it).  Other launches of this kernel (leaf_fft_prepare_tables_f32, leaf_band_classes_f32)
            // pass no dynamic LDS and spec0 = NULL.
            static const bool spec0_off = [] { const char* e = tools_env("LEAF_SPEC0"); return e && atoi(e) == 0; }();   // tools only: A/B
            const int main_grid = cu_grid(B * fp.nblk, ctx.cus);
            size_t prep_dyn = 0;
            // (16-bit PCM: the table launch reads fp32 and bf16 only -- a third sample type in its first-block loads cost the fp32 path
            // 0.9 us of the table launch at cfg1 -- so the main kernel transforms its first blocks itself: the same bits)
            // (the table cache has no first-block spectra -- they depend on x: the main kernel transforms its first blocks itself, the same bits)
            if (!spec0_off && !tables_ready && !stamps && main_grid <= kMaxCusForSpec0 && wl.nw <= 12 && io.xtype != kSamplePcm16 && !ctx.mix.lam) {   // (a mixed call likewise: the table launch does not mix)
                ba.x = io.x; ba.io_bf16 = io.xtype; ba.B = B; ba.nblk = fp.nblk; ba.G = main_grid;
                ba.spec0 = reinterpret_cast<float2*>(dyn + bl.spec0);
                fb.spec0 = ba.spec0;
                prep_dyn = (size_t)(kPrepWaves - 1) * kWgScrFloats * 4;
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fft_prep_band_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)prep_dyn);
            }
            if (!tables_ready || fb.band.n_edge > 0) {
                hipLaunchKernelGGL(fft_prep_band_kernel, dim3(F, tables_ready ? fb.band.n_edge : 2 + fb.band.n_edge), dim3(kPrepWaves * 64), prep_dyn, a.st,
                                   a.kernel, a.pool_w, F, K, fp.GZ, gabor_bounds(K), tp.H, tp.Gz, tp.col_of, ba);
                LEAF_LAUNCH_CHECK();
            }
        }
    }
    if (!tables_ready && !fb.band.rec) {
        hipLaunchKernelGGL(fft_prep_kernel, dim3(F, 1), dim3(kPrepWaves * 64), 0, a.st, a.kernel, a.pool_w, F, K, fp.GZ,
                           gabor_bounds(K), 1, tp.H, tp.Gz, tp.col_of, fft_lone_taps(tables, F, K), stamps, hop, T);
        LEAF_LAUNCH_CHECK();
    }
    return LEAF_OK;
}

// How the static workgroup kernel finalizes: blocks are dealt contiguously.  Whole clips per workgroup (the batch a multiple of the
// grid, or fewer clips than CUs never happens here: grid = min(blocks, CUs)) -> the STREAM variant: frame sums in
// an LDS ring, finalized as the blocks complete, no `part`, no second kernel.  Otherwise a workgroup finalizes the
// clips it owns outright in its tail and the row kernel sees the clips that straddle two workgroups.
// Adjusts the launch (`wl`: kernel and LDS) and the kernel's arguments (`q`); true: every clip is finalized by the main kernel.
static bool fft_wg_fused_finalize(const CallCtx& ctx, const FftPlan& fp, const Shape& s, int grid, size_t band_lds,
                                  const FinParams& fin, FftWgLaunch& wl, FftParams& q, OwnedClips& own) {
    const int B = s.B, F = s.F;
    own = OwnedClips{B * fp.nblk, grid, fp.nblk};
    const bool all_owned = all_clips_owned(own);
    q.fin = fin;
    q.fin_fused = 1;
    // every workgroup gets the same number of whole clips and their per-frame sums fit behind its scratch: the sums stay
    // in LDS (ds_add_f32 of the two blocks a window meets; the tail reads them there) -- no `part` traffic at all
    static const bool lds_sums_off = [] { const char* e = tools_env("LEAF_LDS_SUMS"); return e && atoi(e) == 0; }();   // tools only: A/B
    if (all_owned && wl.lds_sums && fp.nslot == 2 && !lds_sums_off && !ctx.stream_finalize && (B * fp.nblk) % grid == 0) {
        const size_t extra = (((size_t)(B / grid) * F * fp.TP + 7) / 8 * 8 + (size_t)F * 8) * 4;   // the sums + the filters' finalize coefficients
        if (B % grid == 0 && wl.lds + extra + band_lds <= (size_t)kMaxLds) {
            wl.lds += extra;
            q.fin_fused = 3;
        }
    }
    static const int stream_env = [] { const char* e = tools_env("LEAF_WG_STREAM"); return e ? atoi(e) : -1; }();   // tools only: A/B
    // LEAF_ALGO_STREAM_FINALIZE asks for it; without the flag it is what runs wherever the workgroups own whole clips
    // but their frame sums do NOT fit the LDS (several clips per workgroup, long clips: BASELINE configs[3], [4]) --
    // there the alternative is the round trip of every partial sum through `part` in HBM (2x the algorithmic traffic)
    const bool want_stream = stream_env >= 0 ? stream_env != 0 : (ctx.stream_finalize || q.fin_fused != 3);
    if (all_owned && wl.fn_stream && fp.nslot == 2 && want_stream) {
        // the longest ring the LDS holds, up to four times the minimum (lag >= 4: the forward tasks never wait)
        int ring = 0;
        for (int r = 4 * wg_stream_ring_min(wl.sk, wl.shop); r >= wg_stream_ring_min(wl.sk, wl.shop); r >>= 1)
            if (fft_wg_stream_lds_bytes(wl.nw, wl.sk, r, F) + band_lds <= (size_t)kMaxLds) { ring = r; break; }
        if (ring) {
            wl.fn = wl.fn_stream;
            wl.lds = fft_wg_stream_lds_bytes(wl.nw, wl.sk, ring, F);
            q.stream_ring = ring;
            q.fin_fused = 2;
        }
    }
    return all_owned;
}

// The overlap-save forward: (tables) -> main kernel -> finalize.  With tables_ready the tables were produced earlier by
// leaf_fft_prepare_tables_f32 from the same parameters (inference with frozen parameters) and the prep launch is skipped.
// With `stamps` (leaf_forward_cached_f32) `tables` is the caller's table cache: the prep launch validates or builds it.
static int fft_forward(const CallCtx& ctx, const FftPlan& fp, const LeafArgs& a, const FwdIo& io, float* tables, float* part,
                       bool tables_ready, bool use_wg, float* band_scratch = nullptr, unsigned* stamps = nullptr) {
    const auto [B, T, F, K, hop] = a.s;
    const FftTabPtrs tp = fft_tab_ptrs(fp, tables, F);
    record(io.ev, 0, a.st);
    FwdBand fb{};
    int rc = fft_forward_tables(ctx, fp, a, io, tables, tables_ready, use_wg, band_scratch, stamps, fb);
    if (rc != LEAF_OK) return rc;
    record(io.ev, 1, a.st);
    FftParams q{};
    q.x = io.x; q.io_bf16 = io.xtype; q.H = tp.H; q.Gz = tp.Gz; q.part = part;
    fill_fft_params(q, fp, a.s);
    q.lone = fft_lone_taps(tables, F, K);
    q.mix_perm = ctx.mix.perm; q.mix_lam = ctx.mix.lam;
#if LEAF_TRACE
    q.trace = reinterpret_cast<unsigned long long*>(part + align_up(fp.part_floats, 64));
#endif
    const FinParams fin = fwd_fin_params(a, io, part, fp.TP, SlotGeom{fp.L, fp.padL, K, hop, T, fp.nslot});
    OwnedClips own{};                                        // which clips the main kernel finalizes itself (none by default)
    bool all_owned = false;
    if (use_wg) {
        // one persistent workgroup per CU walks its blocks through an LDS task queue (leaf_fft_wg.hpp)
        FftWgLaunch wl = pick_fft_wg_kernel(K, hop, wg_sample_kind(io.xtype, ctx.mix.lam), fp.TP > 128);
        if (!wl.fn || wg_force_generic()) {                   // run-time geometry (any other window, odd or even)
            if (ctx.mix.lam) return LEAF_ERR_BAD_ALGO;        // (these kernels do not mix in their loads: mix_fused_forward sends them a mixed copy)
            wl = pick_fft_wgg_kernel(fp, K, hop);
        }
        if (!wl.fn) return LEAF_ERR_BAD_ALGO;
        const int grid = cu_grid(B * fp.nblk, ctx.cus);
        if (wl.fused_finalize && !fin_fused_off())
            all_owned = fft_wg_fused_finalize(ctx, fp, a.s, grid, fb.lds, fin, wl, q, own);
        if (fb.band.rec) {                                    // (decided before the prep launch, which built the tables)
            q.spec0 = fb.spec0;
            q.band = fb.band;
            q.band.lds_off = (int)(wl.lds / 4);
            wl.lds += fb.lds;
        }
        rc = launch_lds(wl.fn, dim3(grid), wl.nw, wl.lds, a.st, q);
    } else {
        FftKernel kfn = ctx.mix.lam ? pick_fft_kernel_mix(fp, K, hop, false) : pick_fft_kernel(fp, K, hop, false);
        if (!kfn) return LEAF_ERR_BAD_ALGO;                   // (mixed call: mix_fused_forward admits the static odd windows only)
        rc = launch_lds(kfn, dim3(cu_grid(ceil_div(q.total_tasks, kFftWaves), ctx.cus)), kFftWaves, fp.lds, a.st, q);
    }
    if (rc != LEAF_OK) return rc;
    record(io.ev, 2, a.st);
    if (!all_owned) launch_fft_finalize(fin, B, own, ctx.cus, a.st);
    LEAF_LAUNCH_CHECK();
    record(io.ev, 3, a.st);
    return LEAF_OK;
}

int leaf_peak_normalize_f32(const float* x, int B, int T, float* out, void* stream) {
    if (!x || !out) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || T < 1) return LEAF_ERR_BAD_SHAPE;
    if (any_misaligned(x, out)) return LEAF_ERR_ALIGNMENT;
    hipLaunchKernelGGL(peak_normalize_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, T, out);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

// LEAF_ALGO_FFT_SMALL -- one launch: grid (F, B), every workgroup builds its filter's tables, transforms its clip's blocks and
// finalizes its row
static int forward_small(const CallCtx& ctx, const LeafArgs& a, const FwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    const SmallPlan sp = make_small_plan(a.s, ctx.cus);
    if (!sp.ok) return LEAF_ERR_BAD_ALGO;
    const SmallKernel kfn = ctx.mix.lam ? leaf_inst_fft_small_mix(K, sp.split) : leaf_inst_fft_small(K, sp.split);
    if (!kfn) return LEAF_ERR_BAD_ALGO;
    SmallParams q{};
    q.x = io.x; q.io_bf16 = io.xtype; q.kernel = a.kernel; q.pool_w = a.pool_w; q.bd = gabor_bounds(K);
    q.B = B; q.T = T; q.TP = sp.TP; q.F = F; q.nblk = sp.nblk; q.ring = sp.split ? kSmallSplitRing : sp.ring;
    q.mix_perm = ctx.mix.perm; q.mix_lam = ctx.mix.lam;
    q.fin = fwd_fin_params(a, io, nullptr, sp.TP, SlotGeom{fft_block_len(K, hop, true), K / 2 + K % 2 - 1, K, hop, T, 2});
    record(io.ev, 0, a.st); record(io.ev, 1, a.st);
    if (sp.split) {
        // this launch's ticket for the seam hand-over (64 bits from a random seed: stale or uninitialised workspace never matches)
        static std::atomic<unsigned long long> ticket{[] { std::random_device rd; return ((unsigned long long)rd() << 32) ^ rd(); }()};
        q.epoch = ticket.fetch_add(1, std::memory_order_relaxed) + 1;
        if (q.epoch == 0) q.epoch = ticket.fetch_add(1, std::memory_order_relaxed) + 1;   // 0 = "taken out" (the consumer resets the slot)
        q.carry = reinterpret_cast<unsigned long long*>(ws);          // (the per-clip scales sit at the workspace's end)
    }
    const int rc = launch_lds(kfn, dim3(F, B, sp.split ? 2 : 1), sp.split ? kSmallSplitWaves : kSmallWaves, sp.lds, a.st, q);
    if (rc != LEAF_OK) return rc;
    record(io.ev, 2, a.st); record(io.ev, 3, a.st);
    return LEAF_OK;
}

// ---- the one-launch streaming step (leaf_fft_stream.hpp): history and smoother state resident in `state` between calls
// state = [history half 0 | history half 1 | ema], each region a multiple of 256 bytes behind the base
static inline bool stream_geometry(int K, int hop) { return (K == 401 && hop == 160) || (K == 201 && hop == 80); }
struct StreamLayout { int H; size_t half, ema, total; };               // samples per clip and half; byte offsets
static StreamLayout stream_layout(int B, int F, int K, int hop, bool pcm) {
    StreamLayout L{};
    L.H = leaf_stream_history_samples(K, hop);
    L.half = align_up((size_t)B * L.H * (pcm ? 2 : 4), 256);
    L.ema = 2 * L.half;
    L.total = L.ema + (size_t)B * F * 4;
    return L;
}

// The most samples a stream owes its next step.  LeafStream (leaf_pytorch_amd/streaming.py) keeps the buffer from a whole number of
// hops, `lead` = ceil(2 padL / hop) frames, in front of the next frame to emit (the frame's pooling window reaches padL back, the
// filters another padL), and emits frame m once sample m hop + reach has arrived, reach = 2 (K - 1 - padL).  After a step that
// saw L samples and emitted up to frame `last` = floor((L - 1 - reach) / hop), _advance keeps L - (last + 1 - lead) hop samples,
// and (last + 1) hop >= L - reach: at most reach + lead hop.  A step that emits nothing has floor((L - 1 - reach) / hop) < next
// <= lead, so it too holds L <= reach + lead hop samples.
int leaf_stream_history_samples(int K, int hop) {
    if (K < 1 || hop < 1) return 0;
    const int padL = K / 2 + K % 2 - 1;
    return 2 * (K - 1 - padL) + ceil_div(2 * padL, hop) * hop;
}

size_t leaf_stream_state_bytes(int B, int F, int K, int hop, int flags) {
    if (B < 1 || F < 1 || !stream_geometry(K, hop) || (flags & (LEAF_FLAG_IO_BF16 | LEAF_FLAG_PEAKNORM))) return 0;
    return stream_layout(B, F, K, hop, (flags & LEAF_FLAG_X_PCM16) != 0).total;
}

// the blocks c_lo .. c_lo + nb - 1 of a buffer of T samples that the windows of its frames first .. first + n - 1 (n > 0) meet
static void stream_blocks(int first, int n, int T, int K, int hop, int& c_lo, int& nb) {
    const int LS = fft_block_len(K, hop, true), padL = K / 2 + K % 2 - 1;
    c_lo = std::max(0, first * hop - padL) / LS;
    nb = std::min(T - 1, (first + n - 1) * hop - padL + K - 1) / LS - c_lo + 1;
}
// are frames first .. first + n - 1 frames of a clip of T samples?
static inline bool stream_frames_ok(int first, int n, int T, int hop) {
    const int TPv = T > 0 ? (T - 1) / hop + 1 : 0;
    return first >= 0 && n >= 0 && first <= TPv && n <= TPv - first;
}

// where a stream stands (host-side bookkeeping of the caller: nothing is read back from the device) and its buffers
struct StreamIo {
    const void* chunk;
    long long chunk_stride;
    void* state;
    int pcm, hist_len, parity, drop, first, n, started, mode;
    void* out;
};
// one launch: grid (F, B), or (1, B) for a step that only moves history.  (No per-call option reaches this path: one workgroup per
// (stream, filter) whatever the CU count.)
static int stream_step(const CallCtx&, const LeafArgs& a, const StreamIo& io) {
    const auto [B, T, F, K, hop] = a.s;                       // T: the virtual buffer [history | chunk]
    const StreamKernel kfn = leaf_inst_fft_stream(K);
    if (!kfn) return LEAF_ERR_UNSUPPORTED;
    const StreamLayout L = stream_layout(B, F, K, hop, io.pcm == kSamplePcm16);
    const int LS = fft_block_len(K, hop, true), padL = K / 2 + K % 2 - 1;
    char* base = static_cast<char*>(io.state);
    StreamParams q{};
    q.chunk = io.chunk; q.chunk_stride = io.chunk_stride; q.pcm = io.pcm;
    q.hist_in = base + (io.parity ? L.half : 0); q.hist_out = base + (io.parity ? 0 : L.half);
    q.ema_state = reinterpret_cast<float*>(base + L.ema);
    q.kernel = a.kernel; q.pool_w = a.pool_w; q.bd = gabor_bounds(K);
    q.B = B; q.F = F; q.H = L.H; q.hist_len = io.hist_len; q.Tc = T - io.hist_len; q.drop = io.drop;
    q.first = io.first; q.n = io.n; q.started = io.started;
    if (io.n > 0) stream_blocks(io.first, io.n, T, K, hop, q.c_lo, q.nb);
    q.fin = FinParams{nullptr, F, io.n, SlotGeom{LS, padL, K, hop, T, 2}, a.pool_b, a.alpha, a.delta, a.root, a.ema_w, 1e-12f, io.mode, io.out, nullptr, nullptr};
    return launch_lds(kfn, dim3(io.n > 0 ? F : 1, B), kSmallWaves, io.n > 0 ? fft_small_lds_bytes(kSmallWaves, io.n) : 0, a.st, q);
}

int leaf_stream_step_f32(const void* chunk, int B, int Tc, long long chunk_stride, void* state, size_t state_bytes, int hist_len,
                         int parity, int drop_samples, int first, int n, int started, const float* kernel, const float* pool_w,
                         const float* pool_b, const float* alpha, const float* delta, const float* root, const float* ema_w, int F,
                         int K, int hop, int flags, void* out, void* stream) {
    if (flags & (LEAF_FLAG_IO_BF16 | LEAF_FLAG_PEAKNORM)) return LEAF_ERR_UNSUPPORTED;
    if (K >= 1 && hop >= 1 && !stream_geometry(K, hop)) return LEAF_ERR_UNSUPPORTED;
    if (B == 0 && !inst_layouts_ok()) return LEAF_ERR_LAUNCH;
    if (B == 0 && Tc >= 0 && F >= 1 && K >= 1 && hop >= 1) return LEAF_OK;
    const bool use_pcen = (flags & LEAF_FLAG_PCEN) != 0;
    if (!state || !kernel || !pool_w || !pool_b || (Tc > 0 && !chunk) || (n > 0 && !out)) return LEAF_ERR_NULL_POINTER;
    if (use_pcen && (!alpha || !delta || !root || !ema_w)) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || B > 65535 || F < 1 || F > 65535 || K < 1 || hop < 1 || Tc < 0 || (Tc > 0 && B > 1 && chunk_stride < Tc)) return LEAF_ERR_BAD_SHAPE;
    if (!inst_layouts_ok()) return LEAF_ERR_LAUNCH;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0, out_bf16 = (flags & LEAF_FLAG_OUT_BF16) != 0;
    if (misaligned16(state) || (reinterpret_cast<uintptr_t>(chunk) & (pcm ? 1u : 3u)) || (reinterpret_cast<uintptr_t>(out) & (out_bf16 ? 1u : 3u)) ||
        any_misaligned(kernel, pool_w, pool_b, alpha, delta, root, ema_w))
        return LEAF_ERR_ALIGNMENT;
    // the position: everything the kernel derives an address in `state`, `chunk` or `out` from
    const StreamLayout L = stream_layout(B, F, K, hop, pcm);
    const int LS = fft_block_len(K, hop, true);
    if (hist_len < 0 || hist_len > L.H || Tc > kSmallRing * LS || (parity & ~1) || (started & ~1)) return LEAF_ERR_BAD_SHAPE;
    const int T = hist_len + Tc;
    if (T > kSmallRing * LS) return LEAF_ERR_BAD_SHAPE;                   // one pass of the ring
    if (drop_samples < 0 || drop_samples > T || T - drop_samples > L.H) return LEAF_ERR_BAD_SHAPE;
    if (!stream_frames_ok(first, n, T, hop)) return LEAF_ERR_BAD_SHAPE;
    if (n > 0 && fft_small_lds_bytes(kSmallWaves, n) > (size_t)kMaxLds) return LEAF_ERR_BAD_SHAPE;
    if (state_bytes < L.total) return LEAF_ERR_WORKSPACE;
    if (n == 0 && T - drop_samples == 0) return LEAF_OK;                  // nothing to emit and no history to keep
    const int mode = (use_pcen ? 1 : 0) | ((flags & LEAF_FLAG_LOG1P) && !use_pcen ? 2 : 0) | (out_bf16 ? 4 : 0);
    const CallCtx ctx = forward_ctx(LEAF_ALGO_AUTO);          // this entry takes no option word
    return stream_step(ctx, LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream},
                       StreamIo{chunk, chunk_stride, state, pcm ? kSamplePcm16 : kSampleF32, hist_len, parity, drop_samples, first, n, started, mode, out});
}

// ---- the bank (leaf_fft_stream.hpp): B independent streams, every slot at its own position, kBankSlots slots per launch
// One slot's position as the kernel takes it: one pass record, or two for a stream that ends on a chunk that completes frames.
static int bank_records(const leaf_stream_slot& sl, int K, int hop, int n_max, StreamPassRec* rec) {
    auto pack = [](int lo, int hi) { return (unsigned)lo | ((unsigned)hi << 16); };
    const unsigned bits = (unsigned)sl.started | ((unsigned)sl.parity << 1);
    if (sl.idle) {
        *rec = StreamPassRec{{0, 0, 0, 0, pack(0, n_max), 4u | 8u}};
        return 1;
    }
    const int T = sl.hist_len + sl.Tc, two = sl.end_n > 0;
    int c_lo = 0, nb = 0;
    if (sl.n > 0) stream_blocks(sl.first, sl.n, T, K, hop, c_lo, nb);
    // the step; one that is followed by the ending pass hands nothing over and leaves the row's zeros to that pass
    rec[0] = StreamPassRec{{pack(sl.hist_len, sl.Tc), pack(two ? T : sl.drop_samples, sl.first), (unsigned)sl.n | ((unsigned)c_lo << 16) | ((unsigned)nb << 24),
                            0, pack(0, two ? sl.n : n_max), bits | (two ? 0u : 8u)}};
    if (!two) return 1;
    // the ending pass: the samples [drop, T) as a buffer of their own, nothing kept
    const int d = sl.drop_samples, T2 = T - d, hl2 = std::max(sl.hist_len - d, 0);
    stream_blocks(sl.end_first, sl.end_n, T2, K, hop, c_lo, nb);
    rec[1] = StreamPassRec{{pack(hl2, T2 - hl2), pack(T2, sl.end_first), (unsigned)sl.end_n | ((unsigned)c_lo << 16) | ((unsigned)nb << 24),
                            pack(std::min(d, sl.hist_len), std::max(d - sl.hist_len, 0)), pack(sl.n, n_max),
                            ((unsigned)(sl.started | (sl.n > 0))) | ((unsigned)sl.parity << 1) | 8u}};
    return 2;
}

int leaf_stream_bank_step_f32(const void* chunk, long long chunk_stride, int B, const leaf_stream_slot* slots, int n_max, void* state,
                              size_t state_bytes, const float* kernel, const float* pool_w, const float* pool_b, const float* alpha,
                              const float* delta, const float* root, const float* ema_w, int F, int K, int hop, int flags, void* out,
                              void* stream) {
    if (flags & (LEAF_FLAG_IO_BF16 | LEAF_FLAG_PEAKNORM)) return LEAF_ERR_UNSUPPORTED;
    if (K >= 1 && hop >= 1 && !stream_geometry(K, hop)) return LEAF_ERR_UNSUPPORTED;
    if (B == 0 && !inst_layouts_ok()) return LEAF_ERR_LAUNCH;
    if (B == 0 && n_max >= 0 && F >= 1 && K >= 1 && hop >= 1) return LEAF_OK;
    const bool use_pcen = (flags & LEAF_FLAG_PCEN) != 0;
    if (!slots || !state || !kernel || !pool_w || !pool_b || (n_max > 0 && !out)) return LEAF_ERR_NULL_POINTER;
    if (use_pcen && (!alpha || !delta || !root || !ema_w)) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || F < 1 || F > 65535 || K < 1 || hop < 1 || n_max < 0) return LEAF_ERR_BAD_SHAPE;
    int Tc_max = 0;
    for (int b = 0; b < B; ++b) {
        if (slots[b].idle & ~1) return LEAF_ERR_BAD_SHAPE;
        if (!slots[b].idle && slots[b].Tc < 0) return LEAF_ERR_BAD_SHAPE;
        if (!slots[b].idle) Tc_max = std::max(Tc_max, slots[b].Tc);
    }
    if (Tc_max > 0 && !chunk) return LEAF_ERR_NULL_POINTER;
    if (Tc_max > 0 && B > 1 && chunk_stride < Tc_max) return LEAF_ERR_BAD_SHAPE;
    if (!inst_layouts_ok()) return LEAF_ERR_LAUNCH;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0, out_bf16 = (flags & LEAF_FLAG_OUT_BF16) != 0;
    if (misaligned16(state) || (reinterpret_cast<uintptr_t>(chunk) & (pcm ? 1u : 3u)) || (reinterpret_cast<uintptr_t>(out) & (out_bf16 ? 1u : 3u)) ||
        any_misaligned(kernel, pool_w, pool_b, alpha, delta, root, ema_w))
        return LEAF_ERR_ALIGNMENT;
    // the positions: everything the kernel derives an address in `state`, `chunk` or `out` from, slot by slot
    const StreamLayout L = stream_layout(B, F, K, hop, pcm);
    const int LS = fft_block_len(K, hop, true), padL = K / 2 + K % 2 - 1;
    if (n_max > 0 && fft_small_lds_bytes(kSmallWaves, n_max) > (size_t)kMaxLds) return LEAF_ERR_BAD_SHAPE;
    bool work = n_max > 0;
    for (int b = 0; b < B; ++b) {
        const leaf_stream_slot& sl = slots[b];
        if (sl.idle) continue;
        if (sl.hist_len < 0 || sl.hist_len > L.H || sl.Tc > kSmallRing * LS || (sl.parity & ~1) || (sl.started & ~1)) return LEAF_ERR_BAD_SHAPE;
        const int T = sl.hist_len + sl.Tc;
        if (T > kSmallRing * LS) return LEAF_ERR_BAD_SHAPE;               // one pass of the ring
        if (sl.drop_samples < 0 || sl.drop_samples > T) return LEAF_ERR_BAD_SHAPE;
        if (sl.end_n < 0 || (sl.end_n == 0 && T - sl.drop_samples > L.H)) return LEAF_ERR_BAD_SHAPE;   // (an ending pass keeps nothing)
        if (!stream_frames_ok(sl.first, sl.n, T, hop)) return LEAF_ERR_BAD_SHAPE;
        if (sl.end_n > 0 && !stream_frames_ok(sl.end_first, sl.end_n, T - sl.drop_samples, hop)) return LEAF_ERR_BAD_SHAPE;
        if (sl.n > n_max || sl.end_n > n_max - sl.n) return LEAF_ERR_BAD_SHAPE;
        work = work || T - sl.drop_samples > 0;
    }
    if (state_bytes < L.total) return LEAF_ERR_WORKSPACE;
    if (!work) return LEAF_OK;                                            // no slot emits anything or keeps anything
    const StreamBankKernel kfn = leaf_inst_fft_stream_bank(K);
    if (!kfn) return LEAF_ERR_UNSUPPORTED;
    const int mode = (use_pcen ? 1 : 0) | ((flags & LEAF_FLAG_LOG1P) && !use_pcen ? 2 : 0) | (out_bf16 ? 4 : 0);
    char* base = static_cast<char*>(state);
    StreamBankParams q{};
    q.c.chunk = chunk; q.c.chunk_stride = chunk_stride; q.c.pcm = pcm ? kSamplePcm16 : kSampleF32;
    q.c.hist_in = base; q.c.hist_out = base + L.half;                     // halves 0 and 1: a slot's parity picks the one it reads
    q.c.ema_state = reinterpret_cast<float*>(base + L.ema);
    q.c.kernel = kernel; q.c.pool_w = pool_w; q.c.bd = gabor_bounds(K);
    q.c.B = B; q.c.F = F; q.c.H = L.H;
    q.c.fin = FinParams{nullptr, F, n_max, SlotGeom{LS, padL, K, hop, 0, 2}, pool_b, alpha, delta, root, ema_w, 1e-12f, mode, out, nullptr, nullptr};
    q.n_max = n_max;
    // launches of up to kBankSlots slots and kBankSlots pass records (a slot's records stay together)
    for (int b0 = 0; b0 < B;) {
        int ns = 0, nr = 0, n_lds = 0;
        bool keep = false;
        while (b0 + ns < B && ns < kBankSlots && nr + (slots[b0 + ns].idle || slots[b0 + ns].end_n == 0 ? 1 : 2) <= kBankSlots) {
            const leaf_stream_slot& sl = slots[b0 + ns];
            if (ns % 4 == 0) q.first[ns / 4] = 0;
            q.first[ns / 4] |= (unsigned)nr << (8 * (ns % 4));
            nr += bank_records(sl, K, hop, n_max, q.rec + nr);
            if (!sl.idle) {
                n_lds = std::max(n_lds, std::max(sl.n, sl.end_n));
                keep = keep || sl.hist_len + sl.Tc - sl.drop_samples > 0;
            }
            ++ns;
        }
        q.b0 = b0; q.n_lds = n_lds;
        if (n_max > 0 || keep) {                                          // (n_max = 0: a launch whose slots keep nothing has nothing to do)
            const int rc = launch_lds(kfn, dim3(n_max > 0 ? F : 1, ns), kSmallWaves, n_lds > 0 ? fft_small_lds_bytes(kSmallWaves, n_lds) : 0, (hipStream_t)stream, q);
            if (rc != LEAF_OK) return rc;
        }
        b0 += ns;
    }
    return LEAF_OK;
}

// LEAF_ALGO_FFT_WG on 4096-sample blocks: tables -> workgroup kernel -> the same finalize kernel (partials keep their layout)
static int forward_4k(const CallCtx& ctx, const Fft4kPlan& f4, const LeafArgs& a, const FwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    float* tab = ws;
    float* Grow = tab + align_up(f4.tab_floats, 64);
    float* part = Grow + align_up(f4.grow_floats, 64);
    record(io.ev, 0, a.st);
    float2* Wt = reinterpret_cast<float2*>(Grow + (size_t)F * 2 * f4.RG);
    // band-limited filter tasks (leaf_band.hpp): the static instance runs the filters whose spectrum sits in a 512-bin window
    // of the 4096-point spectrum four to a task on 512-point transforms (decided per call by the prep kernel from the
    // spectrum it has just built; tables by fft4k_band_tab_kernel); LEAF_ALGO_FULL_TRANSFORMS switches them off
    BandParams band{};
    BandTabArgs ba{};
    size_t band_lds = 0;
    if (!f4.generic && f4.band_floats && !ctx.band_off && band_env() != 0 && f4.lds + band_lds_bytes(F) <= (size_t)kMaxLds &&
        band_edges(T, K, hop, f4.L, f4.padL, band, ba.e)) {
        const Band4kLayout bl = band4k_layout(F, K, hop);
        float* bt = part + align_up(f4.part_floats, 64);
        wire_band(ba, band, BandTabs{reinterpret_cast<int*>(bt + bl.rec), bt + bl.gz, nullptr, bt + bl.edge, nullptr, reinterpret_cast<int*>(bt + bl.elist)},
                  a.s, f4.L, f4.padL, ctx.band_strict, /*bwd_slabs=*/0, a.pool_b, ctx.band_strict ? 1.0f : 2.0f);
        ba.force = band_env() > 0 ? band_env() : 0;           // (tools: 2 = every filter)
        band_lds = band_lds_bytes(F);
    }
    hipLaunchKernelGGL(fft4k_prep_kernel, dim3(F), dim3(kPrepWaves * 64), 0, a.st, a.kernel, a.pool_w, F, K, gabor_bounds(K), tab,
                       Grow, f4.RG, Wt, ba);
    LEAF_LAUNCH_CHECK();
    if (band.rec) hipLaunchKernelGGL(fft4k_band_tab_kernel, dim3(F, 1 + band.n_edge), dim3(kPrepWaves * 64), 0, a.st, a.pool_w, F, K, ba);
    LEAF_LAUNCH_CHECK();
    record(io.ev, 1, a.st);
    FftParams q{};
    q.x = io.x; q.io_bf16 = io.xtype; q.H = reinterpret_cast<const float2*>(tab); q.Gz = Grow; q.part = part;
    q.B = B; q.T = T; q.TP = f4.TP; q.F = F; q.K = K; q.hop = hop; q.padL = f4.padL; q.L = f4.L; q.nblk = f4.nblk;
    q.nslot = f4.nslot; q.GZ = f4.RG; q.NT = f4.generic ? fft_wgg4k_frame_floats(K, hop) : 0;
    q.mix_perm = ctx.mix.perm; q.mix_lam = ctx.mix.lam;
    q.lone = reinterpret_cast<const float*>(Wt);                  // (static 32 kHz kernel: the shared twiddle table travels in `lone`)
    if (band.rec) {
        q.band = band;
        q.band.lds_off = (int)(f4.lds / 4);
    }
    // blocks dealt contiguously; a workgroup finalizes the clips it ran every block of in its tail (as fft_forward)
    const int grid = cu_grid(B * f4.nblk, ctx.cus);
    const FinParams fin = fwd_fin_params(a, io, part, f4.TP, SlotGeom{f4.L, f4.padL, K, hop, T, f4.nslot});
    OwnedClips own{};
    if (!fin_fused_off()) {
        own = OwnedClips{B * f4.nblk, grid, f4.nblk};
        q.fin = fin;
        q.fin_fused = 1;
    }
    const int rc = launch_lds(f4.generic ? pick_fft_wgg4k_kernel(K) : leaf_inst_fft_wg4k(), dim3(grid), f4.nw, f4.lds + band_lds, a.st, q);
    if (rc != LEAF_OK) return rc;
    record(io.ev, 2, a.st);
    if (fin_fused_off() || !all_clips_owned(own)) launch_fft_finalize(fin, B, own, ctx.cus, a.st);
    LEAF_LAUNCH_CHECK();
    record(io.ev, 3, a.st);
    return LEAF_OK;
}

// the tables of the MFMA kernels inside the workspace (forward: behind each other from its start)
struct FusedTabs { float* W; float* G; int *perm, *col_of, *tile_ks; };
static inline FusedTabs fused_tabs(const FusedPlan& pl, float* W, float* G, int* meta) { return {W, G, meta, meta + pl.FP, meta + 2 * pl.FP}; }
static inline void launch_fused_finalize(const FusedPlan& pl, const LeafArgs& a, const float* part, const int* col_of, int mode, void* out, float* pooled_raw) {
    hipLaunchKernelGGL(finalize_kernel, dim3(a.s.B, ceil_div(a.s.F, kFinGroup)), dim3(kFinGroup * 64), (size_t)kFinGroup * (kFinStride + 3) * 4, a.st, part, a.s.F, pl.FP, pl.TP, pl.noff,
                       pl.q_lo, pl.q_hi, SlotGeom{}, col_of, a.pool_b, a.alpha, a.delta, a.root, a.ema_w, 1e-12f, mode, out, pooled_raw);
}

// LEAF_ALGO_MFMA: tables -> the direct-form kernel over the filter groups -> finalize
static int forward_mfma(const CallCtx& ctx, const FusedPlan& pl, const LeafArgs& a, const FwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    float* G = ws + align_up(pl.w_floats, 64);
    const FusedTabs t = fused_tabs(pl, ws, G, reinterpret_cast<int*>(G + align_up(pl.g_floats, 64)));
    float* part = G + align_up(pl.g_floats, 64) + align_up(pl.meta_ints, 64);
    record(io.ev, 0, a.st);
    hipLaunchKernelGGL(fused_prep_kernel, dim3(ceil_div(pl.R * 2 * pl.FP + pl.FP * pl.GJ, 256)), dim3(256), 0, a.st,
                       a.kernel, a.pool_w, F, pl.FP, K, pl.R, pl.GJ, gabor_bounds(K), t.W, t.G, (float*)nullptr, t.perm, t.col_of,
                       t.tile_ks);
    LEAF_LAUNCH_CHECK();
    record(io.ev, 1, a.st);
    FusedParams prm = base_fused_params(pl, a.s, ctx.desync);
    prm.x = io.x; prm.io_bf16 = io.xtype; prm.W = t.W; prm.G = t.G; prm.tile_ks = t.tile_ks; prm.part = part;
#if LEAF_TRACE
    prm.trace = reinterpret_cast<unsigned long long*>(part + align_up(pl.part_floats, 64));
#endif
    if (launch_fused_groups(prm, pl, ctx.cus, a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
    record(io.ev, 2, a.st);
    launch_fused_finalize(pl, a, part, t.col_of, io.mode, io.out, io.pooled_raw);
    LEAF_LAUNCH_CHECK();
    record(io.ev, 3, a.st);
    return LEAF_OK;
}

// LEAF_ALGO_STAGED: every intermediate of the reference graph is materialised in the workspace
static int forward_staged(const LeafArgs& a, const FwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    if (2 * F > 65535 || B > 65535) return LEAF_ERR_BAD_SHAPE;
    const int TP = (T - 1) / hop + 1;
    float* outf32 = static_cast<float*>(io.out);
    float* taps = ws;
    float* g = taps + align_up((size_t)2 * F * K, 64);
    float* y = g + align_up((size_t)F * K, 64);
    float* e = y + align_up((size_t)B * 2 * F * T, 64);
    float* pooled = e + align_up((size_t)B * F * T, 64);
    int rc = leaf_gabor_conv_f32(static_cast<const float*>(io.x), B, T, a.kernel, F, K, y, taps, (size_t)2 * F * K * 4, a.st);
    if (rc != LEAF_OK) return rc;
    rc = leaf_squared_modulus_f32(y, B, F, T, e, a.st);
    if (rc != LEAF_OK) return rc;
    rc = leaf_gaussian_lowpass_f32(e, B, F, T, a.pool_w, a.pool_b, K, hop, pooled, g, (size_t)F * K * 4, a.st);
    if (rc != LEAF_OK) return rc;
    const size_t n = (size_t)B * F * TP;
    if (io.pooled_raw && hipMemcpyAsync(io.pooled_raw, pooled, n * 4, hipMemcpyDeviceToDevice, a.st) != hipSuccess)
        return LEAF_ERR_LAUNCH;
    if (io.mode & 1) {
        // floor in place, then PCEN
        hipLaunchKernelGGL(floor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a.st, pooled, n, 0, pooled);
        LEAF_LAUNCH_CHECK();
        return leaf_pcen_f32(pooled, B, F, TP, a.alpha, a.delta, a.root, a.ema_w, 1e-12f, outf32, a.st);
    }
    hipLaunchKernelGGL(floor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a.st, pooled, n, io.mode, outf32);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

// checks in the order the ABI documents, then one function per path
static int forward_impl(const void* x, const LeafArgs& a, int flags, CallCtx ctx, void* out, void* workspace, size_t workspace_bytes,
                        hipEvent_t* ev, float* pooled_raw = nullptr, TableCache tc = TableCache{nullptr, 0}) {
    const auto [B, T, F, K, hop] = a.s;
    const bool out_bf16 = feat_bf16(flags);                                           // what the finalize sites store out as
    const int xtype = x_sample_type(flags);                                           // what the kernels read x as: the two types are independent
    const bool fused_only = xtype != kSampleF32 || out_bf16;                          // 16-bit input and bfloat16 features are fused-path features
    // the selector, the flag combination and the build's layout check hold for the empty batch too (a bad selector or a
    // mismatched build must not go unnoticed on an empty shard): only then (0, F, T') -- nothing to compute, nothing launched
    if (!valid_selector(ctx.sel)) return LEAF_ERR_BAD_ALGO;
    if ((flags & LEAF_FLAG_X_PCM16) && (flags & LEAF_FLAG_IO_BF16)) return LEAF_ERR_UNSUPPORTED;   // two types for x (int16 in, bfloat16 out: LEAF_FLAG_OUT_BF16)
    if (fused_only && ctx.sel == LEAF_ALGO_STAGED) return LEAF_ERR_UNSUPPORTED;
    if (B == 0 && !inst_layouts_ok()) return LEAF_ERR_LAUNCH;
    if (empty_batch(B, T, F, K, hop)) return LEAF_OK;
    if (!x || !a.kernel || !a.pool_w || !a.pool_b || !out) return LEAF_ERR_NULL_POINTER;
    const bool use_pcen = (flags & LEAF_FLAG_PCEN) != 0;
    if (use_pcen && (!a.alpha || !a.delta || !a.root || !a.ema_w)) return LEAF_ERR_NULL_POINTER;
    const int rc = check_shape(B, T, F, K, hop);
    if (rc != LEAF_OK) return rc;
    {
        const uintptr_t out_mask = out_bf16 ? 1u : 3u;                                               // bfloat16 features: 2-byte elements
        const uintptr_t x_mask = (flags & (LEAF_FLAG_X_PCM16 | LEAF_FLAG_IO_BF16)) ? 1u : 3u;        // 16-bit PCM / bfloat16 waveform
        if ((reinterpret_cast<uintptr_t>(x) & x_mask) || (reinterpret_cast<uintptr_t>(out) & out_mask) || misaligned16(workspace) ||
            misaligned16(tc.p) || any_misaligned(a.kernel, a.pool_w, a.pool_b, a.alpha, a.delta, a.root, a.ema_w, pooled_raw))
            return LEAF_ERR_ALIGNMENT;
    }
    const FusedPlan pl = make_plan(a.s, ctx.cus);
    if (ctx.sel == LEAF_ALGO_MFMA && !pl.ok) return LEAF_ERR_BAD_ALGO;
    ctx.sel = resolve_selector(ctx.sel, a.s, ctx.cus);
    if (fused_only && ctx.sel == LEAF_ALGO_STAGED) return LEAF_ERR_UNSUPPORTED;       // (what AUTO resolved to)
    // a PCM sample means v / 32768, so no clip's peak exceeds 1: peak normalisation is the identity (no pre-pass, every scale 1)
    if (xtype == kSamplePcm16) flags &= ~LEAF_FLAG_PEAKNORM;
    const size_t need = forward_workspace_bytes(a.s, ctx.sel, ctx.cus);
    if (!workspace || workspace_bytes < need) return LEAF_ERR_WORKSPACE;
    float* ws = static_cast<float*>(workspace);
    const bool overlap_save = ctx.sel == LEAF_ALGO_FFT || ctx.sel == LEAF_ALGO_FFT_WG || ctx.sel == LEAF_ALGO_FFT_SMALL;
    // The table cache serves the kernels of the 2048-sample plan (workgroup -- static and run-time geometry -- and per wave); every
    // other plan, a mixed call and a peak-normalised call take the route of leaf_forward_f32 and leave the cache untouched.
    unsigned* stamps = nullptr;
    if (tc.p && !ctx.no_table_cache && !ctx.mix.lam && !(flags & LEAF_FLAG_PEAKNORM) && !ev && !pooled_raw &&
        (ctx.sel == LEAF_ALGO_FFT || (ctx.sel == LEAF_ALGO_FFT_WG && !make_fft4k_plan(a.s).ok))) {
        const FftPlan fp = make_fft_plan(a.s, ctx.cus);
        if (fp.ok) {
            if (tc.bytes < table_cache_floats(fp, a.s) * 4) return LEAF_ERR_WORKSPACE;
            stamps = table_cache_stamps(fp, tc.p, a.s);
        }
    }
    // LEAF_FLAG_PEAKNORM: per-clip scales into the tail of the workspace (the last align_up(B, 64) floats the overlap-save
    // plans reserve), applied to the pooled energies by the finalize step
    float* clip_scale2 = nullptr;
    if (flags & LEAF_FLAG_PEAKNORM) {
        if (!overlap_save) return LEAF_ERR_UNSUPPORTED;
        clip_scale2 = ws + need / 4 - align_up((size_t)B, 64);
        hipLaunchKernelGGL(peak_scale2_kernel, dim3(B), dim3(1024), 0, a.st, x, xtype, T, clip_scale2);
        LEAF_LAUNCH_CHECK();
    }
    const int mode = (use_pcen ? 1 : 0) | ((flags & LEAF_FLAG_LOG1P) && !use_pcen ? 2 : 0) | (out_bf16 ? 4 : 0);
    const FwdIo io{x, xtype, mode, out, pooled_raw, clip_scale2, ev};
    if (ctx.mix.lam && !overlap_save) return LEAF_ERR_BAD_ALGO;                       // (MFMA and staged kernels do not mix in their loads)
    switch (ctx.sel) {
        case LEAF_ALGO_FFT_SMALL: return forward_small(ctx, a, io, ws);
        case LEAF_ALGO_FFT_WG: {
            const Fft4kPlan f4 = make_fft4k_plan(a.s);
            if (f4.ok) return forward_4k(ctx, f4, a, io, ws);
        }
            [[fallthrough]];                                   // the 2048-sample workgroup kernels
        case LEAF_ALGO_FFT: {
            const FftPlan fp = make_fft_plan(a.s, ctx.cus);
            if (!fp.ok) return LEAF_ERR_BAD_ALGO;
            // [spectra | pooling rows | col_of | band tables], then the partials
            return fft_forward(ctx, fp, a, io, stamps ? tc.p : ws, ws + fft_table_floats(fp, F), /*tables_ready=*/false,
                               ctx.sel == LEAF_ALGO_FFT_WG, nullptr, stamps);
        }
        case LEAF_ALGO_MFMA: return forward_mfma(ctx, pl, a, io, ws);
        default: return forward_staged(a, io, ws);
    }
}

int leaf_forward_f32(const float* x, int B, int T, const float* kernel, const float* pool_w, const float* pool_b,
                     const float* alpha, const float* delta, const float* root, const float* ema_w, int F, int K, int hop,
                     int flags, int algo, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_impl(x, LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream}, flags,
                        forward_ctx(algo), out, workspace, workspace_bytes, nullptr);
}

size_t leaf_table_cache_bytes(int F, int K, int hop, int T) {
    if (check_shape(1, T, F, K, hop) != LEAF_OK) return 0;
    const Shape s{1, T, F, K, hop};
    const FftPlan fp = make_fft_plan(s, device_cus());       // (the tables' sizes do not depend on the batch)
    return fp.ok ? table_cache_floats(fp, s) * 4 : 0;
}

int leaf_forward_cached_f32(const float* x, int B, int T, const float* kernel, const float* pool_w, const float* pool_b,
                            const float* alpha, const float* delta, const float* root, const float* ema_w, int F, int K, int hop,
                            int flags, int algo, float* out, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                            void* stream) {
    return forward_impl(x, LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream}, flags,
                        forward_ctx(algo), out, workspace, workspace_bytes, nullptr, nullptr, TableCache{static_cast<float*>(cache), cache_bytes});
}

int leaf_forward_save_f32(const float* x, int B, int T, const float* kernel, const float* pool_w, const float* pool_b,
                          const float* alpha, const float* delta, const float* root, const float* ema_w, int F, int K, int hop,
                          int flags, int algo, float* out, float* pooled_raw, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (!pooled_raw) return LEAF_ERR_NULL_POINTER;
    // forward-only: pooled_raw would be that of the normalised clips while leaf_backward_f32 differentiates against x
    // (16-bit PCM: normalisation is the identity, so the flag is accepted and changes nothing)
    if ((flags & LEAF_FLAG_PEAKNORM) && !(flags & LEAF_FLAG_X_PCM16)) return LEAF_ERR_UNSUPPORTED;
    return forward_impl(x, LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream}, flags,
                        forward_ctx(algo), out, workspace, workspace_bytes, nullptr, pooled_raw);
}

// ---- waveform mixup (leaf_common.hpp: mix_load): x'[b] = x[b] lam[b] + x[perm[b]] (1 - lam[b]), defined in fp32 with separately
// rounded operations.  The static-geometry and 4096-sample overlap-save families mix in their loads; every other family reads a mixed
// fp32 copy that mixup_kernel writes behind the family's own workspace.
static int launch_mixup(const void* x, int xtype, int B, int T, const int* perm, const float* lam, float* out, hipStream_t st) {
    const int tiles = ceil_div(T, 1024);
    if ((long long)B * tiles >= (1ll << 31)) return LEAF_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(mixup_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, st, x, xtype, B, T, tiles, perm, lam, out);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}
// does the forward kernel behind the RESOLVED selector mix in its loads?
static bool mix_fused_forward(const Shape& s, int sel, int cus) {
    if (sel == LEAF_ALGO_FFT_SMALL) return true;
    if (sel == LEAF_ALGO_FFT) return pick_fft_kernel_mix(make_fft_plan(s, cus), s.K, s.hop, false) != nullptr;   // per-wave: static odd windows
    if (sel != LEAF_ALGO_FFT_WG) return false;                            // MFMA, staged: the mixed copy
    if (make_fft4k_plan(s).ok) return true;                               // 4096-sample blocks, static and run-time geometry
    return fft_wg_static_exists(s.K, s.hop) && !wg_force_generic();   // 2048-sample blocks: the static instances
}
static size_t mix_copy_offset_floats(size_t base_bytes) { return align_up((base_bytes + 3) / 4, 64); }
// workspace of the mixed forward behind a RESOLVED selector: the family's own, and the mixed copy where the family needs one
static size_t forward_mix_workspace_bytes(const Shape& s, int sel, int cus) {
    const size_t base = forward_workspace_bytes(s, sel, cus);
    if (!base || mix_fused_forward(s, sel, cus)) return base;
    return (mix_copy_offset_floats(base) + align_up((size_t)s.B * s.T, 64)) * 4;
}

int leaf_mixup_f32(const void* x, int B, int T, const int* mix_perm, const float* mix_lam, int flags, float* out, void* stream) {
    if (flags & ~LEAF_FLAG_X_PCM16) return LEAF_ERR_UNSUPPORTED;          // fp32 or 16-bit PCM in, fp32 out
    if (B == 0 && T >= 1) return LEAF_OK;
    if (!x || !mix_perm || !mix_lam || !out) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || T < 1 || (long long)B * T >= (1ll << 31)) return LEAF_ERR_BAD_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x) & ((flags & LEAF_FLAG_X_PCM16) ? 1u : 3u)) || any_misaligned(mix_perm, mix_lam, out))
        return LEAF_ERR_ALIGNMENT;
    return launch_mixup(x, x_sample_type(flags), B, T, mix_perm, mix_lam, out, (hipStream_t)stream);
}

size_t leaf_forward_mix_workspace_bytes(int B, int T, int F, int K, int hop, int algo) {
    if (check_shape(B, T, F, K, hop) != LEAF_OK) return 0;
    const CallCtx ctx = forward_ctx(algo);
    const Shape s{B, T, F, K, hop};
    const int sel = resolve_selector(ctx.sel, s, ctx.cus);
    return sel < 0 ? 0 : forward_mix_workspace_bytes(s, sel, ctx.cus);
}

static int forward_mix_impl(const void* x, MixArgs mix, const LeafArgs& a, int flags, int algo, void* out, float* pooled_raw,
                            void* workspace, size_t workspace_bytes) {
    const auto [B, T, F, K, hop] = a.s;
    // a bfloat16 waveform is not mixed (the definition is fp32; bfloat16 FEATURES, LEAF_FLAG_OUT_BF16, pass through); peak normalisation would have to follow the mix, which the fused loads cannot do
    if (flags & (LEAF_FLAG_IO_BF16 | LEAF_FLAG_PEAKNORM)) return LEAF_ERR_UNSUPPORTED;
    CallCtx ctx = forward_ctx(algo);
    if (empty_batch(B, T, F, K, hop))                        // selector and layout checks as without the mix; nothing is read
        return forward_impl(x, a, flags & ~LEAF_FLAG_X_PCM16, ctx, out, workspace, workspace_bytes, nullptr, pooled_raw);
    if (!x || !mix.perm || !mix.lam) return LEAF_ERR_NULL_POINTER;
    const int rc = check_shape(B, T, F, K, hop);
    if (rc != LEAF_OK) return rc;
    if (any_misaligned(mix.perm, mix.lam)) return LEAF_ERR_ALIGNMENT;
    ctx.sel = resolve_selector(ctx.sel, a.s, ctx.cus);
    if (ctx.sel < 0) return ctx.sel;
    // bfloat16 features have no staged forward (as in forward_impl): answered here, before the workspace check and the mixed copy
    if ((flags & LEAF_FLAG_OUT_BF16) && ctx.sel == LEAF_ALGO_STAGED) return LEAF_ERR_UNSUPPORTED;
    if (mix_fused_forward(a.s, ctx.sel, ctx.cus)) {
        ctx.mix = mix;
        return forward_impl(x, a, flags, ctx, out, workspace, workspace_bytes, nullptr, pooled_raw);
    }
    // the mixed fp32 copy behind the family's own workspace, then the unmixed call on it
    const size_t base = forward_workspace_bytes(a.s, ctx.sel, ctx.cus);
    if (!base) return LEAF_ERR_BAD_ALGO;
    if (reinterpret_cast<uintptr_t>(x) & ((flags & LEAF_FLAG_X_PCM16) ? 1u : 3u) || misaligned16(workspace)) return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < forward_mix_workspace_bytes(a.s, ctx.sel, ctx.cus)) return LEAF_ERR_WORKSPACE;
    float* mixed = static_cast<float*>(workspace) + mix_copy_offset_floats(base);
    const int mrc = launch_mixup(x, x_sample_type(flags), B, T, mix.perm, mix.lam, mixed, a.st);
    if (mrc != LEAF_OK) return mrc;
    return forward_impl(mixed, a, flags & ~LEAF_FLAG_X_PCM16, ctx, out, workspace, base, nullptr, pooled_raw);
}

int leaf_forward_mix_f32(const void* x, const int* mix_perm, const float* mix_lam, int B, int T, const float* kernel,
                         const float* pool_w, const float* pool_b, const float* alpha, const float* delta, const float* root,
                         const float* ema_w, int F, int K, int hop, int flags, int algo, float* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return forward_mix_impl(x, MixArgs{mix_perm, mix_lam}, LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream},
                            flags, algo, out, nullptr, workspace, workspace_bytes);
}

int leaf_forward_save_mix_f32(const void* x, const int* mix_perm, const float* mix_lam, int B, int T, const float* kernel,
                              const float* pool_w, const float* pool_b, const float* alpha, const float* delta, const float* root,
                              const float* ema_w, int F, int K, int hop, int flags, int algo, float* out, float* pooled_raw,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!pooled_raw) return LEAF_ERR_NULL_POINTER;
    return forward_mix_impl(x, MixArgs{mix_perm, mix_lam}, LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream},
                            flags, algo, out, pooled_raw, workspace, workspace_bytes);
}

int leaf_forward_profiled_f32(const float* x, int B, int T, const float* kernel, const float* pool_w, const float* pool_b,
                              const float* alpha, const float* delta, const float* root, const float* ema_w, int F, int K,
                              int hop, int flags, int algo, float* out, void* workspace, size_t workspace_bytes,
                              void* stream, float* stage_ms) {
    if (!stage_ms) return LEAF_ERR_NULL_POINTER;
    if (empty_batch(B, T, F, K, hop)) { stage_ms[0] = stage_ms[1] = stage_ms[2] = 0.f; return LEAF_OK; }
    hipEvent_t ev[4];
    for (int i = 0; i < 4; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) return LEAF_ERR_LAUNCH;
    const LeafArgs a{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream};
    CallCtx ctx = forward_ctx(algo);
    ctx.sel = resolve_selector(ctx.sel, a.s, ctx.cus);       // the fused paths only: the staged forward has no stages to time
    int rc = ctx.sel < 0 || ctx.sel == LEAF_ALGO_STAGED ? LEAF_ERR_BAD_ALGO
                                                        : forward_impl(x, a, flags, ctx, out, workspace, workspace_bytes, ev);
    if (rc == LEAF_OK) {
        if (hipEventSynchronize(ev[3]) != hipSuccess) rc = LEAF_ERR_LAUNCH;
        for (int i = 0; i < 3 && rc == LEAF_OK; ++i)
            if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = LEAF_ERR_LAUNCH;
    }
    for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ev[i]);
    return rc;
}


// ---- inference with frozen parameters: parameter-derived tables prepared once, reused by every forward
size_t leaf_fft_tables_bytes(int F, int K, int hop) {
    if (F < 1 || K < 1 || hop < 1) return 0;
    const FftPlan fp = make_fft_plan(Shape{1, std::max(K, 2 * kFftN), F, K, hop}, device_cus());      // table sizes depend on (F, K) only
    return fp.ok ? fft_table_floats(fp, F, false) * 4 : 0;
}

int leaf_fft_prepare_tables_f32(const float* kernel, const float* pool_w, int F, int K, int hop, void* tables,
                                size_t tables_bytes, void* stream) {
    if (!kernel || !pool_w || !tables) return LEAF_ERR_NULL_POINTER;
    const size_t need = leaf_fft_tables_bytes(F, K, hop);
    if (need == 0) return LEAF_ERR_BAD_ALGO;
    if (misaligned16(tables) || any_misaligned(kernel, pool_w)) return LEAF_ERR_ALIGNMENT;
    if (tables_bytes < need) return LEAF_ERR_WORKSPACE;
    const FftPlan fp = make_fft_plan(Shape{1, std::max(K, 2 * kFftN), F, K, hop}, device_cus());
    float* t = static_cast<float*>(tables);
    const FftTabPtrs tp = fft_tab_ptrs(fp, t, F);
    const BandLayout bl = band_layout(F, K, hop);
    if (bl.stat) {
        // + the parameter-only tables of the band-limited filter tasks (per-filter records, decimated pooling windows)
        BandTabArgs ba{};
        ba.hop = hop; ba.padL = fp.padL; ba.L = fp.L; ba.eps2 = kBandEps2; ba.eta = kBandEtaFree; ba.cross = 1;   // (the forward's default rule)
        ba.rec = reinterpret_cast<int*>(tp.band + bl.rec); ba.gz = tp.band + bl.gz;
        hipLaunchKernelGGL(fft_prep_band_kernel, dim3(F, 2), dim3(kPrepWaves * 64), 0, (hipStream_t)stream, kernel, pool_w, F, K, fp.GZ,
                           gabor_bounds(K), tp.H, tp.Gz, tp.col_of, ba);
    } else {
        hipLaunchKernelGGL(fft_prep_kernel, dim3(F, 1), dim3(kPrepWaves * 64), 0, (hipStream_t)stream, kernel, pool_w, F, K, fp.GZ,
                           gabor_bounds(K), 1, tp.H, tp.Gz, tp.col_of, fft_lone_taps(t, F, K), (unsigned*)nullptr, hop, 0);
    }
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_band_classes_f32(const float* kernel, const float* pool_w, const float* pool_b, int F, int K, int hop, int* classes,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!kernel || !pool_w || !classes) return LEAF_ERR_NULL_POINTER;
    if (F < 1 || K < 1 || hop < 1) return LEAF_ERR_BAD_SHAPE;
    {
        // the 4096-sample plan (K = 801 / hop = 320): one class, decided by fft4k_prep_kernel; classes[f] = 512 or 4096
        const Fft4kPlan f4 = make_fft4k_plan(Shape{1, 2 * kFft4N, F, K, hop});
        if (f4.ok && !f4.generic && f4.band_floats) {
            if (misaligned16(workspace) || any_misaligned(kernel, pool_w, pool_b, classes)) return LEAF_ERR_ALIGNMENT;
            if (!workspace || workspace_bytes < fft4k_workspace_floats(f4, 1) * 4) return LEAF_ERR_WORKSPACE;
            float* tab = static_cast<float*>(workspace);
            float* Grow = tab + align_up(f4.tab_floats, 64);
            float* bt = Grow + align_up(f4.grow_floats, 64) + align_up(f4.part_floats, 64);
            const Band4kLayout b4 = band4k_layout(F, K, hop);
            BandTabArgs ba{};
            ba.hop = hop; ba.padL = f4.padL; ba.L = f4.L; ba.eps2 = kBandEps2; ba.eta = pool_b ? kBandEtaFree : kBandEta;   // (pool_b = NULL: round 5's decision)
            ba.rec = reinterpret_cast<int*>(bt + b4.rec); ba.gz = bt + b4.gz; ba.classes = classes;
            ba.cls_bias = pool_b;
            hipLaunchKernelGGL(fft4k_prep_kernel, dim3(F), dim3(kPrepWaves * 64), 0, (hipStream_t)stream, kernel, pool_w, F, K, gabor_bounds(K),
                               tab, Grow, f4.RG, (float2*)nullptr, ba);
            LEAF_LAUNCH_CHECK();
            return LEAF_OK;
        }
    }
    const BandLayout bl = band_layout(F, K, hop);
    if (!bl.stat) return LEAF_ERR_UNSUPPORTED;               // no band tasks for this geometry: every filter on full transforms
    const size_t need = leaf_fft_tables_bytes(F, K, hop);
    if (misaligned16(workspace) || any_misaligned(kernel, pool_w, pool_b, classes)) return LEAF_ERR_ALIGNMENT;
    if (!workspace || need == 0 || workspace_bytes < need) return LEAF_ERR_WORKSPACE;
    const FftPlan fp = make_fft_plan(Shape{1, std::max(K, 2 * kFftN), F, K, hop}, device_cus());
    float* t = static_cast<float*>(workspace);
    const FftTabPtrs tp = fft_tab_ptrs(fp, t, F);
    BandTabArgs ba{};
    ba.hop = hop; ba.padL = fp.padL; ba.L = fp.L; ba.eps2 = kBandEps2; ba.eta = pool_b ? kBandEtaFree : kBandEta; ba.cross = pool_b ? 1 : 0;   // (pool_b = NULL: round 5's decision)
    ba.rec = reinterpret_cast<int*>(tp.band + bl.rec); ba.gz = tp.band + bl.gz; ba.classes = classes;
    ba.cls_bias = pool_b;
    hipLaunchKernelGGL(fft_prep_band_kernel, dim3(F, 2), dim3(kPrepWaves * 64), 0, (hipStream_t)stream, kernel, pool_w, F, K, fp.GZ,
                       gabor_bounds(K), tp.H, tp.Gz, tp.col_of, ba);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

int leaf_forward_prepared_f32(const float* x, int B, int T, const void* tables, size_t tables_bytes, const float* pool_b,
                              const float* alpha, const float* delta, const float* root, const float* ema_w, int F, int K,
                              int hop, int flags, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if ((flags & LEAF_FLAG_X_PCM16) && (flags & LEAF_FLAG_IO_BF16)) return LEAF_ERR_UNSUPPORTED;
    // no scale pre-pass on the prepared-tables path (16-bit PCM needs none: every clip's scale is 1)
    if ((flags & LEAF_FLAG_PEAKNORM) && !(flags & LEAF_FLAG_X_PCM16)) return LEAF_ERR_UNSUPPORTED;
    if (empty_batch(B, T, F, K, hop)) return LEAF_OK;
    if (!x || !tables || !pool_b || !out) return LEAF_ERR_NULL_POINTER;
    const bool use_pcen = (flags & LEAF_FLAG_PCEN) != 0;
    if (use_pcen && (!alpha || !delta || !root || !ema_w)) return LEAF_ERR_NULL_POINTER;
    int rc = check_shape(B, T, F, K, hop);
    if (rc != LEAF_OK) return rc;
    const CallCtx ctx = forward_ctx(LEAF_ALGO_AUTO);          // this entry takes no option word: the defaults, every CU
    const LeafArgs a{{B, T, F, K, hop}, nullptr, nullptr, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream};
    const FftPlan fp = make_fft_plan(a.s, ctx.cus);
    if (!fp.ok) return LEAF_ERR_BAD_ALGO;
    if (tables_bytes < leaf_fft_tables_bytes(F, K, hop)) return LEAF_ERR_WORKSPACE;
    const bool out_bf16 = feat_bf16(flags);
    const uintptr_t out_mask = out_bf16 ? 1u : 3u;
    const uintptr_t x_mask = (flags & (LEAF_FLAG_X_PCM16 | LEAF_FLAG_IO_BF16)) ? 1u : 3u;
    if ((reinterpret_cast<uintptr_t>(x) & x_mask) || (reinterpret_cast<uintptr_t>(out) & out_mask) || misaligned16(workspace) ||
        misaligned16(tables) || any_misaligned(pool_b, alpha, delta, root, ema_w))
        return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < (align_up(fp.part_floats, 64) + (LEAF_TRACE ? 16 * 64 * 2 : 0)) * 4) return LEAF_ERR_WORKSPACE;
    const int mode = (use_pcen ? 1 : 0) | ((flags & LEAF_FLAG_LOG1P) && !use_pcen ? 2 : 0) | (out_bf16 ? 4 : 0);
    // the edge tables of the band-limited filter tasks (they depend on the clip length) go behind the partial sums when the
    // workspace has the room (it has when sized by leaf_workspace_bytes as documented); otherwise full transforms
    const size_t part_end = align_up(fp.part_floats, 64) + (LEAF_TRACE ? 16 * 64 * 2 : 0);
    float* band_scratch = fp.band_dyn && workspace_bytes >= (part_end + fp.band_dyn) * 4 ? static_cast<float*>(workspace) + part_end : nullptr;
    return fft_forward(ctx, fp, a, FwdIo{x, x_sample_type(flags), mode, out, nullptr, nullptr, nullptr},
                       static_cast<float*>(const_cast<void*>(tables)), static_cast<float*>(workspace), /*tables_ready=*/true,
                       auto_algo(a.s, ctx.cus, /*allow_small=*/false) == LEAF_ALGO_FFT_WG,   // the workgroup kernel from the batch AUTO takes it at
                       band_scratch);
}

// ---- overlap-save backward: which geometries it covers, and its workspace layout (float offsets)
inline bool fft_backward_ok(const FftPlan& fp, int K, int hop) {
    return fp.ok && (K >= 224 || fft_static_geometry(K, hop));
}

struct FftBwdLayout {
    size_t R3, lone, Gz, col_of, part, raw, ema, gpre, rowsum, grow, dkpart, dwpart, dxblk, total;
    // band tasks of the static backward (leaf_band_bwd.hpp): records | G~ | G~2 | edge | edge2 | edge list; 0 floats where they do not apply
    size_t brec, bgz, bgz2, bedge, bedge2, belist;
};

// ---- workgroup-per-block backward (leaf_fft_wg_bwd.hpp): the static odd-window geometries; the only fused path that
// also yields dL/dx
struct FftWgBwdLaunch {
    FftKernel fn;
    int nw;
    size_t lds;
    bool block_dx;            // dL/dx from the workgroup-per-block kernel (G per block in LDS): grid over blocks, one plane per block
};
// blocks from which dL/dx comes from the workgroup-per-block kernels (G shared in LDS) rather than a block per wave: the
// thresholds of the parameter-gradient kernels
static bool wg_block_dx_enabled() {
    static const bool off = [] { const char* e = tools_env("LEAF_WG_BWD_DX"); return e && atoi(e) == 0; }();   // tools only: A/B
    return !off;
}
// blocks per CU (in sixteenths) from which the static 401 / 160 backward takes the workgroup kernel, whose narrow-band filters run as
// band tasks (leaf_band_bwd.hpp).  With dL/dx: always (profiles/r05/ab_band_dx.txt: 0.084 vs 0.087 ms at one clip, 0.085 vs 0.136 ms
// at 24); parameter gradients only: from 6/16 (0.063 ms flat from 1 to 24 clips against 0.041 / 0.060 / 0.104 / 0.124 ms of the
// per-wave kernel at 4 / 8 / 16 / 24 clips).  The thresholds assume that the default filters' classes hold (the decision itself is taken
// on the device, per call): a filterbank without narrow-band filters runs full tasks here below the 20/16 its own crossing was measured at.
#ifndef LEAF_WG_BWD_DX_BAND_SIXTEENTHS
#define LEAF_WG_BWD_DX_BAND_SIXTEENTHS 0       // blocks per CU (sixteenths) from which the static 401 / 160 backward WITH dL/dx takes the workgroup kernel (band tasks); 20: as without them
#endif
#ifndef LEAF_WG_BWD_BAND_SIXTEENTHS
#define LEAF_WG_BWD_BAND_SIXTEENTHS 6          // the same for the parameter gradients alone (below: the per-wave kernel); 20: as without band tasks
#endif
#ifndef LEAF_WG4K_BWD_BAND_SIXTEENTHS
#define LEAF_WG4K_BWD_BAND_SIXTEENTHS 8        // the same for the static 801 / 320 parameter-gradient backward on 4096-sample blocks (below: the 2048-sample kernels)
#endif
// the lowered thresholds hold only where band tasks CAN run in this call -- not with LEAF_FLAG_BWD_FULL_TRANSFORMS, more
// than kBandMaxFilters filters or clips whose edge frames band_edges() cannot table; backward_fft says so (`band_possible`) when it picks
// its kernels (the workspace layout does not depend on the pick), and such calls keep the 20/16 crossing measured without band tasks.
inline int wg_bwd_sixteenths(int K, int hop, bool dx, bool band_possible) {
    if (!band_geometry_ok(K, hop) || !band_possible) return 20;
    return dx ? LEAF_WG_BWD_DX_BAND_SIXTEENTHS : LEAF_WG_BWD_BAND_SIXTEENTHS;
}
FftWgBwdLaunch pick_fft_wg_bwd_kernel(int K, int hop, bool dx, int cus, bool band_possible, long long blocks = 0, bool io_bf16 = false) {
    if (dx) {
        if (!(fft_static_geometry(K, hop) && (K & 1))) return {nullptr, 0, 0};
        // (not K = 801: there the block-per-wave kernel measures 5 % faster, 1.89 vs 1.99 ms at 256 x 1 s)
        if (wg_block_dx_enabled() && K != 801 && blocks >= fft_wg_bwd_min_blocks(cus, wg_bwd_sixteenths(K, hop, true, band_possible)) &&
            fft_wg_bwd_dx_lds_bytes(12, K) <= (size_t)kMaxLds)
            return {leaf_inst_fft_wg_bwd_dx(K), 12, fft_wg_bwd_dx_lds_bytes(12, K), true};
        // below that: one wave per block, G in registers (leaf_fft_blk_bwd_dx_kernel)
        return {(io_bf16 ? leaf_inst_fft_blk_bwd_dx_bf16(K) : leaf_inst_fft_blk_bwd_dx(K)), kBlkBwdWaves, fft_blk_bwd_lds_bytes(K)};
    }
    if (fft_static_geometry(K, hop) && (K & 1)) return {leaf_inst_fft_wg_bwd(K), 12, fft_wg_bwd_lds_bytes(12, K)};
    return {nullptr, 0, 0};
}
// any other window of the 2048-sample plan, odd or even: the run-time-geometry kernel (leaf_fft_wgg_bwd.hpp); parameter
// gradients only
FftWgBwdLaunch pick_fft_wgg_bwd_kernel(const FftPlan& fp, int K, int hop) {
    (void)hop;
    if (!fp.ok || K < 64 || K > 64 * 19) return {nullptr, 0, 0};
    static const int full_min = [] { const char* e = tools_env("LEAF_WGG_FULL"); return e ? atoi(e) : 11; }();   // as the forward's
    const int ni = fft_wgg_taps_per_lane(K);
    if (full_min > 0 && ni <= 10) {
        int nwf = 12;
        while (nwf > full_min && fft_wgg_lds_bytes_full(nwf, K) > (size_t)kMaxLds) --nwf;
        if (fft_wgg_lds_bytes_full(nwf, K) <= (size_t)kMaxLds)
            return {leaf_inst_fft_wgg_bwd(ni, false), nwf, fft_wgg_lds_bytes_full(nwf, K)};
    }
    int nw = 12;                                                          // the forward's row layout with the half-size scratch
    while (nw > 6 && fft_wgg_lds_bytes(nw, K) > (size_t)kMaxLds) --nw;
    if (fft_wgg_lds_bytes(nw, K) > (size_t)kMaxLds) return {nullptr, 0, 0};
    const FftWgLaunch fwd{nullptr, nw, fft_wgg_lds_bytes(nw, K)};
    return {leaf_inst_fft_wgg_bwd(ni, true), fwd.nw, fwd.lds};
}
static_assert(fft_wg_bwd_lds_bytes(12, 801) <= (size_t)kMaxLds && fft_blk_bwd_lds_bytes(801) <= (size_t)kMaxLds, "LDS budget");
// used for dL/dx always (nothing else fused yields it), and for the parameter gradients once every CU gets a block
bool fft_wg_bwd_use(const FftPlan& fp, int B, int K, int hop, bool need_dx, int cus, bool band_possible) {
    return fp.ok && pick_fft_wg_bwd_kernel(K, hop, need_dx, cus, band_possible).fn != nullptr &&
           (need_dx || (long long)B * fp.nblk >= fft_wg_bwd_min_blocks(cus, wg_bwd_sixteenths(K, hop, false, band_possible)));
}
// dL/dx for the other windows of the 2048-sample plan, odd or even, at every batch: the workgroup-per-block kernel with the
// block's G shared in LDS (leaf_fft_wgg_bwd_kernel<.., DX = true>), twelve-wave structure and dynamic filter queue.  (A
// block-per-wave run-time-geometry kernel served fewer than 10/16 block per CU until round 4; measured equal or slower there
// -- profiles/r04/dx_small_batches.txt -- and it carried 264..408 B of scratch per lane, so it is gone.)
FftWgBwdLaunch pick_fft_wgg_bwd_dx_kernel(const FftPlan& fp, int K, int hop, int cus) {
    static const bool off = [] { const char* e = tools_env("LEAF_WGG_BWD_DX"); return e && atoi(e) == 0; }();   // tools only: A/B
    if (off || !fp.ok || K < 64 || K > 64 * 19 || pick_fft_wg_bwd_kernel(K, hop, true, cus, /*band_possible=*/true).fn) return {nullptr, 0, 0};   // (only whether a static instance exists)
    int nw = 12;
    while (nw > 6 && fft_wgg_bwd_dx_lds_bytes(nw, K) > (size_t)kMaxLds) --nw;
    const size_t lds = fft_wgg_bwd_dx_lds_bytes(nw, K);
    if (lds > (size_t)kMaxLds) return {nullptr, 0, 0};
    return {leaf_inst_fft_wgg_bwd_dx(fft_wgg_taps_per_lane(K)), nw, lds};
}
// the run-time-geometry kernel: parameter gradients, once every CU gets a block
bool fft_wgg_bwd_use(const FftPlan& fp, int B, int K, int hop, bool need_dx, int cus) {
    static const bool off = [] { const char* e = tools_env("LEAF_WGG_BWD"); return e && atoi(e) == 0; }();   // tools only: A/B
    return !off && !need_dx && fp.ok && !pick_fft_wg_bwd_kernel(K, hop, false, cus, /*band_possible=*/true).fn && pick_fft_wgg_bwd_kernel(fp, K, hop).fn &&
           (long long)B * fp.nblk >= fft_wg_bwd_min_blocks(cus, 10);
}

FftBwdLayout fft_bwd_layout(const FftPlan& fp, int B, int F, bool need_dx) {
    FftBwdLayout L{};
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += align_up(n, 64); return at; };
    L.R3 = take((size_t)3 * F * kFftN);
    L.lone = take((size_t)3 * F * 2);                                     // even K: the unpaired tap and its mu / sigma derivatives
    L.Gz = take(fp.gz_floats);
    L.col_of = take((size_t)F);
    L.part = take(fp.part_floats);
    L.raw = take((size_t)B * F * fp.TP);
    L.ema = take((size_t)B * F * fp.TP);
    L.gpre = take((size_t)B * F * fp.TP);
    L.rowsum = take((size_t)B * F * 4);
    L.grow = take((size_t)B * F);                                         // sum_m g_pre per (clip, filter) row
    L.dkpart = take((size_t)B * fp.nblk * F * 2);
    L.dwpart = take((size_t)B * fp.nblk * F);
    L.dxblk = take(need_dx ? (size_t)B * fp.nblk * fp.nfq * kFftN : 0);    // per-(block, filter group) input gradients (the
                                                                        // workgroup-per-block kernels use one plane per block)
    if (fp.band_stat) {
        constexpr int K = 401;                                            // (band tasks exist for the 401 / 160 geometry only)
        L.brec = take((size_t)4 * F);
        L.bgz = take((size_t)F * band_gz_floats(K, 160));
        L.bgz2 = take((size_t)F * band_gz_floats(K, 160));
        L.bedge = take((size_t)F * 2 * kBandMaxEdge * 512);
        L.bedge2 = take((size_t)F * 2 * kBandMaxEdge * 512);
        L.belist = take((size_t)4 * kBandMaxEdge);
    }
    L.total = o;
    return L;
}

// ---- overlap-save backward on 4096-sample blocks (leaf_fft_wgg4k_bwd.hpp): odd windows 833..2049, parameter gradients,
// once every CU gets a block; run-time geometry
struct Fft4kBwdPlan {
    bool ok;
    bool stat;             // the static K = 801 / hop = 320 instance (register-gather pooling backward); false: run-time geometry
    bool dx;               // ... with dL/dx (static instance only): nine waves, the block's gradient spectra in LDS
    int L, nblk, TP, padL, RG, nw;
    size_t lds;
};
FftKernel pick_fft_wgg4k_bwd_kernel(int K) { return leaf_inst_fft_wgg4k_bwd(fft_wgg4k_taps_per_lane(K)); }
Fft4kBwdPlan make_fft4k_bwd_plan(const Shape& s, bool need_dx, int cus) {
    const auto [B, T, F, K, hop] = s;
    Fft4kBwdPlan bp{};
    static const bool off = [] { const char* e = tools_env("LEAF_4K_BWD"); return e && atoi(e) == 0; }();   // tools only: A/B
    static const int min_k = [] { const char* e = tools_env("LEAF_4K_BWD_MIN_K"); return e ? atoi(e) : 833; }();   // tools only
    // tools only: LEAF_4K_BWD_STATIC=0 keeps the 32 kHz geometry on the static 2048-sample kernel (A/B)
    static const bool stat_off = [] { const char* e = tools_env("LEAF_4K_BWD_STATIC"); return e && atoi(e) == 0; }();
    const bool stat = K == 801 && hop == 320 && !stat_off;
    // run-time geometry from K = 833; at K = 801 it measures slower than the static 2048-sample kernel (2.25 vs 2.09 ms)
    // dL/dx on 4096-sample blocks: the static instance only (tools: LEAF_4K_BWD_DX=0 keeps it on 2048-sample blocks, A/B)
    static const bool dx_off = [] { const char* e = tools_env("LEAF_4K_BWD_DX"); return e && atoi(e) == 0; }();
    if (off || fft4k_disabled() || (need_dx && (!stat || dx_off)) || !(K & 1) || (!stat && K < min_k) || K > 2049 || F > 65535)
        return bp;
    bp.stat = stat;
    bp.dx = need_dx;
    bp.padL = K / 2;
    bp.TP = (T - 1) / hop + 1;
    bp.L = stat ? 3200 : (kFft4N - K + 1) & ~1;                         // static: a multiple of the hop (the forward's plan)
    if ((bp.L + K - 2) / hop + 2 > 64) return bp;                        // g_pre of a block's frames: one per lane
    bp.nblk = ceil_div(T, bp.L);
    if ((long long)B * bp.nblk >= (1ll << 30) || (long long)B * bp.nblk < fft_wg_bwd_min_blocks(cus, stat && !need_dx ? LEAF_WG4K_BWD_BAND_SIXTEENTHS : 8)) return bp;
    if (stat) {
        bp.RG = kWg4RowFloats;
        bp.nw = need_dx ? kWg4BwdDxWaves : LEAF_4K_BWD_NW;
        bp.lds = need_dx ? fft_wg4k_bwd_dx_lds_bytes(kWg4BwdDxWaves) : fft_wg4k_lds_bytes(LEAF_4K_BWD_NW);   // dx: half scratch; else the forward's
        bp.ok = true;
        return bp;
    }
    bp.RG = fft_wgg4k_row_floats(K);
    bp.nw = 12;
    while (bp.nw > 6 && fft_wgg4k_lds_bytes(bp.nw, K, 0) > (size_t)kMaxLds) --bp.nw;     // no frame-sum array in the backward
    bp.lds = fft_wgg4k_lds_bytes(bp.nw, K, 0);
    bp.ok = bp.lds <= (size_t)kMaxLds;
    return bp;
}
struct Fft4kBwdLayout {
    size_t tab3, grow, part, raw, ema, gpre, rowsum, gsrow, dkpart, dwpart, col_of, dxblk, total;
    size_t brec, bgz, bgz2, bedge, bedge2, belist;   // band tasks of the static 32 kHz backward (leaf_band_bwd.hpp); 0 where they do not apply
};
Fft4kBwdLayout fft4k_bwd_layout(const Fft4kBwdPlan& bp, int B, int F) {
    Fft4kBwdLayout L{};
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += align_up(n, 64); return at; };
    L.tab3 = take((size_t)3 * F * kFft4TabFloats);
    L.grow = take((size_t)F * 2 * bp.RG + kFft4WtFloats);                // + the shared twiddle table of the static forward kernel
    L.part = take((size_t)B * bp.TP * 2 * F);
    L.raw = take((size_t)B * F * bp.TP);
    L.ema = take((size_t)B * F * bp.TP);
    L.gpre = take((size_t)B * F * bp.TP);
    L.rowsum = take((size_t)B * F * 4);
    L.gsrow = take((size_t)B * F);                                        // sum_m g_pre per (clip, filter) row
    L.dkpart = take((size_t)B * bp.nblk * F * 2);
    L.dwpart = take((size_t)B * bp.nblk * F);
    L.col_of = take((size_t)F);
    L.dxblk = take(bp.dx ? (size_t)B * bp.nblk * kFft4N : 0);            // per-block input gradients, 4096 samples each
    if (bp.stat && F <= kBandMaxFilters) {                              // (with dL/dx unused: the two layouts differ by dxblk only)
        L.brec = take((size_t)4 * F);
        L.bgz = take((size_t)F * band4k_gz_floats(801, 320));
        L.bgz2 = take((size_t)F * band4k_gz_floats(801, 320));
        L.bedge = take((size_t)F * kBandMaxEdge * 512);
        L.bedge2 = take((size_t)F * kBandMaxEdge * 512);
        L.belist = take((size_t)4 * kBandMaxEdge);
    }
    L.total = o;
    return L;
}

// Which backward implementation serves a call (the same decision sizes the workspace and dispatches the kernels).
enum BwdPath { BWD_PATH_FFT = 0, BWD_PATH_MFMA = 1, BWD_PATH_STAGED = 2, BWD_PATH_FFT4K = 3 };
static BwdPath bwd_path(const Shape& s, int flags, bool need_dx, int cus) {
    if (!(flags & (LEAF_FLAG_BWD_STAGED | LEAF_FLAG_BWD_MFMA))) {
        if (make_fft4k_bwd_plan(s, need_dx, cus).ok) return BWD_PATH_FFT4K;
        const FftPlan fp = make_fft_plan(s, cus);
        if (fft_backward_ok(fp, s.K, s.hop) &&
            (!need_dx || fft_wg_bwd_use(fp, s.B, s.K, s.hop, true, cus, /*band_possible=*/true) ||   // (sizing: with dL/dx the answer does not depend on it)
             pick_fft_wgg_bwd_dx_kernel(fp, s.K, s.hop, cus).fn))
            return BWD_PATH_FFT;
    }
    if (!need_dx && !(flags & LEAF_FLAG_BWD_STAGED)) {
        const FusedPlan pl = make_plan(s, cus);
        if (make_bwd_plan(pl, s.T).ok) return BWD_PATH_MFMA;
    }
    return BWD_PATH_STAGED;
}
static size_t bwd_own_workspace_floats(BwdPath path, const Shape& s, bool need_dx, int cus) {
    const auto [B, T, F, K, hop] = s;
    switch (path) {
        case BWD_PATH_FFT: return fft_bwd_layout(make_fft_plan(s, cus), B, F, need_dx).total;
        case BWD_PATH_FFT4K: return fft4k_bwd_layout(make_fft4k_bwd_plan(s, need_dx, cus), B, F).total;
        case BWD_PATH_MFMA: {
            const FusedPlan pl = make_plan(s, cus);
            return bwd_layout(pl, make_bwd_plan(pl, T), B, T, F, cus).total;
        }
        default: break;
    }
    const int TP = (T - 1) / hop + 1;
    return align_up((size_t)2 * F * K, 64) * 2 /* taps, dtaps unused slot */ + align_up((size_t)F * K, 64) * 2 +
           align_up((size_t)B * 2 * F * T, 64) + align_up((size_t)B * F * T, 64) +
           align_up((size_t)B * F * TP, 64) * 3 + align_up((size_t)B * F * 4, 64) +
           align_up((size_t)B * 2 * F * K, 64);
}

// LEAF_FLAG_IO_BF16 / LEAF_FLAG_X_PCM16 (a 16-bit waveform): the static-geometry overlap-save backwards (K = 401 / 160, 801 / 320, 201 / 80) and the 4096-sample plans read
// the 16-bit waveform directly (nothing added); the run-time-geometry kernels of the 2048-sample plan, the MFMA and the staged backward
// read fp32 only and get a widened copy of x behind their own layout
static size_t bwd_x32_floats(BwdPath path, const Shape& s, int flags) {
    if (!(flags & (LEAF_FLAG_IO_BF16 | LEAF_FLAG_X_PCM16)) || path == BWD_PATH_FFT4K) return 0;
    if (path == BWD_PATH_FFT && fft_static_geometry(s.K, s.hop) && (s.K & 1)) return 0;
    return align_up((size_t)s.B * s.T, 64);
}

size_t leaf_backward_workspace_bytes(int B, int T, int F, int K, int hop, int flags, int need_dx) {
    if (check_shape(B, T, F, K, hop) != LEAF_OK) return 0;
    const Shape s{B, T, F, K, hop};
    const int cus = backward_ctx(flags, MixArgs{nullptr, nullptr}).cus;
    const BwdPath path = bwd_path(s, flags, need_dx != 0, cus);
    return (bwd_own_workspace_floats(path, s, need_dx != 0, cus) + bwd_x32_floats(path, s, flags)) * 4;
}

// Waveform mixup (leaf_backward_mix_f32).  The 4096-sample backwards and the static odd-window kernels of the 2048-sample plan
// (workgroup-per-block and per-wave, K = 401 / 201 / 801) have MIX instances that mix in their block loads; the run-time-geometry
// 2048-sample kernels (they re-read samples in their time-domain terms), MFMA and staged read a mixed fp32 copy behind the path's own
// layout -- where the widened copy of a 16-bit waveform goes, which a mixed call never needs (mixup_kernel widens).
static size_t bwd_mix_floats(BwdPath path, const Shape& s, int cus) {
    if (path == BWD_PATH_FFT4K || (path == BWD_PATH_FFT && pick_fft_kernel_mix(make_fft_plan(s, cus), s.K, s.hop, true) != nullptr)) return 0;
    return align_up((size_t)s.B * s.T, 64);
}

size_t leaf_backward_mix_workspace_bytes(int B, int T, int F, int K, int hop, int flags) {
    if (check_shape(B, T, F, K, hop) != LEAF_OK) return 0;
    const Shape s{B, T, F, K, hop};
    const int cus = backward_ctx(flags, MixArgs{nullptr, nullptr}).cus;
    const BwdPath path = bwd_path(s, flags, false, cus);
    return (bwd_own_workspace_floats(path, s, false, cus) + bwd_mix_floats(path, s, cus)) * 4;
}

// what a backward path reads and writes besides the parameters
struct BwdIo {
    const float* x;                  // the waveform the kernels read: the caller's, or the mixed / widened fp32 copy
    int xtype;                       // its sample type (leaf_common.hpp kSample*)
    const float* grad_out;
    const float* pooled_raw;         // saved by leaf_forward_save_f32, else NULL: recomputed
    float *g_kernel, *g_pool_w, *g_pool_b, *g_alpha, *g_delta, *g_root, *g_ema_w, *g_x;
    // first-stage mode (pcen_bwd_scan_kernel): bit0 PCEN, bit1 log1p compression (PCEN off only, as in the forward), bit2 bf16 grad_out;
    // param_reduce_kernel reads bit0 alone
    // (grad_out is read by that kernel alone, on every path: a bfloat16 grad_out needs no widened copy anywhere)
    int mode;
    bool gx_bf16;                    // LEAF_FLAG_IO_BF16: g_x is a bfloat16 buffer
};
// floor + PCEN backward per (b,f) row; `col_of` / `gcols`: the MFMA path's column-major copy, `rowsums`: sum_m g_pre per row
static int launch_pcen_bwd_scan(const LeafArgs& a, const BwdIo& io, const float* raw_in, float* ema, float* gpre, float* rowsum,
                                const int* col_of, int FP, float* gcols, float* rowsums) {
    const int B = a.s.B, F = a.s.F, TP = (a.s.T - 1) / a.s.hop + 1;
    hipLaunchKernelGGL(pcen_bwd_scan_kernel, dim3(ceil_div(B * F, 4)), dim3(256), 0, a.st, raw_in, io.grad_out, B * F, F, TP, a.alpha,
                       a.delta, a.root, a.ema_w, 1e-12f, io.mode, ema, gpre, rowsum, col_of, FP, gcols, rowsums);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}
// reductions over blocks and the batch, clamp sub-gradients, of the overlap-save backwards
// (the per-block (d mu, d sigma) partials are summed by param_reduce_kernel too: one launch less)
static int launch_fft_param_reduce(const LeafArgs& a, const BwdIo& io, const float* gpre, const float* rowsum, const float* dwpart,
                                   const float* dkpart, int nblocks, const int* col_of, const float* rowsums) {
    const int B = a.s.B, F = a.s.F, K = a.s.K, TP = (a.s.T - 1) / a.s.hop + 1;
    hipLaunchKernelGGL(param_reduce_kernel, dim3(F), dim3(kParamRedThreads), 0, a.st, gpre, (const float*)nullptr,
                       (const float*)nullptr, rowsum, a.pool_w, B, F, TP, K, io.mode, dwpart, nblocks, F, col_of, io.g_pool_w,
                       io.g_pool_b, io.g_alpha, io.g_delta, io.g_root, io.g_ema_w,
                       dkpart, nblocks, a.kernel, gabor_bounds(K), io.g_kernel, rowsums);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}
// tools only (LEAF_BAND_BWD=0): no band tasks in the backwards (A/B)
static inline bool band_bwd_off() {
    static const bool off = [] { const char* e = tools_env("LEAF_BAND_BWD"); return e && atoi(e) == 0; }();
    return off;
}

// ---- overlap-save backward on 4096-sample blocks: long odd windows, parameter gradients (static 801 / 320: dL/dx too)
static int backward_4k(const CallCtx& ctx, const LeafArgs& a, const BwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    const Fft4kBwdPlan bp = make_fft4k_bwd_plan(a.s, io.g_x != nullptr, ctx.cus);
    const Fft4kBwdLayout L = fft4k_bwd_layout(bp, B, F);
    float* tab3 = ws + L.tab3; float* Grow = ws + L.grow; float* part = ws + L.part; float* raw = ws + L.raw;
    float* gpre = ws + L.gpre; float* rowsum = ws + L.rowsum; int* col_of = reinterpret_cast<int*>(ws + L.col_of);
    // 1. tables: 4096-point real spectra of w, dw/dmu, dw/dsigma (+ the D tables of w) and the de-interleaved pooling rows
    float2* Wt = reinterpret_cast<float2*>(Grow + (size_t)F * 2 * bp.RG);
    // band tasks of the static 32 kHz backward (leaf_band_bwd.hpp): decision by fft4k_prep_kernel's workgroups (f, 0), G~, G~2 and
    // the edge tables by fft4k_band_tab_kernel, from the parameters of this call
    BandParams band{};
    BandTabArgs ba{};
    const bool band_bwd = !band_bwd_off() && !ctx.band_off && bp.stat && !bp.dx && L.bgz2 &&
                          bp.lds + band_lds_bytes(F) <= (size_t)kMaxLds &&
                          band_edges(T, K, hop, bp.L, bp.padL, band, ba.e);
    if (band_bwd)   // (bwd_slabs = 2: the class decision also asks band_deriv_fits, leaf_band.hpp; no extra grid rows in this kernel)
        wire_band(ba, band, BandTabs{reinterpret_cast<int*>(ws + L.brec), ws + L.bgz, ws + L.bgz2, ws + L.bedge, ws + L.bedge2, reinterpret_cast<int*>(ws + L.belist)},
                  a.s, bp.L, bp.padL, ctx.band_strict, /*bwd_slabs=*/2, ctx.band_strict ? nullptr : a.pool_b, ctx.band_strict ? 0.0f : 2.0f);   // the forward's bias-aware class decision (leaf_band.hpp)
    hipLaunchKernelGGL(fft4k_prep_kernel, dim3(F, 3), dim3(kPrepWaves * 64), 0, a.st, a.kernel, a.pool_w, F, K, gabor_bounds(K), tab3,
                       Grow, bp.RG, Wt, ba);
    LEAF_LAUNCH_CHECK();
    if (band_bwd) hipLaunchKernelGGL(fft4k_band_tab_kernel, dim3(F, 1 + band.n_edge), dim3(kPrepWaves * 64), 0, a.st, a.pool_w, F, K, ba);
    LEAF_LAUNCH_CHECK();
    hipLaunchKernelGGL(iota_kernel, dim3(ceil_div(F, 256)), dim3(256), 0, a.st, col_of, F);
    LEAF_LAUNCH_CHECK();
    FftParams q{};
    q.x = io.x; q.io_bf16 = io.xtype; q.H = reinterpret_cast<const float2*>(tab3); q.Gz = Grow; q.part = part;
    q.B = B; q.T = T; q.TP = bp.TP; q.F = F; q.K = K; q.hop = hop; q.padL = bp.padL; q.L = bp.L; q.nblk = bp.nblk;
    q.nslot = 2; q.GZ = bp.RG;
    q.mix_perm = ctx.mix.perm; q.mix_lam = ctx.mix.lam;              // (mixed call: the forward recompute and the MIX backward instance mix in their loads)
    q.lone = reinterpret_cast<const float*>(Wt);                      // (read by the static forward kernel when it recomputes below)
    const dim3 grid(cu_grid(B * bp.nblk, ctx.cus));
    const float* raw_in = io.pooled_raw;
    int rc;
    if (!raw_in) {
        // the forward with its own wave count and LDS (run-time geometry: it parks frame sums between the halves)
        const int fbn = bp.stat ? 0 : fft_wgg4k_frame_floats(K, hop);
        int fnw = bp.stat ? LEAF_4K_FWD_NW : 12;
        while (!bp.stat && fnw > 6 && fft_wgg4k_lds_bytes(fnw, K, fbn) > (size_t)kMaxLds) --fnw;
        const size_t flds = bp.stat ? fft_wg4k_lds_bytes(LEAF_4K_FWD_NW) : fft_wgg4k_lds_bytes(fnw, K, fbn);
        if (flds > (size_t)kMaxLds) return LEAF_ERR_BAD_ALGO;
        q.NT = fbn;
        rc = launch_lds(bp.stat ? leaf_inst_fft_wg4k() : pick_fft_wgg4k_kernel(K), grid, fnw, flds, a.st, q);
        if (rc != LEAF_OK) return rc;
        q.NT = 0;
        finalize_pooled_raw(a, part, SlotGeom{bp.L, bp.padL, K, hop, T, 2}, raw, ctx.cus);
        LEAF_LAUNCH_CHECK();
        raw_in = raw;
    }
    // 2. floor + PCEN backward per (b,f) row
    rc = launch_pcen_bwd_scan(a, io, raw_in, ws + L.ema, gpre, rowsum, nullptr, 0, nullptr, ws + L.gsrow);
    if (rc != LEAF_OK) return rc;
    // 3. per-(block, filter) partial gradients
    q.gpre = gpre; q.pool_w = a.pool_w; q.dkpart = ws + L.dkpart; q.dwpart = ws + L.dwpart; q.part = nullptr;
    const bool mixed = ctx.mix.lam != nullptr;
    FftKernel kb = bp.dx ? leaf_inst_fft_wg4k_bwd_dx()
                         : bp.stat ? (mixed ? leaf_inst_fft_wg4k_bwd_mix() : leaf_inst_fft_wg4k_bwd())
                                   : mixed ? leaf_inst_fft_wgg4k_bwd_mix(fft_wgg4k_taps_per_lane(K)) : pick_fft_wgg4k_bwd_kernel(K);
    if (!kb) return LEAF_ERR_BAD_ALGO;
    if (bp.dx) q.part = ws + L.dxblk;                                 // [block][4096] input gradients, un-rotated
    size_t blds = bp.lds;
    if (band_bwd) {
        band.lds_off = (int)(blds / 4);
        blds += band_lds_bytes(F);
        q.band = band;
    }
    rc = launch_lds(kb, grid, bp.nw, blds, a.st, q);
    if (rc == LEAF_OK && bp.dx) rc = launch_dx_gather(io.gx_bf16, ws + L.dxblk, a.s, bp.nblk, 1, bp.L, bp.padL, io.g_x, kFft4N, a.st);
    if (rc != LEAF_OK) return rc;
    // 4. reductions over blocks and the batch, clamp sub-gradients
    return launch_fft_param_reduce(a, io, gpre, rowsum, ws + L.dwpart, ws + L.dkpart, B * bp.nblk, col_of, ws + L.gsrow);
}

// ---- overlap-save backward on 2048-sample blocks: the windows the FFT forward is chosen for (K >= 224 or a static geometry)
static int backward_fft(const CallCtx& ctx, const LeafArgs& a, const BwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    const bool need_dx = io.g_x != nullptr;
    const FftPlan fp = make_fft_plan(a.s, ctx.cus);
    // the lowered thresholds of wg_bwd_sixteenths hold only where band tasks CAN run in this call
    BandParams band_probe{};
    BandEdge edge_probe[kBandMaxEdge];
    const bool band_possible = fp.ok && !ctx.band_off && (K & 1) && F <= kBandMaxFilters && fp.nslot == 2 &&
                               band_edges(T, K, hop, fp.L, fp.padL, band_probe, edge_probe);
    const FftBwdLayout L = fft_bwd_layout(fp, B, F, need_dx);
    float* R3 = ws + L.R3; float* Gz = ws + L.Gz; int* col_of = reinterpret_cast<int*>(ws + L.col_of);
    float* part = ws + L.part; float* raw = ws + L.raw; float* gpre = ws + L.gpre; float* rowsum = ws + L.rowsum;
    // 1. tables: real spectra of w, dw/dmu, dw/dsigma and the pooling rows -- with the band tasks of the static backward
    // (leaf_band_bwd.hpp: the filters the forward runs on 256- / 512-point transforms get their parameter gradients at the
    // decimated rate too) one launch of fft_prep_band_kernel builds them together with the decision, G~, G~2 and the edge
    // tables, from the parameters of THIS call (the decision the forward took from the same parameters)
    BandParams band{};
    BandTabArgs ba{};
    // (with dL/dx: in the workgroup-per-block kernel, whose band tasks add their members' shares to the block's G)
    const bool use_wg = fft_wg_bwd_use(fp, B, K, hop, need_dx, ctx.cus, band_possible);
    const FftWgBwdLaunch bwl = pick_fft_wg_bwd_kernel(K, hop, need_dx, ctx.cus, band_possible, (long long)B * fp.nblk);
    const bool band_bwd = !band_bwd_off() && !ctx.band_off && L.bgz2 && (K & 1) &&
                          F <= kBandMaxFilters && fp.nslot == 2 && use_wg &&
                          (!need_dx || bwl.block_dx) &&
                          bwl.lds + band_lds_bytes(F) <= (size_t)kMaxLds && band_edges(T, K, hop, fp.L, fp.padL, band, ba.e);
    if (band_bwd) {
        wire_band(ba, band, BandTabs{reinterpret_cast<int*>(ws + L.brec), ws + L.bgz, ws + L.bgz2, ws + L.bedge, ws + L.bedge2, reinterpret_cast<int*>(ws + L.belist)},
                  a.s, fp.L, fp.padL, ctx.band_strict, /*bwd_slabs=*/1, ctx.band_strict ? nullptr : a.pool_b, ctx.band_strict ? 0.0f : 2.0f);   // the forward's bias-aware class decision
        hipLaunchKernelGGL(fft_prep_band_kernel, dim3(F, 2 + band.n_edge + 2), dim3(kPrepWaves * 64), 0, a.st, a.kernel, a.pool_w, F, K, fp.GZ,
                           gabor_bounds(K), reinterpret_cast<float2*>(R3), Gz, col_of, ba);
    } else {
        hipLaunchKernelGGL(fft_prep_kernel, dim3(F, 3), dim3(kPrepWaves * 64), 0, a.st, a.kernel, a.pool_w, F, K, fp.GZ,
                           gabor_bounds(K), 1, reinterpret_cast<float2*>(R3), Gz, col_of, (K & 1) ? (float*)nullptr : ws + L.lone,
                           (unsigned*)nullptr, hop, 0);
    }
    LEAF_LAUNCH_CHECK();
    FftParams q{};
    q.x = io.x; q.io_bf16 = io.xtype; q.H = reinterpret_cast<const float2*>(R3); q.Gz = Gz; q.part = part;
    q.lone = (K & 1) ? nullptr : ws + L.lone;
    fill_fft_params(q, fp, a.s);
    q.mix_perm = ctx.mix.perm; q.mix_lam = ctx.mix.lam;               // (non-NULL only where the MIX instances below exist)
    const bool mixed = ctx.mix.lam != nullptr;
    const dim3 wave_grid(cu_grid(ceil_div(q.total_tasks, kFftWaves), ctx.cus)), block_grid(cu_grid(B * fp.nblk, ctx.cus));
    const float* raw_in = io.pooled_raw;
    int rc;
    if (!raw_in) {
        FftKernel kf = mixed ? pick_fft_kernel_mix(fp, K, hop, false) : pick_fft_kernel(fp, K, hop, false);
        if (!kf) return LEAF_ERR_BAD_ALGO;
        rc = launch_lds(kf, wave_grid, kFftWaves, fp.lds, a.st, q);
        if (rc != LEAF_OK) return rc;
        finalize_pooled_raw(a, part, SlotGeom{fp.L, fp.padL, K, hop, T, fp.nslot}, raw, ctx.cus);
        LEAF_LAUNCH_CHECK();
        raw_in = raw;
    }
    // 2. floor + PCEN backward per (b,f) row
    rc = launch_pcen_bwd_scan(a, io, raw_in, ws + L.ema, gpre, rowsum, nullptr, 0, nullptr, ws + L.grow);
    if (rc != LEAF_OK) return rc;
    // 3. filterbank recompute + transposed pooling + second transform: per-block (d mu, d sigma, d pool_w)
    q.gpre = gpre; q.pool_w = a.pool_w; q.dkpart = ws + L.dkpart; q.dwpart = ws + L.dwpart; q.part = nullptr;
    if (use_wg) {
        // workgroup-per-block backward; with g_x the per-block input gradients go to dxblk and are gathered below
        FftWgBwdLaunch wl = pick_fft_wg_bwd_kernel(K, hop, need_dx, ctx.cus, band_possible, (long long)B * fp.nblk, io.xtype == kSampleBf16);
        q.part = need_dx ? ws + L.dxblk : nullptr;
        if (mixed) wl.fn = leaf_inst_fft_wg_bwd_mix(K);
        if (!wl.fn) return LEAF_ERR_BAD_ALGO;
        if (band_bwd) {
            band.lds_off = (int)(wl.lds / 4);
            wl.lds += band_lds_bytes(F);
            q.band = band;
        }
        // dx kernels: one (block, group) per WAVE, or (block_dx) a workgroup per block like the parameter-gradient kernel
        const int wgs = need_dx && !wl.block_dx ? ceil_div(q.total_tasks, wl.nw) : B * fp.nblk;
        rc = launch_lds(wl.fn, dim3(cu_grid(wgs, ctx.cus)), wl.nw, wl.lds, a.st, q);
        if (rc == LEAF_OK && need_dx)
            rc = launch_dx_gather(io.gx_bf16, ws + L.dxblk, a.s, fp.nblk, wl.block_dx ? 1 : fp.nfq, fp.L, fp.padL, io.g_x, kFftN, a.st);
    } else if (need_dx) {
        // dL/dx on a window without a static instance: workgroup per block, G in LDS
        const FftWgBwdLaunch wl = pick_fft_wgg_bwd_dx_kernel(fp, K, hop, ctx.cus);
        if (!wl.fn) return LEAF_ERR_BAD_ALGO;                         // bwd_path() admits the FFT path only with a dL/dx kernel
        q.part = ws + L.dxblk;                                        // [block][2048]: one plane per block
        rc = launch_lds(wl.fn, block_grid, wl.nw, wl.lds, a.st, q);
        if (rc == LEAF_OK) rc = launch_dx_gather(io.gx_bf16, ws + L.dxblk, a.s, fp.nblk, 1, fp.L, fp.padL, io.g_x, kFftN, a.st);
    } else if (fft_wgg_bwd_use(fp, B, K, hop, need_dx, ctx.cus)) {
        const FftWgBwdLaunch wl = pick_fft_wgg_bwd_kernel(fp, K, hop);
        rc = launch_lds(wl.fn, block_grid, wl.nw, wl.lds, a.st, q);
    } else {
        FftKernel kb = mixed ? pick_fft_kernel_mix(fp, K, hop, true) : pick_fft_kernel(fp, K, hop, true);
        if (!kb) return LEAF_ERR_BAD_ALGO;
        rc = launch_lds(kb, wave_grid, kFftWaves, fp.lds, a.st, q);
    }
    if (rc != LEAF_OK) return rc;
    // 4. reductions over blocks and the batch, clamp sub-gradients
    return launch_fft_param_reduce(a, io, gpre, rowsum, ws + L.dwpart, ws + L.dkpart, B * fp.nblk, col_of, ws + L.grow);
}

// ---- fused backward (MFMA): used whenever the geometry fits and dL/dx is not requested
static int backward_mfma(const CallCtx& ctx, const LeafArgs& a, const BwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    const int cus = ctx.cus, TP = (T - 1) / hop + 1;
    const FusedPlan pl = make_plan(a.s, cus);
    const BwdPlan bp = make_bwd_plan(pl, T);
    const BwdLayout L = bwd_layout(pl, bp, B, T, F, cus);
    const FusedTabs t = fused_tabs(pl, ws + L.W, ws + L.G, reinterpret_cast<int*>(ws + L.meta));
    float* Gs = ws + L.Gs; float* part = ws + L.part; float* raw = ws + L.raw; float* gpre = ws + L.gpre;
    float* gcols = ws + L.gcols; float* rowsum = ws + L.rowsum; float* dwpart = ws + L.dwpart;
    float* dHpart = ws + L.dHpart; float* dY = ws + L.dY;
    const int Rp = 16 * bp.NKT;
    // 1. tables, forward recompute up to the pre-floor pooled value
    hipLaunchKernelGGL(fused_prep_kernel, dim3(ceil_div(pl.R * 2 * pl.FP + pl.FP * pl.GJ, 256)), dim3(256), 0, a.st,
                       a.kernel, a.pool_w, F, pl.FP, K, pl.R, pl.GJ, gabor_bounds(K), t.W, t.G, Gs, t.perm, t.col_of, t.tile_ks);
    LEAF_LAUNCH_CHECK();
    FusedParams prm = base_fused_params(pl, a.s, -1);
    prm.x = io.x; prm.W = t.W; prm.G = t.G; prm.tile_ks = t.tile_ks; prm.part = part;
    const float* raw_in = io.pooled_raw;
    if (!raw_in) {
        if (launch_fused_groups(prm, pl, cus, a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
        launch_fused_finalize(pl, a, part, t.col_of, 8, raw, nullptr);
        LEAF_LAUNCH_CHECK();
        raw_in = raw;
    }
    // 2. floor + PCEN backward per (b,f) row
    if (hipMemsetAsync(gcols, 0, (size_t)B * TP * pl.FP * 4, a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
    int rc = launch_pcen_bwd_scan(a, io, raw_in, ws + L.ema, gpre, rowsum, t.col_of, pl.FP, gcols, nullptr);
    if (rc != LEAF_OK) return rc;
    // 3. filterbank recompute with the backward epilogue: dY (time-major) and d pool_w partials
    if (hipMemsetAsync(dwpart, 0, (size_t)cus * kWavesPerWG * pl.FP * 4, a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
    if (hipMemsetAsync(dHpart, 0, (size_t)cus * Rp * 2 * pl.FP * 4, a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
    prm.Gs = Gs; prm.gcols = gcols; prm.dY = dY; prm.dwpart = dwpart; prm.part = nullptr;
    if (launch_fused_groups(prm, pl, cus, a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
    // 4. tap gradients: dH = S^T dY on the MFMA, then chain to (mu, sigma)
    DtapsParams dp{};
    dp.x = io.x; dp.dY = dY; dp.tile_ks = t.tile_ks; dp.dHpart = dHpart;
    dp.B = B; dp.T = T; dp.FP = pl.FP; dp.K = K; dp.Hf = pl.Hf; dp.xshift = pl.xshift;
    dp.NKT = bp.NKT; dp.NW = bp.NW; dp.NS = bp.NS; dp.HPc = bp.HPc; dp.XSC = bp.XSC; dp.LD = bp.LD;
    dp.nch = bp.nch; dp.total_chunks = B * bp.nch;
    if (pl.groups_main > 0) {
        dp.tile_base = 0;
        const int gx = cu_grid(dp.total_chunks, std::max(1, cus / pl.groups_main));
        if (launch_dtaps(dp, pl.rt_main, bp.TPW, pl.groups_main, bp.lds, gx, a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
    }
    if (pl.rt_rem > 0) {
        dp.tile_base = pl.groups_main * pl.rt_main;
        if (launch_dtaps(dp, pl.rt_rem, bp.TPW, 1, bp.lds, cu_grid(dp.total_chunks, cus), a.st) != hipSuccess) return LEAF_ERR_LAUNCH;
    }
    // slab 0 doubles as the reduction target: reduce slabs 1.. into a scratch slab placed after the last one
    const size_t slab = (size_t)Rp * 2 * pl.FP;
    float* dHsum = dHpart + (size_t)cus * slab;
    hipLaunchKernelGGL(dh_reduce_kernel, dim3((unsigned)((slab + 255) / 256)), dim3(256), 0, a.st, dHpart, cus, slab, dHsum);
    LEAF_LAUNCH_CHECK();
    hipLaunchKernelGGL(dkernel_fused_kernel, dim3(F), dim3(256), 0, a.st, dHsum, 1, Rp, t.W, pl.R, pl.FP, t.col_of,
                       a.kernel, F, gabor_bounds(K), io.g_kernel);
    LEAF_LAUNCH_CHECK();
    // 5. parameter sums over the batch
    hipLaunchKernelGGL(param_reduce_kernel, dim3(F), dim3(kParamRedThreads), 0, a.st, gpre, (const float*)nullptr,
                       (const float*)nullptr, rowsum, a.pool_w, B, F, TP, K, io.mode, dwpart, cus * kWavesPerWG, pl.FP,
                       t.col_of, io.g_pool_w, io.g_pool_b, io.g_alpha, io.g_delta, io.g_root, io.g_ema_w);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

// ---- staged backward: the reference graph's kernels, every intermediate in the workspace; the fallback, and dL/dx for the
// geometries nothing else covers
static int backward_staged(const LeafArgs& a, const BwdIo& io, float* ws) {
    const auto [B, T, F, K, hop] = a.s;
    hipStream_t st = a.st;
    const int TP = (T - 1) / hop + 1;
    const int padL = K / 2 + K % 2 - 1;
    float* taps = ws;                         ws += align_up((size_t)2 * F * K, 64) * 2;
    float* g = ws;                            ws += align_up((size_t)F * K, 64);
    float* dg = ws;                           ws += align_up((size_t)F * K, 64);
    float* y = ws;                            ws += align_up((size_t)B * 2 * F * T, 64);
    float* e = ws;                            ws += align_up((size_t)B * F * T, 64);
    float* raw = ws;                          ws += align_up((size_t)B * F * TP, 64);
    float* ema = ws;                          ws += align_up((size_t)B * F * TP, 64);
    float* gpre = ws;                         ws += align_up((size_t)B * F * TP, 64);
    float* rowsum = ws;                       ws += align_up((size_t)B * F * 4, 64);
    float* tpart = ws;
    // forward recompute (staged kernels = the reference graph)
    int rc = leaf_gabor_conv_f32(io.x, B, T, a.kernel, F, K, y, taps, (size_t)2 * F * K * 4, a.st);
    if (rc != LEAF_OK) return rc;
    rc = leaf_squared_modulus_f32(y, B, F, T, e, a.st);
    if (rc != LEAF_OK) return rc;
    rc = leaf_gaussian_lowpass_f32(e, B, F, T, a.pool_w, a.pool_b, K, hop, raw, g, (size_t)F * K * 4, a.st);
    if (rc != LEAF_OK) return rc;
    // PCEN + floor backward
    hipLaunchKernelGGL(pcen_bwd_scan_kernel, dim3(ceil_div(B * F, 4)), dim3(256), 0, st, raw, io.grad_out, B * F, F, TP, a.alpha,
                       a.delta, a.root, a.ema_w, 1e-12f, io.mode, ema, gpre, rowsum, (const int*)nullptr, 0, (float*)nullptr);
    LEAF_LAUNCH_CHECK();
    // pooling backward: window gradient needs e, sample gradient turns y into dy in place
    hipLaunchKernelGGL(pool_bwd_dg_kernel, dim3(ceil_div(K, 128), F), dim3(128), 0, st, e, gpre, B, F, T, TP, K, hop, padL, dg);
    LEAF_LAUNCH_CHECK();
    hipLaunchKernelGGL(param_reduce_kernel, dim3(F), dim3(kParamRedThreads), 0, st, gpre, dg, g, rowsum, a.pool_w, B, F, TP, K, io.mode,
                       (const float*)nullptr, 0, 0, (const int*)nullptr, io.g_pool_w, io.g_pool_b, io.g_alpha, io.g_delta, io.g_root, io.g_ema_w);
    LEAF_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool_bwd_dy_kernel, dim3(ceil_div(T, 256), F, B), dim3(256), 0, st, y, g, gpre, F, T, TP, K, hop, padL);
    LEAF_LAUNCH_CHECK();
    // filterbank backward
    hipLaunchKernelGGL(dtaps_partial_kernel, dim3(ceil_div(K, 128), 2 * F, B), dim3(128), 0, st, y, io.x, T, 2 * F, K, padL,
                       tpart);
    LEAF_LAUNCH_CHECK();
    hipLaunchKernelGGL(dkernel_kernel, dim3(F), dim3(256), 0, st, tpart, taps, a.kernel, B, F, K, gabor_bounds(K), io.g_kernel);
    LEAF_LAUNCH_CHECK();
    if (io.g_x) {
        hipLaunchKernelGGL(dx_kernel, dim3(ceil_div(T, 256), B), dim3(256), 0, st, y, taps, T, 2 * F, K, padL, io.g_x, io.gx_bf16 ? 1 : 0);
        LEAF_LAUNCH_CHECK();
    }
    return LEAF_OK;
}

// checks in the order the ABI documents, the mixed / widened copy of the waveform where the path's kernels need one, then one
// function per path.  io.x arrives as the caller's buffer; ctx.mix.lam != NULL: the mixed call (leaf_backward_mix_f32 has refused
// bfloat16, PEAKNORM, g_x and a missing buffer)
static int backward_impl(CallCtx ctx, const LeafArgs& a, int flags, BwdIo io, void* workspace, size_t workspace_bytes) {
    const auto [B, T, F, K, hop] = a.s;
    // LEAF_FLAG_IO_BF16: x, grad_out and g_x are bfloat16 buffers behind the float pointers (as in the forward); everything else fp32
    // LEAF_FLAG_X_PCM16: x alone is a 16-bit PCM buffer (v / 32768); an integer input has no gradient, so g_x must be NULL
    // LEAF_FLAG_OUT_BF16: grad_out alone is bfloat16 (the feature side); x and g_x follow the two flags above
    if ((flags & LEAF_FLAG_X_PCM16) && ((flags & LEAF_FLAG_IO_BF16) || io.g_x)) return LEAF_ERR_UNSUPPORTED;
    const bool mixed_call = ctx.mix.lam != nullptr, need_dx = io.g_x != nullptr;
    const bool use_pcen = (flags & LEAF_FLAG_PCEN) != 0;
    if (empty_batch(B, T, F, K, hop)) {
        // the sum over zero clips: every parameter gradient is exactly zero (what autograd returns for the reference)
        if (!io.g_kernel || !io.g_pool_w || !io.g_pool_b) return LEAF_ERR_NULL_POINTER;
        if (use_pcen && (!io.g_alpha || !io.g_delta || !io.g_root || !io.g_ema_w)) return LEAF_ERR_NULL_POINTER;
        bool ok = hipMemsetAsync(io.g_kernel, 0, (size_t)2 * F * 4, a.st) == hipSuccess;
        ok = ok && hipMemsetAsync(io.g_pool_w, 0, (size_t)F * 4, a.st) == hipSuccess;
        ok = ok && hipMemsetAsync(io.g_pool_b, 0, (size_t)F * 4, a.st) == hipSuccess;
        if (use_pcen)
            for (float* g : {io.g_alpha, io.g_delta, io.g_root, io.g_ema_w}) ok = ok && hipMemsetAsync(g, 0, (size_t)F * 4, a.st) == hipSuccess;
        return ok ? LEAF_OK : LEAF_ERR_LAUNCH;
    }
    if (!io.x || !a.kernel || !a.pool_w || !a.pool_b || !io.grad_out || !io.g_kernel || !io.g_pool_w || !io.g_pool_b) return LEAF_ERR_NULL_POINTER;
    if (use_pcen && (!a.alpha || !a.delta || !a.root || !a.ema_w || !io.g_alpha || !io.g_delta || !io.g_root || !io.g_ema_w))
        return LEAF_ERR_NULL_POINTER;
    int rc = check_shape(B, T, F, K, hop);
    if (rc != LEAF_OK) return rc;
    if (2 * F > 65535 || B > 65535) return LEAF_ERR_BAD_SHAPE;
    io.gx_bf16 = (flags & LEAF_FLAG_IO_BF16) != 0;           // the waveform side: x and g_x
    const bool go_bf16 = feat_bf16(flags);                   // the feature side: grad_out
    {
        const uintptr_t io_mask = io.gx_bf16 ? 1u : 3u;
        const uintptr_t x_mask = (flags & LEAF_FLAG_X_PCM16) ? 1u : io_mask;
        if ((reinterpret_cast<uintptr_t>(io.x) & x_mask) || (reinterpret_cast<uintptr_t>(io.grad_out) & (go_bf16 ? 1u : 3u)) ||
            (reinterpret_cast<uintptr_t>(io.g_x) & io_mask) || misaligned16(workspace) ||
            any_misaligned(a.kernel, a.pool_w, a.pool_b, a.alpha, a.delta, a.root, a.ema_w, io.pooled_raw, io.g_kernel, io.g_pool_w, io.g_pool_b,
                           io.g_alpha, io.g_delta, io.g_root, io.g_ema_w) || any_misaligned(ctx.mix.perm, ctx.mix.lam))
            return LEAF_ERR_ALIGNMENT;
    }
    const BwdPath path = bwd_path(a.s, flags, need_dx, ctx.cus);
    const size_t own = bwd_own_workspace_floats(path, a.s, need_dx, ctx.cus);
    const size_t copy = mixed_call ? bwd_mix_floats(path, a.s, ctx.cus) : bwd_x32_floats(path, a.s, flags);
    if (!workspace || workspace_bytes < (own + copy) * 4) return LEAF_ERR_WORKSPACE;
    io.mode = (use_pcen ? 1 : 0) | ((flags & LEAF_FLAG_LOG1P) && !use_pcen ? 2 : 0) | (go_bf16 ? 4 : 0);
    io.xtype = x_sample_type(flags);                         // what the kernels below read x as
    float* ws = static_cast<float*>(workspace);
    if (mixed_call && copy) {
        // this path's kernels do not mix in their loads: the mixed fp32 copy behind the path's own layout, then the unmixed call on it
        rc = launch_mixup(io.x, io.xtype, B, T, ctx.mix.perm, ctx.mix.lam, ws + own, a.st);
        if (rc != LEAF_OK) return rc;
        io.x = ws + own; io.xtype = kSampleF32; ctx.mix = MixArgs{nullptr, nullptr};
    } else if (copy) {
        // these families read fp32: one widening pass into the workspace's tail, then the fp32 path
        const size_t n = (size_t)B * T;
        hipLaunchKernelGGL(x16_widen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a.st,
                           reinterpret_cast<const unsigned short*>(io.x), io.xtype, n, ws + own);
        LEAF_LAUNCH_CHECK();
        io.x = ws + own; io.xtype = kSampleF32;
    }
    switch (path) {
        case BWD_PATH_FFT4K: return backward_4k(ctx, a, io, ws);
        case BWD_PATH_FFT: return backward_fft(ctx, a, io, ws);
        case BWD_PATH_MFMA: return backward_mfma(ctx, a, io, ws);
        default: return backward_staged(a, io, ws);
    }
}

int leaf_backward_f32(const float* x, int B, int T, const float* kernel, const float* pool_w, const float* pool_b,
                      const float* alpha, const float* delta, const float* root, const float* ema_w, int F, int K, int hop,
                      int flags, const float* grad_out, const float* pooled_raw, float* g_kernel, float* g_pool_w,
                      float* g_pool_b, float* g_alpha, float* g_delta, float* g_root, float* g_ema_w, float* g_x,
                      void* workspace, size_t workspace_bytes, void* stream) {
    return backward_impl(backward_ctx(flags, MixArgs{nullptr, nullptr}),
                         LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream}, flags,
                         BwdIo{x, 0, grad_out, pooled_raw, g_kernel, g_pool_w, g_pool_b, g_alpha, g_delta, g_root, g_ema_w, g_x, 0, false},
                         workspace, workspace_bytes);
}

int leaf_backward_mix_f32(const void* x, const int* mix_perm, const float* mix_lam, int B, int T, const float* kernel,
                          const float* pool_w, const float* pool_b, const float* alpha, const float* delta, const float* root,
                          const float* ema_w, int F, int K, int hop, int flags, const float* grad_out, const float* pooled_raw,
                          float* g_kernel, float* g_pool_w, float* g_pool_b, float* g_alpha, float* g_delta, float* g_root,
                          float* g_ema_w, float* g_x, void* workspace, size_t workspace_bytes, void* stream) {
    if (g_x || (flags & (LEAF_FLAG_IO_BF16 | LEAF_FLAG_PEAKNORM))) return LEAF_ERR_UNSUPPORTED;   // dL/dx under mixup is a scatter over perm: not built
    if (B != 0 && (!mix_perm || !mix_lam)) return LEAF_ERR_NULL_POINTER;
    return backward_impl(backward_ctx(flags, MixArgs{mix_perm, mix_lam}),
                         LeafArgs{{B, T, F, K, hop}, kernel, pool_w, pool_b, alpha, delta, root, ema_w, (hipStream_t)stream}, flags,
                         BwdIo{static_cast<const float*>(x), 0, grad_out, pooled_raw, g_kernel, g_pool_w, g_pool_b, g_alpha, g_delta, g_root, g_ema_w, g_x, 0, false},
                         workspace, workspace_bytes);
}

// ---- head-only backward (leaf_head_bwd.hpp): d pool_b and the PCEN gradients from pooled_raw, one memset and one launch ----------
// workspace: [tickets: F words, padded to 16 bytes][records: F S kHeadRecFloats floats][ema: F S kHeadWaves rows of TP floats, only
// for rows beyond the scan's register form]
struct HeadLayout {
    int S, L;
    size_t ticket_bytes, rec_floats, ema_floats;
    size_t bytes() const { return ticket_bytes + (rec_floats + ema_floats) * 4; }
};
static HeadLayout head_layout(int B, int TP, int F, int flags) {
    HeadLayout h{};
    leaf_head_bwd_plan(B, F, device_cus(), &h.S, &h.L);
    h.ticket_bytes = align_up((size_t)F * 4, 16);
    h.rec_floats = (size_t)F * h.S * kHeadRecFloats;
    const bool scan_mem = (flags & LEAF_FLAG_PCEN) && TP > kScanRegChunks * 128;
    h.ema_floats = scan_mem ? (size_t)F * h.S * kHeadWaves * TP : 0;
    return h;
}
constexpr int kHeadFlags = LEAF_FLAG_PCEN | LEAF_FLAG_LOG1P | LEAF_FLAG_IO_BF16 | LEAF_FLAG_OUT_BF16;

size_t leaf_backward_head_workspace_bytes(int B, int TP, int F, int flags) {
    if (B < 1 || TP < 1 || F < 1 || (flags & ~kHeadFlags) || (long long)B * F * TP >= (1ll << 31)) return 0;
    return head_layout(B, TP, F, flags).bytes();
}

int leaf_backward_head_f32(const float* pooled_raw, const float* grad_out, int B, int TP, int F, const float* alpha,
                           const float* delta, const float* root, const float* ema_w, int flags, float* g_pool_b, float* g_alpha,
                           float* g_delta, float* g_root, float* g_ema_w, void* workspace, size_t workspace_bytes, void* stream) {
    if (flags & ~kHeadFlags) return LEAF_ERR_UNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    const bool use_pcen = (flags & LEAF_FLAG_PCEN) != 0;
    if (B == 0 && TP >= 1 && F >= 1) {
        // the sum over zero clips (leaf_backward_f32): zero gradients, nothing launched
        if (!g_pool_b || (use_pcen && (!g_alpha || !g_delta || !g_root || !g_ema_w))) return LEAF_ERR_NULL_POINTER;
        if (!inst_layouts_ok()) return LEAF_ERR_LAUNCH;
        bool ok = hipMemsetAsync(g_pool_b, 0, (size_t)F * 4, st) == hipSuccess;
        if (use_pcen)
            for (float* g : {g_alpha, g_delta, g_root, g_ema_w}) ok = ok && hipMemsetAsync(g, 0, (size_t)F * 4, st) == hipSuccess;
        return ok ? LEAF_OK : LEAF_ERR_LAUNCH;
    }
    if (!pooled_raw || !grad_out || !g_pool_b) return LEAF_ERR_NULL_POINTER;
    if (use_pcen && (!alpha || !delta || !root || !ema_w || !g_alpha || !g_delta || !g_root || !g_ema_w)) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || TP < 1 || F < 1) return LEAF_ERR_BAD_SHAPE;
    if ((long long)B * F * TP >= (1ll << 31)) return LEAF_ERR_BAD_SHAPE;          // (the caller slices the batch)
    if (!inst_layouts_ok()) return LEAF_ERR_LAUNCH;
    const bool go_bf16 = feat_bf16(flags);
    if ((reinterpret_cast<uintptr_t>(grad_out) & (go_bf16 ? 1u : 3u)) || misaligned16(workspace) ||
        any_misaligned(pooled_raw, alpha, delta, root, ema_w, g_pool_b, g_alpha, g_delta, g_root, g_ema_w))
        return LEAF_ERR_ALIGNMENT;
    const HeadLayout h = head_layout(B, TP, F, flags);
    if (h.S < 1 || h.S > 65535) return LEAF_ERR_BAD_SHAPE;
    if (!workspace || workspace_bytes < h.bytes()) return LEAF_ERR_WORKSPACE;
    HeadBwdParams p{};
    p.raw = pooled_raw; p.gout = grad_out;
    p.alpha = alpha; p.delta = delta; p.root = root; p.ema_w = ema_w;
    p.floor_ = 1e-12f;
    p.mode = (use_pcen ? 1 : 0) | ((flags & LEAF_FLAG_LOG1P) && !use_pcen ? 2 : 0) | (go_bf16 ? 4 : 0);
    p.B = B; p.F = F; p.TP = TP; p.S = h.S; p.L = h.L;
    p.tickets = static_cast<unsigned*>(workspace);
    p.rec = reinterpret_cast<float*>(static_cast<char*>(workspace) + h.ticket_bytes);
    p.ema = h.ema_floats ? p.rec + h.rec_floats : nullptr;
    p.g_pool_b = g_pool_b; p.g_alpha = g_alpha; p.g_delta = g_delta; p.g_root = g_root; p.g_ema_w = g_ema_w;
    // the tickets: one memset in front of the launch.  While the stream is being captured a kernel node zeroes them instead: on this
    // runtime a captured memset node writes zeros on the first replay of its graph and other bytes on the later ones (a stand-alone
    // probe showed it; the tickets then never reach S - 1), and a kernel node replays as it was captured
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &capture) != hipSuccess) {
        (void)hipGetLastError();
        capture = hipStreamCaptureStatusNone;
    }
    if (capture == hipStreamCaptureStatusActive) {
        const int words = (int)(h.ticket_bytes / 4);
        hipLaunchKernelGGL(zero_words_kernel, dim3(ceil_div(words, 256)), dim3(256), 0, st, p.tickets, words);
        LEAF_LAUNCH_CHECK();
    } else if (hipMemsetAsync(p.tickets, 0, h.ticket_bytes, st) != hipSuccess) {
        return LEAF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(leaf_inst_head_bwd(), dim3(F, h.S), dim3(64 * kHeadWaves), 0, st, p);
    LEAF_LAUNCH_CHECK();
    return LEAF_OK;
}

}  // extern "C"
