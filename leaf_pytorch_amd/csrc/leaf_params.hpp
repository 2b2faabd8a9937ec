// leaf_params.hpp -- everything that crosses a kernel launch: the structs passed by value to a kernel (or embedded in one), the
// constants that size them, and the fingerprint of their layout.
// Included by every unit: types and constants only, no function but the structs' own members.
//
// They live in the NAMED namespace `leaf`, so a struct is one type in every translation unit of libleaf_hip.so: the unit that
// instantiates a kernel and the unit that launches it (leaf_inst.hpp: typed kernel pointers) agree on the argument by the
// language's rules.  Kernels, templates and device functions stay in the headers' unnamed namespaces (internal linkage: what
// the inliner sees does not change with the number of units); leaf_common.hpp brings `leaf` into that namespace once.
// (ClipParams / ClipNoiseParams are leaf_clips.hpp's own: that unit launches its kernels itself.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace leaf {

// the clamp bounds of a Gabor filter's sigma (convolution.py:15-22; gabor_bounds, leaf_common.hpp)
struct GaborBounds { float sigma_lo, sigma_hi; };

// ---- direct form on the fp32 MFMA (leaf_fused.hpp) ----------------------------------------------------------------------------
struct FusedParams {
    const void* x;         // [B][T] fp32, bf16 or 16-bit PCM by io_bf16
    int io_bf16;           // sample type of x: kSampleF32 / kSampleBf16 / kSamplePcm16 (leaf_common.hpp)
    const float* W;        // [R][2*FP] half-support tap table (columns in perm order)
    const float* G;        // [FP][GJ] pooling windows (columns in perm order), zero for j >= K
    const int* tile_ks;    // [FP/16]
    int GJ;                // row length of G: noff*hop + 16*kUB*NU rounded up to 4
    float* part;           // [B][TP][noff][FP] per-frame partial pooled sums (columns in perm order)
    int B, T, TP, F, FP, K, hop, padL;
    int KS;                // k-steps of 4 rows, R = 4*KS
    int Hf;                // largest kk whose forward sample x[n+kk] is a real tap: (K-1)/2
    int xshift;            // K/2 - padL: 0 for odd K, 1 for even K
    int NU;                // units of kUB n-blocks per hop-block
    int HP;                // halo (floats) on each side of a wave's staged window = 4*KS
    int XS;                // floats per wave window = 16*kUB*NU + 2*HP
    int q_lo, nq;          // hop-blocks q_lo .. q_lo+nq-1 cover the samples of one clip
    int noff;              // frames a hop-block contributes to: (K-1)/hop + 1
    int tile_base;         // first 16-filter tile of this launch
    int total_tasks;       // B * nq
    int desync_sleeps;     // s_sleep(127) repetitions the second wave of each SIMD waits once at start
    unsigned long long* trace;   // LEAF_TRACE builds only: [8 waves][64] cycle stamps of block 0
    // backward instantiation (BWD) only:
    const float* Gs;       // [FP][GJ] d g/d s tables (same layout as G)
    const float* gcols;    // [B][TP][FP] grad w.r.t. the pre-floor pooled value, columns in perm order
    float* dY;             // [B*T][2*FP] out: grad w.r.t. the filterbank output, time-major, columns as W
    float* dwpart;         // [gridDim.x*kWavesPerWG][FP] out: per-wave partial sums of d pool_w (pre clamp mask)
};

// Which of a frame's partial slots hold data (finalize_kernel, fft_finalize_rows): L > 0 (overlap-save path: slot s = s-th block
// the frame's window meets) -> computed from the geometry, so the partial buffer needs no zero fill; L = 0: the direct path.
struct SlotGeom {
    int L, padL, K, hop, T;
    int nslot;                   // overlap-save path: slots per frame in the partial buffer (2 or 3)
};

// ---- tap-gradient GEMM of the direct-form backward (leaf_backward.hpp) ---------------------------------------------------------
struct DtapsParams {
    const float* x;        // [B][T]
    const float* dY;       // [B*T][2*FP]
    const int* tile_ks;    // k-steps per column tile (support-sorted)
    float* dHpart;         // [gridDim.x][16*NKT][2*FP]
    int B, T, FP, K, Hf, xshift;
    int NKT;               // 16-row k-tiles
    int NW;                // waves per workgroup
    int NS;                // samples per chunk (multiple of 16)
    int HPc;               // window halo = 16*NKT
    int XSC;               // window floats = NS + 2*HPc
    int LD;                // LDS row stride of the dY tile = 2*FP + 16
    int nch;               // chunks per clip
    int total_chunks;      // B * nch
    int tile_base;         // first column tile of this launch's group 0
};

// ---- the table cache's stamps (leaf_fft.hpp: stamp_word) -----------------------------------------------------------------------
constexpr int kStampWords = 32;                          // 128 bytes per slot
constexpr unsigned kStampMagic = 0x4c454146u;
struct StampKey {
    int kind;              // 1: fft_prep_kernel, 2: fft_prep_band_kernel
    int F, K, hop, T, role, n_edge;
    int e[4];              // the role's edge entry (c, m, lo, hi); zeros for the other roles
    float eps2, eta;
    int cross, force, strict;
};

// ---- overlap-save kernels (leaf_fft.hpp and the workgroup kernels on top of it) ------------------------------------------------
// Contiguous dealing of the nblocks = B * nblk blocks to G workgroups (the first `rem` get one more): workgroup w walks
// blocks [start(w), start(w) + count(w)).  A clip whose nblk blocks all fall to one workgroup is OWNED by it: its partial
// sums never leave that CU's reach and the workgroup finalizes it in its tail.  nblocks = 0: nothing is owned (kernels that
// do not finalize).
struct OwnedClips {
    int nblocks, G, nblk;
    __host__ __device__ int per() const { return nblocks / G; }
    __host__ __device__ int rem() const { return nblocks % G; }
    __host__ __device__ int start(int w) const { return w * per() + (w < rem() ? w : rem()); }
    __host__ __device__ int count(int w) const { return per() + (w < rem() ? 1 : 0); }
    __host__ __device__ int wg_of(int gb) const {
        const int q = per(), r = rem(), cut = r * (q + 1);
        return gb < cut ? gb / (q + 1) : r + (gb - cut) / (q > 0 ? q : 1);
    }
    __host__ __device__ bool owned(int b) const {
        return nblocks > 0 && wg_of(b * nblk) == wg_of(b * nblk + nblk - 1);
    }
};
// what the row arithmetic of the finalize step needs (fft_finalize_rows below)
struct FinParams {
    const float* part;     // [B][F][nslot][T']
    int F, TP;
    SlotGeom geo;
    const float *bias, *alpha, *delta, *root, *ema_w;
    float floor_;
    int mode;              // bit0 PCEN, bit1 log1p, bit2 bf16 output, bit3 no floor (the backward's raw pooled tensor)
    void* out;
    float* raw_out;
    const float* clip_scale2;   // LEAF_FLAG_PEAKNORM: [B] s_b^2 multiplying the pooled energies of clip b (NULL: none)
    // set by a workgroup kernel for its own tail only: the per-frame sums of the clips it owns sit in its LDS, already added
    // up ([rows from lds_row0][T']), instead of in `part`
    const float* lds_sums = nullptr;
    int lds_row0 = 0;
    const void* lds_coef = nullptr;   // (the same kernels) FinCoef[F] in its LDS, evaluated at the kernel's start: the tail does not wait for the parameters
};

// ---- band-limited filter tasks (leaf_band.hpp; static workgroup kernels, frame sums in LDS) ---------------------------------
// A frame whose window -- widened by the tails of the decimated pooling window -- is cut by the clip's ends (or would reach
// past them) is an EDGE frame: its sum over block `c` comes from a dense per-(filter, block) table; [lo, hi) is the part of
// the (cut) window that block owns, in absolute samples.
constexpr int kBandMaxEdge = 12;
struct BandEdge { int c, m, lo, hi; };
struct BandParams {
    const int* rec;        // [F][4]: bit 0 / 1 = the filter passes the 256- / 512-point criteria, first bin of its 256- / 512-point window (NULL: every filter on 2048 points)
    const float* gz;       // [F][kBandGzFloats]: decimated pooling windows of both classes
    const float* edge;     // [F][2][kBandMaxEdge][512]: edge-frame tables, register order of the class
    const float* gz2;      // (backward kernels) gz and edge built from the window g[j] (j - c)^2: d pool_w at the decimated rate
    const float* edge2;
    const int* elist;      // [kBandMaxEdge][4]: the edge list (c, m, lo, hi) in device memory
    int lds_off;           // float offset of the band area (plan, twiddle tables) in dynamic LDS
    int reg_lo, reg_hi;    // frames reg_lo .. reg_hi take the shift-invariant window, the others are edge frames
    int n_edge;
    const float* bias;     // (forward kernels) the pooling biases of THIS call, [F]: the energy bound of the class decision follows them
    float smax;            // > 1: the class decision may take them into account (leaf_band.hpp: band_bias_admits); NULL / <= 1: the strict decision alone (backward kernels, LEAF_ALGO_STRICT_BAND_CLASSES)
};

struct FftParams {
    const void* x;         // [B][T] fp32, bf16 or 16-bit PCM by io_bf16
    int io_bf16;           // sample type of x: kSampleF32 / kSampleBf16 / kSamplePcm16 (leaf_common.hpp)
    const float2* H;       // [F][2048] complex spectra, or (real-spectrum kernels, odd K) [F][2048] floats
    const float* Gz;       // [F][GZ]
    float* part;           // [B][F][nslot][TP]: slot s = s-th block the frame's window meets (2, or 3 when K - 1 > L)
    int nslot;
    int B, T, TP, F, K, hop, padL;
    int L;                 // valid outputs per block
    int nblk;              // blocks per clip
    int GZ;                // row length of Gz (multiple of 4)
    int g_bufs;            // wave-private LDS pooling-row buffers: 2 (next row prefetched) when LDS allows, else 1
    int NT;                // 64-sample rows a pooling window can touch: ceil((K+63)/64)
    int scr_floats;        // wave-private LDS floats for transposes / energy rows
    int fq;                // filters per task: kFftFQ when the batch fills the chip, fewer (more, shorter tasks) when not
    int nfq;               // filter groups of fq
    int total_tasks;       // B * nblk * nfq  (one wave per task)
    // backward instantiation only (BWD = 1; real-spectrum tables R | R_mu | R_sigma stacked in H as [3][F][2048] floats)
    const float* gpre;     // [B][F][TP] dL/d(pooled pre-floor)
    const float* pool_w;   // [F] raw pooling widths
    float* dkpart;         // [B*nblk][F][2] per-block partial (d mu, d sigma), before the clamp sub-gradient
    float* dwpart;         // [B*nblk][F]    per-block partial d pool_w, before the clamp sub-gradient
    const float* lone;     // even K, real-spectrum form: [F][2] the unpaired tap w_f[t = -K/2] (backward: [3][F][2] with d/dmu, d/dsigma)
    int rot;               // rotation of the block for the real-spectrum form: K / 2 (= padL for odd K)
    unsigned long long* trace;   // LEAF_TRACE builds only
    // Clip-resident finalize (workgroup kernels): blocks are dealt contiguously, and with fin_fused != 0 a workgroup runs the
    // row arithmetic (bias, floor, EMA, PCEN) itself for every clip it owns outright; fft_finalize_kernel then handles only
    // the clips that straddle two workgroups.
    FinParams fin;
    int fin_fused;
    int stream_ring;       // STREAM kernels: frames of the LDS ring of per-frame partial sums (a power of two)
    BandParams band;       // band-limited filter tasks (rec == NULL: off)
    const float2* spec0;   // [workgroups][kWgRingFloat2]: the half spectrum of every workgroup's FIRST block, computed by the table
                           // launch on CUs it leaves idle (fft_prep_band_kernel); NULL: the kernel transforms it itself
    // Waveform mixup in the load (leaf_common.hpp: mix_load), the kernels with a fused mix only; mix_lam == NULL: off
    const int* mix_perm;   // [B] partner clip of every clip (clamped into [0, B) on the device)
    const float* mix_lam;  // [B] weight of the clip itself; its partner gets 1 - lam
};

// ---- the table launch of the band tasks (fft_prep_band_kernel, fft4k_prep_kernel, fft4k_band_tab_kernel) -----------------------
struct BandTabArgs {
    int T, L, hop, padL;
    float eps2, eta;
    int force;             // tests / tools: 0 decide, 1 / 2 every filter in the 256- / 512-point class, 3 none
    int edge_only;         // frozen-parameter tables (leaf_forward_prepared_f32): grid (F, n_edge), only the edge tables of this clip length
    int* rec;
    float* gz;
    float* edge;
    float* gz2;            // (backward) the same two tables for the window g_f[j] (j - c)^2, c = (K - 1) / 2: d pool_w at the decimated
    float* edge2;          // rate (impulse_responses.py:74-80: d g / d s = g (j - c)^2 / (c^2 s^3)); NULL: not built
    int* elist;
    int* classes;          // leaf_band_classes_f32: [F] the transform length each filter gets (NULL: not asked for)
    const float* cls_bias; // ... for these pooling biases (round 6: the energy bound follows the bias; NULL: the strict decision)
    int n_edge;
    BandEdge e[kBandMaxEdge];
    // the main kernel's first blocks (round 5): waves 1..7 of the workgroups (f, 0) -- idle while wave 0 transforms the filter's
    // taps -- transform the first block of main-kernel workgroups w = 7 f + wave - 1 (+ 7 F, ...) < G into spec0[w]: the one
    // forward transform nothing in the main kernel can overlap with.  Their transposition scratch is the launch's dynamic LDS.
    const void* x;
    int io_bf16, B, nblk, G;
    float2* spec0;
    int cross;             // != 0 (forward launches of the 2048-sample plan, round 6): windows may reach bin kWgFwdBins - 1 (beyond Nyquist)
    unsigned* stamps;      // the table cache's stamps, [2 + n_edge][F][kStampWords] (leaf_fft.hpp); NULL everywhere else
    int strict;            // (stamped launches) LEAF_ALGO_STRICT_BAND_CLASSES, part of the stamp
    int bwd_slabs;         // (backward) != 0: the class decision also asks band_deriv_fits; 1 (2048-sample plan): two more grid rows, (f, 2 + n_edge) and (f, 3 + n_edge), build the spectra of d w / d mu and
                           // d w / d sigma into slabs 1 and 2 of H (what fft_prep_kernel's grid (F, 3) does): one table launch
};

// ---- one-launch small batch (leaf_fft_small.hpp) -------------------------------------------------------------------------------
struct SmallParams {
    const void* x;          // [B][T] fp32, bf16 or 16-bit PCM by io_bf16
    int io_bf16;            // sample type of x: kSampleF32 / kSampleBf16 / kSamplePcm16 (leaf_common.hpp)
    const float* kernel;    // [F][2] (mu, sigma), unclamped
    const float* pool_w;    // [F]
    GaborBounds bd;
    int B, T, TP, F, nblk;
    int ring;               // block spectra held in LDS per pass (<= kSmallRing)
    FinParams fin;          // part unused: the sums stay in LDS
    // SPLIT variant (two workgroups per (clip, filter), grid (F, B, 2)): the EMA state the first half hands to the second,
    // [B][F] pairs (epoch, value bits) in the workspace; `epoch` is this launch's 64-bit ticket (host counter from a random seed)
    unsigned long long epoch;
    unsigned long long* carry;
    // Waveform mixup in the load (leaf_common.hpp: mix_load); mix_lam == NULL: off
    const int* mix_perm;    // [B]
    const float* mix_lam;   // [B]
};

// ---- one-launch streaming step and the bank (leaf_fft_stream.hpp) --------------------------------------------------------------
struct StreamParams {
    const void* chunk;        // [B][chunk_stride], the first Tc samples of a row; fp32 or 16-bit PCM by `pcm`
    const void* hist_in;      // [B][H]: the history half this step reads, hist_len samples of a row (the bank: half 0)
    void* hist_out;           // [B][H]: the other half, receives the next step's history (the bank: half 1)
    float* ema_state;         // [B][F]
    long long chunk_stride;   // samples
    int pcm;                  // sample type of chunk and history: kSampleF32 / kSamplePcm16 (leaf_common.hpp)
    const float* kernel;      // [F][2] (mu, sigma), unclamped
    const float* pool_w;      // [F]
    GaborBounds bd;
    int B, F, H;
    int hist_len, Tc, drop;   // the virtual buffer is hist_len + Tc samples; [drop, hist_len + Tc) is the next step's history
    int first, n, started;    // frames emitted; has a frame been emitted before (the smoother has a state)
    int c_lo, nb;             // blocks the emitted frames' windows meet
    FinParams fin;            // part unused: the sums stay in LDS; fin.out is [B][F][n]
};

// where ONE stream stands in one pass of the body (wave-uniform: from the kernel arguments alone)
struct StreamPos {
    const void* hist_in;      // the history half the stream reads ...
    void* hist_out;           // ... and the one it hands over to
    int hist_len, Tc, drop, first, n, started, c_lo, nb;   // as in StreamParams
    int hist_off, chunk_off;  // samples skipped in front of the history row / the chunk row (the bank's ending pass; else 0)
    int n_lds;                // frame sums the launch's LDS holds (>= n)
    int n_row, o_lo, o_end;   // out rows are n_row long; this pass's frames start at column o_lo and zeros follow them up to o_end
};

// the bank: up to kBankSlots slots per launch and as many PASS records of 6 words; a slot has one record, or two when its stream
// ends on a chunk that also completes frames (header comment), consecutive, the last one marked
constexpr int kBankSlots = 128;
struct StreamPassRec {
    // w[0] = hist_len | Tc << 16          w[1] = drop | first << 16       w[2] = n | c_lo << 16 | nb << 24
    // w[3] = hist_off | chunk_off << 16   w[4] = o_lo | o_end << 16       (StreamPos)
    // w[5] = started | parity << 1 | idle << 2 | last << 3
    unsigned w[6];
};
struct StreamBankParams {
    StreamParams c;                   // what the slots share; its position fields are unused; fin.out is [B][F][n_max]
    int b0;                           // the launch's first slot: workgroup (f, y) serves row b0 + y
    int n_lds, n_max;
    unsigned first[kBankSlots / 4];   // byte y: slot y's first record
    StreamPassRec rec[kBankSlots];
};
static_assert(sizeof(StreamBankParams) <= 4096, "the records travel in the kernel argument segment");

// ---- head-only backward: pool_b and PCEN gradients from pooled_raw in one launch (leaf_head_bwd.hpp) ----------------------------
constexpr int kHeadWaves = 4;            // waves per workgroup, one (b, f) row each at a time
constexpr int kHeadRecFloats = 8;        // a workgroup's record: (s_a, s_d, s_rho, s_w, s_g), padded to 32 bytes
struct HeadBwdParams {
    const float* raw;         // [B][F][TP] pooled_raw: pre-floor, bias included (leaf_forward_save_f32)
    const void* gout;         // [B][F][TP] grad_out, float32 or bfloat16 by bit 2 of mode
    const float *alpha, *delta, *root, *ema_w;   // [F] (PCEN only)
    float floor_;             // the PCEN floor
    int mode;                 // bit0 PCEN, bit1 log1p behind the floor (PCEN off only), bit2 bfloat16 grad_out
    int B, F, TP;
    int S, L;                 // grid (F, S): workgroup (f, s) walks rows b in [s L, min(B, (s + 1) L)) of filter f
    unsigned* tickets;        // [F], zeroed by the host in front of every launch
    float* rec;               // [F][S][kHeadRecFloats]: one partial record per workgroup
    float* ema;               // [F * S * waves][TP] smoother values of rows beyond the register form; NULL when every row fits
    float *g_pool_b, *g_alpha, *g_delta, *g_root, *g_ema_w;   // [F] out (the PCEN four with bit0 only)
};

// Layout fingerprint of the structs above.  The types are shared, but the OBJECT FILES of an incremental build are not: a unit
// compiled before a field was added, or with a macro that changes a layout, would read its arguments at the wrong offsets.  Every
// unit exports the value it was compiled with (leaf_layout_* of leaf_inst.hpp) and leaf_kernels.hip compares them all with its
// own before the first launch (inst_layouts_ok): a stale object is LEAF_ERR_LAUNCH, not a kernel reading the wrong words.
// One line per struct: its size, then the offsets of the fields behind which the layout has changed before.
constexpr unsigned layout_mix(unsigned h, size_t v) { return (h ^ (unsigned)v) * 16777619u; }
template <typename... V>
constexpr unsigned layout_mix(unsigned h, size_t v, V... rest) { return layout_mix(layout_mix(h, v), rest...); }
constexpr unsigned leaf_params_layout() {
    unsigned h = 2166136261u;
    h = layout_mix(h, sizeof(GaborBounds), sizeof(SlotGeom), offsetof(SlotGeom, nslot), sizeof(OwnedClips), sizeof(BandEdge));
    h = layout_mix(h, sizeof(FusedParams), offsetof(FusedParams, part), offsetof(FusedParams, trace), offsetof(FusedParams, dwpart));
    h = layout_mix(h, sizeof(DtapsParams), offsetof(DtapsParams, dHpart), offsetof(DtapsParams, tile_base));
    h = layout_mix(h, sizeof(StampKey), offsetof(StampKey, e), offsetof(StampKey, strict), (size_t)kStampWords);
    h = layout_mix(h, sizeof(FinParams), offsetof(FinParams, geo), offsetof(FinParams, out), offsetof(FinParams, clip_scale2),
                   offsetof(FinParams, lds_row0), offsetof(FinParams, lds_coef));
    h = layout_mix(h, sizeof(BandParams), offsetof(BandParams, elist), offsetof(BandParams, n_edge), offsetof(BandParams, smax),
                   (size_t)kBandMaxEdge);
    h = layout_mix(h, sizeof(FftParams), offsetof(FftParams, part), offsetof(FftParams, lone), offsetof(FftParams, trace),
                   offsetof(FftParams, fin), offsetof(FftParams, stream_ring), offsetof(FftParams, band), offsetof(FftParams, spec0),
                   offsetof(FftParams, mix_perm), offsetof(FftParams, mix_lam));
    h = layout_mix(h, sizeof(BandTabArgs), offsetof(BandTabArgs, e), offsetof(BandTabArgs, x), offsetof(BandTabArgs, stamps),
                   offsetof(BandTabArgs, bwd_slabs));
    h = layout_mix(h, sizeof(SmallParams), offsetof(SmallParams, bd), offsetof(SmallParams, ring), offsetof(SmallParams, fin),
                   offsetof(SmallParams, carry), offsetof(SmallParams, mix_lam));
    h = layout_mix(h, sizeof(StreamParams), offsetof(StreamParams, bd), offsetof(StreamParams, c_lo), offsetof(StreamParams, fin));
    h = layout_mix(h, sizeof(StreamPos), sizeof(StreamPassRec), sizeof(StreamBankParams), offsetof(StreamBankParams, first),
                   offsetof(StreamBankParams, rec), (size_t)kBankSlots);
    h = layout_mix(h, sizeof(HeadBwdParams), offsetof(HeadBwdParams, floor_), offsetof(HeadBwdParams, S), offsetof(HeadBwdParams, tickets),
                   offsetof(HeadBwdParams, g_pool_b), (size_t)kHeadWaves, (size_t)kHeadRecFloats);
    return h;
}

}  // namespace leaf
