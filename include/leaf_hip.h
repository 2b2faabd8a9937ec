/*
 * leaf_hip.h -- C ABI of the MI355X-native LEAF frontend (libleaf_hip.so, gfx950 only).
 *
 * This is the drop-in boundary for the hot path of SarthakYadav/leaf-pytorch:
 *     leaf_pytorch/frontend.py:78-89   Leaf.forward
 * The reference has no native code and therefore no FFI; each entry point below names the
 * reference function(s) (file:line under the reference repo) whose arithmetic it replaces.
 * The Python host side (leaf_pytorch_amd/frontend.py) binds these with ctypes; PyTorch is only
 * used there for device memory and the current HIP stream.  See INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory (HBM), fp32,
 *     contiguous, owned by the caller; the library never allocates, frees or retains pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is enqueued
 *     asynchronously on that stream; nothing synchronises the host.
 *   - re-entrant; nothing is kept between calls except two process-wide, write-once caches: the CU count per
 *     device ordinal, and ONE environment switch read at first use -- LEAF_NO_4K=1 keeps every window on the
 *     2048-sample plan (a test / A-B switch for the 4096-sample kernels; it changes which kernel runs, never the
 *     results beyond fp32 rounding).  Per-call options travel in `algo` / `flags`, never in setters.  Parameters are
 *     re-read on every call (they are learnable: the clamps of the reference are applied functionally, never
 *     written back).
 *   - a WORKSPACE belongs to one call at a time: calls that may execute concurrently (different streams) need workspaces of
 *     their own -- kernels of one call hand data to each other through it (partial sums, tables, the seam slots of the
 *     one-launch kernel's two halves), and a second call writing the same bytes would be read as the first call's.  Calls on ONE
 *     stream may share a workspace (they execute in order).
 *   - ALIGNMENT.  `workspace` and `tables`: 16 bytes -- the kernels read their regions (each a multiple of 256 bytes behind
 *     the base) as float2 / float4 / int4 rows, with 16-byte direct-to-LDS loads and, at the seam of the one-launch kernel,
 *     64-bit atomics (hipMalloc and every framework allocator give 256 bytes or more).  Every other buffer is reached one
 *     element at a time and needs its element's alignment: 4 bytes for float32 / int32 (x, out, pooled_raw, grad_out, g_x, the
 *     parameters, their gradients, every stage input and output, `classes`, the stream state), 2 bytes where a flag makes the
 *     buffer bfloat16 or int16.  Anything below is answered with LEAF_ERR_ALIGNMENT before the workspace check and before any
 *     launch (NULL for an optional argument passes).
 *   - EXACT SIZES.  A call writes nothing outside the buffers it is given at the sizes this header states, the workspace at
 *     exactly the bytes its size query answers; it reads no workspace byte it has not written itself (the workspace may hold
 *     anything on entry, a previous call's leftovers included) and writes -- never accumulates into -- every element of its
 *     outputs (tests/test_gpu_abi_memory.py).
 *   - return value: LEAF_OK (0) or a negative leaf_status code.  Never throws, never aborts.
 *   - B = 0 is the EMPTY BATCH, not an error (the reference returns a (0, F, T') tensor: frontend.py:78-89 ->
 *     convolution.py:97): leaf_forward_f32 / _save_f32 / _prepared_f32 / _profiled_f32 return LEAF_OK without a launch
 *     (x / out / workspace may be NULL), leaf_backward_f32 zero-fills the parameter gradients (the sum over no clips)
 *     and touches nothing else; the workspace queries return 0.  T, F, K, hop must still be >= 1.
 *
 * Shapes (reference notation):
 *   B batch, T samples per clip, F = n_filters, K = window size in samples, hop = stride in samples,
 *   T' = leaf_num_frames(T, K, hop) = floor((T + padL + padR - K) / hop) + 1 (= floor((T-1)/hop)+1).
 */
#ifndef LEAF_HIP_H_
#define LEAF_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LEAF_ABI_VERSION 6

typedef enum leaf_status {
    LEAF_OK = 0,
    LEAF_ERR_NULL_POINTER = -1,   /* a required pointer argument is NULL                    */
    LEAF_ERR_BAD_SHAPE = -2,      /* T,F,K,hop out of range (all >= 1), B < 0 or B*T >= 2^31 */
    LEAF_ERR_WORKSPACE = -3,      /* workspace missing or smaller than leaf_workspace_bytes */
    LEAF_ERR_BAD_ALGO = -4,       /* unknown / inapplicable algorithm selector              */
    LEAF_ERR_LAUNCH = -5,         /* HIP reported a launch failure (hipGetLastError != 0)   */
    LEAF_ERR_NO_DEVICE = -6,      /* no usable gfx950 device                                */
    LEAF_ERR_ALIGNMENT = -7,      /* a buffer is below its alignment: workspace / tables 16-byte, float32 buffers 4-byte, bfloat16 /
                                     16-bit PCM buffers 2-byte (ALIGNMENT under Conventions); answered before the workspace check
                                     and before any launch */
    LEAF_ERR_UNSUPPORTED = -8     /* valid arguments, unsupported combination: bfloat16 I/O with the staged FORWARD
                                     kernels (the backward takes it on every path, ABI 6); LEAF_FLAG_PEAKNORM with
                                     leaf_forward_save_f32 / leaf_forward_prepared_f32 or off the overlap-save paths;
                                     LEAF_FLAG_X_PCM16 with the staged FORWARD kernels, together with LEAF_FLAG_IO_BF16, or
                                     with g_x != NULL (an integer input has no gradient); LEAF_FLAG_OUT_BF16 with the staged
                                     FORWARD kernels (as bfloat16 I/O: the fused paths narrow in their stores, that one has no
                                     such store) */
} leaf_status;

/* flags */
#define LEAF_FLAG_PCEN   0x1   /* apply PCEN (requires alpha, delta, root, ema_w)                */
#define LEAF_FLAG_LOG1P  0x2   /* extension (not in the reference): out = log1p(max(pooled, 1e-5)), PCEN off (ignored with
                                  LEAF_FLAG_PCEN).  ABI 6: leaf_forward_save_f32 and leaf_backward_f32 honour it too -- the
                                  backward divides grad_out by 1 + pooled above the floor where it reads it (no extra
                                  launch, no extra workspace) */
#define LEAF_FLAG_BWD_STAGED 0x8 /* leaf_backward_f32 only: force the staged (one-lane-per-output) kernels */
#define LEAF_FLAG_BWD_MFMA 0x10 /* leaf_backward_f32 only: force the fused MFMA backward (skip the overlap-save FFT one) */
#define LEAF_FLAG_BWD_FULL_TRANSFORMS 0x40 /* leaf_backward_f32 only (ABI 4): no band-limited filter tasks in the backward -- by default the
                                  static 16 kHz and 32 kHz backwards (K = 401 / hop = 160: parameter gradients from 3/8 block per CU,
                                  with dL/dx at every batch; K = 801 / hop = 320 on 4096-sample blocks: parameter gradients only) give
                                  the filters the forward runs on short transforms their gradients at the decimated rate too
                                  (leaf_band_bwd.hpp): within ~1e-5 of the full-transform gradients' largest component */
#define LEAF_FLAG_BWD_STRICT_BAND_CLASSES 0x80 /* leaf_backward_f32 only (ABI 5): the backward's band tasks decide their classes by round 5's rule
                                  alone; by default they take the forward's decision, which follows the pooling bias of the call
                                  (LEAF_ALGO_STRICT_BAND_CLASSES below) -- measured: gradients stay at ~1e-6 of their column's largest.
                                  Either way a backward launch adds its own condition (leaf_band.hpp band_deriv_fits): the window
                                  holds the DERIVATIVE spectra d/dmu, d/dsigma of the filter, which are wider than the filter; a
                                  filter that fails it takes the next wider class in the backward only */
#define LEAF_FLAG_PEAKNORM 0x20 /* forward only, overlap-save paths (LEAF_ALGO_AUTO / _FFT / _FFT_WG where their plan fits; else
                                  LEAF_ERR_UNSUPPORTED): the result is that of the forward applied to the PEAK-NORMALISED clips
                                  (utilities/data/raw_transforms.py:334-345, the last transform of every reference data
                                  pipeline: a clip whose peak |x| exceeds 1 is divided by that peak) without the normalised
                                  waveform ever being written: one read-only pre-pass finds each clip's scale s, and because the
                                  path is linear up to |.|^2, s^2 multiplies the pooled energies where the bias is added
                                  (pooling.py:41).  Equal to leaf_peak_normalize_f32 + forward up to fp32 rounding (~1e-7). */
#define LEAF_FLAG_IO_BF16 0x4  /* extension (BASELINE configs[4]): x and out are bfloat16 buffers (2 bytes per element, 2-byte
                                  aligned), arithmetic stays fp32; fused forward paths only.  ABI 6, training: leaf_forward_save_f32
                                  takes it (pooled_raw stays fp32), and in leaf_backward_f32 x, grad_out and g_x are bfloat16
                                  (g_x rounded to nearest even) while parameters, their gradients and pooled_raw stay fp32.  The
                                  overlap-save backwards widen x in their loads (no fp32 copy: the workspace does not grow); the
                                  MFMA and the staged backward take one widening pass into the workspace, which
                                  leaf_backward_workspace_bytes accounts for when given the flag */
#define LEAF_FLAG_X_PCM16 0x100 /* extension (additive: the ABI version stays 6): x is an int16_t [B][T] buffer behind the const
                                  float*, 2-byte aligned (an odd address: LEAF_ERR_ALIGNMENT), and each sample means v / 32768 --
                                  exact in fp32, so the results carry the bits of the float32 call on float(v) / 32768.  Everything
                                  else stays float32: out, pooled_raw, grad_out, the parameters and their gradients.  Honoured by
                                  leaf_forward_f32, _save_f32, _prepared_f32, _profiled_f32, leaf_backward_f32 and
                                  leaf_backward_workspace_bytes.  Every fused forward path converts in its loads (sign-extending
                                  16-bit load, int -> float, * 2^-15); LEAF_ALGO_STAGED, explicit or what AUTO resolves to, answers
                                  LEAF_ERR_UNSUPPORTED (leaf_workspace_bytes takes no flags, so that path cannot get a widened copy).
                                  Backward: the static overlap-save kernels and the 4096-sample plans read int16 directly; the
                                  run-time-geometry 2048-sample kernels, the MFMA and the staged backward read one widened fp32 copy
                                  in the workspace, reported by leaf_backward_workspace_bytes exactly where it is for bfloat16.
                                  g_x must be NULL (an integer input has no gradient) and LEAF_FLAG_IO_BF16 must be clear (that flag
                                  says x is bfloat16): LEAF_ERR_UNSUPPORTED, answered before the workspace check and before any
                                  launch.  bfloat16 features from an int16 waveform are LEAF_FLAG_X_PCM16 | LEAF_FLAG_OUT_BF16.
                                  LEAF_FLAG_PEAKNORM with it is valid on every entry point and path: no
                                  |v / 32768| exceeds 1, so every clip's scale is 1 and the peak pre-pass is skipped. */
#define LEAF_FLAG_OUT_BF16 0x200 /* extension (additive: the ABI version stays 6): the FEATURE side alone is bfloat16 -- `out` of the
                                  forward entries and `grad_out` of the backward entries are bfloat16 buffers behind the float
                                  pointers (2 bytes per element, 2-byte aligned; an odd address: LEAF_ERR_ALIGNMENT) -- while x
                                  stays what its own flags say (float32, or int16 with LEAF_FLAG_X_PCM16) and everything else
                                  stays float32: pooled_raw, the parameters, their gradients, and g_x, which follows x.  The
                                  arithmetic is that of the float32 call: the forward rounds each feature to nearest even where
                                  it stores it (NaN to the quiet NaN), so `out` holds the float32 call's result narrowed, bit
                                  for bit; the backward widens grad_out where it reads it (exact), so its gradients are those of
                                  the float32 call on the widened grad_out.  No cast kernel, no float32 copy: no workspace of any
                                  path grows with this flag (the one read of grad_out, by the floor / PCEN backward of every
                                  path, MFMA and staged included, widens in its load).  Honoured by leaf_forward_f32, _save_f32,
                                  _prepared_f32, _profiled_f32, leaf_backward_f32, leaf_backward_workspace_bytes and the
                                  waveform-mixup entries leaf_forward_mix_f32, leaf_forward_save_mix_f32, leaf_backward_mix_f32,
                                  leaf_backward_mix_workspace_bytes (which keep refusing LEAF_FLAG_IO_BF16).  Together with
                                  LEAF_FLAG_IO_BF16 it is redundant and accepted.  LEAF_ALGO_STAGED, explicit or what AUTO
                                  resolves to, answers LEAF_ERR_UNSUPPORTED before the workspace check and before any launch,
                                  as for bfloat16 I/O. */
#define LEAF_FLAG_OUT_PCM16 0x400 /* extension (additive: the ABI version stays 6), leaf_resample_f32 only: `out` is an int16_t buffer
                                  (2-byte aligned) and each output is q = rintf(y * 32768.0f), round half to even, clamped to
                                  [-32768, 32767] (saturating, never wrapping), NaN -> 0.  No other entry names this bit. */

/* algorithm selector for the fused path */
#define LEAF_ALGO_AUTO   0     /* _FFT_SMALL for a handful of clips of a LEAF geometry; else the FFT kernels when their plan fits and K >= 224 or the geometry has a static instance, else MFMA, else staged */
                               /* NOTE: the algorithms agree to ~1e-6 relative, not bit for bit, so under AUTO a clip's output bits depend on
                                  which kernel its batch lands on: they change at the batch thresholds (B * F <= 2 #CUs: _FFT_SMALL; from
                                  ~7/16 block per CU: _FFT_WG; below: _FFT), with the device's CU count and with
                                  LEAF_ALGO_RESERVE_CUS.  Within ONE algorithm a clip's bits do not depend on the batch: pass an explicit
                                  selector where batch-invariant bits matter (tests/test_gpu_dropin.py pins both behaviours). */
#define LEAF_ALGO_STAGED 1     /* unfused stage kernels (materialises every intermediate)    */
#define LEAF_ALGO_MFMA   2     /* fused symmetric-Gabor fp32-MFMA kernel + finalize kernel   */
#define LEAF_ALGO_FFT    3     /* fused overlap-save FFT kernel (2048-point, one wave per block) + finalize kernel */
#define LEAF_ALGO_FFT_WG 4     /* overlap-save, one workgroup per block: the block's spectrum computed once and shared
                                  through LDS by 9-16 waves; static instances for the 16 / 32 / 8 kHz LEAF geometries,
                                  run-time geometry for every other window the plans cover (2048-sample blocks: 64..1216
                                  taps, odd or even; 4096-sample blocks: K = 801 / hop 320 and odd windows 833..2049);
                                  what AUTO picks from about half a block per CU.  2048-sample plan: same tables,
                                  workspace and finalize kernel as LEAF_ALGO_FFT. */

#define LEAF_ALGO_FFT_SMALL 5  /* a handful of clips (test.py:57-71: inference on 1 s chunks) in ONE launch: one workgroup per
                                  (clip, filter) builds the filter's spectrum and pooling weights itself, transforms the
                                  clip's blocks, pools, and runs bias / floor / EMA / PCEN of its row -- no table kernel, no
                                  partial sums in HBM, no row kernel.  16 kHz and 8 kHz LEAF geometries (401/160, 201/80),
                                  B * F <= 2 #CUs (two rounds of workgroups since round 5: 7 .. 12 clips of the default front end 41 -> 30 us), clips of up to 20 blocks; what AUTO picks there.  While 2 B F <= #CUs (clips
                                  of 2..10 blocks) TWO workgroups of seven waves serve a (clip, filter) -- each a half of the
                                  row's frames, the EMA state at the seam handed over through the workspace under a 64-bit
                                  per-launch ticket (ABI 4); a clip's bits are the same in both forms.  The EMA recurrence
                                  runs as a lane scan here: the smoothed value agrees with the other algorithms' sequential
                                  loop to ~1e-7 relative, not to the bit.  Workspace: the per-clip scales of
                                  LEAF_FLAG_PEAKNORM + 16 bytes per (clip, filter) for the seam (leaf_workspace_bytes). */

/* tuning override (tools/ only), OR-ed into `algo`: the fused kernel delays the second wave of every SIMD by
 * n * s_sleep(127) once at start; without it the delay is derived from the geometry. */
#define LEAF_ALGO_TUNE_DESYNC(n) (((n) + 1) << 8)

/* CU reservation, OR-ed into `algo` (forward entry points and leaf_workspace_bytes): this call sizes its persistent kernels
 * for (#CUs - k) compute units, 0 <= k <= 255, leaving k CUs free for kernels of OTHER streams that must make progress
 * while it runs -- the RCCL kernel of the feature all-gather on a side stream: the default kernels keep one
 * workgroup with ~all of a CU's LDS resident on every CU for the whole launch, so a collective launched beside them would
 * otherwise only be scheduled when a launch retires.  Per call, no setter, no state kept between calls. */
#define LEAF_ALGO_RESERVE_CUS(k) (((k) & 0xff) << 16)

/* Streaming finalize, OR-ed into `algo` (forward entry points; static LEAF geometries on the workgroup kernel, batches that
 * give every workgroup whole clips -- otherwise ignored): the per-frame partial sums stay in an LDS *ring* and each block's
 * completed frames are finalized (bias, floor, EMA, PCEN) by the wave that finishes the block's last filter; the finished
 * values are staged in LDS and leave in 128-byte row segments.  No partial-sum buffer in HBM, no second kernel, no tail.
 * Same bits as the default path.  Without the flag it runs exactly where the alternative would be a round trip of the
 * partial sums through HBM: whole clips per workgroup whose frame sums do not fit the LDS (several clips per workgroup,
 * long clips).  Where they do fit (one 1 s clip per workgroup) the default keeps them in LDS and finalizes in the kernel's
 * tail, measured ~1 % faster; the flag selects the streaming form there too. */
#define LEAF_ALGO_STREAM_FINALIZE (1 << 25)

/* Full transforms, OR-ed into `algo` (forward entry points): switches the band-limited filter tasks off.  By default the
 * static 16 kHz workgroup kernel (K = 401, hop = 160) runs every filter whose spectrum -- decided per call on the device from
 * the table the call has just built, i.e. from the CURRENT clamped (mu, sigma) -- holds all but 9e-12 of its energy inside 256
 * or 512 of the 2048 bins on a 256- / 512-point inverse transform of those bins, eight / four filters per task, and pools
 * |y|^2 at the decimated rate (leaf_band.hpp); the static 32 kHz kernel (K = 801, hop = 320, 4096-sample
 * blocks; ABI 4) likewise with one class: a 512-bin window of the 4096-point spectrum, four filters per task, decimation 8.
 * The result differs from the full-transform path by <= ~1e-6 relative (north star: 1e-4); with this flag the
 * call runs the 2048- / 4096-point task for every filter, as before round 5.  leaf_forward_save_f32 (the training forward) takes the
 * band tasks as well (the saved pooled tensor differs by ~1e-6; leaf_backward_f32 has its own band tasks and its own switch,
 * LEAF_FLAG_BWD_FULL_TRANSFORMS), and so does
 * leaf_forward_prepared_f32 when its workspace is sized as documented. */
#define LEAF_ALGO_FULL_TRANSFORMS (1 << 26)

/* Strict band classes, OR-ed into `algo` (forward entry points; ABI 5).  Since round 6 the class decision above also admits a
 * filter whose window drops MORE than 9e-12 of its energy where the pooling BIAS of this call makes that harmless
 * (pooling.py:21-22,31-42): a pooled value is p = bias_f + sum g |y|^2 >= bias_f, and for |x| <= 1 what a window drops adds at most
 * G_0 max_{k outside} R_k^2 / 2 to it (one full-scale tone on the largest dropped bin), so the class is taken when
 * bias_f >= 6 G_0 max R_k^2 / (2 * 5e-6) -- at most 5e-6 of any output; the 6 covers a window edge at DC / Nyquist, where kept
 * components beat against their own dropped images -- provided the filter's pooling window (pool_w) low-passes the cross term
 * between the filter's core and the dropped part: to round 5's level, 6e-6 of a frame's energy, for equal amplitudes, and to 5e-6
 * of the output for a weak kept component next to a strong dropped one, which again asks for a minimal bias (leaf_band.hpp:
 * band_need; one-sample pooling windows take the bias-free part of the rule).  At the default bias 1.0 and pooling width 0.4 this
 * admits four more of the 40 default 16 kHz filters (sigma = 48 samples) and 23 more of the 80 default 32 kHz ones (sigma = 96) to the
 * band tasks.  Two more changes of round 6 ride on the same switch.  (a) On the 2048-sample plan the forward's windows may cross
 * Nyquist (the kernel keeps bins 0..1151 of a block's spectrum; a real block's bins above 1024 mirror those below): a filter whose pass
 * band reaches beyond pi -- the top two of the default 16 kHz bank, anything trained against the clamp of convolution.py:15-22 -- is
 * centred in its window instead of cut by one that ends at Nyquist.  (b) The aliasing bound: two spectral lines more than ~0.3 M bins
 * apart inside an M-bin window beat where the decimated grid cannot represent them; round 5's bound (2e-4 of the filter's energy at lag
 * M / 2) let sigma = 15 - 16 samples onto 256 points, where two tones of amplitude 0.5 at +- 60 bins of the centre were off by 1.5e-4 of
 * (bias 0.1 + pooled energy) on a clip's first frame (profiles/r06/band_alias_pairs.txt).  The pair sums may now reach 1e-5 of the filter's
 * energy only under a minimal bias derived from them (mirror-image pairs of a window across Nyquist included; leaf_band.hpp band_need) and
 * 1e-6 without one; a bias <= 6e-5 (or NaN) takes the bias-free part of the rule.
 * The tables do not depend on the bias (the prep kernels record the smallest admissible bias per filter and class); the decision is
 * taken by the forward kernel from the pool_b of the call.  With this flag round 5's rule applies -- its energy and aliasing bounds,
 * windows inside the half spectrum: its decision, bit for bit.  The backward's band tasks take the same decision, with windows inside
 * the half spectrum (their own switch: LEAF_FLAG_BWD_STRICT_BAND_CLASSES). */
#define LEAF_ALGO_STRICT_BAND_CLASSES (1 << 27)

/* No table cache, OR-ed into `algo` (additive: the ABI version stays 6): leaf_forward_cached_f32 takes the route of
 * leaf_forward_f32 -- the table launch rebuilds everything into the workspace, the cache is neither read nor written.  What tests
 * and A/B runs compare the cached route against; ignored by every other entry point. */
#define LEAF_ALGO_NO_TABLE_CACHE (1 << 28)

int leaf_abi_version(void);
const char* leaf_status_string(int status);

/* utils.py:5-10 (padding) + the strided-conv output length used by pooling.py:41. */
int leaf_num_frames(int T, int K, int hop);

/* Bytes of device scratch leaf_forward_f32 / leaf_pool_f32 need for this problem and algo. */
size_t leaf_workspace_bytes(int B, int T, int F, int K, int hop, int algo);

/*
 * Whole forward: frontend.py:78-89 (GaborConv1d -> SquaredModulus -> GaussianLowPass -> max(.,1e-5)
 * -> PCENLayer).
 *   x        [B][T]        waveform (the reference's (B,1,T) with the unit channel dropped)
 *   kernel   [F][2]        _complex_conv._kernel (mu, sigma), unclamped   (convolution.py:58)
 *   pool_w   [F]           _pooling.weights (1,1,F,1) flattened, unclamped (pooling.py:18-20)
 *   pool_b   [F]           _pooling._bias                                  (pooling.py:21-22)
 *   alpha, delta, root, ema_w [F]  _compression.{alpha,delta,root,ema._weights}
 *                          (postprocessing.py:52-54,11); ignored (may be NULL) without LEAF_FLAG_PCEN
 *   out      [B][F][T']
 */
int leaf_forward_f32(const float* x, int B, int T,
                     const float* kernel, const float* pool_w, const float* pool_b,
                     const float* alpha, const float* delta, const float* root, const float* ema_w,
                     int F, int K, int hop, int flags, int algo,
                     float* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * leaf_forward_f32 with a SELF-VALIDATING TABLE CACHE (additive: the ABI version stays 6).  Everything the table launch of the
 * 2048-sample plan writes except the first-block spectra depends only on (kernel, pool_w, F, K, hop), the band edge tables on T as
 * well; in inference these stay the same from call to call.  `cache` is a caller-owned device buffer of leaf_table_cache_bytes(F, K,
 * hop, T) bytes (16-byte aligned, exact-size, read-write) that holds those tables between calls -- spectra, pooling rows, col_of, the
 * band records and decimated pooling windows, the edge tables and edge list of this T -- and one STAMP per workgroup of the table
 * launch: a magic word and the bit patterns of every input that workgroup reads (kernel[f], pool_w[f], F, K, hop, T, its edge entry,
 * the class rule's constants and options).  The table launch runs in validate-or-build form: a workgroup whose stamp matches returns,
 * any other invalidates its stamp, builds what leaf_forward_f32's launch builds and writes the stamp last (a build cut short never
 * reads as valid).  The tables therefore follow the parameters OF THIS CALL, by content -- no staleness window, nothing keyed on a
 * pointer or a version -- and the result equals leaf_forward_f32's bit for bit (the main kernel transforms its first blocks itself,
 * as for 16-bit PCM input: the same bits).  A default step is then a validator launch (a few microseconds) + the main kernel.
 *   - the caller ZEROES the buffer once, before first use (a zeroed stamp is invalid); afterwards the library alone writes it.
 *   - one cache belongs to one stream at a time, like a workspace; a buffer sized for a T with more edge entries serves one with fewer.
 *   - the pooling bias is not part of a stamp: the tables do not depend on it (the main kernel builds its plan from pool_b of the call).
 *   - served: the workgroup kernels (static and run-time geometry) and the per-wave kernel of the 2048-sample plan.  Every other plan
 *     (4096-sample blocks, the one-launch small-batch kernel, MFMA, staged), LEAF_FLAG_PEAKNORM and LEAF_ALGO_NO_TABLE_CACHE take
 *     leaf_forward_f32's route unchanged and leave the cache untouched; so does cache == NULL.
 *   - a misaligned cache: LEAF_ERR_ALIGNMENT; cache_bytes below the size query on a served route: LEAF_ERR_WORKSPACE; both before any
 *     launch.  `workspace` is leaf_workspace_bytes' as for leaf_forward_f32.
 * leaf_table_cache_bytes returns 0 where the shape has no 2048-sample plan (nothing to cache).
 */
size_t leaf_table_cache_bytes(int F, int K, int hop, int T);
int leaf_forward_cached_f32(const float* x, int B, int T,
                            const float* kernel, const float* pool_w, const float* pool_b,
                            const float* alpha, const float* delta, const float* root, const float* ema_w,
                            int F, int K, int hop, int flags, int algo,
                            float* out, void* workspace, size_t workspace_bytes,
                            void* cache, size_t cache_bytes, void* stream);

/*
 * Training forward: leaf_forward_f32 that additionally stores pooled_raw [B][F][T'] = bias + pooled energy BEFORE
 * the 1e-5 floor (pooling.py:41 output).  Passing it to leaf_backward_f32 saves the backward one filterbank pass.
 */
int leaf_forward_save_f32(const float* x, int B, int T,
                          const float* kernel, const float* pool_w, const float* pool_b,
                          const float* alpha, const float* delta, const float* root, const float* ema_w,
                          int F, int K, int hop, int flags, int algo,
                          float* out, float* pooled_raw, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Measurement variant of leaf_forward_f32 (algo = LEAF_ALGO_AUTO, _MFMA or _FFT): same work on `stream`, bracketed by
 * HIP events recorded on that stream.  Blocks the host until the forward has finished and returns in
 * stage_ms[0..2] the device time (ms) of {table/spectrum preparation, fused filterbank+pool kernel(s), finalize/PCEN
 * kernel}.  Used by bench.py for the per-kernel roofline; not for production calls.
 */
int leaf_forward_profiled_f32(const float* x, int B, int T,
                              const float* kernel, const float* pool_w, const float* pool_b,
                              const float* alpha, const float* delta, const float* root, const float* ema_w,
                              int F, int K, int hop, int flags, int algo,
                              float* out, void* workspace, size_t workspace_bytes, void* stream,
                              float* stage_ms /* host, 3 floats */);
/* which algorithm LEAF_ALGO_AUTO resolves to for this problem (LEAF_ALGO_FFT_SMALL / _FFT_WG / _FFT / _MFMA / _STAGED) */
int leaf_auto_algo(int B, int T, int F, int K, int hop);
/* Plan of the overlap-save path for this problem (measurement / roofline arithmetic in bench.py; no reference
 * counterpart): info[0..7] (host ints) = {transform length N, valid outputs per block L, blocks per clip, filters per
 * task, filter groups, partial-sum slots per frame, pooling-row LDS buffers, dynamic LDS bytes per workgroup} -- of the
 * 4096-sample plan (N = 4096) when that is what LEAF_ALGO_AUTO runs for this problem, else of the 2048-sample plan.
 * LEAF_ERR_BAD_ALGO when neither covers the geometry. */
int leaf_fft_plan_info(int B, int T, int F, int K, int hop, int* info);
/* Which inverse-transform length each filter gets from the band-limited filter tasks (LEAF_ALGO_FULL_TRANSFORMS above;
 * leaf_band.hpp) for the CURRENT parameters (measurement / roofline arithmetic in bench.py, tests; no reference counterpart):
 * classes[f] (DEVICE int32 [F]) = 256, 512 or 2048 -- the decision the forward makes on the device from the filter's own
 * spectrum (convolution.py:15-22 clamps, impulse_responses.py:5-16 taps): all but 9e-12 of the energy of R_f inside the
 * window, and the autocorrelation of |R_f| at lags M/2 and 3M/4 below 2e-4 of its energy.  The forward may still run a
 * 256-class filter on 512 points to fill a task.  On the 4096-sample plan (K = 801, hop = 320) there is one class: 512 (a
 * 512-bin window of the 4096-point spectrum, four filters per task) or 4096.  workspace >= max(leaf_fft_tables_bytes(F, K, hop),
 * leaf_workspace_bytes(1, 8192, F, K, hop, LEAF_ALGO_FFT_WG)).  LEAF_ERR_UNSUPPORTED for a geometry without band tasks (every
 * filter on 2048- / 4096-point transforms).  pool_b (ABI 5; DEVICE [F], may be NULL): the pooling biases the decision is taken
 * for -- what a forward call with these biases runs (LEAF_ALGO_STRICT_BAND_CLASSES above: round 6's bounds, windows that may cross
 * Nyquist on the 2048-sample plan); NULL: round 5's decision, the one quoted in this comment (what the flag runs). */
int leaf_band_classes_f32(const float* kernel, const float* pool_w, const float* pool_b, int F, int K, int hop, int* classes,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * Backward of the whole forward (what autograd derives for frontend.py:78-89): given grad_out = dL/d out
 * [B][F][T'], writes dL/d parameter for the seven parameters (same shapes as the inputs; g_alpha..g_ema_w are
 * ignored without LEAF_FLAG_PCEN) and, when g_x != NULL, dL/d x [B][T].  Clamp sub-gradients follow
 * torch.clamp / torch.min / torch.max / torch.maximum as used by the reference (convolution.py:19-20,
 * impulse_responses.py:75, postprocessing.py:14,63-64, frontend.py:84).  Every forward intermediate is recomputed on
 * the device.  Default for windows of 224 .. 1216 taps, odd or even (incl. the reference's default 401/160), and odd windows
 * up to 2049 taps: overlap-save backward (the forward FFT kernels with a backward epilogue: transposed pooling, a second
 * transform, and the tap gradient as two spectral dot products per block and filter; 4096-sample blocks for the 32 kHz
 * geometry and for windows from 833 taps).  With g_x != NULL the same kernels also yield dL/dx for every window up to
 * 1216 taps (the block's spectral gradient summed over its filters, one more transform per block; deterministic, no
 * atomics; on 4096-sample blocks at the 32 kHz geometry K = 801 / hop 320, on 2048-sample blocks elsewhere).  Otherwise, or with LEAF_FLAG_BWD_MFMA: fused MFMA path (filterbank recompute with a backward epilogue that
 * writes dL/dy time-major, then the tap-gradient GEMM dH = S^T dY on the MFMA).  With g_x != NULL beyond 1216 taps,
 * LEAF_FLAG_BWD_STAGED or a geometry neither covers: staged one-lane-per-output kernels.  Workspace =
 * leaf_backward_workspace_bytes for the SAME flags and need_dx = (g_x != NULL): sized for the path that will actually
 * run (a few MB for the overlap-save backward; the staged path materialises dL/dy, B*T*2F floats).
 * ABI 6: LEAF_FLAG_LOG1P (PCEN off) and LEAF_FLAG_IO_BF16 (x, grad_out, g_x bfloat16 behind the float pointers) as described
 * at the flags; x, grad_out and g_x must be 4-byte (bfloat16: 2-byte) aligned, the workspace 16-byte, else LEAF_ERR_ALIGNMENT.
 * LEAF_FLAG_X_PCM16: x alone is int16 (2-byte aligned), grad_out stays float32, g_x must be NULL (LEAF_ERR_UNSUPPORTED).
 * LEAF_FLAG_OUT_BF16: grad_out alone is bfloat16 (2-byte aligned), widened where it is read; x and g_x as the other flags say.
 */
size_t leaf_backward_workspace_bytes(int B, int T, int F, int K, int hop, int flags, int need_dx);
int leaf_backward_f32(const float* x, int B, int T,
                      const float* kernel, const float* pool_w, const float* pool_b,
                      const float* alpha, const float* delta, const float* root, const float* ema_w,
                      int F, int K, int hop, int flags, const float* grad_out,
                      const float* pooled_raw /* from leaf_forward_save_f32, or NULL = recompute */,
                      float* g_kernel, float* g_pool_w, float* g_pool_b,
                      float* g_alpha, float* g_delta, float* g_root, float* g_ema_w,
                      float* g_x, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Head-only backward (additive: the ABI version stays 6): the gradients of pool_b and of the four PCEN vectors alone, for a
 * frontend whose Gabor kernel and pooling width are frozen and whose input needs no gradient.  They depend on nothing but
 *   pooled_raw [B][F][T'] float32  the pre-floor pooled tensor, bias included, exactly what leaf_forward_save_f32 writes, and
 *   grad_out   [B][F][T']          float32, or bfloat16 behind the float pointer with LEAF_FLAG_OUT_BF16 / LEAF_FLAG_IO_BF16
 *                                  (here both mean "grad_out is bfloat16"; widened where it is read, 2-byte aligned),
 * so the call takes no waveform, builds no tables and runs no transform.  alpha, delta, root, ema_w [F] and g_alpha .. g_ema_w [F]
 * are required with LEAF_FLAG_PCEN and ignored (may be NULL) without it; then g_pool_b [F] is the sum of grad_out over the entries
 * above the 1e-5 floor, each divided by 1 + pooled_raw with LEAF_FLAG_LOG1P (ignored with LEAF_FLAG_PCEN, as everywhere).  The
 * values agree with those leaf_backward_f32 gives for the same five gradients to float32 rounding (the rows' arithmetic is the same
 * code; the sum over the batch is taken in another fixed order), with the same clamp sub-gradients.
 * One hipMemsetAsync (the ticket words at the workspace's start) and ONE kernel launch per call, both on `stream`: the sum over the
 * batch happens inside the launch, in a fixed order and without floating-point atomics, so the result is bit-identical from call
 * to call.  Nothing is allocated and nothing synchronises: the call can be captured into a HIP graph (while `stream` is being
 * captured the tickets are zeroed by a one-workgroup kernel node in place of the memset node, whose replays were seen to write
 * other bytes than zeros: two kernel nodes, replayed with the eager call's bits).  Nothing is assumed about the workspace's
 * contents; its size depends on B, T', F, the flags and the device's CU count.
 * Status, in this order and before anything is launched: a flag other than the four above: LEAF_ERR_UNSUPPORTED; B == 0 (the
 * empty batch): the outputs are zero-filled with memsets, nothing else runs (the inputs and the workspace may be NULL);
 * LEAF_ERR_NULL_POINTER; B < 0, T' < 1, F < 1 or B * F * T' >= 2^31 (slice the batch and add): LEAF_ERR_BAD_SHAPE; buffers below
 * 4-byte (bfloat16 grad_out: 2-byte; workspace: 16-byte) alignment: LEAF_ERR_ALIGNMENT; a workspace that is NULL or below the
 * size query for the same B, T', F and flags: LEAF_ERR_WORKSPACE.  The size query answers 0 for arguments the call refuses.
 */
size_t leaf_backward_head_workspace_bytes(int B, int TP, int F, int flags);
int leaf_backward_head_f32(const float* pooled_raw, const float* grad_out, int B, int TP, int F,
                           const float* alpha, const float* delta, const float* root, const float* ema_w,
                           int flags, float* g_pool_b, float* g_alpha, float* g_delta, float* g_root,
                           float* g_ema_w, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Waveform mixup in front of the frontend (the reference's training loop, utilities/data/mixup.py:17-24 with train.py:237-243),
 * additive to ABI 6.  Per clip b, with the partner clip p = mix_perm[b] and the weight lam = mix_lam[b], a mixed sample is
 *     om = 1 - lam;   x'[b][n] = (x[b][n] * lam) + (x[p][n] * om)
 * in fp32 with three separately rounded operations (no fused multiply-add): bit for bit the reference's expression.  x is float32,
 * or int16 with LEAF_FLAG_X_PCM16 (the sample v means v / 32768, which is exact).  mix_perm [B] int32 and mix_lam [B] float32 are
 * device buffers, 4-byte aligned; an entry of mix_perm outside [0, B) is clamped into it on the device (a wrong partner, never a read
 * out of bounds).  Every *_mix_* entry computes exactly what its plain counterpart computes on x'.
 *
 * leaf_mixup_f32: x' itself, out [B][T] float32, one pass (read two clips, write one).  flags: 0 or LEAF_FLAG_X_PCM16.
 *
 * leaf_forward_mix_f32 / leaf_forward_save_mix_f32 / leaf_backward_mix_f32: leaf_forward_f32 / leaf_forward_save_f32 /
 * leaf_backward_f32 on x', arguments as there plus the two buffers after x.  The static-geometry overlap-save kernels (FFT_SMALL,
 * FFT and FFT_WG at 401/160, 201/80 and 801/320, and the matching per-wave and workgroup backwards) and the 4096-sample plans,
 * forward and backward, mix inside their loads: x' never exists in memory and an int16 batch stays int16 through a training step.
 * Every other selector and path (run-time-geometry kernels of the 2048-sample plan, MFMA, staged) first writes x' behind its own
 * workspace with the kernel of leaf_mixup_f32 and continues on it; the queries below include that copy where it is needed.  Workspace: leaf_forward_mix_workspace_bytes for the same selector,
 * leaf_backward_mix_workspace_bytes for the same flags.  LEAF_FLAG_OUT_BF16 (bfloat16 out / grad_out) is taken as by the plain entries.
 * LEAF_ERR_UNSUPPORTED: LEAF_FLAG_IO_BF16 (the mix is defined in fp32),
 * LEAF_FLAG_PEAKNORM (the normalisation would have to follow the mix) and g_x != NULL (dL/dx would be a scatter over mix_perm, and
 * x is data here).  B == 0 is the empty batch as everywhere; mix_perm and mix_lam may then be NULL.
 */
int leaf_mixup_f32(const void* x, int B, int T, const int* mix_perm /*[B]*/, const float* mix_lam /*[B]*/, int flags,
                   float* out, void* stream);
size_t leaf_forward_mix_workspace_bytes(int B, int T, int F, int K, int hop, int algo);
int leaf_forward_mix_f32(const void* x, const int* mix_perm /*[B]*/, const float* mix_lam /*[B]*/, int B, int T,
                         const float* kernel, const float* pool_w, const float* pool_b,
                         const float* alpha, const float* delta, const float* root, const float* ema_w,
                         int F, int K, int hop, int flags, int algo,
                         float* out, void* workspace, size_t workspace_bytes, void* stream);
int leaf_forward_save_mix_f32(const void* x, const int* mix_perm /*[B]*/, const float* mix_lam /*[B]*/, int B, int T,
                              const float* kernel, const float* pool_w, const float* pool_b,
                              const float* alpha, const float* delta, const float* root, const float* ema_w,
                              int F, int K, int hop, int flags, int algo,
                              float* out, float* pooled_raw, void* workspace, size_t workspace_bytes, void* stream);
size_t leaf_backward_mix_workspace_bytes(int B, int T, int F, int K, int hop, int flags);
int leaf_backward_mix_f32(const void* x, const int* mix_perm /*[B]*/, const float* mix_lam /*[B]*/, int B, int T,
                          const float* kernel, const float* pool_w, const float* pool_b,
                          const float* alpha, const float* delta, const float* root, const float* ema_w,
                          int F, int K, int hop, int flags, const float* grad_out,
                          const float* pooled_raw /* from leaf_forward_save_mix_f32, or NULL = recompute */,
                          float* g_kernel, float* g_pool_w, float* g_pool_b,
                          float* g_alpha, float* g_delta, float* g_root, float* g_ema_w,
                          float* g_x /* must be NULL */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Stage entry points (each is one reference module's forward; they are what the sub-modules of
 * leaf_pytorch_amd.Leaf call when used on their own, and what the parity tests probe).
 */

/* convolution.py:15-22 + impulse_responses.py:5-16,19-63,66-71: constrained Gabor taps,
 * taps [2F][K], row 2f = Re h_f, row 2f+1 = Im h_f (the layout convolution.py:88-90 feeds conv1d). */
int leaf_gabor_taps_f32(const float* kernel, int F, int K, float* taps, void* stream);

/* impulse_responses.py:74-80: un-normalised Gaussian pooling windows, window [F][K]. */
int leaf_lowpass_window_f32(const float* pool_w, int F, int K, float* window, void* stream);

/* convolution.py:71-99 (GaborConv1d.forward): y [B][2F][T], zero "same" padding, stride 1, no bias.
 * workspace must hold 2*F*K floats. */
int leaf_gabor_conv_f32(const float* x, int B, int T, const float* kernel, int F, int K,
                        float* y, void* workspace, size_t workspace_bytes, void* stream);

/* frontend.py:15-19 (SquaredModulus.forward): y [B][2F][T] -> e [B][F][T] = re^2 + im^2. */
int leaf_squared_modulus_f32(const float* y, int B, int F, int T, float* e, void* stream);

/* pooling.py:31-42 (GaussianLowPass.forward): e [B][F][T] -> pooled [B][F][T'] (+bias, no floor).
 * pool_b may be NULL (use_bias=False).  workspace must hold F*K floats. */
int leaf_gaussian_lowpass_f32(const float* e, int B, int F, int T, const float* pool_w, const float* pool_b,
                              int K, int hop, float* pooled, void* workspace, size_t workspace_bytes,
                              void* stream);

/* postprocessing.py:13-28 (ExponentialMovingAverage.forward): p [B][F][T'] -> ema [B][F][T']. */
int leaf_ema_f32(const float* p, int B, int F, int TP, const float* ema_w, float* ema, void* stream);

/* postprocessing.py:62-69 (PCENLayer.forward) with floor = `floor_` (frontend.py:70 passes 1e-12):
 * p [B][F][T'] -> out [B][F][T']. */
int leaf_pcen_f32(const float* p, int B, int F, int TP, const float* alpha, const float* delta,
                  const float* root, const float* ema_w, float floor_, float* out, void* stream);

/* postprocessing.py:62-69 with the smoother's state handed in and out, for CHUNKED real-time use of the frontend (SURVEY 8f:
 * "very-long-clip time tiling with EMA carry"): p [B][F][n] are the floored pooled frames of one chunk of a running stream,
 * ema_in [B][F] the smoother state after the previous chunk (NULL at the start of a stream: the state starts at the first
 * frame, postprocessing.py:15), ema_out [B][F] receives the state after this chunk (may alias ema_in).  The arithmetic is
 * the fused paths' (the reference's recurrence in its fp32 operation order; the cancellation-free PCEN form), so a stream
 * fed in chunks equals the same frames finalized in one call.  alpha == NULL: no PCEN, out = log1p(p) if `log1p_` else p
 * (then ema_in / ema_out / the PCEN parameters are ignored). */
int leaf_pcen_stream_f32(const float* p, int B, int F, int n, const float* alpha, const float* delta, const float* root,
                         const float* ema_w, float floor_, int log1p_, const float* ema_in, float* ema_out, float* out,
                         void* stream);

/*
 * One-launch streaming step (additive: the ABI version stays 6).  A running stream of B waveforms is fed chunk by chunk; the
 * waveform history the next frames still need and the PCEN smoother's state stay ON THE DEVICE, in a `state` buffer the caller
 * owns; WHERE the stream stands stays on the host, in six integers the caller carries from call to call (nothing is read back
 * from the device, nothing synchronises, there is no workspace).  Static geometries of the one-launch kernel only (K = 401 /
 * hop = 160, K = 201 / hop = 80); every other geometry: LEAF_ERR_UNSUPPORTED, and leaf_stream_state_bytes answers 0.
 *
 * leaf_stream_history_samples(K, hop): the most samples a stream can owe its next step, H = 2 (K - 1 - padL) + ceil(2 padL / hop) hop
 *   (880 at 401 / 160): a frame is final once sample m hop + 2 (K - 1 - padL) has arrived, and the buffer is kept from a whole
 *   number of hops, at least 2 padL samples, in front of the next frame (the derivation is next to the function).  Any K, hop >= 1.
 * leaf_stream_state_bytes(B, F, K, hop, flags): two history halves of [B][H] samples in the sample type `flags` names (float32, or
 *   int16 with LEAF_FLAG_X_PCM16) and [B][F] float32 smoother state, each region starting at a multiple of 256 bytes.  The buffer
 *   may hold anything when a stream begins: a step with hist_len = 0 and started = 0 reads none of it.  0: nothing to size -- a
 *   geometry without the kernel, B < 1 or F < 1, or a flag the step refuses (LEAF_FLAG_IO_BF16, LEAF_FLAG_PEAKNORM).
 *
 * leaf_stream_step_f32: the step's signal is the virtual concatenation [history (hist_len samples per stream, in history half
 *   `parity`) | chunk[b][0 .. Tc)], chunk row b starting `chunk_stride` samples behind row b - 1 (a slice of a longer recording goes
 *   in without a copy; Tc = 0: chunk may be NULL).  Frames first .. first + n - 1, numbered from the virtual buffer's first
 *   sample as in a clip of hist_len + Tc samples, are written to out [B][F][n], every element (n = 0: out is not touched and may
 *   be NULL); with LEAF_FLAG_PCEN the smoother starts from the state the previous step left when `started` is 1 and at the first
 *   emitted frame otherwise (postprocessing.py:15), and leaves its state after frame first + n - 1.  Samples
 *   [drop_samples, hist_len + Tc) of the virtual buffer are copied to the OTHER history half: the next call passes
 *   hist_len' = hist_len + Tc - drop_samples and parity' = 1 - parity.  Samples behind the virtual buffer's end count as the
 *   reference's zero padding, which is what the final step of a stream wants (Tc = 0, every remaining frame) and concerns no
 *   frame whose receptive field is complete.  leaf_pytorch_amd/streaming.py: stream_plan() is the arithmetic of the six integers.
 *   Flags: LEAF_FLAG_PCEN, LEAF_FLAG_LOG1P, LEAF_FLAG_X_PCM16 (chunk and history are int16), LEAF_FLAG_OUT_BF16 (out is
 *   bfloat16); LEAF_FLAG_IO_BF16 and LEAF_FLAG_PEAKNORM: LEAF_ERR_UNSUPPORTED.  Checks in this order, all before the launch:
 *   unsupported flag or geometry; B = 0 (LEAF_OK, nothing launched); NULL; shape; alignment (state 16 bytes, chunk and out by
 *   element); the position -- hist_len > H, hist_len + Tc beyond one pass of the kernel (16000 samples), drop_samples >
 *   hist_len + Tc, a new history longer than H, frames outside the virtual buffer: LEAF_ERR_BAD_SHAPE; state_bytes below
 *   leaf_stream_state_bytes: LEAF_ERR_WORKSPACE.  One launch per call, also when n = 0 (then only the history moves); the one
 *   exception is a call with nothing to emit AND nothing to keep (n = 0 and drop_samples = hist_len + Tc: the end of a stream that
 *   owes no frame): LEAF_OK, nothing launched.  Steps of one stream must execute in order (one HIP stream, or events).
 */
int leaf_stream_history_samples(int K, int hop);
size_t leaf_stream_state_bytes(int B, int F, int K, int hop, int flags);
int leaf_stream_step_f32(const void* chunk, int B, int Tc, long long chunk_stride, void* state, size_t state_bytes, int hist_len,
                         int parity, int drop_samples, int first, int n, int started, const float* kernel, const float* pool_w,
                         const float* pool_b, const float* alpha, const float* delta, const float* root, const float* ema_w, int F,
                         int K, int hop, int flags, void* out, void* stream);

/*
 * The bank: one step of B INDEPENDENT streams in one launch (additive: the ABI version stays 6).  leaf_stream_step_f32 moves B
 * streams in lock-step; here every slot b stands at a position of its own -- streams begin and end at different times, take chunks
 * of different lengths, or take nothing in a step -- described by slots[b], a HOST array of B records that the call reads before it
 * returns (the records travel to the kernel by value: no plan buffer on the device, no copy, no readback, nothing synchronises).
 * `state` has the layout and size of leaf_stream_state_bytes(B, F, K, hop, flags); slot b owns row b of both history halves and row
 * b of the smoother state, and carries a parity of its own.  Geometries and flags are those of leaf_stream_step_f32.
 *
 * A slot's record:
 *   idle = 1: the slot takes no part in the step.  Nothing of its state is read or written, no other field of the record is looked
 *     at, its rows of out are zeros; the caller leaves its parity as it is.
 *   idle = 0: hist_len, Tc, parity, drop_samples, first, n, started mean what leaf_stream_step_f32's arguments mean, for this slot
 *     alone: the signal is [history (hist_len samples of row b of half `parity`) | chunk[b * chunk_stride .. + Tc)], frames first ..
 *     first + n - 1 of it are emitted, samples [drop_samples, hist_len + Tc) go to row b of the other half, and the caller flips the
 *     slot's parity.  Only the first Tc samples of a chunk row are read.  A slot whose stream begins passes hist_len = 0 and
 *     started = 0 and reads nothing of the state.
 *   end_n > 0: the stream ENDS with this step, on a chunk that also completed frames.  After the step's frames, frames end_first ..
 *     end_first + end_n - 1 of the buffer made of the samples [drop_samples, hist_len + Tc) -- numbered from that buffer's first
 *     sample, with the reference's zero padding behind its last -- are emitted by the same workgroups, with the smoother carried on;
 *     nothing is handed over to the other half.  These are the frames, bit for bit, that a final leaf_stream_step_f32 (Tc = 0) on
 *     the handed-over history would give.  (A stream that ends without the step completing a frame needs no second pass: n counts
 *     all its remaining frames and drop_samples = hist_len + Tc.)
 * out is [B][F][n_max] (float32, or bfloat16 with LEAF_FLAG_OUT_BF16): row (b, f) holds the slot's n + end_n frames, then zeros up to
 * n_max; EVERY element of out is written.  n_max = 0: out is not touched and may be NULL.  chunk may be NULL when no slot has samples.
 *
 * Checks, all on the host before anything is launched, in leaf_stream_step_f32's order: unsupported flag or geometry; B = 0
 * (LEAF_OK); NULL (slots, state, parameters; chunk when a slot has Tc > 0; out when n_max > 0); shape (B, F, n_max, a slot's idle
 * or Tc, chunk_stride below the longest Tc when B > 1); alignment; then per slot every position of leaf_stream_step_f32's list, the
 * ending pass's frames inside its buffer, n + end_n <= n_max, and the kernel's LDS at n_max: LEAF_ERR_BAD_SHAPE -- one bad slot
 * refuses the whole call; state_bytes: LEAF_ERR_WORKSPACE.  A bank of more than 128 slots is served by several launches (128 pass
 * records each; an ending pass is a record of its own); a call in which no slot emits or keeps anything (n_max = 0 and every slot
 * idle or drop_samples = hist_len + Tc) launches nothing.  Steps on one `state` must execute in order.
 */
typedef struct leaf_stream_slot {
    int idle;
    int hist_len, Tc, parity, drop_samples, first, n, started;
    int end_first, end_n;
} leaf_stream_slot;
int leaf_stream_bank_step_f32(const void* chunk, long long chunk_stride, int B, const leaf_stream_slot* slots, int n_max, void* state,
                              size_t state_bytes, const float* kernel, const float* pool_w, const float* pool_b, const float* alpha,
                              const float* delta, const float* root, const float* ema_w, int F, int K, int hop, int flags, void* out,
                              void* stream);

/*
 * Stage backwards: the gradient autograd derives for each of the modules above when it is called ON ITS OWN (the
 * reference's sub-modules are ordinary differentiable nn.Modules; Leaf.forward as a whole has leaf_backward_f32).
 * One-lane-per-output kernels, every intermediate materialised; clamp sub-gradients as torch.clamp gives them.
 * Nullable outputs are skipped.  Workspace: leaf_stage_backward_workspace_bytes(stage, B, T, F, K, hop) -- for the EMA
 * and PCEN stages pass T = T' (frames) and K = hop = 1.
 */
#define LEAF_STAGE_GABOR_CONV 1
#define LEAF_STAGE_LOWPASS    2
#define LEAF_STAGE_EMA        3
#define LEAF_STAGE_PCEN       4
size_t leaf_stage_backward_workspace_bytes(int stage, int B, int T, int F, int K, int hop);

/* convolution.py:71-99 backward: grad_y [B][2F][T] -> g_kernel [F][2] (through impulse_responses.py:5-16 and the clamps
 * of convolution.py:15-22; nullable), g_x [B][T] (nullable). */
int leaf_gabor_conv_backward_f32(const float* x, int B, int T, const float* kernel, int F, int K, const float* grad_y,
                                 float* g_kernel, float* g_x, void* workspace, size_t workspace_bytes, void* stream);

/* frontend.py:15-19 backward: grad_y [B][2F][T] = 2 y grad_e (grad_e [B][F][T] broadcast over the re/im pair). */
int leaf_squared_modulus_backward_f32(const float* y, const float* grad_e, int B, int F, int T, float* grad_y,
                                      void* stream);

/* pooling.py:31-42 backward: grad_pooled [B][F][T'] -> g_e [B][F][T] (nullable), g_pool_w [F] (through
 * impulse_responses.py:74-80 incl. its clamp; nullable), g_pool_b [F] (nullable). */
int leaf_gaussian_lowpass_backward_f32(const float* e, const float* grad_pooled, int B, int F, int T,
                                       const float* pool_w, int K, int hop, float* g_e, float* g_pool_w,
                                       float* g_pool_b, void* workspace, size_t workspace_bytes, void* stream);

/* postprocessing.py:13-28 backward: grad_ema [B][F][T'] -> g_p [B][F][T'], g_ema_w [F] (per-channel coefficient; the
 * host sums it for a shared one). */
int leaf_ema_backward_f32(const float* p, const float* grad_ema, int B, int F, int TP, const float* ema_w, float* g_p,
                          float* g_ema_w, void* workspace, size_t workspace_bytes, void* stream);

/* postprocessing.py:62-69 backward (no 1e-5 floor in front: that one belongs to frontend.py:84). */
int leaf_pcen_backward_f32(const float* p, const float* grad_out, int B, int F, int TP, const float* alpha,
                           const float* delta, const float* root, const float* ema_w, float floor_, float* g_p,
                           float* g_alpha, float* g_delta, float* g_root, float* g_ema_w, void* workspace,
                           size_t workspace_bytes, void* stream);

/*
 * Inference with frozen parameters (serving): everything derived from (kernel, pool_w) alone -- the filter spectra and
 * the pooling rows of the overlap-save path -- is prepared once into a caller-owned `tables` buffer and reused by every
 * forward, which then skips the table kernel (7 us: 2 % of a 256-clip batch, 20 % of a 4-clip one).  The caller is
 * responsible for preparing again after the parameters change.  Same arithmetic, bit-identical outputs.
 * leaf_fft_tables_bytes returns 0 when the overlap-save path does not cover the geometry (use leaf_forward_f32).
 */
size_t leaf_fft_tables_bytes(int F, int K, int hop);
int leaf_fft_prepare_tables_f32(const float* kernel /*[F][2]*/, const float* pool_w /*[F]*/, int F, int K, int hop,
                                void* tables, size_t tables_bytes, void* stream);
/* x is float32, bfloat16 with LEAF_FLAG_IO_BF16 (then out is bfloat16 too) or int16 with LEAF_FLAG_X_PCM16 (out stays float32);
 * LEAF_FLAG_OUT_BF16 makes out bfloat16 for a float32 or int16 x; workspace >= leaf_workspace_bytes(...,
 * LEAF_ALGO_FFT). */
int leaf_forward_prepared_f32(const float* x, int B, int T, const void* tables, size_t tables_bytes,
                              const float* pool_b, const float* alpha, const float* delta, const float* root,
                              const float* ema_w, int F, int K, int hop, int flags, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);

/* utilities/data/raw_transforms.py:334-345 (PeakNormalization, apply_to="only_too_loud_sounds"; the last transform of
 * every reference data pipeline, there on the CPU through the third-party torch_audiomentations): clips whose peak |x|
 * exceeds 1 are divided by their peak, others are copied unchanged.  x, out [B][T]; out may alias x. */
int leaf_peak_normalize_f32(const float* x, int B, int T, float* out, void* stream);

/* Batch assembly from a packed sample store (additive: the ABI version stays 6).  utilities/data/raw_transforms.py per clip, in
 * the order of get_raw_transforms_v2 -- PadToSize, RandomCrop / CenterCrop, RandomGain, PeakNormalization, TimeMasking -- in ONE
 * launch, one workgroup per clip: the (B, size) float32 batch the forward entries take, from recordings of any length that lie
 * back to back in `store`.  The random draws are the caller's (the plan below); the library applies them.
 *
 *   store     [store_len] samples, float32, or int16_t with flags = LEAF_FLAG_X_PCM16 (a sample v means v / 32768, as everywhere)
 *   rec_off   [B] int64: first sample of clip b's recording in the store      rec_len  [B] int32: its length L
 *   start     [B] int32: crop offset in the padded recording                  pad_mode [B] int32: 0 zero, 1 min, 2 replicate, 3 wrap
 *   gain      [B] float32 linear factors, or NULL                             normalize: 0 / 1
 *   masks     [B][M][2] int32 spans (t0, n), or NULL with M = 0              out      [B][size] float32
 *
 * With r[j] = store[rec_off[b] + j], S = size, P = max(S - L, 0), left = P / 2 and Lp = max(L, S), for t in [0, S):
 *   1. pad and crop: j = start[b] + t - left; 0 <= j < L gives r[j]; otherwise (only when L < S) the pad mode decides: 0 -> 0;
 *      1 -> min(r) over the whole recording (the reference's 'constant', which pads with signal.min()); 2 -> r[clamp(j, 0, L - 1)]
 *      (torch F.pad 'replicate': what the reference's torch PadToSize(mode='wrap') does); 3 -> r[j mod L], floor modulus, any
 *      number of periods (numpy.pad 'wrap': PadToSize_NP);
 *   2. gain: y = v * gain[b], one fp32 multiply (skipped for gain == NULL);
 *   3. normalize != 0: peak = max |y| over the S samples; peak > 1 gives y * (1 / peak), else y unchanged -- bit for bit
 *      leaf_peak_normalize_f32 on the clips of step 2;
 *   4. masks: y[max(t0, 0) : min(t0 + n, S)] = 0 per span; n <= 0 masks nothing.  The peak of step 3 is taken before the masks.
 *
 * MEMORY SAFETY.  The plan is device memory, which the library cannot inspect, so the kernel clamps it: rec_off into
 * [0, store_len], rec_len into [0, store_len - rec_off], start into [0, Lp - S]; a pad_mode outside 0..3 counts as 0; a recording
 * of clamped length 0 gives a clip of zeros (its min is 0).  Whatever the plan holds, nothing outside store[0, store_len) is read
 * and nothing outside out[B][size] is written.
 *
 * Clips of up to 32765 samples stay in registers between the peak and the store (the store is read once); longer ones, any
 * size < 2^31, are gathered twice (the second time from L2 where they fit).  One workgroup works on one clip whatever its
 * length: a few long clips use a few CUs.
 *
 * No workspace.  Alignment: element alignment as everywhere -- store 4 bytes (2 for int16), rec_off 8, every other buffer 4.
 * Status: LEAF_ERR_UNSUPPORTED for a flag other than LEAF_FLAG_X_PCM16; LEAF_ERR_NULL_POINTER; LEAF_ERR_BAD_SHAPE for B < 1,
 * size < 1, store_len < 0, M < 0, or M > 0 with masks == NULL (B == 0 is the caller's to skip: there is nothing to write);
 * LEAF_ERR_ALIGNMENT -- in that order, before any launch.  out must not overlap store. */
int leaf_assemble_clips_f32(const void* store, long long store_len, int flags, int B, int size, const long long* rec_off,
                            const int* rec_len, const int* start, const int* pad_mode, const float* gain, int normalize,
                            const int* masks, int M, float* out, void* stream);

/* The same launch with the reference's two noise transforms in it (additive: the ABI version stays 6): AddRandomNoise -- a background
 * recording mixed in at an SNR, get_raw_transforms_v2 -- and AddGaussianNoise (leaf_supervised_transforms, simple_supervised_transforms).
 * Both sit in front of the peak normalisation, so they cannot be appended behind leaf_assemble_clips_f32.  The arguments of that entry
 * up to `out` come first and mean what they mean there; `stream` stays last.  Behind `out`:
 *
 *   noise_store     [noise_store_len] samples of the background recordings, of the SAME sample type as `store` (flags decides for both)
 *   noise_off       [B] int64, noise_len [B] int32, noise_start [B] int32, noise_pad_mode [B] int32: clip b's noise recording and how it
 *                   is padded and cropped to `size` -- the rule of step 1, on its own plan (the reference: PadToSize(size, 'wrap'), which
 *                   is mode 2 here, then RandomCrop(size))
 *   noise_coeff     [B][2] float32: c = fp32(coeff) and c' = fp32(1 - coeff), the subtraction in double -- what the reference's
 *                   `coeff * x + (1.0 - coeff) * noise` multiplies with for a numpy float64 coeff = r / (1 + r), r = 10^(snr / 10)
 *   gauss_amp       [B] float32 amplitudes            gauss_seed: 64 bits            gauss_stream [B] int64: one stream id per clip
 *
 * The noise group (noise_store .. noise_coeff) is given or NULL as a whole, and so is the Gaussian group (gauss_amp, gauss_stream);
 * with both NULL the call IS leaf_assemble_clips_f32.  The steps, for clip b and t in [0, S):
 *   1.  pad and crop, as above;
 *   1a. background noise, for a clip whose clamped noise_len > 0: y = rn(rn(c v) + rn(c' n[t])), n the noise recording through step 1 --
 *       three separately rounded fp32 operations, no fused multiply-add.  A clip with noise_len <= 0 skips the step (it does not compute
 *       1 v + 0 n, which would change the sign of a zero);
 *   2.  gain, as above;
 *   2a. Gaussian noise, for gauss_amp[b] != 0: y = rn(y + rn(gauss_amp[b] z[b][t])), two separately rounded operations; amplitude 0 skips;
 *   3., 4. peak normalisation of the result, then the masks, as above.
 * A clip that skips 1a and 2a has the bits leaf_assemble_clips_f32 gives it.
 *
 * THE STREAM is exact by definition: z[b][t] depends on (gauss_seed, gauss_stream[b], t) and on nothing else -- not on B, the clip's
 * place in the batch, size, the path, or the alignment of out.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 * 0x9E3779B9 / 0xBB67AE85) with key (lo32(seed), hi32(seed)) and counter (t >> 2, 0, lo32(stream[b]), hi32(stream[b])); its outputs
 * r0..r3 give the normals of row elements 4 g .. 4 g + 3: u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, rho = sqrt(-2 ln u1),
 * z0 = rho cos(2 pi u2), z1 = rho sin(2 pi u2); r2, r3 give z2, z3 the same way.  All fp32, the angle through sincospi(2 u2).  The integer
 * part is exact; the transcendental part is the device's (within 1e-5 of the formula in double: |z| <= 5.8).
 * leaf_gaussian_noise_f32 writes z itself, out [B][size] float32, from the same device function: the same bits.
 *
 * MEMORY SAFETY: the noise plan is clamped exactly as the clip plan (against noise_store_len): nothing outside either store is read,
 * nothing outside out[B][size] is written.  Both noises are computed chunk by chunk on the registers of the plain kernel: clips of
 * up to 32765 samples stay resident here too, longer ones compute the noise twice (the same bits both times).
 *
 * Alignment: noise_store as store, noise_off and gauss_stream 8 bytes, every other buffer 4.  Status, in this order, before any
 * launch: LEAF_ERR_UNSUPPORTED as above; LEAF_ERR_NULL_POINTER (also for a group given in part); LEAF_ERR_BAD_SHAPE (also for
 * noise_store_len < 0; leaf_gaussian_noise_f32: B < 1, size < 1); LEAF_ERR_ALIGNMENT.  out must not overlap either store. */
int leaf_assemble_clips_noise_f32(const void* store, long long store_len, int flags, int B, int size, const long long* rec_off,
                                  const int* rec_len, const int* start, const int* pad_mode, const float* gain, int normalize,
                                  const int* masks, int M, float* out, const void* noise_store, long long noise_store_len,
                                  const long long* noise_off, const int* noise_len, const int* noise_start, const int* noise_pad_mode,
                                  const float* noise_coeff /*[B][2]*/, const float* gauss_amp, unsigned long long gauss_seed,
                                  const long long* gauss_stream, void* stream);
int leaf_gaussian_noise_f32(int B, int size, unsigned long long seed, const long long* stream_ids /*[B]*/, float* out /*[B][size]*/,
                            void* stream);

/* Whole-recording evaluation batches from the same packed store (additive: the ABI version stays 6).  The reference's test.py
 * evaluates a recording r of L samples as a whole: PeakNormalization over the recording (ONE peak per recording), pad_input --
 * n = ceil(L / S) rows of S = sample_rate samples, P = n S, left = (P - L) / 2, F.pad(r, (left, P - L - left), 'replicate'),
 * reshape(-1, 1, S) -- the model on the n rows, and the mean of its outputs.  Two entries restate the data side: the recordings'
 * peaks, once per dataset, and the rows of any number of recordings in one launch.
 *
 * leaf_clip_peaks_f32: peaks[i] = max |r_i[j]| over recording i, r_i[j] = store[rec_off[i] + j], 0 <= j < rec_len[i]; a recording
 * of no samples gives 0.  The result is exact (max does not depend on the order); a NaN sample is ignored, as fmaxf ignores it in
 * leaf_peak_normalize_f32; an int16 store (LEAF_FLAG_X_PCM16, v / 32768) has no peak above 1.  The work is split by tiles of 1024
 * samples, one wave each, not by recording: one long recording spreads over the chip, a short one costs one wave.  Two launches:
 * the tile prefix of the clamped plan into the workspace, then the tiles, folded into peaks[] by an integer max on the bit pattern
 * of the non-negative floats (no float atomics).
 *
 *   store, store_len, flags: as in leaf_assemble_clips_f32          R: the number of recordings
 *   rec_off  [R] int64, rec_len [R] int32: the recordings           peaks [R] float32, out
 *   workspace: leaf_clip_peaks_workspace_bytes(R) = 8 (R + 1) bytes (0 for R < 1), overwritten
 *
 * MEMORY SAFETY: rec_off and rec_len are device memory and are clamped exactly as in leaf_assemble_clips_f32 (rec_off into
 * [0, store_len], rec_len into [0, store_len - rec_off]): nothing outside store[0, store_len) is read, nothing outside peaks[0, R)
 * and the workspace is written.  Alignment: store 4 bytes (2 for int16), rec_off 8, rec_len and peaks 4, workspace 16.  Status, in
 * this order, before any launch: LEAF_ERR_UNSUPPORTED for a flag other than LEAF_FLAG_X_PCM16; LEAF_ERR_NULL_POINTER (store, rec_off,
 * rec_len, peaks); LEAF_ERR_BAD_SHAPE for R < 1 or store_len < 0; LEAF_ERR_ALIGNMENT; LEAF_ERR_WORKSPACE for a workspace that is NULL
 * or below the size query.  peaks and the workspace must not overlap the store or the plan. */
size_t leaf_clip_peaks_workspace_bytes(int R);
int leaf_clip_peaks_f32(const void* store, long long store_len, int flags, int R, const long long* rec_off /*[R]*/,
                        const int* rec_len /*[R]*/, float* peaks /*[R]*/, void* workspace, size_t workspace_bytes, void* stream);

/* leaf_assemble_segments_f32: `rows` rows of `size` samples, each a window of one recording.
 *
 *   rec_off  [rows] int64, rec_len [rows] int32: the row's recording (repeated for each of its rows)
 *   win      [rows] int64: the recording's sample the row starts at; it may lie before the recording or behind it.  test.py's
 *            row k of a recording is win = k S - left
 *   peaks    [R] float32 (leaf_clip_peaks_f32) or NULL; rec [rows] int32: the row's entry of peaks (read only with peaks != NULL)
 *   out      [rows][size] float32
 *
 * With r[j] = store[rec_off[b] + j] and L = rec_len[b], for row b and t in [0, size):
 *   1. v = r[clamp(win[b] + t, 0, L - 1)] -- F.pad 'replicate' on either side; L == 0 gives zeros;
 *   2. peaks != NULL: p = peaks[clamp(rec[b], 0, R - 1)]; p > 1 gives v * (1 / p), else v unchanged -- the arithmetic of
 *      leaf_peak_normalize_f32 with the recording's peak in place of the row's.  Padding a scaled recording by replication equals
 *      scaling the padded one, so the rows have the bits of test.py's order of operations.
 *
 * Nothing is reduced: a row longer than one tile of 32768 samples is split over workgroups (grid = rows x tiles), on the 16-byte
 * chunk grid aligned in `out` and with the element-aligned source loads of leaf_assemble_clips_f32.  No workspace.
 *
 * MEMORY SAFETY: the plan is clamped by the kernel -- rec_off and rec_len as in leaf_assemble_clips_f32, win into [-size, L] (a
 * window further out reads the same samples), rec into [0, R - 1]; win + t is formed in 64 bits from the clamped win.  Whatever
 * the plan holds, nothing outside store[0, store_len) or peaks[0, R) is read and nothing outside out[rows][size] is written.
 * Alignment: store 4 bytes (2 for int16), rec_off and win 8, every other buffer 4.  Status, in this order, before any launch:
 * LEAF_ERR_UNSUPPORTED for a flag other than LEAF_FLAG_X_PCM16; LEAF_ERR_NULL_POINTER (store, rec_off, rec_len, win, out; rec with
 * peaks != NULL); LEAF_ERR_BAD_SHAPE for rows < 1, size < 1, store_len < 0, R < 1 with peaks != NULL, or rows x tiles >= 2^31;
 * LEAF_ERR_ALIGNMENT.  out must not overlap the store. */
int leaf_assemble_segments_f32(const void* store, long long store_len, int flags, int rows, int size, const long long* rec_off,
                               const int* rec_len, const long long* win, const float* peaks /*[R] or NULL*/, const int* rec, int R,
                               float* out /*[rows][size]*/, void* stream);

/* Waveform standardisation in the assembly launches (additive: the ABI version stays 6).  The reference's RawAudioParser with
 * audio_config.normalize (utilities/data/raw_waveform_parser.py:16-23) maps the WHOLE recording r of L samples, as loaded and in
 * front of every other transform, to (r - mean) / (std + 1e-9), std torch's unbiased one.  A clip cut from such a recording depends
 * on samples outside the clip, so the step cannot be appended by the caller: the recordings' moments are computed once per dataset
 * (leaf_clip_moments_f32), and two entries apply the map inside the launches of the entries above.  "Recording" always means the
 * recording as packed in the store.
 *
 * leaf_clip_moments_f32: moments[i] = (mean_i, std_i, min_i, max_i), four float32 per recording, for all R recordings in one call.
 *   mean_i = fp32(sum r / L), the sum in float64;
 *   std_i  = fp32(sqrt(sum (r - m)^2 / (L - 1))), evaluated in float64, m the float64 mean BEFORE its rounding: two passes over the
 *            samples, not sum r^2 - (sum r)^2 / L;
 *   min_i, max_i: exact.  An int16 sample v means v / 32768, as everywhere.
 *   L == 1: std = NaN (0 / 0, as torch);  L == 0: (0, NaN, 0, 0).  A NaN sample makes the mean and the std NaN -- nothing is ignored,
 *   the recording standardises to NaN as in the reference; min and max skip NaN samples (fminf / fmaxf; a recording of NaNs alone
 *   gives +inf, -inf), which no result depends on behind a NaN mean.
 * THE ORDER OF THE ADDITIONS is fixed by L alone: the recording's tiles of 1024 samples are dealt to 32 spans of
 * ceil(ceil(L / 1024) / 32) consecutive tiles; one wave sums one span -- every lane its samples 4 lane + 256 u + 1024 t + e in
 * index order, then a butterfly over the 64 lanes -- into the span's slot of the workspace, and one lane folds the 32 slots in slot
 * order.  No atomics: the result does not depend on the grid, on the store's alignment, on the other recordings or on the run.
 * Four launches (partials and fold, for the sum and for the squared deviations); the float64 means are kept in the workspace between
 * them.
 *
 *   store, store_len, flags, R, rec_off, rec_len: as in leaf_clip_peaks_f32          moments [R][4] float32, out
 *   workspace: leaf_clip_moments_workspace_bytes(R) = 520 R bytes (32 slots of 16 bytes and one float64 per recording; 0 for
 *   R < 1), overwritten
 *
 * MEMORY SAFETY: rec_off and rec_len are clamped exactly as in leaf_clip_peaks_f32: nothing outside store[0, store_len) is read,
 * nothing outside moments[R][4] and the workspace is written.  Alignment: store 4 bytes (2 for int16), rec_off 8, rec_len and
 * moments 4, workspace 16.  Status, in this order, before any launch: LEAF_ERR_UNSUPPORTED for a flag other than LEAF_FLAG_X_PCM16;
 * LEAF_ERR_NULL_POINTER (store, rec_off, rec_len, moments); LEAF_ERR_BAD_SHAPE for R < 1 or store_len < 0; LEAF_ERR_ALIGNMENT;
 * LEAF_ERR_WORKSPACE for a workspace that is NULL or below the size query. */
size_t leaf_clip_moments_workspace_bytes(int R);
int leaf_clip_moments_f32(const void* store, long long store_len, int flags, int R, const long long* rec_off /*[R]*/,
                          const int* rec_len /*[R]*/, float* moments /*[R][4]*/, void* workspace, size_t workspace_bytes,
                          void* stream);

/* leaf_assemble_clips_std_f32: leaf_assemble_clips_noise_f32 on the standardised recording.  The arguments of that entry up to
 * gauss_stream come first and mean what they mean there; `stream` stays last.  Between them the standardisation group:
 *
 *   moments      [R][4] float32 (leaf_clip_moments_f32)
 *   moments_rec  [B] int32: clip b's row of moments, i.e. the recording its rec_off / rec_len name          R: rows of moments
 *
 * The group is given or NULL as a whole (in part: LEAF_ERR_NULL_POINTER); with it NULL the call IS leaf_assemble_clips_noise_f32
 * (and without that entry's groups, leaf_assemble_clips_f32).  With i = clamp(moments_rec[b], 0, R - 1):
 *   0.  d = rn(std_i + 1e-9f), one fp32 add per clip; every sample v of the clip's recording becomes y = rn(rn(v - mean_i) / d): one
 *       fp32 subtraction and one CORRECTLY ROUNDED fp32 division per sample -- no reciprocal multiply, no contraction.  This is bit
 *       for bit (r - mean) / (std + 1e-9) evaluated by torch in float32 on 0-d float32 tensors holding moments[i];
 *   1.  pad and crop, on the standardised samples.  Mode 1 ('min') pads with rn(rn(min_i - mean_i) / d), the minimum of the
 *       standardised recording exactly (the map is monotone in fp32); mode 0 still pads with 0; modes 2 and 3 are index rules;
 *   1a. .. 4. as in leaf_assemble_clips_noise_f32.  The NOISE recording is not standardised (the reference builds its noise generator
 *       with normalize_waveform=False).  The peak normalisation of step 3 is live for an int16 store too: standardised samples
 *       leave [-1, 1].
 * The map is applied where a sample is loaded, on the resident and on the re-reading path alike (the same bits on both).  A clip
 * whose std is NaN (L == 1) or whose recording holds a NaN is NaN throughout, as in the reference.
 *
 * MEMORY SAFETY: as leaf_assemble_clips_noise_f32, and moments_rec is clamped into [0, R - 1]: nothing outside moments[R][4] is read.
 * Alignment: moments and moments_rec 4 bytes.  Status, in that entry's order (moments / moments_rec among the pointers, R < 1 among
 * the shapes), before any launch. */
int leaf_assemble_clips_std_f32(const void* store, long long store_len, int flags, int B, int size, const long long* rec_off,
                                const int* rec_len, const int* start, const int* pad_mode, const float* gain, int normalize,
                                const int* masks, int M, float* out, const void* noise_store, long long noise_store_len,
                                const long long* noise_off, const int* noise_len, const int* noise_start, const int* noise_pad_mode,
                                const float* noise_coeff /*[B][2]*/, const float* gauss_amp, unsigned long long gauss_seed,
                                const long long* gauss_stream, const float* moments /*[R][4]*/, const int* moments_rec /*[B]*/, int R,
                                void* stream);

/* leaf_assemble_segments_std_f32: leaf_assemble_segments_f32 on the standardised recording -- the parser in front of test.py's
 * PeakNormalization and pad_input.  The arguments of that entry up to `out` come first; behind `out`:
 *
 *   moments   [R][4] float32 or NULL; NULL: the call IS leaf_assemble_segments_f32 (normalize is not read)
 *   normalize 0 / 1: PeakNormalization over the whole standardised recording
 *
 * With moments, `rec` [rows] and R name the rows' entries of MOMENTS (rec is required), and peaks must be NULL
 * (LEAF_ERR_UNSUPPORTED: the raw recording's peak has no place behind the map).  For row b, i = clamp(rec[b], 0, R - 1):
 *   1. v = r[clamp(win[b] + t, 0, L - 1)], y = rn(rn(v - mean_i) / d), d = rn(std_i + 1e-9f) (replication commutes with the map);
 *      L == 0 gives zeros;
 *   2. normalize != 0: p = max(|rn(rn(min_i - mean_i) / d)|, |rn(rn(max_i - mean_i) / d)|), the peak of the standardised recording
 *      exactly (monotone map); p > 1 gives y * (1 / p), the arithmetic of leaf_peak_normalize_f32.  An int16 store is scaled too.
 * MEMORY SAFETY, alignment (moments 4 bytes) and status as leaf_assemble_segments_f32, with LEAF_ERR_UNSUPPORTED also for
 * peaks != NULL, rec among the required pointers and R < 1 among the shapes. */
int leaf_assemble_segments_std_f32(const void* store, long long store_len, int flags, int rows, int size, const long long* rec_off,
                                   const int* rec_len, const long long* win, const float* peaks /*NULL*/, const int* rec, int R,
                                   float* out /*[rows][size]*/, const float* moments /*[R][4] or NULL*/, int normalize, void* stream);

/* leaf_draw_clip_plan: the plan of the three assemble_clips entries drawn ON THE DEVICE (additive: the ABI version stays 6) -- the
 * random draws of the reference's training pipelines (pad mode, crop, gain, time masks, background noise, Gaussian amplitude) from a
 * counter-based generator and a step counter that lives in device memory, so that a training step that begins with its batch can be
 * captured into a graph and every replay draws a fresh plan.  One launch of ONE workgroup of 256 lanes that stride over the B clips;
 * no workspace, nothing read back, nothing reduced.
 *
 *   offsets [R] int64, lengths [R] int32: the clip store's recordings (device)
 *   noise_offsets [Rn] int64, noise_lengths [Rn] int32: the noise store's, or both NULL (then the noise outputs must be NULL too)
 *   index [B] int64: clip b's recording -- or NULL and order [N] int64, N >= 1: clip b is order[(step B + b) mod N] (unsigned 64-bit,
 *         wrapping).  Exactly one of index and order is given.  An entry is clamped into [0, R - 1], never trusted.
 *   state: ONE uint64 in device memory, the step counter.  Every lane reads step = state[0]; a workgroup barrier follows; then lane 0
 *         stores step + 1 (a plain store: one workgroup, nothing else to order).  advance == 0 leaves the counter alone.
 *   seed, stream_base: 64 bits each, by value.  size = S in [1, 2^31), train, the two pad modes (0..3), M <= 32 spans, and the
 *         probabilities and ranges below: by value, doubles.
 *
 * Outputs, in the dtypes the assemble entries take: rec_off int64, rec_len / start / pad_mode int32 (required); gain float32; masks
 * int32 [B][M][2] (required for M > 0); rec int32 (the clip's row of moments); the noise group noise_off int64, noise_len /
 * noise_start / noise_pad_mode int32, noise_coeff float32 [B][2] (given or NULL as a whole, together with noise_offsets /
 * noise_lengths); the Gaussian group gauss_amp float32, gauss_stream int64 (as a whole); index_out int64 [B], the recordings chosen
 * (the caller gathers its labels with it).  A NULL output or group is not drawn and not written.
 *
 * THE DRAWS are exact by definition.  Per clip b: id = stream_base + step B + b (unsigned 64-bit, wrapping).  P(q) is Philox4x32-10
 * (the rounds of THE STREAM above) with key (lo32(seed), hi32(seed)) and counter (q, 1, lo32(id), hi32(id)) -- counter word 1 is 1
 * here and 0 in the Gaussian stream, so id also serves as the clip's gauss_stream without the two domains meeting; r0..r3 are its
 * four words.  u(r) = r 2^-32 in double; a uniform integer in [0, n) is (uint64(r) n) >> 32, integers only.  With i the clip's
 * (clamped) recording, L = lengths[i] and span = max(L - S, 0):
 *   P(0):     pad_mode = u(r0) < wrap_pad_prob ? pad_mode_a : pad_mode_b;  start = train ? (r1 (span + 1)) >> 32 : span / 2;
 *             gain = u(r2) < gain_prob ? f32(exp((gain_db_lo + (gain_db_hi - gain_db_lo) u(r3)) (ln10 / 20))) : 1
 *   P(1):     used = 1 + ((r0 M) >> 32)
 *   P(2 + m): m < M: n_m = m < used ? min(S, floor((u(r0) time_perc) S)) : 0 (not below 0);  t0_m = floor(u(r1) double(S - n_m))
 *   P(64):    applied when u(r0) < noise_prob;  snr = snr_lo + (snr_hi + 1 - snr_lo) u(r1);  noise recording j = (r2 Rn) >> 32;
 *             noise_start = (r3 (nspan + 1)) >> 32, nspan = max(noise_lengths[j] - S, 0);  noise_len and noise_start are 0 where not
 *             applied;  noise_pad_mode = 2;  c = r / (1 + r), r = exp(snr (ln10 / 10));  noise_coeff = (f32(c), f32(1 - c))
 *   P(65):    gauss_amp = u(r0) < gauss_prob ? f32(gauss_amp_lo + (gauss_amp_hi - gauss_amp_lo) u(r1)) : 0;  gauss_stream = id
 * All floating point is IEEE double in the association written, no contraction, ln10 = 2.302585092994045684, each result rounded
 * once to float32.  The only inexact operations are the two exp: gain and noise_coeff are within one float32 ulp of the formula,
 * everything else is bit-exact.  csrc/leaf_clip_draws.hpp is this definition as host-and-device code.
 *
 * These are the distributions ClipSampler draws on the host, with 32-bit uniforms in place of 53-bit ones; neither its numbers nor
 * the reference's are reproduced.
 *
 * MEMORY SAFETY: index / order entries are clamped into [0, R - 1]; the noise recording is in [0, Rn - 1] by construction; nothing
 * outside the arrays above is read, nothing outside the outputs' B entries (masks: B M 2) and state[0] is written.  The lengths go out
 * as they are read: the assemble entries clamp them.  Alignment: 8 bytes for the int64 arrays and state, 4 for the others.
 * Status, in this order, before the launch: LEAF_ERR_NULL_POINTER (a required pointer; neither or both of index and order; a group
 * given in part); LEAF_ERR_BAD_SHAPE (B < 1, size < 1, R < 1, M < 0 or M > 32, M > 0 without masks, order with N < 1, the noise group
 * with Rn < 1, a pad mode outside 0..3); LEAF_ERR_ALIGNMENT. */
int leaf_draw_clip_plan(int B, int size, int train, const long long* offsets /*[R]*/, const int* lengths /*[R]*/, int R,
                        const long long* noise_offsets /*[Rn] or NULL*/, const int* noise_lengths, int Rn,
                        const long long* index /*[B] or NULL*/, const long long* order /*[N] or NULL*/, long long N,
                        unsigned long long* state, int advance, unsigned long long seed, unsigned long long stream_base,
                        int pad_mode_a, int pad_mode_b, double wrap_pad_prob, double gain_prob, double gain_db_lo, double gain_db_hi,
                        int M, double time_perc, double noise_prob, double snr_lo, double snr_hi,
                        double gauss_prob, double gauss_amp_lo, double gauss_amp_hi,
                        long long* rec_off, int* rec_len, int* start, int* pad_mode, float* gain, int* masks /*[B][M][2]*/, int* rec,
                        long long* noise_off, int* noise_len, int* noise_start, int* noise_pad_mode, float* noise_coeff /*[B][2]*/,
                        float* gauss_amp, long long* gauss_stream, long long* index_out, void* stream);

/* leaf_draw_mixup: mixup's permutation and weights drawn ON THE DEVICE (additive: the ABI version stays 6) -- what mix_perm and
 * mix_lam of the *_mix_f32 entries and leaf_mixup_f32 take, from the generator and the counter protocol of leaf_draw_clip_plan, so
 * that a step of sample, draw the mix, forward, backward captures into one graph and every replay mixes other pairs with other
 * weights.  One launch of ONE workgroup, as wide as its sort (64 to 1024 lanes); no workspace, nothing read back.
 *
 *   B in [1, 4096]; alpha finite and > 0: the weights are Beta(alpha, alpha), one per clip (the reference's do_mixup)
 *   state: ONE uint64 in device memory, the step counter, read and advanced exactly as by leaf_draw_clip_plan (every lane reads
 *         step = state[0]; a workgroup barrier; lane 0 stores step + 1 unless advance == 0).  A mixer keeps a counter of its own.
 *   seed, stream_base: 64 bits each, by value
 *   perm [B] int32, lam [B] float32: the outputs
 *
 * THE DRAWS.  Per clip b: id = stream_base + step B + b (unsigned 64-bit, wrapping); r0..r3 are the words of Philox4x32-10 with key
 * (lo32(seed), hi32(seed)) on the counter (0, 2, lo32(id), hi32(id)).  Counter word 1 is 2 here, 1 in leaf_draw_clip_plan and 0 in the
 * Gaussian stream: a mixer may share seed and ids with a sampler without sharing numbers.  r3 is not used.
 *
 * lam is Beta(alpha, alpha) without rejection, so a draw costs a fixed number of words.  If T is Student-t with 2 alpha degrees of
 * freedom, 1/2 + T / (2 sqrt(2 alpha + T^2)) is Beta(alpha, alpha), and Bailey's polar form gives
 * T = sqrt(2 alpha (U^(-1/alpha) - 1)) cos(2 pi V).  Multiplied through by U^(1/alpha), so that nothing overflows for a small alpha,
 * in IEEE double in exactly this association, no contraction:
 *       U = (r0 + 1) 2^-32   in (0, 1]             V = r1 2^-32
 *       w = pow(U, 1 / alpha)                      may underflow to 0, never above 1
 *       c = (r1 & 0x7FFFFFFF) == 0x40000000 ? 0.0 : cos(6.283185307179586 V)         V = 1/4 and 3/4: exactly 0
 *       n = (1 - w) (c c);   d = w + n;   s = d > 0 ? sqrt(n / d) : 0
 *       lam = f32(0.5 + 0.5 copysign(s, c))        rounded once to float32, in [0, 1]
 * The exception at V = 1/4 and 3/4 is there because the cos of the double next to pi / 2 is about 6e-17 with a sign that is the
 * library's own, and where w underflows that sign would decide between 0 and 1.  The inexact operations are the pow and the cos;
 * every quantity lies in [0, 1], so two conforming implementations differ by about 1e-15 in front of the rounding: lam is bit-equal
 * except where the double sits on a rounding boundary, and then off by one float32 ulp (at most 2^-24).
 *
 * perm is defined by its result, not by a sorting method: key_b = (uint64(r2) << 32) | b, and perm[k] is the b with the k-th smallest
 * key.  The low word is b, so keys never tie: perm is the stable argsort of r2, exactly, on every implementation.  (The kernel orders
 * the keys in LDS with a bitonic network over the power of two at or above B, padded with all-ones keys.)
 * csrc/leaf_mix_draws.hpp is this definition as host-and-device code.  Neither numpy's nor torch's numbers are reproduced.
 *
 * MEMORY SAFETY: nothing but state[0] is read; nothing outside perm[0, B), lam[0, B) and state[0] is written; perm holds each of
 * 0 .. B - 1 once.  Alignment: 8 bytes for state, 4 for perm and lam.  Status, in this order, before the launch (the counter is not
 * touched): LEAF_ERR_NULL_POINTER (state, perm, lam); LEAF_ERR_BAD_SHAPE (B < 1, B > 4096, alpha NaN, infinite, 0 or negative);
 * LEAF_ERR_ALIGNMENT. */
int leaf_draw_mixup(int B, double alpha, unsigned long long* state, int advance, unsigned long long seed,
                    unsigned long long stream_base, int* perm /*[B]*/, float* lam /*[B]*/, void* stream);

/* Resampling of a packed store on the device (additive: the ABI version stays 6).  The reference's loaders stop at
 * `assert clip_sr == sr` (utilities/data/utils.py:109,159): they expect a data set that was resampled on disk.  The entries below bring
 * every recording of a packed store from orig_freq to new_freq in one call, int16 in and int16 out where asked, without a float32
 * copy and without a sample of one recording reaching its neighbour.
 *
 * THE DEFINITION is the band-limited interpolation torchaudio.functional.resample documents (Hann-windowed sinc, polyphase), stated
 * here exactly; csrc/leaf_resample.hpp is this statement as host-and-device code.  Inputs: integers orig_freq > 0, new_freq > 0,
 * W = lowpass_width >= 1 (torchaudio's default 6), rho = rolloff in (0, 1] (0.99).
 *   g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g;  base = (double)min(o, n) * rho;  width = ceil(W * o / base).
 *   For phase p in [0, n) and tap k in [0, 2 width + o): num = (k - width) * n - p * o in int64, t = (double)num * base / (double)(o * n).
 *   The tap belongs to the phase's SPAN iff |t| < W.  The span is contiguous: k0[p] is its first tap, cnt[p] its size (12 - 13 taps at
 *   44.1 -> 48 kHz, 33 - 34 at 44.1 -> 16 kHz, 37 at 48 -> 16 kHz).  Inside it
 *       h[p][k] = fp32( sinc(t) * cos^2(pi t / (2 W)) * base / o ),   sinc(0) = 1, sinc(t) = sin(pi t) / (pi t),
 *   evaluated in double and rounded once.  Taps outside the span are exactly 0 and are never applied (torchaudio evaluates its window
 *   there and is left with ~1e-33; this library has nothing there).
 *   o == n is special: one phase whose only tap is 1 (width = 0).  Resampling to the same rate is then the identity on every bit
 *   pattern but two: -0 comes back as +0 and a signalling NaN as its quiet twin (payload kept), because the sample still passes
 *   through the chain below, fmaf(1, x, +0).  It also serves as the int16 <-> float32 conversion.
 * For a recording x[0, L), zeros outside it: out_len = ceil(n L / o) = (n L + o - 1) / o in 64 bits, and for j = i n + p
 *       y[j] = sum over the span, k ascending, of h[p][k] * x[i o + k - width],
 * accumulated in float32 as ONE chain acc = fmaf(h, x, acc) from acc = +0.0f: every tap of the span is applied, a sample outside
 * [0, L) enters as +0.0f, an int16 sample v means v * 2^-15 as everywhere.  The fixed order makes y a pure function of the recording:
 * it does not depend on the neighbours in the store, the offsets, the alignment, the number of recordings, the tile or the path, and
 * a CPU build of the same function (tools/resample_check.cpp) has the kernel's bits.  Against the formula in real numbers,
 * |y - y*| <= (cnt + 2) 2^-24 sum |h| |x| + 2^-149.
 * Output: float32, or int16 with LEAF_FLAG_OUT_PCM16: q = rintf(y * 32768.0f), round half to even, clamped to [-32768, 32767] --
 * the Gibbs overshoot of a full-scale signal saturates, it never wraps -- and NaN gives 0.
 *
 * The length, the table and the workspace:
 *   The length entry answers out_len for any L (L <= 0: 0; saturating at 2^63 - 1) and 0 for a frequency <= 0, as a size_t like the
 *   other size queries.  Host only.
 *   The table, host only, no GPU: the size query answers the bytes of the library's own compact layout for these parameters (0 for
 *   parameters the call would refuse), and the builder writes it to HOST memory: eight int32 header words (a magic number, o, n,
 *   width, stride, taps_in_lds, 0, 0), k0[n] and cnt[n] int32, then n rows of `stride` float32 taps -- row p holds h[p][k0 .. k0 + cnt)
 *   and zeros behind; stride is the largest cnt made odd.  The caller uploads it once per (orig_freq, new_freq, W, rho) and hands the
 *   device copy to every call.  The call recomputes o, n, width and stride on the host and reads none of them from the
 *   device; taps_in_lds is the one word the kernel reads: what the library would choose, and a caller may clear it to keep the taps
 *   in global memory where they would fit LDS (the same bits: the plan's switch between the two tap paths, which the tests use;
 *   setting it where the host finds no room changes nothing).  The builder's status: LEAF_ERR_UNSUPPORTED, LEAF_ERR_NULL_POINTER, LEAF_ERR_BAD_SHAPE (also for
 *   table_bytes other than the size query), LEAF_ERR_ALIGNMENT (4 bytes).
 *   The workspace: 8 (R + 1) bytes (0 for R < 1), overwritten.
 *
 * The call:
 *   store, store_len, flags: as in leaf_assemble_clips_f32, flags also LEAF_FLAG_OUT_PCM16            R: the number of recordings
 *   in_off [R] int64, in_len [R] int32: the recordings          out_off [R] int64: where each recording's output begins in `out`
 *   table, table_bytes: the device copy of the table for the SAME four parameters
 *   out: out_total samples, float32 or int16
 * The work is split by TILES of 1024 output samples, not by recording: a first launch of one workgroup writes the tile prefix of the
 * clamped plan into the workspace, a second runs the tiles, one workgroup of 256 lanes each -- one long recording spreads over the
 * chip, a short one costs one workgroup, a tile never spans two recordings.  A tile stages its input window (about 1024 o / n +
 * 2 width + o samples) into LDS as float32, converting int16 in the load and ZERO-FILLING everything outside [0, L): that zero fill is
 * the padding rule and what keeps the neighbouring recording out.  Taps come from LDS when table and window fit 64 KB per workgroup,
 * otherwise from global memory (4096 -> 4099 has a 213 KB table); a window beyond the budget (from o / n of about 15: 16 -> 1, 44100 -> 2000) is read from
 * global memory too.  Stores are 16-byte chunks where out's alignment allows, element stores at a tile's two ends.
 *
 * MEMORY SAFETY: what the library cannot inspect is clamped by the kernel.  in_off / in_len as in leaf_assemble_clips_f32; out_off
 * into [0, out_total]; a record's output length is min(out_len of the clamped L, out_total - out_off); every k0 / cnt read from the
 * table is clamped against the staged window (cnt into [0, stride], k0 into [0, 2 width + o - cnt]); o, n, width and stride are
 * recomputed on the host, never read from the table.  Whatever plan or table the caller hands in, nothing outside store[0, store_len)
 * and table[0, table_bytes) is read, nothing outside out[0, out_total) and the workspace is written.  Records whose outputs overlap
 * leave the overlap to whichever tile stores last.
 * Alignment: store and out 4 bytes (2 for int16), in_off and out_off 8, in_len and table 4, workspace 16.  Status, in this order, before
 * any launch: LEAF_ERR_UNSUPPORTED for a flag other than LEAF_FLAG_X_PCM16 / LEAF_FLAG_OUT_PCM16, for a reduced o or n above 65535 and
 * for a table above 2^26 bytes; LEAF_ERR_NULL_POINTER (store, in_off, in_len, table, out, out_off); LEAF_ERR_BAD_SHAPE for R < 1, a
 * negative store_len or out_total, a frequency <= 0, lowpass_width < 1, rolloff outside (0, 1], or table_bytes other than the size
 * query; LEAF_ERR_ALIGNMENT; LEAF_ERR_WORKSPACE.  out must not overlap the store.
 * Not built: the Kaiser window, gradients, bfloat16.  (Chunked resampling with carried state: the next section.) */
size_t leaf_resample_length(long long L, int orig_freq, int new_freq);
size_t leaf_resample_table_bytes(int orig_freq, int new_freq, int lowpass_width, double rolloff);
int leaf_resample_table_f32(int orig_freq, int new_freq, int lowpass_width, double rolloff, void* table_host, size_t table_bytes);
size_t leaf_resample_workspace_bytes(int R);
int leaf_resample_f32(const void* store, long long store_len, int flags, int R, const long long* in_off /*[R]*/,
                      const int* in_len /*[R]*/, int orig_freq, int new_freq, int lowpass_width, double rolloff,
                      const void* table /*device*/, size_t table_bytes, void* out, long long out_total,
                      const long long* out_off /*[R]*/, void* workspace, size_t workspace_bytes, void* stream);

/* Chunked resampling with carried state (additive: the ABI version stays 6): B INDEPENDENT streams at a device rate (44.1 or 48 kHz
 * from a capture device or the network) are brought to the rate leaf_stream_bank_step_f32 serves, chunk by chunk, in ONE launch per
 * step and 128 slots.  The history the next outputs still need stays ON THE DEVICE in a `state` buffer the caller owns; WHERE a stream
 * stands stays on the host, in a leaf_resample_pos per slot (nothing is read back, nothing synchronises, there is no workspace).
 *
 * THE CONTRACT: an output of leaf_resample_f32 is one fmaf chain over its span, a pure function of the recording.  The outputs a
 * stream emits over its life, concatenated, are therefore BIT FOR BIT those of leaf_resample_f32 on the concatenated chunks, for
 * any chunking (chunks of 0 and 1 samples included), float32 and int16, on both tap paths.
 *
 * The position (csrc/leaf_resample_stream.hpp is this paragraph as code).  With the reduced ratio o : n, width, K = 2 width + o and
 * the spans k0[p], cnt[p] of the definition above, klast[p] = k0[p] + cnt[p] - 1 (non-decreasing in p).  A stream's signal in a step
 * is the virtual buffer V = [history (hist_len samples) | chunk (Tc samples)], Lv = hist_len + Tc.  Window coordinate c means "tap c
 * of group 0", group 0 being the group of the next output to emit.  `shift` virtual +0.0f samples stand in front of V[0]: width of
 * them when a stream begins (the recording starts at its first sample), 0 once the stream has moved width samples in.
 * E = shift + Lv is one past the last sample that has arrived; `phase` is the phase of the next output.
 *   While the stream runs, a step emits, in order from (g, p) = (0, phase), every output whose whole span has arrived:
 *     g o + klast[p] <= E - 1 -- per output, not per group: an output leaves as soon as its last sample is there.
 *   At the end of the stream (end = 1) it emits every remaining output of the recording: (g n + p) o < n (E - width), samples at or
 *     behind E counting as +0.0f.  This is out_len = ceil(n T / o) in relative terms; no absolute position is kept, so a stream may
 *     run for ever.
 *   Hand-over: the next output being (G, p'), the new origin is window coordinate G o: drop_samples = max(0, G o - shift),
 *     shift' = max(0, shift - G o), hist_len' = Lv - drop_samples, phase' = p'.  hist_len' never exceeds H = K - 1, the history
 *     capacity (474 samples at 44.1 -> 16 kHz, 40 at 48 -> 16 kHz, 0 at o == n).  At the end nothing is kept.
 *
 * The history query answers H (0 for parameters the step refuses).  The state query sizes `state`: two history halves of [B][H]
 * samples in the sample type `flags` names (float32, or int16 with LEAF_FLAG_X_PCM16), each region a multiple of 256 bytes and at
 * least 256; 0 for B < 1 and for what the step refuses.  The buffer may hold anything when a stream begins.
 *
 * A slot's record (leaf_resample_slot):
 *   idle = 1: the slot takes no part.  Nothing of its state is read or written, no other field is looked at, its row of out is zeros.
 *   idle = 0: the signal is [history (hist_len samples of row b of half `parity`) | chunk[b * chunk_stride .. + Tc)]; outputs
 *     phase, phase + 1, ... (n of them) of group 0 on are written to out[b][0 .. n); unless end = 1, samples [drop_samples, Lv) go to
 *     row b of the OTHER half, and the caller flips the slot's parity.  Only the first Tc samples of a chunk row are read.
 *
 * The plan entry is the host side of a step for the whole bank, on integers alone (no table, no GPU): from each slot's carried
 * position pos[b] (running, hist_len, shift, phase, parity), its Tc[b] (0 .. 2^20 samples) and its end[b] (NULL: no stream ends) it
 * fills slots[b] and counts[b] (= slots[b].n) and advances pos[b].  Tc = 0 without end leaves a slot idle; a slot that is not running
 * begins a new stream with its first samples (hist_len = 0, shift = width, phase = 0); end on a slot that is not running does
 * nothing; a stream that ends stops running.  All positions move or none: LEAF_ERR_UNSUPPORTED, LEAF_ERR_NULL_POINTER (pos, Tc,
 * slots, counts), LEAF_ERR_BAD_SHAPE (B < 0, bad parameters, a Tc outside its range, a position outside its ranges, a count beyond
 * 2^31 - 1); B = 0: LEAF_OK.
 *
 * The step:
 *   chunk, chunk_stride: float32 or int16 (LEAF_FLAG_X_PCM16: the history is then int16 too); row b starts at b * chunk_stride; may
 *     be NULL when no slot has samples              slots: a HOST array of B records, read before the call returns (they travel to
 *     the kernel by value)              state, state_bytes: as the state query sizes it
 *   the four parameters, table, table_bytes: as in leaf_resample_f32 (the device copy of the same table)
 *   out: [B][n_max], float32 or int16 (LEAF_FLAG_OUT_PCM16): a slot's n outputs, then zeros; EVERY element is written.  n_max = 0:
 *     out is not touched and may be NULL (the launch still moves the history).
 * Grid: (tiles of 1024 outputs over n_max, at least 1) x slots, 256 lanes.  A workgroup stages its tile's window into LDS as float32
 * from the two sources (+0.0f below `shift`, the history below hist_len, the chunk below Lv, +0.0f behind), runs the tile function
 * of leaf_resample_f32 from phase `phase` on and stores with the same aligned store; the workgroup of tile 0 hands the history over.
 * Every workgroup reads only the old half and the chunk: nothing races.  Taps come from LDS or global memory as the table's word 5
 * says.  No atomics, no scratch, no workspace, no readback.  A call in which no slot emits or keeps anything launches nothing.
 * A ratio whose tile window does not fit LDS (16 -> 1, 44100 -> 2000) is NOT served: LEAF_ERR_UNSUPPORTED, and the size queries
 * answer 0.  Steps on one `state` must execute in order (one HIP stream, or events).
 * Checks, all on the host before anything is launched, in this order: a flag other than LEAF_FLAG_X_PCM16 / LEAF_FLAG_OUT_PCM16, or
 * a ratio the library or this entry does not take: LEAF_ERR_UNSUPPORTED; B = 0: LEAF_OK; NULL (slots, state, table; out when n_max >
 * 0; chunk when a slot has Tc > 0); shape (B < 1, n_max < 0, bad parameters, table_bytes, a slot's idle or Tc, chunk_stride below the
 * longest Tc when B > 1): LEAF_ERR_BAD_SHAPE; alignment (state 16 bytes, table 4, chunk and out by element); then per slot, one bad
 * slot refusing the whole call with LEAF_ERR_BAD_SHAPE: hist_len <= H, shift <= width, phase < n, parity and end 0 or 1,
 * drop_samples <= Lv and (end = 0) Lv - drop_samples <= H, n <= n_max, n equal to what the rule gives; state_bytes:
 * LEAF_ERR_WORKSPACE.  Whatever the records say, nothing outside state, table, out and the first Tc samples of a chunk row is touched.
 * Not built: resampling inside the fused streaming kernel, ratios whose window does not fit LDS, a device-resident position. */
typedef struct leaf_resample_slot {
    int idle;
    int hist_len, Tc, parity, shift, phase, n, drop_samples, end;
} leaf_resample_slot;
typedef struct leaf_resample_pos {
    int running, hist_len, shift, phase, parity;
} leaf_resample_pos;
int leaf_resample_stream_history_samples(int orig_freq, int new_freq, int lowpass_width, double rolloff);
size_t leaf_resample_stream_state_bytes(int B, int orig_freq, int new_freq, int lowpass_width, double rolloff, int flags);
int leaf_resample_stream_plan(int B, int orig_freq, int new_freq, int lowpass_width, double rolloff, leaf_resample_pos* pos /*[B] in and out*/,
                              const int* Tc /*[B]*/, const int* end /*[B] or NULL*/, leaf_resample_slot* slots /*[B] out*/,
                              int* counts /*[B] out*/);
int leaf_resample_stream_step_f32(const void* chunk, long long chunk_stride, int B, const leaf_resample_slot* slots /*host*/, int n_max,
                                  void* state, size_t state_bytes, int flags, int orig_freq, int new_freq, int lowpass_width,
                                  double rolloff, const void* table /*device*/, size_t table_bytes, void* out, void* stream);

/* ClipValue and a sox-style reverb on an assembled batch (additive: the ABI version stays 6).  In the reference's training pipeline
 * (utilities/data/raw_transforms.py, get_raw_transforms_v2) both transforms sit between AddRandomNoise and RandomGain, switched
 * off: ClipValue "needs work", RandomReverb -- sox's `reverb` effect per clip on the CPU -- is "TOO SLOW".  One launch maps a
 * float32 batch x [B][S] to y [B][S]; clips are independent, each takes two optional steps in the reference's order.
 *
 * CLIPVALUE.  clip_factor [B] float32 or NULL (no clip takes the step); a negative factor skips the clip's step.  Otherwise, with the
 * exact minimum and maximum of the clip's S samples (a zero of either sign counting as +0),
 *       lo = fp32(min * factor)      hi = fp32(max * factor)      x' = min(max(x, lo), hi)   i.e.  m = x < lo ? lo : x;  hi < m ? hi : m
 * which is torch.clamp(x, min=lo, max=hi) for finite input.  NaN input is unspecified.
 *
 * REVERB.  sox's `reverb` (Freeverb: eight feedback combs with a damping one-pole in the loop, summed, then four all-passes in
 * series) for one channel, stereo depth 0, pre-delay 0, wet gain 0 dB, the dry signal kept.  feedback [B], damp [B] float32 and
 * comb [B][8] int32 delay lengths -- all three or all NULL (no clip takes the step); comb[b][0] <= 0 skips the clip's step.  The four
 * all-pass lengths follow from sample_rate alone (below).  All arithmetic is IEEE float32 and EVERY operation is rounded on its own:
 * no fused multiply-add, no contraction; subnormals are kept.  State per clip, all zero at sample 0: the lines cb[i][comb[i]] and
 * ap[j][allpass[j]], store[i], and one write index per line that wraps at the line's length.  Per sample n = 0 .. S - 1, x' being
 * the sample behind ClipValue:
 *       in = x'[n];  out = 0.0f;
 *       for (i = 7; i >= 0; --i) {                  combs, in this order; out is summed in this order
 *           o = cb[i][p_i];
 *           store[i] = o + (store[i] - o) * damp;   subtract, multiply, add: three roundings
 *           cb[i][p_i] = in + store[i] * feedback;  multiply, add
 *           advance p_i;  out = out + o;
 *       }
 *       for (j = 3; j >= 0; --j) {                  all-passes in series, in this order
 *           o = ap[j][q_j];
 *           ap[j][q_j] = out + o * 0.5f;
 *           advance q_j;  out = o - out;
 *       }
 *       y[n] = in + out * wet;                      multiply, add
 * y has S samples: the tail behind the clip's end is dropped.  A clip that takes neither step is copied bit for bit.
 *
 * THE PLAN is host arithmetic in IEEE double, rounded once where a float32 is stored, from sample_rate and the integer percentages
 * reverberance, damping and room_scale (sox's parameters):
 *       r = sample_rate / 44100            scale = room_scale / 100 * 0.9 + 0.1
 *       comb[i] = (int)(scale * r * C[i] + 0.5),   C = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617}
 *       allpass[j] = (int)(r * A[j] + 0.5),        A = {225, 341, 441, 556}
 *       a = -1 / ln(1 - 0.3);   b = 100 / (ln(1 - 0.98) * a + 1);   feedback = 1 - exp((reverberance - b) / (a * b))
 *       damp = damping / 100 * 0.3 + 0.2
 * (feedback is 0.30 at 0 %, about 0.88 at 50 %, 0.98 at 100 %.)  Every length must be at least 1.  This restates sox's algorithm from
 * its published form; sox is not part of this library's tests, so parity with sox itself is UNPINNED.  Left out: the two one-pole
 * tone filters newer sox versions put behind the all-passes, stereo depth, pre-delay, wet-only mode and sox's drain tail.
 *
 * HOSTILE PLANS.  The plan arrays are device memory that the entry cannot see.  The kernel clamps each comb length into
 * [1, cap_i], cap_i being the length at room_scale = 100 for the call's sample_rate; its LDS is laid out by those caps and the
 * all-pass lengths, so whatever the plan holds it indexes nothing outside its own LDS, reads nothing outside x and the plan arrays'
 * B (or 8 B) entries, and writes nothing outside y.  A sample_rate whose lines do not fit a workgroup's LDS budget (64 KB; 48 kHz
 * takes about 55 KB) is refused with LEAF_ERR_UNSUPPORTED.
 *
 * The kernel (csrc/inst_clip_effects.hip; the arithmetic is csrc/leaf_clip_effects.hpp, host and device) walks a clip in chunks no
 * longer than its shortest line: within a chunk the comb sum and the all-passes are elementwise over all lanes, and only the eight
 * store[i] chains run in order, one lane each, several clips side by side in one wave.  The result is bit for bit the sequential
 * definition above (no parallel scan: that would change the rounding).  No workspace, nothing read back, no host synchronisation:
 * the launch captures into a graph.  tools/clip_effects_check.cpp runs the definition on the CPU.
 *
 * Alignment: 4 bytes for every array.  Status, in this order, before the launch: LEAF_ERR_NULL_POINTER (x, y; a reverb group given
 * in part); LEAF_ERR_BAD_SHAPE (B < 1, S < 1, B * S >= 2^31, y overlapping x, or, with the reverb group, a sample_rate below 1 or one
 * that makes a length 0); LEAF_ERR_ALIGNMENT; LEAF_ERR_UNSUPPORTED (the lines do not fit).  Without the reverb group sample_rate and
 * wet are not looked at. */
int leaf_clip_effects_f32(const float* x /*[B][S]*/, float* y /*[B][S]*/, int B, int S, const float* clip_factor /*[B] or NULL*/,
                          const float* feedback /*[B] or NULL*/, const float* damp /*[B] or NULL*/, const int* comb /*[B][8] or NULL*/,
                          int sample_rate, float wet, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LEAF_HIP_H_ */
