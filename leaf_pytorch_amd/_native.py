"""ctypes binding of the C ABI in include/leaf_hip.h (libleaf_hip.so, HIP kernels for gfx950).

There is deliberately NO fallback: if the shared library is missing or a call returns a non-zero
status, a RuntimeError is raised.  PyTorch is used only for device memory (tensors own the HBM
buffers, the caching allocator provides the scratch workspace) and for the current HIP stream.
"""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
import threading
from typing import Optional

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_REPO_DIR = os.path.dirname(_PKG_DIR)
LIB_PATH = os.path.join(_PKG_DIR, "libleaf_hip.so")
SRC_PATH = os.path.join(_PKG_DIR, "csrc", "leaf_kernels.hip")
INCLUDE_DIR = os.path.join(_REPO_DIR, "include")

ABI_VERSION = 6
ALGO_AUTO, ALGO_STAGED, ALGO_MFMA, ALGO_FFT, ALGO_FFT_WG, ALGO_FFT_SMALL = 0, 1, 2, 3, 4, 5


def algo_reserve_cus(k: int) -> int:
    """LEAF_ALGO_RESERVE_CUS(k): OR into ``algo`` so that the call leaves ``k`` CUs free for kernels of other streams."""
    return (int(k) & 0xff) << 16


FLAG_PCEN, FLAG_LOG1P, FLAG_IO_BF16, FLAG_BWD_STAGED, FLAG_BWD_MFMA, FLAG_PEAKNORM, FLAG_BWD_FULL_TRANSFORMS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
FLAG_X_PCM16 = 0x100           # x is int16 PCM (a sample v means v / 32768); everything else stays float32
FLAG_OUT_BF16 = 0x200          # the feature side alone is bfloat16: out of the forward, grad_out of the backward; x as its own flags say
FLAG_OUT_PCM16 = 0x400         # leaf_resample_f32: the output is int16 PCM, rint(y * 32768) saturated
FLAG_BWD_STRICT_BAND_CLASSES = 0x80   # leaf_backward_f32: the backward's band classes by round 5's rule alone (default: the forward's bias-aware decision)
ALGO_STREAM_FINALIZE = 1 << 25   # LEAF_ALGO_STREAM_FINALIZE: per-frame sums in an LDS ring, finalized as the blocks complete
ALGO_FULL_TRANSFORMS = 1 << 26   # LEAF_ALGO_FULL_TRANSFORMS: no band-limited filter tasks (every filter on 2048-point transforms)
ALGO_STRICT_BAND_CLASSES = 1 << 27   # LEAF_ALGO_STRICT_BAND_CLASSES: the band classes' energy bound does not follow the pooling bias (round 5's decision)
ALGO_NO_TABLE_CACHE = 1 << 28   # LEAF_ALGO_NO_TABLE_CACHE: the forward rebuilds its tables on every call (no self-validating table cache)
OPT_PEAKNORM = 1 << 24          # torch.ops.leaf_amd.forward: option bit in `algo` that sets LEAF_FLAG_PEAKNORM (torch_binding.cpp)
OPT_FULL_BACKWARD = 1 << 29     # torch.ops.leaf_amd.forward_train / _LeafFn: option bit in `algo` -- the autograd formula takes the full backward
                                # (leaf_amd::backward) also where the head-only one would do (Leaf.full_backward(); never reaches the C ABI)
STAGE_GABOR_CONV, STAGE_LOWPASS, STAGE_EMA, STAGE_PCEN = 1, 2, 3, 4

_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None

_f32p = ctypes.c_void_p
_SIGNATURES = {
    # name: (restype, argtypes)   -- must list every symbol include/leaf_hip.h declares
    "leaf_abi_version": (ctypes.c_int, []),
    "leaf_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "leaf_num_frames": (ctypes.c_int, [ctypes.c_int] * 3),
    "leaf_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 6),
    "leaf_forward_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 5
                         + [_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_table_cache_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "leaf_forward_cached_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 5
                                + [_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_auto_algo": (ctypes.c_int, [ctypes.c_int] * 5),
    "leaf_fft_plan_info": (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]),
    "leaf_band_classes_f32": (ctypes.c_int, [_f32p, _f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_forward_profiled_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 5
                                  + [_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_float)]),
    "leaf_backward_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 7),
    "leaf_backward_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 4 + [_f32p] * 10
                          + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_forward_save_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 5
                              + [_f32p, _f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # head-only backward: pooled_raw, grad_out, B, TP, F, the PCEN four, flags, g_pool_b and the four PCEN gradients, workspace, stream
    "leaf_backward_head_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "leaf_backward_head_f32": (ctypes.c_int, [_f32p] * 2 + [ctypes.c_int] * 3 + [_f32p] * 4 + [ctypes.c_int] + [_f32p] * 5
                               + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_gabor_taps_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, _f32p, ctypes.c_void_p]),
    "leaf_lowpass_window_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, _f32p, ctypes.c_void_p]),
    "leaf_gabor_conv_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, _f32p, ctypes.c_int, ctypes.c_int,
                                           _f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_squared_modulus_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p,
                                                ctypes.c_void_p]),
    "leaf_gaussian_lowpass_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p,
                                                 ctypes.c_int, ctypes.c_int, _f32p, ctypes.c_void_p,
                                                 ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_ema_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, ctypes.c_void_p]),
    "leaf_pcen_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _f32p,
                                     ctypes.c_float, _f32p, ctypes.c_void_p]),
    "leaf_pcen_stream_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, _f32p,
                                            ctypes.c_float, ctypes.c_int, _f32p, _f32p, _f32p, ctypes.c_void_p]),
    "leaf_stage_backward_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 6),
    "leaf_gabor_conv_backward_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, _f32p, ctypes.c_int, ctypes.c_int,
                                                    _f32p, _f32p, _f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_squared_modulus_backward_f32": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p,
                                                         ctypes.c_void_p]),
    "leaf_gaussian_lowpass_backward_f32": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p,
                                                          ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p, ctypes.c_void_p,
                                                          ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_ema_backward_f32": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _f32p, _f32p,
                                             ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_pcen_backward_f32": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_f32p] * 4
                               + [ctypes.c_float] + [_f32p] * 5 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_peak_normalize_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, _f32p, ctypes.c_void_p]),
    # batch assembly: store, store_len, flags, B, size, rec_off, rec_len, start, pad_mode, gain, normalize, masks, M, out, stream
    "leaf_assemble_clips_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
                                + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    # ... with the noise group (noise_store, noise_store_len, noise_off, noise_len, noise_start, noise_pad_mode, noise_coeff) and the
    # Gaussian group (gauss_amp, gauss_seed, gauss_stream) between out and stream
    "leaf_assemble_clips_noise_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
                                      + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
                                      + [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_void_p] * 5
                                      + [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p]),
    # the stream itself: B, size, seed, stream ids, out, stream
    "leaf_gaussian_noise_f32": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # whole-recording evaluation.  The peaks: store, store_len, flags, R, rec_off, rec_len, peaks, workspace, workspace_bytes, stream
    "leaf_clip_peaks_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "leaf_clip_peaks_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
                            + [ctypes.c_size_t, ctypes.c_void_p]),
    # ... and the rows: store, store_len, flags, rows, size, rec_off, rec_len, win, peaks, rec, R, out, stream
    "leaf_assemble_segments_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int]
                                   + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    # waveform standardisation.  The moments: store, store_len, flags, R, rec_off, rec_len, moments, workspace, workspace_bytes, stream
    "leaf_clip_moments_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "leaf_clip_moments_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
                              + [ctypes.c_size_t, ctypes.c_void_p]),
    # ... the noise entry with the group (moments, moments_rec, R) between gauss_stream and stream
    "leaf_assemble_clips_std_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
                                    + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
                                    + [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_void_p] * 5
                                    + [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p]
                                    + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    # ... and the rows entry with (moments, normalize) between out and stream
    "leaf_assemble_segments_std_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int]
                                       + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    # the plan drawn on the device: B, size, train, offsets, lengths, R, noise_offsets, noise_lengths, Rn, index, order, N, state, advance,
    # seed, stream_base, the two pad modes, wrap_pad_prob, gain_prob, gain_db (2), M, time_perc, noise_prob, snr (2), gauss_prob,
    # gauss_amp (2), the fifteen outputs, stream
    "leaf_draw_clip_plan": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int] + [ctypes.c_double] * 4
                            + [ctypes.c_int] + [ctypes.c_double] * 7 + [ctypes.c_void_p] * 15 + [ctypes.c_void_p]),
    # mixup's draws on the device: B, alpha, state, advance, seed, stream_base, perm, lam, stream
    "leaf_draw_mixup": (ctypes.c_int, [ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # resampling: the output length (L, orig_freq, new_freq); the table's bytes and the table itself, on the host (orig_freq, new_freq,
    # lowpass_width, rolloff[, table, table_bytes]); the workspace (R); the call -- store, store_len, flags, R, in_off, in_len, the four
    # parameters, table, table_bytes, out, out_total, out_off, workspace, workspace_bytes, stream
    "leaf_resample_length": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]),
    "leaf_resample_table_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    "leaf_resample_table_f32": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t]),
    "leaf_resample_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "leaf_resample_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # chunked resampling with carried state: the history capacity and the state's bytes (the four parameters[, flags]); the host plan --
    # B, the four parameters, pos (leaf_resample_pos[B]), Tc, end, slots (leaf_resample_slot[B]), counts; the step -- chunk,
    # chunk_stride, B, slots, n_max, state, state_bytes, flags, the four parameters, table, table_bytes, out, stream
    "leaf_resample_stream_history_samples": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    "leaf_resample_stream_state_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int]),
    "leaf_resample_stream_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "leaf_resample_stream_step_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                     ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                     ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    # ClipValue and the reverb: x, y, B, S, clip_factor, feedback, damp, comb, sample_rate, wet, stream
    "leaf_clip_effects_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
                              + [ctypes.c_int, ctypes.c_float, ctypes.c_void_p]),
    "leaf_fft_tables_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "leaf_fft_prepare_tables_f32": (ctypes.c_int, [_f32p, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_forward_prepared_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
                                  + [_f32p] * 5 + [ctypes.c_int] * 4
                                  + [_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # waveform mixup: x, mix_perm, mix_lam in front of the plain entries' arguments
    "leaf_mixup_f32": (ctypes.c_int, [_f32p, ctypes.c_int, ctypes.c_int, _f32p, _f32p, ctypes.c_int, _f32p, ctypes.c_void_p]),
    "leaf_forward_mix_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 6),
    "leaf_forward_mix_f32": (ctypes.c_int, [_f32p] * 3 + [ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 5
                             + [_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_forward_save_mix_f32": (ctypes.c_int, [_f32p] * 3 + [ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 5
                                  + [_f32p, _f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "leaf_backward_mix_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 6),
    "leaf_backward_mix_f32": (ctypes.c_int, [_f32p] * 3 + [ctypes.c_int, ctypes.c_int] + [_f32p] * 7 + [ctypes.c_int] * 4 + [_f32p] * 10
                              + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # one-launch streaming step: history and smoother state resident in a caller-owned state buffer
    "leaf_stream_history_samples": (ctypes.c_int, [ctypes.c_int] * 2),
    "leaf_stream_state_bytes": (ctypes.c_size_t, [ctypes.c_int] * 5),
    "leaf_stream_step_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_size_t]
                             + [ctypes.c_int] * 6 + [_f32p] * 7 + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p]),
    # the bank: chunk, chunk_stride, B, slots (leaf_stream_slot[B], a host array), n_max, state, state_bytes
    "leaf_stream_bank_step_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_size_t] + [_f32p] * 7 + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _translation_units(csrc: str):
    """leaf_kernels.hip (C ABI, host logic, small kernels) + one inst_*.hip per family of big kernel templates."""
    return [SRC_PATH] + sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.startswith("inst_") and f.endswith(".hip"))


def _includes_of(path: str, csrc: str, seen=None) -> set:
    """Transitive closure of the quoted #include files of one translation unit (csrc/ and include/ only)."""
    seen = set() if seen is None else seen
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith('#include "'):
                name = line.split('"')[1]
                for base in (csrc, INCLUDE_DIR):
                    cand = os.path.join(base, name)
                    if os.path.exists(cand) and cand not in seen:
                        seen.add(cand)
                        _includes_of(cand, csrc, seen)
    return seen


def build(force: bool = False, verbose: bool = False, jobs: Optional[int] = None, variant: Optional[str] = None,
          extra_flags: Optional[str] = None) -> str:
    """Compile csrc/*.hip for gfx950 into libleaf_hip.so (in-tree).  Needs hipcc, not a GPU.

    The translation units are compiled in parallel into build/*.o (git-ignored) and only those whose sources or headers
    changed are recompiled; the shared library is linked from the objects.  ``variant`` (tools only) builds a second
    library with ``extra_flags`` into build/variants/<variant>/ and returns its path; the product library is untouched."""
    csrc = os.path.dirname(SRC_PATH)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = (os.environ.get("LEAF_HIPCC_EXTRA", "") if extra_flags is None else extra_flags).split()
    LIB_PATH = globals()["LIB_PATH"] if variant is None else os.path.join(_PKG_DIR, "build", "variants", variant, "libleaf_hip.so")
    # -fno-slp-vectorize: the SLP vectorizer packs the FFT butterflies into v_pk_*_f32 (no faster than two scalar ops on
    # gfx950, tools/ubench_valu.hip) at the price of hundreds of v_mov shuffles and ~35 extra VGPRs per kernel
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC", "-I", INCLUDE_DIR] + extra
    obj_dir = os.path.join(_PKG_DIR, "build") if variant is None else os.path.dirname(LIB_PATH)
    os.makedirs(obj_dir, exist_ok=True)
    stamp = os.path.join(obj_dir, "flags.txt")
    flag_text = " ".join([hipcc] + flags)
    if not os.path.exists(stamp) or open(stamp).read() != flag_text:
        force = True                                         # different flags (LEAF_HIPCC_EXTRA): every object is stale
    units, objs, todo = _translation_units(csrc), [], []
    for src in units:
        obj = os.path.join(obj_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        objs.append(obj)
        deps = [src] + sorted(_includes_of(src, csrc))
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(d) for d in deps):
            todo.append((src, obj))
    if not todo and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(o) for o in objs):
        return LIB_PATH
    jobs = jobs or int(os.environ.get("LEAF_BUILD_JOBS", "0")) or min(len(todo) or 1, os.cpu_count() or 1)
    procs, failed = [], []
    pending = list(todo)
    while pending or procs:
        while pending and len(procs) < jobs:
            src, obj = pending.pop(0)
            cmd = [hipcc] + flags + ["-c", src, "-o", obj + ".tmp"]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((subprocess.Popen(cmd), src, obj))
        proc, src, obj = procs.pop(0)
        if proc.wait() != 0:
            failed.append(src)
        else:
            os.replace(obj + ".tmp", obj)
    if failed:
        raise subprocess.CalledProcessError(1, f"hipcc failed for {failed}")
    with open(stamp, "w") as fh:
        fh.write(flag_text)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB_PATH + ".tmp"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


def load() -> ctypes.CDLL:
    """dlopen libleaf_hip.so and attach prototypes; raises RuntimeError (never falls back) if absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU/eager fallback exists). "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or leaf_pytorch_amd.build().")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError here = ABI mismatch, surfaced loudly
            fn.restype, fn.argtypes = res, args
        if lib.leaf_abi_version() != ABI_VERSION:
            raise RuntimeError("libleaf_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().leaf_status_string(status).decode()
        raise RuntimeError(f"{what} failed: {msg} (status {status})")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev_f32(t: torch.Tensor, name: str, device: torch.device) -> torch.Tensor:
    if t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    return t.detach().contiguous()


def _unpack_x(x: torch.Tensor, who: str, mixed: bool = False):
    """The waveform of a call, (B,1,T) or (B,T), as a contiguous (B,T) buffer on its HIP device, and its I/O flag: float32 (0),
    bfloat16 (FLAG_IO_BF16: the features come back in bfloat16 too) or int16 PCM (FLAG_X_PCM16: a sample v means v / 32768, the
    features are float32).  ``mixed``: a call that mixes the clips takes float32 and int16 only."""
    require_hip(x, who)
    if x.dim() == 3 and x.shape[1] == 1:
        x2 = x[:, 0, :]
    elif x.dim() == 2:
        x2 = x
    else:
        raise RuntimeError(f"expected input of shape (B,1,T), got {tuple(x.shape)}")
    if mixed and x2.dtype not in (torch.float32, torch.int16):
        raise RuntimeError(f"{who}: the mix is defined in float32 on a float32 or int16 (PCM) waveform, got {x2.dtype}")
    if x2.dtype == torch.bfloat16 or x2.dtype == torch.int16:
        return x2.detach().contiguous(), (FLAG_IO_BF16 if x2.dtype == torch.bfloat16 else FLAG_X_PCM16)
    return _dev_f32(x2, "x", x.device), 0


def _gather(dev: torch.device, params, pcen: bool, log1p: bool):
    """The seven parameters as the C ABI reads them -- float32, contiguous, on ``dev``, ``pool_w`` flat; the PCEN four None when PCEN
    is off (``kernel`` / ``pool_w`` may be None for a call that takes prepared tables instead) -- and the compression's flag bits."""
    kernel, pool_w, pool_b, alpha, delta, root, ema_w = params
    kernel = None if kernel is None else _dev_f32(kernel, "kernel", dev)
    pool_w = None if pool_w is None else _dev_f32(pool_w.reshape(-1), "pool_w", dev)
    pool_b = _dev_f32(pool_b, "pool_b", dev)
    if not pcen:
        return (kernel, pool_w, pool_b, None, None, None, None), (FLAG_LOG1P if log1p else 0)
    return (kernel, pool_w, pool_b, _dev_f32(alpha, "alpha", dev), _dev_f32(delta, "delta", dev), _dev_f32(root, "root", dev),
            _dev_f32(ema_w, "ema_w", dev)), FLAG_PCEN


def _features(io_flags: int, out_bf16: bool = False):
    """(``out_bf16`` as the call means it, the feature dtype): bfloat16 features for a bfloat16 waveform, or on request
    (LEAF_FLAG_OUT_BF16; redundant for a bfloat16 ``x``, where it is dropped)."""
    out_bf16 = bool(out_bf16) and io_flags != FLAG_IO_BF16
    return out_bf16, (torch.bfloat16 if io_flags == FLAG_IO_BF16 or out_bf16 else torch.float32)


def _check_out(out: torch.Tensor, shape: tuple, dtype: torch.dtype, dev: torch.device) -> None:
    if (out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != shape or out.device != dev):
        raise RuntimeError(f"out must be a contiguous {shape} tensor on {dev} matching the input dtype (float32; bfloat16 for bfloat16 x)")


def require_hip(x: torch.Tensor, who: str) -> None:
    if x.device.type != "cuda":
        raise RuntimeError(
            f"{who}: input is on '{x.device}'. leaf_pytorch_amd runs only on an AMD GPU through its HIP kernels; "
            "there is no CPU path in the product (the CPU restatement lives in oracle/ for tests only).")


def stream_ptr(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _call(dev: torch.device, entry: str, *args, ws=None, after=(), tolerate=()) -> int:
    """Run the C-ABI entry ``entry`` under the device guard of ``dev`` on its current stream and check the status by the entry's name
    (a status in ``tolerate`` is returned instead).  Tensors among ``args`` go in as their addresses; the stream is appended.
    ``ws``: the scratch workspace the entry takes in front of the stream, as its size in bytes or as a function of the loaded library
    that answers it (asked under the same guard: the plans follow the device's CU count); ``after``: arguments behind the stream."""
    lib = load()
    with torch.cuda.device(dev):
        tail = ()
        if ws is not None:
            w = workspace(ws if isinstance(ws, int) else ws(lib), dev)
            tail = (_ptr(w), w.numel())
        rc = getattr(lib, entry)(*[ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args], *tail, stream_ptr(dev), *after)
    if rc not in tolerate:
        check(rc, entry)
    return rc


def num_frames(T: int, K: int, hop: int) -> int:
    return load().leaf_num_frames(T, K, hop)


def fft_plan_info(B: int, T: int, F: int, K: int, hop: int) -> Optional[dict]:
    """Plan of the overlap-save path (leaf_fft_plan_info), or None when it does not cover the geometry."""
    info = (ctypes.c_int * 8)()
    if load().leaf_fft_plan_info(B, T, F, K, hop, info) != 0:
        return None
    keys = ("fft_n", "block_len", "blocks_per_clip", "filters_per_task", "filter_groups", "slots", "row_buffers", "lds_bytes")
    return dict(zip(keys, (int(v) for v in info)))


def band_classes(kernel: torch.Tensor, pool_w: torch.Tensor, K: int, hop: int,
                 pool_b: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Inverse-transform length (256 / 512 / 2048; 512 / 4096 on the 4096-sample plan of the 32 kHz window) each filter gets from the band-limited filter tasks for these parameters
    (leaf_band_classes_f32), as an int32 tensor [F] on the parameters' device; None for a geometry without band tasks.
    ``pool_b``: the pooling biases the decision is taken for (what a forward call with them runs, and the default backward: the
    energy bound follows the bias, ABI 5); None: the strict decision, which looks at no bias (LEAF_ALGO_STRICT_BAND_CLASSES in the
    forward, LEAF_FLAG_BWD_STRICT_BAND_CLASSES in the backward)."""
    require_hip(kernel, "band_classes")
    dev = kernel.device
    kernel = _dev_f32(kernel, "kernel", dev)
    pool_w = _dev_f32(pool_w.reshape(-1), "pool_w", dev)
    pool_b = None if pool_b is None else _dev_f32(pool_b.reshape(-1), "pool_b", dev)
    F = kernel.shape[0]
    out = torch.empty(F, dtype=torch.int32, device=dev)
    rc = _call(dev, "leaf_band_classes_f32", kernel, pool_w, pool_b, F, K, hop, out, tolerate=(-8,),
               ws=lambda lib: max(lib.leaf_fft_tables_bytes(F, K, hop), lib.leaf_workspace_bytes(1, 8192, F, K, hop, ALGO_FFT_WG)))
    return None if rc == -8 else out


def workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    return torch.empty(max(nbytes, 4), dtype=torch.uint8, device=device)


CALL_SAMPLES = 1 << 31           # the C ABI indexes the samples of one call with 32 bits: B * T of a call stays below this


def batch_slices(B: int, T: int):
    """Slices of whole clips for a batch beyond one C-ABI call.  The C ABI indexes the samples of one call with 32 bits and
    refuses B * T >= 2^31 (LEAF_ERR_BAD_SHAPE); the reference's conv1d takes any batch (frontend.py:78-89), and clips are
    independent, so such a batch goes through in as few balanced slices as possible (the same plan as csrc/torch_binding.cpp)."""
    if T >= CALL_SAMPLES:
        raise RuntimeError(f"a clip of {T} samples is beyond the C ABI's 32-bit sample index")
    most = max(1, (CALL_SAMPLES - 1) // max(T, 1))
    calls = max(1, -(-B // most))
    per = -(-B // calls)
    return [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


def _pcm16_lands_on_staged(lib, x2: torch.Tensor, F: int, K: int, hop: int, algo: int) -> bool:
    """Whether one C-ABI forward call on the batch ``x2`` runs the staged kernels (the explicit selector, or what AUTO resolves to):
    they read and store float32 only, so an int16 waveform is widened and bfloat16 features are narrowed on the host around them."""
    B, T = x2.shape
    if B == 0 or B * T >= CALL_SAMPLES:
        return False
    sel = algo & 0xff
    if sel == ALGO_AUTO:
        with torch.cuda.device(x2.device):
            sel = lib.leaf_auto_algo(B, T, F, K, hop)
    return sel == ALGO_STAGED


def _forward(who: str, x, mix, params, K: int, hop: int, pcen: bool, log1p: bool, algo: int, out=None, save_raw: bool = False,
             peak_normalize: bool = False, out_bf16: bool = False):
    """``leaf_forward`` and, with ``mix = (perm, lam)``, ``leaf_forward_mix``.  The mixed call differs as in csrc/torch_binding.cpp:
    no bfloat16 x, one C-ABI call (a batch cannot be mixed across slices), the ``*_mix_*`` entry and workspace query."""
    lib = load()
    x2, flags = _unpack_x(x, who, mix is not None)
    dev = x.device
    B, T = x2.shape
    mix = () if mix is None else mix_args(*mix, B, dev)
    F = params[0].shape[0]
    prm, compression = _gather(dev, params, pcen, log1p)
    prm = [_ptr(p) for p in prm]
    TP = lib.leaf_num_frames(T, K, hop)
    if TP < 1:
        raise RuntimeError(f"bad shape B={B} T={T} K={K} hop={hop}")
    out_bf16, feat = _features(flags, out_bf16)
    if out is not None:
        _check_out(out, (B, F, TP), feat, dev)
    if (algo & 0xff) not in (ALGO_AUTO, ALGO_STAGED, ALGO_MFMA, ALGO_FFT, ALGO_FFT_WG, ALGO_FFT_SMALL):
        raise RuntimeError(f"unknown algorithm selector {algo & 0xff}")
    # the staged forward reads and stores float32 only (LEAF_ERR_UNSUPPORTED from the C ABI).  Where the call lands on it, bfloat16
    # features are narrowed here -- the same rounding, so the same bits -- and an int16 waveform is converted here -- the same values,
    # v / 32768 exactly (a mixed call writes its float32 mix into the workspace anyway; a batch beyond one call: slice by slice)
    staged = (out_bf16 or flags == FLAG_X_PCM16) and _pcm16_lands_on_staged(lib, x2, F, K, hop, algo)
    narrow = out_bf16 and staged
    if flags == FLAG_X_PCM16:
        peak_normalize = False                     # |v / 32768| <= 1: nothing to normalise for int16, and nothing is launched
        if staged and not mix:
            x2, flags = x2.float().mul_(2.0 ** -15), 0
    if out_bf16 and not narrow:
        flags |= FLAG_OUT_BF16
    if peak_normalize:
        flags |= FLAG_PEAKNORM                     # forward of the peak-normalised clips, the scale folded into the finalize
    flags |= compression
    if B == 0:
        # the empty batch: (0, F, T') like the reference (frontend.py:78-89 -> convolution.py:97); nothing is launched
        # (`out`, the selector and the flags are validated above, and a caller-supplied `out` is what comes back)
        if save_raw and (flags & FLAG_PEAKNORM):
            raise RuntimeError("the folded PeakNormalization prologue is forward-only")
        empty = out if out is not None else torch.empty((0, F, TP), dtype=feat, device=dev)
        return (empty, torch.empty((0, F, TP), dtype=torch.float32, device=dev)) if save_raw else empty
    if B * T >= CALL_SAMPLES:
        if mix:
            raise RuntimeError(f"{who}: a batch beyond one C-ABI call (B * T >= 2^31) cannot be mixed across its slices")
        # one C-ABI call per slice of whole clips, into the one output (see batch_slices: it refuses a clip beyond one call first)
        slices = batch_slices(B, T)
        raw = torch.empty((B, F, TP), dtype=torch.float32, device=dev) if save_raw else None
        if out is None:
            out = torch.empty((B, F, TP), dtype=feat, device=dev)
        for b0, b1 in slices:
            r = _forward(who, x2[b0:b1], None, params, K, hop, pcen, log1p, algo, out[b0:b1], save_raw, peak_normalize, out_bf16)
            if save_raw:
                raw[b0:b1].copy_(r[1])
        return (out, raw) if save_raw else out
    res = out if out is not None and not narrow else torch.empty((B, F, TP), dtype=torch.float32 if narrow else feat, device=dev)
    raw = torch.empty((B, F, TP), dtype=torch.float32, device=dev) if save_raw else None
    head = (_ptr(x2), _ptr(mix[0]), _ptr(mix[1]), B, T) if mix else (_ptr(x2), B, T)
    with torch.cuda.device(dev):
        ws = workspace((lib.leaf_forward_mix_workspace_bytes if mix else lib.leaf_workspace_bytes)(B, T, F, K, hop, algo), dev)
        if save_raw:
            entry = lib.leaf_forward_save_mix_f32 if mix else lib.leaf_forward_save_f32
            rc = entry(*head, *prm, F, K, hop, flags, algo, _ptr(res), _ptr(raw), _ptr(ws), ws.numel(), stream_ptr(dev))
        else:
            entry = lib.leaf_forward_mix_f32 if mix else lib.leaf_forward_f32
            rc = entry(*head, *prm, F, K, hop, flags, algo, _ptr(res), _ptr(ws), ws.numel(), stream_ptr(dev))
    if rc:
        check(rc, "leaf_forward" + ("_save" if save_raw else "") + ("_mix" if mix else "") + "_f32")
    if narrow:
        res = res.to(torch.bfloat16) if out is None else out.copy_(res)
    return (res, raw) if save_raw else res


def leaf_forward(x: torch.Tensor, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int,
                 pcen: bool = True, log1p: bool = False, algo: int = ALGO_AUTO,
                 out: Optional[torch.Tensor] = None, save_raw: bool = False, peak_normalize: bool = False,
                 out_bf16: bool = False):
    """x (B,1,T) or (B,T) float32 (bfloat16, or int16 PCM: a sample v means v / 32768) on a HIP device -> (B,F,T').  Wraps leaf_forward_f32 (leaf_forward_save_f32 when
    ``save_raw``: then returns (out, pooled_raw) for the backward).  ``out_bf16``: bfloat16 features from a float32 or int16
    waveform (LEAF_FLAG_OUT_BF16) -- the float32 call's result rounded to nearest even where the kernels store it; the mode is
    explicit, never inferred from a tensor's dtype (redundant for a bfloat16 ``x``)."""
    return _forward("leaf_forward", x, None, (kernel, pool_w, pool_b, alpha, delta, root, ema_w), K, hop, pcen, log1p, algo, out, save_raw,
                    peak_normalize, out_bf16)


def backward_flags(pcen: bool = False, staged: bool = False, mfma: bool = False, full_transforms: bool = False,
                   strict_band_classes: bool = False, log1p: bool = False, io_flags: int = 0) -> int:
    """The ``flags`` of leaf_backward_f32 / leaf_backward_mix_f32 (``full_transforms``: no band-limited filter tasks in the backward;
    ``log1p`` is ignored with PCEN on, as in the forward; ``io_flags``: the waveform's and the features' dtype bits)."""
    return ((FLAG_PCEN if pcen else 0) | (FLAG_BWD_STAGED if staged else 0) | (FLAG_BWD_MFMA if mfma else 0) |
            (FLAG_BWD_FULL_TRANSFORMS if full_transforms else 0) | (FLAG_BWD_STRICT_BAND_CLASSES if strict_band_classes else 0) |
            (FLAG_LOG1P if log1p and not pcen else 0) | io_flags)


def _backward(who: str, x, mix, params, K: int, hop: int, grad_out: torch.Tensor, flags: int, need_dx: bool, pooled_raw, out_bf16: bool):
    """``leaf_backward`` and, with ``mix = (perm, lam)``, ``leaf_backward_mix`` (one C-ABI call, no dL/dx, the ``*_mix_*`` entry and
    workspace query).  ``flags``: the path and compression bits of ``backward_flags``; the dtype bits are added here."""
    pcen = bool(flags & FLAG_PCEN)
    lib = load()
    x2, io_flags = _unpack_x(x, who, mix is not None)
    dev = x.device
    if io_flags == FLAG_X_PCM16 and need_dx:
        raise RuntimeError("an int16 (PCM) input has no gradient: need_dx=True needs a float32 or bfloat16 x")
    B, T = x2.shape
    mix = () if mix is None else mix_args(*mix, B, dev)
    F = params[0].shape[0]
    prm, _ = _gather(dev, params, pcen, False)
    out_bf16 = bool(out_bf16) and io_flags != FLAG_IO_BF16     # (a bfloat16 x: grad_out is bfloat16 already)
    if io_flags == FLAG_IO_BF16 or out_bf16:
        if grad_out.dtype != torch.bfloat16 or grad_out.device != dev:
            raise RuntimeError(f"grad_out must be bfloat16 on {dev} {'with out_bf16=True' if out_bf16 else 'when x is bfloat16'}, "
                               f"got {grad_out.dtype} on {grad_out.device}")
        go = grad_out.detach().contiguous()
        io_flags |= FLAG_OUT_BF16 if out_bf16 else 0
    else:
        go = _dev_f32(grad_out, "grad_out", dev)
    TP = lib.leaf_num_frames(T, K, hop)
    if tuple(go.shape) != (B, F, TP):
        raise RuntimeError(f"grad_out has shape {tuple(go.shape)}, expected {(B, F, TP)}")
    grads = [torch.empty_like(p) for p in prm[:3]] + [torch.empty(F, dtype=torch.float32, device=dev) if pcen else None for _ in range(4)]
    g_x = torch.empty_like(x2) if need_dx else None
    if B == 0:                                     # the sum over no clips: zero parameter gradients, nothing launched
        for g in grads:
            if g is not None:
                g.zero_()
    elif B * T >= CALL_SAMPLES:
        if mix:
            raise RuntimeError(f"{who}: a batch beyond one C-ABI call (B * T >= 2^31) cannot be mixed across its slices")
        # slices of whole clips (batch_slices); parameter gradients added in slice order (fixed: bit-reproducible)
        total = None
        for b0, b1 in batch_slices(B, T):
            g = _backward(who, x2[b0:b1], None, params, K, hop, go[b0:b1], flags, need_dx, None if pooled_raw is None else pooled_raw[b0:b1],
                          out_bf16)
            if need_dx:
                g_x[b0:b1].copy_(g[7])
            total = list(g[:7]) if total is None else [None if a is None else a.add_(b) for a, b in zip(total, g[:7])]
        return (*total, g_x)
    else:
        flags |= io_flags
        tail = (F, K, hop, flags, _ptr(go), _ptr(pooled_raw), *[_ptr(g) for g in grads], _ptr(g_x))
        with torch.cuda.device(dev):
            # sized for the path these flags select (a few MB for the overlap-save backward, not the staged path's dL/dy)
            if mix:
                entry = "leaf_backward_mix_f32"
                ws = workspace(lib.leaf_backward_mix_workspace_bytes(B, T, F, K, hop, flags), dev)
                rc = lib.leaf_backward_mix_f32(_ptr(x2), _ptr(mix[0]), _ptr(mix[1]), B, T, *[_ptr(p) for p in prm], *tail, _ptr(ws), ws.numel(), stream_ptr(dev))
            else:
                entry = "leaf_backward_f32"
                ws = workspace(lib.leaf_backward_workspace_bytes(B, T, F, K, hop, flags, int(need_dx)), dev)
                rc = lib.leaf_backward_f32(_ptr(x2), B, T, *[_ptr(p) for p in prm], *tail, _ptr(ws), ws.numel(), stream_ptr(dev))
        if rc:
            check(rc, entry)
    return (grads[0], grads[1].reshape(params[1].shape), *grads[2:], g_x)


def leaf_backward(x, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int, grad_out: torch.Tensor,
                  pcen: bool = True, need_dx: bool = False, staged: bool = False,
                  pooled_raw: Optional[torch.Tensor] = None, mfma: bool = False, full_transforms: bool = False,
                  strict_band_classes: bool = False, log1p: bool = False, out_bf16: bool = False):
    """Gradients of the forward w.r.t. (kernel, pool_w, pool_b, alpha, delta, root, ema_w[, x]).  Wraps leaf_backward_f32.
    ``staged`` / ``mfma`` force the staged kernels / the fused MFMA backward (default: the overlap-save backward where
    it applies, else MFMA, else staged).  ``log1p``: the backward of the log1p-compressed forward (PCEN off; ignored with
    PCEN on, as in the forward).  A bfloat16 ``x`` selects bfloat16 I/O: ``grad_out`` is bfloat16 too and dL/dx comes back
    in bfloat16; the parameter gradients and ``pooled_raw`` are float32.  An int16 ``x`` (PCM, v / 32768) keeps ``grad_out`` float32
    and has no dL/dx (``need_dx=True`` raises).  ``out_bf16`` (LEAF_FLAG_OUT_BF16, the backward of ``leaf_forward(..., out_bf16=True)``):
    ``grad_out`` alone is bfloat16, widened where the kernels read it -- the gradients are those of the call on ``grad_out.float()``
    bit for bit; ``x`` stays float32 (dL/dx float32) or int16."""
    return _backward("leaf_backward", x, None, (kernel, pool_w, pool_b, alpha, delta, root, ema_w), K, hop, grad_out,
                     backward_flags(pcen, staged, mfma, full_transforms, strict_band_classes, log1p), need_dx, pooled_raw, out_bf16)


CALL_ELEMENTS = 1 << 31          # leaf_backward_head_f32 indexes pooled_raw with 32 bits: B * F * T' of a call stays below this


def leaf_backward_head(pooled_raw: torch.Tensor, grad_out: torch.Tensor, pool_b: torch.Tensor, alpha, delta, root, ema_w,
                       pcen: bool = True, log1p: bool = False, out_bf16: bool = False):
    """The head-only backward (leaf_backward_head_f32): ``(g_pool_b, g_alpha, g_delta, g_root, g_ema_w)`` from the saved pre-floor
    pooled tensor ``pooled_raw`` (B, F, T') and ``grad_out`` alone, one launch -- the gradients a ``Leaf`` with a frozen Gabor kernel and
    pooling width needs; the PCEN four are None with ``pcen=False``.  ``pool_b`` is taken only for its shape and device.  ``log1p``:
    the backward of the log1p-compressed forward (PCEN off; ignored with PCEN on).  ``out_bf16``: ``grad_out`` is bfloat16, widened
    where the kernel reads it -- the gradients are those of the call on ``grad_out.float()`` bit for bit."""
    # shapes and dtypes first, then the devices: every error is raised here, before the library is loaded
    if pooled_raw.dim() != 3 or pooled_raw.shape[1] < 1 or pooled_raw.shape[2] < 1:
        raise RuntimeError(f"pooled_raw must be (B, F, T') with F, T' >= 1, got {tuple(pooled_raw.shape)}")
    B, F, TP = pooled_raw.shape
    if pooled_raw.dtype != torch.float32:
        raise RuntimeError(f"pooled_raw must be float32, got {pooled_raw.dtype}")
    want = torch.bfloat16 if out_bf16 else torch.float32
    if grad_out.dtype != want:
        raise RuntimeError(f"grad_out must be {want} with out_bf16={bool(out_bf16)}, got {grad_out.dtype}")
    if tuple(grad_out.shape) != (B, F, TP):
        raise RuntimeError(f"grad_out has shape {tuple(grad_out.shape)}, expected {(B, F, TP)}")
    if pool_b.numel() != F:
        raise RuntimeError(f"pool_b must hold one bias per filter ({F}), got {tuple(pool_b.shape)}")
    names = ("alpha", "delta", "root", "ema_w")
    pc = (alpha, delta, root, ema_w) if pcen else ()
    for t, name in zip(pc, names):
        if t is None or t.numel() != F:
            raise RuntimeError(f"{name} must hold one entry per filter ({F}) with pcen=True")
    require_hip(pooled_raw, "leaf_backward_head")
    dev = pooled_raw.device
    raw = _dev_f32(pooled_raw, "pooled_raw", dev)
    if grad_out.device != dev or pool_b.device != dev:
        raise RuntimeError(f"grad_out and pool_b must be on {dev}, got {grad_out.device} and {pool_b.device}")
    go = grad_out.detach().contiguous()
    pc = [_dev_f32(t, name, dev) for t, name in zip(pc, names)] if pcen else [None] * 4
    flags = (FLAG_PCEN if pcen else (FLAG_LOG1P if log1p else 0)) | (FLAG_OUT_BF16 if out_bf16 else 0)
    grads = [torch.empty(pool_b.shape, dtype=torch.float32, device=dev)] + [torch.empty(F, dtype=torch.float32, device=dev) if pcen else None
                                                                            for _ in range(4)]
    if B == 0:                                     # the sum over no clips: zero gradients, nothing launched
        for g in grads:
            if g is not None:
                g.zero_()
    elif B * F * TP >= CALL_ELEMENTS:
        # slices over B, the gradients added in slice order (fixed: bit-reproducible), like _backward
        if F * TP >= CALL_ELEMENTS:
            raise RuntimeError(f"a clip of {F} x {TP} pooled values is beyond the C ABI's 32-bit index")
        total = None
        for b0, b1 in batch_slices(B, F * TP):
            g = leaf_backward_head(raw[b0:b1], go[b0:b1], pool_b, *pc, pcen=pcen, log1p=log1p, out_bf16=out_bf16)
            total = list(g) if total is None else [None if a is None else a.add_(b) for a, b in zip(total, g)]
        return tuple(total)
    else:
        _call(dev, "leaf_backward_head_f32", raw, go, B, TP, F, *[_ptr(t) for t in pc], flags, *[_ptr(g) for g in grads],
              ws=lambda lib: lib.leaf_backward_head_workspace_bytes(B, TP, F, flags))
    return tuple(grads)


def mix_args(perm, lam, B: int, device: torch.device):
    """The two mixup buffers of a call, as the C ABI reads them: ``perm`` (any integer tensor or sequence of length B) as int32 and
    ``lam`` (length B) as float32, both on ``device``.  A ``perm`` that arrives on the CPU is validated there: an index outside
    [0, B) raises ValueError before anything is launched (a device-side ``perm`` is clamped by the kernels instead: checking it
    would be a synchronisation per step)."""
    if not isinstance(perm, torch.Tensor):
        perm = torch.as_tensor(perm)
    if perm.dtype.is_floating_point or perm.dtype.is_complex or perm.dtype == torch.bool:
        raise TypeError(f"perm must be an integer tensor or sequence, got {perm.dtype}")
    perm = perm.reshape(-1)
    if perm.numel() != B:
        raise ValueError(f"perm has {perm.numel()} entries, expected one per clip ({B})")
    if perm.device.type == "cpu" and B and (int(perm.min()) < 0 or int(perm.max()) >= B):
        raise ValueError(f"perm holds an index outside [0, {B})")
    if not isinstance(lam, torch.Tensor):
        lam = torch.as_tensor(lam, dtype=torch.float32)
    lam = lam.reshape(-1)
    if lam.numel() != B:
        raise ValueError(f"lam has {lam.numel()} entries, expected one per clip ({B})")
    if lam.dtype != torch.float32:
        raise RuntimeError(f"lam must be float32, got {lam.dtype}")
    return (perm.detach().to(device=device, dtype=torch.int32).contiguous(), lam.detach().to(device=device).contiguous())


def mixup(x: torch.Tensor, perm, lam) -> torch.Tensor:
    """The mixed waveform itself (leaf_mixup_f32): x (B,1,T) or (B,T), float32 or int16 PCM (v / 32768) ->
    float32 of the same shape, ``x * lam + x[perm] * (1 - lam)`` per clip with separately rounded fp32 operations."""
    x2, flags = _unpack_x(x, "mixup", mixed=True)
    B, T = x2.shape
    dev = x2.device
    perm, lam = mix_args(perm, lam, B, dev)
    out = torch.empty((B, T), dtype=torch.float32, device=dev)
    if B * T >= CALL_SAMPLES:
        raise RuntimeError("mixup: a batch beyond one C-ABI call (B * T >= 2^31) cannot be mixed across its slices")
    if B and T:
        _call(dev, "leaf_mixup_f32", x2, B, T, perm, lam, flags, out)
    return out.reshape(x.shape)


def leaf_forward_mix(x: torch.Tensor, perm, lam, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int,
                     pcen: bool = True, log1p: bool = False, algo: int = ALGO_AUTO, save_raw: bool = False, out_bf16: bool = False):
    """``leaf_forward`` of the mixed batch ``x * lam + x[perm] * (1 - lam)`` without materialising it where the kernels mix in their
    loads (leaf_forward_mix_f32 / leaf_forward_save_mix_f32).  x float32 or int16 PCM; bfloat16 raises.  ``out_bf16``: bfloat16
    features (LEAF_FLAG_OUT_BF16), the float32 result rounded where it is stored."""
    return _forward("leaf_forward_mix", x, (perm, lam), (kernel, pool_w, pool_b, alpha, delta, root, ema_w), K, hop, pcen, log1p, algo,
                    save_raw=save_raw, out_bf16=out_bf16)


def leaf_backward_mix(x, perm, lam, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int, grad_out: torch.Tensor,
                      pcen: bool = True, staged: bool = False, pooled_raw: Optional[torch.Tensor] = None, mfma: bool = False,
                      full_transforms: bool = False, strict_band_classes: bool = False, log1p: bool = False, out_bf16: bool = False):
    """Parameter gradients of ``leaf_forward_mix`` (leaf_backward_mix_f32): the seven of ``leaf_backward`` and None for dL/dx,
    which a mixed call does not have.  ``out_bf16``: ``grad_out`` is bfloat16 (LEAF_FLAG_OUT_BF16), widened where it is read."""
    return _backward("leaf_backward_mix", x, (perm, lam), (kernel, pool_w, pool_b, alpha, delta, root, ema_w), K, hop, grad_out,
                     backward_flags(pcen, staged, mfma, full_transforms, strict_band_classes, log1p), False, pooled_raw, out_bf16)


def leaf_forward_profiled(x, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int, pcen: bool = True,
                          algo: int = ALGO_AUTO, log1p: bool = False):
    """Measurement call: returns (out, [taps_ms, fused_ms, finalize_ms]) from HIP events on the current stream.  Same flags
    as ``leaf_forward`` (PCEN on / off, log1p, bfloat16 I/O when ``x`` is bfloat16, PCM input when it is int16), so every BASELINE config can be timed."""
    lib = load()
    x2, flags = _unpack_x(x, "leaf_forward_profiled")
    dev = x.device
    B, T = x2.shape
    F = kernel.shape[0]
    prm, compression = _gather(dev, (kernel, pool_w, pool_b, alpha, delta, root, ema_w), pcen, log1p)
    _, feat = _features(flags)
    out = torch.empty((B, F, lib.leaf_num_frames(T, K, hop)), dtype=feat, device=dev)
    ms = (ctypes.c_float * 3)()
    _call(dev, "leaf_forward_profiled_f32", x2, B, T, *prm, F, K, hop, flags | compression, algo, out,
          ws=lambda lib: lib.leaf_workspace_bytes(B, T, F, K, hop, algo), after=(ms,))
    return out, [float(v) for v in ms]


def gabor_taps(kernel: torch.Tensor, K: int) -> torch.Tensor:
    require_hip(kernel, "gabor_taps")
    kernel = _dev_f32(kernel, "kernel", kernel.device)
    F = kernel.shape[0]
    taps = torch.empty((2 * F, K), dtype=torch.float32, device=kernel.device)
    _call(kernel.device, "leaf_gabor_taps_f32", kernel, F, K, taps)
    return taps


def lowpass_window(pool_w: torch.Tensor, K: int) -> torch.Tensor:
    require_hip(pool_w, "lowpass_window")
    w = _dev_f32(pool_w.reshape(-1), "pool_w", pool_w.device)
    g = torch.empty((w.numel(), K), dtype=torch.float32, device=w.device)
    _call(w.device, "leaf_lowpass_window_f32", w, w.numel(), K, g)
    return g


def gabor_conv(x: torch.Tensor, kernel: torch.Tensor, K: int) -> torch.Tensor:
    require_hip(x, "gabor_conv")
    if x.dim() != 3 or x.shape[1] != 1:
        raise RuntimeError(f"expected input of shape (B,1,T), got {tuple(x.shape)}")
    dev = x.device
    x2 = _dev_f32(x[:, 0, :], "x", dev)
    kernel = _dev_f32(kernel, "kernel", dev)
    B, T = x2.shape; F = kernel.shape[0]
    y = torch.empty((B, 2 * F, T), dtype=torch.float32, device=dev)
    if B:                                          # (the empty batch passes through every stage as an empty tensor)
        _call(dev, "leaf_gabor_conv_f32", x2, B, T, kernel, F, K, y, ws=2 * F * K * 4)
    return y


def squared_modulus(y: torch.Tensor) -> torch.Tensor:
    require_hip(y, "squared_modulus")
    y = _dev_f32(y, "y", y.device)
    B, C2, T = y.shape
    if C2 % 2:
        raise RuntimeError("channel count must be even (interleaved re/im)")
    e = torch.empty((B, C2 // 2, T), dtype=torch.float32, device=y.device)
    if B:
        _call(y.device, "leaf_squared_modulus_f32", y, B, C2 // 2, T, e)
    return e


def gaussian_lowpass(e: torch.Tensor, pool_w: torch.Tensor, pool_b: Optional[torch.Tensor], K: int, hop: int) -> torch.Tensor:
    require_hip(e, "gaussian_lowpass")
    dev = e.device
    e = _dev_f32(e, "e", dev)
    B, F, T = e.shape
    w = _dev_f32(pool_w.reshape(-1), "pool_w", dev)
    b = None if pool_b is None else _dev_f32(pool_b, "pool_b", dev)
    pooled = torch.empty((B, F, load().leaf_num_frames(T, K, hop)), dtype=torch.float32, device=dev)
    if B:
        _call(dev, "leaf_gaussian_lowpass_f32", e, B, F, T, w, b, K, hop, pooled, ws=F * K * 4)
    return pooled


def _ema_w(ema_w: torch.Tensor, F: int, dev: torch.device):
    """The smoother's coefficients as the kernels read them, one per channel (a shared coefficient expanded), and the fold of their
    per-channel gradient back into ``ema_w``'s own shape (summed over the channels when the coefficient is shared)."""
    shared = ema_w.numel() == 1
    w = _dev_f32(ema_w.reshape(-1).expand(F) if shared else ema_w, "ema_w", dev)
    return w, lambda gw: (gw.sum() if shared else gw).reshape(ema_w.shape)


def ema(p: torch.Tensor, ema_w: torch.Tensor) -> torch.Tensor:
    require_hip(p, "ema")
    dev = p.device
    p = _dev_f32(p, "p", dev); B, F, TP = p.shape
    w, _ = _ema_w(ema_w, F, dev)
    out = torch.empty_like(p)
    if B:
        _call(dev, "leaf_ema_f32", p, B, F, TP, w, out)
    return out


def pcen(p: torch.Tensor, alpha, delta, root, ema_w, floor: float) -> torch.Tensor:
    require_hip(p, "pcen")
    dev = p.device
    p = _dev_f32(p, "p", dev); B, F, TP = p.shape
    alpha, delta, root = (_dev_f32(t, n, dev) for t, n in ((alpha, "alpha"), (delta, "delta"), (root, "root")))
    w, _ = _ema_w(ema_w, F, dev)
    out = torch.empty_like(p)
    if B:
        _call(dev, "leaf_pcen_f32", p, B, F, TP, alpha, delta, root, w, float(floor), out)
    return out


def stream_state(B: int, F: int, K: int, hop: int, flags: int, device: torch.device) -> torch.Tensor:
    """The device-resident state of one fused stream (leaf_stream_state_bytes: two history halves and the smoother state),
    uninitialised -- a stream's first step reads none of it."""
    nbytes = load().leaf_stream_state_bytes(B, F, K, hop, flags)
    if nbytes == 0:
        raise RuntimeError(f"leaf_stream_state_bytes: no one-launch streaming kernel for window {K} / hop {hop}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def stream_step(chunk_ptr: int, B: int, Tc: int, chunk_stride: int, state: torch.Tensor, hist_len: int, parity: int, drop_samples: int,
                first: int, n: int, started: bool, params, F: int, K: int, hop: int, flags: int, out_ptr: int,
                device: torch.device) -> None:
    """leaf_stream_step_f32 on the current stream of ``device``: one launch.  ``params``: the seven parameter tensors (float32,
    contiguous, on the device; the four PCEN ones None without FLAG_PCEN); ``chunk_ptr`` / ``out_ptr``: device addresses
    (0 where Tc / n is 0)."""
    _call(device, "leaf_stream_step_f32", ctypes.c_void_p(chunk_ptr), B, Tc, chunk_stride, state, state.numel(), hist_len, parity,
          drop_samples, first, n, int(started), *params, F, K, hop, flags, ctypes.c_void_p(out_ptr))


class StreamSlot(ctypes.Structure):
    """leaf_stream_slot (include/leaf_hip.h): where one slot of a bank stands in one step."""
    _fields_ = [(name, ctypes.c_int) for name in ("idle", "hist_len", "Tc", "parity", "drop_samples", "first", "n", "started", "end_first", "end_n")]


def stream_bank_step(chunk_ptr: int, chunk_stride: int, slots, n_max: int, state: torch.Tensor, params, F: int, K: int, hop: int,
                     flags: int, out_ptr: int, device: torch.device) -> None:
    """leaf_stream_bank_step_f32 on the current stream of ``device``.  ``slots``: a ctypes array of ``StreamSlot`` (host memory, read
    before the call returns); ``params`` as in ``stream_step``."""
    _call(device, "leaf_stream_bank_step_f32", ctypes.c_void_p(chunk_ptr), chunk_stride, len(slots), ctypes.cast(slots, ctypes.c_void_p), n_max,
          state, state.numel(), *params, F, K, hop, flags, ctypes.c_void_p(out_ptr))


# ---- stage backwards (what autograd derives for a sub-module called on its own; modules.py wraps them) ----------

def pcen_stream(p: torch.Tensor, alpha, delta, root, ema_w, floor: float, ema_state: Optional[torch.Tensor] = None,
                log1p: bool = False):
    """leaf_pcen_stream_f32: PCEN of one chunk (B,F,n) of floored pooled frames with the smoother state carried between
    calls.  Returns (out, new_state); ``alpha is None``: no PCEN (state stays None)."""
    require_hip(p, "pcen_stream")
    dev = p.device
    p = _dev_f32(p, "p", dev)
    B, F, n = p.shape
    out = torch.empty_like(p)
    if alpha is None:
        _call(dev, "leaf_pcen_stream_f32", p, B, F, n, None, None, None, None, float(floor), int(log1p), None, None, out)
        return out, None
    alpha, delta, root, ema_w = (_dev_f32(t, nm, dev) for t, nm in
                                 ((alpha, "alpha"), (delta, "delta"), (root, "root"), (ema_w, "ema_w")))
    new_state = torch.empty((B, F), dtype=torch.float32, device=dev)
    if ema_state is not None:
        ema_state = _dev_f32(ema_state, "ema_state", dev)
    _call(dev, "leaf_pcen_stream_f32", p, B, F, n, alpha, delta, root, ema_w, float(floor), 0, ema_state, new_state, out)
    return out, new_state


def _stage_ws(stage: int, B: int, T: int, F: int, K: int, hop: int):
    return lambda lib: lib.leaf_stage_backward_workspace_bytes(stage, B, T, F, K, hop)


def gabor_conv_backward(x, kernel, K: int, grad_y, need_dk: bool = True, need_dx: bool = False):
    require_hip(x, "gabor_conv_backward")
    dev = x.device
    x2 = _dev_f32(x[:, 0, :], "x", dev)
    kernel = _dev_f32(kernel, "kernel", dev)
    gy = _dev_f32(grad_y, "grad_y", dev)
    B, T = x2.shape; F = kernel.shape[0]
    gk = torch.empty_like(kernel) if need_dk else None
    gx = torch.empty_like(x2) if need_dx else None
    if B == 0:                                     # the sum over no clips
        gk = gk.zero_() if need_dk else None
    else:
        _call(dev, "leaf_gabor_conv_backward_f32", x2, B, T, kernel, F, K, gy, gk, gx, ws=_stage_ws(STAGE_GABOR_CONV, B, T, F, K, 1))
    return gk, (gx.reshape(x.shape) if need_dx else None)


def squared_modulus_backward(y, grad_e):
    require_hip(y, "squared_modulus_backward")
    dev = y.device
    y = _dev_f32(y, "y", dev); ge = _dev_f32(grad_e, "grad_e", dev)
    B, C2, T = y.shape
    gy = torch.empty_like(y)
    if B:
        _call(dev, "leaf_squared_modulus_backward_f32", y, ge, B, C2 // 2, T, gy)
    return gy


def gaussian_lowpass_backward(e, pool_w, K: int, hop: int, grad_pooled, need_de: bool = True, need_dw: bool = True,
                              need_db: bool = True):
    require_hip(e, "gaussian_lowpass_backward")
    dev = e.device
    e = _dev_f32(e, "e", dev); gp = _dev_f32(grad_pooled, "grad_pooled", dev)
    w = _dev_f32(pool_w.reshape(-1), "pool_w", dev)
    B, F, T = e.shape
    ge = torch.empty_like(e) if need_de else None
    gw = torch.empty_like(w) if need_dw else None
    gb = torch.empty_like(w) if need_db else None
    if B == 0:
        for g in (gw, gb):
            if g is not None:
                g.zero_()
    else:
        _call(dev, "leaf_gaussian_lowpass_backward_f32", e, gp, B, F, T, w, K, hop, ge, gw, gb, ws=_stage_ws(STAGE_LOWPASS, B, T, F, K, hop))
    return ge, (gw.reshape(pool_w.shape) if need_dw else None), gb


def ema_backward(p, ema_w, grad_ema):
    require_hip(p, "ema_backward")
    dev = p.device
    p = _dev_f32(p, "p", dev); g = _dev_f32(grad_ema, "grad_ema", dev)
    B, F, TP = p.shape
    w, fold = _ema_w(ema_w, F, dev)
    gp, gw = torch.empty_like(p), torch.empty(F, dtype=torch.float32, device=dev)
    if B == 0:
        gw.zero_()
    else:
        _call(dev, "leaf_ema_backward_f32", p, g, B, F, TP, w, gp, gw, ws=_stage_ws(STAGE_EMA, B, TP, F, 1, 1))
    return gp, fold(gw)


def pcen_backward(p, alpha, delta, root, ema_w, floor: float, grad_out):
    require_hip(p, "pcen_backward")
    dev = p.device
    p = _dev_f32(p, "p", dev); g = _dev_f32(grad_out, "grad_out", dev)
    B, F, TP = p.shape
    alpha, delta, root = (_dev_f32(t, n, dev) for t, n in ((alpha, "alpha"), (delta, "delta"), (root, "root")))
    w, fold = _ema_w(ema_w, F, dev)
    gp = torch.empty_like(p)
    ga, gd, gr, gw = (torch.empty(F, dtype=torch.float32, device=dev) for _ in range(4))
    if B == 0:
        for g_ in (ga, gd, gr, gw):
            g_.zero_()
    else:
        _call(dev, "leaf_pcen_backward_f32", p, g, B, F, TP, alpha, delta, root, w, float(floor), gp, ga, gd, gr, gw,
              ws=_stage_ws(STAGE_PCEN, B, TP, F, 1, 1))
    return gp, ga, gd, gr, fold(gw)


def peak_normalize(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Clips (rows of a (B,T) or (B,1,T) tensor) whose peak |x| exceeds 1 are divided by it; wraps leaf_peak_normalize_f32."""
    require_hip(x, "peak_normalize")
    per_clip = 1
    for d in x.shape[1:]:
        per_clip *= int(d)
    x2 = _dev_f32(x.reshape(x.shape[0], per_clip), "x", x.device)        # (an explicit extent: -1 is ambiguous for B = 0)
    B, T = x2.shape
    if out is None:
        out = torch.empty_like(x2)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != x2.numel():
        raise RuntimeError("out must be a contiguous float32 tensor of the input's size")
    if B:
        _call(x.device, "leaf_peak_normalize_f32", x2, B, T, out)
    return out.reshape(x.shape)


PAD_ZERO, PAD_MIN, PAD_REPLICATE, PAD_WRAP = 0, 1, 2, 3     # pad_mode of leaf_assemble_clips_f32
PAD_MODES = {"zero": PAD_ZERO, "min": PAD_MIN, "replicate": PAD_REPLICATE, "wrap": PAD_WRAP}
ASSEMBLE_RESIDENT_MAX = 32765    # csrc/leaf_clips.hpp (kClipResidentMax): clips up to this size stay in registers, longer ones are gathered twice
ASSEMBLE_NOISE_RESIDENT_MAX = 32765   # ... and the cut-over of the instances with noise (kClipNoiseResidentMax): the same eight chunks per lane


def _plan_ints(t, name: str, B: int) -> torch.Tensor:
    """One integer array of a clip plan, flat, with one entry per clip (ValueError otherwise); it stays on its device."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor or sequence, got {t.dtype}")
    t = t.detach().reshape(-1)
    if t.numel() != B:
        raise ValueError(f"{name} has {t.numel()} entries, expected one per clip ({B})")
    return t


def clip_plan(store_len: int, rec_off, rec_len, start, pad_mode, size: int, gain=None, masks=None):
    """The plan of ``assemble_clips`` as flat tensors on the devices they arrived on, checked as far as the host can see it.  An array
    that arrives on the CPU is validated here (ValueError, before anything is launched): ``rec_off`` in [0, store_len], ``rec_len`` in
    [0, store_len - rec_off], ``start`` in [0, max(L, size) - size], ``pad_mode`` in 0..3.  A device-side array is not read back -- that
    would be a synchronisation per step -- and the kernel clamps it instead (include/leaf_hip.h).  Lengths, and the shape (B, M, 2) of
    ``masks``, are checked wherever the arrays live.  Returns (B, rec_off, rec_len, start, pad_mode, gain, masks)."""
    size = int(size)
    if not 1 <= size < CALL_SAMPLES:
        raise ValueError(f"size must be in [1, 2^31), got {size}")
    if not isinstance(rec_off, torch.Tensor):
        rec_off = torch.as_tensor(rec_off)
    B = rec_off.numel()
    rec_off, rec_len, start, pad_mode = (_plan_ints(t, n, B) for t, n in ((rec_off, "rec_off"), (rec_len, "rec_len"), (start, "start"),
                                                                          (pad_mode, "pad_mode")))
    on_cpu = lambda t: t.device.type == "cpu" and B > 0
    if on_cpu(rec_off) and (int(rec_off.min()) < 0 or int(rec_off.max()) > store_len):
        raise ValueError(f"rec_off holds an offset outside [0, {store_len}] (the store's length)")
    if on_cpu(rec_len):
        if int(rec_len.min()) < 0 or int(rec_len.max()) >= CALL_SAMPLES:
            raise ValueError("rec_len holds a length outside [0, 2^31)")
        room = store_len - rec_off.long() if on_cpu(rec_off) else store_len
        if bool((rec_len.long() > room).any()):
            raise ValueError(f"rec_len holds a recording that ends behind the store ({store_len} samples)")
    if on_cpu(start):
        if int(start.min()) < 0:
            raise ValueError("start holds a negative offset")
        if on_cpu(rec_len) and bool((start.long() > (rec_len.long() - size).clamp_(min=0)).any()):
            raise ValueError(f"start holds an offset outside [0, max(rec_len, {size}) - {size}]")
    if on_cpu(pad_mode) and (int(pad_mode.min()) < PAD_ZERO or int(pad_mode.max()) > PAD_WRAP):
        raise ValueError("pad_mode holds a value outside 0..3 (zero, min, replicate, wrap)")
    if gain is not None:
        if not isinstance(gain, torch.Tensor):
            gain = torch.as_tensor(gain, dtype=torch.float32)
        gain = gain.detach().reshape(-1)
        if gain.numel() != B:
            raise ValueError(f"gain has {gain.numel()} entries, expected one per clip ({B})")
        if gain.dtype != torch.float32:
            raise RuntimeError(f"gain must be float32, got {gain.dtype}")
    if masks is not None:
        if not isinstance(masks, torch.Tensor):
            masks = torch.as_tensor(masks)
        if masks.dtype.is_floating_point or masks.dtype.is_complex or masks.dtype == torch.bool:
            raise TypeError(f"masks must be an integer tensor, got {masks.dtype}")
        if masks.dim() != 3 or masks.shape[0] != B or masks.shape[2] != 2:
            raise ValueError(f"masks has shape {tuple(masks.shape)}, expected ({B}, M, 2): M spans (t0, n) per clip")
        masks = None if masks.shape[1] == 0 else masks.detach()
    return B, rec_off, rec_len, start, pad_mode, gain, masks


def noise_coefficients(coeff) -> torch.Tensor:
    """The (B, 2) float32 pairs (c, c') of leaf_assemble_clips_noise_f32 from AddRandomNoise's float64 ``coeff`` = r / (1 + r):
    c = fp32(coeff), c' = fp32(1 - coeff) with the subtraction in double -- what ``coeff * x + (1.0 - coeff) * noise`` multiplies
    with.  A (B, 2) float32 tensor is taken as the pairs themselves."""
    if not isinstance(coeff, torch.Tensor):
        coeff = torch.as_tensor(coeff, dtype=torch.float64)
    coeff = coeff.detach()
    if coeff.dim() == 2:
        if coeff.shape[1] != 2 or coeff.dtype != torch.float32:
            raise ValueError(f"noise coefficients given as pairs must be a (B, 2) float32 tensor, got {tuple(coeff.shape)} {coeff.dtype}")
        return coeff
    if not coeff.dtype.is_floating_point:
        raise TypeError(f"noise coefficients must be floating point, got {coeff.dtype}")
    c = coeff.reshape(-1).double()
    return torch.stack((c, 1.0 - c), dim=1).to(torch.float32)


def snr_coefficients(snr_db) -> torch.Tensor:
    """AddRandomNoise's float64 coeff = r / (1 + r), r = exp(snr ln 10 / 10), for SNRs in dB."""
    import math
    snr = (snr_db if isinstance(snr_db, torch.Tensor) else torch.as_tensor(snr_db, dtype=torch.float64)).detach().double()
    r = torch.exp(snr * (math.log(10.0) / 10.0))
    return r / (1.0 + r)


def noise_plan(noise_store_len: int, noise_off, noise_len, noise_start, noise_pad_mode, coeff, size: int, B: int):
    """The noise group of ``assemble_clips`` checked like ``clip_plan`` checks the clips' (ValueError for what the host can see on
    the CPU; a device-side array is clamped by the kernel) -- except that ``noise_len`` 0 is the way to leave a clip unmixed.
    Returns (noise_off, noise_len, noise_start, noise_pad_mode, coeff (B, 2) float32)."""
    noise_len, noise_start = (t if isinstance(t, torch.Tensor) else torch.as_tensor(t) for t in (noise_len, noise_start))
    if noise_len.device.type == "cpu" and noise_start.device.type == "cpu" and noise_len.numel() == noise_start.numel():
        noise_start = torch.where(noise_len.reshape(-1) > 0, noise_start.reshape(-1), torch.zeros_like(noise_start.reshape(-1)))   # unmixed: no start to check
    nB, noise_off, noise_len, noise_start, noise_pad_mode, _, _ = clip_plan(noise_store_len, noise_off, noise_len, noise_start, noise_pad_mode, size)
    if nB != B:
        raise ValueError(f"the noise plan has {nB} entries, expected one per clip ({B})")
    coeff = noise_coefficients(coeff)
    if coeff.shape[0] != B:
        raise ValueError(f"the noise coefficients have {coeff.shape[0]} entries, expected one per clip ({B})")
    if coeff.device.type == "cpu" and B and not bool(((coeff >= 0) & (coeff <= 1)).all()):
        raise ValueError("a noise coefficient lies outside [0, 1]")
    return noise_off, noise_len, noise_start, noise_pad_mode, coeff


def _gaussian_plan(gaussian, B: int):
    amp, seed, stream = gaussian
    if not isinstance(amp, torch.Tensor):
        amp = torch.as_tensor(amp, dtype=torch.float32)
    amp = amp.detach().reshape(-1)
    if amp.numel() != B:
        raise ValueError(f"the Gaussian amplitudes have {amp.numel()} entries, expected one per clip ({B})")
    if amp.dtype != torch.float32:
        raise RuntimeError(f"the Gaussian amplitudes must be float32, got {amp.dtype}")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"the seed must fit 64 unsigned bits, got {seed}")
    return amp, seed, _plan_ints(stream, "stream", B)


def gaussian_noise(B: int, size: int, seed: int, stream, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The library's normal stream as a (B, size) float32 tensor (leaf_gaussian_noise_f32): ``out[b][t] = z(seed, stream[b], t)``, the
    values ``assemble_clips(..., gaussian=(amp, seed, stream))`` scales and adds -- Philox4x32-10 and Box-Muller as include/leaf_hip.h
    states them; a row depends on nothing but its stream id and the seed.  ``stream``: B int64 ids, on the device or the CPU."""
    B, size, seed = int(B), int(size), int(seed)
    if B < 0 or not 1 <= size < CALL_SAMPLES:
        raise ValueError(f"B must be >= 0 and size in [1, 2^31), got {B}, {size}")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"the seed must fit 64 unsigned bits, got {seed}")
    stream = _plan_ints(stream, "stream", B)
    if out is not None:
        dev = out.device
    elif device is not None:
        dev = torch.device(device)
    else:
        dev = stream.device if stream.device.type != "cpu" else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if out is not None:
        _check_out(out, (B, size), torch.float32, dev)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("gaussian_noise runs only on an AMD GPU (HIP device); there is no CPU fallback")
    if out is None:
        out = torch.empty((B, size), dtype=torch.float32, device=dev)
    if B:
        _call(dev, "leaf_gaussian_noise_f32", B, size, seed, stream.to(device=dev, dtype=torch.int64).contiguous(), out)
    return out


def _moments_group(standardize, B: int, store: torch.Tensor, who: str):
    """The standardisation group (moments (R, 4) float32 on the store's device, rec: one row of it per clip) checked as the host can
    see it: shapes and dtypes wherever the arrays live, the range of a ``rec`` that arrives on the CPU (ValueError)."""
    if len(standardize) != 2:
        raise ValueError(f"{who}: standardize must be (moments, rec)")
    moments, rec = standardize
    if not isinstance(moments, torch.Tensor) or moments.dim() != 2 or moments.shape[1] != 4 or moments.shape[0] < 1:
        raise ValueError(f"{who}: moments must be an (R, 4) tensor of at least one row (clip_moments)")
    if moments.dtype != torch.float32:
        raise TypeError(f"{who}: moments must be float32, got {moments.dtype}")
    if moments.device != store.device:
        raise ValueError(f"{who}: moments is on {moments.device}, the store on {store.device}")
    rec = _plan_ints(rec, "rec", B)
    if rec.device.type == "cpu" and B and (int(rec.min()) < 0 or int(rec.max()) >= moments.shape[0]):
        raise ValueError(f"rec holds an entry outside [0, {moments.shape[0]})")
    return moments.detach().contiguous(), rec


def assemble_clips(store: torch.Tensor, rec_off, rec_len, start, pad_mode, size: int, gain=None, normalize: bool = True, masks=None,
                   out: Optional[torch.Tensor] = None, noise=None, gaussian=None, standardize=None) -> torch.Tensor:
    """The batch (B, 1, size), float32, from a packed sample store in one launch (leaf_assemble_clips_f32, where the semantics are
    stated): per clip b the recording ``store[rec_off[b] : rec_off[b] + rec_len[b]]`` is padded to ``size`` if it is shorter
    (``pad_mode[b]``: PAD_ZERO / PAD_MIN / PAD_REPLICATE / PAD_WRAP, split left = padding // 2), cropped at ``start[b]``, multiplied by
    ``gain[b]``, peak-normalised (``normalize``: the bits of ``peak_normalize`` on the clip so far) and zeroed inside the ``masks``
    (B, M, 2) spans (t0, n).  ``store``: 1-D float32 or int16 PCM (a sample v means v / 32768) on a HIP device.  The plan arrays may
    live on either side: on the CPU they are validated (``clip_plan``) and copied over, on the device they are used as they are and
    clamped by the kernel.

    ``noise`` = (noise_store, noise_off, noise_len, noise_start, noise_pad_mode, coeff) mixes a background recording into every clip
    whose ``noise_len`` is above 0, in front of the gain: ``coeff * v + (1 - coeff) * n`` in AddRandomNoise's fp32 rounding, ``n`` the
    noise recording padded and cropped to ``size`` by its own plan (``noise_plan`` / ``noise_coefficients``; the store of the clips'
    dtype and device).  ``gaussian`` = (amp (B,) float32, seed, stream (B,) int64) adds ``amp[b] * z(seed, stream[b], t)`` behind the
    gain (``gaussian_noise`` returns z); amplitude 0 leaves a clip alone.  Either makes the call leaf_assemble_clips_noise_f32 -- still
    one launch; with neither the call is the one it always was.

    ``standardize`` = (moments (R, 4) float32 from ``clip_moments``, rec: clip b's row of it) puts the reference's waveform
    standardisation (RawAudioParser, ``audio_config.normalize``) in front of everything: every sample of the clip's recording becomes
    ``(v - mean) / (std + 1e-9)`` in torch's float32 rounding, the 'min' padding is the standardised recording's minimum, the noise
    recording stays as it is (leaf_assemble_clips_std_f32, one launch).  None: the call is the one above."""
    if not isinstance(store, torch.Tensor) or store.dim() != 1 or store.dtype not in (torch.float32, torch.int16):
        raise RuntimeError("assemble_clips: store must be a 1-D float32 or int16 tensor")
    size = int(size)
    B, rec_off, rec_len, start, pad_mode, gain, masks = clip_plan(store.numel(), rec_off, rec_len, start, pad_mode, size, gain, masks)
    if noise is not None:
        nstore = noise[0]
        if not isinstance(nstore, torch.Tensor) or nstore.dim() != 1:
            raise TypeError("assemble_clips: the noise store must be a 1-D tensor")
        if nstore.dtype != store.dtype:
            raise TypeError(f"assemble_clips: the noise store is {nstore.dtype}, the clip store {store.dtype}: both int16 PCM or both float32")
        if nstore.device != store.device:
            raise ValueError(f"assemble_clips: the noise store is on {nstore.device}, the clip store on {store.device}")
        noise = (nstore,) + tuple(noise_plan(nstore.numel(), *noise[1:], size, B))
    if gaussian is not None:
        gaussian = _gaussian_plan(gaussian, B)
    if standardize is not None:
        standardize = _moments_group(standardize, B, store, "assemble_clips")
    require_hip(store, "assemble_clips")
    dev = store.device
    store = store.detach().contiguous()
    if out is not None:
        _check_out(out, (B, 1, size), torch.float32, dev)
    else:
        out = torch.empty((B, 1, size), dtype=torch.float32, device=dev)
    if B == 0:
        return out
    rec_off = rec_off.to(device=dev, dtype=torch.int64).contiguous()
    rec_len, start, pad_mode = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (rec_len, start, pad_mode))
    gain = None if gain is None else gain.to(device=dev).contiguous()
    masks = None if masks is None else masks.to(device=dev, dtype=torch.int32).contiguous()
    head = (store, store.numel(), FLAG_X_PCM16 if store.dtype == torch.int16 else 0, B, size,
            rec_off, rec_len, start, pad_mode, gain, int(bool(normalize)), masks, 0 if masks is None else masks.shape[1], out)
    if noise is None and gaussian is None and standardize is None:
        _call(dev, "leaf_assemble_clips_f32", *head)
        return out
    ngroup, ggroup = (None, 0, None, None, None, None, None), (None, 0, None)
    if noise is not None:
        nstore = noise[0].detach().contiguous()
        ngroup = (nstore, nstore.numel(), noise[1].to(device=dev, dtype=torch.int64).contiguous()) + tuple(
            t.to(device=dev, dtype=torch.int32).contiguous() for t in noise[2:5]) + (noise[5].to(device=dev).contiguous(),)
    if gaussian is not None:
        ggroup = (gaussian[0].to(device=dev).contiguous(), gaussian[1], gaussian[2].to(device=dev, dtype=torch.int64).contiguous())
    if standardize is None:
        _call(dev, "leaf_assemble_clips_noise_f32", *head, *ngroup, *ggroup)
        return out
    moments, rec = standardize
    _call(dev, "leaf_assemble_clips_std_f32", *head, *ngroup, *ggroup, moments, rec.to(device=dev, dtype=torch.int32).contiguous(), moments.shape[0])
    return out


DRAW_MAX_MASKS = 32             # csrc/leaf_clip_draws.hpp (kDrawMaxMasks)


def draw_clip_plan(B: int, size: int, train: bool, offsets: torch.Tensor, lengths: torch.Tensor, state: torch.Tensor, seed: int,
                   stream_base: int, consts: dict, out: dict, index: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None,
                   noise_offsets: Optional[torch.Tensor] = None, noise_lengths: Optional[torch.Tensor] = None, advance: bool = True) -> None:
    """One ``leaf_draw_clip_plan`` launch on the current stream: the plan of ``assemble_clips`` for ``B`` clips of ``size`` samples,
    drawn on the device into the tensors of ``out`` (include/leaf_hip.h states the draws bit for bit).  Everything is device memory
    the caller owns -- ``offsets`` int64 / ``lengths`` int32 of the clip store (and of the noise store), ``index`` (B,) int64 or
    ``order`` (N,) int64, ``state`` one int64 holding the step counter's 64 bits -- so nothing is copied to the device, nothing is
    read back and the call can be captured into a graph.  ``consts``: pad_modes (two of 0..3), wrap_pad_prob, gain_prob, gain_db,
    num_masks, time_perc, noise_prob, snr_range, gaussian_prob, gaussian_amplitude.  ``out``: rec_off, rec_len, start, pad_mode
    (required) and any of gain, masks (B, M, 2), rec, the noise group (noise_off, noise_len, noise_start, noise_pad_mode, coeff
    (B, 2)), the Gaussian group (gauss_amp, gauss_stream), index; an absent entry is not drawn."""
    dev = state.device
    require_hip(state, "draw_clip_plan")
    want = {"rec_off": (torch.int64, (B,)), "rec_len": (torch.int32, (B,)), "start": (torch.int32, (B,)), "pad_mode": (torch.int32, (B,)),
            "gain": (torch.float32, (B,)), "masks": (torch.int32, (B, int(consts["num_masks"]), 2)), "rec": (torch.int32, (B,)),
            "noise_off": (torch.int64, (B,)), "noise_len": (torch.int32, (B,)), "noise_start": (torch.int32, (B,)),
            "noise_pad_mode": (torch.int32, (B,)), "coeff": (torch.float32, (B, 2)), "gauss_amp": (torch.float32, (B,)),
            "gauss_stream": (torch.int64, (B,)), "index": (torch.int64, (B,))}
    unknown = set(out) - set(want)
    if unknown:
        raise ValueError(f"draw_clip_plan: unknown outputs {sorted(unknown)}")
    for name, t in out.items():
        if t is not None:
            _check_out(t, want[name][1], want[name][0], dev)
    ins = (("offsets", offsets, torch.int64), ("lengths", lengths, torch.int32), ("noise_offsets", noise_offsets, torch.int64),
           ("noise_lengths", noise_lengths, torch.int32), ("index", index, torch.int64), ("order", order, torch.int64), ("state", state, torch.int64))
    for name, t, dtype in ins:
        if t is not None and (t.dtype != dtype or t.device != dev or t.dim() != 1 or not t.is_contiguous()):
            raise RuntimeError(f"draw_clip_plan: {name} must be a contiguous 1-D {dtype} tensor on {dev}")
    if offsets.numel() != lengths.numel() or state.numel() != 1 or (index is not None and index.numel() != B):
        raise ValueError("draw_clip_plan: offsets and lengths name the same recordings, state is one counter, index has one entry per clip")
    if noise_offsets is not None and (noise_lengths is None or noise_offsets.numel() != noise_lengths.numel()):
        raise ValueError("draw_clip_plan: noise_offsets and noise_lengths name the same recordings")
    seed, stream_base = int(seed), int(stream_base)
    if not (0 <= seed < 2 ** 64 and 0 <= stream_base < 2 ** 64):
        raise ValueError("draw_clip_plan: seed and stream_base must fit 64 unsigned bits")
    M = int(consts["num_masks"])
    o = lambda name: out.get(name)
    _call(dev, "leaf_draw_clip_plan", int(B), int(size), int(bool(train)), offsets, lengths, offsets.numel(),
          noise_offsets, noise_lengths, 0 if noise_offsets is None else noise_offsets.numel(),
          index, order, 0 if order is None else order.numel(), state, int(bool(advance)), seed, stream_base,
          int(consts["pad_modes"][0]), int(consts["pad_modes"][1]), float(consts["wrap_pad_prob"]), float(consts["gain_prob"]),
          float(consts["gain_db"][0]), float(consts["gain_db"][1]), M, float(consts["time_perc"]), float(consts["noise_prob"]),
          float(consts["snr_range"][0]), float(consts["snr_range"][1]), float(consts["gaussian_prob"]),
          float(consts["gaussian_amplitude"][0]), float(consts["gaussian_amplitude"][1]),
          o("rec_off"), o("rec_len"), o("start"), o("pad_mode"), o("gain"), o("masks") if M > 0 else None, o("rec"),
          o("noise_off"), o("noise_len"), o("noise_start"), o("noise_pad_mode"), o("coeff"), o("gauss_amp"), o("gauss_stream"), o("index"))


MIX_MAX_BATCH = 4096            # csrc/leaf_mix_draws.hpp (kMixMaxBatch)


def mix_alpha(alpha) -> float:
    """``alpha`` of Beta(alpha, alpha) as the C ABI takes it: a finite double above 0, anything else is a ValueError."""
    alpha = float(alpha)
    if not (math.isfinite(alpha) and alpha > 0.0):
        raise ValueError(f"alpha must be finite and > 0, got {alpha}")
    return alpha


def draw_mixup(B: int, alpha: float, state: torch.Tensor, seed: int, stream_base: int, perm: torch.Tensor, lam: torch.Tensor,
               advance: bool = True) -> None:
    """One ``leaf_draw_mixup`` launch on the current stream: mixup's permutation (``perm``, (B,) int32) and Beta(alpha, alpha) weights
    (``lam``, (B,) float32) of the step that ``state`` (one int64 holding the counter's 64 bits) stands at, drawn on the device into
    the caller's tensors (include/leaf_hip.h states the draws).  Nothing is copied to the device and nothing is read back, so the call
    can be captured into a graph.  What the host can see is checked here: ``B`` in [1, 4096], ``alpha`` finite and > 0 (ValueError)."""
    dev = state.device
    require_hip(state, "draw_mixup")
    B = int(B)
    if not 1 <= B <= MIX_MAX_BATCH:
        raise ValueError(f"draw_mixup: B must be in [1, {MIX_MAX_BATCH}], got {B}")
    alpha = mix_alpha(alpha)
    _check_out(perm, (B,), torch.int32, dev)
    _check_out(lam, (B,), torch.float32, dev)
    if state.dtype != torch.int64 or state.numel() != 1 or not state.is_contiguous():
        raise RuntimeError(f"draw_mixup: state must be one int64 on {dev}")
    seed, stream_base = int(seed), int(stream_base)
    if not (0 <= seed < 2 ** 64 and 0 <= stream_base < 2 ** 64):
        raise ValueError("draw_mixup: seed and stream_base must fit 64 unsigned bits")
    _call(dev, "leaf_draw_mixup", B, alpha, state, int(bool(advance)), seed, stream_base, perm, lam)


def _recordings(store: torch.Tensor, rec_off, rec_len, who: str, size: int = 1):
    """``store`` and the two arrays that name recordings in it, checked as ``clip_plan`` checks them: (B, rec_off, rec_len)."""
    if not isinstance(store, torch.Tensor) or store.dim() != 1 or store.dtype not in (torch.float32, torch.int16):
        raise RuntimeError(f"{who}: store must be a 1-D float32 or int16 tensor")
    if not isinstance(rec_off, torch.Tensor):
        rec_off = torch.as_tensor(rec_off)
    zeros = torch.zeros(rec_off.numel(), dtype=torch.int64)
    B, rec_off, rec_len, _, _, _, _ = clip_plan(store.numel(), rec_off, rec_len, zeros, zeros, size)
    return B, rec_off, rec_len


def clip_peaks(store: torch.Tensor, rec_off, rec_len) -> torch.Tensor:
    """``max |r_i|`` of every recording ``store[rec_off[i] : rec_off[i] + rec_len[i]]`` as an (R,) float32 tensor on the store's device
    (leaf_clip_peaks_f32): exact; 0 for a recording of no samples; NaN samples are ignored; an int16 store (v / 32768) has no peak
    above 1.  One call for all recordings, split by tiles of samples and not by recording.  The two arrays are validated on the CPU
    and clamped by the kernel on the device, as the plan of ``assemble_clips``."""
    R, rec_off, rec_len = _recordings(store, rec_off, rec_len, "clip_peaks")
    require_hip(store, "clip_peaks")
    dev = store.device
    peaks = torch.empty(R, dtype=torch.float32, device=dev)
    if R:
        _call(dev, "leaf_clip_peaks_f32", store.detach().contiguous(), store.numel(), FLAG_X_PCM16 if store.dtype == torch.int16 else 0, R,
              rec_off.to(device=dev, dtype=torch.int64).contiguous(), rec_len.to(device=dev, dtype=torch.int32).contiguous(), peaks,
              ws=lambda lib: lib.leaf_clip_peaks_workspace_bytes(R))
    return peaks


def clip_moments(store: torch.Tensor, rec_off, rec_len) -> torch.Tensor:
    """(mean, std, min, max) of every recording ``store[rec_off[i] : rec_off[i] + rec_len[i]]`` as an (R, 4) float32 tensor on the
    store's device (leaf_clip_moments_f32): the mean and torch's unbiased std accumulated in float64 (two passes: the deviations are
    taken from the float64 mean) and rounded once, min and max exact; an int16 sample v means v / 32768.  One sample gives std NaN, no
    samples (0, NaN, 0, 0), a NaN sample a NaN mean and std.  The order of the additions depends on a recording's length alone: the
    same bits on every call, whatever else the store holds.  The two arrays are validated on the CPU and clamped by the kernel on
    the device, as in ``clip_peaks``."""
    R, rec_off, rec_len = _recordings(store, rec_off, rec_len, "clip_moments")
    require_hip(store, "clip_moments")
    dev = store.device
    moments = torch.empty((R, 4), dtype=torch.float32, device=dev)
    if R:
        _call(dev, "leaf_clip_moments_f32", store.detach().contiguous(), store.numel(), FLAG_X_PCM16 if store.dtype == torch.int16 else 0, R,
              rec_off.to(device=dev, dtype=torch.int64).contiguous(), rec_len.to(device=dev, dtype=torch.int32).contiguous(), moments,
              ws=lambda lib: lib.leaf_clip_moments_workspace_bytes(R))
    return moments


def assemble_segments(store: torch.Tensor, rec_off, rec_len, win, size: int, peaks: Optional[torch.Tensor] = None, rec=None,
                      out: Optional[torch.Tensor] = None, moments: Optional[torch.Tensor] = None, normalize: bool = True) -> torch.Tensor:
    """Rows (rows, 1, size), float32, cut from whole recordings in one launch (leaf_assemble_segments_f32): row b is the window of
    ``size`` samples that starts at sample ``win[b]`` of the recording ``store[rec_off[b] : rec_off[b] + rec_len[b]]`` -- before it,
    inside it or behind it -- filled by replication outside the recording (F.pad 'replicate'); a recording of no samples gives zeros.
    With ``peaks`` ((R,) float32 on the store's device, ``clip_peaks``) and ``rec`` (the row's entry of it) a row is divided by its
    RECORDING's peak where that exceeds 1 -- ``peak_normalize`` on the whole recording, then the cut.  Arrays on the CPU are validated
    and copied over; on the device they are used as they are and clamped by the kernel.

    With ``moments`` ((R, 4) float32, ``clip_moments``; ``rec`` is then the row's entry of IT and ``peaks`` must be None) the rows are
    cut from the standardised recording ``(r - mean) / (std + 1e-9)`` (leaf_assemble_segments_std_f32), and ``normalize`` divides
    them by the standardised recording's peak where that exceeds 1 -- the peak follows from min and max, nothing else is launched.
    ``normalize`` is read only with ``moments``."""
    size = int(size)
    rows, rec_off, rec_len = _recordings(store, rec_off, rec_len, "assemble_segments", size)
    win = _plan_ints(win, "win", rows)                                          # (any start is a valid window)
    if moments is not None:
        if peaks is not None:
            raise ValueError("assemble_segments: peaks and moments exclude each other (the standardised recording's peak comes from moments)")
        if rec is None:
            raise ValueError("assemble_segments: moments needs rec, the entry of moments each row is standardised by")
        moments, rec = _moments_group((moments, rec), rows, store, "assemble_segments")
    if peaks is not None:
        if rec is None:
            raise ValueError("assemble_segments: peaks needs rec, the entry of peaks each row scales by")
        rec = _plan_ints(rec, "rec", rows)
        if peaks.dim() != 1 or peaks.numel() < 1:
            raise ValueError(f"peaks must be a 1-D tensor of at least one entry, got {tuple(peaks.shape)}")
        if rec.device.type == "cpu" and rows and (int(rec.min()) < 0 or int(rec.max()) >= peaks.numel()):
            raise ValueError(f"rec holds an entry outside [0, {peaks.numel()})")
    require_hip(store, "assemble_segments")
    dev = store.device
    if peaks is not None:
        peaks = _dev_f32(peaks, "peaks", dev)
    if out is not None:
        _check_out(out, (rows, 1, size), torch.float32, dev)
    else:
        out = torch.empty((rows, 1, size), dtype=torch.float32, device=dev)
    if rows == 0:
        return out
    if moments is not None:
        _call(dev, "leaf_assemble_segments_std_f32", store.detach().contiguous(), store.numel(), FLAG_X_PCM16 if store.dtype == torch.int16 else 0,
              rows, size, rec_off.to(device=dev, dtype=torch.int64).contiguous(), rec_len.to(device=dev, dtype=torch.int32).contiguous(),
              win.to(device=dev, dtype=torch.int64).contiguous(), None, rec.to(device=dev, dtype=torch.int32).contiguous(), moments.shape[0], out,
              moments, int(bool(normalize)))
        return out
    _call(dev, "leaf_assemble_segments_f32", store.detach().contiguous(), store.numel(), FLAG_X_PCM16 if store.dtype == torch.int16 else 0,
          rows, size, rec_off.to(device=dev, dtype=torch.int64).contiguous(), rec_len.to(device=dev, dtype=torch.int32).contiguous(),
          win.to(device=dev, dtype=torch.int64).contiguous(), _ptr(peaks),
          None if peaks is None else rec.to(device=dev, dtype=torch.int32).contiguous(), 0 if peaks is None else peaks.numel(), out)
    return out


RESAMPLE_TILE = 1024             # csrc/leaf_resample.hpp (kResampleTile): output samples per tile, one workgroup each
RESAMPLE_LDS_BUDGET = 64 * 1024  # ... (kResampleLdsBudget): bytes of LDS a workgroup may take for outputs, window and table
RESAMPLE_HEADER_INTS = 8         # ... (kResampleHeaderInts): magic, o, n, width, stride, taps_in_lds, 0, 0
_resample_tables: dict = {}


def _resample_params(orig_freq, new_freq, lowpass_filter_width, rolloff):
    """The four parameters as the C ABI takes them; ValueError for what it would answer with LEAF_ERR_BAD_SHAPE."""
    for name, v in (("orig_freq", orig_freq), ("new_freq", new_freq), ("lowpass_filter_width", lowpass_filter_width)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer, got {v!r}")
    orig_freq, new_freq, W, rolloff = int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff)
    if not (0 < orig_freq < 2 ** 31 and 0 < new_freq < 2 ** 31):
        raise ValueError(f"orig_freq and new_freq must be in [1, 2^31), got {orig_freq} and {new_freq}")
    if not 1 <= W < 2 ** 31:
        raise ValueError(f"lowpass_filter_width must be at least 1, got {W}")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"rolloff must be in (0, 1], got {rolloff}")
    return orig_freq, new_freq, W, rolloff


class ResampleTable:
    """The plan and the taps of one (orig_freq, new_freq, lowpass_filter_width, rolloff), on the CPU: ``o, n, width`` (the reduced
    ratio and the half width in input samples), ``k0`` / ``cnt`` (int32 (n,): every phase's span), ``taps`` (float32 (n, stride):
    row p holds the span's taps and zeros behind them), ``taps_in_lds`` / ``window_in_lds`` (the path the tiles take) and ``words``,
    the table as leaf_resample_table_f32 wrote it (int32).  ``on(device)`` is the device copy, uploaded on first use and kept.

    Tables and their device copies live as long as the process (``resample_table`` keeps one per key, this object one copy per
    device): a few hundred bytes to a few hundred KB for audio ratios, up to 64 MB at the library's limit.  That suits a handful
    of ratios; ``drop_resample_tables()`` releases them all."""

    def __init__(self, key, words: torch.Tensor):
        self.key, self.words = key, words
        _, self.o, self.n, self.width, self.stride, lds = (int(v) for v in words[:6])
        n, h = self.n, RESAMPLE_HEADER_INTS
        self.k0, self.cnt = words[h: h + n], words[h + n: h + 2 * n]
        self.taps = words[h + 2 * n:].view(torch.float32).reshape(n, self.stride)
        window = ((RESAMPLE_TILE - 1) // n + 2) * self.o + 2 * self.width
        self.window_in_lds = 4 * (window + RESAMPLE_TILE) <= RESAMPLE_LDS_BUDGET
        self.taps_in_lds = bool(lds)
        self._device = {}

    def on(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = self.words.to(device)
        return self._device[device]

    def with_global_taps(self) -> "ResampleTable":
        """The same table with ``taps_in_lds`` cleared: the tiles read their taps from global memory (the same bits; a test switch).
        The copy is the caller's: ``resample_table`` does not keep it."""
        words = self.words.clone()
        words[5] = 0
        return ResampleTable(self.key, words)


def drop_resample_tables() -> None:
    """Forget every kept table and its device copies; the next ``resample_table`` builds and uploads again."""
    with _lock:
        _resample_tables.clear()


def resample_table(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> ResampleTable:
    """The table of leaf_resample_f32 for these parameters (leaf_resample_table_f32: host only, evaluated in double and rounded once;
    no GPU is needed), kept per key.  ValueError for parameters outside the definition or beyond what the library takes (a reduced
    ratio above 65535, a table above 2^26 bytes)."""
    key = _resample_params(orig_freq, new_freq, lowpass_filter_width, rolloff)
    with _lock:
        table = _resample_tables.get(key)
    if table is None:
        lib = load()
        nbytes = lib.leaf_resample_table_bytes(*key)
        if nbytes == 0:
            raise ValueError(f"resampling {key[0]} -> {key[1]} (width {key[2]}, rolloff {key[3]}) is beyond the library: the reduced "
                             "ratio's terms stay at or below 65535 and the table below 2^26 bytes")
        words = torch.empty(nbytes // 4, dtype=torch.int32)
        check(lib.leaf_resample_table_f32(*key, ctypes.c_void_p(words.data_ptr()), nbytes), "leaf_resample_table_f32")
        table = ResampleTable(key, words)
        with _lock:
            table = _resample_tables.setdefault(key, table)
    return table


def resample_length(L: int, orig_freq: int, new_freq: int) -> int:
    """``ceil(L * n / o)`` for the reduced ratio (leaf_resample_length): the samples a recording of ``L`` samples becomes."""
    if int(orig_freq) <= 0 or int(new_freq) <= 0 or int(orig_freq) >= 2 ** 31 or int(new_freq) >= 2 ** 31:
        raise ValueError(f"orig_freq and new_freq must be in [1, 2^31), got {orig_freq} and {new_freq}")
    return int(load().leaf_resample_length(int(L), int(orig_freq), int(new_freq)))


def resample_records(store: torch.Tensor, in_off: torch.Tensor, in_len: torch.Tensor, orig_freq: int, new_freq: int, out: torch.Tensor,
                     out_off: torch.Tensor, lowpass_filter_width: int = 6, rolloff: float = 0.99, table: Optional[ResampleTable] = None,
                     ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """leaf_resample_f32 as it is: the recordings ``store[in_off[i] : in_off[i] + in_len[i]]`` (1-D float32 or int16 on the device;
    ``in_off`` int64 and ``in_len`` int32 on the device) resampled into ``out`` (1-D float32 or int16) from ``out_off[i]`` (int64 on
    the device) on, in one call.  The plan is used unseen: the kernel clamps it.  ``table``: another table of the same parameters
    (``ResampleTable.with_global_taps``); ``ws``: a workspace of the caller's (uint8, at
    least the size query)."""
    require_hip(store, "resample_records")
    dev = store.device
    if store.dim() != 1 or store.dtype not in (torch.float32, torch.int16) or not store.is_contiguous():
        raise TypeError("store must be a contiguous 1-D float32 or int16 tensor")
    if out.dim() != 1 or out.dtype not in (torch.float32, torch.int16) or not out.is_contiguous() or out.device != dev:
        raise TypeError("out must be a contiguous 1-D float32 or int16 tensor on the store's device")
    R = in_off.numel()
    for name, t, dt in (("in_off", in_off, torch.int64), ("in_len", in_len, torch.int32), ("out_off", out_off, torch.int64)):
        if t.dtype != dt or t.device != dev or t.numel() != R or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dt} tensor of {R} entries on {dev}")
    key = _resample_params(orig_freq, new_freq, lowpass_filter_width, rolloff)
    table = resample_table(*key) if table is None else table
    if table.key != key:
        raise ValueError(f"the table was built for {table.key}, the call is {key}")
    if R == 0:
        return out
    words = table.on(dev)
    flags = (FLAG_X_PCM16 if store.dtype == torch.int16 else 0) | (FLAG_OUT_PCM16 if out.dtype == torch.int16 else 0)
    args = (store, store.numel(), flags, R, in_off, in_len, *key, words, words.numel() * 4, out, out.numel(), out_off)
    if ws is None:
        _call(dev, "leaf_resample_f32", *args, ws=lambda lib: lib.leaf_resample_workspace_bytes(R))
    else:
        _call(dev, "leaf_resample_f32", *args, ws, ws.numel())
    return out


RESAMPLE_STREAM_MAX_CHUNK = 1 << 20   # csrc/leaf_resample_stream.hpp (kResampleStreamMaxChunk): samples one slot takes in one step


class ResampleSlot(ctypes.Structure):
    """leaf_resample_slot (include/leaf_hip.h): one slot of a chunked resampler in one step."""
    _fields_ = [(name, ctypes.c_int) for name in ("idle", "hist_len", "Tc", "parity", "shift", "phase", "n", "drop_samples", "end")]


class ResamplePos(ctypes.Structure):
    """leaf_resample_pos (include/leaf_hip.h): where one slot's stream stands between two steps."""
    _fields_ = [(name, ctypes.c_int) for name in ("running", "hist_len", "shift", "phase", "parity")]


def resample_stream_history(key) -> int:
    """H = K - 1 of the four parameters ``key`` (leaf_resample_stream_history_samples); 0 for what the step refuses."""
    return int(load().leaf_resample_stream_history_samples(*key))


def resample_stream_state(B: int, key, flags: int, device: torch.device) -> torch.Tensor:
    """The device-resident state of ``B`` chunked resamplers (leaf_resample_stream_state_bytes: two history halves), uninitialised --
    a stream's first step reads none of it."""
    nbytes = load().leaf_resample_stream_state_bytes(B, *key, flags)
    if nbytes == 0:
        raise RuntimeError(f"leaf_resample_stream_state_bytes: no chunked resampler for {key[0]} -> {key[1]}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def resample_stream_plan(key, pos, lengths, end):
    """leaf_resample_stream_plan: the host side of a step.  ``pos``: a ctypes array of ``ResamplePos``, advanced in place (all slots
    or none); ``lengths`` / ``end``: host integers per slot.  Returns (the slots' ``ResampleSlot`` records, the counts as a list);
    ValueError for what the entry refuses."""
    B = len(pos)
    Tc = (ctypes.c_int * B)(*lengths)
    ends = (ctypes.c_int * B)(*[int(bool(v)) for v in end])
    slots, counts = (ResampleSlot * B)(), (ctypes.c_int * B)()
    vp = ctypes.c_void_p
    rc = load().leaf_resample_stream_plan(B, *key, ctypes.cast(pos, vp), ctypes.cast(Tc, vp), ctypes.cast(ends, vp), ctypes.cast(slots, vp),
                                          ctypes.cast(counts, vp))
    if rc != 0:
        raise ValueError(f"leaf_resample_stream_plan refused the step: {load().leaf_status_string(rc).decode()} (status {rc})")
    return slots, list(counts)


def resample_stream_step(chunk_ptr: int, chunk_stride: int, slots, n_max: int, state: torch.Tensor, flags: int, key, table: ResampleTable,
                         out_ptr: int, device: torch.device) -> None:
    """leaf_resample_stream_step_f32 on the current stream of ``device``.  ``slots``: a ctypes array of ``ResampleSlot`` (host memory,
    read before the call returns); ``chunk_ptr`` / ``out_ptr``: device addresses (0 where no slot has samples / n_max is 0)."""
    words = table.on(device)
    _call(device, "leaf_resample_stream_step_f32", ctypes.c_void_p(chunk_ptr), chunk_stride, len(slots), ctypes.cast(slots, ctypes.c_void_p),
          n_max, state, state.numel(), flags, *key, words, words.numel() * 4, ctypes.c_void_p(out_ptr))


REVERB_COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)   # csrc/leaf_clip_effects.hpp (kFxCombTuning): Freeverb at 44.1 kHz
REVERB_ALLPASS_TUNING = (225, 341, 441, 556)                              # ... (kFxAllpassTuning)
REVERB_LDS_BUDGET = 64 * 1024                                             # ... (kFxLdsBudget): bytes of LDS a workgroup may take


def reverb_lengths(sample_rate: int, room_scale=100):
    """``(comb, allpass)``: the eight comb and four all-pass delay lengths of leaf_clip_effects_f32 at ``sample_rate`` for
    ``room_scale`` percent, in double as include/leaf_hip.h states them (``room_scale=100`` gives the caps the kernel clamps a plan
    into).  A length below 1 is a ValueError."""
    sample_rate = int(sample_rate)
    if sample_rate < 1:
        raise ValueError(f"sample_rate must be at least 1, got {sample_rate}")
    r = sample_rate / 44100
    scale = float(room_scale) / 100 * 0.9 + 0.1
    comb = [int(scale * r * c + 0.5) if scale * r * c + 0.5 >= 1 else 0 for c in REVERB_COMB_TUNING]
    allpass = [int(r * a + 0.5) for a in REVERB_ALLPASS_TUNING]
    if min(comb + allpass) < 1:
        raise ValueError(f"sample_rate {sample_rate} with room_scale {room_scale} makes a delay line shorter than one sample")
    if max(comb + allpass) >= 1 << 24:
        raise ValueError(f"sample_rate {sample_rate} is beyond the reverb's delay lines")
    return comb, allpass


def _reverb_caps(sample_rate: int):
    """The caps and all-pass lengths of a call, refused (ValueError) where the entry would refuse the rate."""
    caps, allpass = reverb_lengths(sample_rate, 100)
    if 4 * (sum(caps) + sum(allpass) + allpass[0]) > REVERB_LDS_BUDGET:
        raise ValueError(f"sample_rate {sample_rate}: the reverb's delay lines do not fit a workgroup's LDS ({REVERB_LDS_BUDGET} bytes)")
    return caps, allpass


def _percentages(v, name: str):
    if isinstance(v, torch.Tensor):
        v = v.detach().reshape(-1).cpu().tolist()
    elif not isinstance(v, (list, tuple)):
        v = [v]
    out = [float(e) for e in v]
    if any(not (0.0 <= e <= 100.0) for e in out):
        raise ValueError(f"{name} is a percentage in [0, 100]")
    return out


def reverb_plan(reverberance, damping, room_scale, sample_rate: int):
    """The reverb plan of ``clip_effects`` from sox's parameters: ``(feedback (B,) float32, damp (B,) float32, comb (B, 8) int32)``,
    CPU tensors.  ``reverberance``, ``damping`` and ``room_scale`` are percentages in [0, 100], tensors or sequences of B entries (or
    single numbers); the arithmetic is host work in double, rounded once where float32 is stored (include/leaf_hip.h):
    ``feedback = 1 - exp((reverberance - b) / (a b))`` with ``a = -1 / ln 0.7``, ``b = 100 / (ln 0.02 a + 1)``;
    ``damp = damping / 100 * 0.3 + 0.2``; ``comb[i] = int(scale r C[i] + 0.5)``, ``scale = room_scale / 100 * 0.9 + 0.1``,
    ``r = sample_rate / 44100``.  A length below 1 is a ValueError."""
    rev, dmp, room = _percentages(reverberance, "reverberance"), _percentages(damping, "damping"), _percentages(room_scale, "room_scale")
    if not len(rev) == len(dmp) == len(room):
        raise ValueError(f"reverberance, damping and room_scale have {len(rev)}, {len(dmp)} and {len(room)} entries")
    a = -1 / math.log(1 - 0.3)
    b = 100 / (math.log(1 - 0.98) * a + 1)
    fb_of, comb_of = {}, {}
    for v in set(rev):
        fb_of[v] = 1 - math.exp((v - b) / (a * b))
    for v in set(room):
        comb_of[v] = reverb_lengths(sample_rate, v)[0]
    reverb_lengths(sample_rate, 100)                                            # (the all-pass lengths, also without a clip)
    feedback = torch.tensor([fb_of[v] for v in rev], dtype=torch.float64).to(torch.float32)
    damp = torch.tensor([v / 100 * 0.3 + 0.2 for v in dmp], dtype=torch.float64).to(torch.float32)
    comb = torch.tensor([comb_of[v] for v in room], dtype=torch.int32).reshape(len(room), 8)
    return feedback, damp, comb


def _effects_f32(t, name: str, B: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.float32)
    t = t.detach().reshape(-1)
    if t.numel() != B:
        raise ValueError(f"{name} has {t.numel()} entries, expected one per clip ({B})")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    return t


def clip_effects_plan(B: int, clip_factor=None, reverb=None, sample_rate: int = 16000):
    """The plan of ``clip_effects`` as flat tensors on the devices they arrived on: ``(clip_factor, feedback, damp, comb)``, None
    for a step nobody takes.  Shapes and dtypes are checked wherever the arrays live.  An array that arrives on the CPU is validated
    (ValueError, before anything is launched): ``clip_factor`` finite (negative: the clip skips ClipValue); ``comb`` rows either
    skipped (``comb[b][0] <= 0``) or with every length in [1, cap_i], the lengths at ``room_scale = 100``; ``feedback`` in [0, 1) and
    ``damp`` in [0, 1] for the rows that are not skipped (when ``comb`` is on the CPU too: all rows otherwise).  A device-side array
    is not read back and the kernel clamps its lengths.  With ``reverb``, a ``sample_rate`` whose lines are shorter than one sample or
    do not fit LDS is a ValueError."""
    if clip_factor is not None:
        clip_factor = _effects_f32(clip_factor, "clip_factor", B)
        if clip_factor.device.type == "cpu" and B and not bool(torch.isfinite(clip_factor).all()):
            raise ValueError("clip_factor holds a value that is not finite")
    if reverb is None:
        return clip_factor, None, None, None
    if len(reverb) != 3:
        raise ValueError("reverb must be (feedback, damp, comb)")
    caps, _ = _reverb_caps(sample_rate)
    feedback, damp = _effects_f32(reverb[0], "feedback", B), _effects_f32(reverb[1], "damp", B)
    comb = reverb[2] if isinstance(reverb[2], torch.Tensor) else torch.as_tensor(reverb[2], dtype=torch.int32)
    if comb.dtype.is_floating_point or comb.dtype.is_complex or comb.dtype == torch.bool:
        raise TypeError(f"comb must be an integer tensor, got {comb.dtype}")
    if tuple(comb.shape) != (B, 8):
        raise ValueError(f"comb has shape {tuple(comb.shape)}, expected ({B}, 8): eight delay lengths per clip")
    comb = comb.detach()
    live = None
    if comb.device.type == "cpu" and B:
        live = comb[:, 0] > 0
        rows = comb[live].long()
        if bool(((rows < 1) | (rows > torch.tensor(caps))).any()):
            raise ValueError(f"comb holds a delay length outside [1, cap] (the caps at {sample_rate} Hz: {caps})")
    for t, name, hi_ok in ((feedback, "feedback", False), (damp, "damp", True)):
        if t.device.type == "cpu" and B:
            v = t if live is None else t[live]
            if not bool(((v >= 0) & ((v <= 1) if hi_ok else (v < 1))).all()):
                raise ValueError(f"{name} holds a value outside [0, 1{']' if hi_ok else ')'}")
    return clip_factor, feedback, damp, comb


def clip_effects(x: torch.Tensor, clip_factor=None, reverb=None, sample_rate: int = 16000, wet: float = 0.015,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ClipValue and the sox-style reverb on a batch, one launch (leaf_clip_effects_f32, where both are stated bit for bit).  ``x``:
    contiguous float32 ``(B, 1, S)`` or ``(B, S)`` on a HIP device; the result has its shape (``out``, distinct from ``x``, is
    written when given).  ``clip_factor``: B float32 factors -- the clip is clamped into ``[min(x) * factor, max(x) * factor]``, a
    negative factor leaves it alone.  ``reverb`` = (feedback (B,) float32, damp (B,) float32, comb (B, 8) int32), what ``reverb_plan``
    returns; ``comb[b][0] <= 0`` leaves clip b alone.  The all-pass lengths follow from ``sample_rate``; ``wet`` scales the
    reverberated signal that is added to the dry one.  The plan arrays may live on either side: on the CPU they are validated
    (``clip_effects_plan``) and copied over, on the device they are used as they are and the kernel clamps the lengths -- nothing is
    read back, so the call captures into a graph.  Parity with sox itself is unpinned (sox is not in this image)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_contiguous() or not (
            x.dim() == 2 or (x.dim() == 3 and x.shape[1] == 1)):
        raise RuntimeError("clip_effects: x must be a contiguous float32 (B, 1, S) or (B, S) tensor")
    B, S = x.shape[0], x.shape[-1]
    if S < 1 or B * S >= CALL_SAMPLES:
        raise ValueError(f"clip_effects: S must be at least 1 and B * S below 2^31, got B = {B}, S = {S}")
    wet = float(wet)
    if not math.isfinite(wet):
        raise ValueError(f"wet must be finite, got {wet}")
    clip_factor, feedback, damp, comb = clip_effects_plan(B, clip_factor, reverb, sample_rate)
    require_hip(x, "clip_effects")
    dev = x.device
    x = x.detach()
    if out is not None:
        _check_out(out, tuple(x.shape), torch.float32, dev)
        lo, hi = out.data_ptr(), x.data_ptr()
        if lo < hi + 4 * B * S and hi < lo + 4 * B * S:
            raise ValueError("clip_effects: out must not overlap x")
    else:
        out = torch.empty_like(x)
    if B == 0:
        return out
    on = lambda t, dtype: None if t is None else t.to(device=dev, dtype=dtype).contiguous()
    _call(dev, "leaf_clip_effects_f32", x, out, B, S, on(clip_factor, torch.float32), on(feedback, torch.float32), on(damp, torch.float32),
          on(comb, torch.int32), int(sample_rate), wet)
    return out


def prepare_tables(kernel: torch.Tensor, pool_w: torch.Tensor, K: int, hop: int) -> Optional[torch.Tensor]:
    """Parameter-derived tables of the overlap-save path (filter spectra + pooling rows) for frozen-parameter inference;
    ``None`` when that path does not cover the geometry.  Wraps leaf_fft_prepare_tables_f32."""
    require_hip(kernel, "prepare_tables")
    dev = kernel.device
    kernel = _dev_f32(kernel, "kernel", dev)
    pw = _dev_f32(pool_w.reshape(-1), "pool_w", dev)
    F = kernel.shape[0]
    nbytes = load().leaf_fft_tables_bytes(F, K, hop)
    if nbytes == 0:
        return None
    tables = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call(dev, "leaf_fft_prepare_tables_f32", kernel, pw, F, K, hop, tables, nbytes)
    return tables


def leaf_forward_prepared(x: torch.Tensor, tables: torch.Tensor, pool_b, alpha, delta, root, ema_w, F: int, K: int, hop: int,
                          pcen: bool = True, log1p: bool = False, out: Optional[torch.Tensor] = None,
                          out_bf16: bool = False) -> torch.Tensor:
    """Forward with tables from ``prepare_tables`` (same outputs as ``leaf_forward``, without the table kernel).  ``out_bf16``:
    bfloat16 features from a float32 or int16 waveform (LEAF_FLAG_OUT_BF16)."""
    lib = load()
    x2, flags = _unpack_x(x, "leaf_forward_prepared")
    dev = x.device
    B, T = x2.shape
    prm, compression = _gather(dev, (None, None, pool_b, alpha, delta, root, ema_w), pcen, log1p)
    TP = lib.leaf_num_frames(T, K, hop)
    out_bf16, feat = _features(flags, out_bf16)
    if out is not None:
        _check_out(out, (B, F, TP), feat, dev)
    flags |= compression | (FLAG_OUT_BF16 if out_bf16 else 0)
    if out is None:
        out = torch.empty((B, F, TP), dtype=feat, device=dev)
    _call(dev, "leaf_forward_prepared_f32", x2, B, T, tables, tables.numel(), *prm[2:], F, K, hop, flags, out,
          ws=lambda lib: lib.leaf_workspace_bytes(B, T, F, K, hop, ALGO_FFT))
    return out
