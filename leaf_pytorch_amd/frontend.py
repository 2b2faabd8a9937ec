"""``Leaf`` -- the drop-in for ``leaf_pytorch.frontend.Leaf`` (reference leaf_pytorch/frontend.py:22-89).

Same constructor signature (order and defaults), same sub-module attribute names, same ``state_dict``
keys and shapes, same ``(B,1,T) -> (B,F,T')`` forward, same error conventions -- but ``forward`` is one
call into the fused HIP kernels for MI355X (include/leaf_hip.h: ``leaf_forward_f32``).  There is no
CPU / eager fallback: a non-HIP input raises.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _native, _ops
from .initializers import GaborInit
from .modules import GaborConv1d, GaussianLowPass, PCENLayer, _SquaredModulusFn


class SquaredModulus(nn.Module):
    """frontend.py:10-19 -- (B,2F,T) interleaved re/im -> (B,F,T) re^2+im^2 (stage kernel when used alone;
    differentiable like the reference's)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and x.requires_grad:
            return _SquaredModulusFn.apply(x)
        return _native.squared_modulus(x)


class _LeafFn(torch.autograd.Function):
    """The path without the dispatcher ops.  Forward = fused HIP path (leaf_forward_save_f32); backward = leaf_backward_f32 (recomputes
    on device), or leaf_backward_head_f32 where ``_ops.backward_route`` says the head is all that is asked for.  ``lead`` inputs stand
    in front of the seven parameters: x alone, or x, perm, lam for the mixed batch x * lam + x[perm] * (1 - lam)
    (leaf_forward_save_mix_f32 / leaf_backward_mix_f32: parameter gradients only)."""

    @staticmethod
    def forward(ctx, lead, *args):
        head, params, (K, hop, pcen, algo, log1p, out_bf16) = args[:lead], args[lead:lead + 7], args[lead + 7:]
        if algo & _native.OPT_PEAKNORM:
            # leaf_forward_save_f32 would hand the backward a pooled tensor of the NORMALISED clips next to the raw x
            raise RuntimeError("the folded PeakNormalization prologue is forward-only (no backward through it)")
        need = ctx.needs_input_grad[1:]                               # (behind `lead`)
        ctx.route = "full" if algo & _native.OPT_FULL_BACKWARD else _ops.backward_route(need[lead], need[lead + 1], need[0] or (lead == 3 and need[2]), False)
        algo &= ~_native.OPT_FULL_BACKWARD
        fwd = _native.leaf_forward if lead == 1 else _native.leaf_forward_mix
        out, raw = fwd(*head, *params, K, hop, pcen=pcen, log1p=log1p, algo=algo, save_raw=True, out_bf16=out_bf16)
        ctx.lead, ctx.geom = lead, (K, hop)
        if ctx.route == "head":
            # the gradients of the pooling bias and the PCEN vectors: nothing of the waveform side is saved
            ctx.how = dict(pcen=pcen, log1p=bool(log1p) and not pcen, out_bf16=out.dtype == torch.bfloat16)
            ctx.save_for_backward(params[2], raw, *(params[3:] if pcen else ()))
            return out
        ctx.how = dict(pcen=pcen, log1p=bool(log1p) and not pcen,
                       out_bf16=bool(out_bf16),                   # bfloat16 features: their gradient arrives in bfloat16 and goes straight in
                       full_transforms=bool(algo & _native.ALGO_FULL_TRANSFORMS),   # Leaf.full_transforms(): the backward keeps them too
                       strict_band_classes=bool(algo & _native.ALGO_STRICT_BAND_CLASSES))
        ctx.save_for_backward(*head, *params[:3], raw, *(params[3:] if pcen else ()))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable      # (gradients of gradients: the dispatcher-op path, _second_order.py; here they raise)
    def backward(ctx, grad_out):
        lead, saved = ctx.lead, ctx.saved_tensors
        if ctx.route == "head":
            pool_b, raw, *pc = saved
            gpb, *gpc = _native.leaf_backward_head(raw, grad_out, pool_b, *(pc or (None,) * 4), **ctx.how)
            return (None, *(None,) * (lead + 2), gpb, *gpc, *(None,) * 6)      # (one per input of forward)
        head, (kernel, pool_w, pool_b, raw), pc = saved[:lead], saved[lead:lead + 4], saved[lead + 4:] or (None,) * 4
        if lead == 1:
            *grads, gx = _native.leaf_backward(*head, kernel, pool_w, pool_b, *pc, *ctx.geom, grad_out, need_dx=ctx.needs_input_grad[1],
                                               pooled_raw=raw, **ctx.how)
            gx = None if gx is None else gx.reshape(head[0].shape)
        else:
            *grads, gx = _native.leaf_backward_mix(*head, kernel, pool_w, pool_b, *pc, *ctx.geom, grad_out, pooled_raw=raw, **ctx.how)
        return (None, gx, *(None,) * (lead - 1), *grads, *(None,) * 6)          # (one per input of forward)


class Leaf(nn.Module):
    def __init__(self, n_filters: int = 40, sample_rate: int = 16000, window_len: float = 25.,
                 window_stride: float = 10., preemp: bool = False, init_min_freq=60.0, init_max_freq=7800.0,
                 mean_var_norm: bool = False, pcen_compression: bool = True, use_legacy_complex=False,
                 initializer="default"):
        super().__init__()
        window_size = int(sample_rate * window_len // 1000 + 1)
        window_stride = int(sample_rate * window_stride // 1000)
        if preemp:
            raise NotImplementedError("Pre-emp functionality not implemented yet..")
        self._preemp = None
        if initializer == "default":
            initializer = GaborInit(default_window_len=window_size, sample_rate=sample_rate,
                                    min_freq=init_min_freq, max_freq=init_max_freq)
        self._complex_conv = GaborConv1d(filters=2 * n_filters, kernel_size=window_size, strides=1, padding="same",
                                         use_bias=False, initializer=initializer,
                                         use_legacy_complex=use_legacy_complex)
        self._activation = SquaredModulus()
        self._pooling = GaussianLowPass(n_filters, kernel_size=window_size, strides=window_stride, padding="same")
        self._instance_norm = None
        if mean_var_norm:
            raise NotImplementedError("Instance Norm functionality not added yet..")
        if pcen_compression:
            self._compression = PCENLayer(n_filters, alpha=0.96, smooth_coef=0.04, delta=2.0, floor=1e-12,
                                          trainable=True, learn_smooth_coef=True, per_channel_smooth_coef=True)
        else:
            self._compression = None
        self._maximum_val = torch.tensor(1e-5)
        self._algo = _native.ALGO_AUTO       # not part of the reference surface: kernel selector for tests/bench
        self._cache_tables = False           # not part of the reference surface: see cache_tables()
        self._tables = None
        self._tables_key = None
        self._fuse_peaknorm = False          # not part of the reference surface: see fuse_peak_normalization()
        self._log1p = False                  # not part of the reference surface: see log_compression()
        self._out_dtype = None               # not part of the reference surface: see output_dtype()
        self._full_backward = False          # not part of the reference surface: see full_backward()

    def full_transforms(self, enable: bool = True) -> "Leaf":
        """Not part of the reference surface: switch the band-limited filter tasks off for this module -- every filter on the
        full-length inverse transform in the forward (LEAF_ALGO_FULL_TRANSFORMS) AND in the backward the autograd path runs
        (LEAF_FLAG_BWD_FULL_TRANSFORMS).  The default (band tasks where a filter's spectrum allows) stays within ~1e-6 of the
        oracle in the forward and ~1e-5 of the full-transform gradients; this is the opt-out for a caller who wants the
        formulation without the approximation, at ~1.8x the time of the 16 kHz forward."""
        self._algo = (self._algo | _native.ALGO_FULL_TRANSFORMS) if enable else (self._algo & ~_native.ALGO_FULL_TRANSFORMS)
        return self

    def full_backward(self, enable: bool = True) -> "Leaf":
        """Not part of the reference surface: keep the full backward (leaf_backward_f32: every forward intermediate recomputed, all
        seven parameter gradients) also where the head-only backward would do.  By default a training forward whose Gabor kernel
        and pooling width are frozen (``requires_grad_(False)``) and whose input needs no gradient saves the pre-floor pooled
        tensor and the PCEN vectors alone -- no waveform -- and its backward is one launch over them (leaf_backward_head_f32) for
        the gradients of the pooling bias and the PCEN vectors.  This switch is what ``tools/bench_backward.py --frozen-filters``
        measures that route against; the gradients of the two routes agree to float32 rounding."""
        self._full_backward = bool(enable)
        return self

    def log_compression(self, enable: bool = True) -> "Leaf":
        """Not part of the reference surface: log compression in place of PCEN -- ``forward(x)`` returns
        ``log1p(max(pooled, 1e-5))`` (the LEAF paper's ablation without PCEN; LEAF_FLAG_LOG1P), computed where the fused
        kernels finalize a frame, and the backward applies ``1 / (1 + pooled)`` where it reads ``grad_out``: no extra pass over
        the features in either direction.  Needs ``pcen_compression=False`` (``ValueError`` otherwise).  Adds no parameter and
        no buffer: ``state_dict`` keys stay those of the reference, so its checkpoints still load strictly."""
        if enable and self._compression is not None:
            raise ValueError("log_compression() needs a Leaf built with pcen_compression=False (PCEN is the compression of this module)")
        self._log1p = bool(enable)
        return self

    def output_dtype(self, dtype=None) -> "Leaf":
        """Not part of the reference surface: the dtype of the features, independent of the waveform's.  ``None`` (the default):
        the features follow the waveform -- float32 for a float32 or int16 ``x``, bfloat16 for a bfloat16 ``x``.
        ``torch.bfloat16``: bfloat16 features from a float32 or int16 waveform (LEAF_FLAG_OUT_BF16) -- the kernels compute in float32
        as ever and round each feature to nearest even where they store it, so the result is ``forward(x).to(torch.bfloat16)`` of
        the float32 call bit for bit, without the float32 tensor and without the cast kernel; in training the bfloat16 gradient of
        the features is widened where the backward reads it, so the parameter gradients (and ``x.grad``, float32, for a float32
        ``x``) are those of the float32 call on that gradient widened.  ``"autocast"``: bfloat16 exactly when CUDA autocast is
        enabled with bfloat16 at the call (the model behind this module under ``torch.autocast("cuda", torch.bfloat16)``), else as
        ``None``.  ``torch.float32``: float32 features; with a bfloat16 waveform that combination is not built and the call raises
        ``ValueError``.  Anything else raises ``ValueError`` here -- ``torch.float16`` included: with the compression off the
        un-normalised pooled energies leave its range.

        Honoured by ``forward``, ``forward_mixup``, ``cache_tables()``, ``log_compression()``, ``full_transforms()``,
        ``fuse_peak_normalization()`` and training.  Adds no parameter and no buffer: ``state_dict`` keys stay those of the
        reference.  Gradients of gradients raise, as for bfloat16 I/O.  ``LeafStream`` does not look at this setting: a stream keeps
        returning float32 chunks (its smoother state is carried in float32 between calls)."""
        if not (dtype is None or dtype is torch.float32 or dtype is torch.bfloat16 or (isinstance(dtype, str) and dtype == "autocast")):
            raise ValueError(f"output_dtype: expected None, torch.float32, torch.bfloat16 or 'autocast', got {dtype!r} "
                             "(float16 is not offered: un-normalised pooled energies overflow it with the compression off)")
        self._out_dtype = dtype
        return self

    def _features_bf16(self, x: torch.Tensor) -> bool:
        """Whether this call asks the kernels for bfloat16 features (the explicit ``out_bf16`` of the host layers)."""
        mode = self._out_dtype
        if mode is None:
            return False
        if mode is torch.float32:
            if x.dtype == torch.bfloat16:
                raise ValueError("output_dtype(torch.float32) with a bfloat16 waveform is not built: the features of a bfloat16 x are bfloat16")
            return False
        if mode is torch.bfloat16:
            return True
        return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16

    def fuse_peak_normalization(self, enable: bool = True) -> "Leaf":
        """Not part of the reference surface: make ``forward(x)`` return ``Leaf(PeakNormalization(x))`` -- the last transform
        of every reference data pipeline (utilities/data/raw_transforms.py:334-345) folded into the frontend.  On the
        overlap-save paths under ``no_grad`` the normalised waveform is never written (one read-only pass finds each clip's
        scale s; s^2 multiplies the pooled energies where the bias is added: LEAF_FLAG_PEAKNORM); under autograd, or where
        another kernel family serves the geometry, the separate HIP normalisation kernel runs first.  Equal to the two-step
        form up to fp32 rounding."""
        self._fuse_peaknorm = bool(enable)
        return self

    def cache_tables(self, enable: bool = True) -> "Leaf":
        """Serving mode (not part of the reference surface): keep the tables derived from the filter / pooling parameters
        (filter spectra, pooling rows) across no-grad forwards instead of rebuilding them on every call, and rebuild them
        only when those parameters change (torch's per-tensor version counter and storage pointer are checked on every
        call, so optimizer steps, ``load_state_dict`` and ``.to()`` are picked up; writes that bypass the version counter
        are not).  Outputs are bit-identical to the default path."""
        self._cache_tables = bool(enable)
        self._tables = self._tables_key = None
        return self

    def _prepared_tables(self):
        k, w = self._complex_conv._kernel, self._pooling.weights
        key = (k.data_ptr(), k._version, w.data_ptr(), w._version, k.device)
        if self._tables is None or key != self._tables_key:
            self._tables = _native.prepare_tables(k.detach(), w.detach(), self._complex_conv._kernel_size, self._pooling.strides)
            self._tables_key = key if self._tables is not None else None
        return self._tables

    def _kernel_params(self):
        """The seven parameter tensors in the order every host layer takes them (the PCEN four None without PCEN)."""
        c = self._compression
        pcen = (None,) * 4 if c is None else (c.alpha, c.delta, c.root, c.ema._weights)
        return (self._complex_conv._kernel, self._pooling.weights, self._pooling._bias, *pcen)

    def forward_mixup(self, x: torch.Tensor, perm, lam) -> torch.Tensor:
        """Not part of the reference surface: ``forward(x * lam[:, None, None] + x[perm] * (1 - lam[:, None, None]))`` -- the
        waveform mixup of the reference's training loop (utilities/data/mixup.py) -- bit for bit, with the mix done in fp32 inside
        the kernels' loads, forward and backward, on the static geometries (16 / 8 / 32 kHz windows) and the 4096-sample plans: there the
        mixed batch is never written and an int16 batch stays int16 in memory through a training step.  On every other geometry and
        selector (run-time-geometry windows on 2048-sample blocks, MFMA, staged) the forward and the backward each write the mixed
        float32 batch into their workspace first and run on that; the result is the same bits.

        ``x``: (B,1,T) float32 or int16 PCM on the device; a bfloat16 ``x`` raises, and so does ``x.requires_grad`` (the gradient
        would be a scatter over ``perm``; ``x`` is data here).  ``perm``: any integer tensor or sequence of length B, converted to
        int32 on the device; when it arrives on the CPU it is validated there and an index outside [0, B) raises ValueError
        before anything is launched (on the device it is clamped by the kernels).  ``lam``: float32, length B.  The parameters
        train through the call; ``create_graph=True`` is not supported.  ``log_compression()``, ``full_transforms()`` and
        ``pcen_compression=False`` apply as on ``forward``; ``fuse_peak_normalization()`` is NOT applied on this call (the
        normalisation would have to follow the mix; peak-normalised clips stay inside |x| <= 1 under a convex mix), nor is
        ``cache_tables()``.  ``transforms.Mixup`` draws ``perm`` and ``lam`` and mixes the targets."""
        _native.require_hip(x, "Leaf.forward_mixup")
        if x.dim() != 3 or x.shape[1] != 1:
            raise RuntimeError(f"expected input of shape (B,1,T), got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.int16):
            raise RuntimeError(f"Leaf.forward_mixup: the mix is defined in float32 on a float32 or int16 (PCM) waveform, got {x.dtype}")
        if x.requires_grad:
            raise RuntimeError("Leaf.forward_mixup: x.requires_grad is not supported (dL/dx under mixup is a scatter over perm, "
                               "and the waveform is data here)")
        c = self._compression
        if c is not None and c._floor != 1e-12:
            raise NotImplementedError("fused path is specialised for the PCEN floor Leaf constructs (1e-12)")
        perm, lam = _native.mix_args(perm, lam, x.shape[0], x.device)
        params = self._kernel_params()
        K, hop = self._complex_conv._kernel_size, self._pooling.strides
        log1p = self._log1p and c is None
        bf16 = self._features_bf16(x)                             # output_dtype(): bfloat16 features of the mixed batch
        needs_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in params)
        train_algo = self._algo | (_native.OPT_FULL_BACKWARD if self._full_backward else 0)
        if _ops.available():
            _ops.load()
            if needs_grad:
                return _ops.forward_train_mix(x, perm, lam, *params, K, hop, algo=train_algo, log1p=log1p, out_bf16=bf16)
            return _ops.forward_mix(x, perm, lam, *params, K, hop, log1p=log1p, algo=self._algo, out_bf16=bf16)
        if needs_grad:
            return _LeafFn.apply(3, x, perm, lam, *params, K, hop, c is not None, train_algo, log1p, bf16)
        return _native.leaf_forward_mix(x, perm, lam, *params, K, hop, pcen=c is not None, log1p=log1p, algo=self._algo, out_bf16=bf16)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B,1,T) float32 -> (B,F,T') float32, as the reference.  Not part of the reference surface: a bfloat16 ``x`` gives
        bfloat16 features, and an int16 ``x`` is 16-bit PCM -- a sample v means v / 32768, converted inside the kernels' loads --
        and gives the float32 features of ``x.float() / 32768`` bit for bit, on every path (inference, ``cache_tables()``,
        training of the parameters, ``log_compression()``, ``full_transforms()``); it has no gradient of its own.
        ``output_dtype()`` chooses the dtype of the features independently of the waveform's."""
        _native.require_hip(x, "Leaf.forward")
        bf16 = self._features_bf16(x)                             # output_dtype(): bfloat16 features from a float32 / int16 waveform
        algo = self._algo
        c = self._compression
        params = self._kernel_params()
        K, hop, F = self._complex_conv._kernel_size, self._pooling.strides, self._complex_conv._filters
        # from the tensors actually handed to the kernel, not self.parameters(): nn.DataParallel replicas hold plain
        # (non-leaf) tensors, for which parameters() is empty
        params_need_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in params)
        train_full = self._full_backward
        # an int16 waveform (16-bit PCM: a sample v means v / 32768) lies in [-1, 1) by construction: nothing to normalise
        if self._fuse_peaknorm and x.dtype != torch.int16:
            # the folded prologue is forward-only: the same condition that sends the call to the training path below
            fused_ok = (not (params_need_grad or (torch.is_grad_enabled() and x.requires_grad))
                        and not self._cache_tables and x.dim() == 3 and x.shape[1] == 1 and x.shape[0] > 0)
            if fused_ok:
                with torch.cuda.device(x.device):
                    sel = algo & 0xff
                    if sel == _native.ALGO_AUTO:
                        sel = _native.load().leaf_auto_algo(x.shape[0], x.shape[-1], F, K, hop)
                fused_ok = sel in (_native.ALGO_FFT, _native.ALGO_FFT_WG, _native.ALGO_FFT_SMALL)
            if fused_ok:
                algo = algo | _native.OPT_PEAKNORM
            else:
                from .transforms import PeakNormalization
                x = PeakNormalization()(x)
                train_full = True                                 # (under autograd: the backward stays the full one, as before)
        if c is not None and c._floor != 1e-12:
            raise NotImplementedError("fused path is specialised for the PCEN floor Leaf constructs (1e-12)")
        pcen = c is not None
        log1p = self._log1p and not pcen
        needs_grad = params_need_grad or (torch.is_grad_enabled() and x.requires_grad)
        if needs_grad and (algo & _native.OPT_PEAKNORM):
            raise RuntimeError("Leaf.forward: the folded PeakNormalization prologue is forward-only")   # unreachable by design
        if _ops.available():
            # dispatcher ops (csrc/torch_binding.cpp): traceable by torch.compile / export, one hop per eager call
            _ops.load()
            if needs_grad:
                return _ops.forward_train(x, *params, K, hop, algo=algo | (_native.OPT_FULL_BACKWARD if train_full else 0), log1p=log1p,
                                          out_bf16=bf16)
            if not (self._cache_tables and not torch.compiler.is_compiling()):
                return _ops.forward(x, *params, K, hop, log1p=log1p, algo=algo, out_bf16=bf16)
        if needs_grad:
            return _LeafFn.apply(1, x, *params, K, hop, pcen, algo | (_native.OPT_FULL_BACKWARD if train_full else 0), log1p, bf16)
        if self._cache_tables and self._algo in (_native.ALGO_AUTO, _native.ALGO_FFT):
            B, T = x.shape[0], x.shape[-1]
            with torch.cuda.device(x.device):            # the plan is sized for the CU count of the device the call runs on
                plan = _native.fft_plan_info(B, T, F, K, hop)
                auto = _native.load().leaf_auto_algo(B, T, F, K, hop)
            # the prepared tables are those of the 2048-sample plan: used only where that is what the default path runs, so
            # that serving mode stays bit-identical to it (long windows on 4096-sample blocks rebuild their tables per call)
            if auto in (_native.ALGO_FFT, _native.ALGO_FFT_WG) and plan is not None and plan["fft_n"] == 2048:
                tables = self._prepared_tables()
                if tables is not None:
                    return _native.leaf_forward_prepared(x, tables, *params[2:], F, K, hop, pcen=pcen, log1p=log1p, out_bf16=bf16)
        return _native.leaf_forward(x, *params, K, hop, pcen=pcen, log1p=log1p, algo=algo & ~_native.OPT_PEAKNORM,
                                    peak_normalize=bool(algo & _native.OPT_PEAKNORM), out_bf16=bf16)
