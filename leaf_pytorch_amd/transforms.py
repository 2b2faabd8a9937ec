"""On-device counterparts of the reference's waveform transforms that sit directly in front of the frontend
(utilities/data/raw_transforms.py): the crops are views, PeakNormalization is a HIP kernel.  They take batched device
tensors ``(B, T)`` or ``(B, 1, T)`` (the reference versions run per clip on the CPU inside DataLoader workers)."""
import random

import torch

from . import _native


class RandomCrop:
    """raw_transforms.py:121-127 -- a random window of ``size`` samples (one offset per call, shared by the batch)."""

    def __init__(self, size: int):
        self.size = size

    def __call__(self, signal: torch.Tensor) -> torch.Tensor:
        start = random.randint(0, signal.shape[-1] - self.size)
        return signal[..., start: start + self.size]


class CenterCrop:
    """raw_transforms.py:130-140 -- the central ``size`` samples; shorter inputs pass unchanged."""

    def __init__(self, size: int):
        self.size = size

    def __call__(self, signal: torch.Tensor) -> torch.Tensor:
        if signal.shape[-1] > self.size:
            start = (signal.shape[-1] - self.size) // 2
            return signal[..., start: start + self.size]
        return signal


class PeakNormalization:
    """raw_transforms.py:334-345 -- ``torch_audiomentations.PeakNormalization(apply_to="only_too_loud_sounds", p=1)``:
    every clip whose peak |x| exceeds 1 is divided by its peak, quieter clips are returned unchanged.  (The third-party
    package is not in this image: its documented behaviour is restated, parity unpinned.)"""

    def __init__(self, sr: int = 16000):
        self.sr = sr                      # kept for signature compatibility; the operation does not depend on it

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return _native.peak_normalize(x)


class Mixup:
    """utilities/data/mixup.py:5-26 (``do_mixup``) restated for a batch on the device, with the mix itself done by a HIP kernel
    (``_native.mixup``: fp32 or int16 PCM in, fp32 out, bit for bit the reference's ``inputs * lam + inputs[perms] * (1 - lam)``).
    One weight per clip from Beta(alpha, alpha) -- drawn from ``numpy.random.RandomState(random_seed)`` as the reference does, so a
    fixed seed gives the reference's weights -- and one permutation of the batch from torch's generator.

    ``__call__(inputs, targets)`` returns ``(mixed_x, a, b, lam_or_None, perm, lam)``: the reference's four values -- multilabel:
    ``(mixed_x, mixed_y, None, None)``, any other mode: ``(mixed_x, y_a, y_b, lam)`` -- followed by the permutation and the weights,
    so that a caller can hand ``(inputs, perm, lam)`` to ``Leaf.forward_mixup`` instead of the mixed batch.  ``mix_inputs=False``
    skips the waveform kernel for exactly that use (``mixed_x`` is then None).  The targets are mixed with stock ops."""

    def __init__(self, alpha: float = 1., random_seed=1233, mode: str = "multilabel", mix_inputs: bool = True):
        self.alpha = alpha
        self.random_seed = random_seed
        self.mode = mode
        self.mix_inputs = mix_inputs

    def __call__(self, inputs: torch.Tensor, targets: torch.Tensor):
        import numpy as np
        random_state = np.random.RandomState(self.random_seed)      # (re-seeded per call, as the reference's do_mixup)
        bsize = len(inputs)
        lam = torch.from_numpy(random_state.beta(self.alpha, self.alpha, bsize)).to(inputs.device).float()
        perms = torch.randperm(bsize).to(inputs.device)
        mixed_x = _native.mixup(inputs, perms, lam) if self.mix_inputs else None
        if self.mode == "multilabel":
            mixed_y = targets * lam.view(bsize, 1) + targets[perms] * (1 - lam.view(bsize, 1))
            return mixed_x, mixed_y, None, None, perms, lam
        return mixed_x, targets, targets[perms], lam, perms, lam


class PackedClips:
    """A dataset resident on the device: 1-D recordings of any lengths, all int16 PCM or all float32, concatenated once into
    ``store`` (``offsets`` int64 and ``lengths`` int32 beside it, mirrored on the host as ``offsets_host`` / ``lengths_host``), and
    the batches made from it by ONE kernel launch (``_native.assemble_clips`` -> leaf_assemble_clips_f32): per clip the reference's
    PadToSize, RandomCrop / CenterCrop, RandomGain, PeakNormalization and TimeMasking (utilities/data/raw_transforms.py), which
    run per clip on the CPU there.  The draws are the caller's (``ClipSampler`` makes them as the reference pipelines do); this class
    applies them.  The result is the float32 ``(B, 1, size)`` batch ``Leaf.forward`` and ``Leaf.forward_mixup`` take.

    The two noise transforms ride in the same launch (``assemble(..., noise=..., gaussian=...)`` -> leaf_assemble_clips_noise_f32):
    AddRandomNoise, a background recording from a second ``PackedClips`` mixed in at an SNR in front of the gain, and
    AddGaussianNoise, the library's own counter-based normal stream (``_native.gaussian_noise``) scaled and added behind it -- both
    in front of the peak normalisation, as in the reference's pipelines.

    Evaluation as the reference's test.py does it -- whole recordings, one peak per recording, cut into rows -- is ``segments``
    (leaf_assemble_segments_f32) with ``peaks`` (leaf_clip_peaks_f32) behind it; ``segment_mean`` and ``evaluate_recordings`` finish
    the loop.

    The reference's waveform standardisation (RawAudioParser with ``audio_config.normalize``: the WHOLE recording, as loaded and in
    front of every other transform, becomes ``(r - mean) / (std + 1e-9)``) is the keyword ``standardize`` of ``assemble`` and
    ``segments``: the recordings' ``moments()`` (leaf_clip_moments_f32, once per dataset) are looked up by the kernel and the map is
    applied as the samples are loaded (leaf_assemble_clips_std_f32 / leaf_assemble_segments_std_f32) -- still one launch per batch,
    the int16 store stays int16.

    One workgroup assembles one clip: a batch of a few very long clips uses a few CUs (splitting a clip over workgroups is not
    built; the rows of ``segments`` are split).  Not built either: bfloat16 stores, outputs in anything but float32, a noise store
    of another dtype than the clips', a standardised noise store (the reference does not standardise its noise either), and the
    statistics of the reference's ``--cropped_read`` (there the parser sees only the frames that were read, tiled by ``load_audio``:
    another padding convention)."""

    def __init__(self, recordings, device=None):
        recs = [r if isinstance(r, torch.Tensor) else torch.as_tensor(r) for r in recordings]
        if not recs:
            raise ValueError("PackedClips needs at least one recording")
        if any(r.dim() != 1 for r in recs):
            raise ValueError("every recording must be 1-D (one channel)")
        if any(r.dtype != recs[0].dtype for r in recs) or recs[0].dtype not in (torch.int16, torch.float32):
            raise TypeError("the recordings must be all int16 (PCM) or all float32")
        lengths = torch.tensor([r.numel() for r in recs], dtype=torch.int64)
        store = torch.cat([r.detach() for r in recs])
        self._set(store if device is None else store.to(device), torch.cumsum(lengths, 0) - lengths, lengths)

    @classmethod
    def from_store(cls, store: torch.Tensor, offsets, lengths) -> "PackedClips":
        """A store that is packed already (``packed_dataset.py``'s layout): recording i is ``store[offsets[i] : offsets[i] + lengths[i]]``."""
        self = cls.__new__(cls)
        offsets, lengths = (torch.as_tensor(t).detach().reshape(-1).cpu().long() for t in (offsets, lengths))
        if store.dim() != 1 or store.dtype not in (torch.int16, torch.float32):
            raise TypeError("store must be a 1-D int16 (PCM) or float32 tensor")
        if offsets.numel() != lengths.numel():
            raise ValueError(f"{offsets.numel()} offsets for {lengths.numel()} lengths")
        if offsets.numel() and (int(offsets.min()) < 0 or int(lengths.min()) < 0 or int(lengths.max()) >= 2 ** 31
                                or int((offsets + lengths).max()) > store.numel()):
            raise ValueError(f"a recording lies outside the store ({store.numel()} samples)")
        self._set(store.detach(), offsets, lengths)
        return self

    def _set(self, store, offsets, lengths):
        self.store = store.contiguous()
        self.offsets_host, self.lengths_host = offsets.to(torch.int64), lengths.to(torch.int32)
        self.offsets, self.lengths = self.offsets_host.to(store.device), self.lengths_host.to(store.device)
        self._peaks = None                                                      # peaks(): computed on the first call, then kept
        self._moments = None                                                    # ... and moments()

    def __len__(self) -> int:
        return self.lengths_host.numel()

    def _per_clip(self, v, B: int, names=None):
        """A per-clip plan entry given as one value for the batch, or as a sequence / tensor of B of them."""
        if isinstance(v, str):
            v = names[v]
        elif names is not None and not isinstance(v, torch.Tensor) and not isinstance(v, int):
            v = [names[m] if isinstance(m, str) else int(m) for m in v]
        t = v if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=torch.int64)
        return t.reshape(1).expand(B) if t.dim() == 0 else t

    def _records(self, index, what: str = "index"):
        """(B, rec_off, rec_len) of the recordings ``index`` on the side the index lives on (validated on the CPU)."""
        index = (index if isinstance(index, torch.Tensor) else torch.as_tensor(index, dtype=torch.int64)).reshape(-1)
        if index.dtype.is_floating_point or index.dtype == torch.bool:
            raise TypeError(f"{what} must be an integer tensor or sequence, got {index.dtype}")
        if index.device.type == "cpu":
            if index.numel() and (int(index.min()) < 0 or int(index.max()) >= len(self)):
                raise ValueError(f"{what} holds a recording outside [0, {len(self)})")
            return index.numel(), self.offsets_host[index.long()], self.lengths_host[index.long()]
        return index.numel(), self.offsets[index.long()], self.lengths[index.long()]

    def _noise(self, noise, B: int):
        """``assemble``'s noise tuple as the noise group of ``_native.assemble_clips``."""
        if len(noise) not in (4, 5):
            raise ValueError("noise must be (noise_clips, noise_index, noise_start, snr_db_or_coeff[, pad_mode])")
        nclips, nindex, nstart, level = noise[:4]
        pad_mode = noise[4] if len(noise) == 5 else "replicate"
        if not isinstance(nclips, PackedClips):
            raise TypeError("noise_clips must be a PackedClips")
        if nclips.store.dtype != self.store.dtype:
            raise TypeError(f"noise_clips holds {nclips.store.dtype} samples, the clips {self.store.dtype}: both int16 PCM or both float32")
        if nclips.store.device != self.store.device:
            raise ValueError(f"noise_clips is on {nclips.store.device}, the clips on {self.store.device}")
        nindex = (nindex if isinstance(nindex, torch.Tensor) else torch.as_tensor(nindex, dtype=torch.int64)).reshape(-1)
        if nindex.dtype.is_floating_point or nindex.dtype == torch.bool:
            raise TypeError(f"noise_index must be an integer tensor or sequence, got {nindex.dtype}")
        if nindex.numel() != B:
            raise ValueError(f"noise_index has {nindex.numel()} entries, expected one per clip ({B})")
        mixed = nindex >= 0                                                    # a negative entry: the clip gets no noise
        _, noff, nlen = nclips._records(nindex.clamp(min=0), "noise_index")
        nlen = torch.where(mixed.to(nlen.device), nlen, torch.zeros_like(nlen))
        if not isinstance(level, torch.Tensor):
            level = torch.as_tensor(level, dtype=torch.float64)
        if level.dim() == 0:
            level = level.reshape(1).expand(B)
        coeff = level if level.dim() == 2 else _native.snr_coefficients(level)
        return (nclips.store, noff, nlen, self._per_clip(nstart, B), self._per_clip(pad_mode, B, _native.PAD_MODES), coeff)

    def assemble(self, index, start, size: int, pad_mode="zero", gain=None, normalize: bool = True, masks=None, out=None,
                 noise=None, gaussian=None, standardize: bool = False) -> torch.Tensor:
        """The batch of the recordings ``index`` (any order, repeats allowed): clip b is recording ``index[b]`` padded by
        ``pad_mode`` ("zero" / "min" / "replicate" / "wrap" or 0..3; one for the batch or one per clip) when it is shorter than
        ``size``, cropped at ``start[b]`` in [0, max(L, size) - size], then ``gain``, peak normalisation and ``masks`` as in
        ``_native.assemble_clips``.  An ``index`` / plan on the CPU is validated (ValueError); on the device it is used unseen and
        the kernel clamps what it finds.

        ``noise`` = (noise_clips, noise_index, noise_start, snr_db_or_coeff, pad_mode="replicate"): clip b is mixed with recording
        ``noise_index[b]`` of the ``PackedClips`` ``noise_clips`` (same dtype and device; a negative index leaves the clip unmixed),
        padded by ``pad_mode`` and cropped at ``noise_start[b]`` like a clip.  The level is one SNR in dB per clip (a number or B of
        them: coeff = r / (1 + r), r = 10^(snr / 10), AddRandomNoise's rule) or, as a (B, 2) float32 tensor, the coefficient pairs
        (c, c') themselves (``_native.noise_coefficients``).  ``gaussian`` = (amp, seed, stream): amplitudes (B,) float32, a 64-bit
        seed and one int64 stream id per clip (``_native.gaussian_noise``); amplitude 0 leaves a clip alone.

        ``standardize``: the reference's ``audio_config.normalize`` -- recording ``index[b]`` as a whole becomes
        ``(r - mean) / (std + 1e-9)`` (``moments()``; torch's float32 rounding) in front of the padding, so "min" pads with the
        standardised recording's minimum and the peak normalisation sees the standardised clip (it is live for an int16 store too).
        The noise recordings are not standardised, as in the reference.  False: the call, and its bits, are what they were."""
        B, rec_off, rec_len = self._records(index)
        std = None
        if standardize:
            std = (self.moments(), (index if isinstance(index, torch.Tensor) else torch.as_tensor(index, dtype=torch.int64)).reshape(-1))
        return _native.assemble_clips(self.store, rec_off, rec_len, self._per_clip(start, B), self._per_clip(pad_mode, B, _native.PAD_MODES),
                                      size, gain, normalize, masks, out, noise=None if noise is None else self._noise(noise, B),
                                      gaussian=gaussian, standardize=std)

    # ---- whole recordings, the way the reference's test.py evaluates them -----------------------------------------------------------

    def peaks(self) -> torch.Tensor:
        """``max |r_i|`` of every recording, ``(len(self),)`` float32 on the store's device (``_native.clip_peaks`` ->
        leaf_clip_peaks_f32: exact, one call over all recordings, split by tiles of samples so that one long recording fills the
        chip and many short ones cost a wave each).  Computed on the first call and kept: the store is taken as immutable after
        construction (``refresh_peaks`` after writing into it)."""
        if self._peaks is None:
            self._peaks = _native.clip_peaks(self.store, self.offsets, self.lengths)
        return self._peaks

    def refresh_peaks(self) -> None:
        """Drop the kept peaks; the next ``peaks()`` computes them again.  The store is taken as immutable after construction: a
        caller that writes into ``store`` all the same calls this afterwards."""
        self._peaks = None

    def moments(self) -> torch.Tensor:
        """``(mean, std, min, max)`` of every recording, ``(len(self), 4)`` float32 on the store's device (``_native.clip_moments``
        -> leaf_clip_moments_f32: float64 accumulation in an order the recording's length fixes, torch's unbiased std, exact min and
        max) -- what ``standardize`` maps the samples with.  Computed on the first call and kept, like ``peaks()``: the store is
        taken as immutable after construction (``refresh_moments`` after writing into it)."""
        if self._moments is None:
            self._moments = _native.clip_moments(self.store, self.offsets, self.lengths)
        return self._moments

    def refresh_moments(self) -> None:
        """Drop the kept moments; the next ``moments()`` computes them again.  The store is taken as immutable after construction: a
        caller that writes into ``store`` all the same calls this afterwards."""
        self._moments = None

    def segment_plan(self, index, size: int):
        """The integers of ``segments``, all on the CPU from ``lengths_host``: ``(counts, rec, win, left)``.  Recording
        ``index[i]`` of L samples becomes ``counts[i] = ceil(L / size)`` rows; with ``P = counts[i] * size`` the reference's
        pad_input pads ``left[i] = (P - L) // 2`` samples in front (and ``P - L - left[i]`` behind), so its row k starts at the
        recording's sample ``win = k * size - left[i]``.  ``rec`` and ``win`` have one entry per row, recording after recording in
        ``index`` order.  ``index`` is a sequence or a CPU tensor (the number of rows follows from it, and nothing is read back from
        the device for it); a recording outside the store or an empty one raises ValueError."""
        size = int(size)
        if not 1 <= size < _native.CALL_SAMPLES:
            raise ValueError(f"size must be in [1, 2^31), got {size}")
        index = (index if isinstance(index, torch.Tensor) else torch.as_tensor(index, dtype=torch.int64)).reshape(-1)
        if index.dtype.is_floating_point or index.dtype == torch.bool:
            raise TypeError(f"index must be an integer tensor or sequence, got {index.dtype}")
        if index.device.type != "cpu":
            raise TypeError("segments takes its index on the CPU: the number of rows is host work on lengths_host")
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= len(self)):
            raise ValueError(f"index holds a recording outside [0, {len(self)})")
        index = index.long()
        L = self.lengths_host[index].long()
        if bool((L == 0).any()):
            raise ValueError("index names an empty recording: it has no rows (the reference's pad_input cannot pad it either)")
        counts = (L + size - 1) // size
        left = (counts * size - L) // 2
        first = torch.cumsum(counts, 0) - counts
        k = torch.arange(int(counts.sum())) - torch.repeat_interleave(first, counts)
        return counts, torch.repeat_interleave(index, counts), k * size - torch.repeat_interleave(left, counts), left

    def _segment_rows(self, rec: torch.Tensor, win: torch.Tensor, size: int, normalize: bool, out=None, standardize: bool = False) -> torch.Tensor:
        """The rows ``(rec, win)`` of a ``segment_plan`` in one launch.  An int16 store has no peak above 1: like
        ``Leaf.fuse_peak_normalization`` for int16, nothing is scaled and ``peaks()`` is not launched.  ``standardize``: the rows of
        the standardised recordings; their peak comes from ``moments()``, for either store."""
        if standardize:
            plan = torch.stack((self.offsets_host[rec], self.lengths_host[rec].long(), win, rec)).to(self.store.device)
            return _native.assemble_segments(self.store, plan[0], plan[1].to(torch.int32), plan[2], size, None, plan[3].to(torch.int32), out,
                                             moments=self.moments() if rec.numel() else torch.zeros((1, 4), device=self.store.device),
                                             normalize=normalize)
        scaled = bool(normalize) and self.store.dtype == torch.float32 and rec.numel() > 0
        # the four row arrays cross in ONE copy (they come from this object's own validated tables: nothing to check again)
        plan = torch.stack((self.offsets_host[rec], self.lengths_host[rec].long(), win, rec)).to(self.store.device)
        return _native.assemble_segments(self.store, plan[0], plan[1].to(torch.int32), plan[2], size,
                                         self.peaks() if scaled else None, plan[3].to(torch.int32) if scaled else None, out)

    def segments(self, index, size: int, normalize: bool = True, out=None, standardize: bool = False):
        """The evaluation batch of the reference's test.py for the recordings ``index`` (any order, repeats allowed), in ONE launch
        (``_native.assemble_segments`` -> leaf_assemble_segments_f32): ``(batch, counts)``.  Per recording r of L samples test.py runs
        ``PeakNormalization`` over the WHOLE recording (``normalize``; the peak comes from ``peaks()``), then ``pad_input`` --
        ``n = ceil(L / size)``, ``F.pad(r, (left, n * size - L - left), 'replicate')`` with ``left = (n * size - L) // 2``,
        ``reshape(-1, 1, size)``.  ``batch`` is the rows of all recordings behind one another, ``(sum n_i, 1, size)`` float32 as
        ``Leaf.forward`` takes it, bit for bit what those stock ops give; ``counts`` the CPU int64 tensor of the ``n_i``
        (``segment_mean(model(batch), counts)`` is test.py's ``torch.mean(preds, dim=0)`` per recording).  An empty ``index`` returns
        ``(0, 1, size)`` and launches nothing; an empty recording raises ValueError.

        ``standardize``: the reference's ``audio_config.normalize`` in front of it all -- the parser's ``(r - mean) / (std + 1e-9)``
        on the whole recording (``moments()``), THEN ``PeakNormalization`` over the whole standardised recording (its peak is
        ``max(|y(min)|, |y(max)|)``, exact: the map is monotone), then ``pad_input``.  An int16 store is scaled too."""
        counts, rec, win, _ = self.segment_plan(index, size)
        if standardize:
            return self._segment_rows(rec, win, int(size), normalize, out, standardize=True), counts
        return self._segment_rows(rec, win, int(size), normalize, out), counts

    def resampled(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99, out_dtype=None) -> "PackedClips":
        """Every recording brought from ``orig_freq`` to ``new_freq`` (``resample``'s definition) in ONE leaf_resample_f32 call for the
        whole data set: a new ``PackedClips`` on the same device whose recording i has ``ceil(L_i n / o)`` samples, packed back to back
        in the order of this one.  ``lengths_host`` / ``offsets_host`` are integer work on the host; the samples never leave the device,
        and an int16 store stays int16 unless ``out_dtype`` says otherwise.  The zero fill outside a recording is the kernel's, so no
        sample of a neighbour enters a result; kept ``peaks()`` and ``moments()`` are not carried over."""
        out_dtype = _resample_out_dtype(self.store.dtype, out_dtype)
        key = _native._resample_params(orig_freq, new_freq, lowpass_filter_width, rolloff)
        table = _native.resample_table(*key)
        L = self.lengths_host.to(torch.int64)
        lengths = (L * table.n + (table.o - 1)) // table.o                       # L < 2^31, n <= 65535: 64 bits hold it
        if lengths.numel() and int(lengths.max()) >= 2 ** 31:
            raise ValueError(f"a recording would have {int(lengths.max())} samples at {new_freq} Hz: beyond the 32-bit length of a recording")
        offsets = torch.cumsum(lengths, 0) - lengths
        dev = self.store.device
        out = torch.empty(int(lengths.sum()), dtype=out_dtype, device=dev)
        if out.numel():
            _native.resample_records(self.store, self.offsets, self.lengths, key[0], key[1], out, offsets.to(dev), key[2], key[3])
        return PackedClips.from_store(out, offsets, lengths)


def _resample_out_dtype(dtype: torch.dtype, out_dtype) -> torch.dtype:
    out_dtype = dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.int16):
        raise TypeError(f"out_dtype must be torch.float32 or torch.int16, got {out_dtype}")
    return out_dtype


def resample(x: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             out_dtype=None) -> torch.Tensor:
    """``x`` ``(..., T)``, float32 or int16 PCM on the device, from ``orig_freq`` to ``new_freq``: ``(..., ceil(T n / o))`` for the
    reduced ratio ``o : n``, every row a recording of its own (leaf_resample_f32, one call).  The band-limited interpolation
    ``torchaudio.functional.resample`` documents -- a Hann-windowed sinc of ``lowpass_filter_width`` zero crossings, cut off at
    ``rolloff`` of the lower Nyquist frequency, zeros outside the row -- as include/leaf_hip.h states it: each output is one float32
    fma chain over its phase's taps in ascending order, so a row's bits depend on the row alone.  ``out_dtype=None`` keeps ``x``'s
    dtype: an int16 batch stays int16 (``rint(y * 32768)``, saturated); ``orig_freq == new_freq`` is the identity and, with
    ``out_dtype``, the int16 <-> float32 conversion.  No gradient flows through it."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a tensor")
    if x.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"x must be float32 or int16 (PCM), got {x.dtype}")
    if x.requires_grad:
        raise RuntimeError("resample: no gradient is built (detach x first)")
    out_dtype = _resample_out_dtype(x.dtype, out_dtype)
    key = _native._resample_params(orig_freq, new_freq, lowpass_filter_width, rolloff)
    if x.dim() < 1:
        raise ValueError("x must have at least one dimension (..., T)")
    _native.resample_table(*key)                                                # (ValueError for a ratio beyond the library)
    _native.require_hip(x, "resample")
    T = x.shape[-1]
    if T >= 2 ** 31:
        raise ValueError(f"a row of {T} samples is beyond the 32-bit length of a recording")
    rows = x.numel() // T if T else 0
    out_len = _native.resample_length(T, key[0], key[1])
    if out_len >= 2 ** 31:
        raise ValueError(f"a result of {out_len} samples per row is beyond the 32-bit length of a recording")
    out = torch.empty(x.shape[:-1] + (out_len,), dtype=out_dtype, device=x.device)
    if rows == 0 or out_len == 0:
        return out
    store = x.detach().contiguous().reshape(-1)
    r = torch.arange(rows, dtype=torch.int64)
    plan = torch.stack((r * T, torch.full_like(r, T), r * out_len)).to(x.device)
    _native.resample_records(store, plan[0], plan[1].to(torch.int32), key[0], key[1], out.reshape(-1), plan[2], key[2], key[3])
    return out


def _segment_sums(preds: torch.Tensor, counts) -> torch.Tensor:
    """Sums over runs of ``counts[i]`` consecutive rows of ``preds``, in float64 (stock ops: one ``index_add_``).  float64 puts the
    order of the additions far below a float32 ulp of the result, and a NaN or infinity stays in its own recording."""
    counts = torch.as_tensor(counts).reshape(-1).cpu().long()
    if counts.numel() and int(counts.min()) < 1:
        raise ValueError("every recording needs at least one row")
    if int(counts.sum()) != preds.shape[0]:
        raise ValueError(f"counts names {int(counts.sum())} rows, preds has {preds.shape[0]}")
    sums = torch.zeros((counts.numel(),) + tuple(preds.shape[1:]), dtype=torch.float64, device=preds.device)
    return sums.index_add_(0, torch.repeat_interleave(torch.arange(counts.numel()), counts).to(preds.device), preds.double())


def _per_row(counts: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return counts.to(like.device).double().reshape((-1,) + (1,) * (like.dim() - 1))


def segment_mean(preds: torch.Tensor, counts) -> torch.Tensor:
    """``(len(counts), ...)``: the mean over each recording's ``counts[i]`` consecutive rows of ``preds`` ``(sum counts, ...)`` --
    test.py's ``torch.mean(preds, dim=0)`` for a batch of recordings (``PackedClips.segments``), in stock ops on the device ``preds``
    is on, in its dtype.  The caller applies sigmoid / argmax to the mean, as test.py does."""
    counts = torch.as_tensor(counts).reshape(-1).cpu().long()
    sums = _segment_sums(preds, counts)
    return (sums / _per_row(counts, sums)).to(preds.dtype)


def evaluate_recordings(model, clips: PackedClips, size: int, index=None, max_rows: int = 512, normalize: bool = True,
                        standardize: bool = False) -> torch.Tensor:
    """The evaluation loop of the reference's test.py over the recordings ``index`` of ``clips`` (default: all of them): ``(N, C)``,
    per recording the mean of ``model``'s outputs over its rows, in ``index`` order; sigmoid / argmax are the caller's, as there.
    Runs under ``torch.no_grad()`` (``model.eval()`` is the caller's).  Instead of test.py's one recording per forward, the rows of
    consecutive recordings are packed into forwards of at most ``max_rows`` rows -- one ``segments`` launch and one ``model`` call
    each; a recording that does not fit the rest of a forward, or has more rows than ``max_rows``, continues in the next one and its
    sum is carried (in float64, as ``segment_mean`` sums).  ``standardize``: the rows of ``clips.segments(..., standardize=True)``,
    the reference's ``audio_config.normalize``."""
    max_rows = int(max_rows)
    if max_rows < 1:
        raise ValueError(f"max_rows must be at least 1, got {max_rows}")
    counts, rec, win, _ = clips.segment_plan(torch.arange(len(clips)) if index is None else index, size)
    if counts.numel() == 0:
        raise ValueError("evaluate_recordings needs at least one recording")
    place = torch.repeat_interleave(torch.arange(counts.numel()), counts)      # the row's recording, as its place in index
    sums, dtype = None, None
    with torch.no_grad():
        for a in range(0, rec.numel(), max_rows):
            b = min(rec.numel(), a + max_rows)
            extra = {"standardize": True} if standardize else {}
            preds = model(clips._segment_rows(rec[a:b], win[a:b], int(size), normalize, **extra))
            first, last = int(place[a]), int(place[b - 1])
            part = _segment_sums(preds, torch.bincount(place[a:b] - first, minlength=last - first + 1))
            if sums is None:
                sums, dtype = torch.zeros((counts.numel(),) + tuple(part.shape[1:]), dtype=torch.float64, device=part.device), preds.dtype
            sums[first:last + 1] += part
        return (sums / _per_row(counts, sums)).to(dtype)


class ClipPlan(tuple):
    """What ``ClipSampler.plan`` returns: ``(rec_off, rec_len, start, pad_mode, gain, masks)``, CPU tensors in the C ABI's dtypes
    (``masks`` None without time masking) -- the arguments of ``_native.assemble_clips`` / leaf_assemble_clips_f32 behind the store."""
    __slots__ = ()
    rec_off, rec_len, start, pad_mode, gain, masks = (property(lambda self, i=i: self[i]) for i in range(6))


class ClipNoisePlan(ClipPlan):
    """A ``ClipPlan`` (the same six entries, unpacking as before) that carries the noise draws as attributes: ``noise`` =
    (noise_off, noise_len, noise_start, noise_pad_mode, coeff) -- ``coeff`` float64, AddRandomNoise's r / (1 + r); ``noise_len`` 0 for
    a clip without background noise -- or None, and ``gaussian`` = (amp, seed, stream) or None: what ``_native.assemble_clips`` takes
    as ``noise`` (behind the noise store) and ``gaussian``.  A standardising sampler adds ``rec``, the clips' recordings (int32: their
    rows of ``PackedClips.moments()``), or None."""
    noise = None
    gaussian = None
    rec = None
    index = None                                                                # DeviceClipSampler: the recordings chosen, int64 on the device


class ClipSampler:
    """The random draws of the reference's training / validation pipelines (raw_transforms.py: get_raw_transforms_v2,
    simple_supervised_transforms, leaf_supervised_transforms) as a per-clip plan, and the batch ``PackedClips`` makes from it:

    - pad mode: ``pad_modes[0]`` with probability ``wrap_pad_prob``, else ``pad_modes[1]`` -- the reference's
      ``OneOf([PadToSize('wrap'), PadToSize('constant')])`` under their honest names: its torch 'wrap' is ``F.pad(..., 'replicate')``
      and its 'constant' pads with ``signal.min()``.  ("wrap", numpy's periodic padding of PadToSize_NP, and "zero" can be named too.)
    - start: uniform in [0, max(L, size) - size] inclusive when ``train`` (RandomCrop), the centre ``(max(L, size) - size) // 2``
      otherwise (CenterCrop).
    - gain: with probability ``gain_prob`` the factor ``10 ** (dB / 20)``, dB uniform in ``gain_db``, else 1.  The default 0.25 is
      the product of the pipelines' two 0.5s (UseWithProb(RandomGain(prob=0.5), prob=0.5)).  RandomGain wraps the third-party
      ``torch_audiomentations.Gain``, which is not in this image: its documented behaviour is restated, parity unpinned.
    - peak normalisation: ``PeakNormalization``'s bits (the same restatement).
    - time masks, with ``num_masks > 0`` (TimeMasking): ``randint(1, num_masks)`` spans per clip, ``n = int(uniform(0, time_perc) *
      size)`` samples from ``t0 = int(uniform(0, size - n))``; the unused spans carry ``n = 0``.

    - background noise, with ``noise_clips`` (a ``PackedClips`` of the clips' dtype and device: AddRandomNoise under
      UseWithProb(..., noise_prob)): a recording chosen uniformly, padded with 'replicate' (the reference's PadToSize(size, "wrap")) and
      cropped at a start uniform in [0, max(Ln, size) - size]; ``snr = uniform(lo, hi + 1)`` dB from ``snr_range``,
      ``coeff = r / (1 + r)``, ``r = exp(snr ln 10 / 10)`` in float64, and the clip becomes ``coeff * x + (1 - coeff) * noise`` in
      front of the gain.
    - Gaussian noise, with ``gaussian_prob > 0`` (AddGaussianNoise under UseWithProb): an amplitude uniform in
      ``gaussian_amplitude``, else 0; ``x + amplitude * z`` behind the gain, in front of the peak normalisation.  ``z`` is the library's
      stream ``_native.gaussian_noise(seed, stream)``: ``gaussian_seed`` (default: the generator's initial seed) and one stream id per
      clip from a counter on the sampler (``next_stream``) that advances by B per call, so no two clips ever share a stream.

    All draws come from a CPU ``torch.Generator`` (``generator``; a fresh default-seeded one otherwise): the same seed gives the same
    plan.  The noise draws come after all the others, so a sampler without noise draws what it always drew.  With noise ``plan``
    returns a ``ClipNoisePlan``: the same 6-tuple, the noise draws as attributes.
    The reference's own ``random`` / ``numpy.random`` streams are NOT reproduced -- the distributions are, the numbers are not.
    ``plan(index)`` returns the draws (``ClipPlan``), ``__call__(index)`` the assembled ``(B, 1, size)`` float32 batch.

    - ``standardize`` (``audio_config.normalize``): no draw -- the plan carries the clips' recordings (``plan.rec``, a
      ``ClipNoisePlan`` then) and the batch is assembled from the standardised recordings (``PackedClips.assemble(...,
      standardize=True)``).  A sampler without it draws and returns what it always did.

    ClipValue and RandomReverb, which the reference itself has switched off, are ``EffectsClipSampler``'s: a launch of their own
    between two launches of this sampler's kernel."""

    def __init__(self, clips: PackedClips, size: int, train: bool = True, pad_modes=("replicate", "min"), wrap_pad_prob: float = 0.5,
                 gain_prob: float = 0.25, gain_db=(-18.0, 6.0), peak_normalize: bool = True, time_perc: float = 0.0, num_masks: int = 0,
                 generator=None, noise_clips=None, noise_prob: float = 0.5, snr_range=(10, 25), gaussian_prob: float = 0.0,
                 gaussian_amplitude=(0.001, 0.015), gaussian_seed=None, standardize: bool = False):
        self.clips, self.size, self.train = clips, int(size), bool(train)
        self.standardize = bool(standardize)
        self.pad_modes = tuple(_native.PAD_MODES[m] if isinstance(m, str) else int(m) for m in pad_modes)
        if len(self.pad_modes) != 2 or any(m not in _native.PAD_MODES.values() for m in self.pad_modes):
            raise ValueError(f"pad_modes must name two of {sorted(_native.PAD_MODES)}")
        self.wrap_pad_prob, self.gain_prob, self.gain_db = float(wrap_pad_prob), float(gain_prob), (float(gain_db[0]), float(gain_db[1]))
        self.peak_normalize, self.time_perc, self.num_masks = bool(peak_normalize), float(time_perc), int(num_masks)
        self.generator = generator if generator is not None else torch.Generator()
        if noise_clips is not None:
            if not isinstance(noise_clips, PackedClips):
                raise TypeError("noise_clips must be a PackedClips")
            if noise_clips.store.dtype != clips.store.dtype:
                raise TypeError(f"noise_clips holds {noise_clips.store.dtype} samples, the clips {clips.store.dtype}")
            if noise_clips.store.device != clips.store.device:
                raise ValueError(f"noise_clips is on {noise_clips.store.device}, the clips on {clips.store.device}")
        self.noise_clips, self.noise_prob = noise_clips, float(noise_prob)
        self.snr_range = (float(snr_range[0]), float(snr_range[1]))
        self.gaussian_prob = float(gaussian_prob)
        self.gaussian_amplitude = (float(gaussian_amplitude[0]), float(gaussian_amplitude[1]))
        self.gaussian_seed = (self.generator.initial_seed() if gaussian_seed is None else int(gaussian_seed)) % 2 ** 64
        self.next_stream = 0                                                    # the first stream id of the next batch

    def _uniform(self, *shape) -> torch.Tensor:
        return torch.rand(*shape, dtype=torch.float64, generator=self.generator)

    def plan(self, index) -> ClipPlan:
        index = torch.as_tensor(index).reshape(-1).cpu().long()
        B, S = index.numel(), self.size
        if B and (int(index.min()) < 0 or int(index.max()) >= len(self.clips)):
            raise ValueError(f"index holds a recording outside [0, {len(self.clips)})")
        rec_off, rec_len = self.clips.offsets_host[index], self.clips.lengths_host[index]
        first = self._uniform(B) < self.wrap_pad_prob
        pad_mode = torch.where(first, self.pad_modes[0], self.pad_modes[1]).to(torch.int32)
        span = (rec_len.long() - S).clamp_(min=0)                              # max(L, S) - S
        if self.train:
            start = torch.minimum((self._uniform(B) * (span + 1).double()).floor().long(), span)
        else:
            start = span // 2
        apply = self._uniform(B) < self.gain_prob
        db = self.gain_db[0] + (self.gain_db[1] - self.gain_db[0]) * self._uniform(B)
        gain = torch.where(apply, torch.pow(10.0, db / 20.0), 1.0).to(torch.float32)
        masks = None
        if self.num_masks > 0:
            used = torch.randint(1, self.num_masks + 1, (B, 1), generator=self.generator)
            n = (self._uniform(B, self.num_masks) * self.time_perc * S).long()
            n = torch.where(torch.arange(self.num_masks).reshape(1, -1) < used, n, 0).clamp_(0, S)
            t0 = (self._uniform(B, self.num_masks) * (S - n).double()).long()
            masks = torch.stack((t0, n), dim=2).to(torch.int32)
        entries = (rec_off.clone(), rec_len.clone(), start.to(torch.int32), pad_mode, gain, masks)
        if self.noise_clips is None and self.gaussian_prob <= 0.0 and not self.standardize:
            return ClipPlan(entries)
        plan = ClipNoisePlan(entries)
        if self.standardize:
            plan.rec = index.to(torch.int32)
        if self.noise_clips is not None:                                        # AddRandomNoise
            nc = self.noise_clips
            apply = self._uniform(B) < self.noise_prob
            snr = self.snr_range[0] + (self.snr_range[1] + 1.0 - self.snr_range[0]) * self._uniform(B)
            rec = (self._uniform(B) * len(nc)).floor().long().clamp_(max=len(nc) - 1)
            noff, nlen = nc.offsets_host[rec], nc.lengths_host[rec]
            nspan = (nlen.long() - S).clamp_(min=0)
            nstart = torch.minimum((self._uniform(B) * (nspan + 1).double()).floor().long(), nspan)
            plan.noise = (noff.clone(), torch.where(apply, nlen, torch.zeros_like(nlen)), torch.where(apply, nstart, 0).to(torch.int32),
                          torch.full((B,), _native.PAD_REPLICATE, dtype=torch.int32), _native.snr_coefficients(snr))
        if self.gaussian_prob > 0.0:                                            # AddGaussianNoise
            apply = self._uniform(B) < self.gaussian_prob
            amp = self.gaussian_amplitude[0] + (self.gaussian_amplitude[1] - self.gaussian_amplitude[0]) * self._uniform(B)
            stream = torch.arange(self.next_stream, self.next_stream + B, dtype=torch.int64)
            self.next_stream += B
            plan.gaussian = (torch.where(apply, amp, 0.0).to(torch.float32), self.gaussian_seed, stream)
        return plan

    def __call__(self, index, out=None) -> torch.Tensor:
        plan = self.plan(index)
        rec_off, rec_len, start, pad_mode, gain, masks = plan
        noise, rec = getattr(plan, "noise", None), getattr(plan, "rec", None)
        return _native.assemble_clips(self.clips.store, rec_off, rec_len, start, pad_mode, self.size, gain, self.peak_normalize, masks, out,
                                      noise=None if noise is None else (self.noise_clips.store,) + tuple(noise),
                                      gaussian=getattr(plan, "gaussian", None),
                                      standardize=None if rec is None else (self.clips.moments(), rec))


clip_effects = _native.clip_effects
reverb_plan = _native.reverb_plan


class ClipEffectsPlan(ClipNoisePlan):
    """A ``ClipNoisePlan`` (the same six entries, ``noise`` / ``gaussian`` / ``rec`` as the parent sampler fills them) that carries
    the effect draws: ``clip_factor`` (B,) float32, negative for a clip without ClipValue, and ``reverb`` = (feedback (B,) float32,
    damp (B,) float32, comb (B, 8) int32), all zero for a clip without reverb -- the arguments of ``clip_effects``."""
    clip_factor = None
    reverb = None


class EffectsClipSampler(ClipSampler):
    """``ClipSampler`` with the two transforms the reference's get_raw_transforms_v2 holds between AddRandomNoise and RandomGain and
    has switched off -- ClipValue ("needs work") and RandomReverb ("TOO SLOW": sox's reverb per clip on the CPU) -- run on the device
    by ``clip_effects`` (leaf_clip_effects_f32, where both are stated bit for bit).  Keywords and defaults beyond ``ClipSampler``'s are
    the reference's:

    - ClipValue under ``clip_prob``: the clip is clamped into ``[min(x) * f, max(x) * f]``, ``f = uniform(0, max_clip_val)``.
    - RandomReverb under ``reverb_prob``: three inclusive integer draws, reverberance from ``reverb_range``, damping from
      ``damping_range`` and room scale from ``room_scale_range`` (percent), turned into the kernel's plan by ``reverb_plan`` at
      ``sample_rate``.  This restates sox's published algorithm; neither sox nor ``augment`` is in this image, so parity with sox is
      unpinned (as RandomGain's and PeakNormalization's is).  Left out: sox's tone filters, stereo depth, pre-delay, wet-only mode
      and the drain tail -- the batch keeps ``size`` samples.

    ``plan(index)`` makes ``ClipSampler``'s draws first and unchanged, then the effects' (ClipValue: apply flag, factor; reverb: apply
    flag, the three integers): from one generator state the parent's part of the plan is what ``ClipSampler`` draws.  It returns a
    ``ClipEffectsPlan``.  ``__call__`` is three launches in the reference's order: the assemble with pad / crop, background noise and
    standardisation only; ``clip_effects``; and the assemble again over that batch viewed as a packed store, which carries the gain,
    the Gaussian noise, the peak normalisation and the masks.  With both probabilities 0 the batch is bit for bit ``ClipSampler``'s."""

    def __init__(self, clips: PackedClips, size: int, *args, clip_prob: float = 0.0, max_clip_val: float = 0.2, reverb_prob: float = 0.0,
                 reverb_range=(10, 50), damping_range=(10, 50), room_scale_range=(0, 100), sample_rate: int = 16000, **kwargs):
        super().__init__(clips, size, *args, **kwargs)
        self.clip_prob, self.max_clip_val, self.reverb_prob = float(clip_prob), float(max_clip_val), float(reverb_prob)
        if not (self.max_clip_val >= 0.0 and self.max_clip_val < float("inf")):
            raise ValueError(f"max_clip_val must be finite and at least 0, got {max_clip_val}")
        ranges = []
        for name, r in (("reverb_range", reverb_range), ("damping_range", damping_range), ("room_scale_range", room_scale_range)):
            lo, hi = int(r[0]), int(r[1])
            if not 0 <= lo <= hi <= 100:
                raise ValueError(f"{name} must be two integer percentages 0 <= lo <= hi <= 100, got {tuple(r)}")
            ranges.append((lo, hi))
        self.reverb_range, self.damping_range, self.room_scale_range = ranges
        self.sample_rate = int(sample_rate)
        _native._reverb_caps(self.sample_rate)                                  # (ValueError for a rate the launch would refuse)
        _native.reverb_lengths(self.sample_rate, self.room_scale_range[0])

    def _integers(self, B: int, lo: int, hi: int) -> torch.Tensor:
        return torch.randint(lo, hi + 1, (B,), generator=self.generator)

    def plan(self, index) -> ClipEffectsPlan:
        base = super().plan(index)
        plan = ClipEffectsPlan(tuple(base))
        plan.noise, plan.gaussian, plan.rec = getattr(base, "noise", None), getattr(base, "gaussian", None), getattr(base, "rec", None)
        B = base.rec_off.numel()
        apply = self._uniform(B) < self.clip_prob                               # ClipValue
        factor = self._uniform(B) * self.max_clip_val
        plan.clip_factor = torch.where(apply, factor, -1.0).to(torch.float32)
        apply = self._uniform(B) < self.reverb_prob                             # RandomReverb
        rev, dmp, room = (self._integers(B, *r) for r in (self.reverb_range, self.damping_range, self.room_scale_range))
        feedback, damp, comb = _native.reverb_plan(rev, dmp, room, self.sample_rate)
        zero = torch.zeros((), dtype=torch.float32)
        plan.reverb = (torch.where(apply, feedback, zero), torch.where(apply, damp, zero), torch.where(apply.reshape(-1, 1), comb, 0).to(torch.int32))
        return plan

    def __call__(self, index, out=None) -> torch.Tensor:
        plan = self.plan(index)
        rec_off, rec_len, start, pad_mode, gain, masks = plan
        B, S = rec_off.numel(), self.size
        # 1. pad / crop, background noise, standardisation: gain 1, no Gaussian noise, no peak normalisation, no masks
        raw = _native.assemble_clips(self.clips.store, rec_off, rec_len, start, pad_mode, S, None, False, None, None,
                                     noise=None if plan.noise is None else (self.noise_clips.store,) + tuple(plan.noise),
                                     standardize=None if plan.rec is None else (self.clips.moments(), plan.rec))
        # 2. ClipValue and the reverb
        wet = _native.clip_effects(raw, plan.clip_factor, plan.reverb, self.sample_rate)
        # 3. gain, Gaussian noise, peak normalisation, masks: the batch as a packed store of B recordings of S samples
        rows = torch.arange(B, dtype=torch.int64)
        whole, zeros = torch.full((B,), S, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        return _native.assemble_clips(wet.reshape(-1), rows * S, whole, zeros, zeros, S, gain, self.peak_normalize, masks, out,
                                      gaussian=plan.gaussian)


class DeviceClipSampler:
    """``ClipSampler`` with the draws made ON THE DEVICE (``_native.draw_clip_plan`` -> leaf_draw_clip_plan, one launch of one
    workgroup): the same distributions -- pad mode, crop start, gain, time masks, background noise, Gaussian amplitude; the keywords and
    defaults are ``ClipSampler``'s -- from a counter-based generator (Philox4x32-10 keyed by ``seed``) and a step counter that lives in
    device memory.  Nothing crosses from the host per step, so ``sampler(out=static)`` captures into a graph
    (``torch.cuda.graph``) and every replay draws a fresh plan; include/leaf_hip.h states the draws bit for bit.

    - The uniforms are 32-bit (``r * 2**-32``) where ``ClipSampler``'s are 53-bit: a spacing far below anything the pipelines can
      see.  Neither ``ClipSampler``'s numbers nor the reference's are reproduced -- the distributions are.
    - Clip b of step s has the id ``stream_base + s * B + b`` (64-bit, wrapping): its draws depend on (seed, id) alone, and the id is
      also its Gaussian stream.  Samplers that share a seed (data-parallel ranks) take disjoint ``stream_base`` ranges.
    - ``plan(index=None)`` launches the draw and returns a ``ClipNoisePlan`` of DEVICE tensors -- the sampler's static buffers, the
      same objects on every call, overwritten by the next one -- with ``.noise`` / ``.gaussian`` / ``.rec`` as ``ClipSampler`` fills
      them (``coeff`` as the (B, 2) float32 pairs) and ``.index``, the recordings chosen (int64: gather the labels with it; also
      ``sampler.index`` after the call).  It advances the counter.  ``__call__(index=None, out=None)`` is ``plan`` followed by ``_native.assemble_clips`` on those tensors:
      two launches, nothing from the host between them.
    - ``index``: a device tensor is used as it is (a static buffer under capture; entries outside the store are clamped by the
      kernel); a CPU tensor or sequence is validated (ValueError) and copied.  Without it clip b is ``order[(s * B + b) % len(order)]``
      -- ``order`` an int64 device tensor the caller reshuffles in place between epochs (default: 0 .. len(clips) - 1) -- for
      ``batch_size`` clips.
    - ``step`` / ``set_step(n)`` read and write the counter; they are eager and the only calls that synchronise.
    - ``standardize=True`` computes ``clips.moments()`` in the constructor, so nothing is computed under a capture.  The buffers of
      ``batch_size`` are allocated there too; another batch size allocates its own on first use (do that before capturing).

    Mixup's ``perm`` / ``lam`` are ``DeviceMixup``'s, a launch and a counter of their own.  Not built: bfloat16."""

    def __init__(self, clips: PackedClips, size: int, train: bool = True, pad_modes=("replicate", "min"), wrap_pad_prob: float = 0.5,
                 gain_prob: float = 0.25, gain_db=(-18.0, 6.0), peak_normalize: bool = True, time_perc: float = 0.0, num_masks: int = 0,
                 *, noise_clips=None, noise_prob: float = 0.5, snr_range=(10, 25), gaussian_prob: float = 0.0,
                 gaussian_amplitude=(0.001, 0.015), gaussian_seed=None, standardize: bool = False, seed: int = 0, stream_base: int = 0,
                 order=None, batch_size=None):
        self.clips, self.size, self.train = clips, int(size), bool(train)
        if not 1 <= self.size < _native.CALL_SAMPLES:
            raise ValueError(f"size must be in [1, 2^31), got {self.size}")
        self.standardize, self.peak_normalize = bool(standardize), bool(peak_normalize)
        modes = tuple(_native.PAD_MODES[m] if isinstance(m, str) else int(m) for m in pad_modes)
        if len(modes) != 2 or any(m not in _native.PAD_MODES.values() for m in modes):
            raise ValueError(f"pad_modes must name two of {sorted(_native.PAD_MODES)}")
        if not 0 <= int(num_masks) <= _native.DRAW_MAX_MASKS:
            raise ValueError(f"num_masks must be in [0, {_native.DRAW_MAX_MASKS}], got {num_masks}")
        if noise_clips is not None:
            if not isinstance(noise_clips, PackedClips):
                raise TypeError("noise_clips must be a PackedClips")
            if noise_clips.store.dtype != clips.store.dtype:
                raise TypeError(f"noise_clips holds {noise_clips.store.dtype} samples, the clips {clips.store.dtype}")
            if noise_clips.store.device != clips.store.device:
                raise ValueError(f"noise_clips is on {noise_clips.store.device}, the clips on {clips.store.device}")
        self.noise_clips = noise_clips
        self.consts = dict(pad_modes=modes, wrap_pad_prob=float(wrap_pad_prob), gain_prob=float(gain_prob),
                           gain_db=(float(gain_db[0]), float(gain_db[1])), num_masks=int(num_masks), time_perc=float(time_perc),
                           noise_prob=float(noise_prob), snr_range=(float(snr_range[0]), float(snr_range[1])),
                           gaussian_prob=float(gaussian_prob), gaussian_amplitude=(float(gaussian_amplitude[0]), float(gaussian_amplitude[1])))
        self.seed, self.stream_base = int(seed) % 2 ** 64, int(stream_base) % 2 ** 64
        self.gaussian_seed = self.seed if gaussian_seed is None else int(gaussian_seed) % 2 ** 64
        _native.require_hip(clips.store, "DeviceClipSampler")
        dev = clips.store.device
        self._state = torch.zeros(1, dtype=torch.int64, device=dev)             # the step counter's 64 bits
        if order is None:
            order = torch.arange(len(clips), dtype=torch.int64, device=dev)
        if not isinstance(order, torch.Tensor) or order.dtype != torch.int64 or order.device != dev or order.dim() != 1 or order.numel() < 1:
            raise ValueError(f"order must be a 1-D int64 tensor of at least one entry on {dev}")
        self.order = order.contiguous()
        self.moments = clips.moments() if self.standardize else None
        self.batch_size = None if batch_size is None else int(batch_size)
        self._plans = {}                                                        # batch size -> (plan, out dict, index buffer)
        self.index = None                                                       # the last plan's recordings (its static buffer)
        if self.batch_size is not None:
            self._buffers(self.batch_size)

    def _buffers(self, B: int):
        if B not in self._plans:
            if B < 1:
                raise ValueError(f"a batch needs at least one clip, got {B}")
            dev, M = self.clips.store.device, self.consts["num_masks"]
            new = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=dev)
            out = dict(rec_off=new(torch.int64, B), rec_len=new(torch.int32, B), start=new(torch.int32, B), pad_mode=new(torch.int32, B),
                       gain=new(torch.float32, B), index=new(torch.int64, B))
            if M > 0:
                out["masks"] = new(torch.int32, B, M, 2)
            if self.standardize:
                out["rec"] = new(torch.int32, B)
            if self.noise_clips is not None:
                out.update(noise_off=new(torch.int64, B), noise_len=new(torch.int32, B), noise_start=new(torch.int32, B),
                           noise_pad_mode=new(torch.int32, B), coeff=new(torch.float32, B, 2))
            if self.consts["gaussian_prob"] > 0.0:
                out.update(gauss_amp=new(torch.float32, B), gauss_stream=new(torch.int64, B))
            plan = ClipNoisePlan((out["rec_off"], out["rec_len"], out["start"], out["pad_mode"], out["gain"], out.get("masks")))
            plan.index, plan.rec = out["index"], out.get("rec")
            if self.noise_clips is not None:
                plan.noise = (out["noise_off"], out["noise_len"], out["noise_start"], out["noise_pad_mode"], out["coeff"])
            if "gauss_amp" in out:
                plan.gaussian = (out["gauss_amp"], self.gaussian_seed, out["gauss_stream"])
            self._plans[B] = (plan, out, new(torch.int64, B))
        return self._plans[B]

    @property
    def step(self) -> int:
        """The counter: the step the next ``plan`` draws (synchronises)."""
        return int(self._state.item()) % 2 ** 64

    def set_step(self, n: int) -> None:
        """Position the counter: the next ``plan`` draws step ``n`` (mod 2^64)."""
        n = int(n) % 2 ** 64
        self._state.fill_(n - 2 ** 64 if n >= 2 ** 63 else n)

    def plan(self, index=None, advance: bool = True) -> ClipNoisePlan:
        if index is None:
            if self.batch_size is None:
                raise ValueError("without an index the sampler walks `order`: construct it with batch_size")
            B, dindex = self.batch_size, None
        else:
            if not isinstance(index, torch.Tensor):
                index = torch.as_tensor(index, dtype=torch.int64)
            if index.dtype.is_floating_point or index.dtype == torch.bool:
                raise TypeError(f"index must be an integer tensor or sequence, got {index.dtype}")
            index = index.reshape(-1)
            B = index.numel()
        plan, out, ibuf = self._buffers(B)
        if index is not None:
            if index.device.type == "cpu":
                if int(index.min()) < 0 or int(index.max()) >= len(self.clips):
                    raise ValueError(f"index holds a recording outside [0, {len(self.clips)})")
                dindex = ibuf.copy_(index)
            else:
                dindex = index.to(torch.int64).contiguous()
        nc = self.noise_clips
        _native.draw_clip_plan(B, self.size, self.train, self.clips.offsets, self.clips.lengths, self._state, self.seed, self.stream_base,
                               self.consts, out, index=dindex, order=None if dindex is not None else self.order,
                               noise_offsets=None if nc is None else nc.offsets, noise_lengths=None if nc is None else nc.lengths,
                               advance=advance)
        self.index = plan.index
        return plan

    def __call__(self, index=None, out=None) -> torch.Tensor:
        plan = self.plan(index)
        rec_off, rec_len, start, pad_mode, gain, masks = plan
        return _native.assemble_clips(self.clips.store, rec_off, rec_len, start, pad_mode, self.size, gain, self.peak_normalize, masks, out,
                                      noise=None if plan.noise is None else (self.noise_clips.store,) + plan.noise,
                                      gaussian=plan.gaussian, standardize=None if plan.rec is None else (self.moments, plan.rec))


class DeviceMixup:
    """``Mixup``'s draws made ON THE DEVICE (``_native.draw_mixup`` -> leaf_draw_mixup, one launch of one workgroup): one permutation
    of the batch and one weight per clip from Beta(alpha, alpha), from the counter-based generator of ``DeviceClipSampler`` (Philox4x32-10
    keyed by ``seed``) and a step counter of its own in device memory.  Nothing crosses from the host per step, so ``mix()`` captures into
    a graph (``torch.cuda.graph``) and every replay mixes other pairs with other weights -- with any ``alpha``, 0.3 as well as 1;
    include/leaf_hip.h states the draws.

    - ``perm, lam = mix()``: int32 ``(B,)`` and float32 ``(B,)``, the mixer's static buffers -- the same tensors on every call,
      overwritten by the next one -- in the form ``Leaf.forward_mixup(x, perm, lam)`` and ``_native.mixup`` take without a copy.  The
      call validates nothing on the device and allocates nothing.  ``mix(advance=False)`` draws the step without advancing.
    - Clip b of step s has the id ``stream_base + s * B + b`` (64-bit, wrapping); its draws depend on (seed, id) alone and lie in a
      domain of their own (counter word 1 is 2): a mixer may share seed and ids with a ``DeviceClipSampler`` without sharing numbers.
    - ``targets(t)`` mixes the labels with the pair drawn last, returning the last four values of the reference's ``do_mixup``.  Mode
      "multilabel": ``(mixed_y, None, None, None)`` with ``mixed_y = t * lam + t[perm] * (1 - lam)`` per clip -- float32 ``t`` of
      ``B`` rows through ``_native.mixup`` (one launch, bit for bit that separately rounded expression).  Any other mode:
      ``(t, t[perm], lam, None)`` by stock indexing.
    - ``step`` / ``set_step(n)`` read and write the counter; they are eager and the only calls that synchronise.

    Neither numpy's nor torch's numbers are reproduced (``Mixup`` keeps the reference's): the distributions are."""

    def __init__(self, batch_size: int, alpha: float = 1.0, seed: int = 1234, stream_base: int = 0, mode: str = "multilabel", device="cuda"):
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= _native.MIX_MAX_BATCH:
            raise ValueError(f"batch_size must be in [1, {_native.MIX_MAX_BATCH}], got {batch_size}")
        self.alpha = _native.mix_alpha(alpha)
        self.seed, self.stream_base = int(seed) % 2 ** 64, int(stream_base) % 2 ** 64
        self.mode = mode
        self._state = torch.zeros(1, dtype=torch.int64, device=device)          # the step counter's 64 bits
        _native.require_hip(self._state, "DeviceMixup")
        self.perm = torch.arange(self.batch_size, dtype=torch.int32, device=device)
        self.lam = torch.ones(self.batch_size, dtype=torch.float32, device=device)

    @property
    def step(self) -> int:
        """The counter: the step the next call draws (synchronises)."""
        return int(self._state.item()) % 2 ** 64

    def set_step(self, n: int) -> None:
        """Position the counter: the next call draws step ``n`` (mod 2^64)."""
        n = int(n) % 2 ** 64
        self._state.fill_(n - 2 ** 64 if n >= 2 ** 63 else n)

    def __call__(self, advance: bool = True):
        _native.draw_mixup(self.batch_size, self.alpha, self._state, self.seed, self.stream_base, self.perm, self.lam, advance=advance)
        return self.perm, self.lam

    def targets(self, t: torch.Tensor):
        if t.dim() < 1 or t.shape[0] != self.batch_size:
            raise ValueError(f"targets of shape {tuple(t.shape)} for a mixer of {self.batch_size} clips")
        if self.mode != "multilabel":
            return t, t[self.perm], self.lam, None
        if t.dtype != torch.float32:
            raise TypeError(f"multilabel targets are mixed in float32, got {t.dtype}")
        return _native.mixup(t.reshape(self.batch_size, -1), self.perm, self.lam).reshape(t.shape), None, None, None
