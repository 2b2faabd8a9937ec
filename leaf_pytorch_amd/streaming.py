"""Chunked real-time use of the frontend ("very-long-clip time tiling with EMA carry"; not part of the reference
surface -- the reference only ever sees whole clips).

``LeafStream(leaf)`` is fed consecutive chunks of B running waveforms and returns, chunk by chunk, exactly the frames
``leaf`` would produce for the whole recording: a frame is emitted as soon as every sample of its receptive field has
arrived (25 ms after its centre at the default geometry), the waveform history the next frames still need is kept on the
device (2 (K - 1) samples plus alignment), and the PCEN smoother's state travels between calls (``leaf_pcen_stream_f32``).
``flush()`` ends the stream: the remaining frames are produced with the reference's zero padding at the end of the clip.

Every call is two launches of the product kernels: the fused forward without compression on [history | chunk] (the
overlap-save or MFMA path ``LEAF_ALGO_AUTO`` picks for that length), then the stateful PCEN over the new frames.

``LeafStream(leaf, fused=True)`` is the same stream with ONE launch per step (``leaf_stream_step_f32``,
csrc/leaf_fft_stream.hpp): the history and the smoother state live in one device buffer allocated once, the kernel reads
[history | chunk] from the two buffers, emits only the new frames and hands the history over; no ``cat``, no slicing, no
allocation per step beyond the frames returned.  16 kHz and 8 kHz geometries (the static instances of the one-launch kernel).

``LeafStreamBank(leaf, slots)`` serves INDEPENDENT streams -- they begin and end at different times and take chunks of different
lengths -- with that kernel, one call per step for the whole bank (``leaf_stream_bank_step_f32``).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _native


def _geometry(K: int, hop: int):
    """(lead, reach) of a window / hop: see LeafStream.__init__."""
    pad_l = K // 2 + K % 2 - 1
    return -(-2 * pad_l // hop), 2 * (K - 1 - pad_l)


def stream_plan(hist_len: int, next_frame: int, Tc: int, K: int, hop: int, final: bool):
    """Where one step takes a stream: the arithmetic of ``step``, ``_advance`` and ``flush`` in one place, on integers alone.

    The stream holds ``hist_len`` samples, ``next_frame`` (numbered from the first of them) is the next frame to emit, and ``Tc``
    samples arrive (``final``: none do, the stream ends and the frames still owed come with zero padding behind the last sample).
    Returns ``(first, n, drop_samples, new_hist_len, new_next)``: frames ``first .. first + n - 1`` of the buffer [history | chunk]
    are emitted, its samples from ``drop_samples`` on are the next step's history, ``new_hist_len`` of them, and ``new_next`` is the
    next frame to emit in that buffer's numbering.  These are the position arguments of ``leaf_stream_step_f32``."""
    lead, reach = _geometry(K, hop)
    L = hist_len + Tc
    last = (L - 1) // hop if final else (L - 1 - reach) // hop            # last frame of the clip / whose receptive field is complete
    n = max(0, last - next_frame + 1)
    if final:
        return next_frame, n, L, 0, 0
    if n == 0:
        return next_frame, 0, 0, L, next_frame
    drop = max(0, last + 1 - lead)                                        # whole hops in front that frame last + 1 no longer needs
    return next_frame, n, drop * hop, L - drop * hop, last + 1 - drop


def stream_capacity(K: int, hop: int) -> int:
    """Samples [history | chunk] of one ``leaf_stream_step_f32`` call: one pass of the one-launch kernel's ring, kSmallRing = 10
    blocks of fft_block_len(K, hop) valid outputs of a 2048-point transform (csrc/leaf_fft.hpp, csrc/leaf_fft_small.hpp)."""
    unit = 64 // math.gcd(64, hop) * hop
    return 10 * ((2048 - K + 1) // unit * unit)


class LeafStream:
    def __new__(cls, leaf, log1p: bool = False, fused: bool = False, out_dtype=None):
        return object.__new__(_FusedLeafStream if fused and cls is LeafStream else cls)

    def __init__(self, leaf, log1p: bool = False, fused: bool = False, out_dtype=None):
        """``fused=True``: one launch per step (module docstring; ``ValueError`` for a geometry the one-launch kernel does not
        serve).  ``out_dtype=torch.bfloat16`` (needs ``fused=True``, ``ValueError`` otherwise): the frames come back in bfloat16,
        rounded where the kernel stores them; the module's own ``output_dtype()`` is not consulted."""
        if out_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f"LeafStream: out_dtype must be None, torch.float32 or torch.bfloat16, got {out_dtype!r}")
        if out_dtype is torch.bfloat16 and not fused:
            raise ValueError("LeafStream: out_dtype=torch.bfloat16 needs fused=True (the two-launch stream returns float32 frames)")
        conv, pool = leaf._complex_conv, leaf._pooling
        self.leaf = leaf
        self.K, self.hop, self.F = conv._kernel_size, pool.strides, conv._filters
        self.pad_l = self.K // 2 + self.K % 2 - 1                          # utils.py:5-10
        self.pad_r = self.K // 2
        # a frame m' of the buffer is exact once the buffer starts a whole number of hops, >= 2 pad_l samples, before it (its
        # pooling window reaches pad_l back, the filters another pad_l) ...
        self.lead = -(-2 * self.pad_l // self.hop)                        # frames of lead-in
        # ... and holds every sample up to m' hop + 2 (K - 1 - pad_l)
        self.reach = 2 * (self.K - 1 - self.pad_l)
        self.log1p = bool(log1p) or bool(getattr(leaf, "_log1p", False))   # the module's log_compression() switch, or asked for here
        # (B, L): the samples still needed, from a whole number of hops before the next frame to emit.  At the start of a
        # stream the buffer begins at the recording's first sample -- the reference zero-pads the ENERGY in front of a clip
        # (frontend.py:15-19 then pooling.py:41), not the waveform, so the first frames must see the true clip start --
        # and `next` (the buffer's frame number of the next frame to emit) starts at 0; later it stays at `lead`.
        self.buf: Optional[torch.Tensor] = None
        self.next = 0
        self.state: Optional[torch.Tensor] = None                         # (B, F): PCEN smoother after the last emitted frame
        self.started = False                                              # a frame has been emitted (the smoother has a state)

    def _pooled(self, x2: torch.Tensor) -> torch.Tensor:
        """Floored pooled frames (B, F, n) of the buffer through the fused forward, compression off."""
        sd = self.leaf
        return _native.leaf_forward(x2, sd._complex_conv._kernel, sd._pooling.weights, sd._pooling._bias, None, None, None, None,
                                    self.K, self.hop, pcen=False, log1p=False, algo=_native.ALGO_AUTO)

    def _emit(self, first: int, last: int) -> torch.Tensor:
        """Frames first..last (buffer numbering) finalized with the carried smoother state."""
        pooled = self._pooled(self.buf)[:, :, first:last + 1].contiguous()
        c = self.leaf._compression
        if c is None:
            out, _ = _native.pcen_stream(pooled, None, None, None, None, 1e-12, None, log1p=self.log1p)
            return out
        out, self.state = _native.pcen_stream(pooled, c.alpha, c.delta, c.root, c.ema._weights, c._floor,
                                              self.state if self.started else None)
        self.started = True
        return out

    @torch.no_grad()
    def step(self, chunk: torch.Tensor) -> torch.Tensor:
        """chunk (B,1,Tc) or (B,Tc) on the device -> the frames that became final, (B,F,n) float32 with n >= 0.  Chunks are float32
        (every other type but int16 is widened with ``.float()``, as before), or int16 for 16-bit PCM (a sample v means v / 32768): then the history buffer stays
        int16 and the int16 forward runs on it.  A stream keeps the type of its first chunk: a change in mid-stream raises."""
        pcm = chunk.dtype == torch.int16
        if self.buf is not None and pcm != (self.buf.dtype == torch.int16):
            raise RuntimeError(f"LeafStream.step: this stream holds {'int16 PCM' if self.buf.dtype == torch.int16 else 'float32'} "
                               f"samples and got a {chunk.dtype} chunk: one sample type per stream (flush() ends it)")
        _native.require_hip(chunk, "LeafStream.step")
        x2 = chunk[:, 0, :] if chunk.dim() == 3 else chunk
        x2 = x2 if pcm else x2.float()
        self.buf = x2 if self.buf is None else torch.cat([self.buf, x2], dim=1)
        last = (self.buf.shape[1] - 1 - self.reach) // self.hop           # last frame whose receptive field is complete
        if last < self.next:
            return chunk.new_empty((x2.shape[0], self.F, 0), dtype=torch.float32)
        out = self._emit(self.next, last)
        self._advance(last + 1)
        return out

    def _advance(self, nxt: int) -> None:
        """Frame `nxt` (buffer numbering) is the next to emit: drop the whole hops in front that it no longer needs."""
        drop = max(0, nxt - self.lead)
        self.buf = self.buf[:, drop * self.hop:].contiguous()
        self.next = nxt - drop

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        """End of the stream: the frames still owed, with the reference's zero padding behind the last sample."""
        if self.buf is None:
            return torch.empty((0, self.F, 0), device="cuda")
        last = (self.buf.shape[1] - 1) // self.hop                        # frames of a clip of this length: floor((T - 1) / hop) + 1
        out = self._emit(self.next, last) if last >= self.next else self.buf.new_empty((self.buf.shape[0], self.F, 0), dtype=torch.float32)
        self.buf = self.state = None
        self.next = 0
        self.started = False
        return out


class _FusedLeafStream(LeafStream):
    """``LeafStream(leaf, fused=True)``: every step is one ``leaf_stream_step_f32`` launch per piece of the chunk (a chunk beyond
    the kernel's one-pass capacity goes in pieces).  The host keeps where the stream stands -- ``hist_len``, ``next``, ``parity``,
    ``started`` -- and ``stream_plan`` moves it; the device buffer ``state_buf`` is allocated by the first step and kept.
    Inherited from the two-launch class and NOT used here: ``buf`` and ``state`` (they stay None: history and smoother live in
    ``state_buf``), ``_pooled``, ``_emit`` and ``_advance``; the geometry (``K`` .. ``reach``), ``log1p``, ``next`` and ``started`` are."""

    def __init__(self, leaf, log1p: bool = False, fused: bool = True, out_dtype=None):
        super().__init__(leaf, log1p, True, out_dtype)
        if _native.load().leaf_stream_state_bytes(1, self.F, self.K, self.hop, 0) == 0:
            raise ValueError(f"LeafStream(fused=True): no one-launch streaming kernel for window {self.K} / hop {self.hop} "
                             "(16 kHz and 8 kHz geometries: 401 / 160, 201 / 80); use fused=False")
        c = leaf._compression
        if c is not None and c._floor != 1e-12:
            raise NotImplementedError("fused path is specialised for the PCEN floor Leaf constructs (1e-12)")
        self.out_dtype = torch.bfloat16 if out_dtype is torch.bfloat16 else torch.float32
        self.capacity = stream_capacity(self.K, self.hop)
        self.state_buf: Optional[torch.Tensor] = None                     # [history half 0 | history half 1 | smoother], never cleared
        self.state_key = None                                             # (B, int16?, device) the buffer was sized for
        self.pcm: Optional[bool] = None                                   # sample type of the running stream
        self.hist_len = 0
        self.parity = 0

    def _launch(self, x2: Optional[torch.Tensor], at: int, Tc: int, final: bool) -> torch.Tensor:
        B, pcm, dev = self.state_key
        first, n, drop, new_hist, new_next = stream_plan(self.hist_len, self.next, Tc, self.K, self.hop, final)
        params, flags = _native._gather(dev, self.leaf._kernel_params(), self.leaf._compression is not None, self.log1p)
        flags |= (_native.FLAG_X_PCM16 if pcm else 0) | (_native.FLAG_OUT_BF16 if self.out_dtype is torch.bfloat16 else 0)
        out = torch.empty((B, self.F, n), dtype=self.out_dtype, device=dev)
        _native.stream_step(x2.data_ptr() + at * x2.element_size() if Tc else 0, B, Tc, x2.stride(0) if Tc else 0, self.state_buf,
                            self.hist_len, self.parity, drop, first, n, self.started, params, self.F, self.K, self.hop, flags,
                            out.data_ptr() if n else 0, dev)
        self.hist_len, self.next, self.parity = new_hist, new_next, self.parity ^ 1
        self.started = self.started or n > 0
        return out

    @torch.no_grad()
    def step(self, chunk: torch.Tensor) -> torch.Tensor:
        """As ``LeafStream.step``; the frames are ``out_dtype``.  ``chunk`` may be a view into a longer recording
        (``x[:, :, a:b]``): its row stride is passed down, nothing is copied."""
        pcm = chunk.dtype == torch.int16
        if self.pcm is not None and pcm != self.pcm:
            raise RuntimeError(f"LeafStream.step: this stream holds {'int16 PCM' if self.pcm else 'float32'} "
                               f"samples and got a {chunk.dtype} chunk: one sample type per stream (flush() ends it)")
        _native.require_hip(chunk, "LeafStream.step")
        x2 = chunk[:, 0, :] if chunk.dim() == 3 else chunk
        x2 = x2 if pcm else x2.float()
        B, Tc = x2.shape
        if (Tc > 1 and x2.stride(1) != 1) or (Tc >= 1 and B > 1 and x2.stride(0) < Tc):     # (an expanded view: rows overlap)
            x2 = x2.contiguous()
        if self.pcm is None:                                              # a stream begins
            key = (B, pcm, x2.device)
            if self.state_key != key:
                self.state_buf = _native.stream_state(B, self.F, self.K, self.hop, _native.FLAG_X_PCM16 if pcm else 0, x2.device)
                self.state_key = key
            self.pcm = pcm
        elif (B, x2.device) != (self.state_key[0], self.state_key[2]):
            raise RuntimeError(f"LeafStream.step: this stream runs {self.state_key[0]} waveforms on {self.state_key[2]} and got "
                               f"{B} on {x2.device} (flush() ends it)")
        outs, at = [], 0
        while at < Tc:                                                    # one piece unless the chunk exceeds the kernel's one pass
            take = min(Tc - at, self.capacity - self.hist_len)
            outs.append(self._launch(x2, at, take, False))
            at += take
        if not outs:
            return x2.new_empty((B, self.F, 0), dtype=self.out_dtype)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=2)

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        """As ``LeafStream.flush``: one final step without samples.  The state buffer is kept for the next stream as it is."""
        if self.pcm is None:
            return torch.empty((0, self.F, 0), device="cuda")
        out = self._launch(None, 0, 0, True)
        self.pcm = None
        self.hist_len = self.next = 0
        self.started = False
        return out


class LeafStreamBank:
    """``slots`` INDEPENDENT streams served by one ``leaf_stream_bank_step_f32`` call per step (csrc/leaf_fft_stream.hpp: the fused
    stream's kernel with the position taken per slot).  Streams begin and end at different times, take chunks of different lengths,
    or take nothing in a step: what a server with many connections needs, where ``LeafStream(fused=True)`` moves a batch in lock-step.

    The host keeps, per slot, what ``_FusedLeafStream`` keeps for its batch -- ``hist_len``, ``next``, ``parity``, ``started`` -- and
    ``stream_plan`` moves it; the device buffer (``state_buf``: ``leaf_stream_state_bytes`` for ``slots`` rows) is allocated by the
    first step and never cleared.  Every stream's frames are, bit for bit, those of a one-waveform ``LeafStream(leaf, fused=True)`` fed
    the same chunks and flushed."""

    def __init__(self, leaf, slots: int, sample_dtype=torch.float32, log1p: bool = False, out_dtype=None, device=None):
        if out_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f"LeafStreamBank: out_dtype must be None, torch.float32 or torch.bfloat16, got {out_dtype!r}")
        if sample_dtype not in (torch.float32, torch.int16):
            raise ValueError(f"LeafStreamBank: sample_dtype must be torch.float32 or torch.int16 (16-bit PCM), got {sample_dtype!r}")
        if int(slots) < 1:
            raise ValueError(f"LeafStreamBank: slots must be at least 1, got {slots!r}")
        conv, pool = leaf._complex_conv, leaf._pooling
        self.leaf = leaf
        self.slots = int(slots)
        self.K, self.hop, self.F = conv._kernel_size, pool.strides, conv._filters
        self.pcm = sample_dtype is torch.int16                            # fixed for the bank's life: the state layout depends on it
        self.sample_dtype = sample_dtype
        if _native.load().leaf_stream_state_bytes(self.slots, self.F, self.K, self.hop, 0) == 0:
            raise ValueError(f"LeafStreamBank: no one-launch streaming kernel for window {self.K} / hop {self.hop} "
                             "(16 kHz and 8 kHz geometries: 401 / 160, 201 / 80)")
        c = leaf._compression
        if c is not None and c._floor != 1e-12:
            raise NotImplementedError("fused path is specialised for the PCEN floor Leaf constructs (1e-12)")
        self.log1p = bool(log1p) or bool(getattr(leaf, "_log1p", False))
        self.out_dtype = torch.bfloat16 if out_dtype is torch.bfloat16 else torch.float32
        self.max_chunk = stream_capacity(self.K, self.hop) - _native.load().leaf_stream_history_samples(self.K, self.hop)
        self.device = None if device is None else torch.device(device)
        self.state_buf: Optional[torch.Tensor] = None                     # [history half 0 | history half 1 | smoother], never cleared
        self.running = [False] * self.slots
        self.hist_len = [0] * self.slots
        self.next = [0] * self.slots
        self.parity = [0] * self.slots
        self.started = [False] * self.slots

    def _plan(self, lengths, end):
        """The host side of a step, on integers alone: moves every slot's position through ``stream_plan`` and returns
        (the slots' ``_native.StreamSlot`` records, the frames each slot emits)."""
        B = self.slots
        lengths = [int(v) for v in lengths]
        end = [False] * B if end is None else [bool(v) for v in end]
        if len(lengths) != B or len(end) != B:
            raise ValueError(f"LeafStreamBank.step: lengths and end must have one entry per slot ({B})")
        for b, Tc in enumerate(lengths):
            if not 0 <= Tc <= self.max_chunk:
                raise ValueError(f"LeafStreamBank.step: lengths[{b}] = {Tc} is outside 0 .. max_chunk = {self.max_chunk}")
        recs, counts = (_native.StreamSlot * B)(), [0] * B
        for b in range(B):
            Tc, r = lengths[b], recs[b]
            if Tc == 0 and not (end[b] and self.running[b]):              # idle, or `end` on a slot that is not running
                r.idle = 1
                continue
            if not self.running[b]:                                       # a stream begins: nothing of the state is read
                self.running[b], self.hist_len[b], self.next[b], self.started[b] = True, 0, 0, False
            hist, T = self.hist_len[b], self.hist_len[b] + Tc
            r.hist_len, r.Tc, r.parity, r.started = hist, Tc, self.parity[b], int(self.started[b])
            first, n, drop, hist2, next2 = stream_plan(hist, self.next[b], Tc, self.K, self.hop, False) if Tc else (self.next[b], 0, 0, hist, self.next[b])
            if not end[b]:
                r.first, r.n, r.drop_samples = first, n, drop
                self.hist_len[b], self.next[b] = hist2, next2
            else:
                # the stream ends: what a step and then a flush would emit.  The flush's frames are those of the buffer the step
                # keeps, [drop, T); where the step itself emits nothing that is the whole buffer, and one pass serves
                first2, n2, _, _, _ = stream_plan(hist2, next2, 0, self.K, self.hop, True)
                if n == 0:
                    r.first, r.n, r.drop_samples = first2, n2, T
                else:
                    r.first, r.n, r.drop_samples, r.end_first, r.end_n = first, n, drop, first2, n2
                n += n2
                self.running[b], self.hist_len[b], self.next[b] = False, 0, 0
            counts[b] = n
            self.started[b] = (self.started[b] or n > 0) and self.running[b]
            self.parity[b] ^= 1
        return recs, counts

    @torch.no_grad()
    def step(self, chunk: Optional[torch.Tensor], lengths, end=None):
        """One step of every slot.  ``chunk``: (slots,1,Tmax) or (slots,Tmax) on the device, ``sample_dtype`` samples; a strided view
        is read in place, and only ``chunk[b, :lengths[b]]`` is ever read (None: no slot has samples).  ``lengths``: per slot, host
        integers in 0 .. min(Tmax, max_chunk).  ``end``: per slot, host booleans -- the slot's stream ends with this chunk, its
        remaining frames come out in this step with the reference's zero padding behind the last sample, and the slot is free.  A
        slot that is not running begins a new stream with its first samples; no samples and no ``end`` leaves a slot idle (its state
        is not touched); ``end`` on a slot that is not running does nothing.  Returns ``(frames, counts)``: ``frames`` is
        (slots, F, max(counts)) in ``out_dtype``, row b holding ``counts[b]`` frames and zeros behind them; ``counts`` is computed on
        the host, nothing synchronises."""
        B = self.slots
        for b, Tc in enumerate(lengths):                                  # before anything else: nothing is launched, no state moves
            if int(Tc) > self.max_chunk:
                raise ValueError(f"LeafStreamBank.step: lengths[{b}] = {int(Tc)} is outside 0 .. max_chunk = {self.max_chunk}")
        x2 = None
        if chunk is not None:
            _native.require_hip(chunk, "LeafStreamBank.step")
            if chunk.dtype != self.sample_dtype:
                raise ValueError(f"LeafStreamBank.step: this bank takes {self.sample_dtype} samples and got a {chunk.dtype} chunk")
            x2 = chunk[:, 0, :] if chunk.dim() == 3 else chunk
            if x2.dim() != 2 or x2.shape[0] != B:
                raise ValueError(f"LeafStreamBank.step: chunk must be ({B},1,Tmax) or ({B},Tmax), got {tuple(chunk.shape)}")
            if self.device is not None and x2.device != self.device:
                raise ValueError(f"LeafStreamBank.step: this bank lives on {self.device} and got a chunk on {x2.device}")
        Tmax = 0 if x2 is None else x2.shape[1]
        for b, Tc in enumerate(lengths):
            if int(Tc) > Tmax:
                raise ValueError(f"LeafStreamBank.step: lengths[{b}] = {int(Tc)} exceeds the chunk's {Tmax} samples")
        if self.device is None:
            if x2 is None:
                return torch.empty((B, self.F, 0), dtype=self.out_dtype), [0] * B   # (nothing has ever run)
            self.device = x2.device
        if x2 is not None and ((Tmax > 1 and x2.stride(1) != 1) or (B > 1 and x2.stride(0) < Tmax)):    # (an expanded view: rows overlap)
            x2 = x2.contiguous()
        recs, counts = self._plan(lengths, end)
        dev, n_max = self.device, max(counts)
        if self.state_buf is None:
            self.state_buf = _native.stream_state(B, self.F, self.K, self.hop, _native.FLAG_X_PCM16 if self.pcm else 0, dev)
        params, flags = _native._gather(dev, self.leaf._kernel_params(), self.leaf._compression is not None, self.log1p)
        flags |= (_native.FLAG_X_PCM16 if self.pcm else 0) | (_native.FLAG_OUT_BF16 if self.out_dtype is torch.bfloat16 else 0)
        out = torch.empty((B, self.F, n_max), dtype=self.out_dtype, device=dev)
        _native.stream_bank_step(x2.data_ptr() if Tmax else 0, x2.stride(0) if Tmax else 0, recs, n_max, self.state_buf, params,
                                 self.F, self.K, self.hop, flags, out.data_ptr() if n_max else 0, dev)
        return out, counts

    def flush(self, slots=None):
        """A step without samples that ends the named slots (all running slots by default): ``(frames, counts)`` as ``step``."""
        ending = range(self.slots) if slots is None else [int(b) for b in slots]
        end = [False] * self.slots
        for b in ending:
            end[b] = True
        return self.step(None, [0] * self.slots, end)


_SAMPLE_DTYPES = (torch.float32, torch.int16)


class ResampleStreamBank:
    """``slots`` INDEPENDENT streams at a device rate (44.1 or 48 kHz) brought to ``new_freq`` chunk by chunk, one
    ``leaf_resample_stream_step_f32`` call per step for the whole bank: what stands between a microphone and ``LeafStreamBank``.
    Streams begin and end at different steps, take chunks of different lengths, or take nothing in a step.

    Every output of ``resample()`` is one fma chain over its span, a pure function of the recording; so what a slot emits over its
    stream's life, concatenated, is BIT FOR BIT ``resample()`` of the concatenated chunks, for any chunking.  An output leaves in the
    step that brings its last sample.  The host keeps where each slot stands (``pos``: ``_native.ResamplePos``, moved by
    ``leaf_resample_stream_plan``, integers alone); the history the next outputs need (at most ``history`` = K - 1 samples per slot:
    474 at 44.1 -> 16 kHz, 40 at 48 -> 16 kHz) lives in ``state_buf``, allocated by the first step and never cleared.

    ``max_chunk`` (2^20 samples) is the most one slot takes in one step.  Ratios whose tile window does not fit LDS (16 -> 1,
    44100 -> 2000) are not served: ``ValueError``."""

    def __init__(self, orig_freq: int, new_freq: int, slots: int, sample_dtype=torch.float32, out_dtype=None,
                 lowpass_filter_width: int = 6, rolloff: float = 0.99, device=None):
        if sample_dtype not in _SAMPLE_DTYPES:
            raise ValueError(f"ResampleStreamBank: sample_dtype must be torch.float32 or torch.int16 (16-bit PCM), got {sample_dtype!r}")
        if out_dtype not in (None,) + _SAMPLE_DTYPES:
            raise ValueError(f"ResampleStreamBank: out_dtype must be None, torch.float32 or torch.int16, got {out_dtype!r}")
        if isinstance(slots, bool) or int(slots) != slots or int(slots) < 1:
            raise ValueError(f"ResampleStreamBank: slots must be an integer of at least 1, got {slots!r}")
        self.key = _native._resample_params(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.table = _native.resample_table(*self.key)                    # (ValueError for a ratio beyond the library)
        self.slots = int(slots)
        self.sample_dtype = sample_dtype
        self.out_dtype = sample_dtype if out_dtype is None else out_dtype
        self.flags = (_native.FLAG_X_PCM16 if sample_dtype is torch.int16 else 0) | (_native.FLAG_OUT_PCM16 if self.out_dtype is torch.int16 else 0)
        if _native.load().leaf_resample_stream_state_bytes(self.slots, *self.key, self.flags) == 0:
            raise ValueError(f"ResampleStreamBank: {self.key[0]} -> {self.key[1]} is not served in chunks: a tile's input window "
                             "does not fit LDS (resample() takes whole recordings at this ratio)")
        self.history = _native.resample_stream_history(self.key)
        self.max_chunk = _native.RESAMPLE_STREAM_MAX_CHUNK
        self.device = None if device is None else torch.device(device)
        self.state_buf: Optional[torch.Tensor] = None                     # [history half 0 | history half 1], never cleared
        self.pos = (_native.ResamplePos * self.slots)()

    @property
    def running(self):
        return [bool(p.running) for p in self.pos]

    @torch.no_grad()
    def step(self, chunk: Optional[torch.Tensor], lengths, end=None):
        """One step of every slot.  ``chunk``: (slots,1,Tmax) or (slots,Tmax) on the device, ``sample_dtype`` samples; a strided view
        is read in place, and only ``chunk[b, :lengths[b]]`` is ever read (None: no slot has samples).  ``lengths``: per slot, host
        integers in 0 .. min(Tmax, max_chunk).  ``end``: per slot, host booleans -- the slot's stream ends with this chunk, every
        remaining output of its recording comes out in this step (zeros behind the last sample) and the slot is free.  A slot that is
        not running begins a new stream with its first samples; no samples and no ``end`` leaves a slot idle (its state is not
        touched); ``end`` on a slot that is not running does nothing.  Returns ``(y, counts)``: ``y`` is (slots, max(counts)) in
        ``out_dtype``, row b holding ``counts[b]`` samples and zeros behind them; ``counts`` are host integers, nothing synchronises.
        ``ValueError`` for bad lengths or a chunk of another type or shape: nothing is launched and no position moves."""
        B = self.slots
        lengths = [int(v) for v in lengths]
        end = [False] * B if end is None else [bool(v) for v in end]
        if len(lengths) != B or len(end) != B:
            raise ValueError(f"ResampleStreamBank.step: lengths and end must have one entry per slot ({B})")
        for b, Tc in enumerate(lengths):
            if not 0 <= Tc <= self.max_chunk:
                raise ValueError(f"ResampleStreamBank.step: lengths[{b}] = {Tc} is outside 0 .. max_chunk = {self.max_chunk}")
        x2 = None
        if chunk is not None:
            if chunk.dtype != self.sample_dtype:
                raise ValueError(f"ResampleStreamBank.step: this bank takes {self.sample_dtype} samples and got a {chunk.dtype} chunk")
            x2 = chunk[:, 0, :] if chunk.dim() == 3 and chunk.shape[1] == 1 else chunk
            if x2.dim() != 2 or x2.shape[0] != B:
                raise ValueError(f"ResampleStreamBank.step: chunk must be ({B},1,Tmax) or ({B},Tmax), got {tuple(chunk.shape)}")
            _native.require_hip(chunk, "ResampleStreamBank.step")
            if self.device is not None and x2.device != self.device:
                raise ValueError(f"ResampleStreamBank.step: this bank lives on {self.device} and got a chunk on {x2.device}")
        Tmax = 0 if x2 is None else x2.shape[1]
        for b, Tc in enumerate(lengths):
            if Tc > Tmax:
                raise ValueError(f"ResampleStreamBank.step: lengths[{b}] = {Tc} exceeds the chunk's {Tmax} samples")
        if self.device is None:
            if x2 is None:
                return torch.empty((B, 0), dtype=self.out_dtype), [0] * B   # (nothing has ever run)
            self.device = x2.device
        if x2 is not None and ((Tmax > 1 and x2.stride(1) != 1) or (B > 1 and x2.stride(0) < Tmax)):    # (an expanded view: rows overlap)
            x2 = x2.contiguous()
        pos = (_native.ResamplePos * B).from_buffer_copy(self.pos)        # the plan moves a copy: a refusal leaves the bank as it was
        recs, counts = _native.resample_stream_plan(self.key, pos, lengths, end)
        dev, n_max = self.device, max(counts)
        if self.state_buf is None:
            self.state_buf = _native.resample_stream_state(B, self.key, self.flags, dev)
        out = torch.empty((B, n_max), dtype=self.out_dtype, device=dev)
        _native.resample_stream_step(x2.data_ptr() if Tmax else 0, x2.stride(0) if Tmax else 0, recs, n_max, self.state_buf, self.flags,
                                     self.key, self.table, out.data_ptr() if n_max else 0, dev)
        self.pos = pos
        return out, counts

    def flush(self, slots=None):
        """A step without samples that ends the named slots (all running slots by default): ``(y, counts)`` as ``step``."""
        ending = range(self.slots) if slots is None else [int(b) for b in slots]
        end = [False] * self.slots
        for b in ending:
            end[b] = True
        return self.step(None, [0] * self.slots, end)


class ResampleStream:
    """``ResampleStream(orig_freq, new_freq)``: B waveforms in lock-step through ``ResampleStreamBank``'s machinery.  ``step(chunk)``
    returns the outputs that became final, ``flush()`` ends the stream with the rest: concatenated they are ``resample()`` of the
    concatenated chunks, bit for bit.  The sample dtype (float32 or int16) and the batch are those of the first chunk; ``out_dtype=None``
    keeps the sample dtype.  A chunk beyond ``max_chunk`` samples (2^20) goes in pieces."""

    def __init__(self, orig_freq: int, new_freq: int, out_dtype=None, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        if out_dtype not in (None,) + _SAMPLE_DTYPES:
            raise ValueError(f"ResampleStream: out_dtype must be None, torch.float32 or torch.int16, got {out_dtype!r}")
        self.key = _native._resample_params(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.out_dtype = out_dtype
        self.table = _native.resample_table(*self.key)
        if _native.load().leaf_resample_stream_state_bytes(1, *self.key, 0) == 0:
            raise ValueError(f"ResampleStream: {self.key[0]} -> {self.key[1]} is not served in chunks: a tile's input window does not "
                             "fit LDS (resample() takes whole recordings at this ratio)")
        self.max_chunk = _native.RESAMPLE_STREAM_MAX_CHUNK
        self.bank: Optional[ResampleStreamBank] = None                    # made by the first chunk, kept for the next stream
        self.open = False                                                 # a stream is running

    def _rows(self, chunk: torch.Tensor) -> torch.Tensor:
        if not isinstance(chunk, torch.Tensor) or chunk.dtype not in _SAMPLE_DTYPES:
            raise ValueError(f"ResampleStream.step: chunks are float32 or int16 (PCM) tensors, got {getattr(chunk, 'dtype', type(chunk))!r}")
        x2 = chunk[:, 0, :] if chunk.dim() == 3 and chunk.shape[1] == 1 else chunk
        if x2.dim() != 2 or x2.shape[0] < 1:
            raise ValueError(f"ResampleStream.step: chunk must be (B,1,Tc) or (B,Tc) with B >= 1, got {tuple(chunk.shape)}")
        return x2

    @torch.no_grad()
    def step(self, chunk: torch.Tensor) -> torch.Tensor:
        """chunk (B,1,Tc) or (B,Tc) on the device, float32 or int16; a strided view is read in place -> (B, n), n >= 0."""
        x2 = self._rows(chunk)
        _native.require_hip(chunk, "ResampleStream.step")
        B, Tc = x2.shape
        bank = self.bank
        if self.open:
            if x2.dtype != bank.sample_dtype:
                raise RuntimeError(f"ResampleStream.step: this stream holds {bank.sample_dtype} samples and got a {x2.dtype} chunk: "
                                   "one sample type per stream (flush() ends it)")
            if (B, x2.device) != (bank.slots, bank.device):
                raise RuntimeError(f"ResampleStream.step: this stream runs {bank.slots} waveforms on {bank.device} and got {B} on "
                                   f"{x2.device} (flush() ends it)")
        elif bank is None or (bank.slots, bank.sample_dtype, bank.device) != (B, x2.dtype, x2.device):
            bank = self.bank = ResampleStreamBank(self.key[0], self.key[1], B, x2.dtype, self.out_dtype, self.key[2], self.key[3], x2.device)
            bank.table = self.table                                       # (a test switch: ResampleTable.with_global_taps)
        outs, at = [], 0
        while at < Tc:                                                    # one piece unless the chunk exceeds max_chunk
            take = min(Tc - at, self.max_chunk)
            y, _ = bank.step(x2[:, at:at + take], [take] * B)
            self.open = True
            outs.append(y)
            at += take
        if not outs:
            return x2.new_empty((B, 0), dtype=bank.out_dtype)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        """End of the stream: the outputs still owed, with zeros behind the last sample.  The state buffer is kept."""
        if not self.open:
            if self.bank is None:
                return torch.empty((0, 0), dtype=self.out_dtype or torch.float32)
            return torch.empty((self.bank.slots, 0), dtype=self.bank.out_dtype, device=self.bank.device)
        y, _ = self.bank.flush()
        self.open = False
        return y
