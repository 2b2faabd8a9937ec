#!/usr/bin/env python
"""Timing of PackedClips.resampled (leaf_resample_f32) against the stock composition and against a copy of the same bytes.

    python tools/bench_resample.py --out profiles/resample.txt

The sides take turns in one process, per shape, timed with device events around one call each; the median over the rounds counts:
  (a) PackedClips.resampled on R recordings of S seconds, int16 and float32 stores, output in the source dtype; (a') is the
      leaf_resample_f32 call alone, into a preallocated output with the plan on the device already -- (a) without the new store's
      allocation and the upload of its offsets and lengths;
  (b) the stock composition on a float32 copy of the store (made once, not timed): per recording F.pad and F.conv1d(stride=o) with the
      dense (n, 1, 2 width + o) kernels, transpose, crop; then cat.  Its result is first checked against a float64 evaluation of
      the same convolution inside the bound the tests use, (cnt + 2) 2^-24 sum |h| |x| + 2^-149 -- and so is (a)'s;
  (c) copy_ of a buffer of (in bytes + out bytes) / 2: it reads that much and writes that much, the HBM traffic of (a).
Reported: time per call, (in bytes + out bytes) / time, and that rate as a share of (c)'s."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leaf_pytorch_amd import PackedClips, _native  # noqa: E402

DEV = "cuda:0"
RATIOS = [(44100, 16000), (48000, 16000), (16000, 8000), (44100, 48000)]


def dense_kernels(tab, dtype) -> torch.Tensor:
    """(n, 1, 2 width + o): row p holds the span's taps at k0[p] .. and zeros elsewhere."""
    K = 2 * tab.width + tab.o
    w = torch.zeros(tab.n, K, dtype=torch.float32)
    for p in range(tab.n):
        k0, cnt = int(tab.k0[p]), int(tab.cnt[p])
        w[p, k0: k0 + cnt] = tab.taps[p, :cnt]
    return w.to(dtype)[:, None, :].to(DEV)


def stock_one(x: torch.Tensor, w: torch.Tensor, tab, out_len: int) -> torch.Tensor:
    y = F.conv1d(F.pad(x[None, None], (tab.width, tab.width + tab.o)), w, stride=tab.o)
    return y[0].transpose(0, 1).reshape(-1)[:out_len]


def stock(store32: torch.Tensor, offsets, lengths, out_lengths, w, tab) -> torch.Tensor:
    return torch.cat([stock_one(store32[o: o + L], w, tab, n) for o, L, n in zip(offsets, lengths, out_lengths)])


def check(store32, offsets, lengths, out_lengths, tab, got_a, got_b, lines):
    """(a) and (b) on the first recording against the float64 convolution, in units of the bound."""
    o, L, n = offsets[0], lengths[0], out_lengths[0]
    x = store32[o: o + L].double()
    w64, wabs = dense_kernels(tab, torch.float64), dense_kernels(tab, torch.float64).abs()
    want = stock_one(x, w64, tab, n)
    cnt = tab.cnt.to(DEV).double().repeat((n + tab.n - 1) // tab.n)[:n]
    bound = (cnt + 2) * 2.0 ** -24 * stock_one(x.abs(), wabs, tab, n) + 2.0 ** -149
    for name, got in (("(a)", got_a[:n]), ("(b)", got_b[:n])):
        worst = float(((got.double() - want).abs() / bound).max())
        lines.append(f"    check {name}: worst error {worst:.3f} of the bound over {n} outputs -> {'ok' if worst <= 1.0 else 'OUTSIDE'}")
        assert worst <= 1.0, (name, worst)


def timed(fn, ev):
    ev[0].record()
    out = fn()
    ev[1].record()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--recordings", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=12)
    args = ap.parse_args()
    assert args.rounds >= 10
    _native.load()
    props = torch.cuda.get_device_properties(DEV)
    lines = [f"# tools/bench_resample.py on {props.name} ({props.multi_processor_count} CUs): {args.recordings} recordings of {args.seconds:g} s, "
             f"median of {args.rounds} rounds, device events around one call, the sides taking turns",
             "# rate = (in bytes + out bytes) / time; share = that rate over the copy's"]
    g = torch.Generator().manual_seed(0)
    for orig, new in RATIOS:
        tab = _native.resample_table(orig, new)
        L = int(args.seconds * orig)
        lengths = [L] * args.recordings
        offsets = [i * L for i in range(args.recordings)]
        out_lengths = [_native.resample_length(L, orig, new)] * args.recordings
        w = dense_kernels(tab, torch.float32)
        pcm = torch.randint(-32768, 32768, (L * args.recordings,), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
        lines.append(f"{orig} -> {new} Hz (o = {tab.o}, n = {tab.n}, width = {tab.width}, {int(tab.cnt.min())}-{int(tab.cnt.max())} taps per output, "
                     f"taps in {'LDS' if tab.taps_in_lds else 'global memory'})")
        for dtype in (torch.int16, torch.float32):
            store = pcm if dtype == torch.int16 else pcm.float() / 32768.0
            store32 = store if dtype == torch.float32 else pcm.float() / 32768.0
            clips = PackedClips.from_store(store, offsets, lengths)
            item = store.element_size()
            nbytes = item * (store.numel() + sum(out_lengths))
            buf, dst = (torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV) for _ in range(2))
            out = torch.empty(sum(out_lengths), dtype=dtype, device=DEV)
            out_off = torch.tensor([i * out_lengths[0] for i in range(args.recordings)], dtype=torch.int64, device=DEV)
            sides = {"(a) resampled": lambda: clips.resampled(orig, new),
                     "(a') the call alone": lambda: _native.resample_records(store, clips.offsets, clips.lengths, orig, new, out, out_off),
                     "(b) stock conv1d": lambda: stock(store32, offsets, lengths, out_lengths, w, tab),
                     "(c) copy_": lambda: dst.copy_(buf)}
            got_a = clips.resampled(orig, new, out_dtype=torch.float32).store
            got_b = stock(store32, offsets, lengths, out_lengths, w, tab)
            if dtype == torch.int16:
                check(store32, offsets, lengths, out_lengths, tab, got_a, got_b, lines)
            del got_a, got_b
            for fn in sides.values():                                           # warm-up per shape
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in sides}
            for _ in range(args.rounds):
                evs = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in sides}
                for k, fn in sides.items():
                    timed(fn, evs[k])
                torch.cuda.synchronize()
                for k in sides:
                    times[k].append(evs[k][0].elapsed_time(evs[k][1]) * 1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            copy_rate = nbytes / med["(c) copy_"]
            for k in sides:
                rate = nbytes / med[k]
                lines.append(f"  {str(dtype).replace('torch.', ''):8s} {k:20s} {med[k]:10.1f} us  (min {min(times[k]):.1f}, max {max(times[k]):.1f})  "
                             f"{rate / 1e6:7.3f} TB/s  {rate / copy_rate:6.3f} of the copy  [{nbytes / 2 ** 20:.0f} MiB]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
