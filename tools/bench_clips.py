#!/usr/bin/env python3
"""Time of assembling one training batch from a device-resident packed store: ONE leaf_assemble_clips_f32 launch
(PackedClips / _native.assemble_clips) against the stock-op composition of the same batch -- index gather, .float() / 32768,
multiply by the gain, transforms.PeakNormalization, one masked_fill per span.

    python tools/bench_clips.py [--rounds 20] [--steps 50] [--out profiles/clip_assembly.txt]
    python tools/bench_clips.py --noise [--out profiles/clip_noise.txt]
    python tools/bench_clips.py --segments [--out profiles/eval_segments.txt]
    python tools/bench_clips.py --standardize [--out profiles/clip_standardize.txt]
    python tools/bench_clips.py --device-draws [--out profiles/clip_device_draws.txt]
    python tools/bench_clips.py --device-mixup [--out profiles/clip_device_mixup.txt]
    python tools/bench_clips.py --effects [--out profiles/clip_effects.txt]

Both sides run in ONE process on the same store and the same plan (already on the device: drawing it is not timed), taking turns
round after round after a warm-up round, the order alternating.  Every recording is longer than the clip, so the batch is a crop
and the stock side needs no padding (ragged padding has no batched stock op: that side would be a Python loop over the clips).
Before anything is timed the two sides' batches are compared bit for bit.  Two figures per side and shape, each the median [min, max]
over the rounds of (time of `steps` calls) / steps:
  wall    host clock from the first call to the end of a device synchronisation behind the last: what a training loop sees (the
          Python layer's checks and the launch included; for a small batch this is the host's time, not the device's)
  device  HIP events around the same calls, ENQUEUED WHILE THE DEVICE IS KEPT BUSY by a matrix product queued in front, so that the
          calls run back to back from a full queue: the device's own time per call, launch gaps between kernels included, the
          host's enqueue time excluded
and for the kernel the achieved bytes per second: (B * S samples of the store read + 4 * B * S bytes written) / median device time.
B = 64 / 256 clips of 16 000 and 80 000 samples (80 000 is beyond the resident path: the clip is gathered twice), int16 and float32
stores.  No assertion on any time; prints the table and, with --out, writes it.

--noise times the launch with background noise at an SNR and Gaussian noise in it (leaf_assemble_clips_noise_f32) instead: B = 64 /
256 clips of 16 000 samples, both stores, every clip mixed and every amplitude non-zero.  Its stock side is the composition a user
would write without the entry: index gather of the clip and of the noise, .float() / 32768, the multiply-add of the mix, multiply by
the gain, torch.randn scaled and added, transforms.PeakNormalization, one masked_fill per span.  torch.randn is not the library's
stream, so the two sides are NOT compared bit for bit here (tests/test_gpu_clip_noise.py does that, on the library's own z); the
stock side is checked against the kernel with the Gaussian amplitude at 0 instead.  A third column times the plain launch
(leaf_assemble_clips_f32, the same clip plan without noise) in the same rounds: the cost of the augmented launch relative to it.

--segments times the evaluation batch of whole recordings (leaf_assemble_segments_f32): 16 and 64 recordings of 1 - 10.3 s at 16 kHz cut
into one-second rows the way the reference's test.py cuts them, both stores.  Three sides take turns: `kernel`, the one launch with its
row plan already on the device; `segments`, PackedClips.segments as a user calls it (the plan made on the host from lengths_host and
copied over: wall time only, its copies wait for the device); and `stock`, the reference loop restated in stock ops on the device --
per recording transforms.PeakNormalization over the whole recording, F.pad(..., 'replicate'), reshape; then torch.cat.  The two
batches are compared bit for bit before anything is timed.  The one-time PackedClips.peaks() launch (leaf_clip_peaks_f32 over the
whole store; float32 stores only use it) is timed on its own, in rounds of its own, and reported in its own column.

--standardize times the launch on the standardised recordings (leaf_assemble_clips_std_f32: audio_config.normalize in the launch): B =
64 / 256 clips of 16 000 and B = 256 of 80 000 samples, both stores.  Three sides take turns: `std`, the standardising launch; `plain`,
leaf_assemble_clips_f32 on the same plan (what the keyword costs, and whether the plain launch is what it was); `stock`, what a user
without the entry keeps -- a float32 copy of the whole store standardised per recording by the reference's expression (made once on
the CPU from the library's moments, not timed) -- through the stock chain of the first table.  The std and stock batches are compared
bit for bit before anything is timed.  The one-time PackedClips.moments() call (leaf_clip_moments_f32) is timed in rounds of its own.

--device-draws times a training step's batch INCLUDING its random draws: B = 64 / 256 clips of 16 000 samples, both stores, three time
masks and background noise on.  Five sides take turns: `host`, ClipSampler.__call__ with a CPU index (the draws on the CPU from a
torch.Generator, the plan uploaded: the path as it was, the baseline); `device`, DeviceClipSampler.__call__ (leaf_draw_clip_plan, then
the assembling launch on its static buffers); `graph`, the replay of that pair captured with torch.cuda.graph; and, for the device
time of each launch on its own, `plan` (DeviceClipSampler.plan alone) and `assemble` (_native.assemble_clips on the static plan).  A
round is --steps calls (default here: 40) and one synchronisation, so `wall` is the host time per call of a loop that synchronises
every 40 calls.  Before anything is timed the replayed batch is compared bit for bit with the eager batch of a second sampler of the
same seed at the same step.  The last column is the verdict the comparison is made for: `device` wall must not exceed `host` wall by
more than the run-to-run spread of `host` (max - min of its rounds' wall times, measured here, not fixed).

--device-mixup times mixup's draws: B = 64 / 256 / 4096 clips, alpha = 0.3 and 1.  Four sides take turns: `host`, the draws of
transforms.Mixup.__call__ with their upload (numpy's RandomState.beta, torch.randperm on the CPU, two copies to the device: the path as
it was); `device`, DeviceMixup.__call__ (leaf_draw_mixup into the mixer's static buffers); `graph`, the replay of that launch captured
with torch.cuda.graph; and `argsort`, torch.argsort of B 64-bit keys on the device, the stock form of the kernel's sort alone (device
time).  Rounds as for --device-draws.  Before anything is timed the replayed draw is compared bit for bit with the eager draw of a second
mixer of the same seed at the same step, and checked to be a permutation with weights in [0, 1].  No verdict column: the file records
what was measured.

--effects times ClipValue and the reverb (leaf_clip_effects_f32): B = 64 / 256 clips of 16 000 samples at 16 kHz, both stores.  Three
sides take turns: `effects`, EffectsClipSampler.__call__ with a CPU index and every clip clipped and reverberated (its draws on the
host, then assemble, effects, assemble: three launches); `plain`, ClipSampler.__call__ with the same keywords otherwise (one launch);
and `launch`, _native.clip_effects alone on a batch and a plan that are on the device already (its device time is the kernel's).
A round is --steps calls (default here: 20).  Before anything is timed the launch is checked to change every clip and to leave a
batch with an all-skip plan bit for bit alone.  The last line is the sequential definition on the CPU (tools/clip_effects_check.cpp
built with g++ -O2, one core): the per-clip time the reference's "TOO SLOW" is about, for context.  No verdict column."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from leaf_pytorch_amd import PackedClips, PeakNormalization, _native  # noqa: E402

DEV = "cuda:0"
M = 3                                                   # spans per clip, as TimeMasking(num_masks=3)


def make_case(B, S, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(S + 1, 3 * S, (B,), generator=g)
    offsets = torch.cumsum(lengths, 0) - lengths
    n = int(lengths.sum())
    store = (torch.randint(-32768, 32768, (n,), generator=g).to(torch.int16) if dtype == torch.int16
             else torch.rand(n, generator=g) * 2 - 1)
    start = (torch.rand(B, generator=g, dtype=torch.float64) * (lengths - S + 1).double()).long().clamp_(max=lengths - S)
    gain = torch.where(torch.rand(B, generator=g) < 0.5, 10.0 ** ((torch.rand(B, generator=g) * 24 - 18) / 20), torch.ones(B))
    span = (torch.rand(B, M, generator=g) * 0.1 * S).long()
    t0 = (torch.rand(B, M, generator=g) * (S - span)).long()
    plan = dict(rec_off=offsets, rec_len=lengths.to(torch.int32), start=start.to(torch.int32), pad_mode=torch.zeros(B, dtype=torch.int32),
                gain=gain.float(), masks=torch.stack((t0, span), 2).to(torch.int32))
    return store.to(DEV), {k: v.to(DEV) for k, v in plan.items()}


def time_sides(sides, rounds, steps, busy, busy_out):
    """us per call of every side, (device, wall) lists over the rounds: the sides take turns, the order alternating; round 0 warms up."""
    dev_us, wall_us = {k: [] for k in sides}, {k: [] for k in sides}
    for rnd in range(rounds + 1):
        for name in (list(sides) if rnd % 2 == 0 else list(sides)[::-1]):
            fn = sides[name]
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.mm(busy, busy, out=busy_out)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                dev_us[name].append(e0.elapsed_time(e1) * 1e3 / steps)
                wall_us[name].append((t1 - t0) * 1e6 / steps)
    return dev_us, wall_us


def noise_legs(args, busy, busy_out):
    pn = PeakNormalization()
    S = 16000
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {args.steps} calls per side after a "
             "warm-up round; us per call: median [min, max]; device = HIP events, calls queued behind a matrix product; wall = host clock to a "
             "synchronise; noise = leaf_assemble_clips_noise_f32 (background noise + Gaussian noise, every clip), plain = leaf_assemble_clips_f32 "
             "on the same clip plan, stock = gather x 2 + mix + gain + torch.randn + scaled add + PeakNormalization + masked_fill",
             f"{'store':>8} {'B':>4} {'S':>6} | {'noise device':>24} {'noise wall':>11} | {'plain device':>24} | {'stock device':>24} {'stock wall':>11} | "
             f"{'noise / plain':>13} {'stock / noise':>13}"]
    for dtype in (torch.int16, torch.float32):
        for B in (64, 256):
            store, p = make_case(B, S, dtype, seed=B + S)
            nstore, q = make_case(B, S, dtype, seed=B + S + 1)
            g = torch.Generator().manual_seed(B)
            snr = 10.0 + 16.0 * torch.rand(B, generator=g, dtype=torch.float64)
            coeff = _native.noise_coefficients(_native.snr_coefficients(snr)).to(DEV)
            amp = (0.001 + 0.014 * torch.rand(B, generator=g)).to(DEV)
            streams = torch.arange(B, device=DEV)
            noise = (nstore, q["rec_off"], q["rec_len"], q["start"], torch.full((B,), _native.PAD_REPLICATE, dtype=torch.int32, device=DEV), coeff)
            out = torch.empty((B, 1, S), dtype=torch.float32, device=DEV)
            ar = torch.arange(S, device=DEV)
            lo, hi = p["masks"][..., 0].long(), (p["masks"][..., 0] + p["masks"][..., 1]).long()
            first, nfirst = (p["rec_off"] + p["start"])[:, None], (q["rec_off"] + q["start"])[:, None]
            c, cn = coeff[:, :1], coeff[:, 1:]

            def kernel(amp=amp):
                return _native.assemble_clips(store, p["rec_off"], p["rec_len"], p["start"], p["pad_mode"], S, p["gain"], True, p["masks"], out,
                                              noise=noise, gaussian=(amp, 1234, streams))

            def plain():
                return _native.assemble_clips(store, p["rec_off"], p["rec_len"], p["start"], p["pad_mode"], S, p["gain"], True, p["masks"], out)

            def stock(amp=amp):
                x, n = store[first + ar], nstore[nfirst + ar]
                if dtype == torch.int16:
                    x, n = x.float() / 32768, n.float() / 32768
                x = (c * x + cn * n) * p["gain"][:, None]
                x = pn(x + amp[:, None] * torch.randn((B, S), device=DEV))
                for m in range(M):
                    x = x.masked_fill((ar >= lo[:, m, None]) & (ar < hi[:, m, None]), 0.0)
                return x[:, None]

            zero = torch.zeros_like(amp)
            a, b = kernel(zero).clone(), stock(zero)
            torch.cuda.synchronize()
            if not torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32)):
                sys.exit(f"the two sides disagree (Gaussian amplitude 0) at {dtype} B={B}: nothing is timed")
            dev_us, wall_us = time_sides({"noise": kernel, "plain": plain, "stock": stock}, args.rounds, args.steps, busy, busy_out)
            fmt = lambda v: f"{statistics.median(v):9.1f} [{min(v):6.1f},{max(v):7.1f}]"
            med = {k: statistics.median(v) for k, v in dev_us.items()}
            lines.append(f"{str(dtype).replace('torch.', ''):>8} {B:>4} {S:>6} | {fmt(dev_us['noise'])} {statistics.median(wall_us['noise']):11.1f} | "
                         f"{fmt(dev_us['plain'])} | {fmt(dev_us['stock'])} {statistics.median(wall_us['stock']):11.1f} | "
                         f"{med['noise'] / med['plain']:13.2f} {med['stock'] / med['noise']:13.2f}")
            print(lines[-1], flush=True)
    return lines


def segment_legs(args, busy, busy_out):
    pn = PeakNormalization()
    S = 16000
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {args.steps} calls per side after a "
             "warm-up round; us per call: median [min, max]; device = HIP events, calls queued behind a matrix product; wall = host clock to a "
             "synchronise; kernel = leaf_assemble_segments_f32 with the row plan on the device, segments = PackedClips.segments (plan made on the "
             "host and copied), stock = per recording PeakNormalization + F.pad replicate + reshape, then cat; GB/s = (row samples read + 4 bytes "
             "per row sample written) / median device time of the kernel; peaks = the one-time leaf_clip_peaks_f32 call over the whole store",
             f"{'store':>8} {'N':>4} {'rows':>5} | {'kernel device':>24} {'kernel wall':>12} {'GB/s':>7} | {'segments wall':>13} | {'stock device':>26} "
             f"{'stock wall':>11} | {'stock / kernel':>14} | {'peaks device':>24} {'peaks wall':>11}"]
    for dtype in (torch.int16, torch.float32):
        for N in (16, 64):
            g = torch.Generator().manual_seed(N)
            lengths = torch.randint(S, 164801, (N,), generator=g).tolist()                  # 1 s .. 10.3 s
            recs = [(torch.rand(n, generator=g) * 2 - 1) * (1.5 if i % 2 else 0.5) for i, n in enumerate(lengths)]
            if dtype == torch.int16:
                recs = [(r.clamp(-1, 1) * 32767).to(torch.int16) for r in recs]
            pc = PackedClips(recs, device=DEV)
            index = list(range(N))
            counts, rec, win, _ = pc.segment_plan(index, S)
            rows = int(counts.sum())
            out = torch.empty((rows, 1, S), dtype=torch.float32, device=DEV)
            peaks = pc.peaks() if dtype == torch.float32 else None
            d_off, d_len = pc.offsets[rec.to(DEV)], pc.lengths[rec.to(DEV)]
            d_win, d_rec = win.to(DEV), rec.to(device=DEV, dtype=torch.int32)
            bounds = [(int(o), int(o) + int(n)) for o, n in zip(pc.offsets_host, pc.lengths_host)]

            def kernel():
                return _native.assemble_segments(pc.store, d_off, d_len, d_win, S, peaks, None if peaks is None else d_rec, out)

            def segments():
                return pc.segments(index, S, out=out)[0]

            def stock():
                parts = []
                for (a, b), n in zip(bounds, counts.tolist()):
                    r = pc.store[a:b]
                    if dtype == torch.int16:
                        r = r.float() / 32768
                    r = pn(r[None])
                    left = (n * S - (b - a)) // 2
                    parts.append(F.pad(r[None], (left, n * S - (b - a) - left), "replicate").reshape(-1, 1, S))
                return torch.cat(parts)

            def whole_store_peaks():
                pc.refresh_peaks()
                return pc.peaks()

            a, b, c = kernel().clone(), stock(), segments().clone()
            torch.cuda.synchronize()
            if not (torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))):
                sys.exit(f"the sides disagree at {dtype} N={N}: nothing is timed")
            dev_us, wall_us = time_sides({"kernel": kernel, "segments": segments, "stock": stock}, args.rounds, args.steps, busy, busy_out)
            pdev, pwall = time_sides({"peaks": whole_store_peaks}, args.rounds, args.steps, busy, busy_out)
            fmt = lambda v: f"{statistics.median(v):9.1f} [{min(v):6.1f},{max(v):7.1f}]"
            kd, sd = statistics.median(dev_us["kernel"]), statistics.median(dev_us["stock"])
            nbytes = rows * S * (pc.store.element_size() + 4)
            lines.append(f"{str(dtype).replace('torch.', ''):>8} {N:>4} {rows:>5} | {fmt(dev_us['kernel'])} {statistics.median(wall_us['kernel']):12.1f} "
                         f"{nbytes / kd / 1e3:7.1f} | {statistics.median(wall_us['segments']):13.1f} | {fmt(dev_us['stock']):>26} "
                         f"{statistics.median(wall_us['stock']):11.1f} | {sd / kd:14.2f} | {fmt(pdev['peaks'])} {statistics.median(pwall['peaks']):11.1f}")
            print(lines[-1], flush=True)
    return lines


def standardize_legs(args, busy, busy_out):
    pn = PeakNormalization()
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {args.steps} calls per side after a "
             "warm-up round; us per call: median [min, max]; device = HIP events, calls queued behind a matrix product; wall = host clock to a "
             "synchronise; std = leaf_assemble_clips_std_f32 (standardize=(moments, rec)), plain = leaf_assemble_clips_f32 on the same plan, "
             "stock = gather from a float32 copy of the store standardised per recording (made once, not timed) + gain + PeakNormalization + "
             "masked_fill; moments = the one-time leaf_clip_moments_f32 call over the store, rounds of its own",
             f"{'store':>8} {'B':>4} {'S':>6} | {'std device':>24} {'std wall':>9} | {'plain device':>24} | {'stock device':>24} {'stock wall':>11} | "
             f"{'std / plain':>11} {'stock / std':>11} | {'moments device':>24}"]
    for dtype in (torch.int16, torch.float32):
        for B, S in ((64, 16000), (256, 16000), (256, 80000)):
            store, p = make_case(B, S, dtype, seed=B + S)
            rec = torch.arange(B, dtype=torch.int32, device=DEV)
            moments = _native.clip_moments(store, p["rec_off"], p["rec_len"])
            # the copy a user without the entry would keep: every recording through the reference's expression, on the CPU, once
            wide, mo = (store.cpu().float() / 32768 if dtype == torch.int16 else store.cpu().clone()), moments.cpu()
            for i, (o, n) in enumerate(zip(p["rec_off"].tolist(), p["rec_len"].tolist())):
                wide[o:o + n] = (wide[o:o + n] - mo[i, 0]) / (mo[i, 1] + 1e-9)
            wide = wide.to(DEV)
            out = torch.empty((B, 1, S), dtype=torch.float32, device=DEV)
            ar = torch.arange(S, device=DEV)
            lo, hi = p["masks"][..., 0].long(), (p["masks"][..., 0] + p["masks"][..., 1]).long()
            first = (p["rec_off"] + p["start"])[:, None]

            def kernel():
                return _native.assemble_clips(store, p["rec_off"], p["rec_len"], p["start"], p["pad_mode"], S, p["gain"], True, p["masks"], out,
                                              standardize=(moments, rec))

            def plain():
                return _native.assemble_clips(store, p["rec_off"], p["rec_len"], p["start"], p["pad_mode"], S, p["gain"], True, p["masks"], out)

            def stock():
                x = pn(wide[first + ar] * p["gain"][:, None])
                for m in range(M):
                    x = x.masked_fill((ar >= lo[:, m, None]) & (ar < hi[:, m, None]), 0.0)
                return x[:, None]

            def once():
                return _native.clip_moments(store, p["rec_off"], p["rec_len"])

            a, b = kernel().clone(), stock()
            torch.cuda.synchronize()
            if not torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32)):
                sys.exit(f"the two sides disagree at {dtype} B={B} S={S}: nothing is timed")
            dev_us, wall_us = time_sides({"std": kernel, "plain": plain, "stock": stock}, args.rounds, args.steps, busy, busy_out)
            mom_us, _ = time_sides({"moments": once}, args.rounds, args.steps, busy, busy_out)
            fmt = lambda v: f"{statistics.median(v):9.1f} [{min(v):6.1f},{max(v):7.1f}]"
            med = {k: statistics.median(v) for k, v in dev_us.items()}
            lines.append(f"{str(dtype).replace('torch.', ''):>8} {B:>4} {S:>6} | {fmt(dev_us['std'])} {statistics.median(wall_us['std']):9.1f} | "
                         f"{fmt(dev_us['plain'])} | {fmt(dev_us['stock'])} {statistics.median(wall_us['stock']):11.1f} | "
                         f"{med['std'] / med['plain']:11.2f} {med['stock'] / med['std']:11.2f} | {fmt(mom_us['moments'])}")
            print(lines[-1], flush=True)
    return lines


def device_draw_legs(args, busy, busy_out):
    from leaf_pytorch_amd import ClipSampler, DeviceClipSampler
    S = 16000
    steps = args.steps if args.steps_given else 40
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {steps} calls per side after a "
             "warm-up round, one synchronisation per round; us per call: median [min, max]; device = HIP events, calls queued behind a matrix "
             "product; wall = host clock to the synchronise; host = ClipSampler.__call__ (draws on the CPU, plan uploaded), device = "
             "DeviceClipSampler.__call__ (leaf_draw_clip_plan + the assembling launch), graph = replay of that pair captured, plan / assemble = "
             "each launch alone; 3 masks and background noise on; spread = max - min of host's wall over the rounds",
             f"{'store':>8} {'B':>4} | {'host wall':>26} {'host device':>11} | {'device wall':>26} {'device device':>13} | {'graph wall':>26} "
             f"{'graph device':>12} | {'plan device':>24} {'assemble device':>24} | {'spread':>7} {'device <= host + spread':>23}"]
    for dtype in (torch.int16, torch.float32):
        for B in (64, 256):
            g = torch.Generator().manual_seed(B)

            def packed(n_rec, seed):
                gg = torch.Generator().manual_seed(seed)
                lengths = torch.randint(S + 1, 3 * S, (n_rec,), generator=gg).tolist()
                recs = [(torch.randint(-32768, 32768, (n,), generator=gg).to(torch.int16) if dtype == torch.int16
                         else torch.rand(n, generator=gg) * 2 - 1) for n in lengths]
                return PackedClips(recs, device=DEV)

            clips, nclips = packed(B, B + S), packed(32, B + S + 1)
            kw = dict(num_masks=M, time_perc=0.1, noise_clips=nclips)
            host = ClipSampler(clips, S, generator=g, **kw)
            dev, twin = (DeviceClipSampler(clips, S, seed=1234, batch_size=B, **kw) for _ in range(2))
            index = torch.arange(B)
            out = torch.empty((B, 1, S), dtype=torch.float32, device=DEV)
            static = torch.empty((B, 1, S), dtype=torch.float32, device=DEV)
            dev(out=static)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                dev(out=static)
            twin.set_step(dev.step)
            for _ in range(2):
                graph.replay()
                want = twin()
                torch.cuda.synchronize()
                if not torch.equal(static.view(torch.int32), want.view(torch.int32)):
                    sys.exit(f"the replayed batch is not the eager one at {dtype} B={B}: nothing is timed")
            plan = dev.plan()
            rec_off, rec_len, start, pad_mode, gain, masks = plan
            noise = (nclips.store,) + plan.noise
            sides = {"host": lambda: host(index, out=out), "device": lambda: dev(out=out), "graph": graph.replay, "plan": dev.plan,
                     "assemble": lambda: _native.assemble_clips(clips.store, rec_off, rec_len, start, pad_mode, S, gain, True, masks, out, noise=noise)}
            dev_us, wall_us = time_sides(sides, args.rounds, steps, busy, busy_out)
            fmt = lambda v: f"{statistics.median(v):9.1f} [{min(v):6.1f},{max(v):7.1f}]"
            med = lambda v: statistics.median(v)
            spread = max(wall_us["host"]) - min(wall_us["host"])
            ok = med(wall_us["device"]) <= med(wall_us["host"]) + spread
            lines.append(f"{str(dtype).replace('torch.', ''):>8} {B:>4} | {fmt(wall_us['host']):>26} {med(dev_us['host']):11.1f} | {fmt(wall_us['device']):>26} "
                         f"{med(dev_us['device']):13.1f} | {fmt(wall_us['graph']):>26} {med(dev_us['graph']):12.1f} | {fmt(dev_us['plan'])} "
                         f"{fmt(dev_us['assemble'])} | {spread:7.1f} {'PASS' if ok else 'FAIL':>23}")
            print(lines[-1], flush=True)
    return lines


def device_mixup_legs(args, busy, busy_out):
    import numpy as np
    from leaf_pytorch_amd import DeviceMixup
    steps = args.steps if args.steps_given else 40
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {steps} calls per side after a "
             "warm-up round, one synchronisation per round; us per call: median [min, max]; device = HIP events, calls queued behind a matrix "
             "product; wall = host clock to the synchronise; host = the draws of transforms.Mixup.__call__ and their upload (numpy RandomState "
             "beta, torch.randperm on the CPU, two copies to the device), device = DeviceMixup.__call__ (leaf_draw_mixup), graph = replay of that "
             "launch captured, argsort = torch.argsort of B 64-bit keys on the device (the stock form of the kernel's sort alone)",
             f"{'B':>5} {'alpha':>5} | {'host wall':>26} {'host device':>11} | {'device wall':>26} {'device device':>24} | {'graph wall':>26} "
             f"{'graph device':>12} | {'argsort device':>24}"]
    for B in (64, 256, 4096):
        for alpha in (0.3, 1.0):
            mix, twin = (DeviceMixup(B, alpha=alpha, seed=1234, device=DEV) for _ in range(2))
            mix()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                mix()
            twin.set_step(mix.step)
            for _ in range(2):
                graph.replay()
                perm, lam = twin()
                torch.cuda.synchronize()
                if not (torch.equal(mix.perm, perm) and torch.equal(mix.lam.view(torch.int32), lam.view(torch.int32))):
                    sys.exit(f"the replayed draw is not the eager one at B={B} alpha={alpha}: nothing is timed")
                if sorted(perm.tolist()) != list(range(B)) or not bool(((lam >= 0) & (lam <= 1)).all()):
                    sys.exit(f"not a permutation, or a weight outside [0, 1], at B={B} alpha={alpha}: nothing is timed")
            keys = ((torch.randint(0, 2 ** 31, (B,), generator=torch.Generator().manual_seed(B)) << 32) | torch.arange(B)).to(DEV)

            def host():                                                           # transforms.Mixup.__call__, its first three lines
                random_state = np.random.RandomState(1233)
                lam = torch.from_numpy(random_state.beta(alpha, alpha, B)).to(DEV).float()
                return lam, torch.randperm(B).to(DEV)

            sides = {"host": host, "device": mix, "graph": graph.replay, "argsort": lambda: torch.argsort(keys)}
            dev_us, wall_us = time_sides(sides, args.rounds, steps, busy, busy_out)
            fmt = lambda v: f"{statistics.median(v):9.1f} [{min(v):6.1f},{max(v):7.1f}]"
            med = lambda v: statistics.median(v)
            lines.append(f"{B:>5} {alpha:>5} | {fmt(wall_us['host']):>26} {med(dev_us['host']):11.1f} | {fmt(wall_us['device']):>26} "
                         f"{fmt(dev_us['device'])} | {fmt(wall_us['graph']):>26} {med(dev_us['graph']):12.1f} | {fmt(dev_us['argsort'])}")
            print(lines[-1], flush=True)
    return lines


def effects_legs(args, busy, busy_out):
    import shutil
    import subprocess
    import tempfile
    from leaf_pytorch_amd import ClipSampler, EffectsClipSampler
    S, rate = 16000, 16000
    steps = args.steps if args.steps_given else 20
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {steps} calls per side after a "
             "warm-up round; us per call: median [min, max]; device = HIP events, calls queued behind a matrix product; wall = host clock to a "
             "synchronise every round; effects = EffectsClipSampler.__call__ (clip_prob = reverb_prob = 1), plain = ClipSampler.__call__, "
             "launch = _native.clip_effects alone on device-resident plan and batch",
             f"{'store':>8} {'B':>4} {'S':>6} | {'effects wall':>26} {'effects device':>26} | {'plain wall':>26} {'plain device':>26} | "
             f"{'launch device':>26} {'launch wall':>12} {'us/clip':>8}"]
    for dtype in (torch.int16, torch.float32):
        for B in (64, 256):
            g = torch.Generator().manual_seed(B)
            lengths = torch.randint(S + 1, 3 * S, (B,), generator=g)
            n = int(lengths.sum())
            store = (torch.randint(-32768, 32768, (n,), generator=g).to(torch.int16) if dtype == torch.int16 else torch.rand(n, generator=g) * 2 - 1)
            clips = PackedClips.from_store(store.to(DEV), torch.cumsum(lengths, 0) - lengths, lengths)
            index = torch.arange(B)
            kw = dict(num_masks=M, time_perc=0.1, gain_prob=0.5)
            fx = EffectsClipSampler(clips, S, generator=torch.Generator().manual_seed(1), clip_prob=1.0, reverb_prob=1.0, sample_rate=rate, **kw)
            plain = ClipSampler(clips, S, generator=torch.Generator().manual_seed(1), **kw)
            out_fx, out_plain = (torch.empty((B, 1, S), dtype=torch.float32, device=DEV) for _ in range(2))
            plan = fx.plan(index)
            batch = plain(index).clone()
            factor, reverb = plan.clip_factor.to(DEV), tuple(t.to(DEV) for t in plan.reverb)
            out_launch = torch.empty_like(batch)
            wet = _native.clip_effects(batch, factor, reverb, rate, out=out_launch)
            skip = _native.clip_effects(batch, torch.full((B,), -1.0, device=DEV), tuple(torch.zeros_like(t) for t in reverb), rate)
            torch.cuda.synchronize()
            if not torch.equal(skip.view(torch.int32), batch.view(torch.int32)) or bool((wet == batch).flatten(1).all(1).any()):
                sys.exit(f"the launch does not do what it is timed for at {dtype} B={B}: nothing is timed")
            sides = {"effects": lambda: fx(index, out=out_fx), "plain": lambda: plain(index, out=out_plain),
                     "launch": lambda: _native.clip_effects(batch, factor, reverb, rate, out=out_launch)}
            dev_us, wall_us = time_sides(sides, args.rounds, steps, busy, busy_out)
            fmt = lambda v: f"{statistics.median(v):9.1f} [{min(v):6.1f},{max(v):7.1f}]"
            lines.append(f"{str(dtype).replace('torch.', ''):>8} {B:>4} {S:>6} | {fmt(wall_us['effects']):>26} {fmt(dev_us['effects']):>26} | "
                         f"{fmt(wall_us['plain']):>26} {fmt(dev_us['plain']):>26} | {fmt(dev_us['launch']):>26} "
                         f"{statistics.median(wall_us['launch']):12.1f} {statistics.median(dev_us['launch']) / B:8.2f}")
            print(lines[-1], flush=True)
    cxx = shutil.which("g++")
    if cxx is None:
        lines.append("# CPU: NOT MEASURED (no g++ on this machine)")
    else:
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "clip_effects_check")
            subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(REPO, "leaf_pytorch_amd", "csrc"),
                            os.path.join(REPO, "tools", "clip_effects_check.cpp"), "-o", exe], check=True)
            run = subprocess.run([exe, "time", str(S), "64"], capture_output=True, text=True, check=True)
        lines.append("# CPU, the sequential definition (tools/clip_effects_check.cpp, g++ -O2 -ffp-contract=off, one core): " + run.stdout.strip())
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--noise", action="store_true", help="time the launch with background and Gaussian noise (profiles/clip_noise.txt)")
    ap.add_argument("--segments", action="store_true", help="time the whole-recording evaluation batch (profiles/eval_segments.txt)")
    ap.add_argument("--standardize", action="store_true", help="time the standardising launch (profiles/clip_standardize.txt)")
    ap.add_argument("--device-draws", action="store_true", help="time the batch with its draws: ClipSampler, DeviceClipSampler, the captured graph "
                                                                "(profiles/clip_device_draws.txt)")
    ap.add_argument("--device-mixup", action="store_true", help="time mixup's draws: Mixup's on the host, DeviceMixup, the captured graph, "
                                                                "torch.argsort (profiles/clip_device_mixup.txt)")
    ap.add_argument("--effects", action="store_true", help="time ClipValue and the reverb: EffectsClipSampler, ClipSampler, the launch alone, "
                                                           "the CPU program (profiles/clip_effects.txt)")
    args = ap.parse_args()
    args.steps_given = any(a == "--steps" or a.startswith("--steps=") for a in sys.argv[1:])
    if not torch.cuda.is_available():
        sys.exit("bench_clips.py needs the GPU: a time taken anywhere else says nothing about it")
    if args.noise or args.segments or args.standardize or args.device_draws or args.device_mixup or args.effects:
        busy = torch.rand(8192, 8192, device=DEV)
        legs = effects_legs if args.effects else device_mixup_legs if args.device_mixup else device_draw_legs if args.device_draws else (standardize_legs if args.standardize else (segment_legs if args.segments else noise_legs))
        text = "\n".join(legs(args, busy, torch.empty_like(busy))) + "\n"
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(text)
        return
    pn = PeakNormalization()
    busy = torch.rand(8192, 8192, device=DEV)
    busy_out = torch.empty_like(busy)
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {args.steps} calls per side after a "
             "warm-up round; us per call: median [min, max]; device = HIP events, calls queued behind a matrix product; wall = host clock to a synchronise; GB/s = (store bytes read + 4 B S written) / median device time of the kernel",
             f"{'store':>8} {'B':>4} {'S':>6} {'path':>9} | {'kernel device':>24} {'kernel wall':>12} {'GB/s':>7} | {'stock device':>24} "
             f"{'stock wall':>11} | {'stock / kernel':>14}"]
    for dtype in (torch.int16, torch.float32):
        for B in (64, 256):
            for S in (16000, 80000):
                store, p = make_case(B, S, dtype, seed=B + S)
                out = torch.empty((B, 1, S), dtype=torch.float32, device=DEV)
                ar = torch.arange(S, device=DEV)
                lo, hi = p["masks"][..., 0].long(), (p["masks"][..., 0] + p["masks"][..., 1]).long()
                first = (p["rec_off"] + p["start"])[:, None]

                def kernel():
                    return _native.assemble_clips(store, p["rec_off"], p["rec_len"], p["start"], p["pad_mode"], S, p["gain"], True, p["masks"], out)

                def stock():
                    x = store[first + ar]
                    if dtype == torch.int16:
                        x = x.float() / 32768
                    x = pn(x * p["gain"][:, None])
                    for m in range(M):
                        x = x.masked_fill((ar >= lo[:, m, None]) & (ar < hi[:, m, None]), 0.0)
                    return x[:, None]

                a, b = kernel().clone(), stock()
                torch.cuda.synchronize()
                if not torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32)):
                    sys.exit(f"the two sides disagree at {dtype} B={B} S={S}: nothing is timed")
                sides = {"kernel": kernel, "stock": stock}
                dev_us, wall_us = {k: [] for k in sides}, {k: [] for k in sides}
                for rnd in range(args.rounds + 1):
                    for name in (list(sides) if rnd % 2 == 0 else list(sides)[::-1]):
                        fn = sides[name]
                        for _ in range(3):                                    # the side's code and data warm again after the other side
                            fn()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            fn()
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.mm(busy, busy, out=busy_out)                    # the device works on this while the calls below are enqueued
                        e0.record()
                        for _ in range(args.steps):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        if rnd:                                               # round 0 warms up
                            dev_us[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
                            wall_us[name].append((t1 - t0) * 1e6 / args.steps)
                fmt = lambda v: f"{statistics.median(v):9.1f} [{min(v):6.1f},{max(v):7.1f}]"
                nbytes = B * S * store.element_size() + 4 * B * S
                kd, sd = statistics.median(dev_us["kernel"]), statistics.median(dev_us["stock"])
                lines.append(f"{str(dtype).replace('torch.', ''):>8} {B:>4} {S:>6} {'resident' if S <= _native.ASSEMBLE_RESIDENT_MAX else 'reread':>9} | "
                             f"{fmt(dev_us['kernel'])} {statistics.median(wall_us['kernel']):12.1f} {nbytes / kd / 1e3:7.1f} | {fmt(dev_us['stock'])} "
                             f"{statistics.median(wall_us['stock']):11.1f} | {sd / kd:14.2f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
