#!/usr/bin/env python3
"""Per-step time of a running LeafStream, fused (one leaf_stream_step_f32 launch) against unfused (the two-launch class: cat ->
forward -> slice -> leaf_pcen_stream_f32 -> slice), 16 kHz / 40 filters / PCEN, in steady state.

    python tools/bench_stream.py [--rounds 6] [--steps 40] [--out profiles/stream_fused.txt]

Both legs run in ONE process, in turn, round after round after a warm-up round (the order of the legs alternates), on views of one
long recording.  Two figures per leg and shape, each the median / min / max over the rounds of (time of `steps` steps) / steps:
  wall    host clock from the first step() to the end of a device synchronisation behind the last: what a serving loop sees
  device  HIP events around the same steps, ENQUEUED WHILE THE DEVICE IS KEPT BUSY by matrix products queued in front, so that the
          steps run back to back from a full queue: the device's own time per step, launch gaps between dependent kernels included,
          the host's enqueue time excluded
No assertion on any time; prints the table and, with --out, writes it.

    python tools/bench_stream.py --bank [--rounds 20] [--steps 40] [--out profiles/stream_bank.txt]

The bank leg: B INDEPENDENT streams, one LeafStreamBank step for all of them against what a server does without the bank -- a Python
loop over B LeafStream(fused=True) objects of one waveform each -- in one process, the two sides taking turns round after round (the
order alternates) after a warm-up round.  B = 4 / 16 / 64, chunks of 160 and 1600 samples; wall time per step (all B streams served,
device synchronised behind the last step): median [p10, p90] over the rounds, and the ratio of the medians.

    python tools/bench_stream.py --resample [--rounds 20] [--steps 40] [--out profiles/stream_resample.txt]

The resampling leg: B streams at a device rate, one ResampleStreamBank step for all of them against the stock alternative -- a history
tensor of K - 1 samples per stream, torch.cat with the chunk, resample() of the whole buffer and a slice of the outputs that are new --
in one process, the two sides taking turns as above.  B = 4 / 16 / 64, chunks of 10 ms and 100 ms, 48 -> 16 and 44.1 -> 16 kHz, int16
and float32 samples; wall time per step, median [p10, p90], and the ratio of the medians.  (The stock side's slice is sized for a
steady stream and is not the bank's bits at the seams: it stands for the cost of that way, not for its correctness.)"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import leaf_pytorch_amd as L  # noqa: E402

DEV = "cuda:0"


def run_steps(stream, x, chunk, steps, pos):
    T = x.shape[-1]
    for _ in range(steps):
        if pos + chunk > T:
            pos = 0
        stream.step(x[:, :, pos:pos + chunk])
        pos += chunk
    return pos


def bank_leg(m, args):
    rounds = args.rounds if args.rounds > 6 else 20
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {rounds} timed rounds x {args.steps} steps per side after a warm-up round; "
             "wall us per step (all B streams): median [p10, p90]",
             f"{'B':>3} {'chunk':>6} {'bank step':>30} {'loop of B fused streams':>30} {'bank / loop':>12}"]
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(round(q * (len(v) - 1))))]
    for B in (4, 16, 64):
        x = (2 * torch.rand(B, 1, 160000, device=DEV) - 1)
        for chunk in (160, 1600):
            bank = L.LeafStreamBank(m, B)
            loop = [L.LeafStream(m, fused=True) for _ in range(B)]
            lengths = [chunk] * B

            def bank_steps(n, pos):
                for _ in range(n):
                    pos = 0 if pos + chunk > x.shape[-1] else pos
                    bank.step(x[:, :, pos:pos + chunk], lengths)
                    pos += chunk
                return pos

            def loop_steps(n, pos):
                for _ in range(n):
                    pos = 0 if pos + chunk > x.shape[-1] else pos
                    for b, s in enumerate(loop):
                        s.step(x[b:b + 1, :, pos:pos + chunk])
                    pos += chunk
                return pos

            sides = {"bank": bank_steps, "loop": loop_steps}
            pos, wall = {k: 0 for k in sides}, {k: [] for k in sides}
            for rnd in range(rounds + 1):
                for name in (list(sides) if rnd % 2 == 0 else list(sides)[::-1]):
                    pos[name] = sides[name](5, pos[name])                 # the side's code and data warm again after the other side
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pos[name] = sides[name](args.steps, pos[name])
                    torch.cuda.synchronize()
                    if rnd:
                        wall[name].append((time.perf_counter() - t0) / args.steps * 1e6)
            fmt = lambda v: f"{statistics.median(v):9.1f} [{pct(v, 0.1):8.1f}, {pct(v, 0.9):8.1f}]"
            lines.append(f"{B:>3} {chunk:>6} {fmt(wall['bank']):>30} {fmt(wall['loop']):>30} {statistics.median(wall['bank']) / statistics.median(wall['loop']):>12.3f}")
            bank.flush()
            for s in loop:
                s.flush()
    return lines


def resample_leg(args):
    rounds = args.rounds if args.rounds > 6 else 20
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {rounds} timed rounds x {args.steps} steps per side after a warm-up round; "
             "wall us per step (all B streams): median [p10, p90]",
             f"{'rates':>14} {'dtype':>8} {'B':>3} {'chunk':>6} {'bank step':>30} {'cat + resample() + slice':>30} {'bank / stock':>12}"]
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(round(q * (len(v) - 1))))]
    for orig, new in ((48000, 16000), (44100, 16000)):
        for dtype in (torch.int16, torch.float32):
            for B in (4, 16, 64):
                T = orig * 4
                x = torch.randint(-32768, 32768, (B, T), device=DEV, dtype=torch.int32).to(torch.int16) if dtype is torch.int16 else 2 * torch.rand(B, T, device=DEV) - 1
                for chunk in (orig // 100, orig // 10):
                    bank = L.ResampleStreamBank(orig, new, B, sample_dtype=dtype)
                    lengths, H = [chunk] * B, max(bank.history, 1)
                    per_step = chunk * new // orig                       # outputs of a steady step, about
                    hist = [torch.zeros(B, H, dtype=dtype, device=DEV)]

                    def bank_steps(n, pos):
                        for _ in range(n):
                            pos = 0 if pos + chunk > T else pos
                            bank.step(x[:, pos:pos + chunk], lengths)
                            pos += chunk
                        return pos

                    def stock_steps(n, pos):
                        for _ in range(n):
                            pos = 0 if pos + chunk > T else pos
                            buf = torch.cat([hist[0], x[:, pos:pos + chunk]], dim=1)
                            y = L.resample(buf, orig, new)
                            y = y[:, y.shape[1] - per_step:]             # noqa: F841  (the step's result)
                            hist[0] = buf[:, buf.shape[1] - H:]
                            pos += chunk
                        return pos

                    sides = {"bank": bank_steps, "stock": stock_steps}
                    pos, wall = {k: 0 for k in sides}, {k: [] for k in sides}
                    for rnd in range(rounds + 1):
                        for name in (list(sides) if rnd % 2 == 0 else list(sides)[::-1]):
                            pos[name] = sides[name](5, pos[name])         # the side's code and data warm again after the other side
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            pos[name] = sides[name](args.steps, pos[name])
                            torch.cuda.synchronize()
                            if rnd:
                                wall[name].append((time.perf_counter() - t0) / args.steps * 1e6)
                    fmt = lambda v: f"{statistics.median(v):9.1f} [{pct(v, 0.1):8.1f}, {pct(v, 0.9):8.1f}]"
                    lines.append(f"{orig:>6} -> {new:<5} {str(dtype).replace('torch.', ''):>8} {B:>3} {chunk:>6} {fmt(wall['bank']):>30} {fmt(wall['stock']):>30} "
                                 f"{statistics.median(wall['bank']) / statistics.median(wall['stock']):>12.3f}")
                    bank.flush()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resample", action="store_true", help="the ResampleStreamBank leg (module docstring)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--bank", action="store_true", help="the LeafStreamBank leg (module docstring) instead of fused against unfused")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.resample:
        text = "\n".join(resample_leg(args))
        print(text)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        return
    m = L.Leaf().eval().to(DEV)
    for p in m.parameters():
        p.requires_grad_(False)
    if args.bank:
        text = "\n".join(bank_leg(m, args))
        print(text)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        return
    blocker = torch.randn(8192, 8192, device=DEV)
    lines = [f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.rounds} timed rounds x {args.steps} steps per leg after a warm-up round; "
             "us per step: median (min .. max)",
             f"{'B':>3} {'chunk':>6} {'leg':<8} {'wall us':>26} {'device us':>26}"]
    for B in (1, 4, 16):
        x = (2 * torch.rand(B, 1, 160000, device=DEV) - 1)
        for chunk in (160, 1600, 8000):
            legs = {"fused": L.LeafStream(m, fused=True), "unfused": L.LeafStream(m)}
            pos = {k: 0 for k in legs}
            wall, dev = {k: [] for k in legs}, {k: [] for k in legs}
            for rnd in range(args.rounds + 1):
                order = list(legs) if rnd % 2 == 0 else list(legs)[::-1]
                for name in order:
                    s = legs[name]
                    pos[name] = run_steps(s, x, chunk, 5, pos[name])      # the leg's code and data warm again after the other leg
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pos[name] = run_steps(s, x, chunk, args.steps, pos[name])
                    torch.cuda.synchronize()
                    w = (time.perf_counter() - t0) / args.steps
                    # device time: the same steps behind enough queued work to cover the host's enqueue time twice over
                    t0 = time.perf_counter()
                    blocker @ blocker
                    torch.cuda.synchronize()
                    one = time.perf_counter() - t0
                    for _ in range(max(2, int(2 * w * args.steps / one) + 1)):
                        blocker @ blocker
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    pos[name] = run_steps(s, x, chunk, args.steps, pos[name])
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd:
                        wall[name].append(w * 1e6)
                        dev[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
            for name in legs:
                fmt = lambda v: f"{statistics.median(v):8.1f} ({min(v):7.1f} .. {max(v):7.1f})"
                lines.append(f"{B:>3} {chunk:>6} {name:<8} {fmt(wall[name])} {fmt(dev[name])}")
            for s in legs.values():
                s.flush()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
