#!/usr/bin/env python3
"""Time forward and forward+backward of Leaf (parameters require grad) on one GPU.
   usage: bench_backward.py [--no-pcen | --log1p] [--bf16 | --pcm16] [--out-bf16] [--mixup] [--frozen-filters] [--interleave V1,V2,..] [B [n_filters sample_rate seconds [nodx]]]
   (default 256 clips of the default 40 f / 16 kHz / 1 s, PCEN on, float32;
   nodx skips the dL/dx timing -- staged kernels, hundreds of ms, for geometries without a fused dL/dx)
   --no-pcen: PCEN off (BASELINE configs[3] without compression); --log1p: PCEN off with Leaf.log_compression() (configs[3]);
   --bf16: bfloat16 waveform, features, grad_out and dL/dx (configs[4]).
   --pcm16: int16 waveform (16-bit PCM, a sample v means v / 32768), float32 features and grad_out, no dL/dx.
   --out-bf16: bfloat16 features and grad_out from the float32 or --pcm16 waveform (Leaf.output_dtype(torch.bfloat16)); dL/dx stays float32.
   Interleave legs: "+outbf16" the same, fused in the kernels' stores and loads; "+outcast" the stock float32 forward followed by
   .to(torch.bfloat16) (whose backward is grad.float()): the cast kernels the fused leg saves, one per direction.
   --mixup: waveform mixup folded into the step (Leaf.forward_mixup with a fixed permutation and weights; float32 or --pcm16; no dL/dx).
   Interleave legs: "+mixup" the fused step, "+mixstock" the reference's stock-op mixup (x * lam + x[perm] * (1 - lam), an int16 batch
   cast first) followed by the plain step, neither: the plain step.
   --frozen-filters: a Leaf whose Gabor kernel and pooling width are frozen (requires_grad_(False)), so that only the pooling bias and
   PCEN train: the interleave legs "pcen+frozen" (the head-only backward the module then takes: leaf_backward_head_f32, one launch)
   and "pcen+frozen+fullroute" (Leaf.full_backward(): the full backward forced on the same module -- what the step cost before),
   at BASELINE configs[1] (256 x 1 s, 40 filters, 16 kHz) and one GPU's share of configs[2] (128 x 5 s, 80 filters, 32 kHz), or at the
   shape given.  profiles/frozen_filters.txt is this command's output.
   --interleave pcen,off,log1p,pcen+bf16,pcen+pcm16,pcen+pcm16cast,...: ("+pcm16cast": the int16 clips converted by the caller,
   x.float().mul_(2**-15), inside the timed step, then the float32 call; "+fwd": the no-grad forward alone instead of the step) instead of the line above, the training step (grad_out resident; with "+dx": incl. dL/dx)
   of each named variant timed in turn, round after round, in this one process: median, min and max of the rounds per variant, so that
   two variants are compared under the same clocks and the spread of each is on the page."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leaf_pytorch_amd import Leaf  # noqa: E402

dev = torch.device("cuda:0")
OPTS = {a for a in sys.argv[1:] if a in ("--no-pcen", "--log1p", "--bf16", "--pcm16", "--out-bf16", "--mixup", "--frozen-filters")}
INTERLEAVE = None
if "--interleave" in sys.argv:
    i = sys.argv.index("--interleave")
    INTERLEAVE = sys.argv[i + 1].split(",")
    del sys.argv[i:i + 2]
sys.argv = [a for a in sys.argv if a not in OPTS]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
F = int(sys.argv[2]) if len(sys.argv) > 2 else 40
SR = int(sys.argv[3]) if len(sys.argv) > 3 else 16000
SECS = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
torch.manual_seed(0)


def make(pcen=True, log1p=False):
    mod = Leaf(n_filters=F, sample_rate=SR, pcen_compression=pcen and not log1p)
    return (mod.log_compression() if log1p else mod).to(dev)


def set_shape(b, f, sr, secs):
    """The clips (float32 and the same as 16-bit PCM) and the mixup draw of one shape."""
    global B, F, SR, SECS, x, x16, MIX_PERM, MIX_LAM
    B, F, SR, SECS = b, f, sr, secs
    x = 2 * torch.rand(B, 1, int(SR * SECS), device=dev) - 1
    x16 = torch.round(x.float() * 32767).to(torch.int16)          # the same clips as 16-bit PCM
    MIX_PERM = torch.randperm(B, device=dev)                     # one fixed draw: the timing is about the kernels, not the RNG
    MIX_LAM = torch.rand(B, device=dev)


def interleave(legs):
    """The training step of each named variant timed in turn, round after round, in this one process."""
    import statistics
    steps = {}
    for name in legs:
        parts = name.split("+")
        mod = make(pcen=parts[0] == "pcen", log1p=parts[0] == "log1p")
        pcm, cast = "pcm16" in parts, "pcm16cast" in parts
        outcast = "outcast" in parts
        if "outbf16" in parts:
            mod.output_dtype(torch.bfloat16)
        if "frozen" in parts:                            # a pretrained filterbank: only the pooling bias and PCEN train
            mod._complex_conv._kernel.requires_grad_(False)
            mod._pooling.weights.requires_grad_(False)
        if "fullroute" in parts:                         # ... on the full backward all the same (Leaf.full_backward())
            mod.full_backward()
        xv = x16.clone() if pcm or cast else (x.to(torch.bfloat16) if "bf16" in parts else x.float()).clone().requires_grad_("dx" in parts)
        with torch.no_grad():
            gv = torch.randn_like(mod(xv))
        if outcast:
            gv = gv.to(torch.bfloat16)

        def step(mod=mod, xv=xv, gv=gv, cast=cast, fwd_only="fwd" in parts, fused="mixup" in parts, stock="mixstock" in parts, outcast=outcast):
            xin = xv.float().mul_(2.0 ** -15) if cast else xv
            if stock:                                    # utilities/data/mixup.py:20 with stock ops (an integer batch is cast first)
                xf = xin if xin.is_floating_point() else xin.float().mul_(2.0 ** -15)
                lam3 = MIX_LAM.view(B, 1, 1)
                xin = xf * lam3 + xf[MIX_PERM] * (1 - lam3)
            call = (lambda t: mod.forward_mixup(t, MIX_PERM, MIX_LAM)) if fused else mod
            if outcast:                                  # float32 features, then the cast (autograd widens the gradient on the way back)
                inner = call
                call = lambda t: inner(t).to(torch.bfloat16)
            if fwd_only:
                with torch.no_grad():
                    call(xin)
                return
            mod.zero_grad(set_to_none=True)
            xv.grad = None
            torch.autograd.backward(call(xin), gv)
        steps[name] = step
    res = {name: [] for name in steps}
    for rnd in range(9):
        for name, step in steps.items():
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(20):
                step()
            e.record(); e.synchronize()
            if rnd:                                # (the first round warms the clocks and the allocator)
                res[name].append(s.elapsed_time(e) / 20)
    for name, r in res.items():
        print(f"B={B} F={F} sr={SR} {SECS:g}s {name:18s} {'forward (no grad)' if '+fwd' in name else 'forward+backward (grad_out resident)'} median {statistics.median(r):.4f} ms   "
              f"min {min(r):.4f}   max {max(r):.4f}   spread {max(r) - min(r):.4f}")


if "--frozen-filters" in OPTS:
    # Gabor kernel and pooling width frozen: the head-only backward (leaf_backward_head_f32) against the full backward forced on the
    # same module, at BASELINE configs[1] and one GPU's share of configs[2] -- or at the one shape given on the command line
    for shape in ([(B, F, SR, SECS)] if len(sys.argv) > 1 else [(256, 40, 16000, 1.0), (128, 80, 32000, 5.0)]):
        set_shape(*shape)
        interleave(["pcen+frozen", "pcen+frozen+fullroute"])
    sys.exit(0)
set_shape(B, F, SR, SECS)
m = make(pcen="--no-pcen" not in OPTS, log1p="--log1p" in OPTS)
if "--out-bf16" in OPTS:
    m.output_dtype(torch.bfloat16)
if "--bf16" in OPTS:
    x = x.to(torch.bfloat16)
if "--pcm16" in OPTS:
    x = x16
if "--mixup" in OPTS:
    _plain = m.forward
    m.forward = lambda xin: m.forward_mixup(xin, MIX_PERM, MIX_LAM) if not xin.requires_grad else _plain(xin)


def timed(fn, n=20):
    import time
    t0 = time.perf_counter()                      # spin-up: let the clocks settle before timing
    while time.perf_counter() - t0 < 0.25:
        fn()
    torch.cuda.synchronize()
    reps = []                                     # median of five event-timed regions (a host hiccup costs one region, not the figure)
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record(); e.synchronize()
        reps.append(s.elapsed_time(e) / n)
    return sorted(reps)[2]


def fwd():
    with torch.no_grad():
        m(x)


def fwd_bwd():
    m.zero_grad(set_to_none=True)
    m(x).sum().backward()


# the same step with the gradient of the output already resident, as it arrives from a backbone in training
# (train.py:257-259): `.sum().backward()` above adds a reduction, a fill and a broadcast copy of its own (~25 us at cfg1)
with torch.no_grad():
    go = torch.randn_like(m(x))


def fwd_bwd_resident():
    m.zero_grad(set_to_none=True)
    torch.autograd.backward(m(x), go)


xg = x.clone().requires_grad_(True) if x.is_floating_point() and "--mixup" not in OPTS else None


def fwd_bwd_dx():
    m.zero_grad(set_to_none=True)
    xg.grad = None
    m(xg).sum().backward()


def graphed(fn_step):
    """the step captured into one HIP graph (torch.cuda.graph): what is left of the step when the host's dispatcher / autograd work is
    taken out -- for the small batches where that work is longer than the kernels"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn_step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    m.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        torch.autograd.backward(m(x), go)
    return g.replay


NODX = (len(sys.argv) > 5 and sys.argv[5] == "nodx") or xg is None          # (an integer waveform has no gradient)
if INTERLEAVE:
    interleave(INTERLEAVE)
    sys.exit(0)
print(f"B={B} F={F} sr={SR} {SECS:g}s: forward {timed(fwd):.3f} ms   forward+backward {timed(fwd_bwd):.3f} ms   "
      f"(grad_out resident: {timed(fwd_bwd_resident):.3f} ms)   "
      + ("" if NODX else f"forward+backward incl. dL/dx {timed(fwd_bwd_dx):.3f} ms")
      + (f"   as one HIP graph (grad_out resident): {timed(graphed(fwd_bwd_resident)):.3f} ms" if os.environ.get("LEAF_BENCH_GRAPH") else ""))
