"""Cases and the call helper of tests/test_gpu_tail_rows.py (and of tests/golden/make_golden_tail_rows.py, which records a few of
them): the row-owned tail of the static workgroup kernel (csrc/leaf_fft_wg.hpp: wg_tail_rows).  Plain module: no fixtures.

A case is a batch of B clips of T' frames on G workgroups (LEAF_ALGO_RESERVE_CUS).  How the blocks fall decides what finalizes a clip:

* B a multiple of G and the per-frame sums of B / G clips inside the workgroup's LDS (here: at most ``LDS_ELEMS`` sums, the
  default forward's own 40 x 100) -> every workgroup finalizes its clips in its tail from the sums in LDS (``fin_fused == 3``);
* an uneven dealing -> a workgroup finalizes the clips all of whose blocks it ran in its tail from the partial sums in the
  workspace (``fin_fused == 1``, the relaxed agent-scope loads), and the row kernel finalizes the clips that straddle two;
* LEAF_ALGO_STREAM_FINALIZE -> the streaming finalize (another instance, not touched by the tail);
* a dealing in which EVERY clip straddles two workgroups -> the row kernel alone.

The calls go through the C ABI directly, with ``out`` and the saved pre-floor tensor in guarded buffers (tests/guarded.py)."""
import ctypes

import torch

from guarded import guarded
from leaf_pytorch_amd import _native as N

DEV = "cuda:0"
SF = N.ALGO_STREAM_FINALIZE
LDS_ELEMS = 4000                                            # clips per workgroup x F x T' of the default forward (16 kHz, 1 s, 40 filters)
FRAMES = (1, 2, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 130, 257)
FILTERS = (1, 11, 12, 13, 40, 64)
MODES = ("pcen", "pcen-off", "log1p", "bf16", "peaknorm", "delta-le-0", "smoother-0-and-1", "raw")
GEOMETRY = {16000: (401, 160), 8000: (201, 80), 32000: (801, 320)}


def clip_len(tp, hop):
    return hop * (tp - 1) + 1


def cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def grid_bits(g):
    assert 0 < g <= cus() and cus() - g < 256
    return N.algo_reserve_cus(cus() - g)


def owned(B, nblk, G):
    """The clips a workgroup owns outright under the contiguous dealing of B * nblk blocks to G workgroups (csrc/leaf_fft.hpp: OwnedClips)."""
    n = B * nblk
    G = min(G, n)
    per, rem = divmod(n, G)
    start = lambda w: w * per + min(w, rem)
    wg_of = lambda gb: next(w for w in range(G) if start(w) <= gb < start(w + 1))
    return [b for b in range(B) if wg_of(b * nblk) == wg_of(b * nblk + nblk - 1)]


def inputs(F, K, hop, tp, B, mode, seed):
    """Waveform and the seven parameters of a case, on the CPU (deterministic in ``seed``)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    T = clip_len(tp, hop)
    x = 2 * r(B, T) - 1
    if mode == "peaknorm":
        x = x * (0.25 + 3 * r(B, 1))                        # peaks away from 1: the scale matters
    kern = torch.stack([0.1 + r(F) * 2.9, 3.0 + r(F) * K / 4], dim=1)
    pw, pb = 0.2 + 0.4 * r(F), 0.5 + r(F)
    alpha, delta, root, ema_w = 0.9 + 0.1 * r(F), 1.0 + 2 * r(F), 1.0 + 2 * r(F), 0.02 + 0.1 * r(F)
    if mode == "delta-le-0":                                # the reference's literal formula: delta = 0, and a negative one under root 1
        delta[0] = 0.0
        delta[F - 1], root[F - 1] = (-0.25, 1.0) if F > 1 else (0.0, root[0])
    if mode == "smoother-0-and-1":                          # clamped to [0, 1]: 0 holds p_0, 1 follows the input
        ema_w[0] = 0.0
        ema_w[F - 1] = 1.0 if F > 1 else 0.0
        if F > 3:
            ema_w[1], ema_w[2] = -0.2, 1.5
    return x, (kern, pw, pb, alpha, delta, root, ema_w)


def flags_of(mode):
    if mode == "pcen-off":
        return 0
    if mode == "log1p":
        return N.FLAG_LOG1P
    return N.FLAG_PCEN | {"bf16": N.FLAG_OUT_BF16, "peaknorm": N.FLAG_PEAKNORM}.get(mode, 0)


def forward(x, params, K, hop, mode, algo):
    """One C-ABI forward of the case's inputs -> (out, raw or None) on the CPU; the guards of both buffers are checked."""
    lib = N.load()
    dev = torch.device(DEV)
    xd = x.to(dev).contiguous()
    prm = [p.to(dev).contiguous() for p in params]
    B, T = xd.shape
    F = prm[0].shape[0]
    tp = lib.leaf_num_frames(T, K, hop)
    flags = flags_of(mode)
    feat = torch.bfloat16 if flags & N.FLAG_OUT_BF16 else torch.float32
    out = guarded(B * F * tp * (2 if feat == torch.bfloat16 else 4), 0xA5)
    raw = guarded(B * F * tp * 4, 0xA5) if mode == "raw" else None
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        n = lib.leaf_workspace_bytes(B, T, F, K, hop, algo)
        ws = torch.empty(max(n, 4), dtype=torch.uint8, device=dev)
        head = (P(xd), B, T, *[P(p) for p in prm], F, K, hop, flags, algo, out.ptr)
        if raw is not None:
            rc = lib.leaf_forward_save_f32(*head, raw.ptr, P(ws), n, N.stream_ptr(dev))
        else:
            rc = lib.leaf_forward_f32(*head, P(ws), n, N.stream_ptr(dev))
    assert rc == 0, f"status {rc}"
    torch.cuda.synchronize()
    out.check("out")
    if raw is not None:
        raw.check("raw_out")
    return out.cpu(feat, (B, F, tp)), None if raw is None else raw.cpu(torch.float32, (B, F, tp))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a.float(), nan=12345.0), torch.nan_to_num(b.float(), nan=12345.0))


def row_kernel_reference(x, params, K, hop, mode, nblk):
    """The same clips finalized by the row kernel alone: a dealing in which every clip straddles two workgroups (one call for the batch
    when a grid does that, else clip by clip on two workgroups -- the bits of a clip do not depend on the batch)."""
    assert nblk >= 2
    B = x.shape[0]
    for G in range(2, min(B * nblk, 48) + 1):
        if not owned(B, nblk, G):
            return forward(x, params, K, hop, mode, N.ALGO_FFT_WG | grid_bits(G))
    outs = [forward(x[b:b + 1], params, K, hop, mode, N.ALGO_FFT_WG | grid_bits(2)) for b in range(B)]
    return torch.cat([o[0] for o in outs]), (None if outs[0][1] is None else torch.cat([o[1] for o in outs]))


# the cases recorded from the commit before the row-owned tail (tests/golden/tail_rows/<name>.npz): (name, sample rate, F, T', B, G, mode)
GOLDEN = [
    ("lds-40x100-pcen", 16000, 40, 100, 2, 2, "pcen"),
    ("lds-13x130-two-clips-log1p", 16000, 13, 130, 4, 2, "log1p"),
    ("lds-64x17-three-clips-bf16", 16000, 64, 17, 6, 2, "bf16"),
    ("part-40x257-uneven-raw", 16000, 40, 257, 5, 2, "raw"),
    ("part-12x129-uneven-delta-le-0", 16000, 12, 129, 5, 2, "delta-le-0"),
    ("lds-8k-40x100-smoother-0-and-1", 8000, 40, 100, 2, 2, "smoother-0-and-1"),
]


def golden_seed(name):
    return 7000 + sum(name.encode())
