"""LeafStreamBank: independent streams in one leaf_stream_bank_step_f32 call per step (csrc/leaf_fft_stream.hpp).  Every stream of a
bank must give, bit for bit, what a one-waveform LeafStream(fused=True) gives for the same chunks and a flush() -- the two kernels
share one device body -- whatever the other slots do; the C entry keeps the memory contract of include/leaf_hip.h.

Shapes: n_filters = 6 (2 for the launch split), streams of a few thousand samples; chunk sizes below a hop, no multiple of the hop,
one block (1600) and the window length; streams that begin late, end on a chunk that completes frames (the two-pass record), end on a
chunk that completes none, end without samples, and a slot that is used twice."""
import ctypes
import functools

import pytest
import torch

import leaf_pytorch_amd as L
from conftest import rel_err
from guarded import guarded
from leaf_pytorch_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STREAM_TOL = 1e-5     # the project's streaming tolerance (tests/test_gpu_stream_fused.py), restated
F = 6
PRM = ("_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta", "_compression.root",
       "_compression.ema._weights")

# (length, end) per slot and step.  Slot 0 is fed every step; slot 1 begins late, ends on a non-empty chunk and begins a second stream;
# slot 2 is idle for most steps, then carries a one-chunk stream of 100 samples and another of 1 sample.
SCRIPT = [
    [(160, 0), (0, 0), (0, 0)],
    [(1, 0), (0, 0), (0, 0)],
    [(401, 0), (500, 0), (0, 0)],
    [(1600, 0), (1600, 0), (0, 0)],
    [(37, 0), (700, 1), (100, 1)],
    [(160, 0), (0, 0), (0, 0)],
    [(800, 0), (300, 0), (1, 1)],
    [(5, 0), (0, 1), (0, 1)],          # slot 1 ends without samples; `end` on slot 2, which is not running, does nothing
    [(0, 1), (0, 0), (0, 0)],
]


@functools.lru_cache(maxsize=None)
def _module(sample_rate, pcen, log1p, n_filters=F):
    torch.manual_seed(sample_rate + 2 * pcen + log1p)
    m = L.Leaf(n_filters=n_filters, sample_rate=sample_rate, pcen_compression=pcen).eval().to(DEV)
    for p in m.parameters():
        p.requires_grad_(False)
    if log1p:
        m.log_compression()
    return m


@functools.lru_cache(maxsize=None)
def _waves(B, n=6000, seed=5):
    """One recording per slot to cut the streams from -- computed once, shared, never modified."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g).to(DEV)


def _drive(bank, script, waves, poison=float("nan"), strided=False):
    """Run ``script`` through ``bank``; a slot's samples are consecutive samples of its row of ``waves``, the rest of a chunk row is
    poison.  Returns the finished streams in the order they ended: (slot, [its chunks], its frames concatenated)."""
    B = bank.slots
    pos, chunks, frames, done = [0] * B, [[] for _ in range(B)], [[] for _ in range(B)], []
    for row in script:
        lengths, end = [r[0] for r in row], [bool(r[1]) for r in row]
        Tmax = max(lengths)
        chunk = None
        if Tmax:
            wide = torch.full((B, 1, 2 * Tmax + 3), poison if waves.dtype.is_floating_point else 32767, dtype=waves.dtype, device=DEV)
            chunk = wide[:, :, 3:3 + Tmax] if strided else wide[:, :, :Tmax].contiguous()
            for b, n in enumerate(lengths):
                chunk[b, 0, :n] = waves[b, pos[b]:pos[b] + n]
                if n:
                    chunks[b].append(waves[b, pos[b]:pos[b] + n].clone())
                pos[b] += n
        running = list(bank.running)
        out, counts = bank.step(chunk, lengths, end)
        assert out.shape == (B, bank.F, max(counts)) and out.dtype == bank.out_dtype
        for b in range(B):
            assert bool((out[b, :, counts[b]:] == 0).all()), f"slot {b}: the row behind its {counts[b]} frames is not zero"
            if lengths[b] or (end[b] and running[b]):
                frames[b].append(out[b:b + 1, :, :counts[b]].clone())
            else:
                assert counts[b] == 0
            if end[b] and (running[b] or lengths[b]):
                done.append((b, chunks[b], torch.cat(frames[b], dim=-1)))
                chunks[b], frames[b] = [], []
    assert not any(bank.running)
    return done


def _single(m, chunks, **kw):
    """The same stream through a one-waveform LeafStream(fused=True): its chunks, then flush()."""
    s = L.LeafStream(m, fused=True, **kw)
    return torch.cat([s.step(c.reshape(1, 1, -1)) for c in chunks] + [s.flush()], dim=-1)


@pytest.mark.parametrize("sample_rate,pcen,log1p", [(16000, True, False), (16000, False, False), (16000, False, True),
                                                    (8000, True, False), (8000, False, False), (8000, False, True)])
def test_every_stream_equals_its_single_stream_run(sample_rate, pcen, log1p):
    m, waves = _module(sample_rate, pcen, log1p), _waves(3)
    done = _drive(L.LeafStreamBank(m, 3), SCRIPT, waves)
    assert [b for b, _, _ in done] == [1, 2, 2, 1, 0] and [sum(c.numel() for c in ch) for _, ch, _ in done] == [2800, 100, 1, 300, 3164]
    for b, chunks, got in done:
        want = _single(m, chunks)
        assert got.shape == want.shape and got.dtype == torch.float32
        diff = (got != want).sum().item()
        print(f"slot {b}, {sum(c.numel() for c in chunks)} samples: {got.shape[-1]} frames, {diff} elements differ from the single stream")
        assert torch.equal(got, want), f"slot {b}: {diff} elements differ from the one-waveform stream"
        with torch.no_grad():
            whole = m(torch.cat(chunks).reshape(1, 1, -1))
        err = rel_err(got.cpu(), whole.cpu())
        assert got.shape == whole.shape and err < STREAM_TOL, f"slot {b} vs whole clip: {err:.3e}"


def test_a_slot_does_not_see_its_neighbours():
    """Slot 0's frames are the same bits whether the other slots idle, run, or are fed NaN / inf; a slot reused after `end` on top of
    what the earlier stream left (nothing is ever cleared) equals the same stream in a fresh bank."""
    m, waves = _module(16000, True, False), _waves(3)
    alone = [[row[0], (0, 0), (0, 0)] for row in SCRIPT]
    base = _drive(L.LeafStreamBank(m, 3), alone, waves)
    assert len(base) == 1 and base[0][0] == 0
    bad = waves.clone()
    bad[1] = float("nan")
    bad[2] = float("inf")
    for other in (_drive(L.LeafStreamBank(m, 3), SCRIPT, waves), _drive(L.LeafStreamBank(m, 3), SCRIPT, bad, poison=float("inf"))):
        got = [fr for b, _, fr in other if b == 0]
        assert len(got) == 1 and torch.equal(got[0], base[0][2])
    # slot 1's second stream (300 samples from 2800 on), alone in a bank that has never run
    again = _drive(L.LeafStreamBank(m, 3), [[(0, 0), (300, 0), (0, 0)], [(0, 0), (0, 1), (0, 0)]], torch.roll(waves, -2800, dims=1))
    reused = [fr for b, ch, fr in _drive(L.LeafStreamBank(m, 3), SCRIPT, waves) if b == 1][1]
    assert torch.equal(again[0][2], reused)


def test_sample_types_feature_dtype_and_strided_chunks():
    m, waves = _module(16000, True, False), _waves(3)
    pcm = (waves.clamp(-4, 4) * 8000).round().to(torch.int16)
    from_int = _drive(L.LeafStreamBank(m, 3, sample_dtype=torch.int16), SCRIPT, pcm)
    from_float = _drive(L.LeafStreamBank(m, 3), SCRIPT, pcm.float() / 32768)
    f32 = _drive(L.LeafStreamBank(m, 3), SCRIPT, waves)
    bf16 = _drive(L.LeafStreamBank(m, 3, out_dtype=torch.bfloat16), SCRIPT, waves)
    views = _drive(L.LeafStreamBank(m, 3), SCRIPT, waves, strided=True)
    int_views = _drive(L.LeafStreamBank(m, 3, sample_dtype=torch.int16), SCRIPT, pcm, strided=True)
    for i in range(len(f32)):
        assert from_int[i][2].dtype == torch.float32 and torch.equal(from_int[i][2], from_float[i][2])
        assert bf16[i][2].dtype == torch.bfloat16 and torch.equal(bf16[i][2], f32[i][2].to(torch.bfloat16))
        assert torch.equal(views[i][2], f32[i][2]) and torch.equal(int_views[i][2], from_int[i][2])
    bank = L.LeafStreamBank(m, 3)
    with pytest.raises(ValueError, match="samples"):
        bank.step(pcm[:, None, :160], [160, 0, 0])
    with pytest.raises(ValueError, match="exceeds"):
        bank.step(waves[:, None, :160], [161, 0, 0])
    assert bank.running == [False] * 3 and bank.state_buf is None


@pytest.mark.parametrize("pcm", [False, True])
def test_abi_memory_contract(pcm):
    """The raw entry on guarded, poisoned buffers of exactly the documented sizes: chunk rows hold NaN / full-scale poison behind
    lengths[b], out is B F n_max elements of NaN, the state leaf_stream_state_bytes of 0xFF.  Guards intact, every element of out
    written (zeros behind a row's frames), the frames those of LeafStreamBank, and slot 3 -- idle throughout -- keeps its poison."""
    m, B, K, hop = _module(16000, True, False), 4, 401, 160
    lib = _native.load()
    waves = _waves(4)
    xs = (waves.clamp(-4, 4) * 8000).round().to(torch.int16) if pcm else waves
    es = 2 if pcm else 4
    script = [row + [(0, 0)] for row in SCRIPT]
    script[7][3] = (0, 1)                                                 # `end` on the slot that never runs: still untouched
    want = iter(_drive(L.LeafStreamBank(m, B, sample_dtype=xs.dtype), script, xs))
    flags = _native.FLAG_PCEN | (_native.FLAG_X_PCM16 if pcm else 0)
    sd = m.state_dict()
    prm = [ctypes.c_void_p(sd[k].data_ptr()) for k in PRM]
    nbytes = lib.leaf_stream_state_bytes(B, F, K, hop, flags)
    H = lib.leaf_stream_history_samples(K, hop)
    half = -(-B * H * es // 256) * 256
    state = guarded(nbytes, 0xFF)
    book = L.LeafStreamBank(m, B, sample_dtype=xs.dtype)                  # its host bookkeeping only: nothing is launched through it
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos, frames = [0] * B, [[] for _ in range(B)]
    for i, row in enumerate(script):
        lengths, end = [r[0] for r in row], [bool(r[1]) for r in row]
        running = list(book.running)
        recs, counts = book._plan(lengths, end)
        Tmax, n_max = max(lengths), max(counts)
        chunk = guarded(B * Tmax * es, 0xFF) if Tmax else None            # 0xFF bytes: NaN as float32, -1 as int16
        if Tmax:
            rows = chunk.view(xs.dtype, (B, Tmax))
            for b, n in enumerate(lengths):
                rows[b, :n] = xs[b, pos[b]:pos[b] + n]
                pos[b] += n
        out = guarded(B * F * n_max * 4 if n_max else 64, 0xFF)
        rc = lib.leaf_stream_bank_step_f32(chunk.ptr if Tmax else None, Tmax, B, ctypes.cast(recs, ctypes.c_void_p), n_max, state.ptr, nbytes,
                                           *prm, F, K, hop, flags, out.ptr, stream)
        assert rc == 0, (i, rc)
        torch.cuda.synchronize()
        state.check(f"state, step {i}")
        out.check(f"out, step {i}")
        if Tmax:
            chunk.check(f"chunk, step {i}")
        if n_max:
            got = out.view(torch.float32, (B, F, n_max))
            assert bool(torch.isfinite(got).all()), f"step {i}: an element of out was not written"
            for b in range(B):
                assert bool((got[b, :, counts[b]:] == 0).all()), (i, b)
                frames[b].append(got[b:b + 1, :, :counts[b]].clone())
        else:
            assert bool((out.bytes() == 0xFF).all())
        for b in range(B):
            if end[b] and (running[b] or lengths[b]):
                slot, _, fr = next(want)
                assert slot == b and torch.equal(torch.cat(frames[b], dim=-1), fr), (i, b)
                frames[b] = []
        raw = state.bytes()
        for region, width in ((0, H * es), (half, H * es), (2 * half, F * 4)):
            assert bool((raw[region + 3 * width:region + 4 * width] == 0xFF).all()), f"step {i}: the idle slot's state was written"
    assert next(want, None) is None


def test_a_bank_beyond_one_launch():
    """One slot more than a launch holds (128), F = 2, two short steps: the first slot, the slots on both sides of the split and the
    last one equal their single-stream runs; every slot ends in the second step, every other one on a chunk that completes frames
    (two records), so the records run out before the slots do."""
    m, B = _module(16000, True, False, 2), 129
    waves = _waves(B, 2000, seed=9)
    script = [[(600 + b, 0) for b in range(B)], [(700 if b % 2 else 0, 1) for b in range(B)]]
    done = {b: (ch, fr) for b, ch, fr in _drive(L.LeafStreamBank(m, B), script, waves)}
    assert len(done) == B
    for b in (0, 1, 84, 85, 86, 127, 128):
        chunks, got = done[b]
        want = _single(m, chunks)
        assert got.shape == want.shape and torch.equal(got, want), b
