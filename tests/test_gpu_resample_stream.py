"""Chunked resampling on the device: ``ResampleStream`` / ``ResampleStreamBank`` (leaf_resample_stream_step_f32) against ``resample()``
of the concatenated chunks.  An output is one fma chain over its span, a pure function of the recording, so everything here is BIT
equality, for every chunking: there is no tolerance in this file.  The references (``resample`` of the whole signal) are computed
once per (ratio, sample type, output type, length) and shared."""
import ctypes
import random

import numpy as np
import pytest
import torch

import leaf_pytorch_amd as L
from guarded import guarded, guarded_tensor, unchanged
from leaf_pytorch_amd import LeafStream, LeafStreamBank, ResampleStream, ResampleStreamBank, _native, resample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS = [(48000, 16000), (44100, 16000), (44100, 48000), (16000, 8000), (16000, 16000)]
DTYPES = [torch.int16, torch.float32]
IDS = ["int16", "float32"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    _native.load()


def signal(dtype, B: int, T: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        return torch.randint(-32768, 32768, (B, T), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    return (torch.rand(B, T, generator=g, dtype=torch.float32) * 2 - 1).to(DEV)


def bits(t: torch.Tensor) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


_cache = {}


def whole(orig, new, dtype, out_dtype, B, T, seed=11):
    """(the signal, resample() of it): computed once, never modified."""
    key = (orig, new, dtype, out_dtype, B, T, seed)
    if key not in _cache:
        x = signal(dtype, B, T, seed)
        _cache[key] = (x, resample(x, orig, new, out_dtype=out_dtype))
    return _cache[key]


def feed(rs, x: torch.Tensor, sizes) -> torch.Tensor:
    """The chunks of ``x`` by ``sizes`` (the rest in one last chunk) through step, then flush: everything the stream emitted."""
    outs, at = [], 0
    for Tc in list(sizes) + [x.shape[1]]:
        Tc = min(Tc, x.shape[1] - at)
        outs.append(rs.step(x[:, at:at + Tc]))                                  # a view into the recording: read in place
        at += Tc
    outs.append(rs.flush())
    return torch.cat(outs, dim=1)


def chunkings(orig, new, T, seed):
    """All at once; seeded random sizes including 0 and chunks that complete no output; and a chunk of more than 2048 outputs."""
    rng = random.Random(seed)
    sizes, left = [], T
    while left > 0:
        Tc = min(left, rng.choice((0, 1, 2, 3, rng.randrange(0, 60), rng.randrange(0, 1500))))
        sizes.append(Tc)
        left -= Tc
    return {"at once": [], "random": sizes, "a small chunk in front": [37]}


@pytest.mark.parametrize("orig,new", RATIOS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("out_dtype", DTYPES, ids=["to-int16", "to-float32"])
def test_stream_equals_resample_of_the_whole(orig, new, dtype, out_dtype):
    B, T = 2, 5003
    x, want = whole(orig, new, dtype, out_dtype, B, T)
    rs = ResampleStream(orig, new, out_dtype=out_dtype)
    for name, sizes in chunkings(orig, new, T, orig + new).items():
        got = feed(rs, x, sizes)
        assert got.dtype == out_dtype and got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(bits(got), bits(want)), name
    # one sample at a time
    xs, ws = whole(orig, new, dtype, out_dtype, B, 577)
    assert np.array_equal(bits(feed(rs, xs, [1] * 577)), bits(ws))


@pytest.mark.parametrize("orig,new", RATIOS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_chunk_of_three_tiles(orig, new, dtype):
    """One chunk that yields more than 2048 outputs: three tiles, the last partial, behind a first chunk that leaves a history and
    a phase."""
    g = np.gcd(orig, new)
    T = 100 + (2048 + 300) * (orig // g) // (new // g) + 50
    x, want = whole(orig, new, dtype, None, 2, T, seed=5)
    rs = ResampleStream(orig, new)
    first, big, last = rs.step(x[:, :100]), rs.step(x[:, 100:T - 50]), rs.step(x[:, T - 50:])
    assert 2048 < big.shape[1] < 3072
    assert np.array_equal(bits(torch.cat([first, big, last, rs.flush()], dim=1)), bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_taps_from_global_memory_give_the_same_bits(dtype):
    orig, new = 44100, 16000
    x, want = whole(orig, new, dtype, None, 2, 5003)
    rs = ResampleStream(orig, new)
    assert rs.table.taps_in_lds
    rs.table = rs.table.with_global_taps()
    got = feed(rs, x, chunkings(orig, new, 5003, 3)["random"])
    assert not rs.bank.table.taps_in_lds and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("orig,new", RATIOS)
def test_streams_shorter_than_the_filter_and_empty_streams(orig, new):
    width = _native.resample_table(orig, new).width
    rs = ResampleStream(orig, new)
    for T in sorted({0, 1, max(width - 1, 0), width}):
        x, want = whole(orig, new, torch.float32, None, 1, T, seed=2)
        for sizes in ([], [1] * T):
            got = feed(rs, x, sizes)
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (T, sizes)
    assert not rs.open and tuple(rs.flush().shape) == (1, 0)


def test_a_long_chunk_goes_in_pieces():
    x, want = whole(48000, 16000, torch.int16, None, 2, 5003)
    rs = ResampleStream(48000, 16000)
    rs.max_chunk = 1000
    assert np.array_equal(bits(feed(rs, x, [])), bits(want))


# ---- the bank ----------------------------------------------------------------------------------------------------------------------------

def state_rows(bank, b):
    """Slot b's rows of the two history halves, as bytes."""
    es = 2 if bank.sample_dtype == torch.int16 else 4
    half = bank.state_buf.numel() // 2
    row = bank.history * es
    return torch.cat([bank.state_buf[h * half + b * row: h * half + (b + 1) * row] for h in (0, 1)]).clone()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bank_slots_are_independent_streams(dtype):
    """Five slots that begin and end at different steps with chunks of different lengths, fed from a strided view; every slot is
    bit-equal to a one-row ResampleStream fed the same chunks; an idle slot's state rows are unchanged; rows are zero behind counts."""
    orig, new, S, steps, Tmax = 44100, 16000, 5, 9, 1300
    rng = random.Random(17)
    bank = ResampleStreamBank(orig, new, S, sample_dtype=dtype)
    singles = [ResampleStream(orig, new) for _ in range(S)]
    begin, stop = [0, 2, 0, 4, 1], [8, 5, 3, 8, 6]                              # slot 2 ends and stays free; slot 3 begins late
    got, want = [[] for _ in range(S)], [[] for _ in range(S)]
    for step in range(steps):
        store = signal(dtype, S, 2 * Tmax + 6, 100 + step)
        chunk = store[:, 3:3 + 2 * Tmax:2] if step % 2 else store[:, 5:5 + Tmax]   # a strided view / a view with a row stride
        lengths, end = [0] * S, [False] * S
        for b in range(S):
            if begin[b] <= step <= stop[b]:
                lengths[b] = 0 if (b == 0 and step in (3, 4)) else rng.choice((1, 7, 300, 441, Tmax, rng.randrange(1, Tmax)))
                end[b] = step == stop[b]
        idle = [b for b in range(S) if lengths[b] == 0 and not (end[b] and bank.running[b])]
        before = {b: state_rows(bank, b) for b in idle} if bank.state_buf is not None else {}
        y, counts = bank.step(chunk, lengths, end)
        assert tuple(y.shape) == (S, max(counts)) and y.dtype == dtype
        for b in range(S):
            assert not y[b, counts[b]:].any(), (step, b)                        # zeros behind counts[b]
            got[b].append(y[b:b + 1, :counts[b]])
            if b in idle:
                assert counts[b] == 0 and (b not in before or torch.equal(state_rows(bank, b), before[b])), (step, b)
                continue
            want[b].append(singles[b].step(chunk[b:b + 1, :lengths[b]].contiguous()))
            if end[b]:
                want[b].append(singles[b].flush())
        assert bank.running == [begin[b] <= step < stop[b] for b in range(S)]
    for b in range(S):
        a, w = torch.cat(got[b], dim=1), torch.cat(want[b], dim=1)
        assert a.shape == w.shape and a.shape[1] > 0 and np.array_equal(bits(a), bits(w)), b


def test_bank_of_more_than_one_launch():
    """130 slots: two launches (128 slots each at the most), every slot its own stream."""
    orig, new, S = 48000, 16000, 130
    x, want = whole(orig, new, torch.int16, None, S, 700, seed=9)
    bank = ResampleStreamBank(orig, new, S, sample_dtype=torch.int16)
    y0, c0 = bank.step(x[:, :301], [301] * S)
    y1, c1 = bank.step(x[:, 301:], [399] * S, [True] * S)
    assert c0 == [c0[0]] * S and c1 == [c1[0]] * S and c0[0] + c1[0] == want.shape[1]
    assert np.array_equal(bits(torch.cat([y0, y1], dim=1)), bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("out_dtype", DTYPES, ids=["to-int16", "to-float32"])
def test_abi_memory_contract(dtype, out_dtype):
    """leaf_resample_stream_step_f32 on exact-size guarded state, chunk and out, at the least alignment the header promises: the
    guards stay intact, the chunk is not modified, samples behind Tc[b] in a chunk row are never read (they are NaN / full scale and
    would show), an idle slot's state rows keep their poison, and every element of out is written."""
    orig, new, B = 44100, 16000, 3
    key = (orig, new, 6, 0.99)
    lib = _native.load()
    table = _native.resample_table(*key)
    words = table.on(DEV)
    es, eo = (2 if dtype == torch.int16 else 4), (2 if out_dtype == torch.int16 else 4)
    flags = (_native.FLAG_X_PCM16 if dtype == torch.int16 else 0) | (_native.FLAG_OUT_PCM16 if out_dtype == torch.int16 else 0)
    T = [1500, 0, 1201]                                                         # slot 1 stays idle
    x, want = whole(orig, new, dtype, out_dtype, B, 1500, seed=21)
    want2 = resample(x[2:3, :1201], orig, new, out_dtype=out_dtype)
    state = guarded(lib.leaf_resample_stream_state_bytes(B, *key, flags), 0x5A, offset=16)
    pos = (_native.ResamplePos * B)()
    outs = [[], [], []]
    stride = 1000
    for at, last in ((0, False), (700, True)):
        lengths = [min(700, T[b] - at) if not last else T[b] - at for b in range(B)]
        lengths[1] = 0
        rows = torch.full((B, stride), float("nan"), device=DEV) if dtype == torch.float32 else torch.full((B, stride), 32767, dtype=torch.int16, device=DEV)
        for b in range(B):
            rows[b, :lengths[b]] = x[b, at:at + lengths[b]]
        flat = rows.reshape(-1)[:(B - 1) * stride + lengths[B - 1]]             # exactly up to the last row's last sample
        chunk = guarded_tensor(flat, offset=es)
        recs, counts = _native.resample_stream_plan(key, pos, lengths, [last] * B)
        n_max = max(counts)
        out = guarded(B * n_max * eo, 0xEE, offset=eo)
        with torch.cuda.device(DEV):
            rc = lib.leaf_resample_stream_step_f32(chunk.ptr, stride, B, ctypes.cast(recs, ctypes.c_void_p), n_max, state.ptr, state.nbytes, flags,
                                                   *key, ctypes.c_void_p(words.data_ptr()), words.numel() * 4, out.ptr,
                                                   _native.stream_ptr(torch.device(DEV)))
        assert rc == 0
        torch.cuda.synchronize()
        state.check("state")
        unchanged(chunk, "chunk")
        out.check("out")
        y = out.cpu(out_dtype, (B, n_max))
        for b in range(B):
            assert not y[b, counts[b]:].any()
            outs[b].append(y[b, :counts[b]])
    assert np.array_equal(bits(torch.cat(outs[0])), bits(want[0])) and np.array_equal(bits(torch.cat(outs[2])), bits(want2[0]))
    assert torch.cat(outs[1]).numel() == 0
    H, half = 474, state.nbytes // 2
    sb = state.bytes()
    for h in (0, 1):                                                            # the idle slot's rows: still the poison
        assert bool((sb[h * half + H * es: h * half + 2 * H * es] == 0x5A).all())


# ---- composition ---------------------------------------------------------------------------------------------------------------------------

def test_microphone_to_frames():
    """44.1 kHz int16 chunks through ResampleStreamBank into LeafStreamBank: the frames of LeafStream(fused=True) on resample(whole),
    bit for bit.  Three slots, about 1.2 s of audio each, ending at different steps."""
    orig, new, S, chunk = 44100, 16000, 3, 4410
    leaf = L.Leaf(n_filters=40, sample_rate=16000).eval().to(DEV)
    for p in leaf.parameters():
        p.requires_grad_(False)
    T = [52920, 50000, 47003]
    x, _ = whole(orig, new, torch.int16, None, S, max(T), seed=33)
    rbank = ResampleStreamBank(orig, new, S, sample_dtype=torch.int16)
    lbank = LeafStreamBank(leaf, S, sample_dtype=torch.int16)
    frames, parts = [[] for _ in range(S)], [[] for _ in range(S)]
    for at in range(0, max(T), chunk):
        lengths = [max(0, min(chunk, T[b] - at)) for b in range(S)]
        end = [0 < T[b] - at <= chunk for b in range(S)]
        y, counts = rbank.step(x[:, at:at + chunk], lengths, end)
        f, fcounts = lbank.step(y, counts, end)
        for b in range(S):
            frames[b].append(f[b:b + 1, :, :fcounts[b]])
            parts[b].append(counts[b])
    assert rbank.running == [False] * S and lbank.running == [False] * S
    for b in range(S):
        y16 = resample(x[b:b + 1, :T[b]], orig, new)
        assert sum(parts[b]) == y16.shape[1]
        ref, want, at = LeafStream(leaf, fused=True), [], 0
        for n in parts[b]:                                                      # the same recording, cut where the bank's steps cut it
            if n:
                want.append(ref.step(y16[:, at:at + n]))
            at += n
        want.append(ref.flush())
        a, w = torch.cat(frames[b], dim=2), torch.cat(want, dim=2)
        assert a.shape == w.shape and a.shape[2] == (y16.shape[1] - 1) // 160 + 1 and np.array_equal(bits(a), bits(w)), b
