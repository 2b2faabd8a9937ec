"""LeafStream(fused=True): one leaf_stream_step_f32 launch per step (csrc/leaf_fft_stream.hpp), the recording's history and the
PCEN smoother's state resident in one device buffer between calls.  The stream must give, frame for frame, what Leaf gives for
the whole recording and what the two-launch LeafStream emits step by step; the C entry point keeps the memory contract of
include/leaf_hip.h (exact sizes, every output element written, nothing read that it did not write).

Shapes: T = 2 LS + 3 hop + 7 samples (LS = 1600, the block length at 401 / 160 and 201 / 80), so the buffer [history | chunk]
crosses two block boundaries; the chunk sizes contain steps that emit nothing, chunks that are no multiple of the hop, a chunk of
one block and of one block plus a sample.  n_filters = 6: a workgroup serves one (stream, filter) row whatever F is."""
import ctypes
import functools

import pytest
import torch

import leaf_pytorch_amd as L
from conftest import rel_err
from guarded import guarded
from leaf_pytorch_amd import _native
from leaf_pytorch_amd.streaming import stream_capacity, stream_plan
from oracle import leaf_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STREAM_TOL = 1e-5     # the project's streaming tolerance (tests/test_gpu_dropin.py), restated
ORACLE_TOL = 2e-5     # what the parity tests assert against the oracle
F, B, LS = 6, 2, 1600
BAD_SHAPE = -2


def _sizes(hop):
    return [1, 37, hop, 5, LS, LS + 1, 2, hop * 3 - 1, LS // 2]


def _chunks(T, sizes):
    """[(a, b)] consecutive sample ranges of the cycled chunk sizes."""
    out, pos, i = [], 0, 0
    while pos < T:
        n = min(sizes[i % len(sizes)], T - pos)
        out.append((pos, pos + n))
        pos, i = pos + n, i + 1
    return out


@functools.lru_cache(maxsize=None)
def _case(sample_rate, pcen, log1p):
    """(module, x, whole-clip features, fp64 oracle) -- computed once, shared, never modified."""
    torch.manual_seed(sample_rate + 2 * pcen + log1p)
    m = L.Leaf(n_filters=F, sample_rate=sample_rate, pcen_compression=pcen).eval().to(DEV)
    for p in m.parameters():
        p.requires_grad_(False)
    if log1p:
        m.log_compression()
    hop = m._pooling.strides
    x = torch.randn(B, 1, 2 * LS + 3 * hop + 7, device=DEV)
    with torch.no_grad():
        want = m(x)
    params = {k: v.cpu() for k, v in m.state_dict().items()}
    ref = lo.leaf_forward(x.cpu().double(), params, lo.geometry(F, sample_rate), pcen, torch.float64)
    return m, x, want, (torch.log1p(ref) if log1p else ref)


def _run(stream, x, spans, contiguous=False):
    outs = [stream.step(x[:, :, a:b].contiguous() if contiguous else x[:, :, a:b]) for a, b in spans]
    return outs + [stream.flush()]


@pytest.mark.parametrize("sample_rate,pcen,log1p", [(16000, True, False), (16000, False, False), (16000, False, True), (8000, True, False)])
def test_fused_stream_equals_the_whole_clip(sample_rate, pcen, log1p):
    m, x, want, ref = _case(sample_rate, pcen, log1p)
    spans = _chunks(x.shape[-1], _sizes(m._pooling.strides))
    got = _run(L.LeafStream(m, fused=True), x, spans)
    unfused = _run(L.LeafStream(m), x, spans)
    assert [g.shape for g in got] == [u.shape for u in unfused]           # frame for frame the two-launch stream's steps
    assert any(g.shape[-1] == 0 for g in got[:-1]) and got[-1].shape[-1] > 0
    cat = torch.cat(got, dim=-1)
    assert cat.shape == want.shape and cat.dtype == torch.float32
    err, err_o = rel_err(cat.cpu(), want.cpu()), rel_err(cat.cpu(), ref)
    print(f"fused stream vs whole clip {err:.3e}, vs fp64 oracle {err_o:.3e}")
    assert err < STREAM_TOL, f"stream vs whole clip: {err:.3e}"
    assert err_o < ORACLE_TOL, f"stream vs fp64 oracle: {err_o:.3e}"


def test_state_is_used_and_needs_no_clearing(monkeypatch):
    """The state buffer starts as NaN poison (every byte 0xFF: NaN as float32) and is never cleared: two runs of one stream
    through one object, the second after flush() on top of the first's leftovers, are bit-equal and finite."""
    m, x, want, _ = _case(16000, True, False)
    made = []
    fresh = _native.stream_state
    monkeypatch.setattr(_native, "stream_state", lambda *a: made.append(fresh(*a).fill_(0xFF)) or made[-1])
    spans = _chunks(x.shape[-1], _sizes(160))
    s = L.LeafStream(m, fused=True)
    first = _run(s, x, spans)
    assert len(made) == 1
    second = _run(s, x, spans)
    assert len(made) == 1                                                 # allocated once, kept over flush()
    for a, b in zip(first, second):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert rel_err(torch.cat(first, dim=-1).cpu(), want.cpu()) < STREAM_TOL
    # ... and the state IS used: a stream that forgets it started smooths differently
    s.step(x[:, :, :LS])
    s.started = False
    forgot, remembered = s.step(x[:, :, LS:2 * LS]), torch.cat(first, dim=-1)[:, :, 8:18]
    assert forgot.shape == remembered.shape == (B, F, 10) and not torch.equal(forgot, remembered)
    s.flush()


def test_sample_types_and_feature_dtype():
    m, x, _, _ = _case(16000, True, False)
    spans = _chunks(x.shape[-1], _sizes(160))
    pcm = (x.clamp(-4, 4) * 8000).round().to(torch.int16)
    from_int = _run(L.LeafStream(m, fused=True), pcm, spans)
    from_float = _run(L.LeafStream(m, fused=True), pcm.float() / 32768, spans)
    for a, b in zip(from_int, from_float):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    f32 = _run(L.LeafStream(m, fused=True), x, spans)
    bf16 = _run(L.LeafStream(m, fused=True, out_dtype=torch.bfloat16), x, spans)
    for a, b in zip(bf16, f32):
        assert a.dtype == torch.bfloat16 and torch.equal(a, b.to(torch.bfloat16))
    s = L.LeafStream(m, fused=True)
    s.step(x[:, :, :500])
    with pytest.raises(RuntimeError, match="one sample type per stream"):
        s.step(pcm[:, :, 500:900])
    s.flush()
    s.step(pcm[:, :, :500])                                               # flush() ended the float32 stream: an int16 one may begin


def test_strided_chunks_are_read_in_place():
    m, x, _, _ = _case(16000, True, False)
    spans = _chunks(x.shape[-1], _sizes(160))
    assert not x[:, :, 38:198].is_contiguous()
    views = _run(L.LeafStream(m, fused=True), x, spans)
    copies = _run(L.LeafStream(m, fused=True), x, spans, contiguous=True)
    for a, b in zip(views, copies):
        assert torch.equal(a, b)
    pcm = (x.clamp(-4, 4) * 8000).round().to(torch.int16)
    for a, b in zip(_run(L.LeafStream(m, fused=True), pcm, spans), _run(L.LeafStream(m, fused=True), pcm, spans, contiguous=True)):
        assert torch.equal(a, b)
    # a one-sample chunk whose rows overlap (an expanded view, row stride 0) is copied, not refused
    s = L.LeafStream(m, fused=True)
    assert s.step(x[:1, :, :1].expand(B, 1, 1)).shape == (B, F, 0) and s.hist_len == 1
    s.flush()


@pytest.mark.parametrize("pcm", [False, True])
def test_abi_memory_contract(pcm):
    """The raw entry point on guarded, poisoned buffers of exactly the documented sizes: the state at leaf_stream_state_bytes, out at
    B F n elements; the guards stay intact over a whole stream, every element of out is written, a step with n = 0 leaves out alone;
    the frames are those of LeafStream(fused=True)."""
    m, x, _, _ = _case(16000, True, False)
    K, hop = 401, 160
    lib = _native.load()
    xs = (x.clamp(-4, 4) * 8000).round().to(torch.int16) if pcm else x
    flags = _native.FLAG_PCEN | (_native.FLAG_X_PCM16 if pcm else 0)
    sd = m.state_dict()
    prm = [sd[k].contiguous() for k in ("_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
                                       "_compression.root", "_compression.ema._weights")]
    nbytes = lib.leaf_stream_state_bytes(B, F, K, hop, flags)
    H = lib.leaf_stream_history_samples(K, hop)
    assert nbytes == 2 * (-(-B * H * (2 if pcm else 4) // 256) * 256) + B * F * 4
    state = guarded(nbytes, 0xFF)
    spans = _chunks(x.shape[-1], _sizes(hop))
    want = _run(L.LeafStream(m, fused=True), xs, spans)
    hist, nxt, parity, started = 0, 0, 0, 0
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for i, (a, b) in enumerate(spans + [(0, 0)]):                         # ... and the final step, without samples
        final = i == len(spans)
        Tc = 0 if final else b - a
        first, n, drop, hist2, nxt2 = stream_plan(hist, nxt, Tc, K, hop, final)
        out = guarded(B * F * n * 4 if n else 64, 0xFF)
        chunk = None if final else xs[:, 0, a:b]
        rc = lib.leaf_stream_step_f32(None if final else ctypes.c_void_p(chunk.data_ptr()), B, Tc, 0 if final else chunk.stride(0), state.ptr, nbytes, hist,
                                      parity, drop, first, n, started, *(ctypes.c_void_p(t.data_ptr()) for t in prm), F, K, hop, flags,
                                      out.ptr, stream)
        assert rc == 0, (i, rc)
        torch.cuda.synchronize()
        state.check(f"state, step {i}")
        out.check(f"out, step {i}")
        if n:
            got = out.view(torch.float32, (B, F, n))
            assert bool(torch.isfinite(got).all()), f"step {i}: an element of out was not written"
            assert torch.equal(got, want[i])
        else:
            assert bool((out.bytes() == 0xFF).all()) and want[i].shape[-1] == 0
        hist, nxt, parity, started = hist2, nxt2, parity ^ 1, int(started or n > 0)


def test_over_long_chunks_go_in_pieces():
    """A chunk beyond the one-pass capacity (16000 samples of [history | chunk]): LeafStream(fused=True) feeds it in pieces and still
    matches the whole clip; the raw call with that length is LEAF_ERR_BAD_SHAPE, answered before any launch."""
    m, _, _, _ = _case(16000, True, False)
    cap = stream_capacity(401, 160)
    assert cap == 16000
    torch.manual_seed(11)
    x = torch.randn(1, 1, cap + 700, device=DEV)
    with torch.no_grad():
        want = m(x)
    s = L.LeafStream(m, fused=True)
    got = torch.cat([s.step(x[:, :, :300]), s.step(x[:, :, 300:]), s.flush()], dim=-1)
    assert got.shape == want.shape
    err = rel_err(got.cpu(), want.cpu())
    assert err < STREAM_TOL, f"over-long chunk in pieces vs whole clip: {err:.3e}"
    sd = m.state_dict()
    prm = [ctypes.c_void_p(sd[k].data_ptr()) for k in ("_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha",
                                                       "_compression.delta", "_compression.root", "_compression.ema._weights")]
    state = _native.stream_state(1, F, 401, 160, 0, torch.device(DEV))
    out = torch.empty(1, F, 200, device=DEV)
    step = lambda Tc, hist: _native.load().leaf_stream_step_f32(ctypes.c_void_p(x.data_ptr()), 1, Tc, x.shape[-1], ctypes.c_void_p(state.data_ptr()),
                                                                state.numel(), hist, 0, 0, 0, 1, 0, *prm, F, 401, 160, _native.FLAG_PCEN,
                                                                ctypes.c_void_p(out.data_ptr()), None)
    assert step(cap + 1, 0) == BAD_SHAPE and step(cap - 299, 300) == BAD_SHAPE
