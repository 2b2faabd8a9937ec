"""Host side of the one-launch streaming step (no GPU): stream_plan's arithmetic against a brute-force model of a stream, the
three C entry points' export and their argument checks (dummy host pointers: everything here is answered before any launch), and
the construction-time checks of LeafStream(fused=...)."""
import ctypes
import os
import random
import re

import pytest
import torch

import leaf_pytorch_amd as L
from leaf_pytorch_amd import _native
from leaf_pytorch_amd.streaming import stream_capacity, stream_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, WORKSPACE, ALIGNMENT, UNSUPPORTED = -1, -2, -3, -7, -8


@pytest.mark.parametrize("K,hop", [(401, 160), (201, 80), (552, 220)])
def test_stream_plan_against_a_brute_force_stream(K, hop):
    """Seeded random chunk sequences.  The model keeps the ABSOLUTE sample offset of the history and counts arrivals; every frame
    0 .. (T - 1) // hop must come out exactly once, in order, never before sample m hop + reach has arrived (unless final), and
    the history must fit leaf_stream_history_samples."""
    H = _native.load().leaf_stream_history_samples(K, hop)
    pad_l = K // 2 + K % 2 - 1
    reach, lead = 2 * (K - 1 - pad_l), -(-2 * pad_l // hop)
    assert H == reach + lead * hop
    rng = random.Random(1000 * K + hop)
    for trial in range(60):
        sizes = [rng.choice([1, 2, 7, hop - 1, hop, hop + 1, 3 * hop - 1, K, rng.randrange(1, 4000)]) for _ in range(rng.randrange(1, 25))]
        T = sum(sizes)
        hist, nxt, start, arrived, emitted = 0, 0, 0, 0, []               # start: absolute index of the history's first sample
        for Tc in sizes + [0]:
            final = Tc == 0
            first, n, drop, hist2, nxt2 = stream_plan(hist, nxt, Tc, K, hop, final)
            arrived += Tc
            assert start % hop == 0 and first == nxt and n >= 0 and 0 <= drop <= hist + Tc
            for m in range(first, first + n):
                g = start // hop + m                                      # the frame's number in the recording
                emitted.append(g)
                assert final or g * hop + reach <= arrived - 1, (trial, g)
                # ... and its receptive field starts inside the buffer, or at the recording's first sample
                assert start == 0 or m * hop - 2 * pad_l >= 0, (trial, g)
            if final:
                assert (hist2, nxt2) == (0, 0)
            else:
                assert hist2 == hist + Tc - drop and 0 <= hist2 <= H, (trial, hist2)
                start += drop
                # the next frame keeps its number in the recording
                assert start // hop + nxt2 == (emitted[-1] + 1 if emitted else 0)
            hist, nxt = hist2, nxt2
        assert emitted == list(range((T - 1) // hop + 1)), (trial, sizes)


def test_the_three_symbols_are_exported_with_the_headers_signatures():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert "int leaf_stream_history_samples(int K, int hop);" in flat
    assert "size_t leaf_stream_state_bytes(int B, int F, int K, int hop, int flags);" in flat
    assert ("int leaf_stream_step_f32(const void* chunk, int B, int Tc, long long chunk_stride, void* state, size_t state_bytes, int hist_len, "
            "int parity, int drop_samples, int first, int n, int started, const float* kernel, const float* pool_w, const float* pool_b, "
            "const float* alpha, const float* delta, const float* root, const float* ema_w, int F, int K, int hop, int flags, void* out, "
            "void* stream);") in flat
    assert "#define LEAF_ABI_VERSION 6" in header
    lib = _native.load()
    i, v, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {"leaf_stream_history_samples": (i, [i, i]),
            "leaf_stream_state_bytes": (z, [i] * 5),
            "leaf_stream_step_f32": (i, [v, i, i, ctypes.c_longlong, v, z] + [i] * 6 + [v] * 7 + [i] * 4 + [v, v])}
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert name in _native.EXPORTED_SYMBOLS and fn.restype == res and fn.argtypes == args, name
    assert lib.leaf_abi_version() == 6


def test_state_bytes_and_history_samples():
    lib = _native.load()
    assert lib.leaf_stream_history_samples(401, 160) == 880 and lib.leaf_stream_history_samples(201, 80) == 440
    assert lib.leaf_stream_state_bytes(2, 40, 552, 220, 0) == 0           # no kernel for 22.05 kHz
    assert lib.leaf_stream_state_bytes(2, 40, 801, 320, 0) == 0
    for B, F, K, hop in ((1, 40, 401, 160), (3, 6, 201, 80), (16, 40, 401, 160)):
        H = lib.leaf_stream_history_samples(K, hop)
        for flags, es in ((0, 4), (_native.FLAG_X_PCM16, 2), (_native.FLAG_PCEN | _native.FLAG_OUT_BF16, 4)):
            half = -(-B * H * es // 256) * 256                            # every region starts at a multiple of 256 bytes
            assert lib.leaf_stream_state_bytes(B, F, K, hop, flags) == 2 * half + B * F * 4
    assert lib.leaf_stream_state_bytes(2, 40, 401, 160, _native.FLAG_IO_BF16) == 0
    assert stream_capacity(401, 160) == 16000 and stream_capacity(201, 80) == 16000


def test_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    host = (ctypes.c_char * 4096)()
    b = ctypes.addressof(host)
    b += (-b) % 64
    ok, P = ctypes.c_void_p(b), lambda off: ctypes.c_void_p(b + off)
    B, F, K, hop = 2, 40, 401, 160
    nbytes = lib.leaf_stream_state_bytes(B, F, K, hop, 0)

    def step(chunk=ok, Tc=160, stride=160, state=ok, state_bytes=nbytes, hist=880, parity=0, drop=160, first=3, n=1, started=1, prm=None,
             geo=(F, K, hop), flags=_native.FLAG_PCEN, out=ok, B_=B):
        p = [ok] * 7
        if prm is not None:
            p[prm[0]] = prm[1]
        return lib.leaf_stream_step_f32(chunk, B_, Tc, stride, state, state_bytes, hist, parity, drop, first, n, started, *p, *geo, flags, out, None)

    # NULL pointers (chunk only when samples arrive, out only when frames leave, the PCEN parameters only with PCEN)
    assert step(state=None) == NULL_POINTER and step(chunk=None) == NULL_POINTER and step(out=None) == NULL_POINTER
    for i in range(7):
        assert step(prm=(i, None)) == NULL_POINTER, i
    # alignment: the state 16 bytes; chunk and out by element; parameters 4 bytes
    for off in (4, 8, 12):
        assert step(state=P(off)) == ALIGNMENT, off
    assert step(chunk=P(2)) == ALIGNMENT and step(chunk=P(1), flags=_native.FLAG_PCEN | _native.FLAG_X_PCM16) == ALIGNMENT
    assert step(out=P(2)) == ALIGNMENT and step(out=P(1), flags=_native.FLAG_PCEN | _native.FLAG_OUT_BF16) == ALIGNMENT
    assert step(prm=(3, P(2))) == ALIGNMENT
    # what passes those checks is refused next for its size (a 0-byte state): nothing is launched from here
    assert step(state=P(16), state_bytes=0) == WORKSPACE and step(chunk=P(4), state_bytes=0) == WORKSPACE
    assert step(chunk=P(2), flags=_native.FLAG_PCEN | _native.FLAG_X_PCM16, state_bytes=0) == WORKSPACE
    assert step(out=P(2), flags=_native.FLAG_PCEN | _native.FLAG_OUT_BF16, state_bytes=0) == WORKSPACE
    assert step(state_bytes=nbytes - 1) == WORKSPACE
    # positions that would read or write outside the state, the chunk or out
    assert step(hist=881) == BAD_SHAPE and step(hist=-1) == BAD_SHAPE
    assert step(drop=880 + 160 + 1) == BAD_SHAPE and step(drop=-1) == BAD_SHAPE
    assert step(drop=159) == BAD_SHAPE                                    # the new history would be 881 samples
    assert step(parity=2) == BAD_SHAPE and step(started=2) == BAD_SHAPE
    assert step(first=7, n=1) == BAD_SHAPE and step(first=0, n=8) == BAD_SHAPE and step(n=-1) == BAD_SHAPE   # 1040 samples hold frames 0 .. 6
    assert step(Tc=-1) == BAD_SHAPE and step(Tc=160, stride=159) == BAD_SHAPE
    assert step(Tc=16001, stride=16001, hist=0) == BAD_SHAPE and step(Tc=15121, stride=15121) == BAD_SHAPE   # one pass: 16000 samples
    assert step(B_=-1) == BAD_SHAPE and step(geo=(0, K, hop)) == BAD_SHAPE and step(B_=65536) == BAD_SHAPE
    # the empty batch launches nothing; unsupported flags and geometries are answered first
    assert step(B_=0, chunk=None, state=None, out=None) == 0
    for flag in (_native.FLAG_IO_BF16, _native.FLAG_PEAKNORM):
        assert step(flags=_native.FLAG_PCEN | flag) == UNSUPPORTED and step(flags=flag, state=None) == UNSUPPORTED
    assert step(geo=(F, 552, 220)) == UNSUPPORTED and step(geo=(F, 801, 320), B_=0) == UNSUPPORTED
    del host


def test_leafstream_construction():
    with pytest.raises(ValueError, match="one-launch"):
        L.LeafStream(L.Leaf(sample_rate=22050), fused=True)
    with pytest.raises(ValueError):
        L.LeafStream(L.Leaf(sample_rate=32000), fused=True)
    with pytest.raises(ValueError, match="fused=True"):
        L.LeafStream(L.Leaf(), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        L.LeafStream(L.Leaf(), fused=True, out_dtype=torch.float16)
    m = L.Leaf()
    s = L.LeafStream(m)
    assert type(s) is L.LeafStream and type(L.LeafStream(m, False, False)) is L.LeafStream
    # fused=False: exactly the attributes the class had before the fused path existed
    assert set(vars(s)) == {"leaf", "K", "hop", "F", "pad_l", "pad_r", "lead", "reach", "log1p", "buf", "next", "state", "started"}
    assert (s.K, s.hop, s.F, s.pad_l, s.pad_r, s.lead, s.reach, s.log1p, s.buf, s.next, s.state, s.started) == \
        (401, 160, 40, 200, 200, 3, 400, False, None, 0, None, False)
    f = L.LeafStream(m, fused=True, out_dtype=torch.bfloat16)
    assert isinstance(f, L.LeafStream) and f.out_dtype is torch.bfloat16 and f.state_buf is None and f.capacity == 16000
    assert L.LeafStream(L.Leaf(sample_rate=8000), fused=True).out_dtype is torch.float32
    with pytest.raises(RuntimeError):                                     # no CPU path, fused or not
        f.step(torch.zeros(1, 1, 160))
