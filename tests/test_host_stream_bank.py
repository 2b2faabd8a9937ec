"""Host side of the stream bank (no GPU): the header's struct and entry against the exported signature, the C entry's argument
checks (dummy host pointers: everything here is answered before any launch), LeafStreamBank's per-slot bookkeeping against a
brute-force model of independent streams, and its construction-time and step-time refusals."""
import ctypes
import os
import random
import re

import pytest
import torch

import leaf_pytorch_amd as L
from leaf_pytorch_amd import _native
from leaf_pytorch_amd.streaming import stream_capacity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, WORKSPACE, ALIGNMENT, UNSUPPORTED = -1, -2, -3, -7, -8
FIELDS = ("idle", "hist_len", "Tc", "parity", "drop_samples", "first", "n", "started", "end_first", "end_n")


def test_the_struct_and_the_entry_are_declared_as_exported():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("typedef struct leaf_stream_slot { int idle; int hist_len, Tc, parity, drop_samples, first, n, started; int end_first, end_n; } "
            "leaf_stream_slot;") in flat
    assert ("int leaf_stream_bank_step_f32(const void* chunk, long long chunk_stride, int B, const leaf_stream_slot* slots, int n_max, void* state, "
            "size_t state_bytes, const float* kernel, const float* pool_w, const float* pool_b, const float* alpha, const float* delta, "
            "const float* root, const float* ema_w, int F, int K, int hop, int flags, void* out, void* stream);") in flat
    assert "#define LEAF_ABI_VERSION 6" in header
    lib = _native.load()
    i, v, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    fn = lib.leaf_stream_bank_step_f32
    assert "leaf_stream_bank_step_f32" in _native.EXPORTED_SYMBOLS and fn.restype == i
    assert fn.argtypes == [v, ctypes.c_longlong, i, v, i, v, z] + [v] * 7 + [i] * 4 + [v, v]
    assert tuple(n for n, _ in _native.StreamSlot._fields_) == FIELDS and ctypes.sizeof(_native.StreamSlot) == 4 * len(FIELDS)
    assert lib.leaf_abi_version() == 6 and _native.ABI_VERSION == 6


def test_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    host = (ctypes.c_char * 4096)()
    base = ctypes.addressof(host)
    base += (-base) % 64
    ok, P = ctypes.c_void_p(base), lambda off: ctypes.c_void_p(base + off)
    B, F, K, hop = 3, 40, 401, 160
    nbytes = lib.leaf_stream_state_bytes(B, F, K, hop, 0)
    good = dict(idle=0, hist_len=880, Tc=160, parity=0, drop_samples=160, first=3, n=1, started=1, end_first=0, end_n=0)

    def step(slot1=None, chunk=ok, stride=160, state=ok, state_bytes=nbytes, n_max=1, prm=None, geo=(F, K, hop), flags=_native.FLAG_PCEN, out=ok,
             B_=B, slots="auto", idle0=False):
        recs = (_native.StreamSlot * max(B_, 1))()
        for b in range(max(B_, 1)):
            for k, val in dict(good, **(slot1 or {}) if b == 1 else good).items():
                setattr(recs[b], k, val)
        recs[0].idle = int(idle0)
        p = [ok] * 7
        if prm is not None:
            p[prm[0]] = prm[1]
        sl = ctypes.cast(recs, ctypes.c_void_p) if slots == "auto" else slots
        return lib.leaf_stream_bank_step_f32(chunk, stride, B_, sl, n_max, state, state_bytes, *p, *geo, flags, out, None)

    # NULL pointers (chunk only when a slot has samples, out only when n_max > 0, the PCEN parameters only with PCEN)
    assert step(state=None) == NULL_POINTER and step(chunk=None) == NULL_POINTER and step(out=None) == NULL_POINTER and step(slots=None) == NULL_POINTER
    for i in range(7):
        assert step(prm=(i, None)) == NULL_POINTER, i
    # alignment: the state 16 bytes; chunk and out by element; parameters 4 bytes
    for off in (4, 8, 12):
        assert step(state=P(off)) == ALIGNMENT, off
    assert step(chunk=P(2)) == ALIGNMENT and step(chunk=P(1), flags=_native.FLAG_PCEN | _native.FLAG_X_PCM16) == ALIGNMENT
    assert step(out=P(2)) == ALIGNMENT and step(out=P(1), flags=_native.FLAG_PCEN | _native.FLAG_OUT_BF16) == ALIGNMENT
    assert step(prm=(3, P(2))) == ALIGNMENT
    # what passes those checks is refused next for its size: nothing is launched from here
    assert step(state=P(16), state_bytes=0) == WORKSPACE and step(chunk=P(4), state_bytes=0) == WORKSPACE
    assert step(state_bytes=nbytes - 1) == WORKSPACE
    # ONE slot out of range among good ones refuses the call: every position leaf_stream_step_f32 refuses ...
    for bad in (dict(hist_len=881), dict(hist_len=-1), dict(drop_samples=1041), dict(drop_samples=-1), dict(drop_samples=159), dict(parity=2),
                dict(started=2), dict(first=7, n=1), dict(first=0, n=8), dict(n=-1), dict(Tc=-1), dict(Tc=161), dict(Tc=15121), dict(idle=2),
                # ... a slot's frames beyond n_max, and an ending pass outside the buffer it reads (160 + 880 - 160 samples: frames 0 .. 5)
                dict(n=2), dict(end_first=3, end_n=1), dict(end_first=6, end_n=1), dict(end_first=0, end_n=7), dict(end_n=-1)):
        assert step(slot1=bad, state_bytes=0) == BAD_SHAPE, bad
    assert step(slot1=dict(end_first=5, end_n=1), n_max=2, state_bytes=0) == WORKSPACE      # inside the buffer, inside n_max
    assert step(slot1=dict(drop_samples=0, end_first=3, end_n=1), n_max=2, state_bytes=0) == WORKSPACE   # an ending pass keeps nothing: no bound on the rest
    assert step(slot1=dict(idle=1, hist_len=-5, Tc=-1, n=99), state_bytes=0) == WORKSPACE   # an idle slot's other fields are not looked at
    assert step(n_max=-1) == BAD_SHAPE and step(geo=(0, K, hop)) == BAD_SHAPE and step(B_=-1) == BAD_SHAPE
    assert step(n_max=40000, state_bytes=0) == BAD_SHAPE                                    # the kernel's LDS at n_max
    # the empty bank launches nothing; unsupported flags and geometries are answered first
    assert step(B_=0, chunk=None, state=None, out=None, slots=None) == 0
    for flag in (_native.FLAG_IO_BF16, _native.FLAG_PEAKNORM):
        assert step(flags=_native.FLAG_PCEN | flag) == UNSUPPORTED and step(flags=flag, state=None) == UNSUPPORTED
    assert step(geo=(F, 552, 220)) == UNSUPPORTED and step(geo=(F, 801, 320), B_=0) == UNSUPPORTED
    del host


class _Model:
    """One stream, brute force: the absolute sample count and the frames emitted so far."""

    def __init__(self):
        self.arrived, self.emitted = 0, 0


@pytest.mark.parametrize("K,hop,sr", [(401, 160, 16000), (201, 80, 8000)])
def test_bookkeeping_against_independent_brute_force_streams(K, hop, sr):
    """Seeded random schedules of begin / chunk / idle / end per slot through LeafStreamBank._plan (integers alone).  Per stream:
    frames 0 .. (T - 1) // hop come out exactly once and in order, never before sample m hop + reach has arrived unless the stream
    ends; the history stays within H; the records are those a one-stream LeafStream would pass; parity flips exactly on the steps
    that touched the slot."""
    H = _native.load().leaf_stream_history_samples(K, hop)
    pad_l = K // 2 + K % 2 - 1
    reach = 2 * (K - 1 - pad_l)
    B = 5
    rng = random.Random(K)
    bank = L.LeafStreamBank(L.Leaf(n_filters=4, sample_rate=sr), B)
    assert bank.max_chunk == stream_capacity(K, hop) - H and bank.running == [False] * B
    model = [None] * B
    finished = 0
    for step in range(400):
        lengths = [rng.choice([0, 0, 1, 2, hop - 1, hop, hop + 1, 3 * hop - 1, K, 1600, rng.randrange(1, 4000)]) for _ in range(B)]
        end = [rng.random() < 0.15 for _ in range(B)]
        parity = list(bank.parity)
        recs, counts = bank._plan(lengths, end)
        for b in range(B):
            r, Tc = recs[b], lengths[b]
            touched = Tc > 0 or (end[b] and model[b] is not None)
            assert bank.parity[b] == parity[b] ^ int(touched), (step, b)
            if not touched:
                assert r.idle == 1 and counts[b] == 0
                continue
            if model[b] is None:
                model[b] = _Model()
                assert (r.hist_len, r.started) == (0, 0), (step, b)       # a new stream reads nothing stale
            m = model[b]
            assert r.idle == 0 and r.Tc == Tc and r.parity == parity[b] and 0 <= r.hist_len <= H
            assert r.started == int(m.emitted > 0)
            # the buffer [history | chunk] starts a whole number of hops into the recording
            start = m.arrived - r.hist_len
            assert start % hop == 0 and start >= 0
            m.arrived += Tc
            got = [start // hop + r.first + k for k in range(r.n)]
            if r.end_n:
                assert end[b] and r.n > 0 and r.drop_samples % hop == 0
                got += [(start + r.drop_samples) // hop + r.end_first + k for k in range(r.end_n)]
            assert counts[b] == len(got) and got == list(range(m.emitted, m.emitted + len(got))), (step, b)
            m.emitted += len(got)
            if end[b]:
                assert m.emitted == (m.arrived - 1) // hop + 1, (step, b)  # every frame of the clip
                assert not bank.running[b] and (bank.hist_len[b], bank.next[b], bank.started[b]) == (0, 0, False)
                assert r.end_n > 0 or r.drop_samples == r.hist_len + Tc
                model[b] = None
                finished += 1
            else:
                assert all(g * hop + reach <= m.arrived - 1 for g in got), (step, b)
                assert m.emitted == max(0, (m.arrived - 1 - reach) // hop + 1)
                assert bank.running[b] and bank.hist_len[b] == r.hist_len + Tc - r.drop_samples <= H
                assert bank.started[b] == (m.emitted > 0)
    assert finished > 50


def test_construction_and_step_refusals():
    with pytest.raises(ValueError, match="one-launch"):
        L.LeafStreamBank(L.Leaf(sample_rate=22050), 4)
    with pytest.raises(ValueError):
        L.LeafStreamBank(L.Leaf(sample_rate=32000), 4)
    with pytest.raises(ValueError, match="out_dtype"):
        L.LeafStreamBank(L.Leaf(), 4, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="sample_dtype"):
        L.LeafStreamBank(L.Leaf(), 4, sample_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        L.LeafStreamBank(L.Leaf(), 0)
    bank = L.LeafStreamBank(L.Leaf(n_filters=4), 2, out_dtype=torch.bfloat16)
    assert bank.out_dtype is torch.bfloat16 and bank.state_buf is None and bank.max_chunk == 16000 - 880 and bank.running == [False, False]
    assert L.LeafStreamBank(L.Leaf(n_filters=4, sample_rate=8000), 2, sample_dtype=torch.int16).max_chunk == 16000 - 440
    with pytest.raises(ValueError, match="max_chunk"):                    # before anything is launched or moved
        bank.step(torch.zeros(2, 1, 16000), [160, bank.max_chunk + 1])
    with pytest.raises(ValueError, match="max_chunk"):
        bank._plan([160, bank.max_chunk + 1], None)
    with pytest.raises(ValueError):
        bank._plan([160], None)
    assert bank.running == [False, False] and bank.parity == [0, 0]
    with pytest.raises(RuntimeError):                                     # no CPU path
        bank.step(torch.zeros(2, 1, 160), [160, 160])
    pcm_bank = L.LeafStreamBank(L.Leaf(n_filters=4), 2, sample_dtype=torch.int16)
    with pytest.raises((ValueError, RuntimeError)):                       # a float32 chunk for an int16 bank (on the CPU besides)
        pcm_bank.step(torch.zeros(2, 1, 160), [160, 160])
    assert pcm_bank.running == [False, False] and bank.running == [False, False]
