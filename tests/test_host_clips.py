"""Batch assembly from a packed sample store, the host side (no GPU): the C entry leaf_assemble_clips_f32 as declared and exported,
its argument checks, the validation of a plan that arrives on the CPU, ClipSampler's draws -- and ``assemble_ref``, the CPU oracle of
the assembly that tests/test_gpu_clips.py compares the kernel with.

``assemble_ref`` is built from the library calls the reference's transforms make (numpy.pad 'wrap', torch F.pad 'replicate' /
'constant' with the recording's minimum, slicing, one fp32 multiply, slice assignment) and is itself checked here against the
closed-form index rule of include/leaf_hip.h."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from leaf_pytorch_amd import ClipSampler, PackedClips, _native, transforms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, ALIGNMENT, UNSUPPORTED = -1, -2, -7, -8
ZERO, MIN, REPLICATE, WRAP = 0, 1, 2, 3


# ---- the oracle ------------------------------------------------------------------------------------------------------------------

def widen(store: torch.Tensor) -> torch.Tensor:
    """The store's samples as float32: an int16 sample v means v / 32768 (exact)."""
    store = store.detach().cpu()
    return store.float() / 32768 if store.dtype == torch.int16 else store.clone()


def assemble_ref(store, rec_off, rec_len, start, pad_mode, size, gain=None, masks=None, normalize_fn=None) -> torch.Tensor:
    """(B, size) float32 on the CPU: per clip pad (the reference's calls), crop, gain; then ``normalize_fn`` on the whole batch
    (step 3 is not restated here: the GPU tests pass transforms.PeakNormalization on the device), then the masks."""
    x, S = widen(store), int(size)
    B = len(rec_off)
    gain = None if gain is None else torch.as_tensor(gain, dtype=torch.float32).cpu()
    masks = None if masks is None else torch.as_tensor(masks).cpu()
    out = torch.zeros((B, S), dtype=torch.float32)
    for b in range(B):
        off, L, st, mode = int(rec_off[b]), int(rec_len[b]), int(start[b]), int(pad_mode[b])
        r = x[off:off + L]
        assert r.numel() == L and mode in (ZERO, MIN, REPLICATE, WRAP)
        if L < S:
            left = (S - L) // 2
            right = S - L - left
            if L == 0:
                sig = torch.zeros(S)
            elif mode == WRAP:
                sig = torch.from_numpy(np.pad(r.numpy(), (left, right), "wrap"))
            elif mode == REPLICATE:
                sig = F.pad(r[None, None], (left, right), "replicate")[0, 0]
            else:
                sig = F.pad(r[None], (left, right), "constant", value=float(r.min()) if mode == MIN else 0.0)[0]
        else:
            sig = r
        assert 0 <= st <= sig.numel() - S
        out[b] = sig[st:st + S]
        if gain is not None:
            out[b] = out[b] * gain[b]
    if normalize_fn is not None:
        out = normalize_fn(out).clone()
    if masks is not None:
        for b in range(B):
            for t0, n in masks[b].tolist():
                if n > 0:
                    out[b, max(t0, 0):max(min(t0 + n, S), 0)] = 0
    return out


def clamp_plan(store_len, rec_off, rec_len, start, pad_mode, size):
    """What the kernel makes of a plan it cannot trust (include/leaf_hip.h, MEMORY SAFETY), as Python integers."""
    out = []
    for off, L, st, mode in zip(*(t.tolist() for t in (rec_off, rec_len, start, pad_mode))):
        off = min(max(off, 0), store_len)
        L = min(max(L, 0), store_len - off)
        st = min(max(st, 0), max(L, size) - size)
        out.append((off, L, st, mode if 0 <= mode <= 3 else 0))
    return tuple(torch.tensor(c, dtype=torch.int64) for c in zip(*out))


def closed_form(r, L, S, st, mode, t):
    left = max(S - L, 0) // 2
    j = st + t - left
    if 0 <= j < L:
        return r[j]
    assert L < S
    return (0.0, min(r), r[min(max(j, 0), L - 1)], r[j % L])[mode]          # Python's % is the floor modulus


@pytest.mark.parametrize("L,S", [(1, 4), (3, 11), (5, 6), (7, 16), (16, 16), (17, 16), (40, 16)])
@pytest.mark.parametrize("mode", [ZERO, MIN, REPLICATE, WRAP])
def test_the_oracle_follows_the_closed_form_index_rule(L, S, mode):
    g = torch.Generator().manual_seed(100 * L + S)
    store = torch.cat([torch.full((3,), 9.0), torch.rand(L, generator=g) - 0.25, torch.full((3,), -9.0)])
    r = store[3:3 + L].tolist()
    for st in sorted({0, (max(L, S) - S) // 2, max(L, S) - S}):
        got = assemble_ref(store, [3], [L], [st], [mode], S)
        want = torch.tensor([[closed_form(r, L, S, st, mode, t) for t in range(S)]], dtype=torch.float32)
        assert torch.equal(got, want), (L, S, st, mode)


def test_the_oracle_widens_int16_scales_and_masks():
    store = torch.tensor([32767, -32768, 16384, 1, -1], dtype=torch.int16)
    got = assemble_ref(store, [0], [5], [0], [ZERO], 5, gain=torch.tensor([2.0]), masks=torch.tensor([[[3, 9], [-4, 5], [2, 0], [2, -1]]]))
    assert torch.equal(got, torch.tensor([[0.0, -2.0, 1.0, 0.0, 0.0]]))
    clamped = clamp_plan(10, *(torch.tensor(v) for v in ([-3, 4, 99], [5, 99, 5], [7, -2, 1], [9, 3, -1])), 4)
    assert [c.tolist() for c in clamped] == [[0, 4, 10], [5, 6, 0], [1, 0, 0], [0, 3, 0]]


# ---- the C entry -----------------------------------------------------------------------------------------------------------------

def test_the_entry_is_declared_as_exported():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int leaf_assemble_clips_f32(const void* store, long long store_len, int flags, int B, int size, const long long* rec_off, "
            "const int* rec_len, const int* start, const int* pad_mode, const float* gain, int normalize, const int* masks, int M, "
            "float* out, void* stream);") in flat
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6          # additive: the version stays
    i, v = ctypes.c_int, ctypes.c_void_p
    assert _native._SIGNATURES["leaf_assemble_clips_f32"] == (i, [v, ctypes.c_longlong, i, i, i, v, v, v, v, v, i, v, i, v, v])
    assert "leaf_assemble_clips_f32" in _native.EXPORTED_SYMBOLS
    lib = _native.load()
    fn = lib.leaf_assemble_clips_f32
    assert fn.restype == i and fn.argtypes == _native._SIGNATURES["leaf_assemble_clips_f32"][1]
    assert lib.leaf_abi_version() == 6 and _native.ABI_VERSION == 6
    # the documented cut-over of the resident path, on the three sides that state it
    assert _native.ASSEMBLE_RESIDENT_MAX == 32765 and "32765" in header
    assert "kClipResidentMax = kClipChunks * 4 * kClipThreads - 3" in open(os.path.join(REPO, "leaf_pytorch_amd", "csrc", "leaf_clips.hpp")).read()


def test_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000                                        # never dereferenced: every call below is refused before the launch

    def call(store=p, store_len=100, flags=0, B=2, size=8, rec_off=p, rec_len=p, start=p, pad_mode=p, gain=None, normalize=1, masks=None,
             M=0, out=p):
        return lib.leaf_assemble_clips_f32(store, store_len, flags, B, size, rec_off, rec_len, start, pad_mode, gain, normalize, masks, M, out, None)

    for name in ("store", "rec_off", "rec_len", "start", "pad_mode", "out"):
        assert call(**{name: None}) == NULL_POINTER, name
    assert call(B=0) == BAD_SHAPE and call(B=-1) == BAD_SHAPE and call(size=0) == BAD_SHAPE and call(store_len=-1) == BAD_SHAPE
    assert call(M=-1) == BAD_SHAPE and call(M=2, masks=None) == BAD_SHAPE
    assert call(flags=_native.FLAG_IO_BF16) == UNSUPPORTED and call(flags=_native.FLAG_X_PCM16 | _native.FLAG_PCEN) == UNSUPPORTED
    for name in ("store", "rec_len", "start", "pad_mode", "out", "gain"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(rec_off=p + 4) == ALIGNMENT and call(masks=p + 1, M=1) == ALIGNMENT
    assert call(store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT
    assert call(store=p + 2, flags=_native.FLAG_X_PCM16, B=0) == BAD_SHAPE          # (2-byte alignment is enough for int16: the shape answers)


# ---- the Python layer: a plan on the CPU is validated before anything is launched --------------------------------------------------

STORE = torch.zeros(100, dtype=torch.int16)            # a CPU store: a valid plan gets as far as require_hip and no further


def _assemble(rec_off=(0, 10), rec_len=(10, 40), start=(0, 5), pad_mode=(1, 2), size=16, **kw):
    return _native.assemble_clips(STORE, list(rec_off), list(rec_len), list(start), list(pad_mode), size, **kw)


def test_a_cpu_store_raises_as_everywhere():
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _assemble()
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        PackedClips([STORE[:30], STORE[30:]]).assemble([0, 1, 1], 0, 16)
    with pytest.raises(RuntimeError, match="1-D float32 or int16"):
        _native.assemble_clips(STORE.double(), [0], [10], [0], [0], 16)


@pytest.mark.parametrize("bad", [
    dict(rec_off=(-1, 10)), dict(rec_off=(0, 101)), dict(rec_len=(-1, 40)), dict(rec_len=(10, 91)), dict(rec_off=(0, 100), rec_len=(10, 1)),
    dict(start=(1, 5)), dict(start=(0, 25)), dict(start=(-1, 5)), dict(start=(0, 5), rec_len=(10, 16), pad_mode=(0, 0), size=17),
    dict(pad_mode=(4, 0)), dict(pad_mode=(0, -1)),
    dict(rec_len=(10,)), dict(start=(0, 5, 5)), dict(pad_mode=(1,)), dict(gain=torch.ones(3)),
    dict(masks=torch.zeros((2, 2), dtype=torch.int32)), dict(masks=torch.zeros((3, 1, 2), dtype=torch.int32)),
    dict(masks=torch.zeros((2, 1, 3), dtype=torch.int32)), dict(size=0), dict(size=2 ** 31),
])
def test_a_bad_cpu_plan_raises_value_error_before_the_store_is_looked_at(bad):
    with pytest.raises(ValueError):
        _assemble(**bad)


def test_the_boundaries_of_a_valid_plan_pass_validation():
    # start == max(L, S) - S, a recording that ends with the store, one of length 0 at the store's end, M == 0
    B, rec_off, rec_len, start, pad_mode, gain, masks = _native.clip_plan(100, [0, 60, 100], [10, 40, 0], [0, 24, 0], [3, 0, 1], 16,
                                                                          gain=[1.0, 2.0, 0.5], masks=torch.zeros((3, 0, 2), dtype=torch.int32))
    assert B == 3 and masks is None and gain.dtype == torch.float32 and start.tolist() == [0, 24, 0]
    with pytest.raises(TypeError):
        _native.clip_plan(100, [0.0], [10], [0], [0], 16)
    with pytest.raises(ValueError, match="outside"):
        PackedClips([STORE[:30], STORE[30:]]).assemble([0, 2], 0, 16)
    with pytest.raises(ValueError):
        PackedClips.from_store(STORE, [0, 50], [50, 51])


# ---- PackedClips and ClipSampler -------------------------------------------------------------------------------------------------

LENGTHS = (5, 16, 16, 40, 100, 1, 17)                   # shorter than, equal to and longer than size = 16


def _clips():
    g = torch.Generator().manual_seed(3)
    return PackedClips([torch.randint(-20000, 20000, (n,), dtype=torch.int16, generator=g) for n in LENGTHS])


def _sampler(seed=11, **kw):
    return ClipSampler(_clips(), 16, generator=torch.Generator().manual_seed(seed), **kw)


INDEX = torch.arange(len(LENGTHS)).repeat(40)


def test_packed_clips_layout():
    pc = _clips()
    assert len(pc) == len(LENGTHS) and pc.store.dtype == torch.int16 and pc.store.numel() == sum(LENGTHS)
    assert pc.lengths_host.tolist() == list(LENGTHS) and pc.lengths.dtype == torch.int32 and pc.offsets.dtype == torch.int64
    assert pc.offsets_host.tolist() == [0, 5, 21, 37, 77, 177, 178]
    again = PackedClips.from_store(pc.store, pc.offsets_host, pc.lengths_host)
    assert torch.equal(again.offsets, pc.offsets) and torch.equal(again.lengths, pc.lengths)
    with pytest.raises(TypeError):
        PackedClips([torch.zeros(3), torch.zeros(3, dtype=torch.int16)])
    assert transforms.PackedClips is PackedClips


def test_the_same_seed_gives_the_same_plan_and_another_seed_another():
    kw = dict(num_masks=3, time_perc=0.5, gain_prob=0.5)
    a, b, c = _sampler(11, **kw).plan(INDEX), _sampler(11, **kw).plan(INDEX), _sampler(12, **kw).plan(INDEX)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(a[2:], c[2:]))
    assert (a.rec_off.dtype, a.rec_len.dtype, a.start.dtype, a.pad_mode.dtype, a.gain.dtype, a.masks.dtype) == (
        torch.int64, torch.int32, torch.int32, torch.int32, torch.float32, torch.int32)
    s = _sampler(11, **kw)
    first, second = s.plan(INDEX), s.plan(INDEX)                            # one generator: the stream moves on
    assert not torch.equal(first.start, second.start)


def test_starts_are_in_range_and_cover_it_and_the_validation_split_is_centred():
    p = _sampler().plan(INDEX)
    span = (p.rec_len.long() - 16).clamp(min=0)
    assert torch.equal(p.rec_off, _clips().offsets_host[INDEX]) and torch.equal(p.rec_len, _clips().lengths_host[INDEX])
    assert bool((p.start >= 0).all()) and bool((p.start <= span).all())
    assert bool((p.start[span == 0] == 0).all())
    long = p.start[p.rec_len == 40]
    assert int(long.min()) == 0 and int(long.max()) == 24                   # inclusive at both ends (40 draws over 25 values: seed-pinned)
    assert set(p.start[p.rec_len == 17].tolist()) == {0, 1}
    v = _sampler(train=False).plan(INDEX)
    assert torch.equal(v.start.long(), span // 2)
    _native.clip_plan(sum(LENGTHS), *p[:4], 16, p.gain, p.masks)            # what the sampler draws passes the CPU validation


def test_pad_modes_follow_their_probability():
    p = _sampler().plan(INDEX)
    assert set(p.pad_mode.tolist()) == {REPLICATE, MIN}
    assert set(_sampler(wrap_pad_prob=1.0).plan(INDEX).pad_mode.tolist()) == {REPLICATE}
    assert set(_sampler(wrap_pad_prob=0.0, pad_modes=("wrap", "zero")).plan(INDEX).pad_mode.tolist()) == {ZERO}
    with pytest.raises(KeyError):
        _sampler(pad_modes=("reflect", "min"))


def test_gains():
    lo, hi = (torch.tensor(10.0 ** (db / 20.0), dtype=torch.float32) for db in (-18.0, 6.0))
    g = _sampler(gain_prob=0.5).plan(INDEX).gain
    drawn = g[g != 1.0]
    assert 0.3 < drawn.numel() / g.numel() < 0.7                            # 280 draws at p = 0.5: eight standard deviations
    assert bool((drawn >= lo).all()) and bool((drawn <= hi).all()) and drawn.unique().numel() > 50
    assert bool((_sampler(gain_prob=0.0).plan(INDEX).gain == 1.0).all())
    assert bool((_sampler(gain_prob=1.0).plan(INDEX).gain != 1.0).any())


def test_masks():
    assert _sampler().plan(INDEX).masks is None and _sampler(num_masks=0, time_perc=0.5).plan(INDEX).masks is None
    m = _sampler(num_masks=3, time_perc=0.5).plan(INDEX).masks
    assert tuple(m.shape) == (INDEX.numel(), 3, 2)
    t0, n = m[..., 0], m[..., 1]
    assert bool((n >= 0).all()) and bool((n <= 8).all()) and bool((t0 >= 0).all()) and bool((t0 + n <= 16).all())
    used = (n > 0).sum(1)
    assert int(used.max()) == 3 and int(used.min()) <= 1                     # randint(1, 3) spans: the others carry n = 0
