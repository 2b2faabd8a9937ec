"""Whole-recording evaluation batches, the host side (no GPU): the plan integers of ``PackedClips.segments``, the two C entries
leaf_clip_peaks_f32 / leaf_assemble_segments_f32 as declared and exported with their argument checks, ``segment_mean``, the packing
of ``evaluate_recordings`` -- and ``segments_ref``, the CPU oracle tests/test_gpu_segments.py compares the kernel with.

``segments_ref`` is written from the reference's test.py: per recording the (optional) whole-recording normalisation, pad_input's
``F.pad(..., (left, P - L - left), 'replicate')`` and ``reshape(-1, size)``.  It is itself checked here against the closed form of
include/leaf_hip.h, ``r[clamp(k * size - left + t, 0, L - 1)]``."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import leaf_pytorch_amd
from leaf_pytorch_amd import PackedClips, _native, evaluate_recordings, segment_mean, transforms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, WORKSPACE, ALIGNMENT, UNSUPPORTED = -1, -2, -3, -7, -8
SHAPES = [(1, 4), (3, 4), (4, 4), (5, 4), (7, 4), (8, 4), (9, 4), (23, 5)]          # (L, S): no, even and odd paddings


# ---- the oracle ------------------------------------------------------------------------------------------------------------------

def widen(store: torch.Tensor) -> torch.Tensor:
    store = store.detach().cpu()
    return store.float() / 32768 if store.dtype == torch.int16 else store.clone()


def pad_input(r: torch.Tensor, size: int) -> torch.Tensor:
    """test.py's pad_input on a 1-D recording: (n, size)."""
    L = r.numel()
    n = -(-L // size)
    P = n * size
    left = (P - L) // 2
    return F.pad(r[None, None], (left, P - L - left), "replicate").reshape(-1, size)


def segments_ref(store, off, length, index, size, normalize_fn=None):
    """((sum n_i, size) float32 on the CPU, counts): per recording ``normalize_fn`` on the whole recording (a (1, L) batch), then
    pad_input."""
    x = widen(store)
    rows = []
    for i in index:
        r = x[int(off[i]):int(off[i]) + int(length[i])]
        assert r.numel() == int(length[i]) > 0
        if normalize_fn is not None:
            r = normalize_fn(r[None]).reshape(-1).cpu()
        rows.append(pad_input(r, size))
    return torch.cat(rows), torch.tensor([r.shape[0] for r in rows], dtype=torch.int64)


def clamp_segment_plan(store_len, rec_off, rec_len, win, rec, size, R):
    """What the kernel makes of a plan it cannot trust (include/leaf_hip.h, MEMORY SAFETY), as Python integers."""
    out = []
    for off, L, w, i in zip(*(t.tolist() for t in (rec_off, rec_len, win, rec))):
        off = min(max(off, 0), store_len)
        L = min(max(L, 0), store_len - off)
        out.append((off, L, min(max(w, -size), L), min(max(i, 0), R - 1)))
    return tuple(torch.tensor(c, dtype=torch.int64) for c in zip(*out))


def rows_ref(store, rec_off, rec_len, win, size, scale=None):
    """The row rule itself, for a row-level plan: r[clamp(win + t, 0, L - 1)], zeros for L == 0; ``scale``: one factor per row or None."""
    x = widen(store)
    out = torch.zeros((len(rec_off), size), dtype=torch.float32)
    t = torch.arange(size)
    for b, (off, L, w) in enumerate(zip(*(v.tolist() for v in (rec_off, rec_len, win)))):
        if L > 0:
            out[b] = x[off:off + L][(w + t).clamp(0, L - 1)]
            if scale is not None and scale[b] is not None:
                out[b] = out[b] * scale[b]
    return out


@pytest.mark.parametrize("L,S", SHAPES)
def test_the_oracle_follows_the_closed_form(L, S):
    g = torch.Generator().manual_seed(10 * L + S)
    store = torch.cat([torch.full((3,), 9.0), torch.rand(L, generator=g) - 0.25, torch.full((3,), -9.0)])
    got, counts = segments_ref(store, [3], [L], [0], S)
    n = -(-L // S)
    left = (n * S - L) // 2
    r = store[3:3 + L].tolist()
    want = torch.tensor([[r[min(max(k * S - left + t, 0), L - 1)] for t in range(S)] for k in range(n)], dtype=torch.float32)
    assert counts.tolist() == [n] and torch.equal(got, want)
    plan = torch.tensor([[3, L, k * S - left] for k in range(n)])
    assert torch.equal(rows_ref(store, plan[:, 0], plan[:, 1], plan[:, 2], S), want)


def test_the_shapes_cover_odd_paddings():
    pads = [(-(-L // S) * S - L) for L, S in SHAPES]
    assert 0 in pads and any(p % 2 == 1 for p in pads) and any(p % 2 == 0 and p > 0 for p in pads)
    clamped = clamp_segment_plan(10, *(torch.tensor(v) for v in ([-3, 4, 99], [5, 99, 5], [-2 ** 62, 3, 2 ** 62], [-1, 2, 7])), 4, 3)
    assert [c.tolist() for c in clamped] == [[0, 4, 10], [5, 6, 0], [-4, 3, 0], [0, 2, 2]]


# ---- the plan --------------------------------------------------------------------------------------------------------------------

def _clips(dtype=torch.float32, extra=()):
    g = torch.Generator().manual_seed(5)
    recs = [torch.rand(L, generator=g) - 0.5 for L, _ in SHAPES] + [torch.zeros(n) for n in extra]
    return PackedClips([(r * 20000).to(torch.int16) if dtype == torch.int16 else r for r in recs])


@pytest.mark.parametrize("S", [4, 5])
def test_plan_integers(S):
    pc = _clips()
    index = [7, 0, 3, 3, 6, 1, 2, 4, 5]                                     # any order, a repeat
    counts, rec, win, left = pc.segment_plan(index, S)
    Ls = [SHAPES[i][0] for i in index]
    assert counts.dtype == torch.int64 and counts.device.type == "cpu" and counts.tolist() == [-(-L // S) for L in Ls]
    assert left.tolist() == [(n * S - L) // 2 for n, L in zip(counts.tolist(), Ls)]
    assert rec.tolist() == [i for i, n in zip(index, counts.tolist()) for _ in range(n)]
    assert win.tolist() == [k * S - lf for n, lf in zip(counts.tolist(), left.tolist()) for k in range(n)]
    for n, L, lf in zip(counts.tolist(), Ls, left.tolist()):                # pad_input's split: the right pad is left or left + 1
        assert 0 <= n * S - L < S and n * S - L - lf in (lf, lf + 1)
    empty = pc.segment_plan([], S)
    assert [t.numel() for t in empty] == [0, 0, 0, 0]
    assert torch.equal(pc.segment_plan(torch.tensor(index, dtype=torch.int32), S)[2], win)


def test_plan_errors():
    pc = _clips(extra=(0,))
    with pytest.raises(ValueError, match="empty recording"):
        pc.segment_plan([0, len(SHAPES)], 4)
    with pytest.raises(ValueError, match="empty recording"):
        pc.segments([len(SHAPES)], 4)
    for bad in ([-1], [len(SHAPES) + 1], [0, 99]):
        with pytest.raises(ValueError, match="outside"):
            pc.segments(bad, 4)
    with pytest.raises(TypeError):
        pc.segment_plan(torch.tensor([0.5]), 4)
    with pytest.raises(ValueError):
        pc.segment_plan([0], 0)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):      # a valid plan gets as far as the store's device
        pc.segments([0, 1], 4)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        pc.peaks()
    pc.refresh_peaks()
    assert "immutable" in PackedClips.refresh_peaks.__doc__ and pc._peaks is None


def test_the_names_are_exported():
    for name in ("segment_mean", "evaluate_recordings", "PackedClips"):
        assert name in leaf_pytorch_amd.__all__ and getattr(leaf_pytorch_amd, name) is getattr(transforms, name)
    assert callable(PackedClips.segments) and callable(PackedClips.peaks)


# ---- the C entries ---------------------------------------------------------------------------------------------------------------

CTYPE = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}


def declared(name):
    """(restype, argtypes) of ``name`` as include/leaf_hip.h declares it: every pointer a void*, the integers by their C type."""
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    m = re.search(r"(\w[\w ]*?) " + name + r"\(([^)]*)\);", flat)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else CTYPE[a.rsplit(" ", 1)[0].strip()])
    return CTYPE[m.group(1).strip()], args


def test_the_entries_are_declared_as_exported():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6 and _native.ABI_VERSION == 6      # additive
    i, v, ll, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_size_t
    want = {"leaf_clip_peaks_f32": (i, [v, ll, i, i, v, v, v, v, z, v]),
            "leaf_clip_peaks_workspace_bytes": (z, [i]),
            "leaf_assemble_segments_f32": (i, [v, ll, i, i, i, v, v, v, v, v, i, v, v])}
    lib = _native.load()
    assert lib.leaf_abi_version() == 6
    for name, sig in want.items():
        assert name in _native.EXPORTED_SYMBOLS and _native._SIGNATURES[name] == sig == declared(name), name
        fn = getattr(lib, name)
        assert fn.restype == sig[0] and fn.argtypes == sig[1]
    assert declared("leaf_assemble_clips_f32") == _native._SIGNATURES["leaf_assemble_clips_f32"]        # the parser reads a known entry right


def test_peaks_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000                                        # never dereferenced: every call below is refused before the launch
    assert lib.leaf_clip_peaks_workspace_bytes(5) == 48 and lib.leaf_clip_peaks_workspace_bytes(0) == 0 == lib.leaf_clip_peaks_workspace_bytes(-3)

    def call(store=p, store_len=100, flags=0, R=5, rec_off=p, rec_len=p, peaks=p, ws=p, ws_bytes=48):
        return lib.leaf_clip_peaks_f32(store, store_len, flags, R, rec_off, rec_len, peaks, ws, ws_bytes, None)

    for name in ("store", "rec_off", "rec_len", "peaks"):
        assert call(**{name: None}) == NULL_POINTER, name
    assert call(R=0) == BAD_SHAPE and call(R=-1) == BAD_SHAPE and call(store_len=-1) == BAD_SHAPE
    assert call(flags=_native.FLAG_IO_BF16) == UNSUPPORTED and call(flags=_native.FLAG_X_PCM16 | _native.FLAG_PCEN) == UNSUPPORTED
    for name in ("store", "rec_len", "peaks"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(rec_off=p + 4) == ALIGNMENT and call(ws=p + 8) == ALIGNMENT
    assert call(store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT
    assert call(ws=None) == WORKSPACE and call(ws_bytes=47) == WORKSPACE
    # the documented order: flags, pointers, shape, alignment, workspace
    assert call(flags=1, store=None, R=0) == UNSUPPORTED and call(store=None, R=0, peaks=p + 2) == NULL_POINTER
    assert call(R=0, peaks=p + 2, ws=None) == BAD_SHAPE and call(peaks=p + 2, ws=None) == ALIGNMENT
    assert call(store=p + 2, flags=_native.FLAG_X_PCM16, ws_bytes=0) == WORKSPACE   # (2-byte alignment is enough for int16)


def test_segments_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000

    def call(store=p, store_len=100, flags=0, rows=3, size=8, rec_off=p, rec_len=p, win=p, peaks=None, rec=None, R=0, out=p):
        return lib.leaf_assemble_segments_f32(store, store_len, flags, rows, size, rec_off, rec_len, win, peaks, rec, R, out, None)

    for name in ("store", "rec_off", "rec_len", "win", "out"):
        assert call(**{name: None}) == NULL_POINTER, name
    assert call(peaks=p, rec=None, R=2) == NULL_POINTER                     # peaks without the rows' entries
    assert call(rows=0) == BAD_SHAPE and call(rows=-1) == BAD_SHAPE and call(size=0) == BAD_SHAPE and call(store_len=-1) == BAD_SHAPE
    assert call(peaks=p, rec=p, R=0) == BAD_SHAPE
    assert call(rows=2 ** 31 - 1, size=2 ** 31 - 1) == BAD_SHAPE            # rows x tiles beyond a grid
    assert call(flags=_native.FLAG_IO_BF16) == UNSUPPORTED and call(flags=_native.FLAG_X_PCM16 | _native.FLAG_PCEN) == UNSUPPORTED
    for name in ("store", "rec_len", "out"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(rec_off=p + 4) == ALIGNMENT and call(win=p + 4) == ALIGNMENT
    assert call(peaks=p + 2, rec=p, R=2) == ALIGNMENT and call(peaks=p, rec=p + 2, R=2) == ALIGNMENT
    assert call(store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT
    assert call(flags=1, store=None, rows=0) == UNSUPPORTED and call(store=None, rows=0, out=p + 2) == NULL_POINTER
    assert call(rows=0, out=p + 2) == BAD_SHAPE
    assert call(store=p + 2, flags=_native.FLAG_X_PCM16, rows=0) == BAD_SHAPE       # (2-byte alignment is enough for int16: the shape answers)


def test_a_bad_cpu_row_plan_raises_before_the_store_is_looked_at():
    store = torch.zeros(100)
    ok = dict(rec_off=[0, 10], rec_len=[10, 40], win=[-3, 35], size=16)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.assemble_segments(store, **ok)
    for bad in (dict(rec_off=[0, 101]), dict(rec_len=[10, 91]), dict(rec_len=[-1, 40]), dict(win=[0]), dict(size=0), dict(win=[0.5, 1.0])):
        with pytest.raises((ValueError, TypeError)):
            _native.assemble_segments(store, **{**ok, **bad})
    with pytest.raises(ValueError, match="rec"):
        _native.assemble_segments(store, **ok, peaks=torch.ones(2))
    with pytest.raises(ValueError, match="outside"):
        _native.assemble_segments(store, **ok, peaks=torch.ones(2), rec=[0, 2])
    with pytest.raises(RuntimeError, match="1-D float32 or int16"):
        _native.clip_peaks(store.double(), [0], [10])
    with pytest.raises(ValueError):
        _native.clip_peaks(store, [0, 95], [10, 6])


# ---- segment_mean and the packing of evaluate_recordings ---------------------------------------------------------------------------

COUNTS = [1, 3, 1, 7]


def mean_bound(preds, n):
    """Two float32 means of n terms of size <= max|preds|, summed in any order, differ by less than this: each sum carries at most
    (n - 1) roundings of 2^-24 relative to a partial sum <= n max, i.e. (n - 1) 2^-24 max after the division, plus the division's
    own rounding -- n 2^-24 max per side."""
    return n * 2.0 ** -23 * float(preds.abs().max())


def test_segment_mean_is_the_mean_over_each_recordings_rows():
    g = torch.Generator().manual_seed(3)
    preds = (torch.rand(sum(COUNTS), 5, generator=g) - 0.3) * 40
    got = segment_mean(preds, COUNTS)
    assert got.shape == (4, 5) and got.dtype == torch.float32
    a = 0
    for i, n in enumerate(COUNTS):
        want = torch.mean(preds[a:a + n], 0)
        assert float((got[i] - want).abs().max()) <= mean_bound(preds, n), i
        a += n
    assert torch.equal(got[0], preds[0]) and torch.equal(got[2], preds[4])  # a mean over one row is the row
    assert torch.equal(segment_mean(preds, torch.tensor(COUNTS)), got)
    assert segment_mean(preds[:0], []).shape == (0, 5)
    assert segment_mean(preds.reshape(12, 5, 1), COUNTS).shape == (4, 5, 1)
    for bad in ([1, 3, 1, 6], [12, 0], [13]):
        with pytest.raises(ValueError):
            segment_mean(preds, bad)


class HostClips(PackedClips):
    """PackedClips whose rows come from the row rule on the CPU: the packing of ``evaluate_recordings`` without a device."""
    launches = 0

    def _segment_rows(self, rec, win, size, normalize, out=None):
        self.launches += 1
        return rows_ref(self.store, self.offsets_host[rec], self.lengths_host[rec], win, size)[:, None]


@pytest.mark.parametrize("max_rows", [1, 4, 512])
def test_evaluate_recordings_packs_and_carries(max_rows):
    g = torch.Generator().manual_seed(9)
    lengths = [3, 50, 8, 8, 23, 1, 31, 9]                                   # 1 .. 7 rows of 8 samples
    pc = HostClips([torch.rand(n, generator=g) - 0.5 for n in lengths])
    head = torch.nn.Linear(8, 3).double()
    model = lambda x: head(x[:, 0].double()).float()                        # float64 inside: a row's output does not depend on the batch it is in
    index = [7, 1, 0, 1, 2, 3, 4, 5, 6]
    got = evaluate_recordings(model, pc, 8, index, max_rows=max_rows)
    rows = sum(-(-lengths[i] // 8) for i in index)
    assert got.shape == (len(index), 3) and not got.requires_grad and pc.launches == -(-rows // max_rows)
    for place, i in enumerate(index):
        with torch.no_grad():
            preds = model(pad_input(pc.store[pc.offsets_host[i]:pc.offsets_host[i] + lengths[i]], 8)[:, None])
        assert float((got[place] - preds.mean(0)).abs().max()) <= mean_bound(preds, preds.shape[0]), (place, i)
    assert torch.equal(evaluate_recordings(model, pc, 8, max_rows=max_rows), evaluate_recordings(model, pc, 8, list(range(8)), max_rows=max_rows))
    with pytest.raises(ValueError):
        evaluate_recordings(model, pc, 8, index, max_rows=0)
