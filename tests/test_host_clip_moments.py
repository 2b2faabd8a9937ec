"""Waveform standardisation (audio_config.normalize) in the assembly launches, the host side (no GPU): the CPU oracles that
tests/test_gpu_clip_moments.py compares the kernels with, the four C entries as declared and exported with their argument checks,
the validation of the Python layer, the split of leaf_clip_moments_f32's reductions, and ClipSampler's recording index.

The oracles.  ``moments_ref`` is float64 numpy: mean, unbiased std (ddof = 1), min, max of every recording, rounded once to float32.
``standardize_ref`` is the reference's parser on every recording of a store -- the stock torch expression ``(r - mean) / (std + 1e-9)``
on a float32 recording and 0-d float32 ``mean`` / ``std`` tensors that hold given moments -- and the assembly oracles are the existing
ones (tests/test_host_clips.py, test_host_clip_noise.py, test_host_segments.py) on the store that comes back."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import leaf_pytorch_amd
from leaf_pytorch_amd import ClipSampler, PackedClips, _native, evaluate_recordings
from test_host_clip_noise import assemble_noise_ref
from test_host_clips import MIN, REPLICATE, WRAP, ZERO, widen
from test_host_segments import rows_ref, segments_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, WORKSPACE, ALIGNMENT, UNSUPPORTED = -1, -2, -3, -7, -8
TILE, SPANS = 1024, 32                                 # csrc/leaf_segments_view.hpp: kMomentTile, kMomentSpans


# ---- the oracles -------------------------------------------------------------------------------------------------------------------

def moments_ref64(store, off, ln) -> np.ndarray:
    """(R, 5) float64: mean, unbiased std, min, max, mean |r| of every recording, all in float64 numpy (two passes: numpy's std takes the
    deviations from its float64 mean).  L == 1: std NaN; L == 0: (0, NaN, 0, 0, 0)."""
    x = widen(store).numpy().astype(np.float64)
    out = np.zeros((len(off), 5))
    for i, (o, n) in enumerate(zip(off, ln)):
        r = x[int(o):int(o) + int(n)]
        if r.size == 0:
            out[i] = (0.0, np.nan, 0.0, 0.0, 0.0)
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            std = np.sqrt(np.sum((r - r.mean()) ** 2) / (r.size - 1)) if r.size > 1 else np.nan
        out[i] = (r.mean(), std, np.nanmin(r), np.nanmax(r), np.abs(r).mean())
    return out


def moments_ref(store, off, ln) -> torch.Tensor:
    """(R, 4) float32: the float64 moments rounded once."""
    return torch.from_numpy(moments_ref64(store, off, ln)[:, :4].astype(np.float32))


def parser(r: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """utilities/data/raw_waveform_parser.py:16-23 behind its own ``.mean()`` / ``.std()``: the stock expression on 0-d float32 tensors."""
    assert r.dtype == mean.dtype == std.dtype == torch.float32 and mean.dim() == std.dim() == 0
    return (r - mean) / (std + 1e-9)


def standardize_ref(store, off, ln, moments) -> torch.Tensor:
    """The float32 image of ``store`` with every recording put through ``parser`` with its row of ``moments`` ((R, 4) float32);
    samples outside the recordings stay as they are.  The recordings must not overlap."""
    x, moments = widen(store), moments.detach().cpu()
    out = x.clone()
    for i, (o, n) in enumerate(zip(off, ln)):
        o, n = int(o), int(n)
        out[o:o + n] = parser(x[o:o + n], moments[i, 0], moments[i, 1])
    return out


def standardized_peak(moments: torch.Tensor) -> torch.Tensor:
    """max(|y(min)|, |y(max)|) per recording by the stock expression: what leaf_assemble_segments_std_f32 scales by."""
    m = moments.detach().cpu()
    lo, hi = ((m[:, c] - m[:, 0]) / (m[:, 1] + 1e-9) for c in (2, 3))
    return torch.maximum(lo.abs(), hi.abs())


def assemble_std_ref(store, off, ln, moments, rec, start, pad_mode, size, gain=None, masks=None, normalize_fn=None, noise=None, gaussian=None):
    """``assemble_noise_ref`` on the standardised store: clip b is recording ``rec[b]``; the noise store stays as it is."""
    std_store = standardize_ref(store, off, ln, moments)
    rec = [int(i) for i in rec]
    return assemble_noise_ref(std_store, [int(off[i]) for i in rec], [int(ln[i]) for i in rec], start, pad_mode, size, gain, masks, normalize_fn,
                              noise, gaussian)


def segments_std_ref(store, off, ln, moments, index, size, normalize_fn=None):
    """``segments_ref`` (the restated test.py loop) with the parser in front: on the standardised store."""
    return segments_ref(standardize_ref(store, off, ln, moments), off, ln, index, size, normalize_fn)


# ---- the store of the moments tests: the lengths around the tile, a long recording, and the hard cases ----------------------------------

EDGE_LENGTHS = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097, 300001]
DC, CONST, NAN = len(EDGE_LENGTHS), len(EDGE_LENGTHS) + 1, len(EDGE_LENGTHS) + 2


@functools.lru_cache(maxsize=None)
def moment_store(dtype):
    """Recordings back to back, no gaps: EDGE_LENGTHS (each at its own offset and amplitude, so a read across an edge moves a
    moment), one with a DC offset of 0.5 and a deviation of 1e-3 (a one-pass sum-of-squares formula loses it in float32 and most of
    it in float64), a constant one, and -- float32 only -- one with a NaN sample.  Returns (store, offsets, lengths)."""
    g = torch.Generator().manual_seed(7)
    recs = []
    for i, n in enumerate(EDGE_LENGTHS):
        recs.append((torch.rand(n, generator=g) * 2 - 1) * (0.1 + 0.05 * i) + 0.02 * (i - 5))
    recs.append(0.5 + 1e-3 * (torch.rand(5000, generator=g) * 2 - 1))
    recs.append(torch.full((2000,), 0.25))
    if dtype == torch.int16:
        recs = [(r * 32768).round().clamp(-32768, 32767).to(torch.int16) for r in recs]
    else:
        nan = torch.rand(100, generator=g) - 0.5
        nan[37] = float("nan")
        recs.append(nan)
    ln = torch.tensor([r.numel() for r in recs])
    return torch.cat(recs), torch.cumsum(ln, 0) - ln, ln


def mean_bound(m64):
    """|mean - mean64| <= 2^-24 |mean64| + 2^-40 mean|r|: one float32 rounding, and float64 accumulation slack."""
    return 2.0 ** -24 * np.abs(m64[:, 0]) + 2.0 ** -40 * m64[:, 4]


def std_bound(m64):
    """|std - std64| <= 2^-23 std64."""
    return 2.0 ** -23 * m64[:, 1]


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
def test_the_oracle_moments_are_the_references_and_the_hard_cases_are_hard(dtype):
    store, off, ln = moment_store(dtype)
    m64, m = moments_ref64(store, off, ln), moments_ref(store, off, ln)
    x = widen(store).double()
    for i in range(len(ln)):
        r = x[int(off[i]):int(off[i]) + int(ln[i])]
        if i == 0:
            assert np.isnan(m64[i, 1]) and bool(torch.isnan(r.std()))       # L == 1: torch's unbiased std is NaN too
        elif dtype == torch.float32 and i == NAN:
            assert np.isnan(m64[i, 0]) and np.isnan(m64[i, 1]) and bool(torch.isnan(r.mean()))
        else:
            assert abs(float(r.mean()) - m64[i, 0]) <= 2.0 ** -45 * m64[i, 4] and abs(float(r.std()) - m64[i, 1]) <= 2.0 ** -45 * m64[i, 1]
            assert m64[i, 2] == float(r.min()) and m64[i, 3] == float(r.max())
    assert m64[CONST, 1] == 0.0 and float(m[CONST, 1]) == 0.0 and float(m[CONST, 0]) == 0.25
    assert abs(m64[DC, 0] - 0.5) < 1e-4 and 4e-4 < m64[DC, 1] < 7e-4
    # the one-pass formula sqrt((sum x^2 - (sum x)^2 / L) / (L - 1)) in float32 misses the DC recording's std by far more than the bound
    r32 = widen(store)[int(off[DC]):int(off[DC]) + int(ln[DC])]
    one_pass = torch.sqrt(((r32 * r32).sum() - r32.sum() ** 2 / r32.numel()).clamp(min=0) / (r32.numel() - 1))
    assert abs(float(one_pass) - m64[DC, 1]) > 100 * std_bound(m64)[DC]
    assert moments_ref(store[:0], [0], [0]).tolist()[0][0::2] == [0.0, 0.0] and bool(torch.isnan(moments_ref(store[:0], [0], [0])[0, 1]))


# torch's own float32 .mean() / .std() against the bounds the library is held to, on the same recordings (the CPU kernels, torch 2.10).
# Its std (a Welford pass accumulated in double) stays inside the bound on every input: at most 0.39 of it.  Its mean (a float32
# cascade sum) leaves the bound on seven inputs, whose bounds are widened to torch's measured distance -- in units of the library's
# bound: float32 store, L = 63: 1.45, 64: 1.56, 65: 2.67, 1023: 1.27, 1025: 1.19; int16 store, L = 300001: 2.18 with 8 threads (0.94
# with one: the split of a long sum follows the thread count, so the float32 store's long recording, 0.38 here, is widened alike),
# DC recording: 1.05 -- each rounded up to 4 bounds.  Every other input keeps the bound itself.
WIDENED = 4
TORCH_MEAN = {torch.float32: [1, 1, 1, WIDENED, WIDENED, WIDENED, WIDENED, 1, WIDENED, 1, WIDENED, 1, 1],
              torch.int16: [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, WIDENED, WIDENED, 1]}
TORCH_STD = {torch.float32: [0] + [1] * 12, torch.int16: [0] + [1] * 12}


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
def test_torchs_own_float32_moments_against_the_same_bounds(dtype):
    store, off, ln = moment_store(dtype)
    m64 = moments_ref64(store, off, ln)
    x = widen(store)
    mb, sb = mean_bound(m64), std_bound(m64)
    for i in range(CONST + 1):
        r = x[int(off[i]):int(off[i]) + int(ln[i])]
        dm = abs(float(r.mean().double()) - m64[i, 0])
        print(f"{dtype} recording {i} (L={int(ln[i])}): torch mean off by {dm / mb[i] if mb[i] else 0:.2f} bounds", end="")
        assert dm <= TORCH_MEAN[dtype][i] * mb[i], (i, dm, mb[i])
        if i == 0:
            assert bool(torch.isnan(r.std()))
            print()
            continue
        ds = abs(float(r.std().double()) - m64[i, 1])
        print(f", std by {ds / sb[i] if sb[i] else ds:.2f} bounds")
        assert ds <= TORCH_STD[dtype][i] * sb[i], (i, ds, sb[i])


def test_the_parser_is_a_true_float32_division():
    g = torch.Generator().manual_seed(3)
    r = torch.rand(4099, generator=g) * 2 - 0.7
    mean, std = r.mean(), r.std()
    y = parser(r, mean, std)
    m, s = np.float32(float(mean)), np.float32(float(std))
    d = np.float32(s + np.float32(1e-9))                                    # one float32 add
    want = (r.numpy() - m) / d                                              # one float32 subtraction, one correctly rounded division
    assert y.dtype == torch.float32 and np.array_equal(y.numpy().view(np.int32), want.view(np.int32))
    assert not np.array_equal(((r.numpy() - m) * (np.float32(1) / d)).view(np.int32), want.view(np.int32))    # a reciprocal multiply is told apart
    const = parser(torch.full((9,), 0.25), torch.tensor(0.25), torch.tensor(0.0))
    assert const.tolist() == [0.0] * 9
    assert bool(torch.isnan(parser(torch.tensor([0.5]), torch.tensor(0.5), torch.tensor(float("nan")))).all())
    # monotone: the standardised extremes are the extremes of the standardised recording
    assert float(y.min()) == float(parser(r.min(), mean, std)) and float(y.max()) == float(parser(r.max(), mean, std))
    mo = torch.stack((mean, std, r.min(), r.max()))[None]
    assert float(standardized_peak(mo)[0]) == float(y.abs().max())


def test_the_assembly_oracle_standardises_the_whole_recording_first():
    store = torch.tensor([9.0, 1.0, 2.0, 3.0, 6.0, -9.0, 5.0])
    off, ln = [1, 6], [4, 1]
    mo = moments_ref(store, off, ln)
    assert mo[0].tolist() == [3.0, float(np.float32(np.sqrt(14 / 3))), 1.0, 6.0] and bool(torch.isnan(mo[1, 1]))
    y = standardize_ref(store, off, ln, mo)
    assert y[0] == 9.0 and y[5] == -9.0 and bool(torch.isnan(y[6])) and float(y[3]) == 0.0
    got = assemble_std_ref(store, off, ln, mo, [0, 0], [1, 0], [ZERO, MIN], 3)
    assert torch.equal(got[0], y[2:5])                                     # a crop: the moments are the recording's, not the window's
    wide = assemble_std_ref(store, off, ln, mo, [0], [0], [MIN], 8)[0]
    assert torch.equal(wide[2:6], y[1:5]) and wide[0] == wide[7] == y[1] and float(y[1]) == float(parser(torch.tensor(1.0), mo[0, 0], mo[0, 1]))
    rows, counts = segments_std_ref(store, off, ln, mo, [0], 3)
    assert counts.tolist() == [2] and torch.equal(rows.reshape(-1), y[[1, 1, 2, 3, 4, 4]])


# ---- the split of the reductions (csrc/leaf_segments_view.hpp: moment_span) ---------------------------------------------------------------

def moment_span(L, k):
    tiles = -(-L // TILE)
    per = -(-tiles // SPANS)
    return min(k * per * TILE, L), min((k + 1) * per * TILE, L)


@pytest.mark.parametrize("L", [0, 1, 1023, 1024, 1025, 32 * 1024, 32 * 1024 + 1, 300001, 2 ** 31 - 1])
def test_the_spans_tile_the_recording(L):
    spans = [moment_span(L, k) for k in range(SPANS)]
    assert spans[0][0] == 0 and spans[-1][1] == L and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert all(b % TILE == 0 for b, e in spans if b < e) and all(0 <= e - b for b, e in spans)
    header = open(os.path.join(REPO, "leaf_pytorch_amd", "csrc", "leaf_segments_view.hpp")).read()
    assert "kMomentTile = 1024" in header and "kMomentSpans = 32" in header


def test_the_view_functions_run_clean_under_ubsan():
    """tools/segment_view_check.cpp, a program of its own: the clamps of the plans (the moments index among them) and the span
    arithmetic over hostile values, under -fsanitize=undefined on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "segment_view_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(REPO, "leaf_pytorch_amd", "csrc"), os.path.join(REPO, "tools", "segment_view_check.cpp"), "-o", exe], check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout and "runtime error" not in run.stderr, (run.stdout, run.stderr)
    assert "moment_span" in open(os.path.join(REPO, "tools", "segment_view_check.cpp")).read()


# ---- the C entries -----------------------------------------------------------------------------------------------------------------

CTYPE = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "unsigned long long": ctypes.c_ulonglong}
NEW_ENTRIES = ("leaf_clip_moments_workspace_bytes", "leaf_clip_moments_f32", "leaf_assemble_clips_std_f32", "leaf_assemble_segments_std_f32")


def declared(name):
    """(restype, argtypes) of ``name`` as include/leaf_hip.h declares it: every pointer a void*, the integers by their C type."""
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    m = re.search(r"(\w[\w ]*?) " + name + r"\(([^)]*)\);", flat)
    assert m, name
    args = [ctypes.c_void_p if "*" in a else CTYPE[a.strip().rsplit(" ", 1)[0].strip()] for a in m.group(2).split(",")]
    return CTYPE[m.group(1).strip()], args


def test_the_entries_are_declared_as_exported_and_the_old_ones_are_untouched():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6 and _native.ABI_VERSION == 6      # additive
    i, v, ll, ull, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_size_t
    noise = _native._SIGNATURES["leaf_assemble_clips_noise_f32"]
    rows = _native._SIGNATURES["leaf_assemble_segments_f32"]
    want = {"leaf_clip_moments_workspace_bytes": (z, [i]),
            "leaf_clip_moments_f32": _native._SIGNATURES["leaf_clip_peaks_f32"],
            "leaf_assemble_clips_std_f32": (i, noise[1][:-1] + [v, v, i, v]),            # the group between gauss_stream and stream
            "leaf_assemble_segments_std_f32": (i, rows[1][:-1] + [v, i, v])}             # moments, normalize between out and stream
    lib = _native.load()
    assert lib.leaf_abi_version() == 6
    docs = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW_ENTRIES:
        assert name in _native.EXPORTED_SYMBOLS and _native._SIGNATURES[name] == want[name] == declared(name), name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1] and name in docs
    assert declared("leaf_assemble_clips_noise_f32") == noise and declared("leaf_assemble_segments_f32") == rows
    assert noise == (i, [v, ll, i, i, i, v, v, v, v, v, i, v, i, v, v, ll, v, v, v, v, v, v, ull, v, v])
    for name in ("clip_moments", "assemble_clips", "assemble_segments"):
        assert callable(getattr(_native, name))
    assert callable(PackedClips.moments) and callable(PackedClips.refresh_moments) and leaf_pytorch_amd.PackedClips is PackedClips


def test_moments_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000                                        # never dereferenced: every call below is refused before the launch
    size = lib.leaf_clip_moments_workspace_bytes
    assert size(5) == 5 * (SPANS * 16 + 8) == 2600 and size(1) == 520 and size(0) == 0 == size(-3)

    def call(store=p, store_len=100, flags=0, R=5, rec_off=p, rec_len=p, moments=p, ws=p, ws_bytes=2600):
        return lib.leaf_clip_moments_f32(store, store_len, flags, R, rec_off, rec_len, moments, ws, ws_bytes, None)

    for name in ("store", "rec_off", "rec_len", "moments"):
        assert call(**{name: None}) == NULL_POINTER, name
    assert call(R=0) == BAD_SHAPE and call(R=-1) == BAD_SHAPE and call(store_len=-1) == BAD_SHAPE
    assert call(flags=_native.FLAG_IO_BF16) == UNSUPPORTED and call(flags=_native.FLAG_X_PCM16 | _native.FLAG_PCEN) == UNSUPPORTED
    for name in ("store", "rec_len", "moments"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(rec_off=p + 4) == ALIGNMENT and call(ws=p + 8) == ALIGNMENT
    assert call(store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT
    assert call(ws=None) == WORKSPACE and call(ws_bytes=2599) == WORKSPACE
    # the documented order: flags, pointers, shape, alignment, workspace
    assert call(flags=1, store=None, R=0) == UNSUPPORTED and call(store=None, R=0, moments=p + 2) == NULL_POINTER
    assert call(R=0, moments=p + 2, ws=None) == BAD_SHAPE and call(moments=p + 2, ws=None) == ALIGNMENT
    assert call(store=p + 2, flags=_native.FLAG_X_PCM16, ws_bytes=0) == WORKSPACE   # (2-byte alignment is enough for int16)


def test_assemble_std_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000

    def call(store=p, store_len=100, flags=0, B=2, size=8, rec_off=p, rec_len=p, start=p, pad_mode=p, gain=None, normalize=1, masks=None,
             M=0, out=p, noise=(None, 0, None, None, None, None, None), gauss=(None, 0, None), moments=p, rec=p, R=3):
        return lib.leaf_assemble_clips_std_f32(store, store_len, flags, B, size, rec_off, rec_len, start, pad_mode, gain, normalize, masks, M, out,
                                               *noise, *gauss, moments, rec, R, None)

    for name in ("store", "rec_off", "rec_len", "start", "pad_mode", "out", "moments", "rec"):
        assert call(**{name: None}) == NULL_POINTER, name                   # (the group in part, too)
    assert call(noise=(p, 10, p, p, None, p, p)) == NULL_POINTER and call(gauss=(p, 1, None)) == NULL_POINTER
    assert call(B=0) == BAD_SHAPE and call(size=0) == BAD_SHAPE and call(store_len=-1) == BAD_SHAPE and call(M=2) == BAD_SHAPE
    assert call(R=0) == BAD_SHAPE and call(R=-4) == BAD_SHAPE and call(noise=(p, -1, p, p, p, p, p)) == BAD_SHAPE
    assert call(flags=_native.FLAG_IO_BF16) == UNSUPPORTED
    for name in ("store", "rec_len", "start", "pad_mode", "out", "gain", "moments", "rec"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(rec_off=p + 4) == ALIGNMENT and call(store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT
    assert call(gauss=(p, 1, p + 4)) == ALIGNMENT and call(noise=(p, 10, p + 4, p, p, p, p)) == ALIGNMENT
    # the order: flags, pointers, shape, alignment
    assert call(flags=1, store=None, B=0) == UNSUPPORTED and call(moments=None, R=0, out=p + 2) == NULL_POINTER and call(R=0, out=p + 2) == BAD_SHAPE
    # without the group the call IS the noise entry (and, without its groups, the plain one): their answers, R unread
    assert call(moments=None, rec=None, R=0, B=0) == BAD_SHAPE and call(moments=None, rec=None, R=0, out=None) == NULL_POINTER
    assert call(moments=None, rec=None, R=0, out=p + 2) == ALIGNMENT and call(moments=None, rec=None, gauss=(p, 1, None)) == NULL_POINTER


def test_segments_std_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000

    def call(store=p, store_len=100, flags=0, rows=3, size=8, rec_off=p, rec_len=p, win=p, peaks=None, rec=p, R=2, out=p, moments=p, normalize=1):
        return lib.leaf_assemble_segments_std_f32(store, store_len, flags, rows, size, rec_off, rec_len, win, peaks, rec, R, out, moments, normalize, None)

    for name in ("store", "rec_off", "rec_len", "win", "out", "rec"):
        assert call(**{name: None}) == NULL_POINTER, name
    assert call(peaks=p) == UNSUPPORTED and call(flags=_native.FLAG_IO_BF16) == UNSUPPORTED
    assert call(rows=0) == BAD_SHAPE and call(size=0) == BAD_SHAPE and call(store_len=-1) == BAD_SHAPE and call(R=0) == BAD_SHAPE
    assert call(rows=2 ** 31 - 1, size=2 ** 31 - 1) == BAD_SHAPE
    for name in ("store", "rec_len", "out", "rec", "moments"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(rec_off=p + 4) == ALIGNMENT and call(win=p + 4) == ALIGNMENT and call(store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT
    assert call(flags=1, peaks=p, store=None) == UNSUPPORTED and call(store=None, rows=0) == NULL_POINTER and call(rows=0, out=p + 2) == BAD_SHAPE
    # moments == NULL: the call IS leaf_assemble_segments_f32 -- rec and R are the peaks', and optional without them
    assert call(moments=None, rec=None, R=0, rows=0) == BAD_SHAPE and call(moments=None, peaks=p, rec=None) == NULL_POINTER
    assert call(moments=None, rec=None, R=0, out=p + 2) == ALIGNMENT


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------

STORE = torch.zeros(100, dtype=torch.int16)            # a CPU store: a valid call gets as far as require_hip and no further
MOMENTS = torch.zeros((2, 4))


def test_a_bad_cpu_plan_raises_before_anything_is_launched():
    ok = dict(rec_off=[0, 10], rec_len=[10, 40], start=[0, 5], pad_mode=[1, 2], size=16)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.assemble_clips(STORE, **ok, standardize=(MOMENTS, [0, 1]))
    for bad in ((MOMENTS, [0, 2]), (MOMENTS, [-1, 0]), (MOMENTS, [0]), (MOMENTS[:, :3], [0, 1]), (MOMENTS[:0], [0, 0]), (MOMENTS,), (MOMENTS.reshape(-1), [0, 1])):
        with pytest.raises(ValueError):
            _native.assemble_clips(STORE, **ok, standardize=bad)
    with pytest.raises(TypeError):
        _native.assemble_clips(STORE, **ok, standardize=(MOMENTS.double(), [0, 1]))
    with pytest.raises(TypeError):
        _native.assemble_clips(STORE, **ok, standardize=(MOMENTS, [0.0, 1.0]))
    rows = dict(rec_off=[0, 10], rec_len=[10, 40], win=[-3, 35], size=16)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.assemble_segments(STORE, **rows, rec=[1, 0], moments=MOMENTS)
    with pytest.raises(ValueError, match="rec"):
        _native.assemble_segments(STORE, **rows, moments=MOMENTS)
    with pytest.raises(ValueError, match="exclude"):
        _native.assemble_segments(STORE, **rows, rec=[0, 1], moments=MOMENTS, peaks=torch.ones(2))
    with pytest.raises(ValueError, match="outside"):
        _native.assemble_segments(STORE, **rows, rec=[0, 2], moments=MOMENTS)
    with pytest.raises(RuntimeError, match="1-D float32 or int16"):
        _native.clip_moments(STORE.double(), [0], [10])
    with pytest.raises(ValueError):
        _native.clip_moments(STORE, [0, 95], [10, 6])
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.clip_moments(STORE, [0, 10], [10, 40])


def test_packed_clips_keeps_and_refreshes_its_moments():
    pc = PackedClips([STORE[:30], STORE[30:]])
    for call in (pc.moments, lambda: pc.assemble([0, 1], 0, 16, standardize=True), lambda: pc.segments([0, 1], 16, standardize=True)):
        with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
            call()
    with pytest.raises(ValueError, match="outside"):
        pc.assemble([0, 2], 0, 16, standardize=True)
    pc._moments = MOMENTS
    assert pc.moments() is MOMENTS
    pc.refresh_moments()
    assert pc._moments is None and "immutable" in PackedClips.refresh_moments.__doc__
    for fn in (PackedClips.assemble, PackedClips.segments, evaluate_recordings):
        assert "standardize" in fn.__doc__
    assert "cropped_read" in PackedClips.__doc__ and "noise store" in PackedClips.__doc__


class HostClips(PackedClips):
    """PackedClips whose rows come from the oracle on the CPU: what ``evaluate_recordings`` passes down, without a device."""

    def _segment_rows(self, rec, win, size, normalize, out=None, standardize=False):
        self.seen = getattr(self, "seen", []) + [standardize]
        store = standardize_ref(self.store, self.offsets_host, self.lengths_host, moments_ref(self.store, self.offsets_host, self.lengths_host)) \
            if standardize else self.store
        return rows_ref(store, self.offsets_host[rec], self.lengths_host[rec], win, size)[:, None]


def test_evaluate_recordings_passes_the_keyword_down():
    g = torch.Generator().manual_seed(9)
    pc = HostClips([torch.rand(n, generator=g) + 3.0 for n in (3, 50, 8, 23)])
    head = torch.nn.Linear(8, 3).double()
    model = lambda x: head(x[:, 0].double()).float()
    plain = evaluate_recordings(model, pc, 8, max_rows=4)
    assert pc.seen == [False] * len(pc.seen)
    std = evaluate_recordings(model, pc, 8, max_rows=4, standardize=True)
    assert pc.seen[len(pc.seen) // 2:] == [True] * (len(pc.seen) // 2) and not torch.equal(plain, std)


LENGTHS = (5, 16, 16, 40, 100, 1, 17)
INDEX = torch.arange(len(LENGTHS)).repeat(10)


def test_a_standardising_sampler_draws_what_it_drew_and_carries_the_recordings():
    g = torch.Generator().manual_seed(3)
    pc = PackedClips([torch.randint(-20000, 20000, (n,), dtype=torch.int16, generator=g) for n in LENGTHS])
    kw = dict(num_masks=2, time_perc=0.5, gain_prob=0.5)
    plain = ClipSampler(pc, 16, generator=torch.Generator().manual_seed(11), **kw).plan(INDEX)
    std = ClipSampler(pc, 16, generator=torch.Generator().manual_seed(11), standardize=True, **kw).plan(INDEX)
    assert type(plain) is leaf_pytorch_amd.transforms.ClipPlan and not hasattr(plain, "rec")
    assert len(std) == 6 and all(torch.equal(a, b) for a, b in zip(plain, std))
    assert std.rec.dtype == torch.int32 and std.rec.tolist() == INDEX.tolist() and std.noise is None and std.gaussian is None
    both = ClipSampler(pc, 16, generator=torch.Generator().manual_seed(11), standardize=True, gaussian_prob=0.5, **kw).plan(INDEX)
    assert both.rec.tolist() == INDEX.tolist() and both.gaussian is not None
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        ClipSampler(pc, 16, standardize=True)(INDEX)
    assert "standardize" in ClipSampler.__doc__


def test_the_documents_state_what_is_and_is_not_built():
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "audio_config.normalize" in readme and "leaf_clip_moments_f32" in readme and "cropped_read" in readme
    assert "Not built: the mean / std waveform normalisation" not in readme
