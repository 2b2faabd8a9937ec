"""Resampling, the host side (no GPU): the oracle of leaf_resample_f32 -- NumPy float64, written from the definition in
include/leaf_hip.h -- cross-checked once against scipy's polyphase filter, then compared with the library's table
(leaf_resample_table_f32), its length rule, and the per-output function itself (csrc/leaf_resample.hpp, through
tools/resample_check.cpp compiled with plain g++); the C entries as declared and exported, their refusals in the stated order, and
the Python argument errors.  tests/test_gpu_resample.py compares the kernel with the oracle defined here."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import leaf_pytorch_amd
from leaf_pytorch_amd import PackedClips, _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, WORKSPACE, ALIGNMENT, UNSUPPORTED = -1, -2, -3, -7, -8
RATIOS = [(3, 2), (2, 3), (3, 1), (1, 2), (2, 1), (5, 5), (44100, 16000), (44100, 48000), (48000, 16000)]
WIDE = [(16, 1), (44100, 2000)]                 # a tile's window is beyond the LDS budget: the kernel reads samples and taps from global memory


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

class PlanRef:
    """The definition for (orig_freq, new_freq, W, rho): o, n, width, K = 2 width + o, the spans k0 / cnt, and per phase the span's
    taps in float64 BEFORE their one rounding (``h[p]``, cnt[p] of them).  Every tap of every phase is evaluated densely and the span
    is read off the predicate |t| < W; it must be one run."""

    def __init__(self, orig_freq: int, new_freq: int, W: int = 6, rho: float = 0.99):
        g = math.gcd(orig_freq, new_freq)
        self.o, self.n, self.W = orig_freq // g, new_freq // g, W
        o, n = self.o, self.n
        if o == n:
            self.width, self.K, self.k0, self.cnt, self.h = 0, 1, np.zeros(1, np.int64), np.ones(1, np.int64), [np.ones(1)]
            return
        base = float(min(o, n)) * rho
        self.width = width = math.ceil(W * o / base)
        self.K = K = 2 * width + o
        k = np.arange(K, dtype=np.int64)
        self.k0, self.cnt, self.h = np.zeros(n, np.int64), np.zeros(n, np.int64), []
        for p0 in range(0, n, 256):                                             # (in slabs of phases: 4096 -> 4099 has 16.8 M taps)
            p = np.arange(p0, min(n, p0 + 256), dtype=np.int64)[:, None]
            num = (k[None, :] - width) * n - p * o
            t = num.astype(np.float64) * base / float(o * n)
            inside = np.abs(t) < W
            with np.errstate(invalid="ignore", divide="ignore"):
                sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
            dense = sinc * np.cos(np.pi * t / (2 * W)) ** 2 * base / o
            for r in range(p.shape[0]):
                idx = np.flatnonzero(inside[r])
                assert idx.size >= 1 and idx[-1] - idx[0] + 1 == idx.size, "the span is one run"
                self.k0[p0 + r], self.cnt[p0 + r] = idx[0], idx.size
                self.h.append(dense[r, idx[0]: idx[-1] + 1].copy())

    def length(self, L: int) -> int:
        return -((-self.n * L) // self.o) if L > 0 else 0

    def resample(self, x) -> tuple:
        """(y, bound): the outputs of the recording ``x`` (float64 values of the samples) as dense dot products over the zero-padded
        recording, float64, from the taps ROUNDED to float32 (the table's one rounding is part of the definition), and per output the
        bound (cnt + 2) 2^-24 sum |h| |x| + 2^-149 of a float32 fma chain of cnt terms against it."""
        x = np.asarray(x, dtype=np.float64)
        L, o, n = x.size, self.o, self.n
        out_len = self.length(L)
        y, bound = np.zeros(out_len), np.zeros(out_len)
        reach = (out_len // n + 1) * o + self.K
        xpad = np.concatenate((np.zeros(self.width), x, np.zeros(max(reach - L, 0) + 1)))   # element s + width is x[s]
        for p in range(min(n, out_len)):
            i = np.arange(p, out_len, n) // n
            h = self.h[p].astype(np.float32).astype(np.float64)
            win = xpad[(i * o + self.k0[p])[:, None] + np.arange(self.cnt[p])[None, :]]
            y[p::n] = win @ h
            bound[p::n] = (self.cnt[p] + 2) * 2.0 ** -24 * (np.abs(win) @ np.abs(h)) + 2.0 ** -149
        return y, bound


_plans = {}


def plan_ref(orig_freq, new_freq, W=6, rho=0.99) -> PlanRef:
    key = (orig_freq, new_freq, W, rho)
    if key not in _plans:
        _plans[key] = PlanRef(*key)
    return _plans[key]


def quantize_ref(y32: np.ndarray) -> np.ndarray:
    """The int16 output of a float32 output: rint(y 32768) to nearest even, saturated; NaN gives 0."""
    s = y32.astype(np.float32) * np.float32(32768.0)
    return np.clip(np.rint(np.nan_to_num(s, nan=0.0)), -32768, 32767).astype(np.int16)


def test_oracle_against_scipy_upfirdn():
    """The oracle is band-limited interpolation by ONE prototype filter: F(c) = g(c base / (o n)) sampled at the n-fold rate, applied
    by scipy's polyphase upfirdn with up = n, and read at every o-th output from index N (the filter's half length)."""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    for o, n in ((3, 2), (2, 3), (441, 160), (147, 160)):
        ref = plan_ref(o, n)
        base, W = min(o, n) * 0.99, 6
        N = math.ceil(W * o * n / base)
        t = np.arange(-N, N + 1, dtype=np.float64) * base / float(o * n)
        with np.errstate(invalid="ignore", divide="ignore"):
            proto = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t)) * np.cos(np.pi * t / (2 * W)) ** 2 * base / o
        proto[np.abs(t) >= W] = 0.0
        x = rng.uniform(-1, 1, 2 * o + 77)
        z = signal.upfirdn(proto, x, up=n)
        out_len = ref.length(x.size)
        want = np.array([z[N + j * o] if N + j * o < z.size else 0.0 for j in range(out_len)])
        xpad = np.concatenate((np.zeros(ref.width), x, np.zeros(ref.K + o + 1)))
        got = np.array([xpad[(j // n) * o + ref.k0[j % n] + np.arange(ref.cnt[j % n])] @ ref.h[j % n] for j in range(out_len)])   # unrounded taps
        assert np.abs(got - want).max() <= 3e-14, (o, n, np.abs(got - want).max())


# ---- the table, the plan, the length ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig,new", RATIOS + WIDE + [(4096, 4099)])
def test_table_against_the_oracle(orig, new):
    ref = plan_ref(orig, new)
    tab = _native.resample_table(orig, new)
    assert (tab.o, tab.n, tab.width) == (ref.o, ref.n, ref.width)
    assert np.array_equal(tab.k0.numpy(), ref.k0) and np.array_equal(tab.cnt.numpy(), ref.cnt)
    assert tab.stride == int(ref.cnt.max()) | 1 and tab.taps.shape == (ref.n, tab.stride)
    taps = tab.taps.numpy().astype(np.float64)
    for p in range(ref.n):
        h, c = ref.h[p], int(ref.cnt[p])
        assert np.all(np.abs(taps[p, :c] - h) <= 2.0 ** -23 * np.abs(h) + 1e-20), p
        assert np.all(tab.taps.numpy()[p, c:] == 0.0)                           # outside the span: exactly 0
    assert _native.resample_table(orig, new) is tab                            # kept per key
    assert tab.words.numel() * 4 == _native.load().leaf_resample_table_bytes(orig, new, 6, 0.99)


def test_span_sizes_and_paths():
    sizes = {(44100, 48000): {12, 13}, (44100, 16000): {33, 34}, (48000, 16000): {37}}
    for (orig, new), want in sizes.items():
        tab = _native.resample_table(orig, new)
        assert set(tab.cnt.tolist()) == want and tab.taps_in_lds and tab.window_in_lds
    big = _native.resample_table(4096, 4099)
    assert (big.o, big.n, big.width, big.stride) == (4096, 4099, 7, 13) and 4 * big.taps.numel() == 213148
    assert not big.taps_in_lds and big.window_in_lds                            # a 213 KB table: the taps stay in global memory
    for orig, new in WIDE:
        wide = _native.resample_table(orig, new)
        assert not wide.window_in_lds and not wide.taps_in_lds
    forced = _native.resample_table(3, 2).with_global_taps()
    assert not forced.taps_in_lds and torch.equal(forced.taps, _native.resample_table(3, 2).taps)
    assert _native.resample_table(3, 2).taps_in_lds and _native.resample_table(3, 2) is not forced     # the kept table is untouched
    _native.drop_resample_tables()
    assert _native.resample_table(3, 2).taps_in_lds and not _native._resample_tables.keys() - {(3, 2, 6, 0.99)}
    assert _native.resample_table(5, 5).taps.tolist() == [[1.0]] and _native.resample_table(16000, 16000).width == 0
    other = _native.resample_table(3, 2, lowpass_filter_width=2, rolloff=0.5)
    ref = plan_ref(3, 2, 2, 0.5)
    assert other.width == ref.width and np.array_equal(other.cnt.numpy(), ref.cnt)
    src = open(os.path.join(REPO, "leaf_pytorch_amd", "csrc", "leaf_resample.hpp")).read()
    assert f"kResampleTile = {_native.RESAMPLE_TILE};" in src and "kResampleLdsBudget = 64 * 1024;" in src
    assert f"kResampleHeaderInts = {_native.RESAMPLE_HEADER_INTS};" in src and _native.RESAMPLE_LDS_BUDGET == 64 * 1024


def test_resample_length():
    for L in (0, 1, 2, 3, 159, 160, 161, 441, 44100, 2 ** 31 - 1):
        for orig, new in RATIOS + [(4096, 4099), (1, 65535), (65535, 1), (7, 2 ** 31 - 1)]:
            g = math.gcd(orig, new)
            assert _native.resample_length(L, orig, new) == -((-L * (new // g)) // (orig // g)), (L, orig, new)
    assert _native.resample_length(-5, 3, 2) == 0
    lib = _native.load()
    assert lib.leaf_resample_length(10, 0, 2) == 0 and lib.leaf_resample_length(10, 3, -2) == 0
    assert lib.leaf_resample_length(2 ** 63 - 1, 1, 2) == 2 ** 63 - 1          # saturates, never wraps
    assert lib.leaf_resample_workspace_bytes(0) == 0 and lib.leaf_resample_workspace_bytes(5) == 48


# ---- the per-output function, through tools/resample_check.cpp ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path_factory.mktemp("resample") / "resample_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(REPO, "leaf_pytorch_amd", "csrc"),
                    os.path.join(REPO, "tools", "resample_check.cpp"), "-o", exe], check=True)
    return exe


def run_tool(exe, orig, new, x, pcm=False, W=6, rho=0.99, table=False):
    """The tool on the samples ``x`` (int16 values with ``pcm``, float32 otherwise): (plan line as ints, y as float32 array, q as
    int16 array[, the phases' (k0, cnt, taps)])."""
    xs = ",".join(str(int(v)) for v in x) if pcm else ",".join(float(v).hex() for v in np.asarray(x, dtype=np.float32))
    run = subprocess.run([exe, f"orig={orig}", f"new={new}", f"W={W}", f"rolloff={rho!r}", f"pcm={int(pcm)}", f"table={int(table)}", f"x={xs}"],
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    lines = run.stdout.splitlines()
    plan = [int(v) for v in lines[0].split()[1:]]
    ys = [ln.split() for ln in lines if ln.startswith("y ")]
    y = np.array([int(f[2], 16) for f in ys], dtype=np.uint32).view(np.float32)
    q = np.array([int(f[3]) for f in ys], dtype=np.int64).astype(np.int16)
    assert [int(f[1]) for f in ys] == list(range(plan[-1]))
    if not table:
        return plan, y, q
    phases = [(int(f[2]), int(f[3]), np.array([int(v, 16) for v in f[4:]], dtype=np.uint32).view(np.float32))
              for f in (ln.split() for ln in lines if ln.startswith("phase "))]
    return plan, y, q, phases


def samples(dtype, L: int, seed: int) -> np.ndarray:
    """Seeded samples: int16 over the full range, or float32 uniform in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        return torch.randint(-32768, 32768, (L,), generator=g, dtype=torch.int32).to(torch.int16).numpy()
    return (torch.rand(L, generator=g, dtype=torch.float32) * 2 - 1).numpy()


def as_float64(x: np.ndarray) -> np.ndarray:
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


@pytest.mark.parametrize("orig,new", RATIOS + WIDE)
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
def test_tool_outputs_lie_inside_the_bound(tool, orig, new, dtype):
    ref = plan_ref(orig, new)
    for L in (0, 1, 2, ref.width + 1, ref.o + 1, 2 * ref.o + ref.width + 3, 3 * ref.o + 211):
        x = samples(dtype, L, 100 + L)
        plan, y, q = run_tool(tool, orig, new, x, pcm=dtype == torch.int16)
        want, bound = ref.resample(as_float64(x))
        assert plan[:4] == [ref.o, ref.n, ref.width, ref.K] and y.size == want.size == ref.length(L)
        err = np.abs(y.astype(np.float64) - want)
        assert np.all(err <= bound), (L, float((err / bound).max()))
        assert np.array_equal(q, quantize_ref(y))                               # the int16 output IS the quantised float32 output


def test_tool_table_is_the_library_table(tool):
    for orig, new in ((3, 2), (44100, 16000), (147, 160)):
        tab = _native.resample_table(orig, new)
        plan, _, _, phases = run_tool(tool, orig, new, [0.0], table=True)
        assert plan[4] == tab.stride and plan[5] == tab.words.numel() * 4 and plan[6:8] == [int(tab.taps_in_lds), int(tab.window_in_lds)]
        for p, (k0, cnt, h) in enumerate(phases):
            assert (k0, cnt) == (int(tab.k0[p]), int(tab.cnt[p]))
            assert np.array_equal(h.view(np.uint32), tab.taps[p, :cnt].numpy().view(np.uint32))


def test_tool_quantiser_saturates_and_never_wraps(tool):
    """A full-scale square wave overshoots (Gibbs): both rails are reached, and the sign of every saturated sample is its output's."""
    x = np.where((np.arange(400) // 25) % 2 == 0, 32767, -32768).astype(np.int16)
    _, y, q = run_tool(tool, 44100, 16000, x, pcm=True)
    assert (q == 32767).any() and (q == -32768).any() and y.max() > 1.0 and y.min() < -1.0
    assert np.all(q[y >= 1.0] == 32767) and np.all(q[y <= -1.0] == -32768)
    assert quantize_ref(np.array([np.nan, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, 1e9, -1e9, np.inf], np.float32)).tolist() == \
        [0, 0, 2, 2, 0, 32767, -32768, 32767]


def test_tool_refuses_what_the_entry_refuses(tool):
    assert subprocess.run([tool, "hostile=1"], capture_output=True, text=True).stdout.startswith("hostile ok")
    assert subprocess.run([tool, "orig=0", "new=2"], capture_output=True).returncode == 3
    assert subprocess.run([tool, "orig=3", "new=2", "rolloff=1.5"], capture_output=True).returncode == 3
    assert subprocess.run([tool, "orig=65537", "new=65536"], capture_output=True).returncode == 4


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_exported_and_documented():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    i, ll, sz, vp, dbl = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_double
    want = {"leaf_resample_length": (sz, [ll, i, i]),
            "leaf_resample_table_bytes": (sz, [i, i, i, dbl]),
            "leaf_resample_table_f32": (i, [i, i, i, dbl, vp, sz]),
            "leaf_resample_workspace_bytes": (sz, [i]),
            "leaf_resample_f32": (i, [vp, ll, i, i, vp, vp, i, i, i, dbl, vp, sz, vp, ll, vp, vp, sz, vp])}
    ctype = {"int": i, "long long": ll, "size_t": sz, "double": dbl}
    lib = _native.load()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, (res, args) in want.items():
        m = re.search(r"\n([a-z_ ]+?)\s+" + name + r"\(([^;]*)\);", header)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(2).replace("\n", " ").split(",")]
        declared = [vp if "*" in a else ctype[a.rsplit(" ", 1)[0].replace("const ", "").strip()] for a in params]
        assert ctype[m.group(1).strip()] == res and declared == args, (name, declared)
        assert _native._SIGNATURES[name] == (res, args) and name in _native.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args and name in defined and name in integration
    assert "Resampling from C" in integration
    assert re.search(r"#define LEAF_FLAG_OUT_PCM16 0x400\b", header) and _native.FLAG_OUT_PCM16 == 0x400
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6 and lib.leaf_abi_version() == 6 and _native.ABI_VERSION == 6
    assert leaf_pytorch_amd.resample is leaf_pytorch_amd.transforms.resample and callable(PackedClips.resampled)


def test_refusals_come_in_the_stated_order():
    """Every refusal is answered before any launch, so no pointer below is ever followed: they only have to be non-NULL and aligned."""
    lib = _native.load()
    A = 0x10000                                                                 # 'a pointer': aligned to everything, never read
    nbytes = lib.leaf_resample_table_bytes(3, 2, 6, 0.99)
    assert nbytes == 4 * (8 + 2 * 2 + 2 * 19) and lib.leaf_resample_table_bytes(0, 2, 6, 0.99) == 0
    assert lib.leaf_resample_table_bytes(65537, 65536, 6, 0.99) == 0 and lib.leaf_resample_table_bytes(3, 2, 0, 0.99) == 0
    assert lib.leaf_resample_table_bytes(3, 2, 6, 0.0) == 0 and lib.leaf_resample_table_bytes(3, 2, 6, float("nan")) == 0
    assert lib.leaf_resample_table_bytes(65535, 2, 4096, 1.0) == 0             # a table above 2^26 bytes

    def call(store=A, store_len=100, flags=0, R=2, in_off=A, in_len=A, orig=3, new=2, W=6, rho=0.99, table=A, table_bytes=nbytes,
             out=A, out_total=100, out_off=A, ws=A, ws_bytes=24):
        return lib.leaf_resample_f32(store, store_len, flags, R, in_off, in_len, orig, new, W, rho, table, table_bytes, out, out_total,
                                     out_off, ws, ws_bytes, None)

    # LEAF_ERR_UNSUPPORTED first: an unknown flag, a reduced ratio above 65535, a table above 2^26 bytes -- each with everything else wrong too
    assert call(flags=0x1, store=None, R=0, ws=None) == UNSUPPORTED and call(flags=0x200, store=None) == UNSUPPORTED
    assert call(orig=65537, new=65536, store=None, R=0) == UNSUPPORTED and call(orig=65535, new=2, W=4096, rho=1.0, out=None) == UNSUPPORTED
    # then LEAF_ERR_NULL_POINTER, each required pointer, with a bad shape beside it
    for name in ("store", "in_off", "in_len", "table", "out", "out_off"):
        assert call(**{name: None}, R=0, orig=0) == NULL_POINTER, name
    # then LEAF_ERR_BAD_SHAPE, with a misaligned buffer beside it
    for bad in (dict(R=0), dict(R=-1), dict(store_len=-1), dict(out_total=-1), dict(orig=0), dict(new=-3), dict(W=0), dict(rho=0.0),
                dict(rho=1.0000001), dict(rho=float("nan")), dict(table_bytes=nbytes - 4), dict(table_bytes=nbytes + 4)):
        assert call(**bad, out=A + 2, ws=None) == BAD_SHAPE, bad
    # then LEAF_ERR_ALIGNMENT: element alignment, 2 bytes where a flag makes the buffer int16; with no workspace beside it
    for bad in (dict(store=A + 2), dict(store=A + 1, flags=0x100), dict(in_off=A + 4), dict(in_len=A + 2), dict(table=A + 2), dict(out=A + 2),
                dict(out=A + 1, flags=0x400), dict(out_off=A + 4), dict(ws=A + 8)):
        assert call(**bad, ws_bytes=0) == ALIGNMENT, bad
    assert call(store=A + 2, flags=0x100, out=A + 2, ws=None) == ALIGNMENT    # (float32 out at a 2-byte address)
    # last LEAF_ERR_WORKSPACE
    assert call(ws=None) == WORKSPACE and call(ws_bytes=23) == WORKSPACE and call(store=A + 2, out=A + 2, flags=0x500, ws=None) == WORKSPACE
    # the table builder: the same order
    buf = (ctypes.c_int * (nbytes // 4))()
    assert lib.leaf_resample_table_f32(65537, 65536, 6, 0.99, None, 0) == UNSUPPORTED
    assert lib.leaf_resample_table_f32(3, 2, 6, 0.99, None, 0) == NULL_POINTER and lib.leaf_resample_table_f32(0, 2, 6, 0.99, None, 0) == NULL_POINTER
    assert lib.leaf_resample_table_f32(3, 2, 6, 0.99, buf, nbytes - 4) == BAD_SHAPE and lib.leaf_resample_table_f32(3, 0, 6, 0.99, buf, nbytes) == BAD_SHAPE
    assert lib.leaf_resample_table_f32(3, 2, 6, 0.99, ctypes.c_void_p(ctypes.addressof(buf) + 2), nbytes) == ALIGNMENT
    assert lib.leaf_resample_table_f32(3, 2, 6, 0.99, buf, nbytes) == 0 and list(buf[1:8]) == [3, 2, 10, 19, 1, 0, 0]


# ---- Python -----------------------------------------------------------------------------------------------------------------------------

def test_python_argument_errors():
    x = torch.zeros(2, 30)
    with pytest.raises(TypeError):
        leaf_pytorch_amd.resample(x.double(), 3, 2)
    with pytest.raises(TypeError):
        leaf_pytorch_amd.resample(x.to(torch.int32), 3, 2)
    with pytest.raises(TypeError):
        leaf_pytorch_amd.resample(x, 3, 2, out_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="gradient"):
        leaf_pytorch_amd.resample(x.clone().requires_grad_(), 3, 2)
    for bad in (dict(orig_freq=0), dict(new_freq=-1), dict(orig_freq=2.5), dict(lowpass_filter_width=0), dict(rolloff=0.0), dict(rolloff=1.5),
                dict(rolloff=float("nan")), dict(orig_freq=65537, new_freq=65536)):
        kw = {"orig_freq": 3, "new_freq": 2, **bad}
        with pytest.raises(ValueError):
            leaf_pytorch_amd.resample(x, **kw)
        with pytest.raises(ValueError):
            _native.resample_table(**kw)
    with pytest.raises(RuntimeError, match="AMD GPU"):                          # valid arguments on the CPU: there is no CPU path
        leaf_pytorch_amd.resample(x, 3, 2)
    clips = PackedClips([torch.zeros(5, dtype=torch.int16)])
    with pytest.raises(ValueError):
        clips.resampled(0, 2)
    with pytest.raises(TypeError):
        clips.resampled(3, 2, out_dtype=torch.float64)
    big = PackedClips.from_store(torch.zeros(4, dtype=torch.int16), [0], [4])
    big.lengths_host = torch.tensor([2 ** 31 - 1], dtype=torch.int32)          # (only the integer plan is under test: nothing is launched)
    with pytest.raises(ValueError, match="32-bit"):
        big.resampled(1, 2)
