"""Chunked resampling, the host side (no GPU): the position arithmetic of leaf_resample_stream_plan against an independent Python
oracle of the rule in include/leaf_hip.h -- which outputs a step emits, which samples they read, what is kept -- over every
chunking of short streams and seeded chunkings of long ones; the CPU build of the same header (tools/resample_stream_check.cpp)
against the whole-signal tool, bit for bit; its hostile walk under -fsanitize=undefined,address; the C entries as declared, exported
and documented; their refusals in the stated order; the Python argument errors.  tests/test_gpu_resample_stream.py has the kernel."""
import ctypes
import itertools
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import leaf_pytorch_amd
from leaf_pytorch_amd import ResampleStream, ResampleStreamBank, _native
from test_host_resample import plan_ref, run_tool, samples, tool   # noqa: F401  (tool: the compiled whole-signal program)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, WORKSPACE, ALIGNMENT, UNSUPPORTED = -1, -2, -3, -7, -8
CSRC = os.path.join(REPO, "leaf_pytorch_amd", "csrc")


# ---- the oracle: the rule as the header states it, by linear search ----------------------------------------------------------------------

class StreamRef:
    """One stream under the rule: ``step(Tc, end)`` returns (n, drop_samples) and moves the position.  It also keeps what the rule
    itself does not need -- ``base``, the recording's sample behind V[0], and ``emitted`` -- so that every emitted output's sample
    range can be compared with the whole-signal plan."""

    def __init__(self, ref):
        self.ref = ref
        self.klast = [int(ref.k0[p] + ref.cnt[p] - 1) for p in range(ref.n)]
        self.hist_len, self.shift, self.phase = 0, ref.width, 0
        self.base = self.emitted = self.total = 0

    def step(self, Tc: int, end: bool):
        ref, o, n = self.ref, self.ref.o, self.ref.n
        Lv = self.hist_len + Tc
        E = self.shift + Lv
        self.total += Tc
        g, p, m = 0, self.phase, 0
        while ((g * n + p) * o < n * (E - ref.width)) if end else (g * o + self.klast[p] <= E - 1):
            # the samples this output reads, as places in the recording: V[c - shift] is sample base + c - shift
            lo = self.base + g * o + int(ref.k0[p]) - self.shift
            hi = self.base + g * o + self.klast[p] - self.shift
            j = self.emitted + m
            assert j % n == p and (lo, hi) == ((j // n) * o + int(ref.k0[p]) - ref.width, (j // n) * o + self.klast[p] - ref.width), (j, lo, hi)
            assert max(lo, 0) >= self.base or hi < 0, "a sample the output needs was dropped"
            assert end or hi < self.total, "an output left before its last sample arrived"
            m += 1
            p += 1
            if p == n:
                g, p = g + 1, 0
        self.emitted += m
        if end:
            assert self.emitted == ref.length(self.total)
            drop = Lv
            self.hist_len, self.shift, self.phase = 0, ref.width, 0
            self.base = self.emitted = self.total = 0
            return m, drop
        drop = max(0, g * o - self.shift)
        assert drop <= Lv
        self.base += drop
        self.shift, self.hist_len, self.phase = max(0, self.shift - g * o), Lv - drop, p
        return m, drop


class Planned:
    """One slot through leaf_resample_stream_plan."""

    def __init__(self, orig, new):
        self.key = (orig, new, 6, 0.99)
        self.pos = (_native.ResamplePos * 1)()

    def step(self, Tc: int, end: bool):
        recs, counts = _native.resample_stream_plan(self.key, self.pos, [Tc], [end])
        return recs[0], counts[0]


def walk(orig, new, sizes, flush: bool):
    """Feed the chunk sizes to the library's plan and to the oracle; the stream ends with the last chunk, or (flush) behind it."""
    ref = plan_ref(orig, new)
    want, got = StreamRef(ref), Planned(orig, new)
    H, total, emitted = ref.K - 1, sum(sizes), 0
    steps = [(Tc, i == len(sizes) - 1 and not flush) for i, Tc in enumerate(sizes)] + ([(0, True)] if flush else [])
    for Tc, end in steps:
        before = (got.pos[0].running, got.pos[0].hist_len, got.pos[0].shift, got.pos[0].phase, got.pos[0].parity)
        idle = Tc == 0 and not (end and before[0])
        r, n = got.step(Tc, end)
        if idle:
            assert r.idle == 1 and n == 0 and before == (got.pos[0].running, got.pos[0].hist_len, got.pos[0].shift, got.pos[0].phase, got.pos[0].parity)
            continue
        state = (want.hist_len, want.shift, want.phase)
        m, drop = want.step(Tc, end)
        assert (r.idle, r.hist_len, r.shift, r.phase, r.Tc, r.n, r.drop_samples, r.end) == (0, *state, Tc, m, drop, int(end)), (sizes, Tc, end)
        assert n == m and r.parity == before[4] and got.pos[0].parity == before[4] ^ 1
        emitted += m
        p = got.pos[0]
        assert p.running == (0 if end else 1)
        if not end:
            assert (p.hist_len, p.shift, p.phase) == (want.hist_len, want.shift, want.phase) and p.hist_len <= H
    assert emitted == ref.length(total), (sizes, emitted)
    return emitted


def compositions(T: int):
    for cuts in itertools.product((0, 1), repeat=max(T - 1, 0)):
        parts, run = [], 1
        for c in cuts:
            if c:
                parts.append(run)
                run = 1
            else:
                run += 1
        yield parts + [run] if T else []


@pytest.mark.parametrize("orig,new", [(3, 2), (2, 3)])
def test_plan_over_every_composition_of_short_streams(orig, new):
    for T in range(1, 13):
        for parts in compositions(T):
            walk(orig, new, parts, flush=False)
    for parts in compositions(7):
        walk(orig, new, parts, flush=True)


@pytest.mark.parametrize("orig,new", [(3, 1), (441, 160), (147, 160), (2, 1), (1, 1), (1, 3)])
def test_plan_over_seeded_chunkings(orig, new):
    ref = plan_ref(orig, new)
    rng = random.Random(1000 * orig + new)
    for T in (0, 1, ref.width, ref.K - 1, ref.K, ref.K + 1, 4000 + rng.randrange(100)):
        for trial in range(3):
            sizes, left = [], T
            while left > 0:
                Tc = min(left, rng.choice((0, 1, 2, 3, rng.randrange(0, 40), rng.randrange(0, 2001))))
                sizes.append(Tc)
                left -= Tc
            sizes += [0] * trial                                                # (trailing empty chunks: the last one carries `end`)
            a = walk(orig, new, sizes or [0], flush=False)
            b = walk(orig, new, sizes or [0], flush=True)                       # `end` on the last chunk = the step, then a flush
            assert a == b == ref.length(T)


def test_plan_serves_a_bank_and_moves_all_or_none():
    lib = _native.load()
    key = (44100, 16000, 6, 0.99)
    pos = (_native.ResamplePos * 4)()
    recs, counts = _native.resample_stream_plan(key, pos, [441, 0, 4410, 17], [False, True, False, True])
    assert [r.idle for r in recs] == [0, 1, 0, 0] and counts[1] == 0       # `end` on a slot that is not running does nothing
    assert counts[0] == Planned(*key[:2]).step(441, False)[1] and counts[3] == plan_ref(441, 160).length(17)
    assert [p.running for p in pos] == [1, 0, 1, 0] and [p.parity for p in pos] == [1, 0, 1, 1]
    before = bytes(pos)
    with pytest.raises(ValueError):                                           # one bad length: no slot moves
        _native.resample_stream_plan(key, pos, [5, 5, 5, _native.RESAMPLE_STREAM_MAX_CHUNK + 1], [False] * 4)
    with pytest.raises(ValueError):
        _native.resample_stream_plan(key, pos, [5, -1, 5, 5], [False] * 4)
    assert bytes(pos) == before
    pos[2].hist_len = 475                                                       # a position outside its range (H = 474)
    with pytest.raises(ValueError):
        _native.resample_stream_plan(key, pos, [5, 5, 5, 5], [False] * 4)
    vp = ctypes.c_void_p
    assert lib.leaf_resample_stream_plan(0, *key, None, None, None, None, None) == 0
    assert lib.leaf_resample_stream_plan(1, *key, None, None, None, None, None) == NULL_POINTER
    assert lib.leaf_resample_stream_plan(1, 16, 1, 6, 0.99, None, None, None, None, None) == UNSUPPORTED
    one = (_native.ResamplePos * 1)()
    ints, slot = (ctypes.c_int * 1)(3), (_native.ResampleSlot * 1)()
    args = [ctypes.cast(a, vp) for a in (one, ints, ints, slot, ints)]
    assert lib.leaf_resample_stream_plan(-1, *key, *args) == BAD_SHAPE and lib.leaf_resample_stream_plan(1, 0, 2, 6, 0.99, *args) == BAD_SHAPE


# ---- the CPU build of the header, chunk by chunk ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stream_tools(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    d = tmp_path_factory.mktemp("resample_stream")
    src = os.path.join(REPO, "tools", "resample_stream_check.cpp")
    plain, san = str(d / "resample_stream_check"), str(d / "resample_stream_check_san")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, src, "-o", plain], check=True)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", CSRC,
                    src, "-o", san], check=True)
    return plain, san


def run_stream_tool(exe, orig, new, x, sizes, pcm=False, flush=False):
    """The chunked tool on the samples ``x``: (plan line, step lines as int lists, y float32, q int16)."""
    xs = ",".join(str(int(v)) for v in x) if pcm else ",".join(float(v).hex() for v in np.asarray(x, dtype=np.float32))
    run = subprocess.run([exe, f"orig={orig}", f"new={new}", f"pcm={int(pcm)}", f"flush={int(flush)}", f"x={xs}",
                          "chunks=" + ",".join(str(s) for s in sizes)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    lines = run.stdout.splitlines()
    plan = [int(v) for v in lines[0].split()[1:]]
    steps = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("step ")]
    ys = [ln.split() for ln in lines if ln.startswith("y ")]
    y = np.array([int(f[2], 16) for f in ys], dtype=np.uint32).view(np.float32)
    q = np.array([int(f[3]) for f in ys], dtype=np.int64).astype(np.int16)
    return plan, steps, y, q


@pytest.mark.parametrize("orig,new", [(3, 2), (2, 3), (48000, 16000), (44100, 16000), (44100, 48000), (5, 5)])
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
def test_chunked_tool_has_the_bits_of_the_whole_signal_tool(tool, stream_tools, orig, new, dtype):   # noqa: F811
    ref = plan_ref(orig, new)
    pcm = dtype == torch.int16
    rng = random.Random(orig + 7 * new)
    for L in (0, 1, ref.width, ref.K + 1, 3 * ref.o + 700):
        x = samples(dtype, L, 300 + L)
        _, y, q = run_tool(tool, orig, new, x, pcm=pcm)
        chunkings = [[], [1] * min(L, 60), [rng.choice((0, 1, 2, 3, rng.randrange(0, 300))) for _ in range(12)]]
        for sizes, flush in itertools.product(chunkings, (False, True)):
            plan, steps, ys, qs = run_stream_tool(stream_tools[0], orig, new, x, sizes, pcm=pcm, flush=flush)
            assert plan == [ref.o, ref.n, ref.width, ref.K, ref.K - 1, ref.length(L)]
            assert np.array_equal(ys.view(np.uint32), y.view(np.uint32)) and np.array_equal(qs, q), (L, sizes, flush)
            assert sum(s[5] for s in steps) == ref.length(L) and all(s[2] <= ref.K - 1 for s in steps)


def test_hostile_walk_under_the_sanitizers(stream_tools):
    for exe in stream_tools:
        run = subprocess.run([exe, "hostile=1"], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("hostile ok "), (run.stdout, run.stderr[-2000:])
    assert subprocess.run([stream_tools[0], "orig=16", "new=1"], capture_output=True).returncode == 4      # the step's own refusal
    assert subprocess.run([stream_tools[0], "orig=0", "new=1"], capture_output=True).returncode == 3


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_exported_and_documented():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    i, ll, sz, vp, dbl = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_double
    want = {"leaf_resample_stream_history_samples": (i, [i, i, i, dbl]),
            "leaf_resample_stream_state_bytes": (sz, [i, i, i, i, dbl, i]),
            "leaf_resample_stream_plan": (i, [i, i, i, i, dbl, vp, vp, vp, vp, vp]),
            "leaf_resample_stream_step_f32": (i, [vp, ll, i, vp, i, vp, sz, i, i, i, i, dbl, vp, sz, vp, vp])}
    ctype = {"int": i, "long long": ll, "size_t": sz, "double": dbl}
    lib = _native.load()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    readme = open(os.path.join(REPO, "README.md")).read()
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
    assert "typedef struct leaf_resample_slot { int idle; int hist_len, Tc, parity, shift, phase, n, drop_samples, end; } leaf_resample_slot;" in flat
    assert "typedef struct leaf_resample_pos { int running, hist_len, shift, phase, parity; } leaf_resample_pos;" in flat
    assert tuple(n for n, _ in _native.ResampleSlot._fields_) == ("idle", "hist_len", "Tc", "parity", "shift", "phase", "n", "drop_samples", "end")
    assert tuple(n for n, _ in _native.ResamplePos._fields_) == ("running", "hist_len", "shift", "phase", "parity")
    assert ctypes.sizeof(_native.ResampleSlot) == 36 and ctypes.sizeof(_native.ResamplePos) == 20
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6 and lib.leaf_abi_version() == 6 and _native.ABI_VERSION == 6
    assert "ResampleStreamBank" in readme and "ResampleStream(" in readme and "Streaming from C" in integration
    for text in (header, readme):                                               # no longer on the lists of what is not built
        assert "a streaming resampler" not in text
    assert leaf_pytorch_amd.ResampleStream is ResampleStream and leaf_pytorch_amd.ResampleStreamBank is ResampleStreamBank
    assert "ResampleStream" in leaf_pytorch_amd.__all__ and "ResampleStreamBank" in leaf_pytorch_amd.__all__


def test_size_queries():
    lib = _native.load()
    H = lib.leaf_resample_stream_history_samples
    assert [H(44100, 16000, 6, 0.99), H(48000, 16000, 6, 0.99), H(16000, 16000, 6, 0.99)] == [474, 40, 0]
    for orig, new in ((3, 2), (44100, 48000), (16000, 8000)):
        assert H(orig, new, 6, 0.99) == plan_ref(orig, new).K - 1
    assert H(16, 1, 6, 0.99) == 0 and H(44100, 2000, 6, 0.99) == 0 and H(0, 2, 6, 0.99) == 0 and H(65537, 65536, 6, 0.99) == 0
    S = lib.leaf_resample_stream_state_bytes
    assert S(3, 44100, 16000, 6, 0.99, 0) == 2 * 5888 and S(3, 44100, 16000, 6, 0.99, 0x100) == 2 * 3072   # [3][474] made a multiple of 256
    assert S(3, 44100, 16000, 6, 0.99, 0x400) == 2 * 5888 and S(1, 5, 5, 6, 0.99, 0) == 512
    assert S(0, 3, 2, 6, 0.99, 0) == 0 and S(1, 16, 1, 6, 0.99, 0) == 0 and S(1, 3, 2, 6, 0.99, 0x1) == 0 and S(1, 3, 2, 0, 0.99, 0) == 0


def test_refusals_come_in_the_stated_order():
    """Every refusal is answered before any launch, so no device pointer below is ever followed: they only have to be non-NULL and
    aligned.  The slot records are host memory and are read."""
    lib = _native.load()
    A = 0x10000
    key = (3, 2, 6, 0.99)
    nbytes = lib.leaf_resample_table_bytes(*key)
    state_bytes = lib.leaf_resample_stream_state_bytes(2, *key, 0)
    ref = plan_ref(3, 2)
    good = Planned(3, 2).step(30, False)[0]

    def slot(**kw):
        s = _native.ResampleSlot()
        for name, _ in _native.ResampleSlot._fields_:
            setattr(s, name, kw.get(name, getattr(good, name)))
        return s

    def call(slots=None, chunk=A, stride=64, B=2, n_max=None, state=A, sbytes=state_bytes, flags=0, orig=3, new=2, W=6, rho=0.99, table=A,
             table_bytes=nbytes, out=A):
        arr = (_native.ResampleSlot * 2)(*(slots or [slot(), slot()]))
        n_max = max(s.n for s in arr) if n_max is None else n_max
        return lib.leaf_resample_stream_step_f32(chunk, stride, B, ctypes.cast(arr, ctypes.c_void_p), n_max, state,
                                                 sbytes, flags, orig, new, W, rho, table, table_bytes, out, None)

    bad_slot = [slot(hist_len=ref.K), slot()]
    # LEAF_ERR_UNSUPPORTED first: a flag, a ratio beyond the library, a ratio whose window does not fit LDS -- with everything else wrong too
    assert call(flags=0x1, state=None, B=-1) == UNSUPPORTED and call(flags=0x200, table=None) == UNSUPPORTED
    assert call(orig=65537, new=65536, state=None) == UNSUPPORTED and call(orig=16, new=1, state=None, B=-1) == UNSUPPORTED
    assert call(orig=44100, new=2000, table=None) == UNSUPPORTED
    assert call(B=0, state=None, table=None, out=None) == 0                     # B = 0: nothing to do
    # then LEAF_ERR_NULL_POINTER, with a bad shape beside it
    for name in ("state", "table", "out", "chunk"):
        assert call(**{name: None}, W=0) == NULL_POINTER, name
    assert lib.leaf_resample_stream_step_f32(A, 64, 2, None, 5, A, state_bytes, 0, *key, A, nbytes, A, None) == NULL_POINTER
    # no slot has samples, emits or keeps anything: neither chunk nor out is needed, and nothing is launched
    assert call(slots=[slot(Tc=0, n=0, hist_len=0, drop_samples=0), slot(idle=1)], chunk=None, out=None, n_max=0) == 0
    # then LEAF_ERR_BAD_SHAPE, with a misaligned buffer beside it
    for bad in (dict(B=-1), dict(n_max=-1), dict(orig=0), dict(new=-3), dict(W=0), dict(rho=0.0), dict(rho=float("nan")), dict(table_bytes=nbytes - 4),
                dict(slots=[slot(idle=2), slot()]), dict(slots=[slot(Tc=-1), slot()]), dict(slots=[slot(Tc=(1 << 20) + 1), slot()]), dict(stride=29)):
        assert call(**bad, out=A + 2) == BAD_SHAPE, bad
    # then LEAF_ERR_ALIGNMENT, with a bad position beside it
    for bad in (dict(state=A + 8), dict(chunk=A + 2), dict(chunk=A + 1, flags=0x100), dict(table=A + 2), dict(out=A + 2), dict(out=A + 1, flags=0x400)):
        assert call(**bad, slots=bad_slot) == ALIGNMENT, bad
    # then the positions, in the stated order, each with too small a state beside it
    n = good.n
    for bad in (dict(hist_len=ref.K), dict(hist_len=-1), dict(shift=ref.width + 1), dict(shift=-1), dict(phase=ref.n), dict(phase=-1), dict(parity=2),
                dict(end=2), dict(drop_samples=31), dict(drop_samples=-1), dict(Tc=30 + ref.K, drop_samples=0), dict(n=n + 1), dict(n=n - 1)):
        assert call(slots=[slot(), slot(**bad)], sbytes=0, n_max=n + 1) == BAD_SHAPE, bad
    assert call(n_max=n - 1, sbytes=0) == BAD_SHAPE                             # n <= n_max
    # the first failing check decides: with hist_len out of range nothing behind it is computed from it
    assert call(slots=[slot(hist_len=2 ** 31 - 1, Tc=1 << 20, shift=-5, phase=-5, n=-5), slot()], sbytes=0) == BAD_SHAPE
    # last LEAF_ERR_WORKSPACE
    assert call(sbytes=state_bytes - 1) == WORKSPACE and call(sbytes=0) == WORKSPACE


# ---- Python -----------------------------------------------------------------------------------------------------------------------------

def test_python_argument_errors():
    for bad in (dict(orig_freq=0), dict(new_freq=-1), dict(orig_freq=2.5), dict(lowpass_filter_width=0), dict(rolloff=0.0), dict(rolloff=1.5),
                dict(orig_freq=65537, new_freq=65536), dict(orig_freq=16, new_freq=1), dict(orig_freq=44100, new_freq=2000),
                dict(out_dtype=torch.bfloat16)):
        kw = {"orig_freq": 3, "new_freq": 2, **bad}
        with pytest.raises(ValueError):
            ResampleStream(**kw)
        with pytest.raises(ValueError):
            ResampleStreamBank(slots=2, **kw)
    for bad in (dict(slots=0), dict(slots=-1), dict(slots=1.5), dict(sample_dtype=torch.float64), dict(sample_dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            ResampleStreamBank(48000, 16000, **{"slots": 2, **bad})
    bank = ResampleStreamBank(48000, 16000, slots=2, sample_dtype=torch.int16)
    assert (bank.history, bank.max_chunk, bank.out_dtype) == (40, 1 << 20, torch.int16) and bank.max_chunk >= 65536
    before = bytes(bank.pos)
    x = torch.zeros(2, 30, dtype=torch.int16)
    for chunk, lengths, end in ((x, [30], None), (x, [30, 30, 30], None), (x, [30, 30], [True]), (x, [30, -1], None),
                                (x, [30, (1 << 20) + 1], None), (x.float(), [30, 30], None), (x[:1], [30, 30], None), (x[0], [30, 30], None),
                                (x.reshape(2, 2, 15), [30, 30], None)):
        with pytest.raises(ValueError):
            bank.step(chunk, lengths, end)
    with pytest.raises(RuntimeError, match="AMD GPU"):                          # valid arguments on the CPU: there is no CPU path
        bank.step(x, [30, 30])
    assert bytes(bank.pos) == before and bank.state_buf is None and bank.running == [False, False]   # nothing moved
    y, counts = bank.flush()                                                    # nothing has ever run
    assert tuple(y.shape) == (2, 0) and counts == [0, 0]
    rs = ResampleStream(48000, 16000)
    for chunk in (x.double(), x.to(torch.int32), x[0], torch.zeros(0, 5), "x"):
        with pytest.raises(ValueError):
            rs.step(chunk)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        rs.step(x)
    assert tuple(rs.flush().shape) == (0, 0) and not rs.open
