"""Streaming parity at recording-length, chunk and frame-count edges: LeafStream(fused=True), the raw leaf_stream_step_f32,
LeafStreamBank and the two-launch LeafStream on the lattice of tests/stream_edges_cases.py (the streaming counterpart of
tests/test_gpu_forward_edges.py; tests/test_host_stream_edges.py holds the cases' twin, mutations, coverage and conditioning).

A recording of T samples is cut by a chunking, streamed and flushed.  Every case asserts

  1. fused stream: every step()'s frame count is stream_plan's (pieces of an over-long chunk summed), the total (T - 1) // hop + 1; the
     concatenation within STREAM_TOL = 1e-5 of the product's whole-clip forward and ORACLE_TOL = 2e-5 of the fp64 oracle (the
     project's own figures, as tests/test_gpu_stream_fused.py); B = 1 and 3, three parameter sets and the F = 1 module, ONE stream
     object per configuration reused from case to case (its state buffer is never cleared).  Bit for bit: row 0 of a B = 3 stream
     against the B = 1 stream of every case; on the subset (a), (c) hop + 1, (e) 0, (f) every row alone, int16 against v / 32768,
     bfloat16 against float32 rounded, and a second stream after flush() on a state buffer poisoned with 0xFF before the first;
  2. raw leaf_stream_step_f32 windows (first, n) of a whole recording with hist_len = 0, started = 0 -- c_lo up to 9, n up to 129,
     which the Python layer never asks for -- on guarded, poisoned buffers: guards intact, every element written, ORACLE_TOL against
     the oracle's frames (log1p) and against its PCEN with the smoother started at frame `first`;
  3. LeafStreamBank: three slots, each a sequence of lattice streams (the three ending regimes drop <, ==, > hist_len, an end on a
     chunk that completes nothing, an end without samples, reused and idle slots), and 130 slots in two launches: every finished
     stream bit-equal to its one-waveform fused stream and within STREAM_TOL of the whole clip;
  4. two-launch LeafStream: the full lattice at 401 / 160, the reduced one at 201 / 80, 552 / 220, 801 / 320, 1103 / 441: the same
     bounds, and the step shapes of the fused stream's plan;
  5. every event of the coverage list ran on the device (RAN).

Every test prints its case count and worst figures; with LEAF_STREAM_EDGE_LOG set they are appended there as JSON lines
(profiles/stream_edges.txt).

Found with this file and fixed: nothing.  All 45 tests pass on an MI355X against the kernels and the host code as they stood: 7120 fused
streams within 1.21e-6 of the whole clip and 1.23e-6 of the fp64 oracle, 1564 raw windows within 7.2e-7 of the oracle, every bank
stream bit-equal to its single stream, the two-launch stream within 1.01e-6 / 1.28e-6.  What the bounds can see is shown on the CPU
(tests/test_host_stream_edges.py): a frame emitted one sample early, a hop dropped too soon, a sample lost at the history seam, a
forgotten smoother carry (per step, per group of 64 frames) and clip-end padding at a non-final step each leave 2e-5 at a case of this
lattice -- the first two only with the "wide" parameter set, which is why it is here."""
import ctypes
import functools
import json
import os

import pytest
import torch

import leaf_pytorch_amd as L
import stream_edges_cases as se
from conftest import rel_err
from guarded import guarded, guarded_tensor, unchanged
from helpers import make_leaf
from leaf_pytorch_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STREAM_TOL = 1e-5     # the project's streaming tolerance (tests/test_gpu_dropin.py, tests/test_gpu_stream_fused.py), restated
ORACLE_TOL = 2e-5     # what the parity tests assert against the oracle
PRM = ("_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta", "_compression.root",
       "_compression.ema._weights")
_LOG = os.environ.get("LEAF_STREAM_EDGE_LOG")
RAN = {}              # geometry id -> events of the coverage list that ran on the device
_ALONE = {}           # (geometry, set, F, T, chunking) -> the B = 1 fused stream's frames, for the B = 3 test's row 0
G16, G8 = se.geo(401, 160), se.geo(201, 80)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    _native.load()


def record(part, what, **figures):
    print(f"part {part} {what}: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))
    if _LOG:
        with open(_LOG, "a") as fh:
            fh.write(json.dumps(dict(part=part, what=what, **figures)) + "\n")


@functools.lru_cache(maxsize=None)
def module(K, hop, pset, nf=se.F):
    """The product module of a parameter set, loaded with load_state_dict; shared, never modified."""
    return make_leaf(nf, K, hop, True, se.params(se.geo(K, hop), pset, nf), DEV)


def run_stream(stream, x, sizes):
    """x (B, 1, T) cut by `sizes` (views: nothing is copied), then flush(): the frames of every call."""
    outs, pos = [], 0
    for s in sizes:
        outs.append(stream.step(x[:, :, pos:pos + s]))
        pos += s
    return outs + [stream.flush()]


def whole_clip(m, x):
    with torch.no_grad():
        return m(x).cpu()


class Worst:
    def __init__(self):
        self.clip, self.oracle, self.cases = (-1.0, ""), (-1.0, ""), 0

    def take(self, where, cat, want, ref):
        e, eo = rel_err(cat, want), rel_err(cat, ref)
        self.clip, self.oracle, self.cases = max(self.clip, (e, where)), max(self.oracle, (eo, where)), self.cases + 1
        assert e < STREAM_TOL, f"{where}: stream {e:.3e} from the whole clip (bound {STREAM_TOL:.0e})"
        assert eo < ORACLE_TOL, f"{where}: stream {eo:.3e} from the fp64 oracle (bound {ORACLE_TOL:.0e})"

    def figures(self):
        return dict(cases=self.cases, vs_whole_clip=self.clip[0], at=str(self.clip[1]), vs_oracle=self.oracle[0], oracle_at=str(self.oracle[1]))


def lattice_through(g, pset, nf, B, fused, ts=None, kinds="abcdef"):
    """Every (T, chunking) through one stream object: the step shapes, the total, both bounds; the fused stream's events go to RAN."""
    m = module(g.K, g.hop, pset, nf)
    stream = L.LeafStream(m, fused=fused)
    worst = Worst()
    for T in (se.lattice(g) if ts is None else ts):
        x = se.signal(g.K, g.hop, T)[:B].to(DEV)
        want, ref = whole_clip(m, x), se.oracle(g, pset, T, nf)[:B]
        assert want.shape == ref.shape == (B, nf, (T - 1) // g.hop + 1)
        for name, sizes in se.chunkings(g, T, kinds, ts):
            where = f"{se.gid(g)} {pset} F={nf} B={B} T={T} {name}"
            outs = run_stream(stream, x, sizes)
            assert [o.shape[-1] for o in outs] == se.counts_per_chunk(g, sizes), where
            assert all(o.shape[:2] == (B, nf) and o.dtype == torch.float32 for o in outs), where
            cat = torch.cat(outs, dim=-1).cpu()
            assert cat.shape == want.shape and bool(torch.isfinite(cat).all()), where
            worst.take(where, cat, want, ref)
            if fused:
                RAN.setdefault(se.gid(g), set()).update(se.events(g, sizes))
                key = (se.gid(g), pset, nf, T, name)
                if B == 1:
                    _ALONE[key] = cat
                elif key in _ALONE:
                    assert torch.equal(cat[:1], _ALONE[key]), f"{where}: row 0 of the B = 3 stream against the same stream run alone, bit for bit"
    return worst


# ---- 1. the lattice through LeafStream(fused=True)
CONFIGS = [(pset, se.F, B) for pset in se.PSETS for B in (1, 3)] + [("away", 1, 1), ("away", 1, 3)]


@pytest.mark.parametrize("pset,nf,B", CONFIGS, ids=[f"{p}-F{nf}-B{B}" for p, nf, B in CONFIGS])
@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_fused_stream_on_the_lattice(g, pset, nf, B):
    worst = lattice_through(g, pset, nf, B, True)
    record(1, f"{se.gid(g)} {pset} F={nf} B={B}", **worst.figures())


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_fused_stream_bit_for_bit(g, monkeypatch):
    """On the subset of chunkings, B = 3, the "away" set: every row alone, int16 PCM, bfloat16 frames, and a reused object whose state
    buffer was poisoned with 0xFF (NaN as float32, -1 as int16) before its first stream."""
    m = module(g.K, g.hop, "away")
    plain, rows, bf16 = L.LeafStream(m, fused=True), L.LeafStream(m, fused=True), L.LeafStream(m, fused=True, out_dtype=torch.bfloat16)
    from_int, from_float = L.LeafStream(m, fused=True), L.LeafStream(m, fused=True)
    made, armed, fresh = [], [False], _native.stream_state
    monkeypatch.setattr(_native, "stream_state", lambda *a: (made.append(fresh(*a).fill_(0xFF)) or made[-1]) if armed[0] else fresh(*a))
    poisoned = L.LeafStream(m, fused=True)
    cases = 0
    for T in se.lattice(g):
        x = se.signal(g.K, g.hop, T).to(DEV)
        pcm = se.pcm16(x)
        scaled = pcm.float() / 32768
        for name, sizes in se.bitwise_subset(g, T):
            where = f"{se.gid(g)} T={T} {name}"
            f32 = run_stream(plain, x, sizes)
            for b in range(3):
                alone = run_stream(rows, x[b:b + 1], sizes)
                assert all(torch.equal(a, o[b:b + 1]) for a, o in zip(alone, f32)), f"{where}: row {b} alone"
            a16, af = run_stream(from_int, pcm, sizes), run_stream(from_float, scaled, sizes)
            assert all(a.dtype == torch.float32 and torch.equal(a, b) for a, b in zip(a16, af)), f"{where}: int16 against v / 32768"
            ab = run_stream(bf16, x, sizes)
            assert all(a.dtype == torch.bfloat16 and torch.equal(a, b.to(torch.bfloat16)) for a, b in zip(ab, f32)), f"{where}: bfloat16 frames"
            armed[0] = True                                               # (the object allocates in its first step, once)
            first, second = run_stream(poisoned, x, sizes), run_stream(poisoned, x, sizes)
            armed[0] = False
            assert all(torch.equal(a, o) and torch.equal(b, o) for a, b, o in zip(first, second, f32)), f"{where}: a second stream on a poisoned state"
            cases += 1
    assert len(made) == 1                                                 # allocated once, poisoned, kept over every flush()
    record(1, f"{se.gid(g)} bit for bit", cases=cases)


# ---- 2. frame windows through the raw entry point
@pytest.mark.parametrize("mode", ["log1p", "pcen"])
@pytest.mark.parametrize("g,T", [(g, T) for g in (G16, G8) for T in se.window_lengths(g)], ids=lambda v: se.gid(v) if isinstance(v, se.Geo) else f"T{v}")
def test_raw_windows(g, T, mode):
    B, nf, pset = 2, se.F, "wide"
    lib = _native.load()
    sd = {k: v.to(DEV).contiguous() for k, v in se.params(g, pset).items()}
    prm = [ctypes.c_void_p(sd[k].data_ptr()) for k in PRM]
    flags = _native.FLAG_PCEN if mode == "pcen" else _native.FLAG_LOG1P
    x = guarded_tensor(se.signal(g.K, g.hop, T)[:B].to(DEV))              # exactly B T samples: nothing is read past the recording
    nbytes = lib.leaf_stream_state_bytes(B, nf, g.K, g.hop, flags)
    state = guarded(nbytes, 0xFF)
    wins = se.windows(g, T)
    out = guarded(0, 0xFF, capacity=B * nf * max(n for _, n in wins) * 4)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    worst, ran = (-1.0, ""), RAN.setdefault(se.gid(g), set())
    for first, n in wins:
        out.relayout(B * nf * n * 4).fill(0xFF)
        rc = lib.leaf_stream_step_f32(x.ptr, B, T, T, state.ptr, nbytes, 0, 0, T, first, n, 0, *prm, nf, g.K, g.hop, flags, out.ptr, stream)
        assert rc == 0, (T, first, n, rc)
        torch.cuda.synchronize()
        got = out.cpu(torch.float32, (B, nf, n))
        where = f"{se.gid(g)} T={T} first={first} n={n} {mode}"
        out.check(f"out, {where}")
        state.check(f"state, {where}")
        assert bool(torch.isfinite(got).all()), f"{where}: an element of out was not written"
        e = rel_err(got, se.window_oracle(g, pset, T, first, n, mode)[:B])
        worst = max(worst, (e, where))
        assert e < ORACLE_TOL, f"{where}: {e:.3e} from the fp64 oracle's frames (bound {ORACLE_TOL:.0e})"
        c_lo, nb = se.stream_blocks(g, first, n, T)
        ran.update({f"raw c_lo=={c_lo}", f"raw n=={n}", f"raw nb=={nb}"})
    unchanged(x, "the recording")
    record(2, f"{se.gid(g)} T={T} {mode}", cases=len(wins), vs_oracle=worst[0], at=worst[1])


# ---- 3. the lattice through LeafStreamBank
def drive_bank(bank, script, waves):
    """`script` through `bank` (tests/test_gpu_stream_bank.py, _drive): slot b's samples are consecutive samples of waves[b], the rest of
    a chunk row is NaN.  Returns per slot its finished streams in order: [([chunks], frames concatenated)]."""
    B = bank.slots
    pos, chunks, frames, done = [0] * B, [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    for row in script:
        lengths, end = [r[0] for r in row], [bool(r[1]) for r in row]
        Tmax, chunk = max(lengths), None
        if Tmax:
            chunk = torch.full((B, 1, Tmax), float("nan"), device=DEV)
            for b, n in enumerate(lengths):
                if n:
                    chunk[b, 0, :n] = waves[b][pos[b]:pos[b] + n]
                    chunks[b].append(waves[b][pos[b]:pos[b] + n])
                    pos[b] += n
        running = list(bank.running)
        out, counts = bank.step(chunk, lengths, end)
        assert out.shape == (B, bank.F, max(counts)) and out.dtype == torch.float32
        tail = torch.arange(out.shape[-1], device=DEV)[None, None, :] >= torch.tensor(counts, device=DEV)[:, None, None]
        assert bool((out.masked_select(tail.expand_as(out)) == 0).all()), "a row behind its frames is not zero"
        for b in range(B):
            if lengths[b] or (end[b] and running[b]):
                frames[b].append(out[b:b + 1, :, :counts[b]].clone())
            else:
                assert counts[b] == 0
            if end[b] and (running[b] or lengths[b]):
                done[b].append((chunks[b], torch.cat(frames[b], dim=-1)))
                chunks[b], frames[b] = [], []
    assert not any(bank.running)
    return done


def check_bank_stream(m, single, g, T, sizes, chunks, got, worst, where):
    assert [c.numel() for c in chunks] == sizes, where
    want = torch.cat([single.step(c.reshape(1, 1, -1)) for c in chunks] + [single.flush()], dim=-1)
    assert got.shape == want.shape == (1, m._complex_conv._filters, (T - 1) // g.hop + 1), where
    assert torch.equal(got, want), f"{where}: {(got != want).sum().item()} elements differ from the one-waveform fused stream"
    e = rel_err(got.cpu(), whole_clip(m, torch.cat(chunks).reshape(1, 1, -1)))
    assert e < STREAM_TOL, f"{where}: {e:.3e} from the whole clip (bound {STREAM_TOL:.0e})"
    return max(worst, (e, where))


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_bank_on_the_lattice(g):
    m = module(g.K, g.hop, "away")
    script, order = se.bank_script(g)
    bank = L.LeafStreamBank(m, 3)
    events = se.bank_events(g, script, L.LeafStreamBank(m, 3)._plan)      # (a second bank's bookkeeping: nothing is launched through it)
    waves = [torch.cat([se.signal(g.K, g.hop, T)[0, 0] for T, _ in slot]).to(DEV) for slot in order]
    done = drive_bank(bank, script, waves)
    single, worst, n = L.LeafStream(m, fused=True), (-1.0, ""), 0
    for b, slot in enumerate(order):
        assert len(done[b]) == len(slot)
        for (T, sizes), (chunks, got) in zip(slot, done[b]):
            worst, n = check_bank_stream(m, single, g, T, sizes, chunks, got, worst, f"{se.gid(g)} slot {b} T={T}"), n + 1
    assert events == set(se.BANK_EVENTS)
    RAN.setdefault(se.gid(g), set()).update("bank " + e for e in events)
    record(3, f"{se.gid(g)} bank of 3", cases=n, steps=len(script), vs_whole_clip=worst[0], at=worst[1])


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_bank_of_130_slots(g):
    """Two launches (a launch holds 128 slots): the lattice streams sit behind the split, in slots 127 .. 129."""
    m = module(g.K, g.hop, "away")
    script, lat = se.wide_bank_script(g)
    lengths = [sum(row[b][0] for row in script) for b in range(130)]
    waves = [se.signal(g.K, g.hop, T)[0, 0].to(DEV) for T in lengths]
    done = drive_bank(L.LeafStreamBank(m, 130), script, waves)
    single, worst = L.LeafStream(m, fused=True), (-1.0, "")
    assert all(len(d) == 1 for d in done)
    for b in (0, 1, 2, 126, 127, 128, 129):
        T, sizes = lat.get(b, (lengths[b], [lengths[b]]))
        worst = check_bank_stream(m, single, g, T, sizes, *done[b][0], worst, f"{se.gid(g)} slot {b} of 130 T={T}")
    RAN.setdefault(se.gid(g), set()).add("bank of 130")
    record(3, f"{se.gid(g)} bank of 130", cases=7, vs_whole_clip=worst[0], at=worst[1])


# ---- 4. the lattice through the two-launch LeafStream
@pytest.mark.parametrize("B", [1, 3])
def test_two_launch_stream_on_the_16k_lattice(B):
    worst = lattice_through(G16, "away", se.F, B, False)
    record(4, f"401-160 away B={B}", **worst.figures())


@pytest.mark.parametrize("pset", ["away", "wide"])
@pytest.mark.parametrize("K,hop", [(201, 80)] + list(se.TWO_LAUNCH_ONLY), ids=lambda v: str(v))
def test_two_launch_stream_on_the_reduced_lattice(K, hop, pset):
    g = se.geo(K, hop)
    worst = lattice_through(g, pset, se.F, 3, False, ts=se.reduced_lattice(g), kinds="acd")
    record(4, f"{se.gid(g)} {pset} B=3 reduced", **worst.figures())


# ---- 5. what ran
def test_every_event_of_the_coverage_list_ran():
    """Every event of the coverage list ran on the device.  (Run on its own, or with a selection that left some out, this test runs what
    is missing: one configuration of the lattice, the banks, the raw windows.)"""
    for g in (G16, G8):
        want = set(se.STREAM_EVENTS + (se.EVENTS_8K if g is G8 else ()))
        if not want <= RAN.get(se.gid(g), set()):
            lattice_through(g, "away", se.F, 1, True)
        if not {"bank " + e for e in se.BANK_EVENTS} <= RAN[se.gid(g)]:
            test_bank_on_the_lattice(g)
        if "bank of 130" not in RAN[se.gid(g)]:
            test_bank_of_130_slots(g)
        raw = {"raw c_lo==1", "raw c_lo==4", "raw c_lo==9", "raw nb==1"} | {f"raw n=={n}" for n in se.WINDOW_N + ((128, 129) if g is G8 else ())}
        if not raw <= RAN[se.gid(g)]:
            for T in se.window_lengths(g):
                test_raw_windows(g, T, "pcen")
        missing = (want | raw | {"bank " + e for e in se.BANK_EVENTS} | {"bank of 130"}) - RAN[se.gid(g)]
        assert not missing, f"{se.gid(g)}: did not run on the device: {sorted(missing)}"
        assert "c_lo>0" not in RAN[se.gid(g)]                                # (the Python layer never asks for it: the raw windows do)
