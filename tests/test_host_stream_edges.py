"""The cases of tests/test_gpu_stream_edges.py, checked without a GPU (tests/stream_edges_cases.py).

* The geometry table (lead, reach, H, LS, capacity) as streaming._geometry, stream_capacity and leaf_stream_history_samples give it.
* The fp64 twin of the stream equals the whole-clip fp64 oracle within 1e-10 (fp64 rounding of a 401-tap sum with wide margin, five
  orders below anything asserted on the GPU) on every (T, chunking) of the 401 / 160 lattice with T <= 2 LS + 1 and on a sample of the
  rest: `lead`, `reach` and the carry semantics, pinned independently of any kernel.
* Every mutation of the twin leaves the GPU bound (2e-5) at a named case; the carry mutations leave it by more than 1e-2 in the row
  whose smoother is clamped to 0.  What it took: the default bank at F = 6 has sigma <= 11 samples, so a frame emitted one sample early
  or a hop dropped too soon computes the same numbers with it.  The "wide" parameter set (filters as long as the window, the widest
  pooling) and the chunkings that end ON every frame's reach (FOUND) were added to the lattice for these two.
* The coverage list, computed on integers: stream_plan, stream_blocks restated, LeafStreamBank._plan.  c_lo > 0 is shown unreachable
  from the Python layer over every position a stream can stand at; n = 128 and 129 at 201 / 80 ARE reachable (a first chunk of 10361
  samples) and are lattice members; the raw windows cover all three.
* Conditioning: the float32 oracle within 5e-6 of fp64 (the cap of tests/test_host_forward_edges.py) for every parameter set."""
import numpy as np
import pytest
import torch

import leaf_pytorch_amd as L
import stream_edges_cases as se
from conftest import rel_err
from leaf_pytorch_amd.streaming import stream_plan
from oracle import leaf_oracle as lo

TWIN_TOL = 1e-10
GPU_ORACLE_TOL = 2e-5             # tests/test_gpu_stream_edges.py ORACLE_TOL
CARRY_FLOOR = 1e-2
CONDITIONING = 5e-6               # tests/test_host_forward_edges.py
G16, G8 = se.geo(401, 160), se.geo(201, 80)


def test_geometry_table():
    assert tuple(se.geo(401, 160))[:8] == (401, 160, 200, 3, 400, 880, 1600, 16000)
    assert tuple(se.geo(201, 80))[:8] == (201, 80, 100, 3, 200, 440, 1600, 16000)
    for K, hop in se.FUSED + se.TWO_LAUNCH_ONLY:
        g = se.geo(K, hop)
        assert g.H == g.reach + g.lead * g.hop and g.reach == 2 * (K - 1 - g.padL) and g.lead * hop >= 2 * g.padL > (g.lead - 1) * hop
        assert lo.geometry(se.F, g.sr).window_size == K and lo.geometry(se.F, g.sr).hop == hop
        assert se.reduced_lattice(g) == sorted({1, hop, g.reach, g.reach + 1, K, g.LS + 1, 2 * g.LS + 1})
    assert [se.geo(K, hop).LS for K, hop in se.TWO_LAUNCH_ONLY] == [1472, 960, 896]


def test_lattice_holds_every_listed_member():
    for g in (G16, G8):
        K, h, r, H, LS, cap = g.K, g.hop, g.reach, g.H, g.LS, g.cap
        want = {1, 2, h - 1, h, h + 1, g.padL, g.padL + 1, r, r + 1, r + 2, K - 1, K, K + 1, H - 1, H, H + 1, LS - 1, LS, LS + 1, 2 * LS + 1,
                r + 1 + 62 * h, r + 1 + 63 * h, r + 1 + 64 * h, cap - 1, cap, cap + 1, cap + H + 1}
        if g is G8:
            want |= {r + 1 + 126 * h, r + 1 + 127 * h, r + 1 + 128 * h}
        assert set(se.lattice(g)) == want
        # a single chunk of r + 1 + j h samples emits j + 1 frames
        for j in (62, 63, 64) + ((126, 127, 128) if g is G8 else ()):
            assert se.plan_steps(g, [r + 1 + j * h])[0].n == j + 1
        for T in se.lattice(g):
            names = [n for n, _ in se.chunkings(g, T)]
            assert names[0] == "a" and len(set(names)) == len(names)
            assert ("b" in names) == (2 <= T <= K + 1)                        # ([1] is chunking (a) of T = 1)
            assert all(sum(s) == T and min(s) > 0 for _, s in se.chunkings(g, T))
            lists = [s for _, s in se.chunkings(g, T)]                          # (a duplicate keeps its first name: [1, 1] is (b) of T = 2)
            assert all([p, T - p] in lists for p in se.lattice(g) if p < T) and all(se._cut(T, c) in lists for c in (h - 1, h, h + 1))
        assert all(T in se.lattice(g) for T in se.FOUND[(K, h)])
    # the chunk sizes of (e): every member of the size set is drawn somewhere, the fill to the capacity included
    for g in (G16, G8):
        drawn = {s for T in se.lattice(g) for i in range(3) for s in se.random_sizes(g, T, i)}
        assert {1, 2, g.hop - 1, g.hop, g.hop + 1, g.padL, g.reach, g.reach + 1, g.K, g.H, g.LS - 1, g.LS, g.LS + 1} <= drawn
        assert any(s.hist_len + s.Tc == g.cap for T in se.lattice(g) for i in range(3) for s in se.plan_steps(g, se.random_sizes(g, T, i)))


def test_case_count_and_cost():
    for g in (G16, G8):
        cases = se.all_cases(g)
        launches = sum(len(se.plan_steps(g, s)) for _, _, s in cases)
        print(f"{se.gid(g)}: {len(se.lattice(g))} lengths, {len(cases)} (T, chunking) cases, {launches} launches per configuration; "
              f"{sum(len(se.bitwise_subset(g, T)) for T in se.lattice(g))} in the bit-for-bit subset; "
              f"{sum(len(se.windows(g, T)) for T in se.window_lengths(g))} raw windows")
        assert len(cases) < 600 and launches < 10000                          # a configuration of the GPU file: a few seconds
        assert max(T for T, _, _ in cases) == g.cap + g.H + 1
    # the reduced lattice of the two-launch stream: chunkings (a), (c), (d), split at its own members
    for K, hop in ((201, 80),) + se.TWO_LAUNCH_ONLY:
        g = se.geo(K, hop)
        ts = se.reduced_lattice(g)
        for T in ts:
            for name, sizes in se.chunkings(g, T, "acd", ts):
                assert name[0] in "acd" and min(sizes) > 0 and sum(se.counts_per_chunk(g, sizes)) == (T - 1) // hop + 1
            assert [s for n, s in se.chunkings(g, T, "d", ts)] == [[p, T - p] for p in ts if p < T]


# ---- 1. the twin against the whole clip
def _twin_case(g, pset, T, name, sizes, nf=se.F, rows=1):
    x, ref = se.signal(g.K, g.hop, T)[:rows], se.oracle(g, pset, T, nf)[:rows]
    outs, cat = se.Twin(g, se.params(g, pset, nf)).run(x, sizes)
    assert [o.shape[-1] for o in outs] == se.counts_per_chunk(g, sizes), (se.gid(g), T, name)
    assert cat.shape == ref.shape and cat.shape[-1] == (T - 1) // g.hop + 1
    e = rel_err(cat, ref)
    assert e < TWIN_TOL, f"{se.gid(g)} {pset} T={T} {name}: twin {e:.3e} from the whole-clip fp64 oracle"
    return e


@pytest.mark.parametrize("T", [T for T in se.lattice(G16) if T <= 2 * G16.LS + 1])
def test_twin_equals_the_whole_clip_on_the_16k_lattice(T):
    worst = 0.0
    for i, (name, sizes) in enumerate(se.chunkings(G16, T)):
        worst = max(worst, _twin_case(G16, ("away", "wide")[i % 2], T, name, sizes))
    print(f"401-160 T={T}: {len(se.chunkings(G16, T))} chunkings, twin within {worst:.2e} of the whole clip")


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_twin_equals_the_whole_clip_on_a_sample_of_the_rest(g):
    """Beyond 2 LS + 1 at 401 / 160, the 8 kHz lattice, the F = 1 module, three rows: chunkings (a), (c) hop, (e) 0 and (f)."""
    ts = [T for T in se.lattice(g) if T > 2 * g.LS + 1 or g is G8]
    worst, n = 0.0, 0
    for j, T in enumerate(ts):
        for name, sizes in se.chunkings(g, T):
            if name in ("a", "e0") or name[0] == "f" or (name == f"c{g.hop}" and T <= g.reach + 1 + 64 * g.hop):
                worst, n = max(worst, _twin_case(g, se.PSETS[(j + n) % 3], T, name, sizes)), n + 1
    for T, name in ((g.K + 1, "b"), (2 * g.LS + 1, f"c{g.hop + 1}"), (g.H + 1, f"d{g.H}")):
        worst = max(worst, _twin_case(g, "away", T, name, dict(se.chunkings(g, T))[name], nf=1, rows=3))
        worst = max(worst, _twin_case(g, "defaults", T, name, dict(se.chunkings(g, T))[name], rows=3))
    print(f"{se.gid(g)}: {n + 6} sampled cases, twin within {worst:.2e} of the whole clip")


def test_pcen_point_is_the_oracles():
    g = G16
    prm = {k: v.double() for k, v in se.params(g, "away").items()}
    p = se.pooled64(g, "away", g.LS + 1)
    m = lo.ema_scan(p, prm["_compression.ema._weights"])
    want = lo.pcen(p, prm["_compression.alpha"], prm["_compression.delta"], prm["_compression.root"], prm["_compression.ema._weights"])
    assert torch.equal(se.pcen_point(p, m, prm), want)
    assert torch.equal(se.window_oracle(g, "away", g.LS + 1, 0, p.shape[-1], "pcen"), want)
    # row 0 of "away": the smoother holds the recording's first frame for ever
    assert torch.equal(m[:, 0], p[:, 0, :1].expand_as(m[:, 0]))


# ---- 2. mutations: (mutation, parameter set, T as a function of the geometry, chunking name)
MUTATION_CASES = [
    ("reach-1", "wide", lambda g: 2 * g.LS + 1, lambda g: "f-ends-on-every-reach"),
    ("drop+1", "wide", lambda g: 2 * g.LS + 1, lambda g: f"c{g.hop}"),
    ("seam", "away", lambda g: 2 * g.LS + 1, lambda g: f"c{g.hop + 1}"),
    ("carry-step", "away", lambda g: g.H + 1, lambda g: f"d{g.H}"),
    ("carry-group", "away", lambda g: g.reach + 1 + 64 * g.hop, lambda g: "a"),
    ("pad", "away", lambda g: g.reach + 1, lambda g: "a"),
]


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
@pytest.mark.parametrize("mutation,pset,T_of,name_of", MUTATION_CASES, ids=[c[0] for c in MUTATION_CASES])
def test_every_mutation_leaves_the_gpu_bound(g, mutation, pset, T_of, name_of):
    T, name = T_of(g), name_of(g)
    sizes = dict(se.chunkings(g, T))[name]
    x, ref = se.signal(g.K, g.hop, T), se.oracle(g, pset, T)
    _, clean = se.Twin(g, se.params(g, pset)).run(x, sizes)
    _, bad = se.Twin(g, se.params(g, pset), mutation).run(x, sizes)
    assert rel_err(clean, ref) < TWIN_TOL and bad.shape == ref.shape
    per_row = ((bad - ref).abs() / ref.abs()).amax(dim=(0, 2))
    print(f"{se.gid(g)} {mutation} at {pset} T={T} {name}: worst {float(per_row.max()):.2e}, per filter row " + " ".join(f"{float(v):.1e}" for v in per_row))
    assert float(per_row.max()) > GPU_ORACLE_TOL, f"{mutation} stays within the GPU bound at T={T} {name}: {float(per_row.max()):.2e}"
    if mutation.startswith("carry"):
        assert float(se.params(g, pset)["_compression.ema._weights"][0]) == 0.0
        assert float(per_row[0]) > CARRY_FLOOR, f"{mutation}: the w = 0 row moves by {float(per_row[0]):.2e} only"
        # ... and the F = 1 module (that row alone) sees it as well
        _, one = se.Twin(g, se.params(g, pset, 1), mutation).run(x, sizes)
        assert rel_err(one, bad[:, :1]) < TWIN_TOL and rel_err(one, ref[:, :1]) > CARRY_FLOOR


def test_the_unmutated_plan_of_the_twin_is_stream_plan():
    """The twin restates stream_plan where a mutation changes it; without the defect the restatement is stream_plan."""
    g = G8
    tw = se.Twin(g, se.params(g, "away"), "reach-1")
    tw.mutation = "drop+1"
    for hist in range(0, g.H + 1, 7):
        for nxt in range(g.lead + 1):
            for Tc in (0, 1, 79, 80, 81, 200, 201, 441, 1600, 15000):
                for final in (False, True):
                    tw.next = nxt
                    got, want = tw._plan(hist, Tc, final), stream_plan(hist, nxt, Tc, g.K, g.hop, final)
                    assert got == want or (not final and want[1] > 0 and want[2] > 0 and got[:2] == want[:2] and got[2] == want[2] + g.hop)


# ---- 3. coverage, on integers
@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_the_chunkings_reach_every_stream_event(g):
    seen = {}
    for T, name, sizes in se.all_cases(g):
        for e in se.events(g, sizes):
            seen.setdefault(e, (T, name))
    want = se.STREAM_EVENTS + (se.EVENTS_8K if g is G8 else ())
    for e in want:
        assert e in seen, f"{se.gid(g)}: no committed chunking reaches '{e}'"
    print(f"{se.gid(g)}: " + "; ".join(f"{e} at T={seen[e][0]} {seen[e][1]}" for e in want))
    assert "c_lo>0" not in seen
    # the explicit lists do what their names say
    found = {name: se.plan_steps(g, sizes) for T in se.FOUND[(g.K, g.hop)] for name, sizes in se.FOUND[(g.K, g.hop)][T]}
    assert any(s.hist_len == g.H and s.hist_len + s.Tc == g.cap for s in found["f-fill-on-H"])
    for n in (63, 64, 65) + ((127, 128, 129) if g is G8 else ()):
        assert any(s.started and s.n == n for s in found[f"f-started-{n}"]), n
    steps = se.plan_steps(g, dict(se.chunkings(g, 2 * g.LS + 1))["f-ends-on-every-reach"])
    assert all((s.hist_len + s.Tc - g.reach) % g.hop == 0 for s in steps[:-2]) and [s.n for s in steps[:-2]] == [0] + [1] * (len(steps) - 3)
    steps = se.plan_steps(g, dict(se.chunkings(g, 2 * g.LS + 1))["f-completes-one-frame-each"])
    assert all((s.hist_len + s.Tc - 1 - g.reach) % g.hop == 0 and s.n == 1 for s in steps[:-2])


def _plan_arrays(g, hist, nxt, Tc):
    """stream_plan (not final) on numpy arrays of Tc: (n, drop_samples, new_hist_len, new_next)."""
    Lb = hist + Tc
    last = (Lb - 1 - g.reach) // g.hop
    n = np.maximum(0, last - nxt + 1)
    drop = np.where(n > 0, np.maximum(0, last + 1 - g.lead), 0)
    return n, drop * g.hop, Lb - drop * g.hop, np.where(n > 0, last + 1 - drop, nxt)


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_no_position_of_a_stream_reaches_c_lo_above_zero(g):
    """Exhaustive: from EVERY position (hist_len <= H, next <= lead) and EVERY chunk the Python layer can pass (1 .. capacity -
    hist_len samples) a stream lands on such a position again, and its frames start at `next` <= lead; so does the flush.  The first
    block a step's frames meet is then max(0, lead hop - padL) // LS = 0.  (The array form of stream_plan is held to stream_plan on a
    seeded sample.)  The same sweep gives the most frames of one step: 98 at 401 / 160, 198 at 201 / 80."""
    most = 0
    for hist in range(g.H + 1):
        Tc = np.arange(1, g.cap - hist + 1)
        for nxt in range(g.lead + 1):
            n, drop, hist2, nxt2 = _plan_arrays(g, hist, nxt, Tc)
            assert hist2.min() >= 0 and hist2.max() <= g.H and nxt2.min() >= 0 and nxt2.max() <= g.lead
            assert drop.min() >= 0 and (drop <= hist + Tc).all()
            most = max(most, int(n.max()))
    assert max(0, g.lead * g.hop - g.padL) // g.LS == 0
    assert all(se.stream_blocks(g, first, 1, g.cap)[0] == 0 for first in range(g.lead + 1))
    assert most == (g.cap - 1 - g.reach) // g.hop + 1 == {160: 98, 80: 198}[g.hop]
    rng = np.random.default_rng(g.K)
    for _ in range(3000):
        hist, nxt = int(rng.integers(0, g.H + 1)), int(rng.integers(0, g.lead + 1))
        Tc = int(rng.integers(1, g.cap - hist + 1))
        first, n, drop, hist2, nxt2 = stream_plan(hist, nxt, Tc, g.K, g.hop, False)
        got = _plan_arrays(g, hist, nxt, np.array([Tc]))
        assert first == nxt and (n, drop, hist2, nxt2) == tuple(int(v[0]) for v in got)
        assert stream_plan(hist, nxt, 0, g.K, g.hop, True)[0] == nxt


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_the_raw_windows_reach_what_the_python_layer_cannot(g):
    c_los, ns, count = set(), set(), 0
    for T in se.window_lengths(g):
        edges = se.edge_frames(g, T)
        TPv = (T - 1) // g.hop + 1
        assert {0, 1, TPv - 1} <= set(edges)
        for c in range(1, -(-T // g.LS)):                                     # a window starts / ends on either side of every block boundary
            starts = [m * g.hop - g.padL for m in edges]
            ends = [s + g.K - 1 for s in starts]
            assert any(s < c * g.LS for s in starts) and (any(s >= c * g.LS for s in starts) or (TPv - 1) * g.hop - g.padL < c * g.LS), (T, c)
            assert any(e < c * g.LS for e in ends) and (any(e >= c * g.LS for e in ends) or c * g.LS >= T - 1), (T, c)
        for first, n in se.windows(g, T):
            assert n > 0 and se.stream_frames_ok(g, first, n, T)
            c_lo, nb = se.stream_blocks(g, first, n, T)
            assert 0 <= c_lo and 1 <= nb <= 10 and c_lo + nb <= -(-T // g.LS)
            c_los.add(c_lo)
            ns.add(n)
            count += 1
    assert {0, 1, 4, 9} <= c_los and set(se.WINDOW_N) <= ns and ((128 in ns and 129 in ns) == (g is G8))
    print(f"{se.gid(g)}: {count} raw windows, c_lo in {sorted(c_los)}, n in {sorted(ns)}")


@pytest.mark.parametrize("g", [G16, G8], ids=se.gid)
def test_the_bank_scripts_reach_every_bank_event(g):
    script, order = se.bank_script(g)
    bank = L.LeafStreamBank(L.Leaf(n_filters=se.F, sample_rate=g.sr), 3)
    assert bank.max_chunk == g.cap - g.H
    ev = se.bank_events(g, script, bank._plan)
    assert ev == set(se.BANK_EVENTS), sorted(set(se.BANK_EVENTS) - ev)
    assert not any(bank.running) and all(len(row) == 3 for row in script)
    streams = [(T, tuple(sizes)) for slot in order for T, sizes in slot]
    assert len(set(streams)) == len(streams) and all(T in se.lattice(g) or T in se.BANK_FOUND[(g.K, g.hop)] for T, _ in streams)
    big, where = se.wide_bank_script(g)
    wide = L.LeafStreamBank(L.Leaf(n_filters=2, sample_rate=g.sr), 130)
    for row in big:
        wide._plan([r[0] for r in row], [bool(r[1]) for r in row])
    assert len(big[0]) == 130 and sorted(where) == [127, 128, 129] and not any(wide.running)
    print(f"{se.gid(g)}: bank script of {len(script)} steps, {len(streams)} streams; 130-slot script of {len(big)} steps")


# ---- 4. conditioning
@pytest.mark.parametrize("K,hop", se.FUSED + se.TWO_LAUNCH_ONLY, ids=lambda v: str(v))
def test_cases_are_well_conditioned(K, hop):
    g = se.geo(K, hop)
    ts = (1, 2, g.K, 2 * g.LS + 1) + ((g.reach + 1 + 64 * g.hop, g.cap + g.H + 1) if (K, hop) in se.FUSED else ())
    worst, low = (0.0, None), 1e9
    for pset in se.PSETS:
        for T in ts:
            x = se.signal(K, hop, T)
            ref = se.oracle(g, pset, T)
            e = rel_err(lo.leaf_forward(x, se.params(g, pset), se.lgeo(g), True, torch.float32), ref)
            e16 = rel_err(lo.leaf_forward(se.pcm16(x).float() / 32768, se.params(g, pset), se.lgeo(g), True, torch.float32),
                          lo.leaf_forward(se.pcm16(x).double() / 32768, {k: v.double() for k, v in se.params(g, pset).items()}, se.lgeo(g), True, torch.float64))
            worst, low = max(worst, (e, (pset, T)), (e16, (pset, T, "int16"))), min(low, float(ref.min()))
            assert max(e, e16) < CONDITIONING, f"{K}/{hop} {pset} T={T}: float32 oracle {max(e, e16):.3e} from fp64 (cap {CONDITIONING:.0e})"
    print(f"{K}/{hop}: float32 oracle within {worst[0]:.2e} of fp64 (at {worst[1]}), smallest output {low:.3f}")
    assert low > 0.05
