"""Resampling on the device: leaf_resample_f32 through ``resample``, ``PackedClips.resampled`` and ``_native.resample_records`` against
the NumPy float64 oracle of tests/test_host_resample.py, inside the derived bound of a float32 fma chain per output; the int16
quantiser, bit for bit; the invariance of a recording's bits under everything that is not the recording; the bits of the CPU build
of the same header (tools/resample_check.cpp); containment of a NaN; the memory contract on guarded buffers; and the way on into
``ClipSampler`` and ``Leaf.forward``.

Every tested recording sits between a recording of constant +full scale and one of constant -full scale: a read across a seam shows
as an error of order 1.  The whole output store is compared, so a write into a neighbour shows too."""
import numpy as np
import pytest
import torch

import leaf_pytorch_amd
from guarded import guarded, guarded_tensor, unchanged
from leaf_pytorch_amd import ClipSampler, Leaf, PackedClips, _native
from test_host_resample import as_float64, plan_ref, quantize_ref, run_tool, samples, tool   # noqa: F401  (tool: the compiled program)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = _native.RESAMPLE_TILE
RATIOS = [(3, 2), (2, 3), (3, 1), (1, 2), (2, 1), (5, 5), (44100, 16000), (44100, 48000)]
DTYPES = [torch.int16, torch.float32]
WIDE = [(16, 1), (44100, 2000)]                 # the window of a tile is beyond the LDS budget: samples and taps from global memory
GUARD_LEN = 40


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    _native.load()


def bits(t: torch.Tensor) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def full_scale(dtype, sign: int, L: int = GUARD_LEN) -> np.ndarray:
    if dtype == torch.int16:
        return np.full(L, 32767 if sign > 0 else -32768, dtype=np.int16)
    return np.full(L, float(sign), dtype=np.float32)


def length_for(ref, target: int) -> int:
    """The first recording length whose output has at least ``target`` samples (exactly, where the ratio can hit it)."""
    L = 0
    while ref.length(L) < target:
        L += 1
    return L


def lengths_under_test(ref) -> list:
    o, w = ref.o, ref.width
    edge = [0, 1, 2, w, w + 1, o - 1, o, o + 1, 2 * o + w + 3]
    tiles = [length_for(ref, t) for t in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]
    return sorted(set(edge)) + tiles


def fenced(recordings, dtype) -> list:
    """+full scale, r, -full scale for every r."""
    out = []
    for r in recordings:
        out += [full_scale(dtype, +1), r, full_scale(dtype, -1)]
    return out


def oracle_store(ref, recordings):
    """The oracle's output store and bounds for recordings packed back to back, and the integer plan (lengths, offsets)."""
    ys, bs = zip(*(ref.resample(as_float64(r)) for r in recordings))
    lengths = np.array([y.size for y in ys], dtype=np.int64)
    return np.concatenate(ys), np.concatenate(bs), lengths, np.cumsum(lengths) - lengths


def packed(recordings) -> PackedClips:
    return PackedClips([torch.from_numpy(r) for r in recordings], device=DEV)


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig,new", RATIOS, ids=[f"{a}to{b}" for a, b in RATIOS])
@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
def test_store_against_the_oracle(orig, new, dtype):
    ref = plan_ref(orig, new)
    recs = fenced([samples(dtype, L, 7 * L + 1) for L in lengths_under_test(ref)], dtype)
    clips = packed(recs)
    want, bound, lengths, offsets = oracle_store(ref, recs)
    got = clips.resampled(orig, new, out_dtype=torch.float32)
    assert got.lengths_host.tolist() == lengths.tolist() and got.offsets_host.tolist() == offsets.tolist()      # the integer plan
    assert got.lengths_host.tolist() == [_native.resample_length(r.size, orig, new) for r in recs]
    assert got.store.dtype == torch.float32 and got.store.device == clips.store.device and got.store.numel() == want.size
    err = np.abs(got.store.cpu().numpy().astype(np.float64) - want)
    worst = float((err / bound).max())
    print(f"{orig}->{new} {dtype}: worst error {worst:.3f} of the bound over {want.size} outputs")
    assert np.all(err <= bound), worst
    same = clips.resampled(orig, new)                                           # the source dtype is kept
    assert same.store.dtype == dtype
    if dtype == torch.int16:
        assert np.array_equal(same.store.cpu().numpy(), quantize_ref(got.store.cpu().numpy()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
def test_taps_from_global_memory(dtype):
    """4096 -> 4099: a 213 KB table.  The plan says the taps stay in global memory; one recording of 8197 samples covers every phase."""
    tab = _native.resample_table(4096, 4099)
    assert not tab.taps_in_lds and tab.window_in_lds
    ref = plan_ref(4096, 4099)
    recs = fenced([samples(dtype, 8197, 3)], dtype)
    want, bound, lengths, _ = oracle_store(ref, recs)
    got = packed(recs).resampled(4096, 4099, out_dtype=torch.float32)
    assert got.lengths_host.tolist() == lengths.tolist()
    err = np.abs(got.store.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("orig,new", WIDE, ids=[f"{a}to{b}" for a, b in WIDE])
@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
def test_window_from_global_memory(tool, orig, new, dtype):
    """16 -> 1 and 441 -> 20: a tile's window is beyond the LDS budget, so samples and taps are read from global memory, every index
    checked against the recording.  The plan says so; fenced recordings against the oracle, both output dtypes, and the CPU build's bits."""
    tab = _native.resample_table(orig, new)
    assert not tab.window_in_lds and not tab.taps_in_lds
    ref = plan_ref(orig, new)
    o, w = ref.o, ref.width
    lens = sorted({0, 1, 2, w, w + 1, o - 1, o, o + 1, 2 * o + w + 3}) + [length_for(ref, TILE + 1)]
    inner = [samples(dtype, L, 5 * L + 2) for L in lens]
    recs = fenced(inner, dtype)
    clips = packed(recs)
    want, bound, lengths, offsets = oracle_store(ref, recs)
    got = clips.resampled(orig, new, out_dtype=torch.float32)
    assert got.lengths_host.tolist() == lengths.tolist() and got.offsets_host.tolist() == offsets.tolist()
    y = got.store.cpu().numpy()
    err = np.abs(y.astype(np.float64) - want)
    worst = float((err / bound).max())
    print(f"{orig}->{new} {dtype}: worst error {worst:.3f} of the bound over {want.size} outputs")
    assert np.all(err <= bound), worst
    q = clips.resampled(orig, new, out_dtype=torch.int16).store.cpu().numpy()
    assert np.array_equal(q, quantize_ref(y))
    for i in (lens.index(w + 1), lens.index(2 * o + w + 3)):                    # recording 3 i + 1 of the fenced store
        _, ty, tq = run_tool(tool, orig, new, inner[i], pcm=dtype == torch.int16)
        off, n = int(offsets[3 * i + 1]), int(lengths[3 * i + 1])
        assert np.array_equal(y[off: off + n].view(np.uint32), ty.view(np.uint32)) and np.array_equal(q[off: off + n], tq), i


def test_batch_shapes_and_identity():
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-32768, 32768, (2, 3, 501), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    y = leaf_pytorch_amd.resample(x, 44100, 16000)
    ref = plan_ref(44100, 16000)
    assert y.shape == (2, 3, ref.length(501)) and y.dtype == torch.int16
    row = leaf_pytorch_amd.resample(x[1, 2], 44100, 16000)                       # a row alone: the same bits
    assert torch.equal(row, y[1, 2])
    yt = leaf_pytorch_amd.resample(x.transpose(0, 1), 44100, 16000)              # a non-contiguous batch is copied
    assert torch.equal(yt, y.transpose(0, 1))
    assert leaf_pytorch_amd.resample(x[..., :0], 3, 2).shape == (2, 3, 0)
    # o == n: the identity, and with out_dtype the conversions
    assert torch.equal(leaf_pytorch_amd.resample(x, 5, 5), x)
    f = leaf_pytorch_amd.resample(x, 16000, 16000, out_dtype=torch.float32)
    assert f.dtype == torch.float32 and np.array_equal(bits(f), bits(x.float() / 32768.0))
    v = (torch.rand(4, 777, generator=g) * 2.4 - 1.2).to(DEV)                   # beyond full scale: the quantiser saturates
    assert np.array_equal(bits(leaf_pytorch_amd.resample(v, 7, 7)), bits(v))
    q = leaf_pytorch_amd.resample(v, 7, 7, out_dtype=torch.int16)
    assert np.array_equal(q.cpu().numpy(), quantize_ref(v.cpu().numpy())) and int(q.max()) == 32767 and int(q.min()) == -32768


# ---- output modes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig,new", [(44100, 16000), (2, 3), (2, 1)])
def test_int16_output_is_the_quantised_float32_output(orig, new):
    """... for both input dtypes, at an odd output offset (element stores in front of the first 16-byte chunk) and an even one."""
    for dtype in DTYPES:
        recs = [samples(dtype, L, L) for L in (1, 333, 2900, 17)]
        clips = packed(recs)
        y = clips.resampled(orig, new, out_dtype=torch.float32).store.cpu().numpy()
        q = clips.resampled(orig, new, out_dtype=torch.int16).store.cpu().numpy()
        assert q.dtype == np.int16 and np.array_equal(q, quantize_ref(y))
    # a full-scale square wave overshoots: both rails are reached, nothing wraps
    sq = np.where((np.arange(3000) // 25) % 2 == 0, 32767, -32768).astype(np.int16)
    clips = packed([sq])
    y = clips.resampled(orig, new, out_dtype=torch.float32).store.cpu().numpy()
    q = clips.resampled(orig, new).store.cpu().numpy()
    assert np.array_equal(q, quantize_ref(y))
    assert (q == 32767).any() and (q == -32768).any() and y.max() > 1.0 and y.min() < -1.0
    assert np.all(q[y >= 1.0] == 32767) and np.all(q[y <= -1.0] == -32768) and np.all(np.sign(q[np.abs(y) > 0.5]) == np.sign(y[np.abs(y) > 0.5]))


# ---- invariance ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig,new", [(3, 2), (44100, 16000), (2, 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
def test_bits_depend_on_the_recording_alone(orig, new, dtype):
    ref = plan_ref(orig, new)
    r = samples(dtype, length_for(ref, TILE + 300), 21)                         # two tiles
    n_out = ref.length(r.size)
    alone = leaf_pytorch_amd.resample(torch.from_numpy(r).to(DEV)[None], orig, new, out_dtype=torch.float32)[0]
    want = bits(alone)
    others = [samples(dtype, L, 50 + L) for L in (1, 2, 77, 1500, 3, 640, 5, 64)]

    def of(recs, i):
        got = packed(recs).resampled(orig, new, out_dtype=torch.float32)
        off = int(got.offsets_host[i])
        assert int(got.lengths_host[i]) == n_out
        return bits(got.store[off: off + n_out])

    assert np.array_equal(of([r], 0), want)                                     # R = 1
    assert np.array_equal(of([others[0], r], 1), want)                          # an odd store offset (and an odd output offset where o | n allows)
    assert np.array_equal(of([others[1], r], 1), want)                          # an even one
    for place in (0, 4, 8):                                                     # first, in the middle and last of R = 9
        recs = list(others)
        recs.insert(place, r)
        assert np.array_equal(of(recs, place), want), place
    # the taps from global memory instead of LDS: the table's own word, cleared
    tab = _native.resample_table(orig, new)
    assert tab.taps_in_lds and not tab.with_global_taps().taps_in_lds
    clips = packed([others[0], r, others[2]])
    lengths = torch.tensor([ref.length(int(L)) for L in clips.lengths_host], dtype=torch.int64)
    offsets = torch.cumsum(lengths, 0) - lengths
    for table in (tab, tab.with_global_taps()):
        out = torch.full((int(lengths.sum()),), float("nan"), device=DEV)
        _native.resample_records(clips.store, clips.offsets, clips.lengths, orig, new, out, offsets.to(DEV), table=table)
        assert np.array_equal(bits(out[int(offsets[1]): int(offsets[1]) + n_out]), want), table.taps_in_lds


# ---- the CPU function's bits -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig,new", [(3, 2), (44100, 16000), (44100, 48000)])
def test_kernel_has_the_bits_of_the_cpu_build(tool, orig, new):
    ref = plan_ref(orig, new)
    for dtype in DTYPES:
        recs = [samples(dtype, L, 31 * L) for L in (ref.width + 1, 2 * ref.o + ref.width + 3, length_for(ref, TILE + 1))]
        got = packed(recs)
        for out_dtype in (torch.float32, torch.int16):
            res = got.resampled(orig, new, out_dtype=out_dtype)
            for i, r in enumerate(recs):
                _, y, q = run_tool(tool, orig, new, r, pcm=dtype == torch.int16)
                off, n = int(res.offsets_host[i]), int(res.lengths_host[i])
                mine = res.store[off: off + n]
                if out_dtype == torch.float32:
                    assert np.array_equal(bits(mine), y.view(np.uint32)), (dtype, i)
                else:
                    assert np.array_equal(mine.cpu().numpy(), q), (dtype, i)


# ---- NaN containment -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("orig,new", [(3, 2), (44100, 16000), (1, 2)])
def test_a_nan_stays_within_the_filter_width(orig, new):
    ref = plan_ref(orig, new)
    r = samples(torch.float32, 3001, 9)
    s = 1500
    bad = r.copy()
    bad[s] = np.nan
    clean, dirty = (leaf_pytorch_amd.resample(torch.from_numpy(v).to(DEV), orig, new).cpu().numpy() for v in (r, bad))
    j = np.arange(clean.size)
    far = np.abs(j * ref.o / ref.n - s) > ref.width + 1
    assert far.sum() > clean.size - 2 * (ref.width + 2) * ref.n / ref.o - 4 and np.isnan(dirty).any()
    assert np.array_equal(clean.view(np.uint32)[far], dirty.view(np.uint32)[far])
    assert not np.isnan(dirty[far]).any()


# ---- the memory contract ---------------------------------------------------------------------------------------------------------------

def clamped_plan(store_len, out_total, in_off, in_len, out_off, ref):
    """The header's MEMORY SAFETY rule in Python integers."""
    plan = []
    for off, L, ooff in zip(in_off, in_len, out_off):
        off = min(max(off, 0), store_len)
        L = min(max(L, 0), store_len - off)
        ooff = min(max(ooff, 0), out_total)
        plan.append((off, L, ooff, min(ref.length(L), out_total - ooff)))
    return plan


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.int16], ids=["out_float32", "out_int16"])
@pytest.mark.parametrize("orig,new", [(44100, 16000)] + WIDE, ids=["window_in_lds", "16to1", "441to20"])
def test_memory_contract_on_guarded_buffers(orig, new, dtype, out_dtype):
    """store, out and the workspace are payloads of exact size between guard patterns; the plan overruns the store by a few samples,
    starts before it, and names an out_off past out_total and one whose output does not fit.  Nothing outside is touched (the guards
    of out and the workspace), nothing outside the store enters a result (the outputs are the oracle's on the clamped plan), and what
    no clamped record covers keeps its fill."""
    ref = plan_ref(orig, new)
    assert _native.resample_table(orig, new).window_in_lds == ((orig, new) not in WIDE)
    store_np = samples(dtype, 4000, 77)
    n0, n1, n2, n4 = (ref.length(L) for L in (900, 700, 1200, 1500))
    store_len, out_total = store_np.size, n0 + 3 + n1 + 5 + n2 + 11 + n4 // 2
    #           ends 5 past the store   starts before it   fits            out_off past out_total   output cut by out_total   out_off negative
    in_off = [store_len - 900,           -3,                1000,           500,                     2000,                     3990]
    in_len = [905,                       700,               1200,           300,                     1500,                     40]
    out_off = [0,                        n0 + 3,            n0 + n1 + 8,    out_total + 7,           out_total - n4 // 2,      -2]
    plan = clamped_plan(store_len, out_total, in_off, in_len, out_off, ref)
    assert plan[0][1] == 900 and plan[1][:2] == (0, 700) and plan[3][3] == 0 and 0 < plan[4][3] == n4 // 2 < n4 and plan[5][1] == 10
    R = len(in_off)
    item = 2 if out_dtype == torch.int16 else 4
    g_store = guarded_tensor(torch.from_numpy(store_np))
    g_out = guarded(out_total * item, 0x5A, offset=item)                        # (element alignment only: one element past a 4096-byte boundary)
    g_ws = guarded(_native.load().leaf_resample_workspace_bytes(R), 0xFF)
    dev_plan = [torch.tensor(v, dtype=dt, device=DEV) for v, dt in ((in_off, torch.int64), (in_len, torch.int32), (out_off, torch.int64))]
    out = g_out.view(out_dtype)
    assert out.data_ptr() == g_out.address and out.numel() == out_total
    _native.resample_records(g_store.view(dtype), dev_plan[0], dev_plan[1], orig, new, out, dev_plan[2], ws=g_ws.bytes())
    torch.cuda.synchronize()
    unchanged(g_store, "store")
    g_out.check("out")
    g_ws.check("workspace")
    got = out.cpu().numpy()
    fill = np.frombuffer(bytes([0x5A] * item), dtype=got.dtype)[0]
    x = as_float64(store_np)
    for i, (off, L, ooff, n) in enumerate(plan):
        later = np.zeros(out_total, dtype=bool)
        for (_, _, o2, n2) in plan[:i] + plan[i + 1:]:
            later[o2: o2 + n2] = True
        mine = np.zeros(out_total, dtype=bool)
        mine[ooff: ooff + n] = True
        only = mine & ~later                                                    # the outputs no other record writes
        want, bound = ref.resample(x[off: off + L])
        sel = only[ooff: ooff + n]
        have = got[ooff: ooff + n][sel]
        if out_dtype == torch.float32:
            assert np.all(np.abs(have.astype(np.float64) - want[:n][sel]) <= bound[:n][sel]), i
        else:                                                                   # one quantisation step around the oracle's value
            assert np.all(np.abs(have.astype(np.float64) - np.clip(want[:n][sel] * 32768, -32768, 32767)) <= 0.5 + 32768 * bound[:n][sel] + 1e-9), i
    written = np.zeros(out_total, dtype=bool)
    for (_, _, ooff, n) in plan:
        written[ooff: ooff + n] = True
    assert np.all(got[~written] == fill) and (~written).any()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

def test_resampled_store_feeds_the_sampler_and_the_frontend():
    lengths = (44100, 30000, 61111, 9)
    recs = [samples(torch.int16, L, L) for L in lengths]
    clips = packed(recs)
    clips16 = clips.resampled(44100, 16000)
    assert clips16.store.dtype == torch.int16 and clips16.lengths_host.tolist() == [_native.resample_length(L, 44100, 16000) for L in lengths]
    one_by_one = PackedClips([leaf_pytorch_amd.resample(torch.from_numpy(r).to(DEV), 44100, 16000) for r in recs], device=DEV)
    assert torch.equal(one_by_one.store, clips16.store) and one_by_one.lengths_host.tolist() == clips16.lengths_host.tolist()
    index = torch.tensor([0, 1, 2, 3, 2, 0])
    a = ClipSampler(clips16, 16000, generator=torch.Generator().manual_seed(4), num_masks=2, time_perc=0.1)(index)
    b = ClipSampler(one_by_one, 16000, generator=torch.Generator().manual_seed(4), num_masks=2, time_perc=0.1)(index)
    assert a.shape == (6, 1, 16000) and a.dtype == torch.float32 and np.array_equal(bits(a), bits(b))
    torch.manual_seed(0)
    leaf = Leaf().to(DEV).eval()
    with torch.no_grad():
        feats = leaf(a)
    assert feats.shape[0] == 6 and bool(torch.isfinite(feats).all())
    assert clips16._peaks is None and clips16._moments is None                  # nothing is carried over from the source store
