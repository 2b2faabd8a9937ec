"""Whole-recording evaluation batches on the device: leaf_clip_peaks_f32 and leaf_assemble_segments_f32 (csrc/leaf_clips.hpp;
PackedClips.peaks / segments, segment_mean and evaluate_recordings on top).

The oracle is ``segments_ref`` (tests/test_host_segments.py: the reference's test.py in stock ops on the CPU -- F.pad 'replicate',
reshape) with the whole-recording normalisation done by the existing transforms.PeakNormalization on the device, which is not
code under test.  Rows and peaks are compared bit for bit: a row is a copy, or one correctly rounded fp32 multiply, and a maximum
does not depend on the order it is taken in.  The stores are packed as in tests/test_gpu_clips.py, full-scale samples (+-1e3 /
+-32767) between the recordings, so that a read across a recording's edge changes a peak or a padded value."""
import functools

import pytest
import torch
import torch.nn.functional as F

from leaf_pytorch_amd import Leaf, PackedClips, PeakNormalization, _native, evaluate_recordings, segment_mean
from guarded import guarded, guarded_tensor, unchanged
from test_gpu_clips import pack, same_bits
from test_host_segments import clamp_segment_plan, mean_bound, rows_ref, segments_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 1024                                            # csrc/leaf_clips.hpp (kPeakTile): samples one wave reduces at a time
BOTH = pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
REL_TOL = 2e-5                                         # tests/test_gpu_parity.py: the float path's bound against the oracle


def peaknorm(y):
    return PeakNormalization()(y.to(DEV)).cpu()


def clips(store, off, ln):
    return PackedClips.from_store(store.to(DEV), off, ln)


def assert_same_bits(got, want, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not same_bits(got, want):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} samples differ, first at row {int(bad[0, 0])} sample {int(bad[0, 1])}: "
                             f"{float(got[tuple(bad[0])])!r} for {float(want[tuple(bad[0])])!r}")


def true_peaks(store, off, ln):
    x = store.float() / 32768 if store.dtype == torch.int16 else store
    return torch.stack([x[int(o):int(o) + int(n)].abs().max() if n else torch.tensor(0.0) for o, n in zip(off, ln)])


# ---- the peaks ---------------------------------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("loud_at", ["last", "first"])
def test_peaks_are_exact_for_long_and_short_recordings(dtype, loud_at):
    g = torch.Generator().manual_seed(1)
    lengths = [1, 2, 63, 1000, TILE, 3 * TILE + 5] + torch.randint(1, 41, (200,), generator=g).tolist()
    store, off, ln = pack(lengths, dtype, seed=3)
    at = int(off[5]) + (3 * TILE + 4 if loud_at == "last" else 0)
    store[at] = -32768 if dtype == torch.int16 else -3.5                                   # the long recording's only sample above 0.4 (int16: 0.28)
    pc = clips(store, off, ln)
    got = pc.peaks()
    assert got.shape == (206,) and got.dtype == torch.float32 and got.device.type == "cuda"
    want = true_peaks(store, off, ln)
    assert same_bits(got.cpu(), want), (got.cpu() != want).nonzero().reshape(-1)[:8]
    assert float(want[5]) == (1.0 if dtype == torch.int16 else 3.5) and float(want.max()) == float(want[5])
    assert float(want[:5].max()) < 0.5 and (dtype == torch.float32 or float(got.max()) <= 1.0)
    assert pc.peaks() is got                                                               # kept
    store_dev = pc.store
    store_dev[int(off[0])] = 0.75 * (32768 if dtype == torch.int16 else 1)                 # ... so a write into the store goes unseen
    assert pc.peaks() is got
    pc.refresh_peaks()                                                                     # ... until the caller says so
    assert float(pc.peaks()[0]) == 0.75 and same_bits(pc.peaks()[1:].cpu(), want[1:])


def test_peaks_of_a_plan_with_overlaps_empty_recordings_and_nans():
    g = torch.Generator().manual_seed(2)
    N = 5 * TILE + 17
    store = (torch.rand(N, generator=g) * 2 - 1) * 0.9
    store[4000] = float("nan")
    store[N - 1] = 7.0
    # 40 times the whole store (more tiles than the launch is sized for: its waves walk several), empty recordings among them,
    # windows that end one sample before the loud one, a recording that is one NaN
    off = [0, 0, 5] * 40 + [N, 4000, N - 1, 0]
    ln = [N, 0, N - 6] * 40 + [0, 1, 1, 0]
    got = _native.clip_peaks(store.to(DEV), off, ln).cpu()
    quiet = store.clone()
    quiet[4000] = 0.0                                                                      # a NaN sample is ignored
    want = true_peaks(quiet, off, ln)
    assert same_bits(got, want) and got[0] == 7.0 and got[1] == 0.0 and got[2] < 1.0 and got[-3] == 0.0 and got[-2] == 7.0


# ---- the row rule ------------------------------------------------------------------------------------------------------------------

def small_lengths(S):
    return sorted({n for n in (1, 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 2, 7 * S + 3) if n >= 1})


def loud_store(lengths, dtype, seed, size, **kw):
    """pack() at amplitude 0.4, every other float32 recording with ONE sample of 2.5 -- its last, so in its last row: rows before it
    have a peak of 0.4 and a per-row normalisation would leave them alone."""
    store, off, ln = pack(lengths, dtype, seed=seed, **kw)
    if dtype == torch.float32:
        for i in range(0, len(lengths), 2):
            store[int(off[i]) + int(ln[i]) - 1] = 2.5 if i % 4 else -2.5
    return store, off, ln


@BOTH
@pytest.mark.parametrize("size", [4, 5, 13, 16])
def test_rows_follow_the_reference_at_small_shapes(size, dtype):
    lengths = [n for n in small_lengths(size) for _ in (0, 1)]                              # every length loud once and quiet once
    store, off, ln = loud_store(lengths, dtype, size, size)
    pc = clips(store, off, ln)
    index = list(range(len(lengths)))
    want, counts = segments_ref(store, off, ln, index, size, peaknorm)
    got, got_counts = pc.segments(index, size)
    assert got.shape == (int(counts.sum()), 1, size) and got.dtype == torch.float32 and got.is_contiguous()
    assert got_counts.dtype == torch.int64 and got_counts.device.type == "cpu" and torch.equal(got_counts, counts)
    assert counts.tolist() == [-(-n // size) for n in lengths]
    assert_same_bits(got.cpu()[:, 0], want, f"S={size}")
    raw, _ = segments_ref(store, off, ln, index, size)
    if dtype == torch.float32:
        assert float(want.abs().max()) == pytest.approx(1.0, abs=1e-6) and float(raw.abs().max()) == 2.5
        assert not same_bits(peaknorm(raw), want)                                          # a per-row peak gives other bits: the oracle tells them apart
    else:
        assert same_bits(raw, want)
    plain, _ = pc.segments(index, size, normalize=False)
    assert_same_bits(plain.cpu()[:, 0], raw, f"S={size}, normalize=False")
    back = index[::-1] + [3, 3, 0]                                                         # reverse order, repeats
    want_back, counts_back = segments_ref(store, off, ln, back, size, peaknorm)
    out = torch.full((int(counts_back.sum()), 1, size), 7.0, device=DEV)
    res, c = pc.segments(torch.tensor(back), size, out=out)
    assert res is out and torch.equal(c, counts_back)
    assert_same_bits(out.cpu()[:, 0], want_back, f"S={size}, reversed")
    with pytest.raises(RuntimeError):
        pc.segments(index, size, out=torch.empty((int(counts.sum()), size), device=DEV))
    empty, none = pc.segments([], size)
    assert empty.shape == (0, 1, size) and empty.device.type == "cuda" and none.numel() == 0


@BOTH
def test_one_second_rows_of_recordings_up_to_ten_seconds(dtype):
    lengths = [16000, 164800, 23456, 15999, 16001, 48007, 100000, 31999]                    # 1 s .. 10.3 s at 16 kHz
    store, off, ln = loud_store(lengths, dtype, 11, 16000)
    want, counts = segments_ref(store, off, ln, range(8), 16000, peaknorm)
    got, c = clips(store, off, ln).segments(list(range(8)), 16000)
    assert c.tolist() == [1, 11, 2, 1, 2, 4, 7, 2] == counts.tolist()
    assert_same_bits(got.cpu()[:, 0], want, "16 kHz")


def test_rows_longer_than_a_tile_are_split_over_workgroups():
    store, off, ln = loud_store([100001, 7], torch.float32, 12, 40000)
    want, counts = segments_ref(store, off, ln, [0, 1, 0], 40000, peaknorm)
    got, c = clips(store, off, ln).segments([0, 1, 0], 40000)
    assert c.tolist() == [3, 1, 3] and 40000 > 8 * 4 * 1024                                # three rows of two tiles each
    assert_same_bits(got.cpu()[:, 0], want, "S=40000")


@BOTH
@pytest.mark.parametrize("size", [1000, 1001, 1002, 1003])
def test_every_source_and_row_alignment(size, dtype):
    lengths = [1500, 1501, 1502, 1503, 1504, 900, 901, 902]
    store, off, ln = loud_store(lengths, dtype, size, size, gaps=[4, 1, 1, 1, 1, 3, 2, 5])
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
    want, _ = segments_ref(store, off, ln, range(8), size, peaknorm)
    whole = torch.cat([store[:1], store]).to(DEV)
    pc = PackedClips.from_store(whole[1:], off, ln)                                        # the store one element past the allocation's alignment
    assert pc.store.data_ptr() % 16 == store.element_size()
    got, _ = pc.segments(list(range(8)), size)                                             # rows at 4 S b bytes: every shift for odd S
    assert_same_bits(got.cpu()[:, 0], want, f"S={size}")


def test_an_int16_store_gives_the_bits_of_its_float32_image_and_launches_no_peaks():
    store, off, ln = pack([1, 999, 1000, 1001, 3007, 40], torch.int16, seed=5, amp=32767)
    store[int(off[4]) + 3000] = -32768                                                     # |v / 32768| = 1: the largest there is
    pc = clips(store, off, ln)
    image = clips(store.float() / 32768, off, ln)
    index = [5, 4, 3, 2, 1, 0, 4]
    a, ca = pc.segments(index, 1000)
    b, cb = image.segments(index, 1000)
    assert torch.equal(ca, cb) and same_bits(a.cpu(), b.cpu()) and float(a.abs().max()) == 1.0
    assert pc._peaks is None and image._peaks is not None                                  # int16: nothing to scale by, nothing launched
    assert float(pc.peaks().max()) == 1.0 and same_bits(pc.peaks().cpu(), image.peaks().cpu())


# ---- a plan the library cannot see: clamped, and nothing outside the buffers is touched ---------------------------------------------
# (the same hostile values go through the row-view functions on the CPU under -fsanitize=undefined: tools/segment_view_check.cpp)

@BOTH
@pytest.mark.parametrize("size", [13, 1000, 40000])
def test_a_hostile_row_plan_on_the_device_is_clamped(size, dtype):
    lib = _native.load()
    lengths = [size + 9, 40, 2 * size, 7, size - 1, 300, 1, size]
    store, off, ln = pack(lengths, dtype, seed=4)
    N, rows, R = store.numel(), 14, 6
    item = store.element_size()
    big = 2 ** 31 - 1
    rec_off = torch.tensor([-5, N + 100, int(off[2]), N, 2 ** 40, int(off[1]), int(off[4]), N - 3, -2 ** 62, int(off[3]), int(off[0]), int(off[5]),
                            int(off[2]), int(off[7])])
    rec_len = torch.tensor([size + 3, 50, big, 10, 5, -3, size - 1, big, 20, 7, size + 9, 300, 2 * size, size], dtype=torch.int64)
    win = torch.tensor([-7, 0, 2 ** 62, 3, 0, 0, -2 ** 62, -big, 2 ** 63 - 1, -2 ** 63, size, -size - 1, size - 3, 2 ** 31])
    rec = torch.tensor([-1, R, big, 0, 1, 2, 3, 4, 5, -2 ** 31, 2, 1, 0, 5], dtype=torch.int64)
    peaks = torch.tensor([2.5, 0.5, 1.0, 1e3, 1.0000001, 4.0])
    c_off, c_len, c_win, c_rec = clamp_segment_plan(N, rec_off, rec_len, win, rec, size, R)
    assert int(c_len.min()) == 0 and int(c_len.max()) > size and int(c_win.min()) == -size and int((c_win == c_len).sum()) >= 2
    scale = [torch.tensor(1.0) / peaks[i] if float(peaks[i]) > 1 else None for i in c_rec.tolist()]
    want = rows_ref(store, c_off, c_len, c_win, size, scale)

    store_g = guarded_tensor(store.to(DEV), offset=item)                                   # element alignment only: 2 / 4 bytes past a page
    plan_g = [guarded_tensor(t.to(DEV)) for t in (rec_off, rec_len.to(torch.int32), win, peaks, rec.to(torch.int32))]
    out_g = guarded(4 * rows * size, 0xA5, offset=4)
    rc = lib.leaf_assemble_segments_f32(store_g.ptr, N, _native.FLAG_X_PCM16 if dtype == torch.int16 else 0, rows, size,
                                        *(g.ptr for g in plan_g), R, out_g.ptr, _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    out_g.check(f"out, S={size}")
    unchanged(store_g, "store")
    for g in plan_g:
        unchanged(g, "plan")
    got = out_g.cpu(torch.float32, (rows, size))
    assert not bool((got.view(torch.int32) == torch.tensor(0xA5A5A5A5 - 2 ** 32, dtype=torch.int64).to(torch.int32)).any())   # fully written
    assert_same_bits(got, want, f"hostile, S={size}")


@BOTH
def test_a_hostile_recording_list_on_the_device_is_clamped(dtype):
    lib = _native.load()
    store, off, ln = pack([3 * TILE + 9, 40, TILE, 7], dtype, seed=6)
    N, R = store.numel(), 10
    big = 2 ** 31 - 1
    rec_off = torch.tensor([-5, N + 100, int(off[0]), N, 2 ** 40, int(off[1]), N - 3, -2 ** 62, int(off[2]), int(off[3])])
    rec_len = torch.tensor([TILE + 3, 50, big, 10, 5, -3, big, 20, TILE, -2 ** 31], dtype=torch.int64)
    c_off, c_len, _, _ = clamp_segment_plan(N, rec_off, rec_len, torch.zeros(R, dtype=torch.int64), torch.zeros(R, dtype=torch.int64), 1, 1)
    want = true_peaks(store, c_off.tolist(), c_len.tolist())
    store_g = guarded_tensor(store.to(DEV), offset=store.element_size())
    plan_g = [guarded_tensor(rec_off.to(DEV)), guarded_tensor(rec_len.to(torch.int32).to(DEV))]
    peaks_g = guarded(4 * R, 0xA5, offset=4)
    ws_g = guarded(8 * (R + 1), 0xA5, offset=16)
    rc = lib.leaf_clip_peaks_f32(store_g.ptr, N, _native.FLAG_X_PCM16 if dtype == torch.int16 else 0, R, plan_g[0].ptr, plan_g[1].ptr,
                                 peaks_g.ptr, ws_g.ptr, 8 * (R + 1), _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    peaks_g.check("peaks")
    ws_g.check("workspace")
    unchanged(store_g, "store")
    for g in plan_g:
        unchanged(g, "plan")
    assert same_bits(peaks_g.cpu(torch.float32), want), (peaks_g.cpu(torch.float32), want)
    assert float(want.max()) >= (0.99 if dtype == torch.int16 else 1e3) and int((want == 0).sum()) >= 3     # the gaps are inside some; some are empty


# ---- end to end: test.py's loop ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def recordings():
    g = torch.Generator().manual_seed(31)
    lengths = torch.randint(4800, 51201, (12,), generator=g).tolist()                      # 0.3 .. 3.2 s at 16 kHz
    lengths[3], lengths[8] = 51200, 4800
    recs = [(torch.rand(n, generator=g) * 2 - 1) * (0.3 if i % 3 else 1.8) for i, n in enumerate(lengths)]
    return PackedClips(recs, device=DEV)


def reference_loop(model, pc, size, index):
    """test.py, one recording per forward, in stock ops on the device: PeakNormalization, pad_input, the model, the mean."""
    outs, rows = [], []
    with torch.no_grad():
        for i in index:
            r = pc.store[int(pc.offsets_host[i]):int(pc.offsets_host[i]) + int(pc.lengths_host[i])]
            r = PeakNormalization()(r[None])[0]
            L = r.numel()
            n = -(-L // size)
            left = (n * size - L) // 2
            x = F.pad(r[None, None], (left, n * size - L - left), "replicate").reshape(-1, 1, size)
            rows.append(x)
            outs.append(model(x))
    return outs, rows


class Head(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.leaf, self.fc = Leaf(), torch.nn.Linear(40, 3)

    def forward(self, x):
        return self.fc(self.leaf(x).mean(-1))


@pytest.mark.parametrize("max_rows", [4, 512])
def test_evaluate_recordings_matches_the_reference_loop_through_leaf(max_rows):
    pc = recordings()
    torch.manual_seed(0)
    model = Head().to(DEV).eval()
    index = list(range(12))
    got = evaluate_recordings(model, pc, 16000, max_rows=max_rows)
    outs, rows = reference_loop(model, pc, 16000, index)
    counts = [o.shape[0] for o in outs]
    assert got.shape == (12, 3) and not got.requires_grad and max(counts) == 4 and min(counts) == 1 and sum(counts) > 12
    batch, c = pc.segments(index, 16000)
    assert c.tolist() == counts and same_bits(batch.cpu(), torch.cat(rows).cpu())            # the same rows go in
    with torch.no_grad():
        # what 2e-5 on every LEAF feature (all positive with PCEN) means behind the mean over time and the linear layer
        scale = torch.stack([(model.leaf(x).mean(-1) @ model.fc.weight.abs().T).mean(0) for x in rows])
    want = torch.stack([o.mean(0) for o in outs])
    err = (got - want).abs() / scale
    print(f"max_rows={max_rows}: worst |got - want| / (|W| mean features) = {float(err.max()):.3e}")
    assert float(err.max()) <= REL_TOL


@pytest.mark.parametrize("max_rows", [4, 512])
def test_evaluate_recordings_matches_the_reference_loop_with_a_linear_head(max_rows):
    pc = recordings()
    torch.manual_seed(1)
    fc = torch.nn.Linear(16000, 3).double().to(DEV)
    # float64 inside, so that the rows' outputs do not depend on the GEMM kernel picked for a batch size: what is compared is the mean
    model = lambda x: fc(x[:, 0].double()).float()
    index = [11, 3, 3, 0, 8, 5]
    got = evaluate_recordings(model, pc, 16000, index, max_rows=max_rows)
    outs, _ = reference_loop(model, pc, 16000, index)
    batch, counts = pc.segments(index, 16000)
    with torch.no_grad():
        packed = segment_mean(model(batch), counts)
    assert got.shape == packed.shape == (6, 3) and got.dtype == torch.float32
    for place, preds in enumerate(outs):
        bound = mean_bound(preds, preds.shape[0])
        for name, res in (("evaluate_recordings", got), ("segment_mean", packed)):
            err = float((res[place] - preds.mean(0)).abs().max())
            print(f"max_rows={max_rows} {name} recording {index[place]}: {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (name, place, err, bound)
