"""Waveform standardisation (audio_config.normalize) on the device: leaf_clip_moments_f32, leaf_assemble_clips_std_f32 and
leaf_assemble_segments_std_f32 (csrc/leaf_clips.hpp; PackedClips.moments / assemble / segments, evaluate_recordings and ClipSampler
with ``standardize=True`` on top).

The moments are held to float64 numpy within one float32 rounding (tests/test_host_clip_moments.py: ``moments_ref64`` and the two
bounds); min and max bit for bit.  Everything behind them is bit for bit: the oracles put the stock torch expression
``(r - mean) / (std + 1e-9)`` -- on 0-d float32 tensors that hold THE LIBRARY'S moments -- in front of the existing CPU oracles of
the assembly, and every further step is a correctly rounded fp32 operation or none.  Recordings of one sample (std NaN) and with a
NaN sample are compared as NaN, not by their bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from leaf_pytorch_amd import ClipSampler, PackedClips, PeakNormalization, _native, evaluate_recordings
from guarded import guarded, guarded_tensor, unchanged
from test_gpu_clips import pack, same_bits
from test_host_clips import MIN, REPLICATE, WRAP, ZERO, assemble_ref, clamp_plan
from test_host_clip_moments import (CONST, NAN, SPANS, assemble_std_ref, mean_bound, moment_store, moments_ref, moments_ref64,
                                    parser, segments_std_ref, standardize_ref, standardized_peak, std_bound)
from test_host_segments import clamp_segment_plan, mean_bound as mean_of_rows_bound, rows_ref, segments_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOTH = pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
REREAD = _native.ASSEMBLE_RESIDENT_MAX + 1             # 32766: the smallest clip on the re-reading path
SEED = 0x1234_5678_9abc_def0


def peaknorm(y):
    return PeakNormalization()(y.to(DEV)).cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_bits(got, want, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not same_bits(got, want):
        bad = (bits(got) != bits(want)).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} samples differ, first at row {int(bad[0, 0])} sample {int(bad[0, 1])}: "
                             f"{float(got[tuple(bad[0])])!r} for {float(want[tuple(bad[0])])!r}")


# ---- the moments -------------------------------------------------------------------------------------------------------------------

def check_moments(got, store, off, ln, what=""):
    """``got`` (R, 4) on the CPU against float64 numpy: the two bounds, min and max by their bits, NaN where the oracle has NaN."""
    m64 = moments_ref64(store, off, ln)
    mb, sb = mean_bound(m64), std_bound(m64)
    g = got.double().numpy()
    for i in range(len(ln)):
        for c, bound in ((0, mb[i]), (1, sb[i])):
            if np.isnan(m64[i, c]):
                assert np.isnan(g[i, c]), (what, i, c, g[i])
            else:
                err = abs(g[i, c] - m64[i, c])
                print(f"{what} recording {i} (L={int(ln[i])}) {'mean' if c == 0 else 'std'}: off by {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (what, i, c, g[i, c], m64[i, c], bound)
        assert g[i, 2] == np.float32(m64[i, 2]) and g[i, 3] == np.float32(m64[i, 3]), (what, i, g[i], m64[i])


@BOTH
def test_moments_against_float64_and_they_do_not_follow_the_grid_or_the_alignment(dtype):
    store, off, ln = moment_store(dtype)
    R = len(ln)
    dev_store = store.to(DEV)
    got = _native.clip_moments(dev_store, off, ln)
    assert got.shape == (R, 4) and got.dtype == torch.float32 and got.device.type == "cuda"
    got = got.cpu()
    check_moments(got, store, off, ln, str(dtype))
    assert bool(torch.isnan(got[0, 1])) and float(got[0, 0]) == float(got[0, 2]) == float(got[0, 3])          # L == 1
    assert got[CONST].tolist() == [0.25, 0.0, 0.25, 0.25]
    if dtype == torch.float32:
        assert bool(torch.isnan(got[NAN, :2]).all()) and not bool(torch.isnan(got[NAN, 2:]).any())
    # the same recordings, one sample further on in a store of another alignment ...
    shifted = torch.cat([store[:1], store]).to(DEV)
    assert same_bits(_native.clip_moments(shifted[1:], off, ln).cpu(), got)
    assert same_bits(_native.clip_moments(shifted, off + 1, ln).cpu(), got)
    # ... and in a list of 20 R recordings in another order: more units than the launch has waves (they walk several), another grid
    order = torch.arange(R).flip(0).repeat(20)
    assert order.numel() * SPANS > 2048 * 4
    many = _native.clip_moments(dev_store, off[order], ln[order]).cpu()
    assert same_bits(many, got[order])
    empty = _native.clip_moments(dev_store, [0, 5], [0, 0]).cpu()
    assert empty[:, [0, 2, 3]].tolist() == [[0.0] * 3] * 2 and bool(torch.isnan(empty[:, 1]).all())


@BOTH
def test_packed_clips_keeps_its_moments_and_a_constant_recording_standardises_to_zeros(dtype):
    store, off, ln = moment_store(dtype)
    pc = PackedClips.from_store(store.to(DEV), off, ln)
    got = pc.moments()
    assert pc.moments() is got and same_bits(got.cpu(), _native.clip_moments(store.to(DEV), off, ln).cpu())
    rows = pc.assemble([CONST, CONST, CONST], [0, 700, 0], 1000, ["zero", "zero", "min"], standardize=True).cpu()
    assert float(rows.abs().max()) == 0.0                                   # (0.25 - 0.25) / 1e-9, and the 'min' pad value too
    seg, counts = pc.segments([CONST], 512, standardize=True)
    assert counts.tolist() == [4] and float(seg.abs().max()) == 0.0
    one = pc.assemble([0], [0], 16, "replicate", standardize=True).cpu()      # L == 1: std NaN, the clip is NaN as in the reference
    assert bool(torch.isnan(one).all())
    pc.store[int(off[CONST])] += 1 if dtype == torch.int16 else 0.5
    assert pc.moments() is got
    pc.refresh_moments()
    assert float(pc.moments()[CONST, 1]) > 0 and same_bits(pc.moments()[:CONST].cpu(), got[:CONST].cpu())


@BOTH
def test_a_hostile_recording_list_on_the_device_is_clamped(dtype):
    lib = _native.load()
    T = 1024
    store, off, ln = pack([3 * T + 9, 40, T, 7], dtype, seed=6)
    N, R = store.numel(), 10
    big = 2 ** 31 - 1
    rec_off = torch.tensor([-5, N + 100, int(off[0]), N, 2 ** 40, int(off[1]), N - 3, -2 ** 62, int(off[2]), int(off[3])])
    rec_len = torch.tensor([T + 3, 50, big, 10, 5, -3, big, 20, T, -2 ** 31], dtype=torch.int64)
    c_off, c_len, _, _ = clamp_segment_plan(N, rec_off, rec_len, torch.zeros(R, dtype=torch.int64), torch.zeros(R, dtype=torch.int64), 1, 1)
    assert int((c_len == 0).sum()) >= 3 and int(c_len.max()) > 3 * T
    store_g = guarded_tensor(store.to(DEV), offset=store.element_size())
    plan_g = [guarded_tensor(rec_off.to(DEV)), guarded_tensor(rec_len.to(torch.int32).to(DEV))]
    ws_bytes = lib.leaf_clip_moments_workspace_bytes(R)
    assert ws_bytes == 520 * R
    mom_g, ws_g = guarded(16 * R, 0xA5, offset=4), guarded(ws_bytes, 0xA5, offset=16)
    rc = lib.leaf_clip_moments_f32(store_g.ptr, N, _native.FLAG_X_PCM16 if dtype == torch.int16 else 0, R, plan_g[0].ptr, plan_g[1].ptr,
                                   mom_g.ptr, ws_g.ptr, ws_bytes, _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    mom_g.check("moments")
    ws_g.check("workspace")
    unchanged(store_g, "store")
    for g in plan_g:
        unchanged(g, "plan")
    check_moments(mom_g.cpu(torch.float32, (R, 4)), store, c_off.tolist(), c_len.tolist(), "hostile")


# ---- assemble, bit for bit ---------------------------------------------------------------------------------------------------------------

def noise_groups(kind, dtype, B, size, seed):
    """(noise for the library, noise for the oracle, gaussian for the library, gaussian for the oracle) of ``kind``."""
    noise = noise_ref = gauss = gauss_ref = None
    if kind in ("noise", "both"):
        nstore, noff, nln = pack([size + 5, max(size // 2, 1), 3 * size, 2], dtype, seed=seed + 50)
        pick = torch.arange(B) % 4
        nlen = nln[pick].clone()
        nlen[B // 2] = 0                                                    # one clip without background noise
        nstart = (nlen - size).clamp(min=0) // 2
        coeff = _native.noise_coefficients([(0.9, 0.75, 0.6)[b % 3] for b in range(B)])
        group = (noff[pick], nlen, nstart, torch.full((B,), REPLICATE), coeff)
        noise, noise_ref = (nstore.to(DEV),) + group, (nstore,) + group
    if kind in ("gauss", "both"):
        amp = torch.tensor([(0.015, 0.0, 0.3)[b % 3] for b in range(B)])
        streams = torch.arange(B) + 2 ** 33
        gauss, gauss_ref = (amp, SEED, streams), (amp, _native.gaussian_noise(B, size, SEED, streams, device=DEV).cpu())
    return noise, noise_ref, gauss, gauss_ref


def run_std(store, off, ln, rec, start, mode, size, gain=None, normalize=True, masks=None, kind="none", seed=0, what=""):
    """One standardising launch against the oracle on the library's own moments; returns (got, want, moments) on the CPU."""
    dev_store, rec = store.to(DEV), torch.as_tensor(rec)
    moments = _native.clip_moments(dev_store, off, ln)
    noise, noise_ref, gauss, gauss_ref = noise_groups(kind, store.dtype, len(rec), size, seed)
    want = assemble_std_ref(store, off, ln, moments, rec, start, mode, size, gain, masks, peaknorm if normalize else None, noise_ref, gauss_ref)
    got = _native.assemble_clips(dev_store, off[rec], ln[rec], start, mode, size, gain, normalize, masks, noise=noise, gaussian=gauss,
                                 standardize=(moments, rec))
    assert got.shape == (len(rec), 1, size) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu()[:, 0]
    assert not bool(torch.isnan(want).any())
    assert_same_bits(got, want, what)
    return got, want, moments.cpu()


def pad_and_crop_case(size):
    """Recordings of 2, 5 and S - 1 samples in every pad mode (odd and even padding, several periods), S and S + 1, and one of
    3 S + 7 cropped at its first, a middle and its last start: (lengths, rec, start, mode)."""
    lengths = [2, 5, size - 1, size, size + 1, 3 * size + 7]
    rec, start, mode = [], [], []
    for i, n in enumerate(lengths[:3]):
        if n < size:
            for m in (ZERO, MIN, REPLICATE, WRAP):
                rec.append(i), start.append(0), mode.append(m)
    rec += [3, 4, 4, 5, 5, 5]
    start += [0, 0, 1, 0, (2 * size + 7) // 3, 2 * size + 7]
    mode += [ZERO, MIN, REPLICATE, WRAP, ZERO, MIN]
    return lengths, torch.tensor(rec), torch.tensor(start), torch.tensor(mode)


@BOTH
@pytest.mark.parametrize("kind", ["none", "noise", "gauss", "both"])
@pytest.mark.parametrize("size", [16, 65, 1025])
def test_assemble_standardises_the_whole_recording_in_front_of_everything(size, kind, dtype):
    lengths, rec, start, mode = pad_and_crop_case(size)
    store, off, ln = pack(lengths, dtype, seed=size)
    B = len(rec)
    gain = torch.tensor([(3.0, 0.5, 1.0, 2.5)[b % 4] for b in range(B)])
    masks = torch.tensor([[[size // 3, size // 4 + 1], [size - 2, 5]]] * B, dtype=torch.int32)
    got, _, _ = run_std(store, off, ln, rec, start, mode, size, gain, True, masks, kind, seed=size, what=f"S={size} {kind}")
    assert float(got.abs().max()) <= 1.0
    run_std(store, off, ln, rec, start, mode, size, None, False, None, kind, seed=size, what=f"S={size} {kind}, no gain, no peak step")


@BOTH
@pytest.mark.parametrize("kind", ["none", "both"])
def test_assemble_on_the_re_reading_path(kind, dtype):
    size = REREAD
    assert size == 32766 and size > _native.ASSEMBLE_NOISE_RESIDENT_MAX
    store, off, ln = pack([size - 1, 2 * size + 3, 40], dtype, seed=3)
    rec, start, mode = torch.tensor([0, 1, 1, 2, 2]), torch.tensor([0, 0, size + 3, 0, 0]), torch.tensor([MIN, ZERO, ZERO, WRAP, REPLICATE])
    gain = torch.tensor([1.0, 0.5, 2.0, 1.0, 3.0])
    run_std(store, off, ln, rec, start, mode, size, gain, True, None, kind, seed=1, what=f"S={size} {kind}")


@BOTH
@pytest.mark.parametrize("size", [1000, 1001, 1002, 1003])
def test_every_source_and_row_alignment(size, dtype):
    lengths = [1500, 1501, 1502, 1503, 1504, 900, 901, 902]
    store, off, ln = pack(lengths, dtype, seed=size, gaps=[4, 1, 1, 1, 1, 3, 2, 5])
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
    start, mode = torch.tensor([0, 1, 2, 3, 250, 0, 0, 0]), torch.tensor([ZERO] * 5 + [REPLICATE, WRAP, MIN])
    run_std(store, off, ln, torch.arange(8), start, mode, size, None, True, None, what=f"S={size}")     # rows at 4 S b bytes: every shift for odd S


def test_the_moments_are_the_recordings_not_the_clips():
    """A recording whose extremes and most of whose offset lie outside the cropped window, and a short one padded with 'min': a
    clip-local mean / std, or a pad value from the raw minimum, gives other bits -- and the oracle tells them apart."""
    size = 1000
    store, off, ln = pack([4 * size, 600], torch.float32, seed=8, amp=0.05)
    store[int(off[0]) + 3 * size:int(off[0]) + 4 * size] += 0.8               # the offset: in the last quarter
    store[int(off[0]) + 3 * size + 10], store[int(off[0]) + 3 * size + 20] = 2.5, -1.5         # ... and so are the extremes
    got, want, mo = run_std(store, off, ln, [0, 1], [size // 2, 0], [ZERO, MIN], size, None, False, None, what="outside the window")
    window = store[int(off[0]) + size // 2:int(off[0]) + size // 2 + size]
    local = parser(window, window.mean(), window.std())
    assert not same_bits(local, got[0]) and float((local - got[0]).abs().max()) > 0.1
    assert abs(float(got[0].mean())) > 0.3 and float(got[0].std()) < 0.5     # the window is neither centred nor of unit deviation
    raw_min = float(store[int(off[1]):int(off[1]) + 600].min())
    assert float(got[1, 0]) == float(got[1, -1]) == float(parser(torch.tensor(raw_min), mo[1, 0], mo[1, 1])) == float(got[1].min())
    assert float(got[1, 0]) != raw_min and float(got[1, 0]) < -1.0


def test_an_int16_clip_leaves_the_unit_interval_and_the_peak_step_scales_it():
    size = 1000
    store, off, ln = pack([1500, 1500, 700], torch.int16, seed=2, amp=3000)
    store[int(off[0]) + 100] = 32767                                         # inside the window of clip 0: about ten deviations
    rec, start, mode = [0, 1, 2], [50, 0, 0], [ZERO, ZERO, MIN]
    got, _, _ = run_std(store, off, ln, rec, start, mode, size, None, True, None, what="int16, normalised")
    raw, _, _ = run_std(store, off, ln, rec, start, mode, size, None, False, None, what="int16, not normalised")
    assert float(raw.abs().amax(1).min()) > 1.0 and float(raw[0].abs().max()) > 5.0
    assert float(got.abs().max()) == pytest.approx(1.0, abs=1e-6) and not same_bits(got, raw)
    plain = _native.assemble_clips(store.to(DEV), off, ln, start, mode, size).cpu()[:, 0]
    assert float(plain.abs().max()) <= 1.0 and not same_bits(plain, got)


@BOTH
@pytest.mark.parametrize("size", [65, 1000, REREAD + 1])
def test_a_hostile_plan_on_the_device_is_clamped(size, dtype):
    lib = _native.load()
    lengths = [size + 9, 40, 2 * size, 7, size - 1, 300, 1, size]
    store, off, ln = pack(lengths, dtype, seed=4)
    N, B, R = store.numel(), 12, 5
    item, big = store.element_size(), 2 ** 31 - 1
    rec_off = torch.tensor([-5, N + 100, int(off[2]), N, 2 ** 40, int(off[1]), int(off[4]), N - 3, -2 ** 62, int(off[3]), int(off[0]), int(off[5])])
    rec_len = torch.tensor([size + 3, 50, big, 10, 5, -3, size - 1, big, 20, 7, size + 9, 300], dtype=torch.int64)
    start = torch.tensor([-7, 0, big, 3, 0, 0, 5, -big, 1, 2, 10 ** 6, -1], dtype=torch.int64)
    pad_mode = torch.tensor([9, 1, 2, 3, -1, 2, 1, 3, 2, -2 ** 31, 0, 4], dtype=torch.int64)
    rec = torch.tensor([-1, R, big, 0, 1, 2, 3, 4, -2 ** 31, 2, 1, 0], dtype=torch.int64)
    gain = torch.tensor([1.0, 2.0, 0.5, 3.0, 1.0, 1.0, 5.0, 1.0, 2.0, 1.5, 1.0, 2.0])
    masks = torch.tensor([[[-2 ** 31, big], [0, 0]], [[big, big], [5, 3]], [[-2 ** 31, -2 ** 31], [size - 1, big]]] * 4, dtype=torch.int32)
    masks[0::3, 0, 0] = -2 ** 31 + size // 2 + 1
    c_off, c_len, c_start, c_mode = clamp_plan(N, rec_off, rec_len, start, pad_mode, size)
    c_rec = rec.clamp(0, R - 1)
    # the table: any moments -- but the one clip that is padded with 'min' (clip 6, row 3) finds its recording's minimum there
    x = store.float() / 32768 if dtype == torch.int16 else store
    assert [b for b in range(B) if int(c_mode[b]) == MIN and 0 < int(c_len[b]) < size] == [6] and int(c_rec[6]) == 3
    moments = torch.tensor([[0.1, 0.5, -0.4, 0.4], [-0.2, 0.01, -0.3, 0.1], [0.0, 2.0, -1.0, 1.0],
                            [0.05, 0.2, float(x[int(c_off[6]):int(c_off[6]) + int(c_len[6])].min()), 0.4], [1.0, 1e-3, 0.0, 0.0]])
    want = []
    for b in range(B):
        o, L, i = int(c_off[b]), int(c_len[b]), int(c_rec[b])
        own = parser(x[o:o + L].clone(), moments[i, 0], moments[i, 1])        # the clip's clamped recording, standardised by its row
        want.append(assemble_ref(own, [0], [L], [int(c_start[b])], [int(c_mode[b])], size, gain[b:b + 1], masks[b:b + 1], peaknorm))
    want = torch.cat(want)

    store_g = guarded_tensor(store.to(DEV), offset=item)                     # element alignment only: 2 / 4 bytes past a page
    plan_g = [guarded_tensor(t.to(DEV)) for t in (rec_off, rec_len.to(torch.int32), start.to(torch.int32), pad_mode.to(torch.int32),
                                                   gain, masks, moments, rec.to(torch.int32))]
    out_g = guarded(4 * B * size, 0xA5, offset=4)
    rc = lib.leaf_assemble_clips_std_f32(store_g.ptr, N, _native.FLAG_X_PCM16 if dtype == torch.int16 else 0, B, size,
                                         *(g.ptr for g in plan_g[:5]), 1, plan_g[5].ptr, 2, out_g.ptr,
                                         None, 0, None, None, None, None, None, None, 0, None,
                                         plan_g[6].ptr, plan_g[7].ptr, R, _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    out_g.check(f"out, S={size}")
    unchanged(store_g, "store")
    for g in plan_g:
        unchanged(g, "plan")
    got = out_g.cpu(torch.float32, (B, size))
    assert not bool((bits(got) == torch.tensor(0xA5A5A5A5 - 2 ** 32, dtype=torch.int64).to(torch.int32)).any())   # fully written
    assert_same_bits(got, want, f"hostile, S={size}")


# ---- segments and evaluate_recordings ------------------------------------------------------------------------------------------------------

def segment_lengths(S):
    return sorted({n for n in (2, 3, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 2, 7 * S + 3) if n >= 2})


@BOTH
@pytest.mark.parametrize("size", [4, 5, 13, 16000])
def test_segments_follow_test_py_with_the_parser_in_front(size, dtype):
    lengths = segment_lengths(size) if size < 100 else [16000, 40003, 15999, 16001, 52]
    store, off, ln = pack(lengths, dtype, seed=size % 11)
    if dtype == torch.float32:
        for i in range(0, len(lengths), 2):
            store[int(off[i]) + int(ln[i]) - 1] = 2.5 if i % 4 else -2.5     # the raw peak: the recording's last sample
    pc = PackedClips.from_store(store.to(DEV), off, ln)
    mo = pc.moments().cpu()
    index = list(range(len(lengths)))[::-1] + [1, 1, 0]                       # any order, repeats
    y = standardize_ref(store, off, ln, mo)
    peak = standardized_peak(mo)
    for i in range(len(lengths)):                                            # the peak from min / max is the materialised recording's, by its bits
        assert float(peak[i]) == float(y[int(off[i]):int(off[i]) + int(ln[i])].abs().max()), i
    assert bool((peak > 1).any())
    want, counts = segments_std_ref(store, off, ln, mo, index, size, peaknorm)
    got, got_counts = pc.segments(index, size, standardize=True)
    assert got.shape == (int(counts.sum()), 1, size) and got.dtype == torch.float32 and torch.equal(got_counts, counts)
    assert_same_bits(got.cpu()[:, 0], want, f"S={size}")
    assert float(want.abs().max()) == pytest.approx(1.0, abs=1e-6)           # the scaling was launched, for the int16 store too
    raw, _ = segments_std_ref(store, off, ln, mo, index, size)
    plain, _ = pc.segments(index, size, normalize=False, standardize=True)
    assert_same_bits(plain.cpu()[:, 0], raw, f"S={size}, normalize=False")
    assert float(raw.abs().max()) > 1.0
    assert not same_bits(peaknorm(raw), want)                                # a per-row peak gives other bits
    _, rec_rows, win, _ = pc.segment_plan(index, size)
    raw_peaks = pc.peaks().cpu()
    by_raw_peak = rows_ref(y, pc.offsets_host[rec_rows], pc.lengths_host[rec_rows], win, size,
                           [torch.tensor(1.0) / raw_peaks[i] if float(raw_peaks[i]) > 1 else None for i in rec_rows.tolist()])
    assert not same_bits(by_raw_peak, want)                                  # ... and so does the raw recording's peaks()
    unscaled, _ = pc.segments(index, size)                                   # the keyword's default: the rows the parent cut
    assert_same_bits(unscaled.cpu()[:, 0], segments_ref(store, off, ln, index, size, peaknorm)[0], f"S={size}, standardize=False")


@BOTH
@pytest.mark.parametrize("size", [13, 1000, 40000])
def test_a_hostile_row_plan_on_the_device_is_clamped(size, dtype):
    lib = _native.load()
    lengths = [size + 9, 40, 2 * size, 7, size - 1, 300, 1, size]
    store, off, ln = pack(lengths, dtype, seed=4)
    N, rows, R = store.numel(), 14, 6
    item, big = store.element_size(), 2 ** 31 - 1
    rec_off = torch.tensor([-5, N + 100, int(off[2]), N, 2 ** 40, int(off[1]), int(off[4]), N - 3, -2 ** 62, int(off[3]), int(off[0]), int(off[5]),
                            int(off[2]), int(off[7])])
    rec_len = torch.tensor([size + 3, 50, big, 10, 5, -3, size - 1, big, 20, 7, size + 9, 300, 2 * size, size], dtype=torch.int64)
    win = torch.tensor([-7, 0, 2 ** 62, 3, 0, 0, -2 ** 62, -big, 2 ** 63 - 1, -2 ** 63, size, -size - 1, size - 3, 2 ** 31])
    rec = torch.tensor([-1, R, big, 0, 1, 2, 3, 4, 5, -2 ** 31, 2, 1, 0, 5], dtype=torch.int64)
    moments = torch.tensor([[0.1, 0.5, -0.4, 0.4], [-0.2, 0.01, -0.3, 0.1], [0.0, 2.0, -1.0, 1.0], [0.05, 0.2, -0.1, 0.4], [1.0, 1e-3, 0.0, 0.0],
                            [0.0, 1.0, -3.0, 2.0]])
    c_off, c_len, c_win, c_rec = clamp_segment_plan(N, rec_off, rec_len, win, rec, size, R)
    peak = standardized_peak(moments)
    assert bool((peak > 1).any()) and bool((peak <= 1).any())
    x = store.float() / 32768 if dtype == torch.int16 else store
    want = []
    for b in range(rows):
        o, L, i = int(c_off[b]), int(c_len[b]), int(c_rec[b])
        own = parser(x[o:o + L].clone(), moments[i, 0], moments[i, 1])
        want.append(rows_ref(own, torch.tensor([0]), torch.tensor([L]), torch.tensor([int(c_win[b])]), size,
                             [torch.tensor(1.0) / peak[i] if float(peak[i]) > 1 else None]))
    want = torch.cat(want)

    store_g = guarded_tensor(store.to(DEV), offset=item)
    plan_g = [guarded_tensor(t.to(DEV)) for t in (rec_off, rec_len.to(torch.int32), win, rec.to(torch.int32), moments)]
    out_g = guarded(4 * rows * size, 0xA5, offset=4)
    rc = lib.leaf_assemble_segments_std_f32(store_g.ptr, N, _native.FLAG_X_PCM16 if dtype == torch.int16 else 0, rows, size,
                                            plan_g[0].ptr, plan_g[1].ptr, plan_g[2].ptr, None, plan_g[3].ptr, R, out_g.ptr, plan_g[4].ptr, 1,
                                            _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    out_g.check(f"out, S={size}")
    unchanged(store_g, "store")
    for g in plan_g:
        unchanged(g, "plan")
    got = out_g.cpu(torch.float32, (rows, size))
    assert not bool((bits(got) == torch.tensor(0xA5A5A5A5 - 2 ** 32, dtype=torch.int64).to(torch.int32)).any())   # fully written
    assert_same_bits(got, want, f"hostile, S={size}")


@functools.lru_cache(maxsize=None)
def recordings():
    g = torch.Generator().manual_seed(31)
    lengths = [4800, 51200, 16000, 20001, 7, 33000]
    return PackedClips([(torch.rand(n, generator=g) * 2 - 1) * (0.3 if i % 3 else 1.8) + 0.1 * i for i, n in enumerate(lengths)], device=DEV)


@pytest.mark.parametrize("max_rows", [4, 512])
def test_evaluate_recordings_standardises_as_the_reference_loop_does(max_rows):
    pc = recordings()
    torch.manual_seed(1)
    fc = torch.nn.Linear(16000, 3).double().to(DEV)
    model = lambda x: fc(x[:, 0].double()).float()                          # float64 inside: a row's output does not follow its batch
    index = [5, 1, 1, 0, 4, 3]
    got = evaluate_recordings(model, pc, 16000, index, max_rows=max_rows, standardize=True)
    store, off, ln = pc.store.cpu(), pc.offsets_host, pc.lengths_host
    rows, counts = segments_std_ref(store, off, ln, pc.moments(), index, 16000, peaknorm)
    batch, c = pc.segments(index, 16000, standardize=True)
    assert torch.equal(c, counts) and same_bits(batch.cpu()[:, 0], rows)
    with torch.no_grad():
        preds = model(rows[:, None].to(DEV))
    a = 0
    for place, n in enumerate(counts.tolist()):
        err = float((got[place] - preds[a:a + n].mean(0)).abs().max())
        assert err <= mean_of_rows_bound(preds[a:a + n], n), (place, err)
        a += n
    assert not torch.allclose(got, evaluate_recordings(model, pc, 16000, index, max_rows=max_rows))


# ---- the sampler, and the default ----------------------------------------------------------------------------------------------------------

def test_a_standardising_sampler_assembles_its_own_plan():
    pc = recordings()
    kw = dict(gain_prob=0.6, gain_db=(-3.0, 6.0), time_perc=0.1, num_masks=3, gaussian_prob=0.5)
    index = torch.tensor([5, 0, 1, 5, 4, 2, 3, 1])
    plan = ClipSampler(pc, 16000, generator=torch.Generator().manual_seed(8), standardize=True, **kw).plan(index)
    x = ClipSampler(pc, 16000, generator=torch.Generator().manual_seed(8), standardize=True, **kw)(index)
    amp, seed, streams = plan.gaussian
    z = _native.gaussian_noise(8, 16000, seed, streams, device=DEV).cpu()
    want = assemble_std_ref(pc.store.cpu(), pc.offsets_host, pc.lengths_host, pc.moments(), plan.rec, plan.start, plan.pad_mode, 16000, plan.gain,
                            plan.masks, peaknorm, None, (amp, z))
    assert x.shape == (8, 1, 16000) and plan.rec.tolist() == index.tolist()
    assert_same_bits(x.cpu()[:, 0], want, "sampler")
    same_draws = ClipSampler(pc, 16000, generator=torch.Generator().manual_seed(8), **kw)(index)
    assert not same_bits(same_draws.cpu(), x.cpu())


@BOTH
def test_without_the_keyword_every_call_is_the_old_one(dtype):
    lib = _native.load()
    size = 1001
    lengths, rec, start, mode = pad_and_crop_case(size)
    store, off, ln = pack(lengths, dtype, seed=12)
    pc = PackedClips.from_store(store.to(DEV), off, ln)
    B = len(rec)
    gain = torch.tensor([(3.0, 0.5, 1.0, 2.5)[b % 4] for b in range(B)])
    masks = torch.tensor([[[size // 3, size // 4 + 1]]] * B, dtype=torch.int32)
    want = assemble_ref(store, off[rec], ln[rec], start, mode, size, gain, masks, peaknorm)
    for got in (pc.assemble(rec, start, size, mode, gain, True, masks), pc.assemble(rec, start, size, mode, gain, True, masks, standardize=False)):
        assert_same_bits(got.cpu()[:, 0], want, "assemble")
    assert pc._moments is None                                              # nothing was computed for it
    # the C entry without its group IS the noise entry, which without its groups IS the plain one
    flags = _native.FLAG_X_PCM16 if dtype == torch.int16 else 0
    dev = [t.to(DEV) for t in (off[rec], ln[rec].to(torch.int32), start.to(torch.int32), mode.to(torch.int32), gain, masks)]
    outs = [torch.full((B, size), 7.0, device=DEV) for _ in range(2)]
    head = lambda out: (ctypes.c_void_p(pc.store.data_ptr()), store.numel(), flags, B, size, *(ctypes.c_void_p(t.data_ptr()) for t in dev[:5]), 1,
                        ctypes.c_void_p(dev[5].data_ptr()), 1, ctypes.c_void_p(out.data_ptr()))
    stream = _native.stream_ptr(torch.device(DEV))
    assert lib.leaf_assemble_clips_f32(*head(outs[0]), stream) == 0
    assert lib.leaf_assemble_clips_std_f32(*head(outs[1]), None, 0, None, None, None, None, None, None, 0, None, None, None, 0, stream) == 0
    torch.cuda.synchronize()
    assert_same_bits(outs[0].cpu(), want, "plain entry")
    assert_same_bits(outs[1].cpu(), want, "std entry, no group")
    seg, _ = pc.segments([5, 0, 2], 300)
    assert_same_bits(seg.cpu()[:, 0], segments_ref(store, off, ln, [5, 0, 2], 300, peaknorm)[0], "segments")
