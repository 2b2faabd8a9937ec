"""leaf_assemble_clips_f32 on the device: per-clip pad, crop, gain, peak normalisation and time masks in one launch
(csrc/leaf_clips.hpp; PackedClips / ClipSampler on top).  Every comparison is bit for bit: steps 1, 2 and 4 against
``assemble_ref`` (tests/test_host_clips.py: numpy.pad / F.pad / slicing on the CPU), step 3 against transforms.PeakNormalization on
the device -- each step is one correctly rounded fp32 operation or none, so there is nothing to tolerate.

The stores are recordings packed back to back with full-scale samples (+-32767 / +-1e3) between them: a read one sample outside a
recording changes a minimum, a peak or an output value.  Shapes are the kernel's edges, not the workload's: sizes around the wave,
the workgroup and the 16-byte chunk, the documented cut-over of the resident path (_native.ASSEMBLE_RESIDENT_MAX) from both sides,
recordings of 1, 2, S - 1, S, S + 1 and 3 S + 7 samples, every pad mode, both stores, every source and row alignment."""
import functools

import pytest
import torch

from leaf_pytorch_amd import ClipSampler, Leaf, PackedClips, PeakNormalization, _native
from guarded import guarded, guarded_tensor, unchanged
from test_host_clips import MIN, REPLICATE, WRAP, ZERO, assemble_ref, clamp_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUT = _native.ASSEMBLE_RESIDENT_MAX                    # 32765: the largest clip that stays in registers


def path_of(size):
    return "resident" if size <= CUT else "reread"


def pack(lengths, dtype, seed=0, gaps=None, amp=None):
    """Recordings of ``lengths`` samples packed behind, between and in front of full-scale gaps (``gaps[i]`` samples in front of
    recording i, one more gap at the end).  Returns (store on the CPU, offsets, lengths)."""
    g = torch.Generator().manual_seed(seed)
    gaps = list(gaps) if gaps is not None else [1 + (i * 3 + seed) % 4 for i in range(len(lengths))]
    parts, offsets, pos = [], [], 0
    for i, (n, gap) in enumerate(zip(lengths, gaps + [3])):
        sign = torch.tensor([1, -1]).repeat(gap // 2 + 1)[:gap]
        parts.append((sign * 32767).to(torch.int16) if dtype == torch.int16 else sign.float() * 1e3)
        pos += gap
        offsets.append(pos)
        if dtype == torch.int16:
            parts.append(torch.randint(-(amp or 9000), (amp or 9000) + 1, (n,), generator=g).to(torch.int16))
        else:
            parts.append((torch.rand(n, generator=g) * 2 - 1) * (amp or 0.4))
        pos += n
    parts.append(torch.full((3,), 32767, dtype=torch.int16) if dtype == torch.int16 else torch.full((3,), -1e3))
    return torch.cat(parts), torch.tensor(offsets), torch.tensor(list(lengths))


def peaknorm(y):
    return PeakNormalization()(y.to(DEV)).cpu()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(store, rec_off, rec_len, start, pad_mode, size, gain=None, normalize=True, masks=None, what=""):
    """One launch against the oracle; returns the result (B, size) on the CPU."""
    want = assemble_ref(store, rec_off, rec_len, start, pad_mode, size, gain, masks, peaknorm if normalize else None)
    got = _native.assemble_clips(store.to(DEV), rec_off, rec_len, start, pad_mode, size, gain, normalize, masks)
    assert got.shape == (len(rec_off), 1, size) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu()[:, 0]
    if not same_bits(got, want):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} samples differ, first at clip {int(bad[0, 0])} sample {int(bad[0, 1])}: "
                             f"{float(got[tuple(bad[0])])!r} for {float(want[tuple(bad[0])])!r}")
    return got


def starts(rec_len, size):
    """0, max(L, S) - S and a value in between, in turn."""
    span = (rec_len - size).clamp(min=0)
    return torch.stack([(0 * s, s, s // 3)[i % 3] for i, s in enumerate(span)])


def edge_lengths(S):
    return [n for n in (1, 2, S - 1, S, S + 1, 3 * S + 7) if n >= 1]


# ---- sizes and the two paths -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("size", [1, 63, 64, 65, 1000, 1024, 1025, 16000, CUT, CUT + 1, CUT + 4100])
def test_every_size_on_its_path(size, B, dtype):
    assert path_of(size) == ("reread" if size in (CUT + 1, CUT + 4100) else "resident") and CUT == 32765
    lengths = edge_lengths(size)
    lengths = [lengths[(2 + b) % len(lengths)] for b in range(B)]                          # S - 1, S, S + 1, 3 S + 7, 1
    store, off, ln = pack(lengths, dtype, seed=size % 7)
    mode = torch.tensor([(WRAP, MIN, REPLICATE, ZERO, MIN)[b] for b in range(B)])
    gain = torch.tensor([(3.0, 0.5, 1.0, 2.5, 4.0)[b] for b in range(B)])                   # int16 |x| <= 0.28: 4.0 lifts the peak above 1
    masks = torch.tensor([[[size // 3, size // 4 + 1], [size - 2, 5]]] * B, dtype=torch.int32)
    out = check(store, off, ln, starts(ln, size), mode, size, gain, True, masks, f"S={size} ({path_of(size)})")
    assert float(out.abs().max()) <= 1.0


# ---- padding: every mode, odd and even padding, several periods, the three starts ---------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("size", [16, 65, 1025])
def test_padding_modes_lengths_and_starts(size, dtype):
    lengths, modes = [], []
    for n in edge_lengths(size) + [5, 3 * size + 7, 3 * size + 7]:                        # S > 3 L for L = 1, 2, 5: several periods
        for mode in (ZERO, MIN, REPLICATE, WRAP):
            lengths.append(n)
            modes.append(mode)
    store, off, ln = pack(lengths, dtype, seed=size)
    st = starts(ln, size)
    long = (ln == 3 * size + 7).nonzero().reshape(-1)
    assert {int(st[i]) for i in long} == {0, 2 * size + 7, (2 * size + 7) // 3}             # start at 0, at Lp - S, in between
    assert {int((size - n) % 2) for n in lengths if n < size} == {0, 1}                     # odd and even padding
    check(store, off, ln, st, torch.tensor(modes), size, None, False, None, f"S={size}")


# ---- alignment of the source and of the rows ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("size", [1000, 1001, 1002, 1003])
def test_every_source_and_row_alignment(size, dtype):
    lengths = [1500, 1501, 1502, 1503, 1504, 900, 901, 902]
    store, off, ln = pack(lengths, dtype, seed=size, gaps=[4, 1, 1, 1, 1, 3, 2, 5])
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3} and {int(o) % 2 for o in off[:5]} == {0, 1}
    st = torch.tensor([0, 1, 2, 3, 250, 0, 0, 0])
    mode = torch.tensor([ZERO] * 5 + [REPLICATE, WRAP, MIN])
    check(store, off, ln, st, mode, size, None, True, None, f"S={size}")                   # rows at 4 S b bytes: every shift for odd S


def test_an_int16_store_gives_the_bits_of_its_float32_image():
    size = 1000
    store, off, ln = pack([1, 999, 1000, 1001, 3007, 40], torch.int16, seed=5, amp=32767)
    st, mode = starts(ln, size), torch.tensor([WRAP, MIN, ZERO, REPLICATE, ZERO, WRAP])
    gain = torch.tensor([1.0, 1.7, 0.9, 1.2, 2.0, 1.01])
    masks = torch.tensor([[[10, 50]]] * 6, dtype=torch.int32)
    a = _native.assemble_clips(store.to(DEV), off, ln, st, mode, size, gain, True, masks)
    b = _native.assemble_clips((store.float() / 32768).to(DEV), off, ln, st, mode, size, gain, True, masks)
    assert same_bits(a.cpu(), b.cpu())
    check(store, off, ln, st, mode, size, gain, True, masks, "int16 full scale")


# ---- gain and peak normalisation ---------------------------------------------------------------------------------------------------

def test_gain_and_peak_normalisation():
    size = 1000
    store, off, ln = pack([1500, 1500, 1500, 1500, 600, 1500], torch.float32, seed=9, amp=0.5)
    store[off[5] + 7] = 3.0                                                               # a clip that is too loud without any gain
    store[off[4] + 100] = -0.75                                                           # the short recording's minimum is its peak
    st, mode = torch.tensor([3, 4, 5, 6, 0, 0]), torch.tensor([ZERO, ZERO, ZERO, ZERO, MIN, ZERO])
    rec = lambda b: store[off[b] + st[b]: off[b] + st[b] + min(size, int(ln[b]))]
    lift, keep = 1.5 / float(rec(2).abs().max()), 0.999 / float(rec(3).abs().max())
    gain = torch.tensor([1.0, 1.0, lift, keep, 2.5, 1.0])
    plain = check(store, off, ln, st, mode, size, None, True, None, "no gain")
    ones = check(store, off, ln, st, mode, size, torch.ones(6), True, None, "gain 1")
    assert same_bits(plain, ones) and torch.equal(plain[0], rec(0)) and float(plain[5].abs().max()) == 1.0
    out = check(store, off, ln, st, mode, size, gain, True, None, "gains")
    assert float(out[2].abs().max()) == pytest.approx(1.0, abs=1e-6) and not torch.equal(out[2], rec(2) * gain[2])     # it fired
    assert torch.equal(out[3], rec(3) * gain[3]) and 0.99 < float(out[3].abs().max()) <= 1.0                          # it did not
    # the minimum of a min-padded clip is its peak: the padding carries it, and the scale comes from it
    lo = float(rec(4).min())
    assert lo < 0 and -lo * 2.5 > 1.0 and -lo >= float(rec(4).abs().max())
    assert lo == -0.75 and float(out[4, 0]) == float(out[4].min()) == float(out[4, -1]) and abs(float(out[4, 0]) + 1.0) < 1e-6
    raw = check(store, off, ln, st, mode, size, gain, False, None, "normalize off")
    assert torch.equal(raw[2], rec(2) * gain[2]) and float(raw[2].abs().max()) > 1.4 and float(raw[5].abs().max()) == 3.0
    assert float(raw[4, 0]) == lo * 2.5


# ---- masks -------------------------------------------------------------------------------------------------------------------------

def test_masks():
    size = 1000
    store, off, ln = pack([1000] * 8, torch.float32, seed=2, amp=0.9)
    store[off[7] + 500] = 5.0                                                             # the peak sample, inside a mask
    spans = [[[0, 0], [0, 0]],             # n = 0: nothing
             [[0, 100], [0, 0]],           # at t0 = 0
             [[900, 100], [0, 0]],         # ending at S
             [[100, 200], [250, 200]],     # overlapping
             [[950, 500], [0, 0]],         # reaching past S
             [[-50, 120], [-10, 5]],       # t0 < 0; a span that ends before the clip begins
             [[300, -7], [2000, 10]],      # n < 0; a span behind the clip
             [[490, 20], [0, 0]]]          # over the peak
    masks = torch.tensor(spans, dtype=torch.int32)
    st, mode = torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)
    out = check(store, off, ln, st, mode, size, None, True, masks, "masks")
    none = check(store, off, ln, st, mode, size, None, True, None, "no masks")
    assert torch.equal(out[0], none[0]) and torch.equal(out[6], none[6])
    zeroed = [(b, (out[b] == 0).nonzero().reshape(-1)) for b in range(8)]
    want = {1: range(0, 100), 2: range(900, 1000), 3: range(100, 450), 4: range(950, 1000), 5: range(0, 70), 7: range(490, 510)}
    for b, z in zeroed:
        assert z.tolist() == list(want.get(b, [])), b
    # the scale comes from the masked peak: every other sample is the recording's divided by 5
    rec = store[off[7]: off[7] + size]
    keep = torch.ones(size, dtype=torch.bool)
    keep[490:510] = False
    assert torch.equal(out[7][keep], (rec * (torch.tensor(1.0) / 5.0))[keep]) and float(out[7].abs().max()) < 0.2
    many = torch.tensor([[[7 * m, 3] for m in range(40)]] * 8, dtype=torch.int32)          # M beyond any unrolling
    check(store, off, ln, st, mode, size, None, True, many, "40 masks")


# ---- a plan the library cannot see: clamped, and nothing outside the buffers is touched ---------------------------------------------

@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("size", [65, 1000, CUT + 2])
def test_a_hostile_plan_on_the_device_is_clamped(size, dtype):
    lib = _native.load()
    lengths = [size + 9, 40, 2 * size, 7, size - 1, 300, 1, size]
    store, off, ln = pack(lengths, dtype, seed=4)
    N, B = store.numel(), 12
    item = store.element_size()
    big = 2 ** 31 - 1
    rec_off = torch.tensor([-5, N + 100, int(off[2]), N, 2 ** 40, int(off[1]), int(off[4]), N - 3, -2 ** 62, int(off[3]), int(off[0]), int(off[5])])
    rec_len = torch.tensor([size + 3, 50, big, 10, 5, -3, size - 1, big, 20, 7, size + 9, 300], dtype=torch.int64)
    start = torch.tensor([-7, 0, big, 3, 0, 0, 5, -big, 1, 2, 10 ** 6, -1], dtype=torch.int64)
    pad_mode = torch.tensor([9, 1, 2, 3, -1, 2, 1, 3, 2, -2 ** 31, 0, 4], dtype=torch.int64)
    gain = torch.tensor([1.0, 2.0, 0.5, 3.0, 1.0, 1.0, 5.0, 1.0, 2.0, 1.5, 1.0, 2.0])
    masks = torch.tensor([[[-2 ** 31, big], [0, 0]], [[big, big], [5, 3]], [[-2 ** 31, -2 ** 31], [size - 1, big]]] * 4, dtype=torch.int32)
    masks[0::3, 0, 0] = -2 ** 31 + size // 2 + 1                                           # t0 + n = size // 2: the first half; the other sums overflow 32 bits
    want_plan = clamp_plan(N, rec_off, rec_len, start, pad_mode, size)
    assert int(want_plan[1].min()) == 0 and int(want_plan[1].max()) > size                  # clips of no samples, and crops
    want = assemble_ref(store, *want_plan, size, gain, masks, peaknorm)

    store_g = guarded_tensor(store.to(DEV), offset=item)                                   # element alignment only: 2 / 4 bytes past a page
    plan_g = [guarded_tensor(t.to(DEV)) for t in (rec_off, rec_len.to(torch.int32), start.to(torch.int32), pad_mode.to(torch.int32),
                                                   gain, masks)]
    out_g = guarded(4 * B * size, 0xA5, offset=4)
    rc = lib.leaf_assemble_clips_f32(store_g.ptr, N, _native.FLAG_X_PCM16 if dtype == torch.int16 else 0, B, size,
                                     *(g.ptr for g in plan_g[:5]), 1, plan_g[5].ptr, 2, out_g.ptr, _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    out_g.check(f"out, S={size}")
    unchanged(store_g, "store")
    for g in plan_g:
        unchanged(g, "plan")
    got = out_g.cpu(torch.float32, (B, size))
    assert not bool((got.view(torch.int32) == torch.tensor(0xA5A5A5A5 - 2 ** 32, dtype=torch.int64).to(torch.int32)).any())   # fully written
    assert same_bits(got, want), (got.view(torch.int32) != want.view(torch.int32)).nonzero()[:4]


# ---- the sampler, the frontend, index, empty batch, stream ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dataset():
    g = torch.Generator().manual_seed(21)
    lengths = (16000, 8000, 23456, 15999, 16001, 100, 48007, 3)
    return PackedClips([torch.randint(-32768, 32768, (n,), generator=g).to(torch.int16) for n in lengths], device=DEV)


INDEX = torch.tensor([6, 0, 1, 6, 5, 2, 3, 4, 7, 1])                                      # repeats, any order


def test_the_sampler_assembles_its_own_plan_and_feeds_the_frontend():
    pc = dataset()
    kw = dict(gain_prob=0.6, gain_db=(-3.0, 6.0), time_perc=0.1, num_masks=3)
    plan = ClipSampler(pc, 16000, generator=torch.Generator().manual_seed(8), **kw).plan(INDEX)
    x = ClipSampler(pc, 16000, generator=torch.Generator().manual_seed(8), **kw)(INDEX)
    want = assemble_ref(pc.store, *plan[:4], 16000, plan.gain, plan.masks, peaknorm)
    assert x.shape == (10, 1, 16000) and same_bits(x.cpu()[:, 0], want)
    loud = assemble_ref(pc.store, *plan[:4], 16000, plan.gain).abs().amax(1)
    assert set(plan.pad_mode.tolist()) == {REPLICATE, MIN} and bool((loud > 1).any()) and bool((loud < 1).any())      # normalised, and left alone
    assert float(want.abs().max()) <= 1.0
    ref = want[:, None].to(DEV)
    torch.manual_seed(0)
    leaf = Leaf().to(DEV).eval()
    with torch.no_grad():
        assert same_bits(leaf(x).cpu(), leaf(ref).cpu())                                   # the same input bits through the same kernel
        perm, lam = torch.randperm(10, generator=torch.Generator().manual_seed(1)), torch.rand(10, generator=torch.Generator().manual_seed(2))
        y = leaf.forward_mixup(x, perm, lam)
        assert y.shape == (10, 40, 100) and same_bits(y.cpu(), leaf.forward_mixup(ref, perm, lam).cpu())
    val = ClipSampler(pc, 16000, train=False, pad_modes=("wrap", "wrap"), gain_prob=0.0)
    vp = val.plan(INDEX)
    assert same_bits(val(INDEX).cpu()[:, 0], assemble_ref(pc.store, *vp[:4], 16000, vp.gain, None, peaknorm))


def test_index_with_repeats_on_either_side_the_empty_batch_and_out():
    pc = dataset()
    size = 12000
    st = torch.tensor([5, 0, 0, 36007, 0, 100, 0, 4001, 0, 0])
    a = pc.assemble(INDEX, st, size, "wrap", normalize=False)
    b = pc.assemble(INDEX.to(DEV), st.to(DEV), size, torch.full((10,), WRAP, device=DEV), normalize=False)
    want = assemble_ref(pc.store, pc.offsets_host[INDEX], pc.lengths_host[INDEX], st, [WRAP] * 10, size)
    assert same_bits(a.cpu()[:, 0], want) and same_bits(b.cpu()[:, 0], want)
    assert torch.equal(a[2], a[9]) and not torch.equal(a[0], a[3])                          # one recording, two starts
    empty = pc.assemble([], [], size)
    assert empty.shape == (0, 1, size) and empty.dtype == torch.float32 and empty.device.type == "cuda"
    out = torch.full((10, 1, size), 7.0, device=DEV)
    assert pc.assemble(INDEX, st, size, WRAP, normalize=False, out=out) is out and same_bits(out.cpu()[:, 0], want)
    with pytest.raises(RuntimeError):
        pc.assemble(INDEX, st, size, out=torch.empty((10, size), device=DEV))


def test_a_side_stream():
    pc = dataset()
    side = torch.cuda.Stream(device=DEV)
    st = torch.zeros(10, dtype=torch.int64)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        x = pc.assemble(INDEX, st, 16000, "min", gain=torch.full((10,), 1.5))
    side.synchronize()
    want = assemble_ref(pc.store, pc.offsets_host[INDEX], pc.lengths_host[INDEX], st, [MIN] * 10, 16000, torch.full((10,), 1.5), None, peaknorm)
    assert same_bits(x.cpu()[:, 0], want)
