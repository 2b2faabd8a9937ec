"""leaf_clip_effects_f32 on the device: ClipValue and the sox-style reverb in one launch (csrc/inst_clip_effects.hip;
``_native.clip_effects`` / ``EffectsClipSampler`` on top).  Every comparison is bit for bit -- the definition rounds every float32
operation on its own and fixes the order, so there is nothing to tolerate: the kernel against the NumPy oracle of
tests/test_host_clip_effects.py on that file's cases (the shapes at which the chunking can go wrong: the shortest line of 20 samples at
8 kHz, the largest layout at 48 kHz, S around the chunk, the wave and the lines, a tail that decays into subnormals), ClipValue
against torch.clamp on the CPU, skipped clips, exact-size guarded buffers with a hostile device plan, graph capture, and the sampler
against ``ClipSampler`` and against the CPU composition of the three launches."""
import numpy as np
import pytest
import torch

import test_host_clip_effects as H
from leaf_pytorch_amd import ClipSampler, EffectsClipSampler, PackedClips, _native
from guarded import guarded, guarded_tensor, unchanged
from test_gpu_clips import pack, peaknorm, same_bits
from test_host_clip_noise import assemble_noise_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_case(case_id, device_plan=False):
    """The kernel on a case of tests/test_host_clip_effects.py: (x, y) as (B, S) NumPy arrays."""
    rate, x, factor, feedback, damp, comb = H.build(case_id)
    plan = [torch.from_numpy(t.copy()) for t in (factor, feedback, damp, comb)]
    if device_plan:
        plan = [t.to(DEV) for t in plan]
    xd = torch.from_numpy(x.copy()).to(DEV)
    y = _native.clip_effects(xd[:, None, :].contiguous(), plan[0], (plan[1], plan[2], plan[3]), rate, H.WET)
    assert y.shape == (x.shape[0], 1, x.shape[1]) and y.dtype == torch.float32 and y.is_contiguous()
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                          # x is read-only
    return x, y[:, 0].cpu().numpy()


def mismatch(got, want):
    bad = np.argwhere(H.bits(got) != H.bits(want))
    return f"{len(bad)} samples differ, the first at (clip, sample) {tuple(bad[0])}" if len(bad) else ""


@pytest.mark.parametrize("case_id", sorted(H.CASES))
def test_the_kernel_against_the_oracle(case_id):
    x, got = run_case(case_id)
    want = H.oracle(case_id)
    assert np.array_equal(H.bits(got), H.bits(want)), (case_id, mismatch(got, want))
    for b, (_, factor, rev) in enumerate(H.CASES[case_id][2]):                  # a clip that takes neither step is a bit copy
        if factor < 0 and rev is H.SKIP:
            assert np.array_equal(H.bits(got[b]), H.bits(x[b])), (case_id, b)


def test_the_tail_decays_into_subnormals_on_the_device_too():
    _, got = run_case("8000-subnormal-tail", device_plan=True)
    tiny = np.finfo(np.float32).tiny
    mag = np.abs(got[0][got[0] != 0])
    assert (mag < tiny).sum() > 100 and np.array_equal(H.bits(got), H.bits(H.oracle("8000-subnormal-tail")))


def test_clip_value_is_torch_clamp():
    for case_id in ("clipvalue-S37", "clipvalue-S1"):
        x, got = run_case(case_id)
        for b, (_, factor, _) in enumerate(H.CASES[case_id][2]):
            xb = torch.from_numpy(x[b])
            if factor < 0:
                want = xb
            else:
                f = torch.tensor(factor, dtype=torch.float32)
                want = torch.clamp(xb, min=float(xb.min() * f), max=float(xb.max() * f))
            assert torch.equal(torch.from_numpy(got[b]), want), (case_id, b)
    x, got = run_case("clipvalue-S37")
    assert got[0].min() == np.float32(-0.45) and got[0].max() == np.float32(0.4)      # extremes at the first and the last sample
    assert got[1].min() > 0 and not got[2].any() and np.array_equal(H.bits(got[3]), H.bits(x[3]))
    # ClipValue alone, no reverb group at all
    rate, x, factor, _, _, _ = H.build("clipvalue-S37")
    alone = _native.clip_effects(torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(factor.copy()))
    assert alone.shape == x.shape and np.array_equal(H.bits(alone.cpu().numpy()), H.bits(got))


def test_both_steps_in_one_call_are_the_two_oracles_composed():
    rate, x, factor, feedback, damp, comb = H.build("both-S588")
    _, got = run_case("both-S588")
    _, allpass = H.lengths_ref(rate, 100)
    for b in range(x.shape[0]):
        want = H.clip_value_ref(x[b], factor[b])
        if comb[b][0] > 0:
            want = H.reverb_ref(want, feedback[b], damp[b], comb[b], allpass)
        assert np.array_equal(H.bits(got[b]), H.bits(want)), b
    assert not np.array_equal(got[0], x[0]) and not np.array_equal(got[1], x[1])


@pytest.mark.parametrize("case_id", ["16000-S588-B5", "8000-S65-B5", "48000-S588-B5"])
def test_a_clip_does_not_depend_on_its_neighbours_or_on_alignment(case_id):
    rate, x, factor, feedback, damp, comb = H.build(case_id)
    B, S = x.shape
    want = H.oracle(case_id)
    t = lambda a, rows: torch.from_numpy(a[rows].copy())
    for offset in (0, 4):                                                       # x and y on and off a 16-byte boundary
        gx = guarded_tensor(torch.from_numpy(x.copy()), offset)
        gy = guarded(4 * B * S, 0x5A, offset)
        _native.clip_effects(gx.view(torch.float32, (B, 1, S)), t(factor, slice(None)), tuple(t(a, slice(None)) for a in (feedback, damp, comb)),
                             rate, H.WET, out=gy.view(torch.float32, (B, 1, S)))
        torch.cuda.synchronize()
        unchanged(gx, "x")
        gy.check("y")
        assert np.array_equal(H.bits(gy.cpu(torch.float32, (B, S)).numpy()), H.bits(want)), offset
        for b in range(B):                                                      # every clip alone, the skipped one too
            rows = slice(b, b + 1)
            gx1 = guarded_tensor(torch.from_numpy(x[rows].copy()), offset)
            y1 = _native.clip_effects(gx1.view(torch.float32, (1, S)), t(factor, rows), tuple(t(a, rows) for a in (feedback, damp, comb)), rate, H.WET)
            assert np.array_equal(H.bits(y1.cpu().numpy()), H.bits(want[rows])), (offset, b)
    assert np.array_equal(H.bits(want[2]), H.bits(x[2]))                        # the skipped clip


def test_guarded_buffers_and_a_hostile_device_plan():
    rate, S = 16000, 700
    big = 10 ** 9
    comb = np.array([[big, 0, -7, big, 3, 0, -7, big], [0, big, big, big, big, big, big, big], [-7, 5, 5, 5, 5, 5, 5, 5],
                     [big] * 8, [1, -big, 1, 1, 1, 1, 1, 1]], dtype=np.int32)
    B = comb.shape[0]
    x = np.stack([H.signal("noise", S, 50 + b) for b in range(B)])
    factor = np.array([0.3, -1.0, 0.0, -1.0, 0.9], dtype=np.float32)
    feedback, damp = np.full(B, 0.88, dtype=np.float32), np.full(B, 0.35, dtype=np.float32)
    want = H.effects_ref(x, factor, feedback, damp, comb, rate)                 # the oracle run with the clamped lengths
    assert np.isfinite(want).all()
    for offset in (0, 4):
        gx = guarded_tensor(torch.from_numpy(x), offset)
        gplan = [guarded_tensor(torch.from_numpy(a), offset) for a in (factor, feedback, damp, comb)]      # exact-size, on the device
        gy = guarded(4 * B * S, 0xA5, offset)
        views = [g.view(dt, shape) for g, dt, shape in zip(gplan, (torch.float32,) * 3 + (torch.int32,), ((B,), (B,), (B,), (B, 8)))]
        _native.clip_effects(gx.view(torch.float32, (B, S)), views[0], tuple(views[1:]), rate, H.WET, out=gy.view(torch.float32, (B, S)))
        torch.cuda.synchronize()
        unchanged(gx, "x")
        for g, name in zip(gplan, ("clip_factor", "feedback", "damp", "comb")):
            unchanged(g, name)
        gy.check("y")
        got = gy.cpu(torch.float32, (B, S)).numpy()
        assert np.isfinite(got).all() and np.array_equal(H.bits(got), H.bits(want)), offset
    # the same plan on the CPU is refused by the host
    with pytest.raises(ValueError):
        _native.clip_effects(torch.from_numpy(x).to(DEV), None, (torch.from_numpy(feedback), torch.from_numpy(damp), torch.from_numpy(comb)), rate)
    with pytest.raises(ValueError, match="overlap"):
        xd = torch.from_numpy(x).to(DEV)
        _native.clip_effects(xd, out=xd)


def test_a_captured_launch_follows_its_device_plan():
    rate, S, B = 16000, 588, 5
    x = torch.from_numpy(np.stack([H.signal("noise", S, 7 + b) for b in range(B)])).to(DEV)
    plans = []
    for rev, dmp, room, factor in (([50] * B, [50] * B, [0, 25, 50, 75, 100], [0.1, -1, 0.2, -1, 0.05]),
                                   ([10, 90, 30, 70, 50], [0, 100, 50, 20, 80], [100, 0, 37, 100, 5], [-1, 0.15, -1, 0.0, 0.1])):
        fb, dp, comb = _native.reverb_plan(rev, dmp, room, rate)
        plans.append((torch.tensor(factor, dtype=torch.float32), fb, dp, comb))
    plans[1][3][2] = 0                                                          # the second plan skips clip 2's reverb
    static = [t.clone().to(DEV) for t in plans[0]]
    out = torch.zeros((B, S), device=DEV)
    _native.clip_effects(x, static[0], tuple(static[1:]), rate, H.WET, out=out)  # warm: the library is loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.clip_effects(x, static[0], tuple(static[1:]), rate, H.WET, out=out)
    for plan in (plans[1], plans[0], plans[1]):
        for dst, src in zip(static, plan):
            dst.copy_(src)
        out.fill_(7.0)
        graph.replay()
        eager = _native.clip_effects(x, plan[0], tuple(plan[1:]), rate, H.WET)
        assert same_bits(out.cpu(), eager.cpu())
    a, b = (_native.clip_effects(x, p[0], tuple(p[1:]), rate, H.WET).cpu() for p in plans)
    assert not torch.equal(a, b)


# ---- EffectsClipSampler -------------------------------------------------------------------------------------------------------------

LENGTHS = (5, 1500, 1499, 1501, 4000, 1, 700)
SIZE = 1500


def stores(dtype):
    store, offsets, lengths = pack(LENGTHS, dtype, seed=3)
    nstore, noffsets, nlengths = pack((900, 1500, 5000), dtype, seed=4)
    return PackedClips.from_store(store.to(DEV), offsets, lengths), PackedClips.from_store(nstore.to(DEV), noffsets, nlengths)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["float32", "int16"])
def test_without_effects_the_batch_is_clip_samplers(dtype):
    clips, noise = stores(dtype)
    kw = dict(noise_clips=noise, noise_prob=0.7, num_masks=3, time_perc=0.2, gain_prob=0.6, gaussian_prob=0.5)
    index = torch.arange(len(LENGTHS)).repeat(3)
    for seed in (9, 10):                                                        # (fresh samplers: the effect draws move the generator on)
        a = ClipSampler(clips, SIZE, generator=torch.Generator().manual_seed(seed), **kw)
        e = EffectsClipSampler(clips, SIZE, generator=torch.Generator().manual_seed(seed), **kw)
        want, got = a(index), e(index)
        assert got.shape == (index.numel(), 1, SIZE) and same_bits(got.cpu(), want.cpu()), seed
    assert bool((want == 0).any()) and float(want.abs().max()) > 0


def test_with_effects_the_batch_is_the_cpu_composition():
    clips, noise = stores(torch.float32)
    B = 4
    index = torch.tensor([1, 4, 0, 3])
    kw = dict(noise_clips=noise, noise_prob=0.7, num_masks=2, time_perc=0.2, gain_prob=0.6, gaussian_prob=0.6, clip_prob=1.0, reverb_prob=1.0,
              max_clip_val=0.9)
    e = EffectsClipSampler(clips, SIZE, generator=torch.Generator().manual_seed(13), **kw)
    plan = EffectsClipSampler(clips, SIZE, generator=torch.Generator().manual_seed(13), **kw).plan(index)
    got = e(index).cpu()
    assert got.shape == (B, 1, SIZE) and bool((plan.clip_factor >= 0).all()) and bool((plan.reverb[2][:, 0] > 0).all())
    rec_off, rec_len, start, pad_mode, gain, masks = plan
    # launch 1: pad / crop and background noise
    raw = assemble_noise_ref(clips.store, rec_off, rec_len, start, pad_mode, SIZE, noise=(noise.store,) + tuple(plan.noise[:4]) + (
        _native.noise_coefficients(plan.noise[4]),))
    # launch 2: the effects
    fb, dp, comb = (t.numpy() for t in plan.reverb)
    wet = torch.from_numpy(H.effects_ref(raw.numpy(), plan.clip_factor.numpy(), fb, dp, comb, 16000))
    # launch 3: gain, Gaussian noise, peak normalisation, masks over the batch as a store of B recordings of SIZE samples
    amp, seed, stream = plan.gaussian
    rows = torch.arange(B)
    want = assemble_noise_ref(wet.reshape(-1), rows * SIZE, torch.full((B,), SIZE), torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64),
                              SIZE, gain, masks, peaknorm, gaussian=(amp, _native.gaussian_noise(B, SIZE, seed, stream, device=DEV).cpu()))
    assert same_bits(got[:, 0], want), int((got[:, 0].view(torch.int32) != want.view(torch.int32)).sum())
    assert not torch.equal(wet, raw)
