"""The plan drawn on the device (leaf_draw_clip_plan, DeviceClipSampler) against the oracle of tests/test_host_clip_draws.py: the plan
itself, the step counter, hostile ``order`` entries, the batch made from it, and the captured graph."""
import numpy as np
import pytest
import torch

from leaf_pytorch_amd import DeviceClipSampler, PackedClips, _native
from test_host_clip_draws import LENGTHS, NOISE_LENGTHS, S, compare, plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x1234_5678_9abc_def0
M = 3
FULL = dict(num_masks=M, time_perc=0.3, gain_prob=0.5, noise_prob=0.6, gaussian_prob=0.5)


def _packed(lengths, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    recs = [torch.randint(-30000, 30000, (n,), dtype=torch.int16, generator=g) for n in lengths]
    if dtype == torch.float32:
        recs = [r.float() / 16384 for r in recs]                                # peaks above 1: the normalisation is live
    return PackedClips(recs, device=DEV)


@pytest.fixture(scope="module", params=[torch.int16, torch.float32], ids=["int16", "float32"])
def stores(request):
    return _packed(LENGTHS, request.param, 3), _packed(NOISE_LENGTHS, request.param, 4)


def make(stores, noise=True, **kw):
    clips, nclips = stores
    return DeviceClipSampler(clips, S, noise_clips=nclips if noise else None, seed=kw.pop("seed", SEED), **kw)


def as_dict(plan) -> dict:
    """A ClipNoisePlan of the sampler, copied to the CPU, under the oracle's names."""
    cpu = lambda t: t.cpu().numpy()
    d = dict(rec_off=cpu(plan.rec_off), rec_len=cpu(plan.rec_len), start=cpu(plan.start), pad_mode=cpu(plan.pad_mode), gain=cpu(plan.gain),
             index=cpu(plan.index))
    if plan.masks is not None:
        d["masks"] = cpu(plan.masks)
    if plan.rec is not None:
        d["rec"] = cpu(plan.rec)
    if plan.noise is not None:
        d.update(zip(("noise_off", "noise_len", "noise_start", "noise_pad_mode", "coeff"), (cpu(t) for t in plan.noise)))
    if plan.gaussian is not None:
        d["gauss_amp"], d["gauss_stream"] = cpu(plan.gaussian[0]), cpu(plan.gaussian[2])
    return d


def want(s: DeviceClipSampler, step: int, B: int, index=None, order=None):
    return plan_ref(s.consts, S, s.train, s.seed, s.stream_base, step, B, LENGTHS, index=index, order=order,
                    noise_lengths=None if s.noise_clips is None else NOISE_LENGTHS)


def _from_cpu_plan(s: DeviceClipSampler, plan) -> torch.Tensor:
    """``_native.assemble_clips`` fed the kernel's own plan copied to the CPU: there it goes through ``clip_plan`` / ``noise_plan``,
    which raise ValueError for a draw outside the store, its span, the pad modes or [0, 1]."""
    cpu = lambda t: None if t is None else t.cpu()
    noise = None if plan.noise is None else (s.noise_clips.store,) + tuple(cpu(t) for t in plan.noise)
    gaussian = None if plan.gaussian is None else (cpu(plan.gaussian[0]), plan.gaussian[1], cpu(plan.gaussian[2]))
    rec_off, rec_len, start, pad_mode, gain, masks = (cpu(t) for t in plan)
    return _native.assemble_clips(s.clips.store, rec_off, rec_len, start, pad_mode, S, gain, s.peak_normalize, masks, noise=noise,
                                  gaussian=gaussian, standardize=None if plan.rec is None else (s.clips.moments(), cpu(plan.rec)))


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 5, 300])                                      # 300: more clips than lanes, the stride loop
def test_the_plan_is_the_oracles(stores, B):
    index = [(7 * b + 5) % len(LENGTHS) for b in range(B)]
    s = make(stores, standardize=True, stream_base=2 ** 40, **FULL)
    for where in ("cpu", DEV):                                                  # a CPU index is copied, a device index is used as it is
        s.set_step(9)
        got = as_dict(s.plan(torch.tensor(index, device=where)))
        assert {"masks", "rec", "coeff", "gauss_amp", "index"} <= set(got)
        compare(got, want(s, 9, B, index=index))
    assert s.step == 10 and torch.equal(s.index.cpu(), torch.tensor(index))


def test_the_centre_crop_and_each_group_left_out(stores):
    index = list(range(len(LENGTHS)))
    B = len(index)
    s = make(stores, train=False, **FULL)
    got = as_dict(s.plan(index))
    compare(got, want(s, 0, B, index=index))
    assert got["start"].tolist() == [max(n - S, 0) // 2 for n in LENGTHS] and "rec" not in got       # no standardisation: no rec
    for kw, gone in ((dict(FULL, num_masks=0), "masks"), (dict(FULL, gaussian_prob=0.0), "gauss_amp")):
        s = make(stores, **kw)
        got = as_dict(s.plan(index))
        assert gone not in got and "coeff" in got
        compare(got, want(s, 0, B, index=index))
    s = make(stores, noise=False, **FULL)
    got = as_dict(s.plan(index))
    assert "coeff" not in got and "noise_len" not in got and "gauss_amp" in got
    compare(got, want(s, 0, B, index=index))
    # the entry itself with nothing but the required outputs: a null gain, rec and index_out are not written either
    clips = stores[0]
    state = torch.full((1,), 4, dtype=torch.int64, device=DEV)
    out = dict(rec_off=torch.zeros(B, dtype=torch.int64, device=DEV), **{n: torch.zeros(B, dtype=torch.int32, device=DEV) for n in ("rec_len", "start", "pad_mode")})
    bare = dict(s.consts, num_masks=0)
    _native.draw_clip_plan(B, S, True, clips.offsets, clips.lengths, state, SEED, 0, bare, out, index=torch.tensor(index, device=DEV))
    compare({n: t.cpu().numpy() for n, t in out.items()}, plan_ref(bare, S, True, SEED, 0, 4, B, LENGTHS, index=index))
    assert int(state.item()) == 5


def test_order_is_walked_by_the_counter(stores):
    order = [3, 5, 5, 0]                                                        # N = 4 < B: the place wraps inside a batch and across steps
    s = make(stores, order=torch.tensor(order, device=DEV), batch_size=7, **FULL)
    s.set_step(3)
    got = as_dict(s.plan())
    compare(got, want(s, 3, 7, order=order))
    assert got["index"].tolist() == [order[(3 * 7 + b) % 4] for b in range(7)] and torch.equal(s.index.cpu(), torch.from_numpy(got["index"]))


# ---- the counter ------------------------------------------------------------------------------------------------------------------------

def test_the_counter_steps_repeats_and_wraps(stores):
    index = [5, 4, 3, 2, 1]
    s = make(stores, stream_base=11, **FULL)
    assert s.step == 0
    s.set_step(6)
    plans = []
    for step in (6, 7, 8):                                                      # three consecutive calls: steps s, s + 1, s + 2
        got = as_dict(s.plan(index))
        compare(got, want(s, step, 5, index=index))
        plans.append(got)
    assert s.step == 9 and not np.array_equal(plans[0]["gauss_stream"], plans[1]["gauss_stream"])
    assert plans[1]["gauss_stream"].tolist() == [11 + 7 * 5 + b for b in range(5)]
    a, b = as_dict(s.plan(index, advance=False)), as_dict(s.plan(index, advance=False))   # advance = 0 repeats a step
    assert s.step == 9 and all(np.array_equal(a[n], b[n]) for n in a)
    compare(a, want(s, 9, 5, index=index))
    for step in (2 ** 64 - 1, 2 ** 63 + 5):                                     # close to 2^64: step B + b wraps as the oracle's does
        s.set_step(step)
        assert s.step == step
        compare(as_dict(s.plan(index)), want(s, step, 5, index=index))
        assert s.step == (step + 1) % 2 ** 64
    order = [5, 4, 0]
    so = make(stores, order=torch.tensor(order, device=DEV), batch_size=5, stream_base=2 ** 64 - 2, **FULL)
    so.set_step(2 ** 64 - 1)
    compare(as_dict(so.plan()), want(so, 2 ** 64 - 1, 5, order=order))


# ---- what cannot be seen is clamped -------------------------------------------------------------------------------------------------------

def test_hostile_order_entries_are_clamped(stores):
    R = len(LENGTHS)
    order = [-5, R + 9, 2, -2 ** 62, 2 ** 62]
    s = make(stores, order=torch.tensor(order, device=DEV), batch_size=8, **FULL)
    got = as_dict(s.plan(advance=False))
    compare(got, want(s, 0, 8, order=order))
    assert got["index"].min() >= 0 and got["index"].max() < R and got["index"].tolist()[:5] == [0, R - 1, 2, 0, R - 1]
    x = s()                                                                     # the batch of that plan assembles
    assert x.shape == (8, 1, S) and bool(torch.isfinite(x).all()) and s.step == 1
    assert torch.equal(x.view(torch.int32), _from_cpu_plan(s, s.plan(advance=False) if s.set_step(0) is None else None).view(torch.int32))
    hostile = torch.tensor([-1, R, 2 ** 40, -2 ** 40], device=DEV)              # ... and a device index likewise
    compare(as_dict(s.plan(hostile, advance=False)), want(s, 0, 4, index=hostile.tolist()))


# ---- the batch --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(FULL, standardize=True), dict(noise=False)], ids=["everything", "plain"])
def test_the_batch_is_assemble_clips_on_the_kernels_plan(stores, kw):
    index = torch.tensor([(5 * b + 2) % len(LENGTHS) for b in range(17)], device=DEV)
    s = make(stores, **kw)
    for step in (0, 1):
        ref = _from_cpu_plan(s, s.plan(index, advance=False))
        x = s(index)
        assert s.step == step + 1 and x.shape == (17, 1, S) and x.dtype == torch.float32
        assert torch.equal(x.view(torch.int32), ref.view(torch.int32))
    out = torch.empty((17, 1, S), device=DEV)
    s.set_step(0)
    first = s(index, out=out).clone()
    assert s(index, out=out) is out and not torch.equal(first, out)             # another step, another batch


# ---- the graph --------------------------------------------------------------------------------------------------------------------------

def test_a_captured_step_draws_a_new_plan_on_every_replay(stores):
    B, s0 = 9, 5
    a, b = (make(stores, batch_size=B, standardize=True, **FULL) for _ in range(2))
    static = torch.zeros((B, 1, S), device=DEV)
    a(out=static)                                                               # warm: the library is loaded, the buffers exist
    torch.cuda.synchronize()
    a.set_step(s0)
    b.set_step(s0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one stream, a chain of two kernels
        a(out=static)
    a.set_step(s0)                                                              # (whatever the capture did to the counter)
    batches = []
    for step in range(3):
        graph.replay()
        eager = b()
        assert torch.equal(static.view(torch.int32), eager.view(torch.int32)), step
        assert torch.equal(a.index, b.index)
        batches.append(static.clone())
    assert not torch.equal(batches[0], batches[1]) and not torch.equal(batches[1], batches[2]) and not torch.equal(batches[0], batches[2])
    assert a.step == s0 + 3 == b.step
