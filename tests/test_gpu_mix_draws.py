"""Mixup's draws on the device (leaf_draw_mixup, DeviceMixup) against the oracle of tests/test_host_mix_draws.py: perm and lam, the step
counter, the memory contract on guarded buffers, forward_mixup and the targets on the device pair, the errors, and the whole training
step -- sample, draw the mix, forward, backward -- captured into one graph."""
import ctypes

import numpy as np
import pytest
import torch

from guarded import guarded
from leaf_pytorch_amd import DeviceClipSampler, DeviceMixup, Leaf, PackedClips, _native
from test_host_mix_draws import BAD_SHAPE, LAM_TOL, SEED, compare, mix_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def drawn(mix: DeviceMixup, advance: bool = True):
    perm, lam = mix(advance=advance)
    assert perm is mix.perm and lam is mix.lam and perm.dtype == torch.int32 and lam.dtype == torch.float32
    return perm.cpu().numpy()[None], lam.cpu().numpy().astype(np.float64)[None]


def want(mix: DeviceMixup, step: int):
    return mix_ref(mix.batch_size, mix.alpha, mix.seed, mix.stream_base, step)


# ---- the kernel against the oracle -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("B", [1, 2, 3, 64, 255, 256, 257, 1000, 4096,        # one clip, padded sorts, a width and its neighbours, the cap
                               65, 129, 513, 1024, 1025, 2049])                # every size at which the sort, and with it the workgroup, widens
def test_perm_and_lam_are_the_oracles(B, alpha):
    mix = DeviceMixup(B, alpha=alpha, seed=SEED, stream_base=2 ** 40 + 11, device=DEV)
    mix.set_step(6)
    for step in (6, 7):
        perm, lam = drawn(mix)
        assert sorted(perm[0].tolist()) == list(range(B))                       # a permutation
        assert float(lam.min()) >= 0.0 and float(lam.max()) <= 1.0 and not np.isnan(lam).any()
        d = np.abs(lam - want(mix, step)[1].astype(np.float32).astype(np.float64))
        print(f"B={B} alpha={alpha} step={step}: max |lam - oracle| = {float(d.max()):.3e} (bound {LAM_TOL:.3e}), {int((d > 0).sum())} of {B} differ")
        compare(perm, lam, *want(mix, step))
    assert mix.step == 8


# ---- the counter -----------------------------------------------------------------------------------------------------------------------

def test_the_counter_steps_repeats_and_wraps():
    B = 37
    a, b = (DeviceMixup(B, alpha=0.3, seed=SEED, stream_base=11, device=DEV) for _ in range(2))
    assert a.step == 0
    a.set_step(6)
    b.set_step(6)
    for step in (6, 7, 8):                                                      # n calls: steps s .. s + n - 1
        pa, la = drawn(a)
        compare(pa, la, *want(a, step))
        pb, lb = drawn(b)                                                       # two mixers of one seed agree
        assert np.array_equal(pa, pb) and np.array_equal(la, lb)
    assert a.step == 9 == b.step
    first, again = drawn(a, advance=False), drawn(a, advance=False)             # advance = 0 repeats a step
    assert a.step == 9 and np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    compare(*first, *want(a, 9))
    for step in (2 ** 64 - 1, 2 ** 63 + 5):                                     # close to 2^64: step B + b wraps as the oracle's does
        a.set_step(step)
        assert a.step == step
        compare(*drawn(a), *want(a, step))
        assert a.step == (step + 1) % 2 ** 64
    shifted, plain = DeviceMixup(B, alpha=0.3, seed=SEED, stream_base=B, device=DEV), DeviceMixup(B, alpha=0.3, seed=SEED, device=DEV)
    shifted.set_step(4)
    plain.set_step(5)                                                           # step s at stream_base = B is step s + 1 at base 0
    ps, ls = drawn(shifted)
    pp, lp = drawn(plain)
    assert np.array_equal(ps, pp) and np.array_equal(ls, lp)
    other = DeviceMixup(B, alpha=0.3, seed=SEED + 1, device=DEV)
    other.set_step(5)
    assert not np.array_equal(drawn(other)[1], lp)


# ---- the memory contract ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 257, 4096])
def test_the_outputs_stay_inside_exact_size_guarded_buffers(B):
    lib = _native.load()
    state = guarded(8, torch.tensor([3], dtype=torch.int64))
    perm, lam = guarded(4 * B, 0xFF), guarded(4 * B, 0xFF)
    torch.cuda.synchronize()
    rc = lib.leaf_draw_mixup(B, 0.3, state.ptr, 1, SEED, 5, perm.ptr, lam.ptr, None)
    torch.cuda.synchronize()
    assert rc == 0
    for g, name in ((state, "state"), (perm, "perm"), (lam, "lam")):
        g.check(f"leaf_draw_mixup B={B} {name}")
    assert state.cpu(torch.int64).tolist() == [4]
    got_lam = lam.cpu(torch.float32).numpy().astype(np.float64)[None]
    assert not np.isnan(got_lam).any()                                          # 0xFF bytes are a NaN: every entry was written
    compare(perm.cpu(torch.int32).numpy()[None], got_lam, *mix_ref(B, 0.3, SEED, 5, 3))


# ---- forward_mixup and the targets ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["float32", "int16"])
def test_forward_mixup_takes_the_device_pair_as_it_takes_its_copies(dtype):
    B, T = 5, 16000
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-30000, 30000, (B, 1, T), dtype=torch.int16, generator=g)
    x = (x if dtype == torch.int16 else x.float() / 32768).to(DEV)
    leaf = Leaf().to(DEV).eval()
    mix = DeviceMixup(B, alpha=0.3, seed=SEED, device=DEV)
    perm, lam = mix()
    assert len(set(perm.tolist())) == B and not torch.equal(lam, torch.ones_like(lam))
    with torch.no_grad():
        on_device = leaf.forward_mixup(x, perm, lam)
        from_copies = leaf.forward_mixup(x, perm.cpu(), lam.cpu())
    assert on_device.shape == (B, 40, 100) and torch.equal(on_device.view(torch.int32), from_copies.view(torch.int32))


def test_targets_are_the_stock_expression_bit_for_bit():
    B, C = 7, 11
    t = torch.rand(B, C, generator=torch.Generator().manual_seed(7)).to(DEV)
    mix = DeviceMixup(B, alpha=0.3, seed=SEED, device=DEV)
    perm, lam = mix()
    mixed, a, b, c = mix.targets(t)
    stock = t * lam.view(B, 1) + t[perm.long()] * (1 - lam.view(B, 1))          # transforms.Mixup's line, the reference's do_mixup
    assert (a, b, c) == (None, None, None) and mixed.shape == (B, C) and torch.equal(mixed.view(torch.int32), stock.view(torch.int32))
    assert not torch.equal(mixed, t)
    other = DeviceMixup(B, alpha=0.3, seed=SEED, mode="multiclass", device=DEV)
    perm, lam = other()
    labels = torch.arange(B, device=DEV) * 3
    y_a, y_b, lam_out, none = other.targets(labels)
    assert y_a is labels and torch.equal(y_b, labels[perm.long()]) and lam_out is lam and none is None


# ---- the errors ------------------------------------------------------------------------------------------------------------------------

def test_what_the_host_can_see_is_refused_before_any_launch():
    for bad in (dict(batch_size=4097), dict(batch_size=0), dict(batch_size=8, alpha=0.0), dict(batch_size=8, alpha=float("nan"))):
        with pytest.raises(ValueError):
            DeviceMixup(device=DEV, **bad)
    mix = DeviceMixup(8, alpha=0.3, device=DEV)
    for t in (torch.zeros(7, 3, device=DEV), torch.zeros(9, device=DEV), torch.zeros((), device=DEV)):
        with pytest.raises(ValueError):
            mix.targets(t)
    # the C entry: a status, no launch -- the counter and the outputs are as they were
    lib = _native.load()
    state = torch.tensor([5], dtype=torch.int64, device=DEV)
    perm = torch.full((4097,), -7, dtype=torch.int32, device=DEV)
    lam = torch.full((4097,), -7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for B, alpha in ((4097, 0.3), (0, 0.3), (8, 0.0), (8, float("nan")), (8, float("inf")), (8, -1.0)):
        assert lib.leaf_draw_mixup(B, alpha, p(state), 1, SEED, 0, p(perm), p(lam), None) == BAD_SHAPE, (B, alpha)
    torch.cuda.synchronize()
    assert state.item() == 5 and bool((perm == -7).all()) and bool((lam == -7.0).all())
    with pytest.raises(ValueError):
        _native.draw_mixup(8, float("nan"), state, SEED, 0, perm[:8], lam[:8])
    assert state.item() == 5


# ---- the graph -------------------------------------------------------------------------------------------------------------------------

def test_a_whole_training_step_is_captured_and_every_replay_draws_anew():
    B, S, s0 = 8, 16000, 5
    g = torch.Generator().manual_seed(8)
    clips = PackedClips([torch.randint(-30000, 30000, (n,), dtype=torch.int16, generator=g) for n in (S + 1, 2 * S, S - 7, 3 * S + 5, S, 900)], device=DEV)
    samplers = [DeviceClipSampler(clips, S, gain_prob=0.5, num_masks=2, time_perc=0.1, seed=SEED, batch_size=B) for _ in range(2)]
    mixers = [DeviceMixup(B, alpha=0.3, seed=SEED, device=DEV) for _ in range(2)]      # the sampler's seed and ids, numbers of its own
    torch.manual_seed(8)
    leaf = Leaf().to(DEV)
    twin = Leaf().to(DEV)
    twin.load_state_dict(leaf.state_dict())
    go = torch.randn(B, 40, 100, device=DEV)
    static = torch.zeros((B, 1, S), device=DEV)
    held = {}

    def step(sampler, mix, model, out=None):
        x = sampler(out=out)
        perm, lam = mix()
        y = model.forward_mixup(x, perm, lam)
        torch.autograd.backward(y, go)
        return x, y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            leaf.zero_grad(set_to_none=True)
            step(samplers[0], mixers[0], leaf, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for counter in samplers + mixers:
        counter.set_step(s0)
    graph = torch.cuda.CUDAGraph()
    leaf.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        held["x"], held["y"] = step(samplers[0], mixers[0], leaf, static)
    samplers[0].set_step(s0)                                                    # (whatever the capture did to the counters)
    mixers[0].set_step(s0)
    seen = []
    for replay in range(3):
        graph.replay()
        twin.zero_grad(set_to_none=True)
        x, y = step(samplers[1], mixers[1], twin)
        assert held["x"] is static and torch.equal(static.view(torch.int32), x.view(torch.int32)), replay
        assert torch.equal(mixers[0].perm, mixers[1].perm) and torch.equal(mixers[0].lam.view(torch.int32), mixers[1].lam.view(torch.int32)), replay
        assert torch.equal(held["y"].view(torch.int32), y.view(torch.int32)), replay
        for (name, p), q in zip(leaf.named_parameters(), twin.parameters()):
            assert p.grad is not None and torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32)), (replay, name)
        compare(mixers[0].perm.cpu().numpy()[None], mixers[0].lam.cpu().numpy().astype(np.float64)[None], *want(mixers[0], s0 + replay))
        seen.append((mixers[0].perm.clone(), mixers[0].lam.clone()))
    assert all(not torch.equal(seen[i][0], seen[j][0]) or not torch.equal(seen[i][1], seen[j][1]) for i, j in ((0, 1), (1, 2), (0, 2)))
    assert [c.step for c in samplers + mixers] == [s0 + 3] * 4
