"""leaf_assemble_clips_noise_f32 and leaf_gaussian_noise_f32 on the device: background noise at an SNR and Gaussian noise inside the
assembly launch (csrc/leaf_clips.hpp), against the oracles of tests/test_host_clip_noise.py.

The stream is compared with its float64 oracle at 1e-5.  That bound is derived, not measured: |z| <= sqrt(-2 ln 2^-24) = 5.77, and
an error of one or two ulp in each of ln, sqrt and sincospi and in the final product comes to about 3e-6 at that magnitude (an fp32
numpy restatement of the same formula stays within 1.7e-6 of float64 over 2e6 draws).  Everything else is bit for bit, on int32
views: the noise mix against ``assemble_noise_ref`` (three separately rounded fp32 operations), the Gaussian step against the stock
composition of the same steps with the ``z`` tensor ``_native.gaussian_noise`` returns for the same (seed, stream) -- each step is one
correctly rounded fp32 operation, so there is nothing to tolerate.  Shapes are the kernel's edges: sizes around the wave, the
workgroup and the 16-byte chunk, the noise instances' cut-over to the re-reading path from both sides, every alignment of the rows."""
import numpy as np
import pytest
import torch

from leaf_pytorch_amd import ClipSampler, Leaf, PackedClips, _native
from guarded import guarded, guarded_tensor, unchanged
from test_gpu_clips import DEV, pack, peaknorm, same_bits
from test_host_clips import MIN, REPLICATE, WRAP, ZERO, assemble_ref, clamp_plan
from test_host_clip_noise import assemble_noise_ref, gaussian_ref

pytestmark = pytest.mark.gpu
CUT = _native.ASSEMBLE_NOISE_RESIDENT_MAX              # the largest clip a noise instance keeps in registers
SEED = 0x9E3779B97F4A7C15                              # the high word is set
STREAMS = (0, 2 ** 32 + 7, 2 ** 40)
DTYPES = pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["int16", "float32"])


def diff_message(got, want, what):
    bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    return (f"{what}: {bad.shape[0]} of {got.numel()} samples differ, first at clip {int(bad[0, 0])} sample {int(bad[0, 1])}: "
            f"{float(got[tuple(bad[0])])!r} for {float(want[tuple(bad[0])])!r}")


def pairs(B, seed=0):
    """(B, 2) float32 coefficient pairs of SNRs spread over the reference's range and beyond."""
    snr = torch.linspace(-3.0, 26.0, B, dtype=torch.float64) + seed % 3
    return _native.noise_coefficients(_native.snr_coefficients(snr))


# ---- the stream --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [1, 5, 1027])
def test_the_stream_against_its_float64_oracle(size):
    z = _native.gaussian_noise(len(STREAMS), size, SEED, list(STREAMS), device=DEV)
    assert z.shape == (len(STREAMS), size) and z.dtype == torch.float32 and z.device.type == "cuda"
    want = np.stack([gaussian_ref(SEED, s, size) for s in STREAMS])
    err = float(np.abs(z.cpu().numpy().astype(np.float64) - want).max())
    print(f"gaussian_noise size={size}: max |z - oracle| = {err:.3e}")
    assert err <= 1e-5
    other = _native.gaussian_noise(1, size, SEED ^ 1, [0], device=DEV)
    assert size < 5 or not torch.equal(other[0], z[0])                      # the seed's low word is part of the key


def test_a_row_depends_on_its_stream_alone():
    full = _native.gaussian_noise(3, 1027, SEED, list(STREAMS), device=DEV)
    for b, s in enumerate(STREAMS):
        for size in (1, 5, 64, 1026):
            alone = _native.gaussian_noise(1, size, SEED, torch.tensor([s], device=DEV))
            assert same_bits(alone.cpu(), full[b:b + 1, :size].cpu()), (s, size)
    turned = _native.gaussian_noise(5, 300, SEED, [STREAMS[2], 9, STREAMS[0], STREAMS[1], STREAMS[0]], device=DEV)
    assert same_bits(turned[[2, 3, 0]].cpu(), full[:, :300].cpu()) and torch.equal(turned[2], turned[4])
    out = torch.full((3, 1027), 7.0, device=DEV)
    assert _native.gaussian_noise(3, 1027, SEED, list(STREAMS), out=out) is out and same_bits(out.cpu(), full.cpu())
    assert _native.gaussian_noise(0, 8, SEED, torch.empty(0, dtype=torch.int64), device=DEV).shape == (0, 8)


def test_moments_over_2_20_values():
    z = _native.gaussian_noise(4, 1 << 18, 12345, [3, 4, 5, 6], device=DEV).double()
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"2^20 normals: mean {mean:+.5f}, var {var:.5f}, max |z| {float(z.abs().max()):.3f}")
    assert abs(mean) <= 0.005 and abs(var - 1.0) <= 0.007                   # 5 sigma: 5 / 1024 and 5 sqrt(2) / 1024
    assert float(z.abs().max()) <= 5.8 and bool(torch.isfinite(z).all())


# ---- background noise, bit for bit ---------------------------------------------------------------------------------------------------

def noise_case(size, k):
    """The k-th kind of noise recording for a clip of ``size`` samples: (length, start, pad mode)."""
    short = max(size - 1 - 3 * k, 1) if size > 1 else 1
    long = 2 * size + 5
    return [(short, 0, ZERO), (short, 0, MIN), (short, 0, REPLICATE), (short, 0, WRAP), (size, 0, ZERO),
            (long, 0, REPLICATE), (long, (size + 5) // 2, REPLICATE), (long, size + 5, REPLICATE), (max(size // 7, 1), 0, WRAP)][k % 9]


def run_noise(dtype, size, lengths, kinds, seed, gain=None, normalize=False, masks=None, gaussian=None, what=""):
    """One launch with a noise plan against the oracle; returns (got, plan pieces) on the CPU."""
    B = len(lengths)
    store, off, ln = pack(lengths, dtype, seed=seed)
    cases = [noise_case(size, k) for k in kinds]
    nstore, noff, nln = pack([c[0] for c in cases], dtype, seed=seed + 1)
    nstart, nmode = torch.tensor([c[1] for c in cases]), torch.tensor([c[2] for c in cases])
    span = (ln - size).clamp(min=0)
    start, mode = span // 2, torch.tensor([(WRAP, MIN, REPLICATE, ZERO, MIN)[b % 5] for b in range(B)])
    coeff = pairs(B, seed)
    zs = None
    if gaussian is not None:
        amp, streams = gaussian
        zs = (amp, _native.gaussian_noise(B, size, SEED, streams, device=DEV).cpu())
    want = assemble_noise_ref(store, off, ln, start, mode, size, gain, masks, peaknorm if normalize else None,
                              noise=(nstore, noff, nln, nstart, nmode, coeff), gaussian=zs)
    got = _native.assemble_clips(store.to(DEV), off, ln, start, mode, size, gain, normalize, masks,
                                 noise=(nstore.to(DEV), noff, nln, nstart, nmode, coeff),
                                 gaussian=None if gaussian is None else (gaussian[0], SEED, gaussian[1]))
    assert got.shape == (B, 1, size) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu()[:, 0]
    assert same_bits(got, want), diff_message(got, want, what)
    return got


@DTYPES
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("size", [1, 63, 65, 1000, 1001, 1002, 1003, 1025, 4100, CUT - 1, CUT, CUT + 1, CUT + 4100])
def test_background_noise_at_every_size(size, B, dtype):
    lengths = [(size + 1, size, max(size - 1, 1), 3 * size + 7, 1)[b] for b in range(B)]
    kinds = [(size + 3 * b) % 9 for b in range(B)]
    run_noise(dtype, size, lengths, kinds, seed=size % 7, what=f"S={size} B={B}")


@DTYPES
@pytest.mark.parametrize("size", [65, 1001])
def test_every_kind_of_noise_recording(size, dtype):
    # shorter than the clip in each pad mode, equal, longer with the start at 0, in the middle and at the end, a few periods of wrap
    kinds = list(range(9))
    assert {noise_case(size, k)[2] for k in kinds[:4]} == {ZERO, MIN, REPLICATE, WRAP}
    assert [noise_case(size, k)[1] for k in (5, 6, 7)] == [0, (size + 5) // 2, size + 5]
    run_noise(dtype, size, [size + 2 * k for k in kinds], kinds, seed=size, normalize=True, gain=torch.linspace(0.5, 4.0, 9),
              what=f"S={size}")


@pytest.mark.parametrize("size", [1001, CUT + 2])
def test_clips_without_a_noise_recording_keep_the_plain_bits(size):
    B = 4
    store, off, ln = pack([size + 3, size, size - 5, size], torch.float32, seed=3)
    store[off[1]: off[1] + size] = -0.0                                      # a row of negative zeros
    nstore, noff, nln = pack([size, 2 * size, 40, size], torch.float32, seed=4)
    nln = torch.tensor([int(nln[0]), 0, 0, -3])                             # rows 1 .. 3 are not mixed (a device-side -3 is clamped to 0)
    start, mode = torch.zeros(B, dtype=torch.int64), torch.tensor([ZERO, ZERO, MIN, WRAP])
    gain, coeff = torch.tensor([1.5, 2.0, 0.5, 3.0]), pairs(B)
    plain = _native.assemble_clips(store.to(DEV), off, ln, start, mode, size, gain, True).cpu()[:, 0]
    noise = (nstore.to(DEV), noff.to(DEV), nln.to(DEV), torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV), coeff)
    got = _native.assemble_clips(store.to(DEV), off, ln, start, mode, size, gain, True, noise=noise).cpu()[:, 0]
    assert same_bits(got[1:], plain[1:]) and not torch.equal(got[0], plain[0])
    assert bool((got[1].view(torch.int32) == -2 ** 31).all())               # -0.0 stays -0.0: no 1 v + 0 n was computed
    want = assemble_noise_ref(store, off, ln, start, mode, size, gain, None, peaknorm,
                              noise=(nstore, noff, nln.clamp(min=0), [0] * B, [ZERO] * B, coeff))
    assert same_bits(got, want), diff_message(got, want, f"S={size}")


# ---- Gaussian noise, bit for bit against the composition on the stream's own values ----------------------------------------------------

@DTYPES
@pytest.mark.parametrize("size", [1001, 4100, CUT, CUT + 2])
def test_gaussian_noise_is_the_composition_on_the_stream(size, dtype):
    B = 5
    store, off, ln = pack([size + 1, size, max(size - 1, 1), 3 * size + 7, 1], dtype, seed=size % 5)
    start, mode = (ln - size).clamp(min=0) // 3, torch.tensor([WRAP, MIN, REPLICATE, ZERO, MIN])
    amp = torch.tensor([0.015, 0.0, 0.3, 0.001, 2.0])
    streams = torch.tensor([5, 6, 2 ** 40, -1, 2 ** 32 + 7])
    gain = torch.tensor([3.0, 0.5, 1.0, 2.5, 4.0])
    masks = torch.tensor([[[size // 3, size // 4 + 1], [size - 2, 5]]] * B, dtype=torch.int32)
    z = _native.gaussian_noise(B, size, SEED, streams, device=DEV).cpu()
    for normalize in (True, False):
        want = assemble_noise_ref(store, off, ln, start, mode, size, gain, masks, peaknorm if normalize else None, gaussian=(amp, z))
        got = _native.assemble_clips(store.to(DEV), off, ln, start, mode, size, gain, normalize, masks, gaussian=(amp, SEED, streams)).cpu()[:, 0]
        assert same_bits(got, want), diff_message(got, want, f"S={size} normalize={normalize}")
        plain = _native.assemble_clips(store.to(DEV), off, ln, start, mode, size, gain, normalize, masks).cpu()[:, 0]
        assert same_bits(got[1], plain[1]) and not torch.equal(got[0], plain[0])            # amplitude 0 leaves the clip alone


@pytest.mark.parametrize("size", [1000, 1001, CUT + 3])
def test_the_stream_does_not_follow_the_alignment_of_out(size):
    B = 3
    store, off, ln = pack([size + 9, size, size - 1], torch.float32, seed=1)
    start, mode = torch.tensor([4, 0, 0]), torch.tensor([ZERO, ZERO, REPLICATE])
    amp, streams = torch.tensor([0.5, 0.25, 1.0]), torch.tensor([11, 12, 13])
    store_d, results = store.to(DEV), []
    for k in range(4):
        buf = torch.full((B * size + 8,), 9.0, device=DEV)
        out = buf[k: k + B * size].view(B, 1, size)
        assert (out.data_ptr() // 4) % 4 == (buf.data_ptr() // 4 + k) % 4
        assert _native.assemble_clips(store_d, off, ln, start, mode, size, None, True, None, out, gaussian=(amp, SEED, streams)) is out
        assert bool((buf[:k] == 9.0).all()) and bool((buf[k + B * size:] == 9.0).all())
        results.append(out.cpu()[:, 0].clone())
    for k in range(1, 4):
        assert same_bits(results[k], results[0]), diff_message(results[k], results[0], f"S={size} out + {k}")
    z = _native.gaussian_noise(B, size, SEED, streams, device=DEV).cpu()
    want = assemble_noise_ref(store, off, ln, start, mode, size, None, None, peaknorm, gaussian=(amp, z))
    assert same_bits(results[0], want), diff_message(results[0], want, f"S={size}")


# ---- everything together -------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("size", [1001, CUT + 2])
def test_noise_gain_gaussian_normalise_and_masks_together(size, dtype):
    B = 6
    masks = torch.tensor([[[size // 3, size // 4 + 1], [size - 2, 5], [-4, 9]]] * B, dtype=torch.int32)
    gain = torch.tensor([3.0, 0.5, 1.0, 2.5, 4.0, 9.0])
    amp, streams = torch.tensor([0.015, 0.0, 0.3, 0.001, 2.0, 0.01]), torch.tensor([1, 2, 3, 2 ** 33, 5, 6])
    out = run_noise(dtype, size, [size + 1, size, size - 1, 3 * size + 7, 1, 2 * size], [1, 6, 3, 4, 7, 8], seed=2, gain=gain,
                    normalize=True, masks=masks, gaussian=(amp, streams), what=f"S={size}")
    assert float(out.abs().max()) <= 1.0                                     # gain 9: without the normalisation the peak is above 2


# ---- a noise plan the library cannot see ---------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("size", [65, 1000, CUT + 2])
def test_a_hostile_noise_plan_on_the_device_is_clamped(size, dtype):
    lib = _native.load()
    B, big = 12, 2 ** 31 - 1
    store, off, ln = pack([size + 9, size, 40] * 4, dtype, seed=6)
    nstore, noffs, nlns = pack([size + 9, 40, 2 * size, 7, size - 1, 300, 1, size], dtype, seed=4)
    N, item = nstore.numel(), nstore.element_size()
    noise_off = torch.tensor([-5, N + 100, int(noffs[2]), N, 2 ** 40, int(noffs[1]), int(noffs[4]), N - 3, -2 ** 62, int(noffs[3]), int(noffs[0]), int(noffs[5])])
    noise_len = torch.tensor([size + 3, 50, big, 10, 5, -3, size - 1, big, 20, 7, size + 9, 300], dtype=torch.int64)
    noise_start = torch.tensor([-7, 0, big, 3, 0, 0, 5, -big, 1, 2, 10 ** 6, -1], dtype=torch.int64)
    noise_mode = torch.tensor([9, 1, 2, 3, -1, 2, 1, 3, 2, -2 ** 31, 0, 4], dtype=torch.int64)
    start, mode = torch.zeros(B, dtype=torch.int64), torch.tensor([ZERO, MIN, REPLICATE] * 4)
    gain, coeff = torch.linspace(0.5, 3.0, B), pairs(B)
    amp, streams = torch.tensor([0.0, 0.5] * 6), torch.arange(B) - 3
    want_plan = clamp_plan(N, noise_off, noise_len, noise_start, noise_mode, size)
    assert int(want_plan[1].min()) == 0 and int(want_plan[1].max()) > size                  # unmixed clips, and crops
    z = _native.gaussian_noise(B, size, SEED, streams, device=DEV).cpu()
    want = assemble_noise_ref(store, off, ln, start, mode, size, gain, None, peaknorm, noise=(nstore, *want_plan, coeff), gaussian=(amp, z))

    store_g, nstore_g = guarded_tensor(store.to(DEV), offset=item), guarded_tensor(nstore.to(DEV), offset=item)
    plan_g = [guarded_tensor(t.to(DEV)) for t in (off, ln.to(torch.int32), start.to(torch.int32), mode.to(torch.int32), gain)]
    noise_g = [guarded_tensor(t.to(DEV)) for t in (noise_off, noise_len.to(torch.int32), noise_start.to(torch.int32), noise_mode.to(torch.int32),
                                                    coeff)]
    gauss_g = [guarded_tensor(t.to(DEV)) for t in (amp, streams)]
    out_g = guarded(4 * B * size, 0xA5, offset=4)
    rc = lib.leaf_assemble_clips_noise_f32(store_g.ptr, store.numel(), _native.FLAG_X_PCM16 if dtype == torch.int16 else 0, B, size,
                                           *(g.ptr for g in plan_g), 1, None, 0, out_g.ptr, nstore_g.ptr, N, *(g.ptr for g in noise_g),
                                           gauss_g[0].ptr, SEED, gauss_g[1].ptr, _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    out_g.check(f"out, S={size}")
    for g in [store_g, nstore_g] + plan_g + noise_g + gauss_g:
        unchanged(g, "a read-only input")
    got = out_g.cpu(torch.float32, (B, size))
    assert same_bits(got, want), diff_message(got, want, f"S={size}")


# ---- no noise through the new entry ----------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("size", [1001, CUT + 2])
def test_without_noise_the_result_is_the_old_entrys(size, dtype):
    lib = _native.load()
    B = 4
    store, off, ln = pack([size + 1, size - 1, 3 * size, 5], dtype, seed=8)
    start, mode = (ln - size).clamp(min=0) // 2, torch.tensor([ZERO, MIN, ZERO, WRAP])
    gain = torch.tensor([1.0, 3.0, 0.5, 2.0])
    masks = torch.tensor([[[10, 50]]] * B, dtype=torch.int32)
    want = assemble_ref(store, off, ln, start, mode, size, gain, masks, peaknorm)
    got = _native.assemble_clips(store.to(DEV), off, ln, start, mode, size, gain, True, masks).cpu()[:, 0]
    assert same_bits(got, want), diff_message(got, want, "no keyword")
    dev = [t.to(DEV) for t in (store, off, ln.to(torch.int32), start.to(torch.int32), mode.to(torch.int32), gain, masks)]
    flags = _native.FLAG_X_PCM16 if dtype == torch.int16 else 0
    head = (dev[0].data_ptr(), store.numel(), flags, B, size, *(t.data_ptr() for t in dev[1:6]), 1, dev[6].data_ptr(), 1)
    old, new = torch.empty((B, size), device=DEV), torch.empty((B, size), device=DEV)
    st = _native.stream_ptr(torch.device(DEV))
    assert lib.leaf_assemble_clips_f32(*head, old.data_ptr(), st) == 0
    assert lib.leaf_assemble_clips_noise_f32(*head, new.data_ptr(), None, 0, None, None, None, None, None, None, 0, None, st) == 0
    torch.cuda.synchronize()
    assert same_bits(new.cpu(), old.cpu()) and same_bits(old.cpu(), want)


# ---- the sampler, end to end -------------------------------------------------------------------------------------------------------------

def test_a_sampler_with_both_noises_feeds_the_frontend():
    g = torch.Generator().manual_seed(21)
    rec = lambda n: torch.randint(-12000, 12000, (n,), generator=g).to(torch.int16)
    clips = PackedClips([rec(n) for n in (16000, 8000, 23456, 15999, 16001, 100)], device=DEV)
    noise = PackedClips([rec(n) for n in (4000, 16000, 50000)], device=DEV)
    index = torch.tensor([5, 0, 1, 4, 2, 3, 3, 0])
    kw = dict(noise_clips=noise, noise_prob=0.6, gaussian_prob=0.6, gain_prob=0.5, time_perc=0.1, num_masks=2, gaussian_seed=77)
    a, b = (ClipSampler(clips, 16000, generator=torch.Generator().manual_seed(8), **kw) for _ in range(2))
    plan = ClipSampler(clips, 16000, generator=torch.Generator().manual_seed(8), **kw).plan(index)
    xa, xb = a(index), b(index)
    assert xa.shape == (8, 1, 16000) and same_bits(xa.cpu(), xb.cpu())       # the same seed gives the same batch
    assert not torch.equal(a(index), xa)                                     # ... and the next call another one
    mixed, noisy = plan.noise[1] > 0, plan.gaussian[0] != 0
    assert bool(mixed.any()) and bool((~mixed).any()) and bool(noisy.any()) and bool((~noisy).any())
    z = _native.gaussian_noise(8, 16000, 77, plan.gaussian[2], device=DEV).cpu()
    want = assemble_noise_ref(clips.store, *plan[:4], 16000, plan.gain, plan.masks, peaknorm,
                              noise=(noise.store, *plan.noise[:4], _native.noise_coefficients(plan.noise[4])), gaussian=(plan.gaussian[0], z))
    assert same_bits(xa.cpu()[:, 0], want), diff_message(xa.cpu()[:, 0], want, "sampler")
    torch.manual_seed(0)
    leaf = Leaf().to(DEV).eval()
    with torch.no_grad():
        y = leaf(xa)
    assert y.shape == (8, 40, 100) and bool(torch.isfinite(y).all())
    # PackedClips.assemble with the same draws, SNRs given in dB
    rows = torch.searchsorted(noise.offsets_host, plan.noise[0], right=True) - 1
    nidx = torch.where(mixed, rows, -1)
    snr = 10 * torch.log10(plan.noise[4] / (1 - plan.noise[4]))
    xc = clips.assemble(index, plan.start, 16000, plan.pad_mode, plan.gain, True, plan.masks,
                        noise=(noise, nidx, plan.noise[2], _native.noise_coefficients(plan.noise[4])), gaussian=plan.gaussian)
    assert same_bits(xc.cpu(), xa.cpu())
    xd = clips.assemble(index, plan.start, 16000, plan.pad_mode, plan.gain, True, plan.masks, noise=(noise, nidx, plan.noise[2], snr))
    assert xd.shape == xa.shape and bool(torch.isfinite(xd).all())
