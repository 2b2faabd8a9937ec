"""Background noise at an SNR and Gaussian noise in the assembly launch, the host side (no GPU): the oracle of the random stream
(Philox4x32-10 in Python integers against its known answers, Box-Muller in float64), ``assemble_noise_ref`` -- ``assemble_ref`` of
tests/test_host_clips.py with the two noise steps in the fp32 order include/leaf_hip.h states -- the two C entries as declared and
exported, their argument checks, the validation of a noise plan that arrives on the CPU, and ClipSampler's noise draws.
tests/test_gpu_clip_noise.py compares the kernels with the oracles defined here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from leaf_pytorch_amd import ClipSampler, PackedClips, _native, transforms
from test_host_clips import MIN, REPLICATE, WRAP, ZERO, assemble_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, ALIGNMENT, UNSUPPORTED = -1, -2, -7, -8
MASK32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


# ---- the oracle of the stream ------------------------------------------------------------------------------------------------------

def philox4x32_10(counter, key):
    """Philox4x32-10 in plain Python integers: four counter words, two key words -> four output words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox_groups(seed: int, stream: int, groups: int) -> np.ndarray:
    """The words of the counters (g, 0, lo32(stream), hi32(stream)), g in [0, groups), under the key (lo32(seed), hi32(seed)):
    (groups, 4) uint64 holding 32-bit values -- the same rounds as ``philox4x32_10``, over numpy arrays."""
    stream &= 2 ** 64 - 1
    u = lambda v: np.full(groups, v, dtype=np.uint64)
    c0, c1, c2, c3 = np.arange(groups, dtype=np.uint64), u(0), u(stream & MASK32), u(stream >> 32)
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    m = np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return np.stack((c0, c1, c2, c3), axis=1)


def gaussian_ref(seed: int, stream: int, size: int) -> np.ndarray:
    """z(seed, stream, t) for t in [0, size) by the definition in include/leaf_hip.h, evaluated in float64 (the integer part is exact,
    u1 and u2 are exact in either precision)."""
    r = philox_groups(seed, stream, (size + 3) // 4)
    z = np.empty((r.shape[0], 4), dtype=np.float64)
    for pair in (0, 1):
        u1 = ((r[:, 2 * pair] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        u2 = (r[:, 2 * pair + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        rho = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * pair], z[:, 2 * pair + 1] = rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)
    return z.reshape(-1)[:size]


def gaussian_ref_f32(seed: int, streams, size: int) -> torch.Tensor:
    """(B, size) float32: the float64 oracle rounded once."""
    return torch.from_numpy(np.stack([gaussian_ref(seed, int(s), size) for s in streams]).astype(np.float32))


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((MASK32,) * 4, (MASK32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert " ".join(f"{w:08x}" for w in philox4x32_10(counter, key)) == want


def test_the_vectorised_rounds_are_the_plain_ones_and_the_counter_layout_is_the_documented_one():
    seed, stream = 0xa4093822_299f31d0, 2 ** 40 + 5
    r = philox_groups(seed, stream, 7)
    for g in (0, 3, 6):
        assert tuple(int(w) for w in r[g]) == philox4x32_10((g, 0, stream & MASK32, stream >> 32), (seed & MASK32, seed >> 32))
    assert tuple(int(w) for w in philox_groups(0, 0, 1)[0]) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    neg = philox_groups(seed, -1, 1)[0]                                     # an int64 stream id goes in as its 64 bits
    assert tuple(int(w) for w in neg) == philox4x32_10((0, 0, MASK32, MASK32), (seed & MASK32, seed >> 32))


def test_box_muller_of_the_oracle():
    z = gaussian_ref(1, 2, 9)
    r = philox4x32_10((1, 0, 2, 0), (1, 0))                                 # row elements 4 .. 7
    u1, u2 = ((r[0] >> 8) + 1) / 2 ** 24, (r[1] >> 8) / 2 ** 24
    assert z[4] == pytest.approx(math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2), abs=1e-15)
    assert z[5] == pytest.approx(math.sqrt(-2 * math.log(u1)) * math.sin(2 * math.pi * u2), abs=1e-15)
    u1, u2 = ((r[2] >> 8) + 1) / 2 ** 24, (r[3] >> 8) / 2 ** 24
    assert z[7] == pytest.approx(math.sqrt(-2 * math.log(u1)) * math.sin(2 * math.pi * u2), abs=1e-15)
    assert np.array_equal(gaussian_ref(1, 2, 1027)[:9], z)                  # a prefix, whatever the size
    big = gaussian_ref(5, 6, 1 << 16)
    assert abs(big.mean()) < 5 / 256 and abs(big.var() - 1) < 5 * math.sqrt(2) / 256 and np.abs(big).max() < 5.8     # 5 sigma at 2^16 draws


# ---- the oracle of the assembly ------------------------------------------------------------------------------------------------------

def assemble_noise_ref(store, rec_off, rec_len, start, pad_mode, size, gain=None, masks=None, normalize_fn=None, noise=None, gaussian=None):
    """``assemble_ref`` with the two noise steps.  ``noise`` = (noise_store, noise_off, noise_len, noise_start, noise_pad_mode,
    coeff (B, 2) float32): rows with noise_len > 0 become fl(fl(c v) + fl(c' n)), n the noise recording through ``assemble_ref``'s
    pad and crop.  ``gaussian`` = (amp (B,) float32, z (B, size) float32): rows with amp != 0 become fl(y + fl(amp z)) behind the
    gain.  torch's CPU float32 ops round every operation on its own: there is no fused multiply-add in them."""
    B = len(rec_off)
    y = assemble_ref(store, rec_off, rec_len, start, pad_mode, size)
    if noise is not None:
        nstore, noff, nlen, nstart, nmode, coeff = noise
        coeff = torch.as_tensor(coeff)
        assert coeff.dtype == torch.float32 and tuple(coeff.shape) == (B, 2)
        n = assemble_ref(nstore, noff, nlen, nstart, nmode, size)
        for b in range(B):
            if int(nlen[b]) > 0:
                y[b] = coeff[b, 0] * y[b] + coeff[b, 1] * n[b]
    if gain is not None:
        y = y * torch.as_tensor(gain, dtype=torch.float32).cpu()[:, None]
    if gaussian is not None:
        amp, z = gaussian
        amp = torch.as_tensor(amp, dtype=torch.float32).cpu()
        for b in range(B):
            if float(amp[b]) != 0.0:
                y[b] = y[b] + amp[b] * z[b].cpu()
    if normalize_fn is not None:
        y = normalize_fn(y).clone()
    if masks is not None:
        masks = torch.as_tensor(masks).cpu()
        for b in range(B):
            for t0, n_ in masks[b].tolist():
                if n_ > 0:
                    y[b, max(t0, 0):max(min(t0 + n_, size), 0)] = 0
    return y


def test_the_mix_is_the_reference_expression_bit_for_bit():
    g = torch.Generator().manual_seed(1)
    x, n = torch.rand(4096, generator=g) * 2 - 1, torch.rand(4096, generator=g) * 2 - 1
    for snr in (10.0, 17.3, 25.99, 0.0, -3.0):
        r = np.exp(snr * np.log(10) / 10)
        coeff = r / (1 + r)
        assert isinstance(coeff, np.float64)
        literal = coeff * x + (1.0 - coeff) * n                             # AddRandomNoise.__call__
        pair = _native.noise_coefficients([float(coeff)])
        assert pair.dtype == torch.float32 and float(pair[0, 0]) == float(np.float32(coeff)) and float(pair[0, 1]) == float(np.float32(1.0 - coeff))
        want = assemble_noise_ref(x, [0], [4096], [0], [ZERO], 4096, noise=(n, [0], [4096], [0], [ZERO], pair))
        assert literal.dtype == torch.float32 and torch.equal(literal.view(torch.int32), want[0].view(torch.int32))
        assert torch.equal(_native.snr_coefficients([snr]), torch.tensor([coeff], dtype=torch.float64))
    # 1 - fp32(coeff) would not do: the complement is rounded from the double
    c = 1 / 3
    assert float(_native.noise_coefficients([c])[0, 1]) == float(np.float32(1.0 - c)) != float(np.float32(1.0) - np.float32(c))


def test_the_oracle_orders_the_steps_and_skips_what_is_off():
    store, nstore = torch.tensor([0.5, -0.0, 0.25, 1.0]), torch.tensor([1.0, 1.0, 1.0, 1.0, 3.0])
    pair = torch.tensor([[0.5, 0.5], [0.5, 0.5]])
    z = torch.tensor([[1.0, 1.0, -1.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    got = assemble_noise_ref(store, [0, 0], [4, 4], [0, 0], [ZERO, ZERO], 4, gain=[2.0, 2.0], masks=[[[3, 1]], [[0, 0]]],
                             noise=(nstore, [0, 0], [5, 0], [1, 0], [ZERO, ZERO], pair), gaussian=([0.5, 0.0], z))
    # row 0: (0.5 v + 0.5 n) 2 + 0.5 z with n = (1, 1, 1, 3), the last sample masked; row 1: neither noise, -0.0 keeps its sign
    assert got[0].tolist() == [2.0, 1.5, 0.75, 0.0] and got[1].tolist() == [1.0, -0.0, 0.5, 2.0]
    assert math.copysign(1.0, float(got[1, 1])) == -1.0
    peak = assemble_noise_ref(store, [0], [4], [0], [ZERO], 4, gain=[1.0], normalize_fn=lambda y: y / y.abs().amax(1, keepdim=True),
                              gaussian=([1.0], torch.tensor([[3.5, 0.0, 0.0, 0.0]])))
    assert peak[0].tolist() == [1.0, -0.0, 0.0625, 0.25]                    # the peak is taken behind the Gaussian noise


# ---- the C entries -----------------------------------------------------------------------------------------------------------------

def test_the_entries_are_declared_as_exported():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", header))
    flat = re.sub(r"\s+", " ", flat)
    assert ("int leaf_assemble_clips_noise_f32(const void* store, long long store_len, int flags, int B, int size, const long long* rec_off, "
            "const int* rec_len, const int* start, const int* pad_mode, const float* gain, int normalize, const int* masks, int M, "
            "float* out, const void* noise_store, long long noise_store_len, const long long* noise_off, const int* noise_len, "
            "const int* noise_start, const int* noise_pad_mode, const float* noise_coeff , const float* gauss_amp, "
            "unsigned long long gauss_seed, const long long* gauss_stream, void* stream);") in flat
    assert "int leaf_gaussian_noise_f32(int B, int size, unsigned long long seed, const long long* stream_ids , float* out , void* stream);" in flat
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6          # additive: the version stays
    i, v, ll, ull = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong
    old = _native._SIGNATURES["leaf_assemble_clips_f32"]
    assert old == (i, [v, ll, i, i, i, v, v, v, v, v, i, v, i, v, v])                      # the old entry keeps its signature
    assert _native._SIGNATURES["leaf_assemble_clips_noise_f32"] == (i, old[1][:-1] + [v, ll, v, v, v, v, v, v, ull, v, v])
    assert _native._SIGNATURES["leaf_gaussian_noise_f32"] == (i, [i, i, ull, v, v, v])
    lib = _native.load()
    for name in ("leaf_assemble_clips_noise_f32", "leaf_gaussian_noise_f32"):
        assert name in _native.EXPORTED_SYMBOLS and name in open(os.path.join(REPO, "INTEGRATION.md")).read()
        fn = getattr(lib, name)
        assert fn.restype == i and fn.argtypes == _native._SIGNATURES[name][1]
    assert lib.leaf_abi_version() == 6 and _native.ABI_VERSION == 6
    # the cut-over of the noise instances, on the three sides that state it
    src = open(os.path.join(REPO, "leaf_pytorch_amd", "csrc", "leaf_clips.hpp")).read()
    chunks = int(re.search(r"constexpr int kClipNoiseChunks = (\d+);", src).group(1))
    assert "kClipNoiseResidentMax = kClipNoiseChunks * 4 * kClipThreads - 3" in src
    assert _native.ASSEMBLE_NOISE_RESIDENT_MAX == chunks * 4 * 1024 - 3 and str(_native.ASSEMBLE_NOISE_RESIDENT_MAX) in header


def test_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000                                        # never dereferenced: every call below is refused before the launch

    def call(store=p, store_len=100, flags=0, B=2, size=8, rec_off=p, rec_len=p, start=p, pad_mode=p, gain=None, normalize=1, masks=None,
             M=0, out=p, noise_store=p, noise_store_len=50, noise_off=p, noise_len=p, noise_start=p, noise_pad_mode=p, noise_coeff=p,
             gauss_amp=p, gauss_seed=7, gauss_stream=p):
        return lib.leaf_assemble_clips_noise_f32(store, store_len, flags, B, size, rec_off, rec_len, start, pad_mode, gain, normalize, masks, M,
                                                 out, noise_store, noise_store_len, noise_off, noise_len, noise_start, noise_pad_mode,
                                                 noise_coeff, gauss_amp, gauss_seed, gauss_stream, None)

    noise_group = ("noise_store", "noise_off", "noise_len", "noise_start", "noise_pad_mode", "noise_coeff")
    no_noise, no_gauss = {k: None for k in noise_group}, dict(gauss_amp=None, gauss_stream=None)
    for name in ("store", "rec_off", "rec_len", "start", "pad_mode", "out") + noise_group + ("gauss_amp", "gauss_stream"):
        assert call(**{name: None}) == NULL_POINTER, name                                  # a group given in part is refused
    assert call(store=None, **no_noise) == NULL_POINTER and call(out=None, **no_gauss) == NULL_POINTER
    assert call(store=None, **no_noise, **no_gauss) == NULL_POINTER                         # both groups NULL: the old entry answers
    for kw in (dict(B=0), dict(B=-1), dict(size=0), dict(store_len=-1), dict(M=-1), dict(M=2, masks=None), dict(noise_store_len=-1)):
        assert call(**kw) == BAD_SHAPE, kw
    assert call(B=0, **no_noise, **no_gauss) == BAD_SHAPE
    assert call(flags=_native.FLAG_IO_BF16) == UNSUPPORTED and call(flags=_native.FLAG_X_PCM16 | _native.FLAG_PCEN) == UNSUPPORTED
    assert call(flags=_native.FLAG_IO_BF16, store=None) == UNSUPPORTED and call(store=None, B=0) == NULL_POINTER      # the order
    assert call(B=0, out=p + 2) == BAD_SHAPE
    for name in ("store", "rec_len", "start", "pad_mode", "out", "gain", "noise_store", "noise_len", "noise_start", "noise_pad_mode",
                 "noise_coeff", "gauss_amp"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    for name in ("rec_off", "noise_off", "gauss_stream"):
        assert call(**{name: p + 4}) == ALIGNMENT, name
    assert call(masks=p + 1, M=1) == ALIGNMENT
    assert call(noise_store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT and call(store=p + 1, flags=_native.FLAG_X_PCM16) == ALIGNMENT

    def gauss(B=2, size=8, seed=1, stream=p, out=p):
        return lib.leaf_gaussian_noise_f32(B, size, seed, stream, out, None)

    assert gauss(stream=None) == NULL_POINTER and gauss(out=None) == NULL_POINTER
    assert gauss(B=0) == BAD_SHAPE and gauss(size=0) == BAD_SHAPE and gauss(B=-3) == BAD_SHAPE and gauss(B=0, out=None) == NULL_POINTER
    assert gauss(B=2 ** 31 - 1, size=2 ** 31 - 1) == BAD_SHAPE                             # more workgroups than a launch takes
    assert gauss(stream=p + 4) == ALIGNMENT and gauss(out=p + 2) == ALIGNMENT


# ---- the Python layer: a noise plan on the CPU is validated before anything is launched ---------------------------------------------

STORE = torch.zeros(100, dtype=torch.int16)            # CPU stores: a valid plan gets as far as require_hip and no further
NOISE = torch.zeros(60, dtype=torch.int16)


def _assemble(noise_off=(0, 10), noise_len=(10, 40), noise_start=(0, 5), noise_pad_mode=(2, 2), coeff=(0.9, 0.99), nstore=NOISE, gaussian=None,
              with_noise=True, size=16):
    noise = (nstore, list(noise_off), list(noise_len), list(noise_start), list(noise_pad_mode), coeff) if with_noise else None
    return _native.assemble_clips(STORE, [0, 10], [10, 40], [0, 5], [1, 2], size, noise=noise, gaussian=gaussian)


def test_a_valid_noise_plan_reaches_the_device_check():
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _assemble()
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _assemble(noise_len=(0, 0), gaussian=(torch.zeros(2), 2 ** 64 - 1, [0, 1]))
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _assemble(coeff=torch.tensor([[0.5, 0.5], [1.0, 0.0]]), noise_off=(60, 0), noise_len=(0, 60))
    with pytest.raises(RuntimeError, match="AMD GPU"):
        _native.gaussian_noise(2, 8, 1, [0, 1], device="cpu")


@pytest.mark.parametrize("bad", [
    dict(noise_off=(-1, 10)), dict(noise_off=(0, 61)), dict(noise_len=(-1, 40)), dict(noise_len=(10, 51)), dict(noise_start=(1, 5)),
    dict(noise_start=(0, 25)), dict(noise_start=(-1, 5)), dict(noise_pad_mode=(4, 0)), dict(noise_pad_mode=(0, -1)),
    dict(noise_len=(10,)), dict(noise_off=(0, 10, 20), noise_len=(1, 1, 1), noise_start=(0, 0, 0), noise_pad_mode=(0, 0, 0)),
    dict(coeff=(0.9,)), dict(coeff=(0.9, 1.5)), dict(coeff=(-0.1, 0.5)), dict(coeff=torch.zeros((2, 3))),
    dict(with_noise=False, gaussian=(torch.zeros(3), 1, [0, 1])), dict(with_noise=False, gaussian=(torch.zeros(2), 1, [0, 1, 2])),
    dict(with_noise=False, gaussian=(torch.zeros(2), -1, [0, 1])), dict(with_noise=False, gaussian=(torch.zeros(2), 2 ** 64, [0, 1])),
])
def test_a_bad_cpu_noise_plan_raises_value_error_before_the_store_is_looked_at(bad):
    with pytest.raises(ValueError):
        _assemble(**bad)


def test_a_noise_store_of_another_dtype_raises():
    with pytest.raises(TypeError, match="both int16 PCM or both float32"):
        _assemble(nstore=NOISE.float())
    clips, noise_f32 = PackedClips([STORE[:30], STORE[30:]]), PackedClips([NOISE.float()])
    with pytest.raises(TypeError, match="both int16 PCM or both float32"):
        clips.assemble([0, 1], 0, 16, noise=(noise_f32, [0, 0], 0, 20.0))
    with pytest.raises(TypeError):
        ClipSampler(clips, 16, noise_clips=noise_f32)
    with pytest.raises(TypeError):
        clips.assemble([0, 1], 0, 16, noise=(NOISE, [0, 0], 0, 20.0))       # a tensor is not a PackedClips
    with pytest.raises(TypeError):
        _native.assemble_clips(STORE, [0], [10], [0], [0], 16, gaussian=(torch.zeros(1), 1, [0.5]))
    noise = PackedClips([NOISE[:20], NOISE[20:]])
    with pytest.raises(ValueError, match="outside"):
        clips.assemble([0, 1], 0, 16, noise=(noise, [0, 2], 0, 20.0))
    with pytest.raises(ValueError):
        clips.assemble([0, 1], 0, 16, noise=(noise, [0], 0, 20.0))
    with pytest.raises(ValueError):
        clips.assemble([0, 1], 0, 16, noise=(noise, [0, 1], [0, 25], 20.0))  # a start behind max(Ln, S) - S
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):       # SNRs in dB, a clip without noise (-1), pairs
        clips.assemble([0, 1], 0, 16, noise=(noise, [1, -1], [24, 0], [10.0, 25.0], "wrap"))
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        clips.assemble([0, 1], 0, 16, noise=(noise, [1, 0], 0, torch.tensor([[0.5, 0.5], [0.9, 0.1]])), gaussian=([0.1, 0.0], 3, [5, 6]))


# ---- ClipSampler -----------------------------------------------------------------------------------------------------------------

LENGTHS = (5, 16, 16, 40, 100, 1, 17)
NOISE_LENGTHS = (7, 16, 50, 300)
S = 16


def _packed(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return PackedClips([torch.randint(-20000, 20000, (n,), dtype=torch.int16, generator=g) for n in lengths])


def _sampler(seed=11, noise=True, **kw):
    return ClipSampler(_packed(LENGTHS, 3), S, generator=torch.Generator().manual_seed(seed),
                       noise_clips=_packed(NOISE_LENGTHS, 4) if noise else None, **kw)


INDEX = torch.arange(len(LENGTHS)).repeat(40)
MANY = torch.arange(4000) % len(LENGTHS)


def _same(a, b):
    return all((x is None and y is None) or (isinstance(x, int) and x == y) or (isinstance(x, torch.Tensor) and x.dtype == y.dtype and torch.equal(x, y))
               for x, y in zip(a, b)) and len(a) == len(b)


def test_the_same_seed_gives_the_same_plan():
    kw = dict(num_masks=2, time_perc=0.5, gaussian_prob=0.5)
    a, b, c = _sampler(11, **kw).plan(INDEX), _sampler(11, **kw).plan(INDEX), _sampler(12, **kw).plan(INDEX)
    assert isinstance(a, transforms.ClipNoisePlan) and isinstance(a, transforms.ClipPlan) and len(a) == 6
    rec_off, rec_len, start, pad_mode, gain, masks = a                       # it unpacks as before
    assert a.rec_off is rec_off and a.masks is masks
    assert _same(a, b) and _same(a.noise, b.noise) and _same(a.gaussian, b.gaussian)
    assert not _same(a.noise, c.noise) and not torch.equal(a.gaussian[0], c.gaussian[0])
    noff, nlen, nstart, nmode, coeff = a.noise
    assert (noff.dtype, nlen.dtype, nstart.dtype, nmode.dtype, coeff.dtype) == (torch.int64, torch.int32, torch.int32, torch.int32, torch.float64)
    amp, seed, stream = a.gaussian
    assert amp.dtype == torch.float32 and stream.dtype == torch.int64 and seed == 11      # default: the generator's initial seed
    assert _sampler(11, gaussian_prob=0.5, gaussian_seed=2 ** 63 + 1).plan(INDEX).gaussian[1] == 2 ** 63 + 1


def test_without_noise_the_plan_is_what_it_was():
    kw = dict(num_masks=3, time_perc=0.5, gain_prob=0.5)
    plain = _sampler(11, noise=False, **kw)
    p1, p2 = plain.plan(INDEX), plain.plan(INDEX)
    assert type(p1) is transforms.ClipPlan
    # the draws of the sampler as it was before the noise arguments existed, recorded from it for this seed (two calls)
    digest = lambda p: (int(p.start.sum()), int(p.masks.sum()), int(p.gain.view(torch.int32).long().sum()))
    assert p1.start[:12].tolist() == [0, 0, 0, 5, 52, 0, 1, 0, 0, 0, 16, 73] and p1.pad_mode[:8].tolist() == [2, 1, 1, 1, 1, 2, 2, 2]
    assert p1.gain[:4].view(torch.int32).tolist() == [1049376966, 1065353216, 1072438940, 1065353216]
    assert p1.masks[:2].tolist() == [[[5, 0], [9, 1], [12, 0]], [[8, 5], [10, 0], [12, 0]]]
    assert digest(p1) == (2178, 7501, 297195157432) and digest(p2) == (2370, 7441, 296920143959)
    old = ClipSampler(_packed(LENGTHS, 3), S, True, ("replicate", "min"), 0.5, 0.5, (-18.0, 6.0), True, 0.5, 3, torch.Generator().manual_seed(11))
    assert _same(p1, old.plan(INDEX))                                        # the old positional signature still means what it meant
    # ... and with noise on the first six entries are the same draws: the new ones come after all the existing ones
    noisy = _sampler(11, gaussian_prob=0.7, **kw)
    n1, n2 = noisy.plan(INDEX), noisy.plan(INDEX)
    assert _same(tuple(n1), tuple(p1)) and not _same(tuple(n2), tuple(p2))   # (the second call starts behind the noise draws)
    off = _sampler(11, noise=False, gaussian_prob=0.0, noise_prob=0.9, **kw)
    assert _same(off.plan(INDEX), p1) and _same(off.plan(INDEX), p2) and off.next_stream == 0


def test_noise_frequencies_are_binomial():
    n = MANY.numel()
    for p_noise, p_gauss in ((0.5, 0.5), (0.2, 0.9)):
        plan = _sampler(5, noise_prob=p_noise, gaussian_prob=p_gauss).plan(MANY)
        for got, p in ((int((plan.noise[1] > 0).sum()), p_noise), (int((plan.gaussian[0] != 0).sum()), p_gauss)):
            assert abs(got - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (got, p)
    assert int((_sampler(5, noise_prob=0.0).plan(MANY).noise[1] > 0).sum()) == 0
    assert int((_sampler(5, noise_prob=1.0).plan(MANY).noise[1] > 0).sum()) == n
    assert _sampler(5, noise_prob=1.0).plan(MANY).gaussian is None and _sampler(5, noise=False, gaussian_prob=1.0).plan(MANY).noise is None


def test_noise_draws_are_in_range():
    s = _sampler(7, noise_prob=1.0, gaussian_prob=1.0, snr_range=(10, 25), gaussian_amplitude=(0.001, 0.015))
    plan = s.plan(MANY)
    noff, nlen, nstart, nmode, coeff = plan.noise
    nc = s.noise_clips
    rec = torch.searchsorted(nc.offsets_host, noff, right=True) - 1
    assert torch.equal(nc.offsets_host[rec], noff) and torch.equal(nc.lengths_host[rec], nlen)
    assert set(rec.tolist()) == set(range(len(NOISE_LENGTHS)))               # every recording is chosen
    span = (nlen.long() - S).clamp(min=0)
    assert bool((nstart >= 0).all()) and bool((nstart.long() <= span).all())
    assert int(nstart[nlen == 300].min()) == 0 and int(nstart[nlen == 300].max()) == 284   # inclusive at both ends (1000 draws over 285 values)
    assert set(nmode.tolist()) == {REPLICATE}
    lo, hi = (_native.snr_coefficients([v]) for v in (10.0, 26.0))           # snr = uniform(lo, hi + 1)
    assert bool((coeff >= lo).all()) and bool((coeff <= hi).all()) and float(coeff.max()) > float(_native.snr_coefficients([25.0]))
    snr = 10 * torch.log10(coeff / (1 - coeff))
    assert abs(float(snr.mean()) - 18.0) < 5 * 16 / math.sqrt(12 * 4000)      # uniform over [10, 26): 5 sigma of the mean
    amp = plan.gaussian[0]
    assert float(amp.min()) >= 0.001 and float(amp.max()) <= 0.015 and amp.unique().numel() > 3000
    _native.noise_plan(nc.store.numel(), *plan.noise, S, MANY.numel())       # what the sampler draws passes the CPU validation


def test_streams_are_distinct_across_calls():
    s = _sampler(3, gaussian_prob=0.5)
    a, b, c = s.plan(INDEX).gaussian[2], s.plan(INDEX[:5]).gaussian[2], s.plan(INDEX).gaussian[2]
    ids = torch.cat((a, b, c))
    assert ids.unique().numel() == ids.numel() == 2 * INDEX.numel() + 5
    assert a.tolist() == list(range(INDEX.numel())) and int(c[0]) == INDEX.numel() + 5 and s.next_stream == ids.numel()
