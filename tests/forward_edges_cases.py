"""Cases of tests/test_gpu_forward_edges.py and tests/test_host_forward_edges.py: the forward families, their clip-length lattices and
the seeded draws.  Plain module: no fixtures, nothing of the product imported (the host test runs it without a GPU).

A GROUP is one (family of the table, geometry, batch shape); a CASE is a group at one (T, pcen).  The lattice of a group is the one of
tests/test_gpu_backward_edges.py, restated,

    T in {1, 2, 3, h-1, h, h+1, padL, padL+1, K-1, K, K+1, L-1, L, L+1, 2L, 2L+1}      (h the hop, padL = K/2 + K%2 - 1, L the block length)

plus one longer clip, 5L + 3 (several block seams at different frame phases), plus the group's extras.  PCEN alternates on / off over
the sorted lattice; T = L + 1 and 2L + 1 also run with the other setting.

Block lengths are restated here from the formulas of csrc/leaf_fft.hpp (fft_block_len) and csrc/leaf_kernels.hip (make_fft4k_plan);
the host test holds the literal L of every group to them, the GPU test to the plan the library reports."""
import math
from collections import namedtuple

import torch

from oracle import leaf_oracle as lo

FFT_N, FFT4K_N = 2048, 4096
MAX_B, MAX_F = 6, 10
STATIC = ((401, 160), (801, 320), (201, 80))                    # leaf_fft.hpp, fft_static_geometry


def pad_left(K):
    return K // 2 + K % 2 - 1


def fft_block_len(K, hop, static):
    """leaf_fft.hpp: valid outputs per 2048-sample block -- whole 64-sample rows; a static instance also starts every block on a frame."""
    unit = 64 // math.gcd(64, hop) * hop if static else 64
    return (FFT_N - K + 1) // unit * unit


def fft4k_block_len(K, hop):
    """leaf_kernels.hip, make_fft4k_plan: 3200 for the static 801 / 320 instance, else the even number of valid outputs (odd K, 833 .. 2049)."""
    if (K, hop) == (801, 320):
        return 3200
    assert K % 2 == 1 and 833 <= K <= 2049, K
    return (FFT4K_N - K + 1) & ~1


def ragged(K):
    """What 2048 - K + 1 valid outputs would cut, had the plan not rounded them down to whole rows: clip ends the rounding moves."""
    v = FFT_N - K + 1
    return (v - 1, v, v + 1, 2 * v + 1)


def lattice(K, hop, L, extra=()):
    padL = pad_left(K)
    return sorted({1, 2, 3, hop - 1, hop, hop + 1, padL, padL + 1, K - 1, K, K + 1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 5 * L + 3} | set(extra))


def reduced_lattice(K, hop, L):
    return sorted({1, hop, pad_left(K) + 1, K, L + 1, 2 * L + 1})


def lattice_cases(ts, L):
    """[(T, pcen)]: PCEN alternates over the sorted lattice; L + 1 and 2L + 1 run with the other setting too."""
    out = [(t, i % 2 == 0) for i, t in enumerate(sorted(ts))]
    return out + [(t, not p) for t, p in out if t in (L + 1, 2 * L + 1)]


def seam_subset(L):
    """The clip lengths the dealings (b), (c) and the streaming finalize of the workgroup kernels run."""
    return (L - 1, L, L + 1, 2 * L, 2 * L + 1, 5 * L + 3)


def train_subset(hop, L):
    return (1, hop, hop + 1, L - 1, L, L + 1, 2 * L + 1)


def kinds_subset(hop, L):
    return (1, hop, L - 1, L, L + 1, 2 * L + 1)


BAND_LPHI_16 = 12 * (128 // 16)                                 # leaf_band.hpp: band_lphi(16) = kBandLh * band_d(16)
# the first T with one regular (shift-invariant) band frame at 401 / 160 (tests/test_gpu_backward_edges.py, FIRST_REGULAR_T)
FIRST_REGULAR_T = -(-(200 + BAND_LPHI_16) // 160) * 160 + 401 + BAND_LPHI_16 - 200

# family: the row of the table; selector: the name of the _native.ALGO_* constant; L: the block length, a literal (the host test holds
# it to the formulas above); band: the default bank's slice (band tasks) in place of drawn (mu, sigma); shape: the small-batch form
Group = namedtuple("Group", "family name selector K hop L F B seed extra band reduced shape")


def _g(family, name, selector, K, hop, L, F, B, seed, extra=(), band=False, reduced=False, shape=None):
    return Group(family, name, selector, K, hop, L, F, B, seed, tuple(extra), band, reduced, shape)


GROUPS = [
    # 1. per-wave kernel, static instances (801 / 320 on 2048-sample blocks: the plan leaf_forward_prepared keeps)
    _g(1, "1-per-wave-16k", "ALGO_FFT", 401, 160, 1600, 5, 3, 3101),
    _g(1, "1-per-wave-32k-on-2048", "ALGO_FFT", 801, 320, 960, 4, 3, 3102),
    # 2. per-wave kernel, generic instances: odd, even, three slots (K - 1 > L)
    _g(2, "2-per-wave-K601", "ALGO_FFT", 601, 240, 1408, 4, 3, 3201, ragged(601)),
    _g(2, "2-per-wave-K552", "ALGO_FFT", 552, 220, 1472, 4, 3, 3202, ragged(552)),
    _g(2, "2-per-wave-K1216-three-slots", "ALGO_FFT", 1216, 300, 832, 4, 3, 3203, ragged(1216)),
    # 3 .. 5. workgroup kernels, static instances
    _g(3, "3-workgroup-16k", "ALGO_FFT_WG", 401, 160, 1600, 10, 5, 3301, (FIRST_REGULAR_T - 1, FIRST_REGULAR_T), band=True),
    _g(4, "4-workgroup-8k", "ALGO_FFT_WG", 201, 80, 1600, 5, 5, 3401),
    _g(5, "5-workgroup-32k-on-4096", "ALGO_FFT_WG", 801, 320, 3200, 10, 5, 3501, (959, 960, 961, 1920, 1921), band=True),
    # 6. workgroup kernel, run-time geometry on 2048-sample blocks: <= 10 taps per lane (full transposition scratch), 19 (half, three slots)
    _g(6, "6-workgroup-runtime-K552", "ALGO_FFT_WG", 552, 220, 1472, 4, 5, 3601, ragged(552)),
    _g(6, "6-workgroup-runtime-K601", "ALGO_FFT_WG", 601, 240, 1408, 4, 5, 3602, ragged(601)),
    _g(6, "6-workgroup-runtime-K1216-three-slots", "ALGO_FFT_WG", 1216, 300, 832, 4, 5, 3603, ragged(1216)),
    # 7. workgroup kernel, run-time geometry on 4096-sample blocks
    _g(7, "7-workgroup-runtime-4096-K833", "ALGO_FFT_WG", 833, 333, 3264, 3, 5, 3701),
    _g(7, "7-workgroup-runtime-4096-K2049", "ALGO_FFT_WG", 2049, 800, 2048, 3, 5, 3702),
    # 8. one-launch small-batch kernel: SPLIT (2 B F <= CUs) and one workgroup per pair (CUs / 2 < B F <= 2 CUs, the call's CUs)
    _g(8, "8-small-16k-split", "ALGO_FFT_SMALL", 401, 160, 1600, 10, 2, 3801, shape="split"),
    _g(8, "8-small-16k-pair", "ALGO_FFT_SMALL", 401, 160, 1600, 10, 3, 3802, shape="pair"),
    _g(8, "8-small-8k-split", "ALGO_FFT_SMALL", 201, 80, 1600, 10, 2, 3803, shape="split"),
    _g(8, "8-small-8k-pair", "ALGO_FFT_SMALL", 201, 80, 1600, 10, 3, 3804, shape="pair"),
    # 9. MFMA: the three overlap instances and the even window (no block length of its own: 2048 - K + 1 places the long clips)
    _g(9, "9-mfma-K31-noff1", "ALGO_MFMA", 31, 50, 2018, 8, 3, 3901, (99, 100, 101)),
    _g(9, "9-mfma-K64-even-noff1", "ALGO_MFMA", 64, 64, 1985, 8, 3, 3902, (127, 128, 129)),
    _g(9, "9-mfma-K101-noff3", "ALGO_MFMA", 101, 40, 1948, 8, 3, 3903, (79, 80, 81)),
    _g(9, "9-mfma-K201-noff6", "ALGO_MFMA", 201, 40, 1848, 8, 3, 3904, (79, 80, 81)),
    # 10. staged, on the reduced lattice
    _g(10, "10-staged-K31", "ALGO_STAGED", 31, 50, 2018, 4, 2, 4001, reduced=True),
    _g(10, "10-staged-K552", "ALGO_STAGED", 552, 220, 1497, 4, 2, 4002, reduced=True),
]
FAMILIES = tuple(range(1, 11))
SMALL_CUS = 40                   # the CUs a "pair" call of family 8 may use (the rest reserved): 2 B F = 60 > 40 >= B F = 30 > 40 / 2


def expected_block_len(g):
    """The formula behind a group's literal L."""
    if g.family in (5, 7):
        return fft4k_block_len(g.K, g.hop)
    if g.family in (9, 10):
        return FFT_N - g.K + 1
    if g.family == 8:
        return fft_block_len(g.K, g.hop, True)
    return fft_block_len(g.K, g.hop, (g.K, g.hop) in STATIC)


def group_lattice(g):
    return reduced_lattice(g.K, g.hop, g.L) if g.reduced else lattice(g.K, g.hop, g.L, g.extra)


def group_cases(g):
    return lattice_cases(group_lattice(g), g.L)


def all_cases():
    return [(g, T, pcen) for g in GROUPS for T, pcen in group_cases(g)]


def case_id(T, pcen):
    return f"T{T}-{'pcen' if pcen else 'off'}"


def band_kernel(g):
    """Every fourth (eighth) member of the default 16 kHz (32 kHz) bank: narrow-band filters kept, so band classes other than the
    full transform occur (as default_every_fourth() of tests/test_gpu_backward_edges.py)."""
    if (g.K, g.hop) == (401, 160):
        return lo.default_params(lo.geometry())["_complex_conv._kernel"][::4].clone()
    assert (g.K, g.hop) == (801, 320)
    return lo.default_params(lo.geometry(80, 32000))["_complex_conv._kernel"][::8].clone()


def draw(g, T, pcen):
    """(geometry, parameters, clips): the parameters first, so that those of a (group, seed) do not depend on T; mu in [0.1, pi - 0.1],
    sigma in [3, 3 + K / 4], every other tensor within +- 10 % of its default; the band groups keep their slice of the default bank.
    Clips are 2 rand - 1: |x| <= 1."""
    gen = torch.Generator().manual_seed(g.seed)
    F, K = g.F, g.K
    geo = lo.LeafGeometry(F, 0, K, g.hop, *lo.same_padding(K))
    mu, sigma = 0.1 + torch.rand(F, generator=gen) * (math.pi - 0.2), 3.0 + torch.rand(F, generator=gen) * K / 4
    kernel = band_kernel(g) if g.band else torch.stack([mu, sigma], dim=1)
    assert kernel.shape == (F, 2)
    params = lo.default_params(geo, pcen, kernel=kernel)
    params = {k: (v * (1 + 0.1 * (2 * torch.rand(v.shape, generator=gen) - 1)) if k != "_complex_conv._kernel" else v) for k, v in params.items()}
    x = 2 * torch.rand(g.B, 1, T, generator=torch.Generator().manual_seed(g.seed * 100003 + T)) - 1
    return geo, params, x


def oracle(x, params, geo, pcen, dtype=torch.float64, stages=False):
    """The reference of every case: lo.leaf_forward on the widened inputs; with `stages` also the pooled tensor before its floor."""
    p = {k: v.to(dtype) for k, v in params.items()}
    if not stages:
        return lo.leaf_forward(x.to(dtype), p, geo, pcen, dtype)
    out, st = lo.leaf_forward(x.to(dtype), p, geo, pcen, dtype, True)
    return out, lo.gaussian_pool(st["energy"], st["lowpass"], p["_pooling._bias"], geo.hop)


# ---- the small-batch kernel's workspace, restated (leaf_kernels.hip: make_small_plan, forward_workspace_bytes)
SMALL_SPLIT_MAX_BLOCKS = 2 * (7 - 1 - 1)                        # 2 * (kSmallSplitRing - 1), kSmallSplitRing = kSmallSplitWaves - 1 = 6


def small_is_split(B, F, T, L, cus):
    nblk = -(-T // L)
    return 2 * B * F <= cus and 2 <= nblk <= SMALL_SPLIT_MAX_BLOCKS


def small_workspace_bytes(B, F, split):
    """The per-clip scales, and for SPLIT `carry_floats`: the seam's (ticket, value) pairs, [B][F] x 4 floats in whole 64-float rows."""
    up = lambda n: -(-n // 64) * 64
    return 4 * (up(B) + (up(4 * B * F) if split else 0))
