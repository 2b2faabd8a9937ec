"""The cases of tests/test_gpu_forward_edges.py, checked without a GPU (tests/forward_edges_cases.py).

* Conditioning: at every (group, T, pcen) the float32 oracle lies within 5e-6 of the fp64 oracle -- a quarter of the GPU test's
  REL_TOL = 2e-5 -- so that the GPU bound judges the kernel and not the case.  A seed that misses is replaced; the cap stays.
* Sensitivity: the oracle with one sample read past a clip end, and with one sample's energy lost at the first block seam, leaves
  REL_TOL at the cases' own draws (measured: 3.4e-3 .. 7.5e-2 and 1.6e-4 .. 2.9e-2): the GPU bound sees defects of that size.
* The lattice of every group holds every listed member, the extras of its row of the table included.
* The literal block lengths equal the formulas of fft_block_len (csrc/leaf_fft.hpp) and make_fft4k_plan (csrc/leaf_kernels.hip),
  restated in the cases module.
* The case count stays below 900 and no case is larger than B = 6, F = 10, T = 5L + 3."""
import pytest
import torch

import forward_edges_cases as fe
from conftest import rel_err

CONDITIONING = 5e-6
GPU_REL_TOL = 2e-5                # tests/test_gpu_forward_edges.py REL_TOL


@pytest.mark.parametrize("g", fe.GROUPS, ids=[g.name for g in fe.GROUPS])
def test_cases_are_well_conditioned(g):
    worst = (0.0, None)
    for T, pcen in fe.group_cases(g):
        geo, params, x = fe.draw(g, T, pcen)
        assert float(x.abs().max()) <= 1.0
        e = rel_err(fe.oracle(x, params, geo, pcen, torch.float32), fe.oracle(x, params, geo, pcen))
        worst = max(worst, (e, fe.case_id(T, pcen)))
        assert e < CONDITIONING, f"{g.name} {fe.case_id(T, pcen)}: float32 oracle {e:.3e} from the fp64 oracle (cap {CONDITIONING:.0e})"
    print(f"{g.name}: {len(fe.group_cases(g))} cases, float32 oracle within {worst[0]:.2e} of fp64 (at {worst[1]})")


def test_the_gpu_bound_rejects_a_sample_past_the_clip_end_and_a_sample_lost_at_a_seam():
    """What the GPU file is for, shown on the oracle itself: a forward that reads ONE sample past a clip end (here: a sample of 0.5 where
    the padding's zero belongs), and one that loses ONE sample's energy at the first block seam (n = L), both leave REL_TOL = 2e-5 by
    more than a factor of two at the cases' own draws -- at every geometry of the table, PCEN on and off.  (The seam: families 1 - 8,
    whose plans cut blocks.  Not at 31 / 50: with K < hop some samples lie in no frame's window, and no output depends on them.)"""
    from oracle import leaf_oracle as lo
    seen = set()
    for g in fe.GROUPS:
        if (g.K, g.hop, g.L) in seen or g.K < g.hop:
            continue
        seen.add((g.K, g.hop, g.L))
        for T, pcen in ((g.L + 1, True), (2 * g.L + 1, False)):
            geo, params, x = fe.draw(g, T, pcen)
            p = {k: v.double() for k, v in params.items()}
            ref, st = lo.leaf_forward(x.double(), p, geo, pcen, torch.float64, True)
            past = fe.oracle(torch.cat([x, torch.full((g.B, 1, 1), 0.5)], dim=-1), params, geo, pcen)[..., :ref.shape[-1]]
            e = st["energy"].clone()
            e[:, :, g.L] = 0.0
            lost = lo.gaussian_pool(e, st["lowpass"], p["_pooling._bias"], geo.hop).clamp_min(lo.FLOOR_POOLED)
            if pcen:
                lost = lo.pcen(lost, p["_compression.alpha"], p["_compression.delta"], p["_compression.root"], p["_compression.ema._weights"])
            a, b = rel_err(past, ref), rel_err(lost, ref)
            print(f"{g.name} T={T} pcen={pcen}: one sample past the end {a:.1e}, one sample lost at the seam {b:.1e}")
            assert a > 2 * GPU_REL_TOL and (b > 2 * GPU_REL_TOL or g.family > 8), (g.name, T, pcen, a, b)


def test_parameters_of_a_group_do_not_depend_on_the_clip_length():
    for g in fe.GROUPS:
        a, b = fe.draw(g, 1, True)[1], fe.draw(g, g.L + 1, True)[1]
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), g.name
        off = fe.draw(g, 7, False)[1]
        assert all(torch.equal(off[k], a[k]) for k in off), g.name           # PCEN off: the same filters and pooling
        k = a["_complex_conv._kernel"]
        if g.band:
            assert torch.equal(k, fe.band_kernel(g))
        else:
            assert 0.1 <= float(k[:, 0].min()) and float(k[:, 0].max()) <= 3.1416 - 0.1
            assert 3.0 <= float(k[:, 1].min()) and float(k[:, 1].max()) <= 3.0 + g.K / 4


def test_lattice_holds_every_listed_member():
    extras = {2: fe.ragged, 6: fe.ragged, 3: lambda K: (616, 617), 5: lambda K: (959, 960, 961, 1920, 1921)}
    assert fe.FIRST_REGULAR_T == 617
    assert fe.ragged(552) == (1496, 1497, 1498, 2995) and fe.ragged(1216) == (832, 833, 834, 1667)
    for g in fe.GROUPS:
        K, h, L, padL = g.K, g.hop, g.L, fe.pad_left(g.K)
        ts = set(fe.group_lattice(g))
        cases = fe.group_cases(g)
        if g.reduced:
            assert g.family == 10 and ts == {1, h, padL + 1, K, L + 1, 2 * L + 1}, g.name
        else:
            want = {1, 2, 3, h - 1, h, h + 1, padL, padL + 1, K - 1, K, K + 1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 5 * L + 3}
            want |= set(extras.get(g.family, lambda K: ())(K))
            if g.family == 9:
                want |= {2 * h - 1, 2 * h, 2 * h + 1}
            assert ts == want, (g.name, sorted(want ^ ts))
            assert set(fe.seam_subset(L)) <= ts and set(fe.train_subset(h, L)) <= ts and set(fe.kinds_subset(h, L)) <= ts
        assert min(ts) == 1 and max(ts) == (2 * L + 1 if g.reduced else 5 * L + 3)
        # PCEN alternates over the sorted lattice; L + 1 and 2L + 1 run both ways
        first = cases[:len(ts)]
        assert [t for t, _ in first] == sorted(ts) and [p for _, p in first] == [i % 2 == 0 for i in range(len(ts))], g.name
        for t in (L + 1, 2 * L + 1):
            assert (t, True) in cases and (t, False) in cases, (g.name, t)
        assert len(cases) == len(ts) + 2 == len(set(cases))


def test_block_lengths_equal_the_plans_formulas():
    by_name = {g.name: g for g in fe.GROUPS}
    for g in fe.GROUPS:
        assert g.L == fe.expected_block_len(g), (g.name, g.L, fe.expected_block_len(g))
    # the figures of the table
    assert fe.fft_block_len(401, 160, True) == 1600 and fe.fft_block_len(201, 80, True) == 1600 and fe.fft_block_len(801, 320, True) == 960
    assert fe.fft_block_len(601, 240, False) == 1408 == (2048 - 601 + 1) // 64 * 64
    assert fe.fft_block_len(552, 220, False) == 1472 and fe.fft_block_len(1216, 300, False) == 832
    assert fe.fft4k_block_len(801, 320) == 3200 and fe.fft4k_block_len(833, 333) == 3264 == (4096 - 833 + 1) & ~1
    assert fe.fft4k_block_len(2049, 800) == 2048
    # three partial slots: a window longer than a block's valid outputs
    assert by_name["6-workgroup-runtime-K1216-three-slots"].K - 1 > 832 and 552 - 1 <= 1472
    # taps per lane of the run-time-geometry workgroup kernel (leaf_kernels.hip: the full transposition scratch up to 10)
    assert -(-552 // 64) <= 10 and -(-601 // 64) <= 10 and -(-1216 // 64) == 19
    # MFMA: frames a hop-block overlaps, (K - 1) / hop + 1, and the instance that serves it (1, 3, 6)
    assert [(g.K - 1) // g.hop + 1 for g in fe.GROUPS if g.family == 9] == [1, 1, 3, 6]


def test_case_count_and_cost():
    cases = fe.all_cases()
    per_family = {f: sum(1 for g, _, _ in cases if g.family == f) for f in fe.FAMILIES}
    print(f"{len(cases)} GPU cases in {len(fe.GROUPS)} groups; per family {per_family}")
    assert all(per_family[f] > 0 for f in fe.FAMILIES)
    assert len(cases) < 900
    for g, T, _ in cases:
        assert g.B <= fe.MAX_B == 6 and g.F <= fe.MAX_F == 10 and T <= 5 * g.L + 3, (g.name, T)
    # the small-batch shapes: SPLIT needs 2 B F workgroups on the device's CUs, the pair form B F between half and twice the call's
    for g in fe.GROUPS:
        if g.shape == "split":
            assert 2 * g.B * g.F <= 64                                       # (any device from 64 CUs)
            assert fe.small_is_split(g.B, g.F, g.L + 1, g.L, 64) and not fe.small_is_split(g.B, g.F, g.L, g.L, 64)
            assert fe.small_is_split(g.B, g.F, 5 * g.L + 3, g.L, 64)
        if g.shape == "pair":
            assert fe.SMALL_CUS / 2 < g.B * g.F <= 2 * fe.SMALL_CUS and not fe.small_is_split(g.B, g.F, g.L + 1, g.L, fe.SMALL_CUS)
    assert fe.small_workspace_bytes(2, 10, True) - fe.small_workspace_bytes(2, 10, False) == 4 * 128
