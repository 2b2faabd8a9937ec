"""The row-owned tail of the static workgroup kernel (csrc/leaf_fft_wg.hpp: wg_tail_rows): after the drain barrier every wave
finalizes the rows it owns end to end -- pooled value, floor, the smoother's recurrence, the point function -- in its own scratch.

Every comparison is exact (``torch.equal``; NaNs of the reference's literal delta <= 0 formula must sit in the same places):

* against the ROW KERNEL (fft_finalize_kernel, an independent implementation of the same arithmetic): the same clips in a dealing
  where every clip straddles two workgroups, so the main kernel finalizes none of them;
* against the STREAMING FINALIZE (LEAF_ALGO_STREAM_FINALIZE: another kernel instance, frame sums in an LDS ring);
* against outputs recorded on an MI355X from the commit before this tail (tests/golden/tail_rows/, written by
  tests/golden/make_golden_tail_rows.py): the direct evidence that no bit moved.

Which tail a case runs follows from its dealing (tests/tail_rows_cases.py): B a multiple of the grid with at most 4000 sums per
workgroup -- the default forward's own count, which fits -- runs the tail on the sums in LDS; an uneven dealing runs the tail on the
partial sums in the workspace for the clips a workgroup owns (and the row kernel for the others: T' = 257 is there, because with whole
clips per workgroup and sums beyond the LDS the dispatcher takes the streaming finalize instead).  A clip of one block (T' = 1, 2) can
not straddle: those cases are held to the streaming finalize alone.  Launches are tiny: 2-4 workgroups (LEAF_ALGO_RESERVE_CUS)."""
import os

import numpy as np
import pytest
import torch

import tail_rows_cases as C
from leaf_pytorch_amd import _native as N

pytestmark = pytest.mark.gpu
G = 4


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    N.load()


def check(sr, F, tp, B, g, mode, seed, stream=True):
    """The case's default call against the row kernel (clips of two blocks or more) and the streaming finalize (``stream``)."""
    K, hop = C.GEOMETRY[sr]
    x, params = C.inputs(F, K, hop, tp, B, mode, seed)
    T = x.shape[1]
    plan = N.fft_plan_info(B, T, F, K, hop)
    assert plan is not None and plan["fft_n"] == 2048, plan
    nblk = plan["blocks_per_clip"]
    algo = N.ALGO_FFT_WG | C.grid_bits(g)
    got = C.forward(x, params, K, hop, mode, algo)
    assert got[0].shape == (B, F, tp)
    refs = []
    if nblk >= 2:
        refs.append(("row kernel", C.row_kernel_reference(x, params, K, hop, mode, nblk)))
    if stream and len(C.owned(B, nblk, g)) == B:             # whole clips per workgroup: the flag is honoured
        refs.append(("streaming finalize", C.forward(x, params, K, hop, mode, algo | C.SF)))
    assert refs, "a case without a reference"
    for what, ref in refs:
        for name, a, b in (("out", got[0], ref[0]), ("raw_out", got[1], ref[1])):
            if a is None:
                continue
            assert C.same(a, b), (f"{name} differs from the {what}: {int((torch.nan_to_num(a.float(), nan=12345.0) != torch.nan_to_num(b.float(), nan=12345.0)).sum())} "
                                  f"of {a.numel()} values, first at {tuple(int(v) for v in (torch.nan_to_num(a.float(), nan=12345.0) != torch.nan_to_num(b.float(), nan=12345.0)).nonzero()[0])}")


# ---- frames per row: both chunk lengths, chunk and group edges; 13 rows on twelve waves (one or two rows per wave)
@pytest.mark.parametrize("tp", C.FRAMES)
def test_frames_per_row_sums_in_lds(tp):
    check(16000, 13, tp, G, G, "pcen", 100 + tp)


@pytest.mark.parametrize("tp", C.FRAMES)
def test_frames_per_row_partial_sums_in_the_workspace(tp):
    check(16000, 13, tp, 2 * G + 1, G, "pcen", 200 + tp)


# ---- filters x clips per workgroup: fewer rows than waves, an uneven deal, a full 64-row set; 1, 2 and 3 clips per workgroup
LDS_CASES = [(F, tp, n) for F in C.FILTERS for tp in (17, 100, 130) for n in (1, 2, 3) if n * F * tp <= C.LDS_ELEMS]


@pytest.mark.parametrize("F,tp,n", LDS_CASES)
def test_filters_and_clips_per_workgroup_sums_in_lds(F, tp, n):
    check(16000, F, tp, n * G, G, "pcen", 300 + F + tp + n)


@pytest.mark.parametrize("F", C.FILTERS)
@pytest.mark.parametrize("tp,B", [(100, 2 * G + 1), (130, 3 * G + 1), (257, G + 1)])
def test_filters_and_owned_clips_partial_sums_in_the_workspace(F, tp, B):
    K, hop = C.GEOMETRY[16000]
    nblk = N.fft_plan_info(B, C.clip_len(tp, hop), F, K, hop)["blocks_per_clip"]
    assert 0 < len(C.owned(B, nblk, G)) < B                  # the tail and the row kernel both have clips
    check(16000, F, tp, B, G, "pcen", 400 + F + tp + B)


# ---- modes
@pytest.mark.parametrize("mode", C.MODES)
def test_modes_sums_in_lds(mode):
    check(16000, 13, 100, 2 * G, G, mode, 500 + len(mode))


@pytest.mark.parametrize("mode", C.MODES)
def test_modes_partial_sums_in_the_workspace(mode):
    check(16000, 40, 129, 2 * G + 1, G, mode, 600 + len(mode))


# ---- the other static geometries
@pytest.mark.parametrize("tp,B", [(17, G), (100, G), (130, 2 * G), (100, 2 * G + 1), (257, G + 1)])
def test_8_khz_geometry(tp, B):
    check(8000, 13, tp, B, G, "pcen", 700 + tp + B)


def test_32_khz_geometry_on_2048_sample_blocks():
    """801/320 runs the 2048-sample static instance (ten waves) where the tables are prepared ahead (leaf_forward_prepared_f32: no
    option word, every CU); LEAF_ALGO_FFT_WG itself means the 4096-sample kernel there.  One clip per CU finalizes in the tails from
    the sums in LDS; a batch half as large again deals unevenly: its clips go to the row kernel or to the tail on the workspace's
    partial sums.  The clips both batches share must agree."""
    K, hop = C.GEOMETRY[32000]
    F, tp, n = 40, 17, C.cus()
    x, params = C.inputs(F, K, hop, tp, n + n // 2, "pcen", 800)
    dev = torch.device(C.DEV)
    kern, pw, pb, alpha, delta, root, ema_w = [p.to(dev) for p in params]
    assert N.load().leaf_auto_algo(n, x.shape[1], F, K, hop) == N.ALGO_FFT_WG
    tables = N.prepare_tables(kern, pw, K, hop)
    assert tables is not None
    even = N.leaf_forward_prepared(x[:n].to(dev), tables, pb, alpha, delta, root, ema_w, F, K, hop)
    uneven = N.leaf_forward_prepared(x.to(dev), tables, pb, alpha, delta, root, ema_w, F, K, hop)
    torch.cuda.synchronize()
    assert torch.equal(even, uneven[:n]), f"{int((even != uneven[:n]).sum())} values differ"


# ---- the bits of the commit before the row-owned tail
@pytest.mark.parametrize("name,sr,F,tp,B,g,mode", C.GOLDEN, ids=[c[0] for c in C.GOLDEN])
def test_bits_of_the_tile_tail(name, sr, F, tp, B, g, mode):
    K, hop = C.GEOMETRY[sr]
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_rows", name + ".npz"))
    x, params = C.inputs(F, K, hop, tp, B, mode, C.golden_seed(name))
    out, raw = C.forward(x, params, K, hop, mode, N.ALGO_FFT_WG | C.grid_bits(g))
    w = torch.from_numpy(want["out"])
    w = w.view(torch.bfloat16) if out.dtype == torch.bfloat16 else w
    assert C.same(out, w), f"out: {int((torch.nan_to_num(out.float(), nan=12345.0) != torch.nan_to_num(w.float(), nan=12345.0)).sum())} values moved"
    if raw is not None:
        assert torch.equal(raw, torch.from_numpy(want["raw"])), "raw_out moved"
