"""The early first-block forward of the static workgroup kernel (csrc/leaf_fft_wg.hpp): without first-block spectra from the table
launch, the last two waves of a workgroup request its first two blocks before the twiddle tables are built, transform them right
after the barrier and publish them as fwd(0) / fwd(1); the task queue starts behind them.  The cached route (a table-cache hit
builds no first-block spectra), int16 PCM and mixed calls take it in the tail-finalize instances; the streaming-finalize instances keep
the queue's own start but load through the same loader function (the kind chosen at run time), so their cases run here too: they
cover the loader, not the early path.

Every fp32 / bf16 case at 16 kHz is ``torch.equal`` against the same call with LEAF_ALGO_NO_TABLE_CACHE: that route gets the first
spectra from the table launch and never takes the early path -- independent code, the same bits.  int16 PCM is compared with its
float32 twin and ``forward_mixup`` with the forward of the explicitly mixed waveform, both on that route.  At 8 kHz (201/80) the table
launch has no first-block spectra on any route, so both routes take the early path there: that case is compared with the output the
commit before the early path gave for the same input (tests/golden/early_forward/parent_8k.npz, recorded on an MI355X).  Calls meant
for the cached route assert that the dispatcher sent them through leaf_forward_cached_f32.  The first two clips are also held to the
fp64 oracle at the parity suite's REL_TOL.  The selector is an explicit ALGO_FFT_WG (bits are batch-invariant within one kernel),
the grid comes from LEAF_ALGO_RESERVE_CUS."""
import pytest
import torch

from conftest import rel_err
from helpers import make_leaf
from oracle import leaf_oracle as lo
from leaf_pytorch_amd import _native, _ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = _native
REL_TOL = 2e-5                                               # tests/test_gpu_parity.py
SF = N.ALGO_STREAM_FINALIZE


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    N.load()
    _ops.load()


def cached_calls():
    """Calls the dispatcher op has sent through leaf_forward_cached_f32 so far (tests/test_gpu_table_cache.py)."""
    return int(torch.ops.leaf_amd.table_cache_info()[1])


def grid(g):
    """algo bits that leave the call ``g`` CUs: ``g`` workgroups when there are at least as many blocks"""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert 0 < g <= cus and cus - g < 256
    return N.algo_reserve_cus(cus - g)


_MODELS = {}


def model(sample_rate=16000):
    """(module, oracle parameters, geometry): the default front end at a sample rate, built once"""
    if sample_rate not in _MODELS:
        geo = lo.geometry(sample_rate=sample_rate)
        params = lo.default_params(geo)
        _MODELS[sample_rate] = (make_leaf(geo.n_filters, geo.window_size, geo.hop, True, params, DEV), params, geo)
    return _MODELS[sample_rate]


def waveform(b, t, seed):
    return 2 * torch.rand(b, 1, t, generator=torch.Generator().manual_seed(seed)) - 1


def run(m, x, algo, cached=True):
    """One no-grad forward; ``cached``: through the table cache (asserted), else with LEAF_ALGO_NO_TABLE_CACHE (asserted too)."""
    m._algo = algo if cached else algo | N.ALGO_NO_TABLE_CACHE
    n0 = cached_calls()
    try:
        with torch.no_grad():
            out = m(x)
    finally:
        m._algo = N.ALGO_AUTO
    torch.cuda.synchronize()
    assert cached_calls() - n0 == (1 if cached else 0), "the call did not take the route the test is about"
    return out


def check_oracle(out, x_float, sample_rate=16000):
    _, params, geo = model(sample_rate)
    n = min(2, x_float.shape[0])
    ref = lo.leaf_forward(x_float[:n].cpu().float(), params, geo, True, torch.float32)
    err = rel_err(out[:n].float().cpu(), ref)
    print(f"first {n} clips vs fp64 oracle: rel err {err:.3e} (bound {REL_TOL})")
    assert err < REL_TOL


# (name, B, T, workgroups, extra algo bits)
SHAPES = [
    ("nset1-task1-is-the-skipped-slot", 1, 16000, 10, 0),
    ("nset2-exactly-the-two-early-blocks", 1, 16000, 5, 0),
    ("uneven-nset-clips-straddle-workgroups", 3, 16000, 4, 0),
    ("second-early-block-mostly-beyond-T", 2, 1600 + 7, 2, 0),
    ("streaming-finalize-whole-clips", 2, 16000, 2, SF),
]


@pytest.mark.parametrize("name,B,T,g,extra", SHAPES, ids=[s[0] for s in SHAPES])
def test_early_path_gives_the_bits_of_the_table_launch_spectra(name, B, T, g, extra):
    m, _, geo = model()
    assert (geo.window_size, geo.hop) == (401, 160)
    x = waveform(B, T, seed=len(name)).to(DEV)
    algo = N.ALGO_FFT_WG | grid(g) | extra
    want = run(m, x, algo, cached=False)
    for i in range(2):                                       # a miss (the validator builds the tables), then a hit: no spectra either way
        got = run(m, x, algo)
        assert torch.equal(got, want), f"{name} call {i}: max diff {float((got - want).abs().max()):.3e}"
    check_oracle(got, x)


def test_sample_kind_fp32():
    m, _, _ = model()
    x = waveform(2, 16000, seed=21).to(DEV)
    algo = N.ALGO_FFT_WG | grid(2)
    got = run(m, x, algo)
    assert torch.equal(got, run(m, x, algo, cached=False))
    check_oracle(got, x)


def test_sample_kind_bf16():
    m, _, _ = model()
    x = waveform(2, 16000, seed=22).to(torch.bfloat16).to(DEV)
    for extra in (0, SF):
        algo = N.ALGO_FFT_WG | grid(2) | extra
        got = run(m, x, algo)
        want = run(m, x, algo, cached=False)
        assert got.dtype == want.dtype and torch.equal(got, want), f"extra={extra:#x}"
    ref = run(m, x.float(), N.ALGO_FFT_WG | grid(2), cached=False)      # the bf16 call rounds its output: one bf16 ulp of the fp32 result
    assert float(((got.float() - ref).abs() / ref.abs().clamp_min(1e-30)).max()) < 2.0 ** -7


def test_sample_kind_int16_pcm_against_its_float32_twin():
    m, _, _ = model()
    x16 = (waveform(2, 16000, seed=23) * 32767).round().to(torch.int16).to(DEV)
    twin = x16.float() / 32768
    for extra in (0, SF):
        algo = N.ALGO_FFT_WG | grid(2) | extra
        want = run(m, twin, algo, cached=False)
        assert torch.equal(run(m, x16, algo), want), f"cached route, extra={extra:#x}"
        assert torch.equal(run(m, x16, algo, cached=False), want), f"table launch without spectra, extra={extra:#x}"
    check_oracle(want, twin)


def test_sample_kind_mixed_against_the_forward_of_the_mixed_waveform():
    m, _, _ = model()
    B = 2
    lam = torch.tensor([0.3, 0.75])
    perm = torch.tensor([1, 0])
    for int16 in (False, True):
        x = waveform(B, 16000, seed=24) * 0.98
        x = torch.where(x.abs() < 2.0 ** -10, torch.full_like(x, 0.125), x)       # (no subnormal product: tests/test_gpu_mixup.py)
        x = (torch.round(x * 32767).to(torch.int16) if int16 else x).to(DEV)
        xf = x.float() / 32768 if int16 else x
        lam_d = lam.to(DEV).view(B, 1, 1)
        mixed = xf * lam_d + xf[perm.to(DEV)] * (1 - lam_d)
        for extra in (0, SF):
            algo = N.ALGO_FFT_WG | grid(2) | extra
            want = run(m, mixed, algo, cached=False)
            m._algo = algo
            try:
                with torch.no_grad():
                    got = m.forward_mixup(x, perm, lam)
            finally:
                m._algo = N.ALGO_AUTO
            assert torch.equal(got, want), f"int16={int16} extra={extra:#x}: max diff {float((got - want).abs().max()):.3e}"
    check_oracle(want, mixed)


def test_the_8_khz_static_instance():
    m, _, geo = model(8000)
    assert (geo.window_size, geo.hop) == (201, 80)
    import os
    import numpy as np
    x = waveform(2, 8000, seed=25).to(DEV)
    want = torch.from_numpy(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "early_forward", "parent_8k.npz"))["out"])
    for g in (2, 5):
        algo = N.ALGO_FFT_WG | grid(g)
        got = run(m, x, algo)
        assert torch.equal(got.cpu(), want), f"g={g}: max diff {float((got.cpu() - want).abs().max()):.3e}"
        assert torch.equal(run(m, x, algo, cached=False), got), g
    check_oracle(got, x, 8000)
