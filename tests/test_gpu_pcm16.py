"""16-bit PCM input (LEAF_FLAG_X_PCM16; ``torch.int16`` waveforms through every Python layer).

The conversion float(v) * 2^-15 is exact in fp32, so the acceptance test is equality: the int16 path gives the BITS of the float32
path fed ``x.float() / 32768`` -- forward on every selector and geometry family, the saved pooled tensor, the parameter gradients
where the float32 backward is itself reproducible run to run -- plus one direct parity check against the fp64 oracle."""
import ctypes
import os
import socket

import pytest
import torch

from conftest import Golden, rel_err
from helpers import assert_grad_close, make_leaf
from oracle import leaf_oracle as lo
from leaf_pytorch_amd import _native
import leaf_pytorch_amd as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REL_TOL = 2e-5                                        # tests/test_gpu_parity.py: the float path's bound against the oracle
SELECTORS = {"auto": _native.ALGO_AUTO, "fft_small": _native.ALGO_FFT_SMALL, "fft": _native.ALGO_FFT, "fft_wg": _native.ALGO_FFT_WG,
             "mfma": _native.ALGO_MFMA}
# (name, F, K, hop): the static 16 / 32 / 8 kHz instances, a run-time geometry on 2048-sample blocks (22.05 kHz) and an odd window
# from 833 taps (run-time geometry on 4096-sample blocks)
GEOMETRIES = [("16k", 40, 401, 160), ("32k", 12, 801, 320), ("8k", 40, 201, 80), ("22k", 12, 552, 220), ("k833", 6, 833, 333)]
# the selectors that have a kernel at each geometry (leaf_workspace_bytes > 0 at the clip lengths of pcm_batches): each must have run
EXPECTED_SELECTORS = {"16k": set(SELECTORS), "8k": set(SELECTORS),
                      **{n: {"auto", "fft", "fft_wg", "mfma"} for n in ("32k", "22k", "k833")}}   # (the small-batch kernel: static 2048-sample instances only)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    _native.load()


def as_float(x16):
    return x16.float() / 32768


def quantise(x):
    return torch.round(x.clamp(-1, 1) * 32767).to(torch.int16)


def pcm_batches(K, hop, seed):
    """Seeded int16 batches (B,1,T): T below one block, several blocks, a ragged last block; uniform over the full range, a golden
    waveform quantised, an all-zero clip, and clips holding -32768 / 32767 at the first and last sample and across a block
    boundary."""
    g = torch.Generator().manual_seed(seed)
    info = _native.fft_plan_info(4, 8 * 4096, 8, K, hop)
    L_blk = info["block_len"] if info else 2048 - K + 1
    gold = quantise(Golden("default_b2").x)[:, 0]            # (2, 16000)
    out = []
    for T in (max(K, L_blk - 37), 3 * L_blk, 2 * L_blk + L_blk // 3 + 5):
        x = torch.randint(-32768, 32768, (5, T), generator=g, dtype=torch.int32).to(torch.int16)
        x[1, :min(T, 16000)] = gold[0, :min(T, 16000)]
        x[1, min(T, 16000):] = 0
        x[2] = 0
        x[3, 0], x[3, -1] = -32768, 32767
        x[4, 0], x[4, -1] = 32767, -32768
        for e in range(L_blk, T - 1, L_blk):                 # the extremes on both sides of every block boundary
            x[3, e - 1], x[3, e] = 32767, -32768
            x[4, e - 1], x[4, e] = -32768, 32767
        out.append(x[:, None, :].contiguous())
    return out


def module(F, K, hop, pcen, seed=0):
    torch.manual_seed(seed)
    kernel = torch.stack([0.2 + 2.5 * torch.rand(F), 6.0 + torch.rand(F) * K / 4], dim=1)
    geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
    params = lo.default_params(geo, pcen, kernel=kernel)
    return make_leaf(F, K, hop, pcen, params, DEV), params, geo


def covered(B, T, F, K, hop, algo):
    return _native.load().leaf_workspace_bytes(B, T, F, K, hop, algo & 0xff) > 0


# ---- 1. forward equals the float path bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pcen", "off", "log1p"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_forward_bits_equal_the_float_path(geom, mode):
    name, F, K, hop = geom
    m, _, _ = module(F, K, hop, mode == "pcen")
    if mode == "log1p":
        m.log_compression()
    ran = set()
    for x16 in pcm_batches(K, hop, seed=len(name) + K):
        x16 = x16.to(DEV)
        xf = as_float(x16)
        B, T = x16.shape[0], x16.shape[2]
        for sel, algo in SELECTORS.items():
            if not covered(B, T, F, K, hop, algo):
                continue
            for extra in (0, _native.ALGO_FULL_TRANSFORMS, _native.ALGO_STREAM_FINALIZE):
                m._algo = algo | extra
                with torch.no_grad():
                    got, want = m(x16), m(xf)
                assert got.dtype == torch.float32 and got.shape == want.shape
                assert torch.equal(got, want), f"{name}/{mode}/{sel}/extra={extra:#x} T={T}: max diff {float((got - want).abs().max()):.3e}"
                ran.add(sel)
        # serving mode and the folded peak normalisation (the identity on int16: equal to the plain call)
        m._algo = _native.ALGO_AUTO
        with torch.no_grad():
            plain = m(x16)
            m.cache_tables()
            cached = m(x16), m(x16)
            m.cache_tables(False)
            m.fuse_peak_normalization()
            folded = m(x16)
            m.fuse_peak_normalization(False)
        assert torch.equal(cached[0], plain) and torch.equal(cached[1], plain) and torch.equal(folded, plain)
        # the training forward: features and the saved pooled tensor
        prm = args_of(m)
        for sel, algo in SELECTORS.items():
            if not covered(B, T, F, K, hop, algo):
                continue
            o16, r16 = _native.leaf_forward(x16, *prm, K, hop, pcen=mode == "pcen", log1p=mode == "log1p", algo=algo, save_raw=True)
            o32, r32 = _native.leaf_forward(xf, *prm, K, hop, pcen=mode == "pcen", log1p=mode == "log1p", algo=algo, save_raw=True)
            assert torch.equal(o16, o32) and torch.equal(r16, r32), f"{name}/{mode}/{sel} T={T}: training forward"
    assert ran == EXPECTED_SELECTORS[name], (name, sorted(ran))


def args_of(m):
    c = m._compression
    return (m._complex_conv._kernel.detach(), m._pooling.weights.detach(), m._pooling._bias.detach(),
            *((c.alpha.detach(), c.delta.detach(), c.root.detach(), c.ema._weights.detach()) if c is not None else (None,) * 4))


def test_forward_bits_at_a_batch_the_workgroup_kernel_takes_under_auto():
    """AUTO at small batches is the small-batch kernel; from ~7/16 block per CU it is the workgroup kernel (what bench.py times)."""
    m = L.Leaf().eval().to(DEV)
    g = torch.Generator().manual_seed(5)
    x16 = torch.randint(-32768, 32768, (24, 1, 16000), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    assert _native.load().leaf_auto_algo(24, 16000, 40, 401, 160) == _native.ALGO_FFT_WG
    with torch.no_grad():
        assert torch.equal(m(x16), m(as_float(x16)))
        m.cache_tables()
        assert torch.equal(m(x16), m(as_float(x16)))
    assert torch.equal(_native.leaf_forward_profiled(x16, *args_of(m), 401, 160)[0], m(as_float(x16)).detach())


@pytest.mark.parametrize("geom", [("32k", 12, 801, 320, 3200), ("k833", 6, 833, 333, (4096 - 833 + 1) & ~1)], ids=["32k", "k833"])
def test_forward_bits_across_4096_sample_block_boundaries(geom):
    """LEAF_ALGO_FFT_WG at these windows is the 4096-sample plan at every batch (pcm_batches sizes its clips for the 2048-sample
    plan's blocks): clips of several 4096-sample blocks with a ragged last one, the extremes on both sides of every boundary."""
    name, F, K, hop, L4 = geom
    T = 2 * L4 + L4 // 3 + 5
    g = torch.Generator().manual_seed(K)
    x16 = torch.randint(-32768, 32768, (3, 1, T), generator=g, dtype=torch.int32).to(torch.int16)
    x16[2] = 0
    for e in (L4, 2 * L4):
        x16[0, 0, e - 1], x16[0, 0, e] = 32767, -32768
        x16[2, 0, e - 1], x16[2, 0, e] = -32768, 32767
    x16 = x16.to(DEV)
    assert _native.load().leaf_workspace_bytes(3, T, F, K, hop, _native.ALGO_FFT_WG) > 0
    for mode in ("pcen", "off", "log1p"):
        m, _, _ = module(F, K, hop, mode == "pcen")
        if mode == "log1p":
            m.log_compression()
        for extra in (0, _native.ALGO_FULL_TRANSFORMS, _native.ALGO_STREAM_FINALIZE):
            m._algo = _native.ALGO_FFT_WG | extra
            with torch.no_grad():
                got, want = m(x16), m(as_float(x16))
            assert torch.equal(got, want), f"{name}/{mode}/extra={extra:#x}: max diff {float((got - want).abs().max()):.3e}"
        o16, r16 = _native.leaf_forward(x16, *args_of(m), K, hop, pcen=mode == "pcen", log1p=mode == "log1p", algo=_native.ALGO_FFT_WG, save_raw=True)
        o32, r32 = _native.leaf_forward(as_float(x16), *args_of(m), K, hop, pcen=mode == "pcen", log1p=mode == "log1p", algo=_native.ALGO_FFT_WG, save_raw=True)
        assert torch.equal(o16, o32) and torch.equal(r16, r32), f"{name}/{mode}: training forward"


def test_staged_geometries_convert_once_and_never_raise_for_the_dtype():
    """Where the call lands on the staged forward (the explicit selector; a window beyond every fused path, where AUTO resolves to
    it), the Python layers convert with torch ops and run the float path: the same bits again, through the op and through ctypes."""
    lib = _native.load()
    for F, K, hop, T, auto_is_staged in ((5, 31, 7, 900, False), (4, 2113, 500, 9000, True)):
        assert (lib.leaf_auto_algo(3, T, F, K, hop) == _native.ALGO_STAGED) == auto_is_staged
        m, _, _ = module(F, K, hop, True)
        g = torch.Generator().manual_seed(6)
        x16 = torch.randint(-32768, 32768, (3, 1, T), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
        for algo in (_native.ALGO_AUTO, _native.ALGO_STAGED):
            m._algo = algo
            with torch.no_grad():
                assert torch.equal(m(x16), m(as_float(x16)))
            prm = args_of(m)
            want = _native.leaf_forward(as_float(x16), *prm, K, hop, algo=algo)
            assert torch.equal(_native.leaf_forward(x16, *prm, K, hop, algo=algo), want)
            if algo == _native.ALGO_STAGED or auto_is_staged:
                for x in (x16, as_float(x16)):     # the measurement call has no staged forward: int16 is answered as float32 is
                    with pytest.raises(RuntimeError, match="algorithm selector"):
                        _native.leaf_forward_profiled(x, *prm, K, hop, algo=algo)
            else:
                assert torch.equal(_native.leaf_forward_profiled(x16, *prm, K, hop, algo=algo)[0], want)
    m, _, _ = module(5, 31, 7, True)
    x16 = torch.randint(-32768, 32768, (3, 1, 900), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    for p in m.parameters():
        p.requires_grad_(True)
    m._algo = _native.ALGO_AUTO
    m(x16).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


# ---- 2. one direct parity check at the default geometry ------------------------------------------------------------------------
def test_default_geometry_matches_the_fp64_oracle():
    gd = Golden("default_b2")
    x16 = quantise(gd.x)
    m = make_leaf(gd.n_filters, gd.window_size, gd.hop, gd.pcen, gd.params, DEV)
    with torch.no_grad():
        out = m(x16.to(DEV)).cpu()
    p64 = {k: v.double() for k, v in gd.params.items()}
    ref = lo.leaf_forward(x16.double() / 32768, p64, gd.geometry(), gd.pcen, torch.float64)
    err = rel_err(out, ref.float())
    print(f"int16 forward vs fp64 oracle: elementwise rel err {err:.3e} (bound {REL_TOL})")
    assert err < REL_TOL, f"rel err {err:.3e}"


# ---- 3. backward -------------------------------------------------------------------------------------------------------------
BWD_PATHS = [("16k-default", 40, 401, 160, {}), ("32k-default", 12, 801, 320, {}), ("8k-default", 40, 201, 80, {}),
             ("22k-runtime", 12, 552, 220, {}), ("16k-mfma", 40, 401, 160, {"mfma": True}), ("16k-staged", 8, 401, 160, {"staged": True})]
# the clip lengths at which a block load ends ragged (tests/test_gpu_backward_edges.py): one sample, one hop h, h + 1, and L - 1, L, L + 1
# of the plan's block length L -- at odd T a clip's 16-bit row does not start on a 4-byte boundary.  Sixth field: T (else from the plan).
EDGE_LENGTHS = lambda hop, L: (1, hop, hop + 1, L - 1, L, L + 1)
BWD_PATHS += [(f"16k-per-wave-edge-T{T}", 40, 401, 160, {}, T) for T in EDGE_LENGTHS(160, 1600)]
GRAD_NAMES = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
              "_compression.root", "_compression.ema._weights"]


@pytest.mark.parametrize("full", [False, True], ids=["band", "full"])
@pytest.mark.parametrize("mode", ["pcen", "log1p"])
@pytest.mark.parametrize("path", BWD_PATHS, ids=[p[0] for p in BWD_PATHS])
def test_parameter_gradients_equal_the_float_backward(path, mode, full):
    """The seven parameter gradients (three with PCEN off).  The float32 backward runs twice first: where those two runs are
    bit-equal the int16 result must be bit-equal too; a path that is not reproducible run to run (none is expected: the
    backward sums in a fixed order, no atomics) is held to fp64 autograd through the oracle with assert_grad_close instead."""
    name, F, K, hop, force = path[:5]
    pcen = mode == "pcen"
    m, params, geo = module(F, K, hop, pcen, seed=3)
    prm = args_of(m)
    info = _native.fft_plan_info(4, 8 * 4096, F, K, hop)
    L_blk = info["block_len"] if info else 2048 - K + 1
    T = (2 * L_blk + L_blk // 3 + 5) if not force.get("staged") else 1500
    if len(path) > 5:
        T = path[5]
    g = torch.Generator().manual_seed(11)
    x16 = torch.randint(-32768, 32768, (3, 1, T), generator=g, dtype=torch.int32).to(torch.int16)
    x16[1, 0, 0], x16[1, 0, -1] = -32768, 32767
    x16[2] = quantise(0.3 * torch.randn(1, T, generator=g))
    x16 = x16.to(DEV)
    xf = as_float(x16)
    kw = dict(pcen=pcen, log1p=mode == "log1p", full_transforms=full, **force)
    out, raw = _native.leaf_forward(xf, *prm, K, hop, pcen=pcen, log1p=mode == "log1p", save_raw=True)
    go = torch.randn(out.shape, generator=g).to(DEV)
    a = _native.leaf_backward(xf, *prm, K, hop, go, pooled_raw=raw, **kw)
    b = _native.leaf_backward(xf, *prm, K, hop, go, pooled_raw=raw, **kw)
    got = _native.leaf_backward(x16, *prm, K, hop, go, pooled_raw=raw, **kw)
    n = 7 if pcen else 3
    assert got[7] is None
    reproducible = all(torch.equal(a[i], b[i]) for i in range(n))
    print(f"{name}/{mode}/{'full' if full else 'band'}: float32 backward reproducible run to run: {reproducible}")
    if reproducible:
        for i in range(n):
            assert torch.equal(got[i], a[i]), f"{name}/{mode}: {GRAD_NAMES[i]} differs by {float((got[i] - a[i]).abs().max()):.3e}"
        return
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}            # not reproducible: fp64 autograd decides
    o64 = lo.leaf_forward(x16.cpu().double() / 32768, p64, geo, pcen, torch.float64)
    if mode == "log1p":
        o64 = torch.log1p(o64)
    o64.backward(go.cpu().double())
    for i in range(n):
        assert_grad_close(GRAD_NAMES[i], got[i], p64[GRAD_NAMES[i]].grad, ctx=f"({name}/{mode}, not reproducible run to run)")


# The batches above are a few blocks: the one-wave-per-block backward.  From a number of blocks per CU the dispatcher takes the
# workgroup-per-block kernels, which have their own int16 loads (leaf_fft_wg_bwd.hpp, leaf_fft_wgg4k_bwd.hpp) or read the widened
# copy (leaf_fft_wgg_bwd.hpp).  (name, F, K, hop, T, largest block length the plan can have, threshold in sixteenths of a block per CU
# with band tasks possible / with full_transforms -- leaf_kernels.hip: wg_bwd_sixteenths, fft_wgg_bwd_use, make_fft4k_bwd_plan).
WG_BWD_PATHS = [("16k-workgroup", 40, 401, 160, 15900, 2048 - 401 + 1, 6, 20),          # static instance; band tasks from 6/16, else 20/16
                ("8k-workgroup", 40, 201, 80, 8000, 2048 - 201 + 1, 20, 20),             # static instance, no band tasks
                ("32k-4096", 12, 801, 320, 7000, 3200, 8, 8),                            # static 4096-sample plan
                ("22k-runtime-workgroup", 12, 552, 220, 9000, 2048 - 552 + 1, 10, 10),   # run-time geometry: the widened copy
                ("k833-runtime-4096", 6, 833, 333, 7000, (4096 - 833 + 1) & ~1, 8, 8)]   # run-time geometry on 4096-sample blocks
# ... and at the clip-length edges: one or two blocks per clip (here the block length field is the plan's own)
WG_BWD_PATHS += [(f"16k-workgroup-edge-T{T}", 40, 401, 160, T, 1600, 6, 20) for T in EDGE_LENGTHS(160, 1600)]
WG_BWD_PATHS += [(f"32k-4096-edge-T{T}", 12, 801, 320, T, 3200, 8, 8) for T in EDGE_LENGTHS(320, 3200)]
WG_BWD_PATHS += [(f"k833-runtime-4096-edge-T{T}", 6, 833, 333, T, (4096 - 833 + 1) & ~1, 8, 8) for T in EDGE_LENGTHS(333, (4096 - 833 + 1) & ~1)]


@pytest.mark.parametrize("full", [False, True], ids=["band", "full"])
@pytest.mark.parametrize("mode", ["pcen", "log1p"])
@pytest.mark.parametrize("path", WG_BWD_PATHS, ids=[p[0] for p in WG_BWD_PATHS])
def test_parameter_gradients_equal_the_float_backward_on_the_workgroup_kernels(path, mode, full):
    """The batch is sized from the device's CU count so that the call is past the dispatcher's threshold for the workgroup kernel of
    its family (one clip more than the threshold asks for; the block count is a lower bound, from the largest block length).  Held
    as above: float32 twice, then bit equality -- and the backward recomputing the pooled tensor itself from the int16 waveform,
    against the float32 backward doing the same."""
    name, F, K, hop, T, L_max, six_band, six_full = path
    pcen = mode == "pcen"
    m, params, geo = module(F, K, hop, pcen, seed=4)
    prm = args_of(m)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    nblk = -(-T // L_max)
    need = -(-cus * (six_full if full else six_band) // 16)
    B = -(-need // nblk) + 1
    edge = "-edge-" in name                               # (one or two blocks per clip, one frame at T <= hop)
    assert B * nblk >= need and (nblk >= 3 or edge)
    g = torch.Generator(device=DEV).manual_seed(13)
    x16 = torch.randint(-32768, 32768, (B, 1, T), generator=g, dtype=torch.int32, device=DEV).to(torch.int16)
    x16[1, 0, 0], x16[1, 0, -1] = -32768, 32767
    x16[2] = 0
    if T >= L_max + 2:
        x16[B - 1, 0, L_max - 2:L_max + 2] = torch.tensor([32767, -32768, 32767, -32768], dtype=torch.int16, device=DEV)
    xf = as_float(x16)
    kw = dict(pcen=pcen, log1p=mode == "log1p", full_transforms=full)
    out, raw = _native.leaf_forward(xf, *prm, K, hop, pcen=pcen, log1p=mode == "log1p", save_raw=True)
    go = torch.randn(out.shape, generator=g, device=DEV)
    a = _native.leaf_backward(xf, *prm, K, hop, go, pooled_raw=raw, **kw)
    b = _native.leaf_backward(xf, *prm, K, hop, go, pooled_raw=raw, **kw)
    got = _native.leaf_backward(x16, *prm, K, hop, go, pooled_raw=raw, **kw)
    # no pooled_raw: the backward recomputes the pooled tensor from the waveform with a kernel of its own choice, so the reference is
    # the float32 backward that does the same
    again = _native.leaf_backward(x16, *prm, K, hop, go, **kw)
    again_f = _native.leaf_backward(xf, *prm, K, hop, go, **kw)
    n = 7 if pcen else 3
    reproducible = all(torch.equal(a[i], b[i]) for i in range(n))
    print(f"{name}/{mode}/{'full' if full else 'band'}: B={B} ({B * nblk}+ blocks, {cus} CUs), float32 backward reproducible: {reproducible}")
    if reproducible:
        for i in range(n):
            # (a clip of one frame has no smoother step, a clip of one sample meets the pooling window at its centre alone: those
            # gradients are exact zeros, in fp64 as here)
            exact_zero = (T <= hop and GRAD_NAMES[i] == "_compression.ema._weights") or (T == 1 and GRAD_NAMES[i] == "_pooling.weights")
            assert float(a[i].abs().max()) > 0 or exact_zero, GRAD_NAMES[i]
            assert torch.equal(got[i], a[i]), f"{name}/{mode}: {GRAD_NAMES[i]} differs by {float((got[i] - a[i]).abs().max()):.3e}"
            assert torch.equal(again[i], again_f[i]), f"{name}/{mode}: {GRAD_NAMES[i]} (pooled tensor recomputed) differs by {float((again[i] - again_f[i]).abs().max()):.3e}"
        return
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}            # not reproducible: fp64 autograd decides
    o64 = lo.leaf_forward(x16.cpu().double() / 32768, p64, geo, pcen, torch.float64)
    if mode == "log1p":
        o64 = torch.log1p(o64)
    o64.backward(go.cpu().double())
    for i in range(n):
        assert_grad_close(GRAD_NAMES[i], got[i], p64[GRAD_NAMES[i]].grad, ctx=f"({name}/{mode}, not reproducible run to run)")


@pytest.mark.parametrize("masked", [False, True], ids=["dispatcher-op", "autograd-function"])
def test_module_backward_fills_every_parameter_gradient(masked, monkeypatch):
    from leaf_pytorch_amd import _ops
    if masked:
        monkeypatch.setattr(_ops, "available", lambda: False)        # the ops library masked off: _LeafForward over ctypes
    else:
        _ops.load()
    torch.manual_seed(2)
    g = torch.Generator().manual_seed(2)
    x16 = torch.randint(-32768, 32768, (3, 1, 8000), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    m16, m32 = L.Leaf().to(DEV), L.Leaf().to(DEV)
    m32.load_state_dict(m16.state_dict())
    m16(x16).sum().backward()
    m32(as_float(x16)).sum().backward()
    for (k, p), (_, q) in zip(m16.named_parameters(), m32.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
        assert torch.equal(p.grad, q.grad), k


# ---- 4. surface --------------------------------------------------------------------------------------------------------------
def test_opcheck_and_compile():
    from leaf_pytorch_amd import _ops
    _ops.load()
    m = L.Leaf().eval().to(DEV)
    prm = args_of(m)
    g = torch.Generator().manual_seed(4)
    x16 = torch.randint(-32768, 32768, (3, 1, 4000), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    out = torch.ops.leaf_amd.forward(x16, *prm, 401, 160, False, 0)
    assert out.dtype == torch.float32 and torch.equal(out, _native.leaf_forward(as_float(x16), *prm, 401, 160))
    torch.library.opcheck(torch.ops.leaf_amd.forward.default, (x16, *prm, 401, 160, False, 0), test_utils=("test_schema", "test_faketensor"))
    req = [p.clone().requires_grad_(True) for p in prm]
    torch.library.opcheck(torch.ops.leaf_amd.forward_train.default, (x16, *req, 401, 160, 0, False),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    o, raw = torch.ops.leaf_amd.forward_train(x16, *prm, 401, 160, 0, False)
    go = torch.randn_like(o)
    torch.library.opcheck(torch.ops.leaf_amd.backward.default, (x16, *prm, 401, 160, go, raw, False, 0), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="int16"):
        torch.ops.leaf_amd.backward(x16, *prm, 401, 160, go, raw, True, 0)
    with pytest.raises(RuntimeError, match="int16"):
        _native.leaf_backward(x16, *prm, 401, 160, go, need_dx=True, pooled_raw=raw)
    for p in m.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        eager = m(x16)
        compiled = torch.compile(m, fullgraph=True)(x16)
    assert compiled.dtype == torch.float32 and torch.equal(compiled, eager)
    with pytest.raises(RuntimeError):
        m(x16.double())
    with pytest.raises(RuntimeError):
        m(torch.cat([x16, x16], dim=1))


def test_sharded_empty_and_raw_abi():
    import torch.distributed as dist
    from leaf_pytorch_amd import parallel
    m = L.Leaf().eval().to(DEV)
    g = torch.Generator().manual_seed(8)
    x16 = torch.randint(-32768, 32768, (5, 1, 4000), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    with torch.no_grad():
        ref = m(x16)
        empty = m(x16[:0])
    assert tuple(empty.shape) == (0, 40, 25) and empty.dtype == torch.float32
    assert _native.leaf_forward(x16[:0], *args_of(m), 401, 160).dtype == torch.float32
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        with torch.no_grad():
            assert torch.equal(parallel.forward_sharded(m, x16), ref)
    finally:
        dist.destroy_process_group()
    # the C ABI raw through ctypes: an int16 device buffer at a 2-byte-but-not-4-byte aligned offset equals the aligned call
    lib = _native.load()
    B, T, F, K, hop = 5, 4000, 40, 401, 160
    prm = [t.contiguous() for t in args_of(m)]
    flat = torch.zeros(B * T + 8, dtype=torch.int16, device=DEV)
    flat[1:1 + B * T] = x16.reshape(-1)
    assert flat.data_ptr() % 4 == 0
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = _native.workspace(lib.leaf_workspace_bytes(B, T, F, K, hop, 0), torch.device(DEV))
    outs = []
    for ptr in (ctypes.c_void_p(flat.data_ptr() + 2), P(x16.contiguous())):
        out = torch.empty(B, F, 25, device=DEV)
        rc = lib.leaf_forward_f32(ptr, B, T, *(P(t) for t in prm), F, K, hop, _native.FLAG_PCEN | _native.FLAG_X_PCM16, 0, P(out), P(ws),
                                  ctypes.c_size_t(ws.numel()), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], ref)


@pytest.mark.parametrize("pcen", [True, False])
def test_stream_of_int16_chunks_equals_the_float_stream(pcen):
    from leaf_pytorch_amd.streaming import LeafStream
    m = L.Leaf(pcen_compression=pcen).eval().to(DEV)
    g = torch.Generator().manual_seed(12)
    T = int(1.7 * 16000) + 11
    x16 = torch.randint(-32768, 32768, (2, 1, T), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)
    cuts = [0, 700, 701, 5000, 5160, 14000, T]
    s16, s32 = LeafStream(m), LeafStream(m)
    f16, f32 = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        f16.append(s16.step(x16[:, :, a:b]))
        f32.append(s32.step(as_float(x16[:, :, a:b])))
        assert s16.buf is None or s16.buf.dtype == torch.int16
    with pytest.raises(RuntimeError, match="one sample type per stream"):
        s16.step(as_float(x16[:, :, :100]))
    f16.append(s16.flush())
    f32.append(s32.flush())
    got, want = torch.cat(f16, dim=2), torch.cat(f32, dim=2)
    assert got.dtype == torch.float32 and got.shape == (2, 40, (T - 1) // 160 + 1)
    assert torch.equal(got, want)


def test_stream_widens_other_integer_chunks_as_before():
    """Only int16 means PCM: an int32 chunk is still widened with ``.float()``, unscaled, as it was before int16 streams existed."""
    from leaf_pytorch_amd.streaming import LeafStream
    m = L.Leaf().eval().to(DEV)
    g = torch.Generator().manual_seed(14)
    x = torch.randint(-3, 4, (2, 1, 3000), generator=g, dtype=torch.int32).to(DEV)
    a, b = LeafStream(m), LeafStream(m)
    fa, fb = a.step(x), b.step(x.float())
    assert a.buf.dtype == torch.float32 and fa.shape[2] > 0 and torch.equal(fa, fb)
    assert torch.equal(a.flush(), b.flush())
