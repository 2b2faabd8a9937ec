"""bfloat16 features from float32 and int16 PCM waveforms (LEAF_FLAG_OUT_BF16; ``out_bf16=True`` in the host layers and the ops;
``Leaf.output_dtype``).

Every criterion is exact.  The kernels compute in float32 as without the flag and round each feature to nearest even where they
store it, so the forward must give the BITS of the float32 call's result cast with ``.to(torch.bfloat16)`` -- same explicit selector
on both sides, because AUTO changes kernels at batch thresholds.  Widening bfloat16 is exact, so the backward on a bfloat16
``grad_out`` must give the bits of the float32 backward on ``grad_out.float()``."""
import ctypes

import pytest
import torch

from guarded import guarded, guarded_tensor, unchanged
from helpers import make_leaf
from oracle import leaf_oracle as lo
from leaf_pytorch_amd import _native as N
import leaf_pytorch_amd as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
FULL, SFIN = N.ALGO_FULL_TRANSFORMS, N.ALGO_STREAM_FINALIZE
PC, OUT, IO, PCM = N.FLAG_PCEN, N.FLAG_OUT_BF16, N.FLAG_IO_BF16, N.FLAG_X_PCM16
MODES = ["pcen", "off", "log1p"]
XTYPES = [torch.float32, torch.int16]
GRAD_NAMES = ["kernel", "pool_w", "pool_b", "alpha", "delta", "root", "ema_w"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    N.load()


def n_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def waveform(B, T, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        x = torch.randint(-32768, 32768, (B, 1, T), generator=g, dtype=torch.int32).to(torch.int16)
        x[0, 0, 0], x[0, 0, -1] = -32768, 32767
    else:
        x = 2 * torch.rand(B, 1, T, generator=g) - 1
    return x.to(DEV)


def module(F, K, hop, mode, seed=0):
    """16 kHz with 40 filters: the default (mel) initialisation, whose narrow-band filters run as band tasks; elsewhere seeded filters."""
    pcen = mode == "pcen"
    if (F, K, hop) == (40, 401, 160):
        m = L.Leaf(pcen_compression=pcen).eval()
        for p in m.parameters():
            p.requires_grad_(False)
        m = m.to(DEV)
    else:
        torch.manual_seed(seed)
        kernel = torch.stack([0.2 + 2.5 * torch.rand(F), 6.0 + torch.rand(F) * K / 4], dim=1)
        geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
        m = make_leaf(F, K, hop, pcen, lo.default_params(geo, pcen, kernel=kernel), DEV)
    if mode == "log1p":
        m.log_compression()
    return m


def args_of(m):
    c = m._compression
    return (m._complex_conv._kernel.detach(), m._pooling.weights.detach(), m._pooling._bias.detach(),
            *((c.alpha.detach(), c.delta.detach(), c.root.detach(), c.ema._weights.detach()) if c is not None else (None,) * 4))


def covered(B, T, F, K, hop, algo):
    return N.load().leaf_workspace_bytes(B, T, F, K, hop, algo & 0xff) > 0


def check_forward(m, x, algo, what):
    """Three routes to bfloat16 features against the float32 call narrowed: the module (dispatcher op), the ctypes host function and
    its training entry (leaf_forward_save_f32: the saved pooled tensor stays float32 and keeps its bits)."""
    K, hop = m._complex_conv._kernel_size, m._pooling.strides
    pcen, log1p = m._compression is not None, m._log1p
    m._algo = algo
    with torch.no_grad():
        want32 = m.output_dtype(None)(x)
        got = m.output_dtype(BF)(x)
    m.output_dtype(None)
    assert want32.dtype == torch.float32 and got.dtype == BF and got.shape == want32.shape, what
    want = want32.to(BF)
    assert torch.isfinite(want32).all(), what
    assert torch.equal(got, want), f"{what}: module: {int((got != want).sum())} of {want.numel()} features differ"
    prm = args_of(m)
    nat = N.leaf_forward(x, *prm, K, hop, pcen=pcen, log1p=log1p, algo=algo, out_bf16=True)
    assert nat.dtype == BF and torch.equal(nat, want), f"{what}: ctypes: {int((nat != want).sum())} features differ"
    o, raw = N.leaf_forward(x, *prm, K, hop, pcen=pcen, log1p=log1p, algo=algo, out_bf16=True, save_raw=True)
    o32, raw32 = N.leaf_forward(x, *prm, K, hop, pcen=pcen, log1p=log1p, algo=algo, save_raw=True)
    assert o.dtype == BF and raw.dtype == torch.float32 and torch.equal(o, o32.to(BF)) and torch.equal(raw, raw32), f"{what}: training forward"


# ---- 1. forward: selector x geometry ---------------------------------------------------------------------------------------------
# T = 801: a 6-frame row; 4000: several blocks with a ragged tail; 16001: T' = 101, odd -- the 2-byte stores of a row and the 128-byte
# segments of the streaming finalize end in the middle of a 4-byte word
LENGTHS = (801, 4000, 16001)


@pytest.mark.parametrize("xtype", XTYPES, ids=["f32", "pcm16"])
@pytest.mark.parametrize("mode", MODES)
def test_forward_16k_every_selector_band_and_full(mode, xtype):
    m = module(40, 401, 160, mode)
    ran = set()
    for B in (1, 3):
        for T in LENGTHS:
            x = waveform(B, T, xtype, seed=B * 100003 + T)
            for name, sel in (("fft_small", N.ALGO_FFT_SMALL), ("fft", N.ALGO_FFT), ("fft_wg", N.ALGO_FFT_WG), ("mfma", N.ALGO_MFMA)):
                if not covered(B, T, 40, 401, 160, sel):
                    continue
                for extra in (0, FULL):
                    check_forward(m, x, sel | extra, f"16k/{mode}/{name}/extra={extra:#x} B={B} T={T}")
                ran.add(name)
    assert ran == {"fft_small", "fft", "fft_wg", "mfma"}, sorted(ran)


@pytest.mark.parametrize("xtype", XTYPES, ids=["f32", "pcm16"])
@pytest.mark.parametrize("mode", MODES)
def test_forward_streaming_finalize_on_whole_clips(mode, xtype):
    """B = #CUs: the contiguous dealing gives every workgroup of the workgroup kernel whole clips, so every row is finalized as its
    blocks complete, 128-byte segments at a time (LEAF_ALGO_STREAM_FINALIZE); T' = 25 and the odd T' = 101."""
    m = module(40, 401, 160, mode)
    B = n_cus()
    for T in (4000, 16001):
        check_forward(m, waveform(B, T, xtype, seed=T), N.ALGO_FFT_WG | SFIN, f"stream/{mode} B={B} T={T}")
    check_forward(m, waveform(3, 16001, xtype, seed=9), N.ALGO_FFT_WG | SFIN, f"stream/{mode} B=3 T=16001")


GEOMS = [("8k", 40, 201, 80, (801, 4000, 16001), (N.ALGO_FFT_SMALL, N.ALGO_FFT, N.ALGO_FFT_WG)),
         ("32k", 12, 801, 320, (8200,), (N.ALGO_FFT_WG, N.ALGO_FFT_WG | FULL)),                      # 4096-sample blocks: just over 8192
         ("22k-runtime", 12, 552, 220, (801, 4000, 16001), (N.ALGO_FFT, N.ALGO_FFT_WG))]                # a run-time-geometry window


@pytest.mark.parametrize("xtype", XTYPES, ids=["f32", "pcm16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_forward_other_geometries(geom, mode, xtype):
    name, F, K, hop, lengths, selectors = geom
    m = module(F, K, hop, mode)
    ran = 0
    for B in (1, 3):
        for T in lengths:
            x = waveform(B, T, xtype, seed=B * 7919 + T)
            for algo in selectors:
                if covered(B, T, F, K, hop, algo):
                    check_forward(m, x, algo, f"{name}/{mode}/algo={algo:#x} B={B} T={T}")
                    ran += 1
    assert ran >= 2 * len(lengths), ran
    if name == "32k":
        assert N.fft_plan_info(1, 8200, F, K, hop) is not None and covered(1, 8200, F, K, hop, N.ALGO_FFT_WG)


@pytest.mark.parametrize("xtype", XTYPES, ids=["f32", "pcm16"])
def test_forward_where_auto_lands_on_staged_narrows_on_the_host(xtype):
    """A window beyond every fused plan: AUTO resolves to the staged kernels, which store float32 only (LEAF_ERR_UNSUPPORTED at the C
    ABI); the host layers run float32 and narrow -- the same rounding, so the same bits -- through the op and through ctypes."""
    F, K, hop, T = 4, 2113, 500, 9000
    assert N.load().leaf_auto_algo(3, T, F, K, hop) == N.ALGO_STAGED
    for mode in MODES:
        m = module(F, K, hop, mode)
        x = waveform(3, T, xtype, seed=4)
        for algo in (N.ALGO_AUTO, N.ALGO_STAGED):
            check_forward(m, x, algo, f"staged/{mode}/algo={algo}")


def test_forward_serving_mode_peak_normalisation_and_mixup():
    m = module(40, 401, 160, "pcen")
    for xtype in XTYPES:
        for B, T in ((3, 16001), (24, 4000)):                 # (24 clips: AUTO takes the workgroup kernel, as does the prepared-tables call)
            x = waveform(B, T, xtype, seed=B + T)
            if xtype == torch.float32:
                x[1] *= 3.5                                   # a clip louder than 1: its scale is not 1
            with torch.no_grad():
                m.output_dtype(None)
                plain32 = m(x)
                m.cache_tables(); cached32 = m(x); m.cache_tables(False)
                m.fuse_peak_normalization(); folded32 = m(x); m.fuse_peak_normalization(False)
                perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
                lam = torch.rand(B, generator=torch.Generator().manual_seed(T))
                mixed32 = m.forward_mixup(x, perm, lam)
                m.output_dtype(BF)
                plain = m(x)
                m.cache_tables(); cached = m(x), m(x); m.cache_tables(False)
                m.fuse_peak_normalization(); folded = m(x); m.fuse_peak_normalization(False)
                mixed = m.forward_mixup(x, perm, lam)
                m.output_dtype(None)
            assert all(t.dtype == BF for t in (plain, *cached, folded, mixed))
            assert torch.equal(plain, plain32.to(BF))
            assert torch.equal(cached[0], cached32.to(BF)) and torch.equal(cached[1], cached32.to(BF))
            assert torch.equal(folded, folded32.to(BF))
            if xtype == torch.float32:
                assert not torch.equal(folded32, plain32)      # the loud clip was normalised
            assert torch.equal(mixed, mixed32.to(BF))
            prm = args_of(m)
            for algo in (N.ALGO_FFT_SMALL, N.ALGO_FFT_WG, N.ALGO_MFMA):      # mixed in the loads / on the mixed copy
                if not covered(B, T, 40, 401, 160, algo):
                    continue
                a = N.leaf_forward_mix(x, perm, lam, *prm, 401, 160, algo=algo, out_bf16=True)
                b = N.leaf_forward_mix(x, perm, lam, *prm, 401, 160, algo=algo)
                assert a.dtype == BF and torch.equal(a, b.to(BF)), (xtype, B, T, algo)


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------
# (name, F, K, hop, B, T, mode, keywords of leaf_backward)
BWD = [("16k-band", 40, 401, 160, 3, 4000, "pcen", {}),
       ("16k-band-T16001", 40, 401, 160, 1, 16001, "pcen", {}),
       ("16k-full", 40, 401, 160, 3, 4000, "pcen", {"full_transforms": True}),
       ("32k", 12, 801, 320, 3, 8200, "pcen", {}),
       ("22k-runtime", 12, 552, 220, 3, 4000, "pcen", {}),
       ("16k-mfma", 40, 401, 160, 3, 4000, "pcen", {"mfma": True}),
       ("16k-staged", 8, 401, 160, 3, 801, "pcen", {"staged": True}),
       ("16k-log1p", 40, 401, 160, 3, 4000, "log1p", {}),
       ("16k-off", 40, 401, 160, 1, 801, "off", {})]
# ... and at the clip lengths where a block load ends ragged (tests/test_gpu_backward_edges.py): one sample, one hop h, h + 1, and
# L - 1, L, L + 1 of the plan's block length L, on the per-wave kernel (three clips) and on the workgroup kernels (B = ("cus", s): one clip
# more than s/16 of a block per CU asks for)
EDGE_LENGTHS = lambda hop, L: (1, hop, hop + 1, L - 1, L, L + 1)
BWD += [(f"16k-per-wave-edge-T{T}", 40, 401, 160, 3, T, "pcen", {}) for T in EDGE_LENGTHS(160, 1600)]
BWD += [(f"16k-workgroup-edge-T{T}", 40, 401, 160, ("cus", 6), T, "pcen", {}) for T in EDGE_LENGTHS(160, 1600)]
BWD += [(f"32k-4096-edge-T{T}", 12, 801, 320, ("cus", 8), T, "pcen", {}) for T in EDGE_LENGTHS(320, 3200)]


def grad_out_bf16(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF).to(DEV)


def assert_same_grads(got, want, n, what):
    for i in range(n):
        assert got[i].dtype == torch.float32
        assert torch.equal(got[i], want[i]), f"{what}: d {GRAD_NAMES[i]} differs by {float((got[i] - want[i]).abs().max()):.3e}"


@pytest.mark.parametrize("xtype", XTYPES, ids=["f32", "pcm16"])
@pytest.mark.parametrize("case", BWD, ids=[c[0] for c in BWD])
def test_backward_equals_the_float32_backward_on_the_widened_gradient(case, xtype):
    name, F, K, hop, B, T, mode, kw = case
    if isinstance(B, tuple):
        B = n_cus() * B[1] // 16 + 1
    m = module(F, K, hop, mode, seed=3)
    prm = args_of(m)
    pcen, log1p = mode == "pcen", mode == "log1p"
    n = 7 if pcen else 3
    x = waveform(B, T, xtype, seed=11)
    out, raw = N.leaf_forward(x, *prm, K, hop, pcen=pcen, log1p=log1p, save_raw=True, out_bf16=True)
    go = grad_out_bf16(out.shape, 5)
    for dx in ((False, True) if xtype == torch.float32 else (False,)):
        for saved in (raw, None):                             # the saved pooled tensor, and the recompute
            k = dict(pcen=pcen, log1p=log1p, need_dx=dx, pooled_raw=saved, **kw)
            want = N.leaf_backward(x, *prm, K, hop, go.float(), **k)
            got = N.leaf_backward(x, *prm, K, hop, go, out_bf16=True, **k)
            what = f"{name}/{xtype}/dx={dx}/raw={'saved' if saved is not None else 'recomputed'}"
            assert all(torch.isfinite(t).all() for t in want[:n]), what
            assert_same_grads(got, want, n, what)
            if dx:
                assert got[7].dtype == torch.float32 and got[7].shape == want[7].shape
                assert torch.equal(got[7], want[7]), f"{what}: dL/dx differs by {float((got[7] - want[7]).abs().max()):.3e}"
            else:
                assert got[7] is None
    with pytest.raises(RuntimeError, match="grad_out must be float32"):       # the mode is explicit, never inferred
        N.leaf_backward(x, *prm, K, hop, go, pcen=pcen, log1p=log1p)
    with pytest.raises(RuntimeError, match="grad_out must be bfloat16"):
        N.leaf_backward(x, *prm, K, hop, go.float(), pcen=pcen, log1p=log1p, out_bf16=True)


@pytest.mark.parametrize("xtype", XTYPES, ids=["f32", "pcm16"])
@pytest.mark.parametrize("case", [BWD[0], BWD[3], BWD[4], BWD[5], BWD[6]], ids=[BWD[i][0] for i in (0, 3, 4, 5, 6)])
def test_mix_backward_equals_the_float32_mix_backward(case, xtype):
    """In the loads (static 16 / 32 kHz), and on the mixed copy (run-time geometry, MFMA, staged)."""
    name, F, K, hop, B, T, mode, kw = case
    m = module(F, K, hop, mode, seed=3)
    prm = args_of(m)
    x = waveform(B, T, xtype, seed=12)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1))
    lam = torch.rand(B, generator=torch.Generator().manual_seed(2))
    out, raw = N.leaf_forward_mix(x, perm, lam, *prm, K, hop, save_raw=True, out_bf16=True)
    out32, raw32 = N.leaf_forward_mix(x, perm, lam, *prm, K, hop, save_raw=True)
    assert out.dtype == BF and torch.equal(out, out32.to(BF)) and torch.equal(raw, raw32)
    go = grad_out_bf16(out.shape, 6)
    want = N.leaf_backward_mix(x, perm, lam, *prm, K, hop, go.float(), pooled_raw=raw, **kw)
    got = N.leaf_backward_mix(x, perm, lam, *prm, K, hop, go, pooled_raw=raw, out_bf16=True, **kw)
    assert_same_grads(got, want, 7, f"mix/{name}/{xtype}")
    lib = N.load()
    fl = PC | (PCM if xtype == torch.int16 else 0) | (N.FLAG_BWD_MFMA if kw.get("mfma") else 0) | (N.FLAG_BWD_STAGED if kw.get("staged") else 0)
    assert lib.leaf_backward_mix_workspace_bytes(B, T, F, K, hop, fl | OUT) == lib.leaf_backward_mix_workspace_bytes(B, T, F, K, hop, fl)
    assert lib.leaf_backward_workspace_bytes(B, T, F, K, hop, fl | OUT, 0) == lib.leaf_backward_workspace_bytes(B, T, F, K, hop, fl, 0)


def test_autograd_step_through_output_dtype_with_an_int16_batch():
    m = L.Leaf().to(DEV).output_dtype(BF)
    x16 = waveform(3, 16001, torch.int16, seed=21)
    out = m(x16)
    assert out.dtype == BF and out.requires_grad and tuple(out.shape) == (3, 40, 101)
    go = grad_out_bf16(out.shape, 22)
    out.backward(go)
    prm = args_of(m)
    o2, raw = N.leaf_forward(x16, *prm, 401, 160, save_raw=True, out_bf16=True)
    assert torch.equal(out.detach(), o2)
    want = N.leaf_backward(x16, *prm, 401, 160, go, pooled_raw=raw, out_bf16=True)
    c = m._compression
    for p, w, nm in zip((m._complex_conv._kernel, m._pooling.weights, m._pooling._bias, c.alpha, c.delta, c.root, c.ema._weights), want, GRAD_NAMES):
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), nm
        assert torch.equal(p.grad, w.reshape(p.grad.shape)), f"d {nm} differs from the explicit two-step by {float((p.grad - w.reshape(p.grad.shape)).abs().max()):.3e}"
    # a float32 waveform that asks for its gradient: float32, the float32 backward's on the widened gradient; mixup trains too
    m.zero_grad()
    x = waveform(2, 4000, torch.float32, seed=23).requires_grad_(True)
    y = m(x)
    g = grad_out_bf16(y.shape, 24)
    y.backward(g)
    o3, raw3 = N.leaf_forward(x.detach(), *prm, 401, 160, save_raw=True)
    w3 = N.leaf_backward(x.detach(), *prm, 401, 160, g.float(), pooled_raw=raw3, need_dx=True)
    assert y.dtype == BF and x.grad.dtype == torch.float32 and torch.equal(x.grad, w3[7].reshape(x.shape))
    assert torch.equal(m._complex_conv._kernel.grad, w3[0])
    m.zero_grad()
    perm, lam = torch.tensor([1, 2, 0]), torch.tensor([0.3, 0.9, 0.5])
    z = m.forward_mixup(x16, perm, lam)
    assert z.dtype == BF
    z.backward(go)
    _, rawm = N.leaf_forward_mix(x16, perm, lam, *prm, 401, 160, save_raw=True)
    wm = N.leaf_backward_mix(x16, perm, lam, *prm, 401, 160, go.float(), pooled_raw=rawm)
    assert torch.equal(m._complex_conv._kernel.grad, wm[0]) and torch.equal(c.alpha.grad, wm[3])
    # second order: refused, as for bfloat16 I/O
    m.zero_grad()
    y = m(waveform(1, 801, torch.float32, seed=25))
    (gk,) = torch.autograd.grad(y.float().sum(), m._complex_conv._kernel, create_graph=True)
    with pytest.raises(RuntimeError, match="bfloat16 features"):
        gk.sum().backward()


def test_autocast_mode_follows_the_autocast_region():
    m = module(40, 401, 160, "pcen").output_dtype("autocast")
    for xtype in XTYPES:
        x = waveform(2, 4000, xtype, seed=31)
        with torch.no_grad():
            outside = m(x)
            with torch.autocast("cuda", BF):
                inside = m(x)
            with torch.autocast("cuda", torch.float16):
                half = m(x)
            with torch.autocast("cuda", BF, enabled=False):
                disabled = m(x)
        assert outside.dtype == torch.float32 and half.dtype == torch.float32 and disabled.dtype == torch.float32
        assert inside.dtype == BF and torch.equal(inside, outside.to(BF))
    with pytest.raises(ValueError, match="not built"):
        m.output_dtype(torch.float32)(waveform(1, 801, torch.float32, seed=1).to(BF))
    assert m.output_dtype(None)(waveform(1, 801, torch.float32, seed=1).to(BF)).dtype == BF       # bfloat16 I/O as before


def test_ops_schema_fake_kernels_and_autograd_registration():
    m = module(40, 401, 160, "pcen")
    prm = args_of(m)
    ops = torch.ops.leaf_amd
    from leaf_pytorch_amd import _ops
    _ops.load()
    for xtype in XTYPES:
        x = waveform(2, 4000, xtype, seed=41)
        torch.library.opcheck(ops.forward.default, (x, *prm, 401, 160, False, 0), {"out_bf16": True}, test_utils=("test_schema", "test_faketensor"))
        torch.library.opcheck(ops.forward_train.default, (x, *prm, 401, 160, 0, False), {"out_bf16": True},
                              test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
        out, raw = ops.forward_train(x, *prm, 401, 160, 0, False, out_bf16=True)
        go = grad_out_bf16(out.shape, 42)
        torch.library.opcheck(ops.backward.default, (x, *prm, 401, 160, go, raw, xtype == torch.float32, 0), {"out_bf16": True},
                              test_utils=("test_schema", "test_faketensor"))
        perm, lam = torch.tensor([1, 0], dtype=torch.int32, device=DEV), torch.tensor([0.25, 0.75], device=DEV)
        torch.library.opcheck(ops.forward_mix.default, (x, perm, lam, *prm, 401, 160, False, 0), {"out_bf16": True},
                              test_utils=("test_schema", "test_faketensor"))
        torch.library.opcheck(ops.backward_mix.default, (x, perm, lam, *prm, 401, 160, go, None, 0), {"out_bf16": True},
                              test_utils=("test_schema", "test_faketensor"))
        with pytest.raises(RuntimeError, match="grad_out must be bfloat16"):
            ops.backward(x, *prm, 401, 160, go.float(), raw, False, 0, out_bf16=True)
        with pytest.raises(RuntimeError, match="grad_out must be float32"):
            ops.backward(x, *prm, 401, 160, go, raw, False, 0)


# ---- 3. the C ABI's memory contract with 2-byte features (tests/test_gpu_abi_memory.py, tests/guarded.py) ---------------------------
def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


ABI_FWD = [("small-401", 40, 401, 160, 2, 16001, N.ALGO_FFT_SMALL), ("fft-401", 40, 401, 160, 3, 4000, N.ALGO_FFT),
           ("wg-401", 40, 401, 160, 3, 16001, N.ALGO_FFT_WG), ("wg-401-stream", 40, 401, 160, 3, 16001, N.ALGO_FFT_WG | SFIN),
           ("wg4k-801", 12, 801, 320, 3, 8200, N.ALGO_FFT_WG), ("wgg-552", 12, 552, 220, 3, 16001, N.ALGO_FFT_WG),
           ("mfma-401", 40, 401, 160, 3, 16001, N.ALGO_MFMA)]


@pytest.mark.parametrize("xtype", XTYPES, ids=["f32", "pcm16"])
@pytest.mark.parametrize("case", ABI_FWD, ids=[c[0] for c in ABI_FWD])
def test_abi_forward_writes_exactly_its_two_byte_out_and_its_queried_workspace(case, xtype):
    name, F, K, hop, B, T, algo = case
    lib = N.load()
    m = module(F, K, hop, "pcen")
    prm = args_of(m)
    pp = [P(t) for t in prm]
    x = waveform(B, T, xtype, seed=51)
    TP = lib.leaf_num_frames(T, K, hop)
    flags = PC | OUT | (PCM if xtype == torch.int16 else 0)
    need = lib.leaf_workspace_bytes(B, T, F, K, hop, algo)
    assert need > 0
    want = N.leaf_forward(x, *prm, K, hop, algo=algo).to(BF)
    xg = guarded_tensor(x)
    for save in (False, True):
        for off in (0, 2):                                   # 4096-byte boundary, and 2 bytes past it: 2-byte aligned, not 4
            out = guarded(B * F * TP * 2, 0xFF, off)
            raw = guarded(B * F * TP * 4, 0xFF) if save else None
            ws = guarded(need, 0xFF)
            if save:
                rc = lib.leaf_forward_save_f32(xg.ptr, B, T, *pp, F, K, hop, flags, algo, out.ptr, raw.ptr, ws.ptr, need, None)
            else:
                rc = lib.leaf_forward_f32(xg.ptr, B, T, *pp, F, K, hop, flags, algo, out.ptr, ws.ptr, need, None)
            torch.cuda.synchronize()
            what = f"{name}/{xtype}/save={save}/off={off}"
            assert rc == 0, f"{what}: {lib.leaf_status_string(rc)}"
            out.check(what + " out"); ws.check(what + " workspace"); unchanged(xg, what + " x")
            got = out.cpu(torch.int16, (B, F, TP))
            assert torch.equal(got, want.cpu().view(torch.int16)), f"{what}: {int((got != want.cpu().view(torch.int16)).sum())} features differ"
            if save:
                raw.check(what + " pooled_raw")
                assert not bool((raw.cpu(torch.int32) == -1).any())
        # an odd address: refused before anything is touched; one word of workspace short: refused too
        out = guarded(B * F * TP * 2, 0xFF, 1)
        ws = guarded(need, 0x5A)
        assert lib.leaf_forward_f32(xg.ptr, B, T, *pp, F, K, hop, flags, algo, out.ptr, ws.ptr, need, None) == -7
        out2 = guarded(B * F * TP * 2, 0xFF)
        assert lib.leaf_forward_f32(xg.ptr, B, T, *pp, F, K, hop, flags, algo, out2.ptr, ws.ptr, need - 4, None) == -3
        torch.cuda.synchronize()
        for o in (out, out2):
            o.check(name + " refused out")
            assert bool((o.bytes() == 0xFF).all())
        assert bool((ws.bytes() == 0x5A).all())


def test_abi_refusals_touch_nothing():
    lib = N.load()
    F, K, hop, B, T = 8, 401, 160, 2, 801
    m = module(F, K, hop, "pcen", seed=1)
    pp = [P(t) for t in args_of(m)]
    TP = lib.leaf_num_frames(T, K, hop)
    x, x16 = guarded_tensor(waveform(B, T, torch.float32, 1)), guarded_tensor(waveform(B, T, torch.int16, 1))
    need = lib.leaf_workspace_bytes(B, T, F, K, hop, N.ALGO_STAGED)
    assert need > 0
    out, ws = guarded(B * F * TP * 2, 0xFF), guarded(need, 0x5A)
    # the staged forward has no bfloat16 store: LEAF_ERR_UNSUPPORTED, nothing written (with a full-size workspace, and with none)
    assert lib.leaf_forward_f32(x.ptr, B, T, *pp, F, K, hop, PC | OUT, N.ALGO_STAGED, out.ptr, ws.ptr, need, None) == -8
    assert lib.leaf_forward_f32(x.ptr, B, T, *pp, F, K, hop, PC | OUT, N.ALGO_STAGED, out.ptr, ws.ptr, 0, None) == -8
    assert lib.leaf_forward_mix_f32(x.ptr, pp[2], pp[2], B, T, *pp, F, K, hop, PC | OUT, N.ALGO_STAGED, out.ptr, ws.ptr, 0, None) == -8
    # two types for x: as before, with or without the new flag
    for extra in (0, OUT):
        assert lib.leaf_forward_f32(x16.ptr, B, T, *pp, F, K, hop, PC | IO | PCM | extra, N.ALGO_FFT, out.ptr, ws.ptr, need, None) == -8
    g = [guarded(n * 4, 0xFF) for n in (2 * F, F, F, F, F, F, F)]
    go = guarded(B * F * TP * 2, 0x3C)
    bneed = lib.leaf_backward_workspace_bytes(B, T, F, K, hop, PC | OUT, 0)
    bws = guarded(bneed, 0x5A)
    gp = [b.ptr for b in g]
    assert lib.leaf_backward_f32(x16.ptr, B, T, *pp, F, K, hop, PC | IO | PCM, go.ptr, None, *gp, None, bws.ptr, bneed, None) == -8
    # an odd grad_out address
    go_odd = guarded(B * F * TP * 2, 0x3C, 1)
    assert lib.leaf_backward_f32(x.ptr, B, T, *pp, F, K, hop, PC | OUT, go_odd.ptr, None, *gp, None, bws.ptr, bneed, None) == -7
    torch.cuda.synchronize()
    out.check("refused out"); ws.check("refused workspace"); bws.check("refused backward workspace")
    assert bool((out.bytes() == 0xFF).all()) and bool((ws.bytes() == 0x5A).all()) and bool((bws.bytes() == 0x5A).all())
    assert all(bool((b.bytes() == 0xFF).all()) for b in g)


ABI_BWD = [("b401", 40, 401, 160, 3, 4000, 0, False), ("b401-dx", 40, 401, 160, 2, 4000, 0, True), ("b801", 12, 801, 320, 2, 8200, 0, False),
           ("b552", 12, 552, 220, 2, 4000, 0, False), ("b401-mfma", 40, 401, 160, 2, 4000, N.FLAG_BWD_MFMA, False),
           ("b401-staged", 8, 401, 160, 2, 801, N.FLAG_BWD_STAGED, True)]


@pytest.mark.parametrize("case", ABI_BWD, ids=[c[0] for c in ABI_BWD])
def test_abi_backward_reads_a_two_byte_grad_out_and_writes_only_its_queried_workspace(case):
    name, F, K, hop, B, T, bflags, dx = case
    lib = N.load()
    m = module(F, K, hop, "pcen", seed=2)
    prm = args_of(m)
    pp = [P(t) for t in prm]
    kw = dict(mfma=bool(bflags & N.FLAG_BWD_MFMA), staged=bool(bflags & N.FLAG_BWD_STAGED))
    for xtype in (XTYPES if not dx else XTYPES[:1]):
        x = waveform(B, T, xtype, seed=61)
        TP = lib.leaf_num_frames(T, K, hop)
        gob = grad_out_bf16((B, F, TP), 62)
        want = N.leaf_backward(x, *prm, K, hop, gob.float(), need_dx=dx, **kw)
        flags = PC | OUT | bflags | (PCM if xtype == torch.int16 else 0)
        need = lib.leaf_backward_workspace_bytes(B, T, F, K, hop, flags, int(dx))
        assert need == lib.leaf_backward_workspace_bytes(B, T, F, K, hop, flags & ~OUT, int(dx)) > 0      # no widened copy of grad_out
        for off in (0, 2):
            xg, go = guarded_tensor(x), guarded_tensor(gob, off)
            g = [guarded(n * 4, 0xFF) for n in (2 * F, F, F, F, F, F, F)]
            gx = guarded(B * T * 4, 0xFF) if dx else None
            ws = guarded(need, 0xFF)
            rc = lib.leaf_backward_f32(xg.ptr, B, T, *pp, F, K, hop, flags, go.ptr, None, *[b.ptr for b in g], gx.ptr if dx else None,
                                       ws.ptr, need, None)
            torch.cuda.synchronize()
            what = f"{name}/{xtype}/off={off}"
            assert rc == 0, f"{what}: {lib.leaf_status_string(rc)}"
            unchanged(xg, what + " x"); unchanged(go, what + " grad_out"); ws.check(what + " workspace")
            for b, w, nm in zip(g, want, GRAD_NAMES):
                b.check(what + " d " + nm)
                assert torch.equal(b.cpu(torch.float32), w.cpu().reshape(-1)), f"{what}: d {nm}"
            if dx:
                gx.check(what + " g_x")
                assert torch.equal(gx.cpu(torch.float32, (B, T)), want[7].cpu().reshape(B, T)), what + ": g_x"
