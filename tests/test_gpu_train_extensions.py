"""Training through the two extensions of the forward: log1p compression (BASELINE configs[3]; ``Leaf.log_compression()``,
LEAF_FLAG_LOG1P in leaf_forward_save_f32 / leaf_backward_f32) and bfloat16 I/O (configs[4]; LEAF_FLAG_IO_BF16 in the same calls).

log1p: fp64 autograd through ``torch.log1p(oracle)`` is the reference, compared with helpers.assert_grad_close at its defaults
(the tolerances every PCEN-off backward test passes).  bfloat16: the reference has no bf16 path, so -- like
test_bf16_io_extension_matches_fp32_path_within_bf16_rounding -- parity is against this project's fp32 path on the same
bf16-valued tensors, and because widening is exact and neither the arithmetic nor the kernel choice depends on the I/O type, the
comparisons are equalities."""
import math

import pytest
import torch
import torch._dynamo

from conftest import rel_err
from helpers import assert_grad_close, make_leaf
from oracle import leaf_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 2e-5                     # the suite's forward tolerance (tests/test_gpu_parity.py)
NAMES = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
         "_compression.root", "_compression.ema._weights"]


def _params(F, K, hop, pcen, gen):
    geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
    params = lo.default_params(geo, pcen, kernel=torch.stack(
        [0.1 + torch.rand(F, generator=gen) * (math.pi - 0.2), 3.0 + torch.rand(F, generator=gen) * K / 4], dim=1))
    return geo, {k: v * (1 + 0.1 * (2 * torch.rand(v.shape, generator=gen) - 1)) for k, v in params.items()}


def _args(m, pcen):
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    return [sd[n] for n in NAMES[:3]] + ([sd[n] for n in NAMES[3:]] if pcen else [None] * 4)


def _oracle_log1p_grads(x, params, geo, grad_out, need_dx):
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().requires_grad_(need_dx)
    out = torch.log1p(lo.leaf_forward(x64, p64, geo, False, torch.float64))
    out.backward(grad_out.double())
    return {k: v.grad for k, v in p64.items()}, (x64.grad if need_dx else None)


def log1p_case(F, K, hop, T, B, seed, need_dx=False, full=False, forced=(), params=None, x=None):
    """Gradients of Leaf(pcen_compression=False).log_compression() against fp64 autograd through log1p(oracle)."""
    from leaf_pytorch_amd import _native
    gen = torch.Generator().manual_seed(seed)
    geo, p = _params(F, K, hop, False, gen)
    params = p if params is None else params
    if x is None:
        x = torch.randn(B, 1, T, generator=gen)
    m = make_leaf(F, K, hop, False, params, DEV).log_compression()
    if full:
        m.full_transforms()
    for q in m.parameters():
        q.requires_grad_(True)
    xd = x.to(DEV).requires_grad_(need_dx)
    out = m(xd)
    grad_out = torch.randn(out.shape, generator=gen)
    out.backward(grad_out.to(DEV))
    ref, ref_dx = _oracle_log1p_grads(x, params, geo, grad_out, need_dx)
    got = {k: v.grad.cpu() for k, v in m.named_parameters()}
    ctx = f"(log1p F={F} K={K} hop={hop} T={T} B={B} dx={need_dx} full={full} seed={seed})"
    for k in ref:
        assert got[k].shape == ref[k].shape, k
        assert_grad_close(k, got[k], ref[k], ctx)
    if need_dx:
        assert_grad_close("x", xd.grad, ref_dx, ctx, entrywise=False)
    for label in forced:                       # the same through a forced backward family (it recomputes the pooled tensor itself)
        grads = _native.leaf_backward(x.to(DEV), *_args(m, False), K, hop, grad_out.to(DEV), pcen=False, log1p=True,
                                      need_dx=need_dx, **{label: True})
        for name, gs in zip(NAMES[:3], grads[:3]):
            assert_grad_close(name, gs, ref[name], label + " " + ctx)
        if need_dx:
            assert_grad_close("x", grads[7].reshape(x.shape), ref_dx, label + " " + ctx, entrywise=False)
    return got, (xd.grad.cpu() if need_dx else None)


# ---------------------------------------------------------------------------------------------------------------------------
# log1p
# ---------------------------------------------------------------------------------------------------------------------------

def test_log1p_forward_through_the_module():
    """(1) The module switch reaches the fused forward: bit-equal to the ctypes call with log1p=True for the same selector, within
    the suite's forward tolerance of log1p(oracle); also in serving mode, with the folded PeakNormalization, with bf16 input."""
    from leaf_pytorch_amd import _native
    torch.manual_seed(4)
    geo = lo.geometry()
    params = lo.default_params(geo, pcen_compression=False)
    x = torch.randn(2, 1, 8000)
    m = make_leaf(40, 401, 160, False, params, DEV).log_compression()
    with torch.no_grad():
        out = m(x.to(DEV))
    want = _native.leaf_forward(x.to(DEV), *_args(m, False), 401, 160, pcen=False, log1p=True)
    assert torch.equal(out, want)
    ref = torch.log1p(lo.leaf_forward(x, params, geo, False, torch.float32))
    assert rel_err(out.cpu(), ref) < REL_TOL
    plain = make_leaf(40, 401, 160, False, params, DEV)
    with torch.no_grad():
        assert not torch.equal(plain(x.to(DEV)), out)                       # the switch is per module, off by default
        assert torch.equal(m.log_compression(False)(x.to(DEV)), plain(x.to(DEV)))
        m.log_compression()
        assert torch.equal(m.cache_tables()(x.to(DEV)), out)                 # prepared tables take the flag
        m.cache_tables(False)
        loud = 3 * x.to(DEV)
        peak = m.fuse_peak_normalization()(loud)
        m.fuse_peak_normalization(False)
        from leaf_pytorch_amd.transforms import PeakNormalization
        assert rel_err(peak.cpu(), m(PeakNormalization()(loud)).cpu()) < REL_TOL
        xb = x.to(torch.bfloat16).to(DEV)
        assert torch.equal(m(xb), m(xb.float()).to(torch.bfloat16))
    torch._dynamo.reset()
    compiled = torch.compile(m, fullgraph=True, backend="aot_eager")
    with torch.no_grad():
        assert torch.equal(compiled(x.to(DEV)), out)


@pytest.mark.parametrize("need_dx", [False, True])
def test_log1p_backward_default_geometry(need_dx):
    """(2) 16 kHz geometry, with and without dL/dx; the forced staged backward on the same case."""
    log1p_case(40, 401, 160, 2400, 2, seed=1, need_dx=need_dx, forced=("staged",))


def test_log1p_backward_many_blocks():
    log1p_case(40, 401, 160, 16000, 3, seed=11)
    log1p_case(40, 401, 160, 4801, 2, seed=12)
    log1p_case(40, 401, 160, 1599, 2, seed=13)


@pytest.mark.parametrize("need_dx", [False, True])
def test_log1p_backward_band_tasks_and_full_transforms(need_dx):
    """A batch whose backward runs the workgroup kernel with band tasks (16 clips of 1 s = 160 blocks), and the same with
    ``full_transforms()``."""
    gen = torch.Generator().manual_seed(31)
    geo = lo.geometry()
    params = lo.default_params(geo, pcen_compression=False)
    x = 2 * torch.rand(16, 1, 16000, generator=gen) - 1
    log1p_case(40, 401, 160, 16000, 16, seed=31, need_dx=need_dx, params=params, x=x)
    log1p_case(40, 401, 160, 16000, 16, seed=31, need_dx=need_dx, full=True, params=params, x=x)


def test_log1p_backward_other_families():
    """The 32 kHz geometry on 4096-sample blocks, a run-time geometry (22.05 kHz: K = 552, even), a short window on the MFMA
    backward (also forced), the forced staged backward with dL/dx."""
    from leaf_pytorch_amd import _native
    lib = _native.load()
    assert lib.leaf_backward_workspace_bytes(60, 7000, 3, 801, 320, _native.FLAG_LOG1P, 0) == \
        lib.leaf_backward_workspace_bytes(60, 7000, 3, 801, 320, 0, 0)         # no extra buffer for log1p
    log1p_case(3, 801, 320, 7000, 60, seed=81)
    log1p_case(6, 552, 220, 9000, 40, seed=51)
    log1p_case(6, 552, 220, 9000, 2, seed=52, need_dx=True)
    log1p_case(8, 31, 50, 400, 2, seed=4, forced=("mfma", "staged"))
    log1p_case(8, 31, 50, 400, 2, seed=4, need_dx=True)


@pytest.mark.parametrize("B", [1, 2, 3])
def test_log1p_backward_smallest_batches(B):
    log1p_case(40, 401, 160, 3000, B, seed=20 + B)


def test_log1p_backward_long_rows_cross_scan_chunks():
    """More than 128 frames per clip: the first-stage kernel walks several 128-frame chunks per row (overlap-save and MFMA)."""
    log1p_case(6, 401, 160, 25000, 1, seed=15)
    log1p_case(8, 31, 50, 14000, 1, seed=16)


def test_log1p_floor_gate_gives_exact_zeros():
    """(3) Pooling bias -50: every frame sits on the 1e-5 floor, log1p(max(., 1e-5)) is constant there, and every gradient is
    exactly zero -- what autograd through the oracle gives."""
    gen = torch.Generator().manual_seed(7)
    geo = lo.geometry()
    params = lo.default_params(geo, pcen_compression=False)
    params["_pooling._bias"] = torch.full_like(params["_pooling._bias"], -50.0)
    x = torch.randn(2, 1, 4000, generator=gen)
    got, gx = log1p_case(40, 401, 160, 4000, 2, seed=7, need_dx=True, params=params, x=x)
    ref, ref_dx = _oracle_log1p_grads(x, params, geo, torch.randn(2, 40, 25, generator=gen), True)
    assert all(float(v.abs().max()) == 0.0 for v in ref.values()) and float(ref_dx.abs().max()) == 0.0
    assert all(float(v.abs().max()) == 0.0 for v in got.values()) and float(gx.abs().max()) == 0.0


@pytest.mark.parametrize("B,T,need_dx", [(2, 2400, True), (16, 16000, False), (16, 16000, True)])
def test_log1p_backward_is_the_plain_backward_of_the_divided_gradient(B, T, need_dx):
    """(4) Chain rule, bit level: the kernels DIVIDE grad_out by (1 + raw) above the floor (no reciprocal), so the log1p backward
    equals, bit for bit, the PCEN-off backward fed that quotient computed in fp32 on the device with the floor gate applied."""
    from leaf_pytorch_amd import _native
    torch.manual_seed(41)
    m = make_leaf(40, 401, 160, False, lo.default_params(lo.geometry(), pcen_compression=False), DEV)
    a = _args(m, False)
    x = 2 * torch.rand(B, 1, T, device=DEV) - 1
    out, raw = _native.leaf_forward(x, *a, 401, 160, pcen=False, log1p=True, save_raw=True)
    assert torch.equal(out, torch.log1p(raw.clamp_min(1e-5))) or rel_err(out.cpu(), torch.log1p(raw.clamp_min(1e-5)).cpu()) < REL_TOL
    go = torch.randn_like(out)
    got = _native.leaf_backward(x, *a, 401, 160, go, pcen=False, log1p=True, need_dx=need_dx, pooled_raw=raw)
    floor = torch.tensor(1e-5, device=DEV)
    divided = torch.where(raw > floor, go / (1.0 + torch.maximum(raw, floor)), torch.zeros_like(go))
    want = _native.leaf_backward(x, *a, 401, 160, divided, pcen=False, log1p=False, need_dx=need_dx, pooled_raw=raw)
    for i in (0, 1, 2) + ((7,) if need_dx else ()):
        assert torch.equal(got[i], want[i]), i
    assert float(got[0].abs().max()) > 0


def test_log1p_module_surface():
    """(5) ValueError on a PCEN module; no parameter, no buffer; opcheck on the extended ops; LeafStream picks the switch up."""
    import leaf_pytorch_amd as L
    from leaf_pytorch_amd import _native, _ops
    with pytest.raises(ValueError):
        L.Leaf().log_compression()
    assert L.Leaf().log_compression(False) is not None                        # switching it off is always allowed
    plain, logm = L.Leaf(pcen_compression=False), L.Leaf(pcen_compression=False).log_compression()
    assert list(plain.state_dict().keys()) == list(logm.state_dict().keys())
    assert [n for n, _ in logm.named_buffers()] == [n for n, _ in plain.named_buffers()]
    logm.load_state_dict(plain.state_dict(), strict=True)
    _ops.load()
    torch.manual_seed(9)
    m = make_leaf(40, 401, 160, False, lo.default_params(lo.geometry(), pcen_compression=False), DEV)
    prm = _args(m, False)
    x = torch.randn(3, 1, 4000, device=DEV)
    out, raw = torch.ops.leaf_amd.forward_train(x, *prm, 401, 160, 0, True)
    assert torch.equal(out, _native.leaf_forward(x, *prm, 401, 160, pcen=False, log1p=True))
    go = torch.randn_like(out)
    via_op = torch.ops.leaf_amd.backward(x, *prm, 401, 160, go, raw, True, _native.FLAG_LOG1P)
    via_ctypes = _native.leaf_backward(x, *prm, 401, 160, go, pcen=False, log1p=True, need_dx=True, pooled_raw=raw)
    for i in (0, 1, 2, 7):
        assert torch.equal(via_op[i].reshape(-1), via_ctypes[i].reshape(-1)), i
    req = [p.clone().requires_grad_(True) for p in prm[:3]] + [None] * 4
    torch.library.opcheck(torch.ops.leaf_amd.forward_train.default, (x, *req, 401, 160, 0, True),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    xb, gb = x.to(torch.bfloat16), go.to(torch.bfloat16)
    torch.library.opcheck(torch.ops.leaf_amd.forward_train.default, (xb, *req, 401, 160, 0, True),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    torch.library.opcheck(torch.ops.leaf_amd.backward.default, (xb, *prm, 401, 160, gb, raw, True, _native.FLAG_LOG1P),
                          test_utils=("test_schema", "test_faketensor"))
    # LeafStream over chunks == the one-shot log1p forward (the module's switch; tolerance: STREAM_TOL of tests/test_gpu_dropin.py)
    ml = L.Leaf(pcen_compression=False).log_compression().eval().to(DEV)
    T = int(2.3 * 16000) + 7
    xs = torch.randn(2, 1, T, device=DEV)
    with torch.no_grad():
        want = ml(xs)
    s = L.LeafStream(ml)
    outs, pos, i, sizes = [], 0, 0, [1, 37, 160, 5, 4000, 16003, 2, 8000]
    while pos < T:
        n = min(sizes[i % len(sizes)], T - pos)
        outs.append(s.step(xs[:, :, pos:pos + n]))
        pos += n
        i += 1
    outs.append(s.flush())
    got = torch.cat(outs, dim=-1)
    assert got.shape == want.shape and rel_err(got.cpu(), want.cpu()) < REL_TOL
    assert rel_err(got.cpu(), torch.log1p(L.Leaf(pcen_compression=False).eval().to(DEV)(xs)).cpu()) < REL_TOL


def test_log1p_training_step_is_hip_graph_capturable():
    """(5) Forward + backward with log compression captured into one HIP graph replay the eager step's gradients bit for bit."""
    from leaf_pytorch_amd import Leaf
    for B, need_dx in ((2, False), (16, True)):
        torch.manual_seed(B)
        m = Leaf(pcen_compression=False).log_compression().to(DEV)
        xs = [(2 * torch.rand(B, 1, 16000, device=DEV) - 1) for _ in range(2)]
        go = torch.randn(B, 40, 100, device=DEV)
        static_x = xs[0].clone().requires_grad_(need_dx)

        def step():
            torch.autograd.backward(m(static_x), go)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                m.zero_grad(set_to_none=True)
                static_x.grad = None
                step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        m.zero_grad(set_to_none=True)
        static_x.grad = None
        with torch.cuda.graph(graph):
            step()
        for x in xs:
            with torch.no_grad():
                static_x.copy_(x)
            graph.replay()
            got = [p.grad.clone() for p in m.parameters()] + ([static_x.grad.clone()] if need_dx else [])
            m2 = Leaf(pcen_compression=False).log_compression().to(DEV)
            m2.load_state_dict(m.state_dict())
            xe = x.clone().requires_grad_(need_dx)
            torch.autograd.backward(m2(xe), go)
            want = [p.grad for p in m2.parameters()] + ([xe.grad] if need_dx else [])
            for a, b in zip(got, want):
                assert torch.equal(a, b), (B, need_dx)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_empty_batch_under_grad_with_the_extensions(dtype):
    """(6) B = 0 under grad: zero parameter gradients and an empty dL/dx, with log compression and with bf16 I/O."""
    from leaf_pytorch_amd import Leaf
    for m in (Leaf(pcen_compression=False).log_compression().to(DEV), Leaf().to(DEV)):
        x = torch.zeros(0, 1, 16000, device=DEV, dtype=dtype).requires_grad_(True)
        out = m(x)
        assert out.shape == (0, 40, 100) and out.dtype == dtype
        out.sum().backward()
        assert x.grad.shape == x.shape and x.grad.dtype == dtype
        for p in m.parameters():
            assert p.grad is not None and p.grad.dtype == torch.float32 and float(p.grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# bfloat16 I/O
# ---------------------------------------------------------------------------------------------------------------------------

def bf16_case(F, K, hop, T, B, mode, need_dx, seed, x_scale=1.0):
    """Forward + backward on bf16 tensors == the fp32 path on the same (widened) tensors: out and dL/dx after round-to-nearest-even,
    the saved pooled tensor and every parameter gradient bit for bit."""
    from leaf_pytorch_amd import _native
    pcen, log1p = mode == "pcen", mode == "log1p"
    gen = torch.Generator().manual_seed(seed)
    geo, params = _params(F, K, hop, pcen, gen)
    m = make_leaf(F, K, hop, pcen, params, DEV)
    if log1p:
        m.log_compression()
    for q in m.parameters():
        q.requires_grad_(True)
    xb = (x_scale * torch.randn(B, 1, T, generator=gen)).to(torch.bfloat16).to(DEV)
    TP = (T - 1) // hop + 1
    gb = torch.randn(B, F, TP, generator=gen).to(torch.bfloat16).to(DEV)
    ctx = f"(bf16 F={F} K={K} hop={hop} T={T} B={B} {mode} dx={need_dx})"
    a = _args(m, pcen)
    out_b, raw_b = _native.leaf_forward(xb, *a, K, hop, pcen=pcen, log1p=log1p, save_raw=True)
    out_f, raw_f = _native.leaf_forward(xb.float(), *a, K, hop, pcen=pcen, log1p=log1p, save_raw=True)
    assert out_b.dtype == torch.bfloat16 and raw_b.dtype == torch.float32
    assert torch.equal(raw_b, raw_f), ctx
    assert torch.equal(out_b, out_f.to(torch.bfloat16)), ctx
    # through the module (autograd): bf16 features, bf16 dL/dx, fp32 parameter gradients
    xg = xb.clone().requires_grad_(need_dx)
    y = m(xg)
    assert y.dtype == torch.bfloat16 and torch.equal(y, out_b), ctx
    y.backward(gb)
    got = [q.grad.clone() for q in m.parameters()]
    assert all(g.dtype == torch.float32 for g in got)
    m.zero_grad(set_to_none=True)
    xf = xb.float().requires_grad_(need_dx)
    m(xf).backward(gb.float())
    want = [q.grad for q in m.parameters()]
    for (name, _), g, w in zip(m.named_parameters(), got, want):
        assert torch.equal(g, w), (name, float((g - w).abs().max()), ctx)
    assert float(got[0].abs().max()) > 0
    if need_dx:
        assert xg.grad.dtype == torch.bfloat16 and xg.grad.shape == xb.shape
        assert torch.equal(xg.grad, xf.grad.to(torch.bfloat16)), ctx
    # the backward recomputing the pooled tensor itself from the bf16 waveform (no pooled_raw), C ABI through ctypes
    r_b = _native.leaf_backward(xb, *a, K, hop, gb, pcen=pcen, log1p=log1p, need_dx=need_dx)
    r_f = _native.leaf_backward(xb.float(), *a, K, hop, gb.float(), pcen=pcen, log1p=log1p, need_dx=need_dx)
    for i in range(7):
        if r_f[i] is not None:
            assert r_b[i].dtype == torch.float32 and torch.equal(r_b[i], r_f[i]), (i, ctx)
    if need_dx:
        assert torch.equal(r_b[7], r_f[7].to(torch.bfloat16)), ctx


@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("mode", ["pcen", "off", "log1p"])
def test_bf16_training_static_16k_geometry(mode, need_dx):
    """(7) K = 401 / hop = 160, the kernels that read the bf16 waveform directly: a small batch (one wave per block), and 16 clips of
    1 s (the workgroup kernel with band tasks; its dL/dx instance)."""
    bf16_case(40, 401, 160, 2400, 2, mode, need_dx, seed=1)
    bf16_case(40, 401, 160, 16000, 16, mode, need_dx, seed=2)


@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("mode", ["pcen", "off", "log1p"])
@pytest.mark.parametrize("T", [1, 160, 161, 1599, 1600, 1601])
def test_bf16_training_static_16k_geometry_at_clip_edges(T, mode, need_dx):
    """(7) at the clip lengths where a block load ends ragged (tests/test_gpu_backward_edges.py): one sample, one hop, one more, and
    L - 1, L, L + 1 of the 1600-sample block -- at odd T a clip's 16-bit row does not start on a 4-byte boundary.  Two clips (one wave
    per block) and one clip more than 6/16 of a block per CU asks for (the workgroup kernel)."""
    bf16_case(40, 401, 160, T, 2, mode, need_dx, seed=3)
    bf16_case(40, 401, 160, T, torch.cuda.get_device_properties(DEV).multi_processor_count * 6 // 16 + 1, mode, need_dx, seed=4)


@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("mode", ["pcen", "off", "log1p"])
@pytest.mark.parametrize("T", [1, 320, 321, 3199, 3200, 3201])
def test_bf16_training_static_32k_geometry_at_clip_edges(T, mode, need_dx):
    """The same on the 4096-sample blocks of the 32 kHz geometry (L = 3200): one clip more than 8/16 of a block per CU asks for."""
    bf16_case(3, 801, 320, T, torch.cuda.get_device_properties(DEV).multi_processor_count * 8 // 16 + 1, mode, need_dx, seed=82)


@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("mode", ["pcen", "off", "log1p"])
def test_bf16_training_other_families(mode, need_dx):
    """(7) 32 kHz geometry on 4096-sample blocks (direct loads), a run-time geometry (K = 552, even; the workgroup kernel and the one wave
    per block kernel) and a short window (MFMA backward without dL/dx, staged with it): the last two through one widening pass, then
    the fp32 kernels.  No family picks a different kernel for bf16 than for fp32, so every comparison is an equality."""
    from leaf_pytorch_amd import _native
    lib = _native.load()
    bf16_case(3, 801, 320, 7000, 60, mode, need_dx, seed=81)
    bf16_case(6, 552, 220, 9000, 40, mode, need_dx, seed=51)
    bf16_case(6, 552, 220, 9000, 2, mode, need_dx, seed=52)
    bf16_case(8, 31, 50, 400, 2, mode, need_dx, seed=4)
    fl = (_native.FLAG_PCEN if mode == "pcen" else 0) | _native.FLAG_IO_BF16
    plain = lib.leaf_backward_workspace_bytes(2, 400, 8, 31, 50, fl & ~_native.FLAG_IO_BF16, int(need_dx))
    assert lib.leaf_backward_workspace_bytes(2, 400, 8, 31, 50, fl, int(need_dx)) == plain + 4 * 832     # the widened copy: 2 x 400 floats, 64-aligned


def test_bf16_forced_backward_families():
    """No combination answers LEAF_ERR_UNSUPPORTED: the forced staged and MFMA backwards take bf16 through the widening pass and
    equal their fp32 runs."""
    from leaf_pytorch_amd import _native
    torch.manual_seed(3)
    m = make_leaf(40, 401, 160, True, lo.default_params(lo.geometry()), DEV)
    a = _args(m, True)
    xb = torch.randn(2, 1, 2400, device=DEV).to(torch.bfloat16)
    gb = torch.randn(2, 40, 15, device=DEV).to(torch.bfloat16)
    for kw in (dict(staged=True), dict(staged=True, need_dx=True), dict(mfma=True), dict(full_transforms=True, need_dx=True),
               dict(strict_band_classes=True)):
        r_b = _native.leaf_backward(xb, *a, 401, 160, gb, **kw)
        r_f = _native.leaf_backward(xb.float(), *a, 401, 160, gb.float(), **kw)
        for i in range(7):
            assert torch.equal(r_b[i], r_f[i]), (i, kw)
        if kw.get("need_dx"):
            assert r_b[7].dtype == torch.bfloat16 and torch.equal(r_b[7], r_f[7].to(torch.bfloat16)), kw
    with pytest.raises(RuntimeError):
        _native.leaf_backward(xb, *a, 401, 160, gb.float())                  # grad_out must match the I/O type


def test_bf16_second_order_raises_clearly():
    from leaf_pytorch_amd import Leaf
    m = Leaf().to(DEV)
    xb = torch.randn(2, 1, 4000, device=DEV).to(torch.bfloat16).requires_grad_(True)
    y = m(xb)
    (gx,) = torch.autograd.grad(y.float().pow(2).sum(), xb, create_graph=True)
    with pytest.raises(RuntimeError, match="bfloat16"):
        gx.float().pow(2).sum().backward()


def test_bf16_full_size_configs4_shape():
    """(9) BASELINE configs[4]'s per-GPU shape, 256 clips of 10 s in bf16, forward + backward with dL/dx: finite gradients, and the first
    and the last clip computed on their own through the fp32 path give the batch's rows of the features and of dL/dx (after rounding to
    bf16).  The selector is pinned (LEAF_ALGO_FFT_WG): under AUTO one clip alone lands on another kernel family than 256, and only within
    one family are a clip's bits independent of its batch (include/leaf_hip.h, LEAF_ALGO_AUTO)."""
    from leaf_pytorch_amd import Leaf, _native
    torch.manual_seed(0)
    m = Leaf().to(DEV)
    m._algo = _native.ALGO_FFT_WG
    B, T = 256, 160000
    xb = (2 * torch.rand(B, 1, T, device=DEV) - 1).to(torch.bfloat16).requires_grad_(True)
    gb = torch.randn(B, 40, 1000, device=DEV).to(torch.bfloat16)
    y = m(xb)
    assert y.dtype == torch.bfloat16 and y.shape == (B, 40, 1000)
    y.backward(gb)
    assert xb.grad.dtype == torch.bfloat16 and bool(torch.isfinite(xb.grad.float()).all())
    for p in m.parameters():
        assert p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    for b in (0, B - 1):
        xf = xb[b:b + 1].detach().float().requires_grad_(True)
        yf = m(xf)
        assert torch.equal(y[b:b + 1], yf.to(torch.bfloat16)), b
        yf.backward(gb[b:b + 1].float())
        assert torch.equal(xb.grad[b:b + 1], xf.grad.to(torch.bfloat16)), b


def test_bf16_log1p_training_loop_lowers_the_loss():
    """(10) A few SGD steps on bf16 clips with log compression: fp32 parameters, bf16 features."""
    from leaf_pytorch_amd import Leaf
    torch.manual_seed(0)
    m = Leaf(pcen_compression=False).log_compression().to(DEV)
    x = torch.randn(4, 1, 4000, device=DEV).to(torch.bfloat16)
    target = torch.zeros(4, 40, 25, device=DEV)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        out = m(x)
        assert out.dtype == torch.bfloat16
        loss = ((out.float() - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0]
