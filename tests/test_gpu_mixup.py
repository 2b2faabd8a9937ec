"""Waveform mixup folded into the frontend (``Leaf.forward_mixup``, the leaf_*_mix_f32 entries, ``_native.mixup``).

The oracle of every case is the SAME module called as ``forward(mixed)``, with ``mixed`` computed by the definition in torch fp32
(x * lam + x[perm] * (1 - lam), separately rounded), and the assertion is ``torch.equal``: a kernel that mixes in its loads must hand
its transforms the same bits, and a family that reads the mixed copy trivially does.  Both calls are served by the same kernel family
everywhere (the selector and the batch are the same; a MIX instance of a kernel differs from the plain one in its block load
only), so no case needs the looser fp64 comparison; one forward and one backward are
additionally held to the fp64 oracle with the suite's existing bounds."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import rel_err
from guarded import guarded, guarded_tensor, unchanged
from helpers import assert_grad_close, make_leaf
from oracle import leaf_oracle as lo
from leaf_pytorch_amd import _native, transforms
import leaf_pytorch_amd as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REL_TOL = 2e-5                                        # tests/test_gpu_parity.py: the float path's bound against the oracle
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixup", "mixup_b6.npz")
GRAD_NAMES = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
              "_compression.root", "_compression.ema._weights"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    _native.load()


def mix_definition(x, perm, lam):
    lam = lam.to(torch.float32).view(-1, *([1] * (x.dim() - 1)))
    om = 1 - lam
    return x * lam + x[perm.long()] * om


def module(F, K, hop, pcen, seed=0):
    torch.manual_seed(seed)
    kernel = torch.stack([0.2 + 2.5 * torch.rand(F), 6.0 + torch.rand(F) * K / 4], dim=1)
    geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
    params = lo.default_params(geo, pcen, kernel=kernel)
    return make_leaf(F, K, hop, pcen, params, DEV), params, geo


def args_of(m):
    c = m._compression
    return (m._complex_conv._kernel.detach(), m._pooling.weights.detach(), m._pooling._bias.detach(),
            *((c.alpha.detach(), c.delta.detach(), c.root.detach(), c.ema._weights.detach()) if c is not None else (None,) * 4))


def mix_draw(B, seed):
    """A permutation with a fixed point (clip 0) and a 2-cycle (1 <-> 2) where the batch allows, and weights that include 0, 1 and
    0.5 next to random ones."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.arange(B)
    if B >= 3:
        perm[1], perm[2] = 2, 1
    if B > 3:
        rest = torch.arange(3, B)
        perm[3:] = rest.roll(1)
    lam = torch.rand(B, generator=g)
    for i, v in enumerate((0.5, 0.0, 1.0)[:B]):
        lam[i] = v
    return perm, lam


def batch(B, T, seed, int16=False):
    """Samples in 2^-10 <= |x| < 1 (no product with a weight from mix_draw is subnormal), or their int16 quantisation."""
    g = torch.Generator().manual_seed(seed)
    x = (2 * torch.rand(B, 1, T, generator=g) - 1) * 0.98
    x = torch.where(x.abs() < 2.0 ** -10, torch.full_like(x, 0.125), x)
    return torch.round(x * 32767).to(torch.int16) if int16 else x


def as_float(x):
    return x.float() / 32768 if x.dtype == torch.int16 else x


# (name, F, K, hop, B, T, selector, mixes in its loads): every family of the issue's table.  Both routes give torch.equal, so which
# one served a case is pinned through the workspace query: a kernel that mixes in its loads asks for nothing beyond the plain call's
# workspace, the copy route for at least the mixed fp32 batch more.
FWD_CASES = [
    ("fft_small-auto", 40, 401, 160, 3, 4001, _native.ALGO_AUTO, True),
    ("fft-per-wave", 40, 401, 160, 5, 4001, _native.ALGO_FFT, True),
    ("fft-per-wave-8k", 40, 201, 80, 5, 4001, _native.ALGO_FFT, True),
    ("fft_wg-16k-ragged", 40, 401, 160, 5, 4001, _native.ALGO_FFT_WG, True),
    ("fft_wg-16k-short", 40, 401, 160, 5, 801, _native.ALGO_FFT_WG, True),
    ("fft_wg-32k-4096", 8, 801, 320, 3, 6401, _native.ALGO_FFT_WG, True),
    ("fft_wg-8k", 40, 201, 80, 5, 4001, _native.ALGO_FFT_WG, True),
    ("fft_wg-runtime-even", 8, 552, 220, 3, 4001, _native.ALGO_FFT_WG, False),
    ("fft_wg-runtime-1201", 8, 1201, 480, 3, 9001, _native.ALGO_FFT_WG, True),      # the 4096-sample plan, run-time geometry
    ("fft-per-wave-runtime", 8, 552, 220, 3, 4001, _native.ALGO_FFT, False),
    ("mfma", 40, 401, 160, 3, 4001, _native.ALGO_MFMA, False),
    ("staged", 8, 401, 160, 3, 1501, _native.ALGO_STAGED, False),
]


@pytest.mark.parametrize("int16", [False, True], ids=["fp32", "int16"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward_mixup_equals_forward_of_the_mixed_batch(case, int16):
    name, F, K, hop, B, T, algo, in_loads = case
    lib = _native.load()
    plain_ws = lib.leaf_workspace_bytes(B, T, F, K, hop, algo)
    assert plain_ws > 0, "the selector has no kernel at this shape"
    mix_ws = lib.leaf_forward_mix_workspace_bytes(B, T, F, K, hop, algo)
    assert (mix_ws == plain_ws) if in_loads else (mix_ws >= plain_ws + B * T * 4), (name, plain_ws, mix_ws)
    if name == "fft_small-auto":
        assert lib.leaf_auto_algo(B, T, F, K, hop) == _native.ALGO_FFT_SMALL
    x = batch(B, T, seed=K + T, int16=int16).to(DEV)
    perm, lam = mix_draw(B, seed=T)
    mixed = mix_definition(as_float(x), perm.to(DEV), lam.to(DEV))
    for mode in ("pcen", "off", "log1p"):
        m, _, _ = module(F, K, hop, mode == "pcen")
        if mode == "log1p":
            m.log_compression()
        for extra in (0, _native.ALGO_FULL_TRANSFORMS):           # band tasks on / full_transforms()
            m._algo = algo | extra
            with torch.no_grad():
                got = m.forward_mixup(x, perm, lam)                 # perm, lam from the CPU: validated, then moved
                want = m(mixed)
            assert got.dtype == torch.float32 and got.shape == want.shape
            assert torch.equal(got, want), f"{name}/{mode}/extra={extra:#x}: max diff {float((got - want).abs().max()):.3e}"
        # the training forward through the C ABI: features and the saved pooled tensor
        prm = args_of(m)
        o, r = _native.leaf_forward_mix(x, perm, lam, *prm, K, hop, pcen=mode == "pcen", log1p=mode == "log1p", algo=algo, save_raw=True)
        o2, r2 = _native.leaf_forward(mixed, *prm, K, hop, pcen=mode == "pcen", log1p=mode == "log1p", algo=algo, save_raw=True)
        assert torch.equal(o, o2) and torch.equal(r, r2), f"{name}/{mode}: training forward"


def test_forward_mixup_matches_the_fp64_oracle_and_a_device_perm_is_clamped():
    F, K, hop, B, T = 40, 401, 160, 5, 4001
    m, params, geo = module(F, K, hop, True)
    m._algo = _native.ALGO_FFT_WG
    x = batch(B, T, seed=1)
    perm, lam = mix_draw(B, seed=2)
    with torch.no_grad():
        out = m.forward_mixup(x.to(DEV), perm.to(DEV), lam.to(DEV)).cpu()
    mixed64 = x.double() * lam.double().view(B, 1, 1) + x.double()[perm] * (1 - lam.double().view(B, 1, 1))
    ref = lo.leaf_forward(mixed64, {k: v.double() for k, v in params.items()}, geo, True, torch.float64)
    err = rel_err(out, ref.float())
    print(f"forward_mixup vs fp64 oracle: elementwise rel err {err:.3e} (bound {REL_TOL})")
    assert err < REL_TOL
    # an out-of-range index that only exists on the device is clamped into [0, B): a wrong partner, never a read out of bounds
    wild = perm.clone()
    wild[0], wild[3] = B + 1000, -7
    with torch.no_grad():
        got = m.forward_mixup(x.to(DEV), wild.to(DEV), lam.to(DEV))
        want = m.forward_mixup(x.to(DEV), wild.clamp(0, B - 1).to(DEV), lam.to(DEV))
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        m.forward_mixup(x.to(DEV), wild, lam)                    # the same indices on the CPU are refused before any launch


def test_empty_batch():
    m, _, _ = module(40, 401, 160, True)
    out = m.forward_mixup(torch.empty(0, 1, 4001, device=DEV), torch.empty(0, dtype=torch.int64), torch.empty(0))
    assert out.shape == (0, 40, 26) and out.dtype == torch.float32


# ---- training ----------------------------------------------------------------------------------------------------------------
# (name, F, K, hop, T, largest block length, threshold in sixteenths of a block per CU with band tasks / with full_transforms): the
# workgroup-per-block backwards, sized from the CU count as tests/test_gpu_pcm16.py does; and one small batch on the per-wave backward
# ... and the run-time geometry on 2048-sample blocks, whose backward reads the mixed copy (last field: mixes in its loads)
TRAIN_CASES = [("16k-workgroup", 40, 401, 160, 15900, 2048 - 401 + 1, 6, 20, True), ("32k-4096", 12, 801, 320, 7000, 3200, 8, 8, True),
               ("8k-workgroup", 40, 201, 80, 8000, 2048 - 201 + 1, 20, 20, True),
               ("k833-runtime-4096", 6, 833, 333, 7000, (4096 - 833 + 1) & ~1, 8, 8, True),
               ("16k-per-wave", 40, 401, 160, 4001, 2048 - 401 + 1, 0, 0, True),
               ("22k-runtime-workgroup", 12, 552, 220, 9000, 2048 - 552 + 1, 10, 10, False)]
# ... and at the clip lengths where a block load ends ragged (tests/test_gpu_backward_edges.py): one sample, one hop h, h + 1, and
# L - 1, L, L + 1 of the plan's block length L; the batch follows each case's length (one or two blocks per clip)
EDGE_LENGTHS = lambda hop, L: (1, hop, hop + 1, L - 1, L, L + 1)
TRAIN_CASES += [(f"16k-workgroup-edge-T{T}", 40, 401, 160, T, 1600, 6, 20, True) for T in EDGE_LENGTHS(160, 1600)]
TRAIN_CASES += [(f"32k-4096-edge-T{T}", 12, 801, 320, T, 3200, 8, 8, True) for T in EDGE_LENGTHS(320, 3200)]
TRAIN_CASES += [(f"16k-per-wave-edge-T{T}", 40, 401, 160, T, 1600, 0, 0, True) for T in EDGE_LENGTHS(160, 1600)]
TRAIN_CASES += [(f"k833-runtime-4096-edge-T{T}", 6, 833, 333, T, (4096 - 833 + 1) & ~1, 8, 8, True) for T in EDGE_LENGTHS(333, (4096 - 833 + 1) & ~1)]


@pytest.mark.parametrize("int16", [False, True], ids=["fp32", "int16"])
@pytest.mark.parametrize("full", [False, True], ids=["band", "full"])
@pytest.mark.parametrize("case", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_parameter_gradients_equal_those_through_forward_of_the_mixed_batch(case, full, int16):
    name, F, K, hop, T, L_max, six_band, six_full, in_loads = case
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    nblk = -(-T // L_max)
    need = -(-cus * (six_full if full else six_band) // 16)
    B = (-(-need // nblk) + 1) if need else 3
    lib = _native.load()
    own_ws = lib.leaf_backward_workspace_bytes(B, T, F, K, hop, _native.FLAG_PCEN | (_native.FLAG_BWD_FULL_TRANSFORMS if full else 0), 0)
    mix_ws = lib.leaf_backward_mix_workspace_bytes(B, T, F, K, hop, _native.FLAG_PCEN | (_native.FLAG_BWD_FULL_TRANSFORMS if full else 0))
    assert (mix_ws == own_ws) if in_loads else (mix_ws >= own_ws + B * T * 4), (name, own_ws, mix_ws)   # which route serves the backward
    m, _, _ = module(F, K, hop, True, seed=4)
    if full:
        m.full_transforms()
    for p in m.parameters():
        p.requires_grad_(True)
    g = torch.Generator(device=DEV).manual_seed(13)
    x = (2 * torch.rand(B, 1, T, generator=g, device=DEV) - 1) * 0.98
    x = torch.where(x.abs() < 2.0 ** -10, torch.full_like(x, 0.125), x)
    if int16:
        x = torch.round(x * 32767).to(torch.int16)
    perm, lam = mix_draw(B, seed=B)
    mixed = mix_definition(as_float(x), perm.to(DEV), lam.to(DEV))
    go = torch.randn(B, F, (T - 1) // hop + 1, generator=g, device=DEV)
    grads = []
    for call in (lambda: m(mixed), lambda: m(mixed), lambda: m.forward_mixup(x, perm, lam)):
        for p in m.parameters():
            p.grad = None
        out = call()
        out.backward(go)
        grads.append((out.detach(), [p.grad.clone() for _, p in sorted(m.named_parameters())]))
    (oa, a), (ob, b), (og, got) = grads
    assert torch.equal(og, oa)
    assert all(torch.equal(u, v) for u, v in zip(a, b)), "the float32 backward is not reproducible run to run"
    assert len(got) == 7
    for (n, _), u, v in zip(sorted(m.named_parameters()), got, a):
        # (a clip of one frame has no smoother step, a clip of one sample meets the pooling window at its centre alone: those
        # gradients are exact zeros, in fp64 as here)
        assert float(v.abs().max()) > 0 or (T <= hop and n == "_compression.ema._weights") or (T == 1 and n == "_pooling.weights"), n
        assert torch.equal(u, v), f"{name}: {n} differs by {float((u - v).abs().max()):.3e}"


def test_parameter_gradients_match_fp64_autograd_through_the_oracle():
    F, K, hop, B, T = 40, 401, 160, 3, 4001
    m, params, geo = module(F, K, hop, True, seed=5)
    x = batch(B, T, seed=21)
    perm, lam = mix_draw(B, seed=22)
    g = torch.Generator().manual_seed(23)
    go = torch.randn(B, F, (T - 1) // hop + 1, generator=g)
    for p in m.parameters():
        p.requires_grad_(True)
    m.forward_mixup(x.to(DEV), perm, lam).backward(go.to(DEV))
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    mixed64 = x.double() * lam.double().view(B, 1, 1) + x.double()[perm] * (1 - lam.double().view(B, 1, 1))
    lo.leaf_forward(mixed64, p64, geo, True, torch.float64).backward(go.double())
    named = dict(m.named_parameters())
    for n in GRAD_NAMES:
        assert_grad_close(n, named[n].grad, p64[n].grad, ctx="(forward_mixup)")


# ---- the stand-alone kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int16", [False, True], ids=["fp32", "int16"])
def test_standalone_mixup_equals_the_definition(int16):
    for B, T in ((5, 4001), (1, 1), (3, 1024), (2, 70001)):
        x = batch(B, T, seed=B + T, int16=int16).to(DEV)
        perm, lam = mix_draw(B, seed=T)
        got = _native.mixup(x, perm, lam)
        assert got.dtype == torch.float32 and got.shape == x.shape
        assert torch.equal(got, mix_definition(as_float(x), perm.to(DEV), lam.to(DEV))), (B, T)
        assert torch.equal(_native.mixup(x[:, 0], perm, lam), got[:, 0])


def test_standalone_mixup_and_the_transform_reproduce_the_reference_fixture():
    d = np.load(FIXTURE)
    x, perm, lam = torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["perm"]), torch.from_numpy(d["lam"])
    assert torch.equal(_native.mixup(x, perm, lam).cpu(), torch.from_numpy(d["mixed_x"]))
    # transforms.Mixup restates do_mixup: the reference's weights from the seed, its permutation from torch's generator
    y = torch.from_numpy(d["y"]).to(DEV)
    torch.manual_seed(int(d["torch_seed"]))
    mx, my, _, _, p, l = transforms.Mixup(alpha=float(d["alpha"]), random_seed=int(d["random_seed"]))(x, y)
    assert torch.equal(p.cpu(), perm) and torch.equal(l.cpu(), lam)
    assert torch.equal(mx.cpu(), torch.from_numpy(d["mixed_x"])) and torch.equal(my.cpu(), torch.from_numpy(d["mixed_y"]))
    torch.manual_seed(int(d["torch_seed"]))
    mx2, ya, yb, l2, p2, _ = transforms.Mixup(random_seed=int(d["random_seed"]), mode="multiclass")(x, y)
    assert torch.equal(mx2, mx) and torch.equal(ya, y) and torch.equal(yb, y[p2]) and torch.equal(l2.cpu(), lam)


# ---- the C ABI's memory contract ------------------------------------------------------------------------------------------------
def test_raw_c_abi_calls_stay_inside_exact_size_buffers():
    lib = _native.load()
    F, K, hop, B, T = 40, 401, 160, 5, 4001
    TP = (T - 1) // hop + 1
    m, _, _ = module(F, K, hop, True)
    prm = [t.contiguous() for t in args_of(m)]
    pp = [ctypes.c_void_p(t.data_ptr()) for t in prm]
    perm, lam = mix_draw(B, seed=3)
    x = batch(B, T, seed=4).to(DEV)
    mixed = mix_definition(x, perm.to(DEV), lam.to(DEV))
    gx, gperm, glam = guarded_tensor(x), guarded_tensor(perm.to(torch.int32).to(DEV)), guarded_tensor(lam.to(DEV))
    st = _native.stream_ptr(torch.device(DEV))
    for algo in (_native.ALGO_FFT_WG, _native.ALGO_FFT):                      # mixed in the loads / through the mixed copy
        nws = lib.leaf_forward_mix_workspace_bytes(B, T, F, K, hop, algo)
        ws, out, raw = guarded(nws, 0xA5), guarded(B * F * TP * 4, 0xFF), guarded(B * F * TP * 4, 0xFF)
        rc = lib.leaf_forward_save_mix_f32(gx.ptr, gperm.ptr, glam.ptr, B, T, *pp, F, K, hop, _native.FLAG_PCEN, algo, out.ptr, raw.ptr,
                                           ws.ptr, nws, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for gbuf in (gx, gperm, glam):
            unchanged(gbuf, "forward input")
        for gbuf in (ws, out, raw):
            gbuf.check("forward")
        o = out.view(torch.float32, (B, F, TP))
        assert not torch.isnan(o).any() and not torch.isnan(raw.view(torch.float32)).any()       # the 0xFF poison is fully overwritten
        want, want_raw = _native.leaf_forward(mixed, *prm, K, hop, algo=algo, save_raw=True)
        assert torch.equal(o, want) and torch.equal(raw.view(torch.float32, (B, F, TP)), want_raw)
        if nws > 16:
            assert lib.leaf_forward_mix_f32(gx.ptr, gperm.ptr, glam.ptr, B, T, *pp, F, K, hop, _native.FLAG_PCEN, algo, out.ptr, ws.ptr,
                                            nws - 16, st) == -3
    # backward, fed the pooled tensor saved above
    go = torch.randn(B, F, TP, device=DEV)
    nws = lib.leaf_backward_mix_workspace_bytes(B, T, F, K, hop, _native.FLAG_PCEN)
    ws = guarded(nws, 0xA5)
    sizes = [2 * F * 4] + [F * 4] * 6
    gs = [guarded(n, 0xFF) for n in sizes]
    rc = lib.leaf_backward_mix_f32(gx.ptr, gperm.ptr, glam.ptr, B, T, *pp, F, K, hop, _native.FLAG_PCEN, ctypes.c_void_p(go.data_ptr()),
                                   raw.ptr, *[g_.ptr for g_ in gs], None, ws.ptr, nws, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for gbuf in (gx, gperm, glam):
        unchanged(gbuf, "backward input")
    ws.check("backward workspace")
    want = _native.leaf_backward(mixed, *prm, K, hop, go, pooled_raw=raw.view(torch.float32, (B, F, TP)).clone())
    for g_, w in zip(gs, want[:7]):
        g_.check("backward gradient")
        assert torch.equal(g_.view(torch.float32), w.reshape(-1))
    assert lib.leaf_backward_mix_f32(gx.ptr, gperm.ptr, glam.ptr, B, T, *pp, F, K, hop, _native.FLAG_PCEN, ctypes.c_void_p(go.data_ptr()),
                                     raw.ptr, *[g_.ptr for g_ in gs], None, ws.ptr, nws - 16, st) == -3


# ---- refusals and tracing -------------------------------------------------------------------------------------------------------
def test_raises():
    m, _, _ = module(40, 401, 160, True)
    x = batch(3, 4001, seed=7).to(DEV)
    perm, lam = mix_draw(3, seed=8)
    with pytest.raises(RuntimeError, match="float32 or int16"):
        m.forward_mixup(x.bfloat16(), perm, lam)
    with pytest.raises(RuntimeError, match="requires_grad"):
        m.forward_mixup(x.clone().requires_grad_(True), perm, lam)
    with pytest.raises(ValueError):
        m.forward_mixup(x, [0, 1, 3], lam)
    for p in m.parameters():
        p.requires_grad_(True)
    out = m.forward_mixup(x, perm, lam)
    (gk,) = torch.autograd.grad(out.square().sum(), m._complex_conv._kernel, create_graph=True)
    with pytest.raises(RuntimeError, match="gradients of gradients"):
        gk.square().sum().backward()


def test_torch_compile_traces_forward_mixup_without_graph_breaks():
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.leaf = L.Leaf()

        def forward(self, x, perm, lam):
            return self.leaf.forward_mixup(x, perm, lam).mean(dim=-1)

    net = Net().to(DEV)
    x = batch(4, 4001, seed=9).to(DEV)
    perm, lam = mix_draw(4, seed=10)
    perm, lam = perm.to(DEV), lam.to(DEV)
    want = net(x, perm, lam)
    got = torch.compile(net, fullgraph=True, backend="aot_eager")(x, perm, lam)
    assert torch.equal(got, want)
    got.sum().backward()
    assert all(p.grad is not None for p in net.parameters())
