"""The ctypes autograd route of ``Leaf.forward_mixup`` (the ops library masked off: frontend._LeafFn over leaf_forward_save_mix_f32 /
leaf_backward_mix_f32) against the same training step through the dispatcher ops: the same C-ABI entries with the same flags, so
the features and all seven parameter gradients are bit-equal."""
import pytest
import torch

from helpers import make_leaf
from oracle import leaf_oracle as lo
from leaf_pytorch_amd import _native, _ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (name, F, K, hop, B, T): the default window, where the mix is inside the kernels' loads, and a run-time geometry, where the
# mixed copy goes into the workspace
GEOMETRIES = [("default-401-160", 40, 401, 160, 3, 2400), ("runtime-101-40", 8, 101, 40, 3, 700)]
MODES = [("float32", False, False), ("int16", True, False), ("float32-bf16-features", False, True)]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    _native.load()
    _ops.load()


def _step(m, x, perm, lam, seed):
    """One training step: the features, and the gradient of every parameter for a fixed upstream gradient."""
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None
    out = m.forward_mixup(x, perm, lam)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(out.dtype)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), [(k, p.grad.clone()) for k, p in m.named_parameters()]


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_ctypes_autograd_step_equals_the_dispatcher_step(geometry, mode, monkeypatch):
    _, F, K, hop, B, T = geometry
    _, int16, bf16 = mode
    torch.manual_seed(3)
    kernel = torch.stack([0.2 + 2.5 * torch.rand(F), 6.0 + torch.rand(F) * K / 4], dim=1)
    params = lo.default_params(lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K)), True, kernel=kernel)
    m = make_leaf(F, K, hop, True, params, DEV)
    if bf16:
        m.output_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    x = (2 * torch.rand(B, 1, T, generator=g) - 1) * 0.98
    x = (torch.round(x * 32767).to(torch.int16) if int16 else x).to(DEV)
    perm = torch.tensor([0, 2, 1])                               # a fixed point and a swap
    lam = torch.tensor([0.0, 1.0, 0.375])                        # all of the partner, all of the clip, a proper mix

    want_out, want = _step(m, x, perm, lam, seed=7)              # through torch.ops.leaf_amd.forward_train_mix
    monkeypatch.setattr(_ops, "available", lambda: False)        # the ops library masked off: _LeafFn over ctypes
    got_out, got = _step(m, x, perm, lam, seed=7)

    assert got_out.dtype == want_out.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert tuple(got_out.shape) == (B, F, (T - 1) // hop + 1) and torch.isfinite(got_out.float()).all()
    assert torch.equal(got_out, want_out)
    assert len(got) == len(want) == 7
    for (k, a), (_, b) in zip(got, want):
        assert a.shape == b.shape and torch.isfinite(a).all() and float(a.abs().max()) > 0, k
        assert torch.equal(a, b), f"{k}: differs by {float((a - b).abs().max()):.3e}"
