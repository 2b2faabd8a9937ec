"""Host-side contract of the training extensions (log1p compression, bfloat16 I/O through leaf_forward_save_f32 /
leaf_backward_f32): ABI version, workspace arithmetic, argument checks that answer before any launch, the module switch."""
import ctypes
import os
import re
import types

import pytest
import torch

from leaf_pytorch_amd import Leaf, _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_is_6_on_both_sides():
    lib = _native.load()
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _native.ABI_VERSION == 6 and lib.leaf_abi_version() == 6
    assert "no backward" not in lib.leaf_status_string(-8).decode().replace("has no backward)", "")   # (PEAKNORM's note stays)
    assert "bfloat16 I/O has no backward" not in lib.leaf_status_string(-8).decode()


@pytest.mark.parametrize("dx", [0, 1])
@pytest.mark.parametrize("B", [1, 16, 256])
def test_bf16_backward_workspace_does_not_grow_on_the_static_16k_geometry(B, dx):
    """No fp32 copy of the waveform on K = 401 / hop = 160: with LEAF_FLAG_IO_BF16 the backward asks for at most what it asks for
    without it, for PCEN on, PCEN off and log1p; and log1p never adds a byte."""
    lib = _native.load()
    for T in (16000, 160000):
        for flags in (_native.FLAG_PCEN, 0, _native.FLAG_LOG1P, _native.FLAG_PCEN | _native.FLAG_BWD_FULL_TRANSFORMS):
            plain = lib.leaf_backward_workspace_bytes(B, T, 40, 401, 160, flags, dx)
            assert plain > 0
            assert lib.leaf_backward_workspace_bytes(B, T, 40, 401, 160, flags | _native.FLAG_IO_BF16, dx) <= plain
        assert lib.leaf_backward_workspace_bytes(B, T, 40, 401, 160, _native.FLAG_LOG1P, dx) == \
            lib.leaf_backward_workspace_bytes(B, T, 40, 401, 160, 0, dx)


def test_bf16_backward_workspace_says_where_a_widened_copy_is_made():
    """The families that read fp32 only (forced staged / MFMA, short windows, the run-time-geometry kernels of the 2048-sample plan) get
    one widened copy of x: B * T floats, 64-aligned."""
    lib = _native.load()
    up = lambda n: -(-n // 64) * 64
    for B, T, F, K, hop, flags, dx in ((2, 2400, 40, 401, 160, _native.FLAG_BWD_STAGED, 1), (2, 2400, 40, 401, 160, _native.FLAG_BWD_MFMA, 0),
                                       (3, 700, 16, 101, 40, _native.FLAG_PCEN, 0), (3, 700, 16, 101, 40, _native.FLAG_PCEN, 1),
                                       (40, 9000, 6, 552, 220, 0, 0), (40, 9000, 6, 552, 220, 0, 1)):      # a run-time geometry (22.05 kHz)
        plain = lib.leaf_backward_workspace_bytes(B, T, F, K, hop, flags, dx)
        assert lib.leaf_backward_workspace_bytes(B, T, F, K, hop, flags | _native.FLAG_IO_BF16, dx) == plain + 4 * up(B * T)
    # the static geometries and the 4096-sample plans read bf16 directly: 32 kHz on 4096- and on 2048-sample blocks, 8 kHz, a long window
    for B, T, F, K, hop in ((60, 7000, 3, 801, 320), (2, 7000, 3, 801, 320), (4, 8000, 40, 201, 80), (70, 9000, 3, 1201, 480)):
        for dx in ((0,) if K == 1201 else (0, 1)):       # (dL/dx at K = 1201 comes from the run-time-geometry kernel on 2048-sample blocks)
            assert lib.leaf_backward_workspace_bytes(B, T, F, K, hop, _native.FLAG_IO_BF16, dx) == \
                lib.leaf_backward_workspace_bytes(B, T, F, K, hop, 0, dx) > 0


def test_bf16_pointer_checks_answer_before_any_launch():
    """NULL and misaligned (odd address) bf16 buffers: LEAF_ERR_NULL_POINTER / LEAF_ERR_ALIGNMENT from the argument checks (no GPU
    is needed to get these answers: nothing is launched)."""
    lib = _native.load()
    B, T, F, K, hop = 2, 2400, 40, 401, 160
    host = (ctypes.c_char * 4096)()
    base = ctypes.addressof(host)
    base += (-base) % 64
    even, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 1)
    two = ctypes.c_void_p(base + 2)                           # 2-byte aligned, not 4: fine for bf16, not for fp32
    fl = _native.FLAG_PCEN | _native.FLAG_IO_BF16

    def bwd(x, go, gx, flags=fl):
        return lib.leaf_backward_f32(x, B, T, even, even, even, even, even, even, even, F, K, hop, flags, go, None, even, even, even, even,
                                     even, even, even, gx, even, 0, None)
    assert bwd(None, even, None) == -1 and bwd(even, None, None) == -1
    assert bwd(odd, even, None) == -7 and bwd(even, odd, None) == -7 and bwd(even, even, odd) == -7
    assert bwd(two, even, None, _native.FLAG_PCEN) == -7       # fp32 buffers stay 4-byte aligned
    assert bwd(two, two, two) == -3                            # 2-byte alignment passes for bf16: the next check answers (a workspace of 0 bytes)

    def fwd(x, out, raw, flags=fl):
        return lib.leaf_forward_save_f32(x, B, T, even, even, even, even, even, even, even, F, K, hop, flags, 0, out, raw, even, 0, None)
    assert fwd(even, even, None) == -1 and fwd(None, even, even) == -1 and fwd(even, None, even) == -1
    assert fwd(odd, even, even) == -7 and fwd(even, odd, even) == -7
    assert fwd(two, two, even) == -3                           # accepted (no LEAF_ERR_UNSUPPORTED any more): the 0-byte workspace is what is refused


def test_log_compression_switch_on_the_module():
    with pytest.raises(ValueError):
        Leaf().log_compression()
    m = Leaf(pcen_compression=False)
    assert m.log_compression() is m and m._log1p is True
    assert m.log_compression(False) is m and m._log1p is False
    assert list(Leaf(pcen_compression=False).log_compression().state_dict().keys()) == list(Leaf(pcen_compression=False).state_dict().keys())
    assert not list(m.buffers())
    doc = Leaf.log_compression.__doc__
    assert "Not part of the reference surface" in doc
    from leaf_pytorch_amd.streaming import LeafStream
    assert LeafStream(m.log_compression()).log1p is True and LeafStream(Leaf(pcen_compression=False)).log1p is False
    assert LeafStream(Leaf(pcen_compression=False), log1p=True).log1p is True


def test_second_order_formula_applies_log1p_and_refuses_bf16():
    """_second_order.py: the composite gets log1p on top when leaf_amd::backward carried LEAF_FLAG_LOG1P; bf16 I/O raises."""
    from leaf_pytorch_amd import _second_order as so
    from oracle import leaf_oracle as lo
    torch.manual_seed(0)
    F, K, hop, T, B = 4, 101, 40, 600, 2
    geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
    kernel = torch.stack([0.2 + 2.5 * torch.rand(F), 6.0 + torch.rand(F) * K / 4], dim=1)
    params = {k: v.double() for k, v in lo.default_params(geo, False, kernel=kernel).items()}
    x = torch.randn(B, 1, T).double()
    names = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias"]
    leaves = {k: params[k].clone().requires_grad_(True) for k in names}
    out = torch.log1p(lo.leaf_forward(x, leaves, geo, False, torch.float64))
    go = torch.randn_like(out)
    G = torch.autograd.grad(out, list(leaves.values()), go, create_graph=True)
    s = sum((2 * g.detach() * g).sum() for g in G)
    want = torch.autograd.grad(s, list(leaves.values()))
    ctx = types.SimpleNamespace()
    inputs = (x, params[names[0]], params[names[1]], params[names[2]], None, None, None, None, K, hop, go, None, False, so.FLAG_LOG1P)
    ctx.save_for_backward = lambda *t: setattr(ctx, "saved_tensors", t)
    so.setup_context(ctx, inputs, None)
    assert ctx.log1p and not ctx.io_bf16
    res = so.backward(ctx, [2 * g.detach() for g in G] + [None] * 5)
    assert len(res) == 14
    for r, w in zip(res[1:4], want):
        assert float((r - w.reshape(r.shape)).abs().max() / w.abs().max()) < 1e-10
    ctx.io_bf16 = True
    with pytest.raises(RuntimeError, match="bfloat16"):
        so.backward(ctx, [None] * 8)
