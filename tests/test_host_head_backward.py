"""Host side of the head-only backward (no GPU): the route decision, the argument checks of ``_native.leaf_backward_head`` (raised in
Python, before the library is loaded), the C ABI's two new entries in the header and in the binding's signature table, and the
second-order formula of ``leaf_amd::backward_head`` on the CPU against the formula of the full op (as tests/test_host_logic.py pins
``composite_forward``)."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from leaf_pytorch_amd import _native, _ops, _second_order

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_route_truth_table():
    for need_kernel, need_pool_w, need_x, create_graph in itertools.product((False, True), repeat=4):
        want = "full" if (need_kernel or need_pool_w or need_x or create_graph) else "head"
        assert _ops.backward_route(need_kernel, need_pool_w, need_x, create_graph) == want
    assert _ops.backward_route(False, False, False, False) == "head"
    assert _ops.backward_route(False, False, False, True) == "full"          # create_graph alone keeps the full formula's route


def _args(B=2, F=3, TP=5, pcen=True, dtype=torch.float32, device="cpu"):
    raw = torch.rand(B, F, TP, device=device)
    go = torch.randn(B, F, TP, device=device).to(dtype)
    vec = lambda: torch.rand(F, device=device)
    return [raw, go, vec()] + ([vec(), vec(), vec(), vec()] if pcen else [None] * 4)


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the errors below are raised before it is touched."""
    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_native, "load", boom)


def test_head_backward_argument_errors_come_before_the_library(no_library):
    a = _args()
    with pytest.raises(RuntimeError, match="pooled_raw must be"):
        _native.leaf_backward_head(a[0][0], *a[1:])                                  # (F, T'): not a batch
    with pytest.raises(RuntimeError, match="grad_out has shape"):
        _native.leaf_backward_head(a[0], a[1][:, :, :4], *a[2:])
    with pytest.raises(RuntimeError, match="pool_b must hold"):
        _native.leaf_backward_head(a[0], a[1], torch.rand(4), *a[3:])
    with pytest.raises(RuntimeError, match="alpha must hold"):
        _native.leaf_backward_head(a[0], a[1], a[2], torch.rand(2), *a[4:])
    with pytest.raises(RuntimeError, match="delta must hold"):
        _native.leaf_backward_head(a[0], a[1], a[2], a[3], None, *a[5:])
    # the dtype of grad_out is what out_bf16 says, in both directions
    with pytest.raises(RuntimeError, match="grad_out must be torch.bfloat16 with out_bf16=True"):
        _native.leaf_backward_head(*a, out_bf16=True)
    b = _args(dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="grad_out must be torch.float32 with out_bf16=False"):
        _native.leaf_backward_head(*b)
    with pytest.raises(RuntimeError, match="pooled_raw must be float32"):
        _native.leaf_backward_head(a[0].double(), *a[1:])
    # well-formed arguments on the CPU: there is no CPU path
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.leaf_backward_head(*a)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.leaf_backward_head(*_args(pcen=False), pcen=False, log1p=True)


def test_header_declares_the_two_entries_and_the_binding_lists_them():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert re.search(r"size_t\s+leaf_backward_head_workspace_bytes\(int B, int TP, int F, int flags\);", header)
    m = re.search(r"int\s+leaf_backward_head_f32\(([^;]*)\);", header)
    assert m
    decl = " ".join(m.group(1).split())
    assert decl == ("const float* pooled_raw, const float* grad_out, int B, int TP, int F, const float* alpha, const float* delta, "
                    "const float* root, const float* ema_w, int flags, float* g_pool_b, float* g_alpha, float* g_delta, float* g_root, "
                    "float* g_ema_w, void* workspace, size_t workspace_bytes, void* stream")
    assert re.search(r"#define LEAF_ABI_VERSION\s+6\b", header) and _native.ABI_VERSION == 6      # additive
    res, args = _native._SIGNATURES["leaf_backward_head_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int] * 4
    res, args = _native._SIGNATURES["leaf_backward_head_f32"]
    assert res is ctypes.c_int and len(args) == len(decl.split(","))
    for name in ("leaf_backward_head_workspace_bytes", "leaf_backward_head_f32"):
        assert name in _native.EXPORTED_SYMBOLS and name in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_library_exports_the_entries_and_answers_their_checks_without_a_gpu():
    """Status codes that need no device: the flag check comes first, then the empty batch's and the call's NULL checks, then the shape."""
    lib = _native.load()
    call = lib.leaf_backward_head_f32
    null = [None] * 2
    dims = (2, 5, 3)
    tail = [None] * 4 + [_native.FLAG_PCEN] + [None] * 5 + [None, 0, None]
    assert call(*null, *dims, *[None] * 4, _native.FLAG_PCEN | _native.FLAG_BWD_STAGED, *[None] * 5, None, 0, None) == -8
    assert call(*null, *dims, *[None] * 4, _native.FLAG_X_PCM16, *[None] * 5, None, 0, None) == -8
    assert call(*null, *dims, *tail) == -1                                   # NULL pointers
    assert call(*null, 0, 5, 3, *tail) == -1                                 # the empty batch still needs its outputs
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    full = lambda B, TP, F, flags=_native.FLAG_PCEN: call(p, p, B, TP, F, p, p, p, p, flags, p, p, p, p, p, None, 0, None)
    assert full(-1, 5, 3) == -2 and full(2, 0, 3) == -2 and full(2, 5, 0) == -2
    assert full(1 << 16, 1 << 10, 1 << 5) == -2                              # B F T' = 2^31: the caller slices
    assert lib.leaf_backward_head_workspace_bytes(1 << 16, 1 << 10, 1 << 5, _native.FLAG_PCEN) == 0
    assert lib.leaf_backward_head_workspace_bytes(2, 5, 3, _native.FLAG_BWD_MFMA) == 0
    assert lib.leaf_backward_head_workspace_bytes(0, 5, 3, _native.FLAG_PCEN) == 0


@pytest.mark.parametrize("mode", ["pcen", "off", "log1p"])
def test_second_order_of_the_head_op_is_the_full_ops_formula_with_the_filterbank_constant(mode):
    """``_second_order._backward_head`` differentiates <v, G> from the saved pooled tensor; the full op's formula does it from the
    waveform.  In float64 on the CPU, with the pooled tensor taken from ``composite_forward``'s own filterbank, the two agree on the
    gradients they share (pool_b, the PCEN vectors, grad_out) to rounding."""
    torch.manual_seed(5)
    B, F, K, hop, T = 2, 3, 31, 10, 95
    pcen = mode == "pcen"
    x = torch.randn(B, 1, T, dtype=torch.float64)
    kernel = torch.stack([0.3 + torch.rand(F, dtype=torch.float64) * 2.0, 4.0 + torch.rand(F, dtype=torch.float64) * 3.0], dim=1)
    pool_w = (0.3 + 0.1 * torch.rand(F, dtype=torch.float64)).reshape(1, 1, F, 1)
    pool_b = 0.01 * torch.rand(F, dtype=torch.float64)
    pc = [0.9 + 0.05 * torch.rand(F, dtype=torch.float64), 1.5 + torch.rand(F, dtype=torch.float64),
          1.5 + torch.rand(F, dtype=torch.float64), 0.03 + 0.05 * torch.rand(F, dtype=torch.float64)] if pcen else [None] * 4
    # the pre-floor pooled tensor: composite_forward without the compression, where the floor is seen to be inactive
    raw = _second_order.composite_forward(x, kernel, pool_w, pool_b, None, None, None, None, K, hop)
    assert float(raw.min()) > 1e-5 * 1.01                                       # (no entry sits on the floor or its kink)
    go = torch.randn_like(raw)
    vs = [torch.randn(F, dtype=torch.float64) for _ in range(5 if pcen else 1)]

    class Ctx:
        pass

    full = Ctx()
    full.saved_tensors = (x, kernel, pool_w, pool_b, go, *(pc if pcen else ()))
    full.pcen, full.geom, full.need_dx, full.log1p = pcen, (K, hop), False, mode == "log1p"
    cot = [torch.zeros_like(kernel), torch.zeros_like(pool_w), vs[0]] + (vs[1:] if pcen else [None] * 4) + [None]
    r_full = _second_order.backward(full, cot)
    head = Ctx()
    head.saved_tensors = (raw, go, pool_b, *(pc if pcen else ()))
    head.pcen, head.log1p, head.out_bf16 = pcen, mode == "log1p", False
    r_head = _second_order._backward_head(head, vs + [None] * (5 - len(vs)))
    assert r_head[0] is None and r_head[-1] is None and len(r_head) == 8
    # full: gx, gk, gpw, gpb, 4 PCEN, K, hop, ggo, ...; head: raw, ggo, gpb, 4 PCEN, flags
    pairs = [("grad_out", r_head[1], r_full[10]), ("pool_b", r_head[2], r_full[3])]
    if pcen:
        pairs += [(n, r_head[3 + i], r_full[4 + i]) for i, n in enumerate(("alpha", "delta", "root", "ema_w"))]
    for name, h, f in pairs:
        if h is None or f is None:                                              # (no dependence: None on one side, None or zeros on the other)
            other = f if h is None else h
            assert other is None or float(other.abs().max()) == 0.0, name
            continue
        assert h.shape == f.shape, name
        assert float((h - f).abs().max()) <= 1e-9 * max(1.0, float(f.abs().max())), (name, float((h - f).abs().max()))
