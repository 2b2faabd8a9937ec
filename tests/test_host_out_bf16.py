"""Host-side contract of bfloat16 features from float32 / int16 waveforms (LEAF_FLAG_OUT_BF16): the flag's value on both sides of the
C ABI, the argument checks that answer before the workspace check and before any launch (dummy host pointers, a 0-byte workspace:
nothing is launched, no GPU is needed), ``Leaf.output_dtype``'s validation, the ops' schemas and fake kernels, and the empty batch."""
import ctypes
import os
import re
import types

import pytest
import torch

from leaf_pytorch_amd import Leaf, _native, _ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, F, K, HOP = 2, 2400, 40, 401, 160
PC, OUT, IO, PCM = _native.FLAG_PCEN, _native.FLAG_OUT_BF16, _native.FLAG_IO_BF16, _native.FLAG_X_PCM16


def _pointers():
    host = (ctypes.c_char * 4096)()
    base = ctypes.addressof(host)
    base += (-base) % 64
    # even: 4-byte aligned; two: 2-byte aligned, not 4 (fine for a 16-bit buffer, not for fp32); odd: never fine
    return host, ctypes.c_void_p(base), ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 1)


def _fwd(lib, flags, x=None, out=None, algo=0, entry="leaf_forward_f32", t=T):
    _, even, _, _ = _pointers()
    x = even if x is None else x
    out = even if out is None else out
    p = (even,) * 7
    if entry == "leaf_forward_save_f32":
        return lib.leaf_forward_save_f32(x, B, t, *p, F, K, HOP, flags, algo, out, even, even, 0, None)
    if entry == "leaf_forward_mix_f32":
        return lib.leaf_forward_mix_f32(x, even, even, B, t, *p, F, K, HOP, flags, algo, out, even, 0, None)
    if entry == "leaf_forward_save_mix_f32":
        return lib.leaf_forward_save_mix_f32(x, even, even, B, t, *p, F, K, HOP, flags, algo, out, even, even, 0, None)
    if entry == "leaf_forward_prepared_f32":
        return lib.leaf_forward_prepared_f32(x, B, 16000, even, lib.leaf_fft_tables_bytes(F, K, HOP), even, even, even, even, even, F, K, HOP,
                                             flags, out, even, 0, None)
    return lib.leaf_forward_f32(x, B, t, *p, F, K, HOP, flags, algo, out, even, 0, None)


def _bwd(lib, flags, x=None, go=None, gx=None, mix=False):
    _, even, _, _ = _pointers()
    x = even if x is None else x
    go = even if go is None else go
    tail = (F, K, HOP, flags, go, None, even, even, even, even, even, even, even, gx, even, 0, None)
    if mix:
        return lib.leaf_backward_mix_f32(x, even, even, B, T, *(even,) * 7, *tail)
    return lib.leaf_backward_f32(x, B, T, *(even,) * 7, *tail)


def test_flag_value_on_both_sides_and_the_version_stays():
    lib = _native.load()
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert int(re.search(r"#define LEAF_FLAG_OUT_BF16 (0x[0-9a-fA-F]+)", header).group(1), 16) == 0x200
    assert _native.FLAG_OUT_BF16 == 0x200
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6          # additive: the version stays
    assert _native.ABI_VERSION == 6 and lib.leaf_abi_version() == 6
    # the header's LEAF_ERR_UNSUPPORTED list and the LEAF_FLAG_X_PCM16 paragraph name the new flag; "not built" is gone from the latter
    assert "LEAF_FLAG_OUT_BF16" in header[header.index("LEAF_ERR_UNSUPPORTED = -8"):header.index("} leaf_status;")]
    pcm = header[header.index("#define LEAF_FLAG_X_PCM16"):header.index("#define LEAF_FLAG_OUT_BF16")]
    assert "LEAF_FLAG_OUT_BF16" in pcm and "not built" not in pcm
    assert "LEAF_FLAG_OUT_BF16" in lib.leaf_status_string(-8).decode()


@pytest.mark.parametrize("entry", ["leaf_forward_f32", "leaf_forward_save_f32", "leaf_forward_mix_f32", "leaf_forward_save_mix_f32",
                                   "leaf_forward_prepared_f32"])   # (leaf_forward_profiled_f32 creates its events first: it needs a device)
def test_forward_entries_take_a_two_byte_out_only_with_the_flag(entry):
    lib = _native.load()
    keep, even, two, odd = _pointers()
    assert _fwd(lib, PC | OUT, out=two, entry=entry) == -3        # accepted: the 0-byte workspace is what is refused next
    assert _fwd(lib, PC | OUT, out=odd, entry=entry) == -7        # an odd address is never fine
    assert _fwd(lib, PC, out=two, entry=entry) == -7              # float32 features stay 4-byte aligned
    assert _fwd(lib, PC | OUT, x=two, entry=entry) == -7          # x stays float32: the flag says nothing about it
    assert _fwd(lib, PC | OUT | PCM, x=two, out=two, entry=entry) == -3   # int16 in, bfloat16 out
    if "mix" not in entry:
        assert _fwd(lib, PC | OUT | IO, x=two, out=two, entry=entry) == -3    # redundant with bfloat16 I/O, accepted
        assert _fwd(lib, PC | IO | PCM, x=two, out=two, entry=entry) == -8    # two types for x: as before
    else:
        assert _fwd(lib, PC | OUT | IO, x=two, out=two, entry=entry) == -8    # the mixed entries keep refusing a bfloat16 waveform
    del keep


def test_backward_entries_take_a_two_byte_grad_out_only_with_the_flag():
    lib = _native.load()
    keep, even, two, odd = _pointers()
    for mix in (False, True):
        assert _bwd(lib, PC | OUT, go=two, mix=mix) == -3
        assert _bwd(lib, PC | OUT, go=odd, mix=mix) == -7
        assert _bwd(lib, PC, go=two, mix=mix) == -7
        assert _bwd(lib, PC | OUT, x=two, mix=mix) == -7          # x float32
        assert _bwd(lib, PC | OUT | PCM, x=two, go=two, mix=mix) == -3
    assert _bwd(lib, PC | OUT, go=two, gx=two) == -7              # g_x follows x: float32
    assert _bwd(lib, PC | OUT, go=two, gx=even) == -3
    assert _bwd(lib, PC | OUT | IO, x=two, go=two, gx=two) == -3  # redundant, accepted
    assert _bwd(lib, PC | IO | PCM, x=two, go=two) == -8          # as before
    assert _bwd(lib, PC | OUT | PCM, x=two, go=two, gx=even) == -8   # an integer input has no gradient, with or without the flag
    del keep


def test_staged_forward_answers_unsupported_before_the_workspace_check():
    lib = _native.load()
    keep, even, two, odd = _pointers()
    for entry in ("leaf_forward_f32", "leaf_forward_save_f32", "leaf_forward_mix_f32"):
        assert _fwd(lib, PC | OUT, out=two, algo=_native.ALGO_STAGED, entry=entry) == -8    # (0-byte workspace: -8 comes first)
        assert _fwd(lib, PC, algo=_native.ALGO_STAGED, entry=entry) == -3                   # float32: the workspace is what is refused
    # what AUTO resolves to: a window no fused plan covers
    assert lib.leaf_auto_algo(2, 300, 17, 64, 7) == _native.ALGO_STAGED
    p = (even,) * 7
    assert lib.leaf_forward_f32(even, 2, 300, *p, 17, 64, 7, PC | OUT, 0, two, even, 0, None) == -8
    assert lib.leaf_forward_f32(even, 2, 300, *p, 17, 64, 7, PC, 0, even, even, 0, None) == -3
    del keep


def test_no_workspace_grows_with_the_flag():
    """grad_out is widened where it is read (the floor / PCEN backward of every path): the size queries answer the same with and
    without the flag, on the overlap-save paths and on MFMA / staged alike, next to float32 and int16 waveforms."""
    lib = _native.load()
    for b, t, f, k, hop, flags, dx in ((2, 2400, 40, 401, 160, PC, 0), (2, 2400, 40, 401, 160, PC, 1), (2, 2400, 40, 401, 160, _native.FLAG_BWD_STAGED, 1),
                                       (2, 2400, 40, 401, 160, PC | _native.FLAG_BWD_MFMA, 0), (3, 700, 16, 101, 40, PC, 0),
                                       (3, 4001, 12, 552, 220, PC, 0), (1, 8200, 40, 801, 320, PC, 0), (2, 1501, 40, 201, 80, _native.FLAG_LOG1P, 0)):
        for xf in (0, PCM):
            if xf and dx:
                continue
            assert lib.leaf_backward_workspace_bytes(b, t, f, k, hop, flags | xf | OUT, dx) == \
                lib.leaf_backward_workspace_bytes(b, t, f, k, hop, flags | xf, dx) > 0, (b, t, f, k, hop, flags, xf, dx)
            if not dx:
                assert lib.leaf_backward_mix_workspace_bytes(b, t, f, k, hop, flags | xf | OUT) == \
                    lib.leaf_backward_mix_workspace_bytes(b, t, f, k, hop, flags | xf) > 0


def test_empty_batch_needs_no_pointer_and_no_launch(monkeypatch):
    lib = _native.load()
    nul = (None,) * 7
    assert lib.leaf_forward_f32(None, 0, 1600, *nul, 40, 401, 160, PC | OUT, 0, None, None, 0, None) == 0
    assert lib.leaf_forward_f32(None, 0, 1600, *nul, 40, 401, 160, PC | OUT | PCM, 0, None, None, 0, None) == 0
    assert lib.leaf_forward_f32(None, 0, 1600, *nul, 40, 401, 160, PC | OUT, _native.ALGO_STAGED, None, None, 0, None) == -8
    assert lib.leaf_forward_mix_f32(None, None, None, 0, 1600, *nul, 40, 401, 160, PC | OUT, 0, None, None, 0, None) == 0
    # the Python host layer: a (0, F, T') bfloat16 tensor, nothing launched (CPU tensors: only the device check is set aside)
    monkeypatch.setattr(_native, "require_hip", lambda x, who: None)
    m = Leaf()
    c = m._compression
    prm = (m._complex_conv._kernel, m._pooling.weights, m._pooling._bias, c.alpha, c.delta, c.root, c.ema._weights)
    for dt in (torch.float32, torch.int16):
        x = torch.zeros(0, 1, 1600, dtype=dt)
        out = _native.leaf_forward(x, *prm, 401, 160, out_bf16=True)
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (0, 40, 10)
        out, raw = _native.leaf_forward(x, *prm, 401, 160, out_bf16=True, save_raw=True)
        assert out.dtype == torch.bfloat16 and raw.dtype == torch.float32 and tuple(raw.shape) == (0, 40, 10)
        assert _native.leaf_forward(x, *prm, 401, 160).dtype == torch.float32           # the mode is explicit: the default stays
        perm, lam = torch.zeros(0, dtype=torch.int64), torch.zeros(0)
        mo = _native.leaf_forward_mix(x, perm, lam, *prm, 401, 160, out_bf16=True)
        assert mo.dtype == torch.bfloat16 and tuple(mo.shape) == (0, 40, 10)
        g = _native.leaf_backward(x, *prm, 401, 160, torch.zeros(0, 40, 10, dtype=torch.bfloat16), out_bf16=True)
        assert all(float(t.abs().sum()) == 0.0 for t in g[:7])
    # the mode is not inferred from a tensor: a bfloat16 grad_out without it, and a float32 one with it, are refused as a wrong dtype
    x = torch.zeros(0, 1, 1600)
    with pytest.raises(RuntimeError, match="grad_out must be float32"):
        _native.leaf_backward(x, *prm, 401, 160, torch.zeros(0, 40, 10, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="grad_out must be bfloat16"):
        _native.leaf_backward(x, *prm, 401, 160, torch.zeros(0, 40, 10), out_bf16=True)
    with pytest.raises(RuntimeError, match="out must be a contiguous"):
        _native.leaf_forward(x, *prm, 401, 160, out=torch.zeros(0, 40, 10, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="out must be a contiguous"):
        _native.leaf_forward(x, *prm, 401, 160, out=torch.zeros(0, 40, 10), out_bf16=True)


def test_output_dtype_validates_and_adds_no_state():
    m = Leaf()
    keys = list(m.state_dict())
    assert m._features_bf16(torch.zeros(1, 1, 8)) is False                                  # default: the features follow the waveform
    for ok in (None, torch.float32, torch.bfloat16, "autocast"):
        assert m.output_dtype(ok) is m
    for bad in (torch.float16, torch.float64, torch.int16, "bfloat16", "bf16", 16, True):
        with pytest.raises(ValueError, match="output_dtype"):
            m.output_dtype(bad)
    assert m._out_dtype == "autocast"                                                        # a refused value changes nothing
    assert list(m.state_dict()) == keys and len(list(m.buffers())) == 0 and len(list(m.parameters())) == 7
    assert list(Leaf().state_dict()) == keys
    m.output_dtype(torch.bfloat16)
    assert m._features_bf16(torch.zeros(1, 1, 8)) and m._features_bf16(torch.zeros(1, 1, 8, dtype=torch.int16))
    m.output_dtype(torch.float32)
    assert not m._features_bf16(torch.zeros(1, 1, 8)) and not m._features_bf16(torch.zeros(1, 1, 8, dtype=torch.int16))
    with pytest.raises(ValueError, match="not built"):
        m._features_bf16(torch.zeros(1, 1, 8, dtype=torch.bfloat16))
    m.output_dtype("autocast")
    assert not m._features_bf16(torch.zeros(1, 1, 8))                                        # no autocast region here
    m.output_dtype(None)
    assert not m._features_bf16(torch.zeros(1, 1, 8, dtype=torch.bfloat16))
    # the device check still answers first on forward, whatever the setting
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        m.output_dtype(torch.bfloat16)(torch.zeros(1, 1, 800))
    assert "LeafStream" in Leaf.output_dtype.__doc__ and "float32" in Leaf.output_dtype.__doc__


def test_op_schemas_carry_the_keyword_and_fake_kernels_the_dtype():
    _ops.load()
    ops = torch.ops.leaf_amd
    for name in ("forward", "forward_train", "backward", "forward_mix", "forward_train_mix", "backward_mix"):
        args = getattr(ops, name).default._schema.arguments
        a = args[-1]
        assert a.name == "out_bf16" and a.kwarg_only and a.default_value is False and str(a.type) == "bool", name
        assert [b.name for b in args].count("out_bf16") == 1
    kernel, pw, pb = (torch.zeros(s, device="meta") for s in ((40, 2), (1, 1, 40, 1), (40,)))
    pc = tuple(torch.zeros(40, device="meta") for _ in range(4))
    perm, lam = torch.zeros(3, dtype=torch.int32, device="meta"), torch.zeros(3, device="meta")
    for dt in (torch.float32, torch.int16):
        x = torch.zeros(3, 1, 16001, dtype=dt, device="meta")
        for flag, want in ((False, torch.float32), (True, torch.bfloat16)):
            o = ops.forward(x, kernel, pw, pb, *pc, 401, 160, False, 0, out_bf16=flag)
            assert o.dtype == want and tuple(o.shape) == (3, 40, 101)
            o, raw = ops.forward_train(x, kernel, pw, pb, *pc, 401, 160, 0, False, out_bf16=flag)
            assert o.dtype == want and raw.dtype == torch.float32
            o = ops.forward_mix(x, perm, lam, kernel, pw, pb, *pc, 401, 160, False, 0, out_bf16=flag)
            assert o.dtype == want and tuple(o.shape) == (3, 40, 101)
            o, raw = ops.forward_train_mix(x, perm, lam, kernel, pw, pb, *pc, 401, 160, 0, False, out_bf16=flag)
            assert o.dtype == want and raw.dtype == torch.float32
    xb = torch.zeros(3, 1, 16001, dtype=torch.bfloat16, device="meta")
    assert ops.forward(xb, kernel, pw, pb, *pc, 401, 160, False, 0).dtype == torch.bfloat16                 # as before
    assert ops.forward(xb, kernel, pw, pb, *pc, 401, 160, False, 0, out_bf16=True).dtype == torch.bfloat16  # redundant
    x = torch.zeros(3, 1, 16001, device="meta")
    g = ops.backward(x, kernel, pw, pb, *pc, 401, 160, torch.zeros(3, 40, 101, dtype=torch.bfloat16, device="meta"), None, True, 0, out_bf16=True)
    assert g[7].dtype == torch.float32 and tuple(g[7].shape) == (3, 1, 16001) and all(t.dtype == torch.float32 for t in g[:7])


def test_second_order_refuses_bfloat16_features():
    from leaf_pytorch_amd import _second_order as so
    Fq, Kq, hopq, Tq = 4, 101, 40, 600
    x = torch.zeros(2, 1, Tq)
    kernel, pw, pb = torch.zeros(Fq, 2), torch.zeros(Fq), torch.zeros(Fq)
    go = torch.zeros(2, Fq, (Tq - 1) // hopq + 1, dtype=torch.bfloat16)
    ctx = types.SimpleNamespace()
    ctx.save_for_backward = lambda *t: setattr(ctx, "saved_tensors", t)
    so.setup_context(ctx, (x, kernel, pw, pb, None, None, None, None, Kq, hopq, go, None, False, 0), None, {"out_bf16": True})
    assert ctx.out_bf16 and not ctx.io_bf16 and not ctx.x_pcm16
    with pytest.raises(RuntimeError, match="bfloat16 features"):
        so.backward(ctx, [None] * 8)
    so.setup_context(ctx, (x, kernel, pw, pb, None, None, None, None, Kq, hopq, go.float(), None, False, 0), None, {"out_bf16": False})
    assert not ctx.out_bf16
    assert len(so.backward(ctx, [None] * 8)) == 14              # one slot per positional input of the op
