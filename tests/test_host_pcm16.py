"""Host-side contract of 16-bit PCM input (LEAF_FLAG_X_PCM16): the flag's value on both sides of the C ABI, the argument checks that
answer before the workspace check and before any launch (dummy host pointers, a 0-byte workspace: nothing is launched, no GPU is
needed), the backward's workspace arithmetic, and the Python layers' refusals."""
import ctypes
import os
import re
import types

import pytest
import torch

from leaf_pytorch_amd import Leaf, _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, F, K, HOP = 2, 2400, 40, 401, 160


def _pointers():
    host = (ctypes.c_char * 4096)()
    base = ctypes.addressof(host)
    base += (-base) % 64
    # even: 4-byte aligned; two: 2-byte aligned, not 4 (fine for int16, not for fp32); odd: never fine
    return host, ctypes.c_void_p(base), ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 1)


def _fwd(lib, x, flags, algo=0, out=None, entry="leaf_forward_f32"):
    _, even, _, _ = _pointers()
    out = even if out is None else out
    if entry == "leaf_forward_save_f32":
        return lib.leaf_forward_save_f32(x, B, T, even, even, even, even, even, even, even, F, K, HOP, flags, algo, out, even, even, 0, None)
    return lib.leaf_forward_f32(x, B, T, even, even, even, even, even, even, even, F, K, HOP, flags, algo, out, even, 0, None)


def _bwd(lib, x, flags, gx=None, go=None):
    _, even, _, _ = _pointers()
    go = even if go is None else go
    return lib.leaf_backward_f32(x, B, T, even, even, even, even, even, even, even, F, K, HOP, flags, go, None, even, even, even, even,
                                 even, even, even, gx, even, 0, None)


def test_flag_value_and_abi_version_on_both_sides():
    lib = _native.load()
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert int(re.search(r"#define LEAF_FLAG_X_PCM16 (0x[0-9a-fA-F]+)", header).group(1), 16) == 0x100
    assert _native.FLAG_X_PCM16 == 0x100
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6          # additive: the version stays
    assert _native.ABI_VERSION == 6 and lib.leaf_abi_version() == 6


def test_odd_address_is_refused_and_two_byte_alignment_passes_only_with_the_flag():
    lib = _native.load()
    keep, even, two, odd = _pointers()
    pcm = _native.FLAG_PCEN | _native.FLAG_X_PCM16
    for entry in ("leaf_forward_f32", "leaf_forward_save_f32"):
        assert _fwd(lib, odd, pcm, entry=entry) == -7
        assert _fwd(lib, two, pcm, entry=entry) == -3                 # accepted: the 0-byte workspace is what is refused next
        assert _fwd(lib, two, _native.FLAG_PCEN, entry=entry) == -7   # fp32 buffers stay 4-byte aligned
        assert _fwd(lib, even, pcm, out=two, entry=entry) == -7       # out is float32 with the flag
    assert _bwd(lib, odd, pcm) == -7
    assert _bwd(lib, two, pcm) == -3
    assert _bwd(lib, two, _native.FLAG_PCEN) == -7
    assert _bwd(lib, even, pcm, go=two) == -7                         # grad_out is float32 with the flag
    del keep


def test_prepared_forward_takes_the_flag():
    lib = _native.load()
    keep, even, two, odd = _pointers()
    Tl = 16000
    tb = lib.leaf_fft_tables_bytes(F, K, HOP)
    assert tb > 0

    def call(x, flags):
        return lib.leaf_forward_prepared_f32(x, B, Tl, even, tb, even, even, even, even, even, F, K, HOP, flags, even, even, 0, None)
    pcm = _native.FLAG_PCEN | _native.FLAG_X_PCM16
    assert call(odd, pcm) == -7
    assert call(two, pcm) == -3 and call(two, _native.FLAG_PCEN) == -7
    assert call(even, pcm | _native.FLAG_IO_BF16) == -8
    assert call(two, pcm | _native.FLAG_PEAKNORM) == -3               # valid: every int16 clip's scale is 1
    assert call(even, _native.FLAG_PCEN | _native.FLAG_PEAKNORM) == -8  # (float32: as before)
    del keep


def test_unsupported_combinations_answer_before_the_workspace_check():
    lib = _native.load()
    keep, even, two, odd = _pointers()
    pcm = _native.FLAG_PCEN | _native.FLAG_X_PCM16
    # int16 in with bfloat16 out is not built
    assert _fwd(lib, even, pcm | _native.FLAG_IO_BF16) == -8
    assert _fwd(lib, even, pcm | _native.FLAG_IO_BF16, entry="leaf_forward_save_f32") == -8
    assert _bwd(lib, even, pcm | _native.FLAG_IO_BF16) == -8
    # an integer input has no gradient
    assert _bwd(lib, even, pcm, gx=even) == -8
    assert _bwd(lib, even, _native.FLAG_PCEN, gx=even) == -3          # (float32: accepted, the workspace is what is refused)
    # the staged forward reads float32 only
    assert _fwd(lib, even, pcm, algo=_native.ALGO_STAGED) == -8
    assert _fwd(lib, even, pcm, algo=_native.ALGO_STAGED, entry="leaf_forward_save_f32") == -8
    assert _fwd(lib, even, _native.FLAG_PCEN, algo=_native.ALGO_STAGED) == -3
    # peak normalisation is the identity on int16 clips: valid, also on the training forward, where float32 refuses it
    assert _fwd(lib, even, pcm | _native.FLAG_PEAKNORM) == -3
    assert _fwd(lib, even, pcm | _native.FLAG_PEAKNORM, entry="leaf_forward_save_f32") == -3
    assert _fwd(lib, even, _native.FLAG_PCEN | _native.FLAG_PEAKNORM, entry="leaf_forward_save_f32") == -8
    del keep


def test_backward_workspace_reports_the_widened_copy_where_bf16_does():
    """The geometries tests/test_host_train_extensions.py lists for bfloat16: the families that read fp32 only get one widened copy
    of x (B * T floats, 64-aligned); the static geometries and the 4096-sample plans read int16 directly."""
    lib = _native.load()
    up = lambda n: -(-n // 64) * 64
    pcm = _native.FLAG_X_PCM16
    for b, t, f, k, hop, flags, dx in ((2, 2400, 40, 401, 160, _native.FLAG_BWD_STAGED, 1), (2, 2400, 40, 401, 160, _native.FLAG_BWD_MFMA, 0),
                                       (3, 700, 16, 101, 40, _native.FLAG_PCEN, 0), (3, 700, 16, 101, 40, _native.FLAG_PCEN, 1),
                                       (40, 9000, 6, 552, 220, 0, 0), (40, 9000, 6, 552, 220, 0, 1)):
        plain = lib.leaf_backward_workspace_bytes(b, t, f, k, hop, flags, dx)
        assert plain > 0
        assert lib.leaf_backward_workspace_bytes(b, t, f, k, hop, flags | pcm, dx) == plain + 4 * up(b * t)
        assert lib.leaf_backward_workspace_bytes(b, t, f, k, hop, flags | pcm, dx) == \
            lib.leaf_backward_workspace_bytes(b, t, f, k, hop, flags | _native.FLAG_IO_BF16, dx)
    for b, t, f, k, hop in ((60, 7000, 3, 801, 320), (2, 7000, 3, 801, 320), (4, 8000, 40, 201, 80), (70, 9000, 3, 1201, 480)):
        for dx in ((0,) if k == 1201 else (0, 1)):
            assert lib.leaf_backward_workspace_bytes(b, t, f, k, hop, pcm, dx) == lib.leaf_backward_workspace_bytes(b, t, f, k, hop, 0, dx) > 0
    for b in (1, 16, 256):
        for t in (16000, 160000):
            for flags in (_native.FLAG_PCEN, 0, _native.FLAG_LOG1P, _native.FLAG_PCEN | _native.FLAG_BWD_FULL_TRANSFORMS):
                assert lib.leaf_backward_workspace_bytes(b, t, 40, 401, 160, flags | pcm, 0) == \
                    lib.leaf_backward_workspace_bytes(b, t, 40, 401, 160, flags, 0) > 0


def test_status_string_names_the_new_cases():
    s = _native.load().leaf_status_string(-8).decode()
    assert "LEAF_FLAG_X_PCM16" in s and "staged" in s and "LEAF_FLAG_IO_BF16" in s and "g_x" in s
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert "LEAF_FLAG_X_PCM16" in header[header.index("LEAF_ERR_UNSUPPORTED = -8"):header.index("} leaf_status;")]


def test_second_order_refuses_int16():
    from leaf_pytorch_amd import _second_order as so
    Fq, Kq, hopq, Tq = 4, 101, 40, 600
    x = torch.zeros(2, 1, Tq, dtype=torch.int16)
    kernel, pw, pb = torch.zeros(Fq, 2), torch.zeros(Fq), torch.zeros(Fq)
    go = torch.zeros(2, Fq, (Tq - 1) // hopq + 1)
    ctx = types.SimpleNamespace()
    ctx.save_for_backward = lambda *t: setattr(ctx, "saved_tensors", t)
    so.setup_context(ctx, (x, kernel, pw, pb, None, None, None, None, Kq, hopq, go, None, False, 0), None)
    assert ctx.x_pcm16 and not ctx.io_bf16
    with pytest.raises(RuntimeError, match="int16"):
        so.backward(ctx, [None] * 8)
    so.setup_context(ctx, (x.float(), kernel, pw, pb, None, None, None, None, Kq, hopq, go, None, False, 0), None)
    assert not ctx.x_pcm16


def test_stream_refuses_a_dtype_change_before_any_device_call():
    """CPU tensors: the sample-type check of LeafStream.step answers before the device check and before any kernel call."""
    from leaf_pytorch_amd.streaming import LeafStream
    st = LeafStream(Leaf())
    st.buf = torch.zeros(2, 500, dtype=torch.int16)                   # a stream that has taken int16 chunks
    with pytest.raises(RuntimeError, match="one sample type per stream"):
        st.step(torch.zeros(2, 1, 300))
    st.buf = torch.zeros(2, 500)                                      # ... and one that has taken float32 chunks
    with pytest.raises(RuntimeError, match="one sample type per stream"):
        st.step(torch.zeros(2, 1, 300, dtype=torch.int16))
    st.buf = None
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):   # any other type is widened as before: only the device check answers
        st.step(torch.zeros(2, 1, 300, dtype=torch.int32))
