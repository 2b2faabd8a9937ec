"""Alignment the C ABI asks for, answered before the workspace check and before any launch (dummy host pointers, a 0-byte
workspace: nothing is launched, no GPU is needed).  `workspace` and `tables` are read with 8- and 16-byte accesses (float2 / float4 /
int4 rows, 16-byte direct-to-LDS loads, the 64-bit seam tickets) and must be 16-byte aligned; every other float32 buffer is reached
one element at a time and must be 4-byte aligned (bfloat16 / int16 buffers: 2; tests/test_host_pcm16.py,
tests/test_host_train_extensions.py).  INTEGRATION.md has the table."""
import ctypes
import os
import re

from leaf_pytorch_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, F, K, HOP = 2, 2400, 40, 401, 160
ALIGNMENT, WORKSPACE = -7, -3


def _base():
    host = (ctypes.c_char * 4096)()
    base = ctypes.addressof(host)
    return host, base + (-base) % 64


def P(addr):
    return ctypes.c_void_p(addr)


def test_forward_entry_points_want_a_16_byte_workspace_and_4_byte_parameters():
    lib = _native.load()
    keep, b = _base()
    ok = P(b)

    def fwd(ws=ok, prm=None, raw=None, save=False):
        p = [ok] * 7
        if prm is not None:
            p[prm[0]] = P(b + prm[1])
        if save or raw is not None:
            return lib.leaf_forward_save_f32(ok, B, T, *p, F, K, HOP, _native.FLAG_PCEN, 0, ok, ok if raw is None else P(b + raw), ws, 0, None)
        return lib.leaf_forward_f32(ok, B, T, *p, F, K, HOP, _native.FLAG_PCEN, 0, ok, ws, 0, None)
    for save in (False, True):
        for off in (4, 8, 12, 20):
            assert fwd(P(b + off), save=save) == ALIGNMENT, off
        for off in (0, 16, 48):
            assert fwd(P(b + off), save=save) == WORKSPACE, off          # accepted: the 0-byte workspace is what is refused next
        for i in range(7):
            assert fwd(prm=(i, 2), save=save) == ALIGNMENT and fwd(prm=(i, 4), save=save) == WORKSPACE, i
    assert fwd(raw=2) == ALIGNMENT and fwd(raw=4) == WORKSPACE
    del keep


def test_backward_wants_a_16_byte_workspace_and_4_byte_parameters_and_gradients():
    lib = _native.load()
    keep, b = _base()
    ok = P(b)

    def bwd(ws=ok, slot=None, off=0):
        a = [ok] * 7 + [F, K, HOP, _native.FLAG_PCEN, ok, ok] + [ok] * 7 + [ok]     # parameters | ... grad_out, pooled_raw | gradients | g_x
        if slot is not None:
            a[slot] = P(b + off)
        return lib.leaf_backward_f32(ok, B, T, *a, ws, 0, None)
    for off in (4, 8, 12):
        assert bwd(P(b + off)) == ALIGNMENT, off
    assert bwd(P(b + 16)) == WORKSPACE
    for slot in list(range(7)) + [12] + list(range(13, 20)):                       # parameters, pooled_raw, the seven gradients
        assert bwd(slot=slot, off=2) == ALIGNMENT and bwd(slot=slot, off=4) == WORKSPACE, slot
    del keep


def test_tables_and_their_callers():
    lib = _native.load()
    keep, b = _base()
    ok = P(b)
    tb = lib.leaf_fft_tables_bytes(F, K, HOP)
    assert tb > 0
    prep = lambda t, k=ok: lib.leaf_fft_prepare_tables_f32(k, ok, F, K, HOP, t, 0, None)
    assert prep(P(b + 4)) == ALIGNMENT and prep(P(b + 8)) == ALIGNMENT and prep(ok, P(b + 2)) == ALIGNMENT
    assert prep(P(b + 16)) == WORKSPACE                                            # (tables_bytes = 0: the size check answers)
    run = lambda t=ok, ws=ok, bias=ok: lib.leaf_forward_prepared_f32(ok, B, 16000, t, tb, bias, ok, ok, ok, ok, F, K, HOP, _native.FLAG_PCEN, ok, ws, 0,
                                                                     None)
    assert run(t=P(b + 4)) == ALIGNMENT and run(t=P(b + 8)) == ALIGNMENT and run(ws=P(b + 4)) == ALIGNMENT and run(ws=P(b + 8)) == ALIGNMENT
    assert run(bias=P(b + 2)) == ALIGNMENT
    assert run(t=P(b + 16), ws=P(b + 32)) == WORKSPACE
    cls = lambda ws=ok, c=ok, k=ok: lib.leaf_band_classes_f32(k, ok, ok, F, K, HOP, c, ws, 0, None)
    assert cls(ws=P(b + 4)) == ALIGNMENT and cls(ws=P(b + 8)) == ALIGNMENT and cls(c=P(b + 2)) == ALIGNMENT and cls(k=P(b + 2)) == ALIGNMENT
    assert cls(ws=P(b + 16)) == WORKSPACE
    assert lib.leaf_band_classes_f32(ok, ok, ok, 80, 801, 320, ok, P(b + 8), 0, None) == ALIGNMENT     # the 4096-sample plan's branch
    del keep


def test_stage_entry_points():
    lib = _native.load()
    keep, b = _base()
    ok, two, ws8 = P(b), P(b + 2), P(b + 8)
    Tf, TP = 333, 9
    assert lib.leaf_gabor_taps_f32(two, F, K, ok, None) == ALIGNMENT and lib.leaf_gabor_taps_f32(ok, F, K, two, None) == ALIGNMENT
    assert lib.leaf_lowpass_window_f32(two, F, K, ok, None) == ALIGNMENT and lib.leaf_lowpass_window_f32(ok, F, K, two, None) == ALIGNMENT
    assert lib.leaf_gabor_conv_f32(ok, B, Tf, ok, F, K, ok, ws8, 0, None) == ALIGNMENT
    assert lib.leaf_gabor_conv_f32(two, B, Tf, ok, F, K, ok, ok, 0, None) == ALIGNMENT
    assert lib.leaf_gabor_conv_f32(ok, B, Tf, ok, F, K, ok, ok, 0, None) == WORKSPACE
    assert lib.leaf_squared_modulus_f32(two, B, F, Tf, ok, None) == ALIGNMENT and lib.leaf_squared_modulus_f32(ok, B, F, Tf, two, None) == ALIGNMENT
    assert lib.leaf_gaussian_lowpass_f32(ok, B, F, Tf, ok, ok, K, HOP, ok, ws8, 0, None) == ALIGNMENT
    assert lib.leaf_gaussian_lowpass_f32(ok, B, F, Tf, ok, two, K, HOP, ok, ok, 0, None) == ALIGNMENT
    assert lib.leaf_gaussian_lowpass_f32(ok, B, F, Tf, ok, None, K, HOP, ok, ok, 0, None) == WORKSPACE       # pool_b may be NULL
    assert lib.leaf_ema_f32(two, B, F, TP, ok, ok, None) == ALIGNMENT and lib.leaf_ema_f32(ok, B, F, TP, ok, two, None) == ALIGNMENT
    assert lib.leaf_pcen_f32(ok, B, F, TP, ok, ok, two, ok, 1e-6, ok, None) == ALIGNMENT
    assert lib.leaf_pcen_stream_f32(ok, B, F, TP, ok, ok, ok, ok, 1e-6, 0, two, ok, ok, None) == ALIGNMENT
    assert lib.leaf_pcen_stream_f32(ok, B, F, TP, ok, ok, ok, ok, 1e-6, 0, ok, two, ok, None) == ALIGNMENT
    assert lib.leaf_peak_normalize_f32(two, B, Tf, ok, None) == ALIGNMENT and lib.leaf_peak_normalize_f32(ok, B, Tf, two, None) == ALIGNMENT
    assert lib.leaf_gabor_conv_backward_f32(ok, B, Tf, ok, F, K, ok, ok, ok, ws8, 0, None) == ALIGNMENT
    assert lib.leaf_gabor_conv_backward_f32(ok, B, Tf, ok, F, K, ok, two, None, ok, 0, None) == ALIGNMENT
    assert lib.leaf_gabor_conv_backward_f32(ok, B, Tf, ok, F, K, ok, ok, None, ok, 0, None) == WORKSPACE
    assert lib.leaf_squared_modulus_backward_f32(ok, two, B, F, Tf, ok, None) == ALIGNMENT
    assert lib.leaf_gaussian_lowpass_backward_f32(ok, ok, B, F, Tf, ok, K, HOP, ok, ok, ok, ws8, 0, None) == ALIGNMENT
    assert lib.leaf_gaussian_lowpass_backward_f32(ok, ok, B, F, Tf, ok, K, HOP, None, two, ok, ok, 0, None) == ALIGNMENT
    assert lib.leaf_ema_backward_f32(ok, ok, B, F, TP, ok, ok, ok, ws8, 0, None) == ALIGNMENT
    assert lib.leaf_ema_backward_f32(ok, ok, B, F, TP, ok, ok, two, ok, 0, None) == ALIGNMENT
    assert lib.leaf_pcen_backward_f32(ok, ok, B, F, TP, ok, ok, ok, ok, 1e-6, ok, ok, ok, ok, ok, ws8, 0, None) == ALIGNMENT
    assert lib.leaf_pcen_backward_f32(ok, ok, B, F, TP, ok, ok, ok, ok, 1e-6, ok, ok, two, ok, ok, ok, 0, None) == ALIGNMENT
    assert lib.leaf_pcen_backward_f32(ok, ok, B, F, TP, ok, ok, ok, ok, 1e-6, ok, ok, ok, ok, ok, ok, 0, None) == WORKSPACE
    del keep


def test_header_and_status_string_state_the_alignments():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    assert re.search(r"LEAF_ERR_ALIGNMENT = -7,[^\n]*16-byte", header)
    assert b"16-byte" in _native.load().leaf_status_string(-7)
