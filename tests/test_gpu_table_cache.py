"""The self-validating table cache of the default no-grad forward (include/leaf_hip.h: leaf_forward_cached_f32; the dispatcher op
keeps the buffers, csrc/torch_binding.cpp).  Every comparison is ``torch.equal`` against the same call with
LEAF_ALGO_NO_TABLE_CACHE -- the table launch that rebuilds everything into the workspace -- never a tolerance: the cache may only
skip work, not change a bit.  Default shape: F = 40, 16 kHz, B = 24, the smallest batch the smoke sends through the workgroup kernel
(240 blocks, 120 workgroups)."""
import ctypes

import pytest
import torch

from guarded import guarded, guarded_tensor, unchanged
from leaf_pytorch_amd import Leaf, _native, _ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = _native
B, T, F, K, HOP = 24, 16000, 40, 401, 160


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    N.load()
    _ops.load()


def cached_calls():
    """Calls the dispatcher op has sent through leaf_forward_cached_f32 so far."""
    return int(torch.ops.leaf_amd.table_cache_info()[1])


def call(m, x, cached=True):
    algo = m._algo
    m._algo = algo if cached else algo | N.ALGO_NO_TABLE_CACHE
    try:
        with torch.no_grad():
            out = m(x)
    finally:
        m._algo = algo
    torch.cuda.synchronize()
    return out


def waveform(b, t, seed, dtype=torch.float32):
    x = 2 * torch.rand(b, 1, t, generator=torch.Generator().manual_seed(seed)) - 1
    if dtype == torch.int16:
        return (x * 32767).round().to(torch.int16).to(DEV)
    return x.to(dtype).to(DEV)


def module(pcen=True, log1p=False, seed=None):
    m = Leaf(pcen_compression=pcen).eval().to(DEV)
    if log1p:
        m.log_compression()
    if seed is not None:                                     # other parameters, the same geometry
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            m._complex_conv._kernel.mul_((1 + 0.05 * (2 * torch.rand(F, 2, generator=g) - 1)).to(DEV))
            m._pooling.weights.mul_((1 + 0.2 * (2 * torch.rand(1, 1, F, 1, generator=g) - 1)).to(DEV))
    return m


def routed(fn):
    """Run ``fn`` and return (its result, how many calls it sent through the cached entry)."""
    n0 = cached_calls()
    out = fn()
    return out, cached_calls() - n0


@pytest.mark.parametrize("mode,dtype", [("pcen", torch.float32), ("off", torch.float32), ("log1p", torch.float32),
                                        ("pcen", torch.bfloat16), ("pcen", torch.int16)],
                         ids=["pcen", "pcen-off", "log1p", "bf16-x", "int16-x"])
def test_miss_hit_hit(mode, dtype):
    m = module(pcen=mode == "pcen", log1p=mode == "log1p")
    x = waveform(B, T, 1, dtype)
    assert N.load().leaf_auto_algo(B, T, F, K, HOP) == N.ALGO_FFT_WG
    ref, n = routed(lambda: call(m, x, cached=False))
    assert n == 0                                            # the reference is today's route
    for i in range(3):
        out, n = routed(lambda: call(m, x))
        assert n == 1, f"the dispatcher's cached route does not admit {dtype} / {mode}"
        assert out.dtype == ref.dtype and torch.equal(out, ref), f"call {i}"


def test_clip_length_change():
    """Other edge lists, a partial last block; the buffers are per clip length and each validates by content."""
    m = module()
    for i, t in enumerate((16000, 12345, 4000, 16000)):
        x = waveform(B, t, 10 + i)
        out, n = routed(lambda: call(m, x))
        assert n == 1
        assert torch.equal(out, call(m, x, cached=False)), t


@pytest.mark.parametrize("which", ["kernel", "pool_w"])
def test_write_that_bypasses_the_version_counter(which):
    m = module()
    x = waveform(B, T, 2)
    before = call(m, x)
    assert torch.equal(call(m, x), before)                   # (a hit)
    if which == "kernel":
        m._complex_conv._kernel.data[3, 1] *= 1.01
    else:
        m._pooling.weights.data[0, 0, 5, 0] *= 0.9
    after, n = routed(lambda: call(m, x))
    assert n == 1
    assert torch.equal(after, call(m, x, cached=False))
    assert not torch.equal(after, before)
    assert torch.equal(call(m, x), after)                    # (a hit again)


def test_only_the_touched_filter_changes():
    m = module()
    x = waveform(B, T, 3)
    before = call(m, x)
    m._complex_conv._kernel.data[7, 0] *= 1.003
    after = call(m, x)
    assert torch.equal(after, call(m, x, cached=False))
    others = [f for f in range(F) if f != 7]
    assert torch.equal(after[:, others], before[:, others])
    assert not torch.equal(after[:, 7], before[:, 7])


def test_two_modules_called_alternately():
    m1, m2 = module(), module(seed=5)
    x = waveform(B, T, 4)
    r1, r2 = call(m1, x, cached=False), call(m2, x, cached=False)
    assert not torch.equal(r1, r2)
    for _ in range(3):
        assert torch.equal(call(m1, x), r1)
        assert torch.equal(call(m2, x), r2)


def test_side_stream():
    m = module()
    x = waveform(B, T, 6)
    ref = call(m, x, cached=False)
    first = call(m, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out, n = routed(lambda: call(m, x))
        again = call(m, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert n == 1
    assert torch.equal(first, ref) and torch.equal(out, ref) and torch.equal(again, ref)


def test_per_wave_kernel():
    """B = 3 under LEAF_ALGO_FFT: the per-wave kernel, tables from the plain table launch, frames through the row kernel."""
    m = module()
    m._algo = N.ALGO_FFT
    x = waveform(3, T, 7)
    ref = call(m, x, cached=False)
    for _ in range(3):
        out, n = routed(lambda: call(m, x))
        assert n == 1 and torch.equal(out, ref)
    m._complex_conv._kernel.data[3, 1] *= 1.01
    after = call(m, x)
    assert torch.equal(after, call(m, x, cached=False)) and not torch.equal(after, ref)
    assert torch.equal(call(m, x), after)


def test_clips_that_straddle_workgroups():
    """B = 25, T = 20000: 13 blocks per clip dealt contiguously, so clips straddle workgroups and the row kernel finalizes them."""
    m = module()
    assert N.load().leaf_auto_algo(25, 20000, F, K, HOP) == N.ALGO_FFT_WG
    x = waveform(25, 20000, 8)
    ref = call(m, x, cached=False)
    for _ in range(2):
        out, n = routed(lambda: call(m, x))
        assert n == 1 and torch.equal(out, ref)


def test_bias_change_between_calls():
    """The band plan follows the pooling bias of the call; the tables (and their stamps) do not depend on it."""
    m = module()
    x = waveform(B, T, 9)
    first = call(m, x)
    assert torch.equal(first, call(m, x, cached=False))
    m._pooling._bias.data.fill_(0.05)                        # low enough to move filters out of the band classes
    m._pooling._bias.data[::3] = 2.0
    out = call(m, x)
    assert torch.equal(out, call(m, x, cached=False))
    assert not torch.equal(out, first)


# ---- the C ABI, raw, on guarded buffers --------------------------------------------------------------------------------------------
def _abi_case():
    lib = N.load()
    m = module()
    sd = m.state_dict()
    keys = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
            "_compression.root", "_compression.ema._weights"]
    params = [guarded_tensor(sd[k].reshape(-1).float()) for k in keys]
    x = guarded_tensor(waveform(B, T, 11).reshape(B, T))
    TP = lib.leaf_num_frames(T, K, HOP)
    algo = N.ALGO_FFT_WG
    ws_bytes = lib.leaf_workspace_bytes(B, T, F, K, HOP, algo)
    cache_bytes = lib.leaf_table_cache_bytes(F, K, HOP, T)
    assert ws_bytes > 0 and cache_bytes > 0
    return lib, params, x, TP, algo, ws_bytes, cache_bytes


def _cached(lib, x, params, algo, out, ws, ws_bytes, cache_ptr, cache_bytes):
    return lib.leaf_forward_cached_f32(x.ptr, B, T, *[p.ptr for p in params], F, K, HOP, N.FLAG_PCEN, algo, out.ptr, ws.ptr, ws_bytes,
                                       cache_ptr, cache_bytes, None)


def test_c_abi_exact_size_cache_inside_guard_pages():
    lib, params, x, TP, algo, ws_bytes, cache_bytes = _abi_case()
    cache = guarded(cache_bytes, 0)                          # zeroed once, before first use
    ref = guarded(B * F * TP * 4, 0xFF)
    ws = guarded(ws_bytes, 0xFF)
    rc = lib.leaf_forward_f32(x.ptr, B, T, *[p.ptr for p in params], F, K, HOP, N.FLAG_PCEN, algo, ref.ptr, ws.ptr, ws_bytes, None)
    torch.cuda.synchronize()
    assert rc == 0
    for i in range(2):                                       # a miss, then a hit; the workspace poisoned both times
        out = guarded(B * F * TP * 4, 0xFF)
        ws.fill(0xFF)
        rc = _cached(lib, x, params, algo, out, ws, ws_bytes, cache.ptr, cache_bytes)
        torch.cuda.synchronize()
        assert rc == 0
        for g, name in ((cache, "cache"), (out, "out"), (ws, "workspace")):
            g.check(f"call {i}: {name}")
        for g in (x, *params):
            unchanged(g, f"call {i}")
        assert torch.equal(out.view(torch.float32), ref.view(torch.float32)), f"call {i}"
    # with the option bit the cache is neither read nor written
    cache.fill(0xFF)
    out = guarded(B * F * TP * 4, 0xFF)
    rc = _cached(lib, x, params, algo | N.ALGO_NO_TABLE_CACHE, out, ws, ws_bytes, cache.ptr, cache_bytes)
    torch.cuda.synchronize()
    assert rc == 0 and bool((cache.bytes() == 0xFF).all())
    assert torch.equal(out.view(torch.float32), ref.view(torch.float32))


def test_c_abi_refuses_a_short_or_misaligned_cache_before_any_launch():
    lib, params, x, TP, algo, ws_bytes, cache_bytes = _abi_case()
    out = guarded(B * F * TP * 4, 0xFF)
    ws = guarded(ws_bytes, 0xFF)
    cache = guarded(cache_bytes - 1, 0)
    assert _cached(lib, x, params, algo, out, ws, ws_bytes, cache.ptr, cache_bytes - 1) == -3        # LEAF_ERR_WORKSPACE
    off = guarded(cache_bytes, 0, offset=4)
    assert _cached(lib, x, params, algo, out, ws, ws_bytes, off.ptr, cache_bytes) == -7              # LEAF_ERR_ALIGNMENT
    torch.cuda.synchronize()
    # nothing ran: the output and the workspace keep their fill, the caches their zeros
    assert bool((out.bytes() == 0xFF).all()) and bool((ws.bytes() == 0xFF).all())
    assert not bool(cache.bytes().any()) and not bool(off.bytes().any())
    for g in (out, ws, cache, off):
        g.check("refused call")
