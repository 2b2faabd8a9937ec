"""The head-only backward on the GPU: ``leaf_backward_head_f32`` (csrc/leaf_head_bwd.hpp) through ``_native.leaf_backward_head``, and the
route ``Leaf`` takes to it when its Gabor kernel and pooling width are frozen.

A. The kernel.  No forward is involved: ``pooled_raw`` and ``grad_out`` are drawn tensors.  The reference is fp64 autograd through
   oracle/leaf_oracle.py's floor (``torch.clamp(pooled, min=1e-5)``) and ``pcen`` on the same ``pooled_raw``, with the gradient of the
   pooling bias taken as the gradient of a per-filter shift of ``pooled_raw``; judged by ``helpers.assert_grad_close`` at the suite's
   bounds.  Rows of 1 .. 1000 frames cross the scan's 128-frame chunk seams and the switch from registers to memory at
   kScanRegChunks * 128 = 512 frames; the batches are placed around the slice length the kernel's own constants give (one slice minus
   a row, one slice, one slice plus a row, three slices with a last one of a single row).
   One convention needs a word: the oracle clamps alpha and root with ``Tensor.clamp``, whose sub-gradient at the bound itself is 1,
   while the reference takes ``torch.min(alpha, 1)`` and ``torch.max(root, 1)`` (postprocessing.py:63-64), whose sub-gradient there is
   1/2 -- the convention the kernels follow (include/leaf_hip.h).  The filters placed exactly ON a bound therefore expect half the
   oracle's (one-sided) derivative; everywhere else the oracle's gradient is taken as it is.
B. The route.  With kernel and pooling width frozen the five remaining gradients must agree with those the same module yields with
   everything trainable (the full backward), nothing of the waveform side may be saved by the forward, and ``create_graph=True`` keeps
   giving the second-order results of the full route.

Nothing here asserts a speed."""
import ctypes
import math
import os
import re

import pytest
import torch

from guarded import guarded, guarded_tensor, unchanged
from helpers import assert_grad_close, make_leaf
from oracle import leaf_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["_pooling._bias", "_compression.alpha", "_compression.delta", "_compression.root", "_compression.ema._weights"]
FROZEN = ["_complex_conv._kernel", "_pooling.weights"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's own constants, and the split of the batch they give (restated; checked against the workspace query below)
# ---------------------------------------------------------------------------------------------------------------------------
def _const(name):
    for header in ("leaf_head_bwd.hpp", "leaf_params.hpp", "leaf_pcen_scan.hpp"):
        m = re.search(r"constexpr int " + name + r" = (\d+)\b", open(os.path.join(REPO, "leaf_pytorch_amd", "csrc", header)).read())
        if m:
            return int(m.group(1))
    raise AssertionError(name)


WAVES, REC, SLICE_ROWS, WG_PER_CU, REG_CHUNKS = (_const(n) for n in ("kHeadWaves", "kHeadRecFloats", "kHeadSliceRows", "kHeadWgPerCu",
                                                                     "kScanRegChunks"))
REG_FRAMES = REG_CHUNKS * 128


def n_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def plan(B, F):
    """(S, L) of head_plan (leaf_head_bwd.hpp)."""
    cap = max(1, WG_PER_CU * n_cus() // F)
    s0 = max(1, min(-(-B // SLICE_ROWS), cap))
    per = -(-B // s0)                                # rows per slice, rounded up to whole rounds of the waves
    L = -(-per // WAVES) * WAVES
    return -(-B // L), L


def expected_workspace(B, TP, F, pcen):
    S, _ = plan(B, F)
    return -(-4 * F // 16) * 16 + 4 * F * S * REC + (4 * F * S * WAVES * TP if pcen and TP > REG_FRAMES else 0)


def ws_bytes(B, TP, F, flags):
    from leaf_pytorch_amd import _native
    with torch.cuda.device(DEV):
        return _native.load().leaf_backward_head_workspace_bytes(B, TP, F, flags)


# ---------------------------------------------------------------------------------------------------------------------------
# A. the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def draw(B, F, TP, seed):
    """pooled_raw over several decades with a tenth of the entries at or below the 1e-5 floor (some on it, some negative) and one row
    entirely below it; grad_out; PCEN parameters perturbed from the defaults.  With F = 5 every filter carries one special value:
    alpha == 1, alpha > 1, root == 1, root < 1, and an ema_w outside [0, 1] together with delta = 1e-31 (the library powf / logf branch)."""
    gen = torch.Generator().manual_seed(seed)
    raw = 10.0 ** (-4.0 + 5.0 * torch.rand(B, F, TP, generator=gen))
    low = torch.rand(B, F, TP, generator=gen) < 0.1
    kind = torch.randint(0, 3, (B, F, TP), generator=gen)
    below = torch.where(kind == 0, torch.full_like(raw, 1e-5), torch.where(kind == 1, 1e-5 * torch.rand(B, F, TP, generator=gen),
                                                                             -torch.rand(B, F, TP, generator=gen)))
    raw = torch.where(low, below, raw)
    if B * F >= 2:
        raw[B - 1, F - 1] = torch.where(torch.arange(TP) % 2 == 0, torch.tensor(-0.5), torch.tensor(3e-6))
    go = torch.randn(B, F, TP, generator=gen)
    r = lambda: 2 * torch.rand(F, generator=gen) - 1
    prm = {"alpha": 0.96 * (1 + 0.03 * r()), "delta": 2.0 * (1 + 0.3 * r()), "root": 2.0 * (1 + 0.3 * r()), "ema_w": 0.04 * (1 + 0.5 * r())}
    tied = {"alpha": [], "root": []}
    if F == 5:
        prm["alpha"][0], prm["alpha"][1] = 1.0, 1.25
        prm["root"][2], prm["root"][3] = 1.0, 0.75
        prm["ema_w"][4] = -0.25 if seed % 2 else 1.5
        prm["delta"][4] = 1e-31
        tied = {"alpha": [0], "root": [2]}
    return raw.float(), go.float(), prm, tied


_REF = {}


def reference(key, raw, go, prm, tied, mode):
    """fp64 autograd through the oracle's floor and PCEN (computed once per drawn case and mode, then shared)."""
    if (key, mode) in _REF:
        return _REF[(key, mode)]
    F = raw.shape[1]
    shift = torch.zeros(F, dtype=torch.float64, requires_grad=True)
    p64 = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    pooled = torch.clamp(raw.double() + shift.reshape(1, -1, 1), min=lo.FLOOR_POOLED)
    if mode == "pcen":
        out = lo.pcen(pooled, p64["alpha"], p64["delta"], p64["root"], p64["ema_w"])
    else:
        out = torch.log1p(pooled) if mode == "log1p" else pooled
    out.backward(go.double())
    ref = {"_pooling._bias": shift.grad}
    if mode == "pcen":
        ref.update({"_compression.alpha": p64["alpha"].grad, "_compression.delta": p64["delta"].grad, "_compression.root": p64["root"].grad,
                    "_compression.ema._weights": p64["ema_w"].grad})
        # exactly ON the bound: torch.min / torch.max of the reference give half of Tensor.clamp's one-sided derivative (module docstring)
        for f in tied["alpha"]:
            ref["_compression.alpha"][f] *= 0.5
        for f in tied["root"]:
            ref["_compression.root"][f] *= 0.5
    _REF[(key, mode)] = ref
    return ref


def head(raw, go, prm, mode, out_bf16=False):
    from leaf_pytorch_amd import _native
    F = raw.shape[1]
    pc = [prm[k].to(DEV) for k in ("alpha", "delta", "root", "ema_w")] if mode == "pcen" else [None] * 4
    return _native.leaf_backward_head(raw.to(DEV), go.to(DEV), torch.zeros(F, device=DEV), *pc, pcen=mode == "pcen", log1p=mode == "log1p",
                                      out_bf16=out_bf16)


def kernel_case(B, F, TP, seed):
    from leaf_pytorch_amd import _native
    raw, go, prm, tied = draw(B, F, TP, seed)
    S, L = plan(B, F)
    ctx = f"(B={B} F={F} frames={TP} S={S} L={L} seed={seed})"
    print(f"head backward {ctx}: {'registers' if TP <= REG_FRAMES else 'memory'} form, last slice of {B - (S - 1) * L} rows")
    assert ws_bytes(B, TP, F, _native.FLAG_PCEN) == expected_workspace(B, TP, F, True), ctx
    assert ws_bytes(B, TP, F, 0) == ws_bytes(B, TP, F, _native.FLAG_LOG1P) == expected_workspace(B, TP, F, False), ctx
    for mode in ("pcen", "off", "log1p"):
        got = head(raw, go, prm, mode)
        ref = reference((B, F, TP, seed), raw, go, prm, tied, mode)
        assert len(got) == 5 and all(g is None for g in got[1:]) == (mode != "pcen")
        for name, g in zip(HEAD, got):
            if g is not None:
                assert g.dtype == torch.float32 and g.shape == (F,)
                assert_grad_close(name, g, ref[name], f"{mode} {ctx}")
        again = head(raw, go, prm, mode)                               # a second call on the same inputs: the same bits
        for name, g, h in zip(HEAD, got, again):
            assert g is None or torch.equal(g, h), (name, mode, ctx)
        # a bfloat16 grad_out: the bits of the float32 call on the widened tensor
        gb = go.to(torch.bfloat16)
        narrow, wide = head(raw, gb, prm, mode, out_bf16=True), head(raw, gb.float(), prm, mode)
        for name, g, h in zip(HEAD, narrow, wide):
            assert g is None or torch.equal(g, h), (name, mode, "bfloat16 grad_out", ctx)
    return raw, go, prm


FRAMES = [1, 2, 127, 128, 129, 511, 512, 513, 1000]


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("TP", FRAMES)
def test_rows_across_chunk_seams_and_the_register_memory_switch(TP, F):
    for B in (1, 2):
        kernel_case(B, F, TP, seed=100 + TP + B)


def split_batches():
    """From the constants: one slice minus a row, one slice, one slice plus a row, and S >= 3 with a last slice of one row."""
    L = SLICE_ROWS
    return [L - 1, L, L + 1, 2 * L + 1]


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("TP", [129, 513])
@pytest.mark.parametrize("which", range(4))
def test_batches_around_the_slice_length(which, TP, F):
    B = split_batches()[which]
    S, L = plan(B, F)
    # the restated plan puts these batches where they are meant to be (it is checked against the workspace query in kernel_case)
    assert L == SLICE_ROWS and (S, B - (S - 1) * L) == [(1, L - 1), (1, L), (2, 1), (3, 1)][which], (B, S, L)
    kernel_case(B, F, TP, seed=300 + 10 * which + TP)


def test_many_slices_through_the_staged_reducer():
    """More records per filter than the reducer brings into LDS at a time (kHeadStage), short rows."""
    stage = _const("kHeadStage")
    B = SLICE_ROWS * (stage + 2) + 1
    assert plan(B, 1)[0] > stage or WG_PER_CU * n_cus() <= stage          # (a small device caps S below the stage)
    kernel_case(B, 1, 3, seed=77)


@pytest.mark.parametrize("B,F,TP", [(17, 5, 129), (9, 5, 513)])
def test_exact_size_poisoned_guarded_buffers(B, F, TP):
    """The C ABI call itself on an exact-size, 0xFF-poisoned, guarded workspace and guarded outputs and inputs: the same bits as through
    the wrapper, every guard intact, the inputs unchanged -- twice on the same workspace (the second call finds the first one's tickets)."""
    from leaf_pytorch_amd import _native
    lib = _native.load()
    raw, go, prm, _ = draw(B, F, TP, seed=500 + TP)
    want = head(raw, go, prm, "pcen")
    flags = _native.FLAG_PCEN
    nbytes = ws_bytes(B, TP, F, flags)
    ins = [guarded_tensor(t.to(DEV)) for t in (raw, go, prm["alpha"], prm["delta"], prm["root"], prm["ema_w"])]
    ws = guarded(nbytes, 0xFF)
    outs = [guarded(4 * F, 0xFF) for _ in range(5)]
    stream = _native.stream_ptr(torch.device(DEV))
    for attempt in range(2):
        with torch.cuda.device(DEV):
            rc = lib.leaf_backward_head_f32(ins[0].ptr, ins[1].ptr, B, TP, F, *[g.ptr for g in ins[2:]], flags, *[o.ptr for o in outs],
                                            ws.ptr, nbytes, stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        ws.check(f"workspace, call {attempt}")
        for name, o, w in zip(HEAD, outs, want):
            o.check(name)
            assert torch.equal(o.view(torch.float32), w), (name, attempt)
        for g in ins:
            unchanged(g, "input")
        for o in outs:
            o.fill(0xFF)
    # one byte short: refused before anything runs; a workspace off its 16-byte alignment too
    with torch.cuda.device(DEV):
        args = (ins[0].ptr, ins[1].ptr, B, TP, F, *[g.ptr for g in ins[2:]], flags, *[o.ptr for o in outs])
        assert lib.leaf_backward_head_f32(*args, ws.ptr, nbytes - 1, stream) == -3
        assert lib.leaf_backward_head_f32(*args, ctypes.c_void_p(ws.address + 4), nbytes, stream) == -7
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.bytes() == 0xFF).all())


def test_captured_into_a_graph_and_replayed():
    """The call captured once into a HIP graph: every replay re-zeroes the tickets and gives the eager call's bits.  (Under capture the
    tickets are zeroed by a kernel node: a captured memset node wrote zeros on the first replay only, include/leaf_hip.h.)"""
    B, F, TP = 17, 5, 129
    raw, go, prm, _ = draw(B, F, TP, seed=600)
    want = head(raw, go, prm, "pcen")
    rawd, god = raw.to(DEV), go.to(DEV)
    pc = [prm[k].to(DEV) for k in ("alpha", "delta", "root", "ema_w")]
    from leaf_pytorch_amd import _native
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _native.leaf_backward_head(rawd, god, torch.zeros(F, device=DEV), *pc)
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = _native.leaf_backward_head(rawd, god, torch.zeros(F, device=DEV), *pc)
    for _ in range(3):
        for t in got:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(HEAD, got, want):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("pcen", [True, False])
def test_empty_batch_gives_zeros(pcen):
    from leaf_pytorch_amd import _native
    F, TP = 5, 7
    vec = lambda: torch.rand(F, device=DEV)
    got = _native.leaf_backward_head(torch.empty(0, F, TP, device=DEV), torch.empty(0, F, TP, device=DEV), vec(),
                                     *([vec(), vec(), vec(), vec()] if pcen else [None] * 4), pcen=pcen)
    assert all((g is None) == (not pcen) for g in got[1:])
    assert all(g is None or (g.shape == (F,) and not bool(g.any())) for g in got)
    # the C ABI itself: memsets on poisoned outputs, nothing else is touched
    lib = _native.load()
    outs = [guarded(4 * F, 0xFF) for _ in range(5)]
    with torch.cuda.device(DEV):
        rc = lib.leaf_backward_head_f32(None, None, 0, TP, F, None, None, None, None, _native.FLAG_PCEN if pcen else 0,
                                        *[o.ptr if (pcen or i == 0) else None for i, o in enumerate(outs)], None, 0,
                                        _native.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        o.check("empty batch")
        assert bool((o.bytes() == (0 if (pcen or i == 0) else 0xFF)).all()), i


# ---------------------------------------------------------------------------------------------------------------------------
# B. through Leaf
# ---------------------------------------------------------------------------------------------------------------------------
def leaf_params(F, K, hop, pcen, seed):
    gen = torch.Generator().manual_seed(seed)
    geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
    params = lo.default_params(geo, pcen, kernel=torch.stack(
        [0.1 + torch.rand(F, generator=gen) * (math.pi - 0.2), 3.0 + torch.rand(F, generator=gen) * K / 4], dim=1))
    return {k: v * (1 + 0.1 * (2 * torch.rand(v.shape, generator=gen) - 1)) for k, v in params.items()}


@pytest.fixture
def routes(monkeypatch):
    """Every decision ``_ops.backward_route`` takes during the test, in order."""
    from leaf_pytorch_amd import _ops
    taken, real = [], _ops.backward_route

    def spy(*a):
        taken.append(real(*a))
        return taken[-1]
    monkeypatch.setattr(_ops, "backward_route", spy)
    return taken


def set_trainable(m, frozen):
    for name, p in m.named_parameters():
        p.requires_grad_(not (frozen and name in FROZEN))
        p.grad = None


def both_routes(m, step, routes, ctx):
    """``step(m)`` runs forward and backward.  First with every parameter trainable (the full route: today's backward), then with the
    Gabor kernel and the pooling width frozen (the head route): the five remaining gradients agree, the frozen two stay None."""
    set_trainable(m, frozen=False)
    del routes[:]
    step(m)
    assert routes and set(routes) == {"full"}, (routes, ctx)
    ref = {k: p.grad.clone() for k, p in m.named_parameters()}
    set_trainable(m, frozen=True)
    del routes[:]
    step(m)
    assert routes and set(routes) == {"head"}, (routes, ctx)
    got = dict(m.named_parameters())
    for name in FROZEN:
        assert got[name].grad is None, (name, ctx)
    seen = 0
    for name in HEAD:
        if name in got:
            assert got[name].grad is not None and got[name].grad.shape == ref[name].shape, (name, ctx)
            assert_grad_close(name, got[name].grad, ref[name], f"head against full {ctx}")
            seen += 1
    assert seen == (5 if m._compression is not None else 1), ctx


def plain_step(x, go):
    def step(m):
        m(x).backward(go)
    return step


def module_and_clips(F, K, hop, T, B, pcen, seed, dtype=torch.float32, out_dtype=torch.float32):
    m = make_leaf(F, K, hop, pcen, leaf_params(F, K, hop, pcen, seed), DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 1, T, generator=gen)
    x = (x.clamp(-3, 3) * 8000).to(torch.int16) if dtype == torch.int16 else x.to(dtype)
    go = torch.randn(B, F, (T - 1) // hop + 1, generator=gen).to(out_dtype)
    return m, x.to(DEV), go.to(DEV)


@pytest.mark.parametrize("T", [1, 1600, 3201])
def test_static_16k(T, routes):
    m, x, go = module_and_clips(5, 401, 160, T, 2, True, seed=11 + T)
    both_routes(m, plain_step(x, go), routes, f"(16 kHz static T={T})")


def test_static_32k(routes):
    m, x, go = module_and_clips(8, 801, 320, 3201, 2, True, seed=21)
    both_routes(m, plain_step(x, go), routes, "(32 kHz static F=8)")


def test_runtime_geometry_22k(routes):
    m, x, go = module_and_clips(4, 552, 220, 5000, 2, True, seed=22)
    both_routes(m, plain_step(x, go), routes, "(22.05 kHz run-time geometry K=552)")


def test_forward_mixup(routes):
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=23)
    perm, lam = torch.tensor([1, 0], dtype=torch.int32, device=DEV), torch.tensor([0.3, 0.8], device=DEV)
    both_routes(m, lambda mod: mod.forward_mixup(x, perm, lam).backward(go), routes, "(forward_mixup)")


def test_int16_waveform(routes):
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=24, dtype=torch.int16)
    assert x.dtype == torch.int16
    both_routes(m, plain_step(x, go), routes, "(int16 waveform)")


def test_bfloat16_waveform(routes):
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=25, dtype=torch.bfloat16, out_dtype=torch.bfloat16)
    both_routes(m, plain_step(x, go), routes, "(bfloat16 waveform)")


def test_output_dtype_bfloat16(routes):
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=26, out_dtype=torch.bfloat16)
    m.output_dtype(torch.bfloat16)
    assert m(x).dtype == torch.bfloat16
    both_routes(m, plain_step(x, go), routes, "(output_dtype(torch.bfloat16))")


def test_log_compression(routes):
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, False, seed=27)
    m.log_compression()
    both_routes(m, plain_step(x, go), routes, "(log_compression, PCEN off)")
    m.log_compression(False)
    both_routes(m, plain_step(x, go), routes, "(PCEN off)")


def test_full_transforms(routes):
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=28)
    m.full_transforms()
    both_routes(m, plain_step(x, go), routes, "(full_transforms)")


@pytest.mark.parametrize("mixed", [False, True])
def test_ctypes_autograd_path(mixed, routes, monkeypatch):
    """The dispatcher ops masked off: ``frontend._LeafFn`` over the ctypes layer takes the same decision."""
    from leaf_pytorch_amd import _native, _ops
    monkeypatch.setattr(_ops, "available", lambda: False)        # the ops library masked off: _LeafFn over ctypes
    calls = []
    real = _native.leaf_backward_head
    monkeypatch.setattr(_native, "leaf_backward_head", lambda *a, **k: calls.append(1) or real(*a, **k))
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=29)
    perm, lam = torch.tensor([1, 0], dtype=torch.int32, device=DEV), torch.tensor([0.3, 0.8], device=DEV)
    step = (lambda mod: mod.forward_mixup(x, perm, lam).backward(go)) if mixed else plain_step(x, go)
    both_routes(m, step, routes, f"(_LeafFn mixed={mixed})")
    assert len(calls) == 1                                       # the frozen step, and only it


def test_full_backward_switch_keeps_the_full_route():
    """``Leaf.full_backward()``: the frozen module on the full route (what tools/bench_backward.py --frozen-filters compares with)."""
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=30)
    set_trainable(m, frozen=True)
    m(x).backward(go)
    head_grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert set(head_grads) == set(HEAD)
    set_trainable(m, frozen=True)
    m.full_backward()
    m(x).backward(go)
    for name, p in m.named_parameters():
        if name in FROZEN:
            assert p.grad is None
        else:
            assert_grad_close(name, head_grads[name], p.grad, "head against the forced full route")


def test_compiled_training_step():
    """One ``torch.compile(fullgraph=True)`` training step of the frozen module: traced through leaf_amd::backward_head's fake."""
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=31)
    set_trainable(m, frozen=False)
    m(x).backward(go)
    ref = {k: p.grad.clone() for k, p in m.named_parameters()}
    set_trainable(m, frozen=True)
    torch._dynamo.reset()
    cm = torch.compile(m, fullgraph=True)
    (cm(x) * go).sum().backward()
    got = dict(m.named_parameters())
    for name in FROZEN:
        assert got[name].grad is None
    for name in HEAD:
        assert_grad_close(name, got[name].grad, ref[name], "compiled frozen step against the eager full route")


def test_frozen_training_step_is_hip_graph_capturable():
    """Forward + head backward of the frozen module captured into one HIP graph (as tests/test_gpu_backward.py does for the full
    step): replays on new clips return the eager step's gradients bit for bit."""
    m, x, go = module_and_clips(5, 401, 160, 1600, 4, True, seed=34)
    set_trainable(m, frozen=True)
    xs = [torch.randn_like(x) for _ in range(3)]
    static_x = x.clone()

    def step():
        torch.autograd.backward(m(static_x), go)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(3):
            m.zero_grad(set_to_none=True)
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    m.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        step()
    params = dict(m.named_parameters())
    for xi in xs:
        static_x.copy_(xi)
        graph.replay()
        got = {k: params[k].grad.clone() for k in HEAD}
        m2, _, _ = module_and_clips(5, 401, 160, 1600, 4, True, seed=34)
        set_trainable(m2, frozen=True)
        torch.autograd.backward(m2(xi), go)
        for k, p in m2.named_parameters():
            assert (p.grad is None) == (k in FROZEN) and (k in FROZEN or torch.equal(got[k], p.grad)), k


@pytest.mark.parametrize("call", ["forward", "forward_mixup", "ctypes"])
def test_forward_saves_nothing_of_the_waveform_side(call, monkeypatch):
    """Under saved_tensors_hooks: no tensor the forward saves for the backward is the waveform (nor perm, nor lam, nor the frozen two)."""
    from leaf_pytorch_amd import _ops
    if call == "ctypes":
        monkeypatch.setattr(_ops, "available", lambda: False)
    m, x, go = module_and_clips(5, 401, 160, 1600, 2, True, seed=32)
    perm, lam = torch.tensor([1, 0], dtype=torch.int32, device=DEV), torch.tensor([0.3, 0.8], device=DEV)
    set_trainable(m, frozen=True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.data_ptr()) or t, lambda t: t):
        out = m.forward_mixup(x, perm, lam) if call == "forward_mixup" else m(x)
    assert saved, "the forward saved nothing at all"
    params = dict(m.named_parameters())
    banned = {"x": x, "perm": perm, "lam": lam, **{k: params[k] for k in FROZEN}}
    for name, t in banned.items():
        assert t.data_ptr() not in saved, f"the forward saved {name}"
    out.backward(go)
    assert all(params[k].grad is not None for k in HEAD) and all(params[k].grad is None for k in FROZEN)


def test_create_graph_on_the_frozen_module_keeps_the_second_order_results():
    """A gradient penalty on the five head gradients: the frozen module (whose backward is leaf_amd::backward_head and its own
    autograd formula, from the saved pooled tensor) against the same module with everything trainable (leaf_amd::backward and the
    formula of _second_order.py, from the waveform)."""
    F, K, hop, T = 4, 401, 160, 1100
    results = {}
    for frozen in (False, True):
        m, x, go = module_and_clips(F, K, hop, T, 2, True, seed=33)
        set_trainable(m, frozen=frozen)
        params = dict(m.named_parameters())
        out = m(x)
        first = torch.autograd.grad(out, [params[k] for k in HEAD], go, create_graph=True)
        assert all(g.requires_grad for g in first)
        sum(g.square().sum() for g in first).backward()
        results[frozen] = ({k: g.detach().clone() for k, g in zip(HEAD, first)}, {k: params[k].grad.clone() for k in HEAD})
        if frozen:
            assert all(params[k].grad is None for k in FROZEN)
    for name in HEAD:
        assert_grad_close(name, results[True][0][name], results[False][0][name], "first order, frozen against trainable")
        assert_grad_close(name, results[True][1][name], results[False][1][name], "gradient of the penalty, frozen against trainable")
