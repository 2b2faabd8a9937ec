"""Backward parity at clip-length edges and on PCEN rows beyond 512 frames.

tests/test_gpu_backward.py holds every backward family to fp64 autograd through the oracle at clips of a few thousand samples; this
file runs the same comparison (helpers.assert_grad_close at the suite's bounds, helpers.make_leaf, oracle/leaf_oracle.py) where the
kernels index past an end if they are wrong:

  A. `pcen_bwd_scan_kernel` on rows across its 128-frame chunk seams and beyond the kScanRegChunks * 128 = 512 frames it keeps in
     registers (longer rows store the smoother's values and read them back), through the overlap-save backward and through the forced
     MFMA backward (the `gcols / col_of` stores).
  B. every backward family on the lattice of clip lengths T in {1, 2, 3, h-1, h, h+1, padL, padL+1, K-1, K, K+1, L-1, L, L+1, 2L, 2L+1}
     (h the hop, padL = K/2 + K%2 - 1 the left padding, L the block length of the family's plan), the batch sized from the device's CU
     count so that the call lies on the intended side of the dispatcher's threshold.

Vanishing columns.  Below one hop a clip is one frame over a cut window: at T = 1 the fp64 gradients of mu, of the pooling weights and
of the smoother weights are exactly 0, at T in {2, 3} the pooling-weight column peaks at 7e-7 / 2e-6 (default 16 kHz parameters, 96
clips).  Such a column cannot be judged against its own largest entry, so for T < h - 1 the column scale of both bounds is
max(max|r_col|, 1e-3 * max|r_col at T = h + 1|), the second term from the fp64 oracle on the same family, seed and batch -- a scale from
the reference alone.  An exactly zero reference column keeps the helper's absolute rule; from T = h - 1 on the helper applies unmodified.

Every case prints the threshold or forced selector that served it; with LEAF_GRAD_LOG set every comparison is recorded
(tools/summarize_grad_log.py --by-family; profiles/backward_edges.txt).

Found with this file and fixed: a clip of ONE frame with PCEN on (T <= h) missed the per-filter bound in every family alike (39 of the
473 cases: 1.0x .. 8.0x of bound (B) at column figures of 1.0e-6 .. 1.2e-5; a draw with all alphas within 8e-3 of their clamp 61x, and
2.1e-4 on bound (A)).  With one frame the smoother's state is the frame itself, M = p, and dL/dp = (dv / u) (1 - alpha p / (floor + M)):
`pcen_bwd_scan_kernel` formed it as the difference of two rounded products that agree to 1 - alpha, losing 25x .. 125x their rounding.
It now takes the frame's own share in factored form and starts the smoother from M_0 = p_0 exactly (leaf_backward.hpp); all 473 cases
pass on an MI355X (256 CUs), worst per-filter figure 0.34 of the bound, worst column figure 4.0e-5 (profiles/backward_edges.txt)."""
import json
import math

import pytest
import torch

import helpers
from helpers import GRAD_COL_TOL, GRAD_ENTRY_ATOL, GRAD_ENTRY_RTOL, assert_grad_close, grad_columns, make_leaf
from oracle import leaf_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
         "_compression.root", "_compression.ema._weights"]
FLOOR_OF_REFERENCE = 1e-3          # share of the column's largest entry at T = h + 1 below which a column of a tiny clip is not resolved


def n_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def min_blocks(sixteenths):
    """leaf_kernels.hip, fft_wg_bwd_min_blocks: blocks from which a workgroup backward serves the call."""
    return n_cus() * sixteenths // 16


def clips_above(sixteenths, nblk):
    """The smallest batch whose blocks exceed the threshold by at least one."""
    return -(-(min_blocks(sixteenths) + 1) // nblk)


def lattice(K, hop, L):
    padL = K // 2 + K % 2 - 1
    return sorted({1, 2, 3, hop - 1, hop, hop + 1, padL, padL + 1, K - 1, K, K + 1, L - 1, L, L + 1, 2 * L, 2 * L + 1})


def oracle_grads(x, params, geo, pcen, grad_out, need_dx=False, log1p=False):
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
    x64 = x.double().requires_grad_(need_dx)
    out = lo.leaf_forward(x64, p64, geo, pcen, torch.float64)
    if log1p:
        out = torch.log1p(out)
    out.backward(grad_out.double())
    return {k: v.grad for k, v in p64.items()}, (x64.grad if need_dx else None)


def draw(F, K, hop, T, B, pcen, seed, kernel=None, over=None):
    """Parameters first, then the clips and the incoming gradient: the parameters of a (family, seed) do not depend on T."""
    gen = torch.Generator().manual_seed(seed)
    geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
    if kernel is None:
        params = lo.default_params(geo, pcen, kernel=torch.stack(
            [0.1 + torch.rand(F, generator=gen) * (math.pi - 0.2), 3.0 + torch.rand(F, generator=gen) * K / 4], dim=1))
        params = {k: v * (1 + 0.1 * (2 * torch.rand(v.shape, generator=gen) - 1)) for k, v in params.items()}
    else:                                                    # a given filterbank keeps its (mu, sigma): the band classes are its own
        params = lo.default_params(geo, pcen, kernel=kernel.clone())
        params = {k: (v * (1 + 0.05 * (2 * torch.rand(v.shape, generator=gen) - 1)) if "kernel" not in k else v) for k, v in params.items()}
    if over and pcen:
        params.update({k: v.clone() for k, v in over.items()})
    x = torch.randn(B, 1, T, generator=gen)
    grad_out = torch.randn(B, F, (T - 1) // hop + 1, generator=gen)
    return geo, params, x, grad_out


_LAST = {}


def drawn_with_reference(F, K, hop, T, B, pcen, seed, need_dx, kernel, over, log1p):
    """draw() and its fp64 gradients, computed once for calls that follow each other on the same clips (band / full transforms)."""
    key = (F, K, hop, T, B, pcen, seed, need_dx, log1p, None if kernel is None else tuple(kernel.reshape(-1).tolist()), over is None)
    if _LAST.get("key") != key:
        geo, params, x, go = draw(F, K, hop, T, B, pcen, seed, kernel, over)
        _LAST.update(key=key, value=(geo, params, x, go, *oracle_grads(x, params, geo, pcen, go, need_dx, log1p)))
    return _LAST["value"]


_FLOORS = {}


def column_floor(key, F, K, hop, B, pcen, seed, need_dx, kernel, over, log1p):
    """1e-3 of every column's largest fp64 entry at T = h + 1, same family, seed and batch."""
    if key not in _FLOORS:
        geo, params, x, go = draw(F, K, hop, hop + 1, B, pcen, seed, kernel, over)
        ref, ref_dx = oracle_grads(x, params, geo, pcen, go, need_dx, log1p)
        fl = {}
        for name, r in ref.items():
            for label, col in grad_columns(name, r):
                fl[label] = FLOOR_OF_REFERENCE * float(col.abs().max())
        if need_dx:
            fl["x"] = FLOOR_OF_REFERENCE * float(ref_dx.abs().max())
        _FLOORS[key] = fl
    return _FLOORS[key]


def check(name, g, r, ctx, floor=None, entrywise=True):
    """helpers.assert_grad_close; with `floor` (T < h - 1) the column scale of bounds (A) and (B) is max(max|r_col|, floor[column])."""
    if floor is None:
        return assert_grad_close(name, g, r, ctx, entrywise=entrywise)
    g = g.detach().cpu().double().reshape(r.shape)
    r = r.detach().cpu().double()
    for (label, gc), (_, rc) in zip(grad_columns(name, g), grad_columns(name, r)):
        top = float(rc.abs().max()) if rc.numel() else 0.0
        if top == 0.0:                                       # an exactly zero column: the helper's absolute rule
            assert_grad_close(label, gc, rc, ctx, entrywise=entrywise)
            continue
        scale = max(top, floor[label])
        d = (gc - rc).abs()
        ea = float(d.max()) / scale
        eb = float((d / (GRAD_ENTRY_RTOL * rc.abs() + GRAD_ENTRY_ATOL * scale)).max())
        if helpers._GRAD_LOG:
            with open(helpers._GRAD_LOG, "a") as fh:
                fh.write(json.dumps({"column": label, "rel_to_col_max": ea, "entry_bound_used": eb if entrywise else None,
                                     "ctx": str(ctx), "floored": floor[label] > top}) + "\n")
        assert ea < GRAD_COL_TOL, f"{label}: {ea:.3e} of the column's scale {scale:.3e} (largest entry {top:.3e}; bound {GRAD_COL_TOL:.0e}) {ctx}"
        if entrywise:
            assert eb < 1.0, (f"{label}: an entry is off by {eb:.2f}x the per-filter bound ({GRAD_ENTRY_RTOL:.0e} |r_f| + "
                              f"{GRAD_ENTRY_ATOL:.0e} x {scale:.3e}); column figure {ea:.3e} {ctx}")


def vs_full(name, gb, gf, r, bound, ctx, floor=None):
    """Band-task gradients against the full-transform backward's, per column of the reference gradient's scale (tests/test_gpu_backward.py)."""
    gb, gf = gb.cpu().double().reshape(r.shape), gf.cpu().double().reshape(r.shape)
    for (label, cb), (_, cf), (_, cr) in zip(grad_columns(name, gb), grad_columns(name, gf), grad_columns(name, r.double())):
        scale = max(float(cr.abs().max()), floor[label] if floor else 0.0)
        d = float((cb - cf).abs().max()) / (scale + 1e-12)
        assert d < bound, (label, d, ctx)


def native_args(params, pcen):
    return [params[k].to(DEV) for k in NAMES[:3]] + ([params[k].to(DEV) for k in NAMES[3:]] if pcen else [None] * 4)


def edge_case(family, F, K, hop, T, B, pcen, seed, need_dx=False, kernel=None, over=None, forced=None, full=False, log1p=False,
              served=""):
    """One clip shape through one backward family: the module under autograd (the backward gets the pooled tensor its forward saved)
    and leaf_backward_f32 recomputing that tensor itself, every gradient against fp64 autograd through the oracle.  `forced`: the
    keywords that force the staged / MFMA backward (the C ABI call alone).  Returns (the direct call's gradients, reference, floor)."""
    from leaf_pytorch_amd import _native
    geo, params, x, go, ref, ref_dx = drawn_with_reference(F, K, hop, T, B, pcen, seed, need_dx, kernel, over, log1p)
    floor = None
    if T < hop - 1:
        floor = column_floor((F, K, hop, B, pcen, seed, need_dx, log1p, kernel is None, over is None), F, K, hop, B, pcen, seed, need_dx, kernel, over, log1p)
    ctx = f"(family={family} T={T} B={B} F={F} K={K} hop={hop} pcen={pcen} log1p={log1p} dx={need_dx} full={full} seed={seed})"
    print(f"{family}: T={T} B={B} frames={(T - 1) // hop + 1} served by {served or 'the default dispatch'}"
          f"{' [columns floored at 1e-3 of T = h + 1]' if floor else ''}")
    if forced is None:
        m = make_leaf(F, K, hop, pcen, params, DEV)
        if log1p:
            m.log_compression()
        if full:
            m.full_transforms()
        for p in m.parameters():
            p.requires_grad_(True)
        xd = x.to(DEV).requires_grad_(need_dx)
        m(xd).backward(go.to(DEV))
        got = dict(m.named_parameters())
        for k in ref:
            assert got[k].grad.shape == ref[k].shape, k
            check(k, got[k].grad, ref[k], "saved " + ctx, floor)
        if need_dx:
            check("x", xd.grad, ref_dx, "saved " + ctx, floor, entrywise=False)
    grads = _native.leaf_backward(x.to(DEV), *native_args(params, pcen), K, hop, go.to(DEV), pcen=pcen, log1p=log1p, need_dx=need_dx,
                                  full_transforms=full, **(forced or {}))
    for name, gs in zip(NAMES, grads[:7]):
        if gs is not None:
            check(name, gs, ref[name], "recompute " + ctx, floor)
    if need_dx:
        check("x", grads[7].reshape(x.shape), ref_dx, "recompute " + ctx, floor, entrywise=False)
    return grads, dict(ref, x=ref_dx), floor


def ws_bytes(B, T, F, K, hop, flags=0, need_dx=False):
    from leaf_pytorch_amd import _native
    return _native.load().leaf_backward_workspace_bytes(B, T, F, K, hop, flags, int(need_dx))


def assert_not_the_staged_workspace(B, T, F, K, hop, need_dx=False, flags=0):
    """The workspace query sizes the path that serves the call: a fused backward asks for its own layout, not the staged one's
    (B, 2F, T) intermediates (at these small shapes the staged layout is the smaller one: the fused paths carry their tables)."""
    from leaf_pytorch_amd import _native
    fused = ws_bytes(B, T, F, K, hop, flags, need_dx)
    assert fused > 0 and fused != ws_bytes(B, T, F, K, hop, (flags & ~_native.FLAG_BWD_MFMA) | _native.FLAG_BWD_STAGED, need_dx), (B, T, F, K, hop, need_dx)


# ---------------------------------------------------------------------------------------------------------------------------
# A. PCEN backward rows across the scan seams and beyond the register path
# ---------------------------------------------------------------------------------------------------------------------------
SCAN_FRAMES = [1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 640, 641, 1000]
SCAN_EXTRA_FRAMES = [129, 513, 1000]
# smoother weights clamped at 0 (below it, and on it), clamped at 1 (above it, and on it) and at 0.04; deltas from 1e-4 to 2
OVER3 = {"_compression.ema._weights": torch.tensor([-0.25, 1.5, 0.04]), "_compression.delta": torch.tensor([1e-4, 2.0, 0.7])}
OVER8 = {"_compression.ema._weights": torch.tensor([-0.25, 1.5, 0.04, 0.0, 1.0, 0.3, 0.04, 0.9]),
         "_compression.delta": torch.tensor([1e-4, 2.0, 0.5, 1.0, 1e-4, 2.0, 0.1, 1.5])}
# the last frame over one sample (T = 160 (TP - 1) + 1), and seen full (T = 160 TP) on both sides of the register path
SCAN_OS = [(tp, 160 * (tp - 1) + 1) for tp in SCAN_FRAMES] + [(128, 160 * 128), (513, 160 * 513)]


@pytest.mark.parametrize("TP,T", SCAN_OS, ids=[f"TP{tp}-T{t}" for tp, t in SCAN_OS])
def test_pcen_scan_rows_through_the_overlap_save_backward(TP, T):
    assert (T - 1) // 160 + 1 == TP
    assert_not_the_staged_workspace(2, T, 3, 401, 160)
    edge_case("A-scan-overlap-save", 3, 401, 160, T, 2, True, seed=1001, over=OVER3,
              served=f"the overlap-save backward ({2 * -(-T // 1600)} blocks, {min_blocks(6)} from 6/16 per CU)")


@pytest.mark.parametrize("TP", SCAN_FRAMES)
def test_pcen_scan_rows_through_the_forced_mfma_backward(TP):
    """The same kernel's column-major copy (`gcols / col_of`) for the MFMA backward; the workspace is the MFMA plan's, not the staged one's."""
    from leaf_pytorch_amd import _native
    T = 50 * TP
    assert_not_the_staged_workspace(1, T, 8, 31, 50, flags=_native.FLAG_PCEN | _native.FLAG_BWD_MFMA)
    edge_case("A-scan-mfma", 8, 31, 50, T, 1, True, seed=1002, over=OVER8, forced={"mfma": True}, served="mfma=True")


@pytest.mark.parametrize("variant", ["off", "log1p", "dx"])
@pytest.mark.parametrize("TP", SCAN_EXTRA_FRAMES)
def test_pcen_scan_rows_other_modes(TP, variant):
    """PCEN off, log1p compression (the kernel's first branch: one lane strides the row) and dL/dx on the rows beyond a chunk, beyond
    the register path and at the 10 s row."""
    T = 160 * (TP - 1) + 1
    edge_case("A-scan-" + variant, 3, 401, 160, T, 2, variant == "dx", seed=1003, over=OVER3, need_dx=variant == "dx",
              log1p=variant == "log1p", served="the overlap-save backward")


@pytest.mark.parametrize("TP", SCAN_EXTRA_FRAMES)
def test_pcen_scan_rows_bf16_grad_out(TP):
    """A bfloat16 grad_out through the bfloat16 waveform call: the bits of the fp32 call on the widened tensors (as bf16_case,
    tests/test_gpu_train_extensions.py), and that fp32 call against the oracle."""
    from leaf_pytorch_amd import _native
    T = 160 * (TP - 1) + 1
    geo, params, x, go = draw(3, 401, 160, T, 2, True, 1004, over=OVER3)
    xb, gb = x.to(torch.bfloat16).to(DEV), go.to(torch.bfloat16).to(DEV)
    a = native_args(params, True)
    ctx = f"(family=A-scan-bf16 T={T} B=2 F=3 K=401 hop=160 pcen=True)"
    print(f"A-scan-bf16: T={T} frames={TP} served by the overlap-save backward, bfloat16 I/O")
    for need_dx in (False, True):
        r_b = _native.leaf_backward(xb, *a, 401, 160, gb, pcen=True, need_dx=need_dx)
        r_f = _native.leaf_backward(xb.float(), *a, 401, 160, gb.float(), pcen=True, need_dx=need_dx)
        for i in range(7):
            assert r_b[i].dtype == torch.float32 and torch.equal(r_b[i], r_f[i]), (NAMES[i], need_dx, ctx)
        if need_dx:
            assert torch.equal(r_b[7], r_f[7].to(torch.bfloat16)), ctx
        ref, ref_dx = oracle_grads(xb.float().cpu(), params, geo, True, gb.float().cpu(), need_dx)
        for name, g in zip(NAMES, r_f[:7]):
            assert_grad_close(name, g, ref[name], f"widened dx={need_dx} " + ctx)
        if need_dx:
            assert_grad_close("x", r_f[7].reshape(x.shape), ref_dx, "widened " + ctx, entrywise=False)


# ---------------------------------------------------------------------------------------------------------------------------
# B. every backward family on its clip-length lattice
# ---------------------------------------------------------------------------------------------------------------------------
def lattice_params(K, hop, L, extra=()):
    """(T, pcen): PCEN alternates over the sorted lattice."""
    ts = sorted(set(lattice(K, hop, L)) | set(extra))
    return [pytest.param(t, i % 2 == 0, id=f"T{t}-{'pcen' if i % 2 == 0 else 'off'}") for i, t in enumerate(ts)]


def test_lattice_restates_the_plans_block_lengths():
    """L is restated per family below; the plan's own figure where the library reports it (the 2048-sample plans)."""
    from leaf_pytorch_amd import _native
    for K, hop, L in ((401, 160, 1600), (201, 80, 1600), (801, 320, 960), (552, 220, 1472), (601, 240, 1408)):
        assert _native.fft_plan_info(4, 8 * 4096, 8, K, hop)["block_len"] == L, (K, hop)
    assert all(L == (2048 - K + 1) // 64 * 64 for K, _, L in RUNTIME_2048)
    assert (4096 - 1201 + 1) & ~1 == 2896 and (4096 - 833 + 1) & ~1 == 3264


# ---- 1. per-wave static backward: 401 / 160 below 6/16 of a block per CU
@pytest.mark.parametrize("T,pcen", lattice_params(401, 160, 1600))
def test_per_wave_static_16k(T, pcen):
    F, B, nblk = 5, 2, -(-T // 1600)
    assert B * nblk < min_blocks(6)
    if T == 1601:
        assert_not_the_staged_workspace(B, T, F, 401, 160)
    edge_case("1-per-wave-16k", F, 401, 160, T, B, pcen, seed=2001, served=f"{B * nblk} blocks, below 6/16 per CU = {min_blocks(6)}")


# ---- 2. static 16 kHz workgroup backward with band tasks; the same clips on full transforms
def default_every_fourth():
    return lo.default_params(lo.geometry())["_complex_conv._kernel"][::4].clone()          # 10 of the default 40, narrow-band members kept


BAND_LPHI_16 = 12 * (128 // 16)        # leaf_band.hpp: band_lphi(16) = kBandLh * band_d(16)
# band_edges(): frames reg_lo .. reg_hi take the shift-invariant window, reg_lo = ceil((padL + lphi) / hop),
# reg_hi = (T - K - lphi + padL) / hop; the first T with reg_hi >= reg_lo has one regular frame, one sample less has edge frames only
FIRST_REGULAR_T = -(-(200 + BAND_LPHI_16) // 160) * 160 + 401 + BAND_LPHI_16 - 200


@pytest.mark.parametrize("T,pcen", lattice_params(401, 160, 1600, extra=(FIRST_REGULAR_T - 1, FIRST_REGULAR_T)))
def test_workgroup_static_16k_band_tasks_and_full_transforms(T, pcen):
    from leaf_pytorch_amd import _native
    assert FIRST_REGULAR_T == 617
    F, nblk = 10, -(-T // 1600)
    B = clips_above(20, nblk)                            # past 20/16 (full transforms), hence past 6/16 (band tasks) with the same clips
    assert B * nblk > min_blocks(20) >= min_blocks(6)
    kernel = default_every_fourth()
    if T == 1601:
        assert_not_the_staged_workspace(B, T, F, 401, 160)
    band, ref, floor = edge_case("2-workgroup-16k-band", F, 401, 160, T, B, pcen, seed=2002, kernel=kernel,
                                 served=f"{B * nblk} blocks, above 6/16 per CU = {min_blocks(6)}")
    full, _, _ = edge_case("2-workgroup-16k-full", F, 401, 160, T, B, pcen, seed=2002, kernel=kernel, full=True,
                           served=f"full_transforms=True, {B * nblk} blocks, above 20/16 per CU = {min_blocks(20)}")
    _, params, _, _ = draw(F, 401, 160, 1, 1, pcen, 2002, kernel)                     # (the parameters do not depend on the clips)
    cls = _native.band_classes(params["_complex_conv._kernel"].to(DEV), params["_pooling.weights"].reshape(-1).to(DEV), 401, 160,
                               params["_pooling._bias"].to(DEV)).cpu().tolist()
    assert any(c != 2048 for c in cls), cls
    for name, gb, gf in zip(NAMES, band[:7], full[:7]):
        if gb is not None:
            vs_full(name, gb, gf, ref[name], 3e-5, (T, B, pcen), floor)


# ---- 3. the same with dL/dx: band tasks add into the block's G from the first block on; block per wave with full transforms
@pytest.mark.parametrize("route", ["band-2-clips", "band-above-6/16", "full-block-per-wave"])
@pytest.mark.parametrize("T,pcen", lattice_params(401, 160, 1600))
def test_static_16k_with_input_gradient(T, pcen, route):
    F, nblk = 10, -(-T // 1600)
    full = route == "full-block-per-wave"
    B = clips_above(6, nblk) if route == "band-above-6/16" else 2
    if route == "band-above-6/16":
        assert B * nblk > min_blocks(6)
        served = f"{B * nblk} blocks, above 6/16 per CU = {min_blocks(6)} (threshold with dL/dx: 0)"
    elif full:
        assert B * nblk < min_blocks(20)
        served = f"full_transforms=True, {B * nblk} blocks, below 20/16 per CU = {min_blocks(20)}"
    else:
        served = f"{B * nblk} blocks (threshold with dL/dx: 0)"
    if T == 1601:
        assert_not_the_staged_workspace(B, T, F, 401, 160, need_dx=True)
    edge_case("3-static-16k-dx-" + route, F, 401, 160, T, B, pcen, seed=2003, need_dx=True, kernel=default_every_fourth(), full=full,
              served=served)


# ---- 4. static 8 kHz
@pytest.mark.parametrize("need_dx", [False, True], ids=["params", "dx"])
@pytest.mark.parametrize("T,pcen", lattice_params(201, 80, 1600))
def test_workgroup_static_8k(T, pcen, need_dx):
    F, nblk = 5, -(-T // 1600)
    B = clips_above(20, nblk)
    assert B * nblk > min_blocks(20)
    if T == 1601:
        assert_not_the_staged_workspace(B, T, F, 201, 80, need_dx)
    edge_case("4-workgroup-8k" + ("-dx" if need_dx else ""), F, 201, 80, T, B, pcen, seed=2004, need_dx=need_dx,
              served=f"{B * nblk} blocks, above 20/16 per CU = {min_blocks(20)}")


# ---- 5. static 32 kHz on 4096-sample blocks, and below its threshold on 2048-sample blocks (whose plan cuts blocks of 960 = 3 hops:
# leaf_fft.hpp, fft_block_len; its L - 1, L, L + 1, 2L, 2L + 1 join the lattice)
def plan4k_static_bytes(B, T, F, need_dx):
    """The workspace of the static 801 / 320 backward on 4096-sample blocks (tests/test_gpu_backward.py, restated)."""
    up = lambda n: -(-n // 64) * 64
    TP, nblk = (T - 1) // 320 + 1, -(-T // 3200)
    return 4 * (up(3 * F * 12288) + up(F * 2 * 528 + 4096) + up(B * TP * 2 * F) + 3 * up(B * F * TP) + up(B * F * 4) + up(B * F) +
                up(B * nblk * F * 2) + up(B * nblk * F) + up(F) + (up(B * nblk * 4096) if need_dx else 0) +
                up(4 * F) + 2 * up(F * 144) + 2 * up(F * 12 * 512) + up(48))


@pytest.mark.parametrize("route", ["4096-blocks", "4096-blocks-dx", "2-clips", "2-clips-dx"])
@pytest.mark.parametrize("T,pcen", lattice_params(801, 320, 3200, extra=(959, 960, 961, 1920, 1921)))
def test_static_32k(T, pcen, route):
    F, nblk = 4, -(-T // 3200)
    need_dx = route.endswith("-dx")
    if route.startswith("4096"):
        B = clips_above(8, nblk)
        assert B * nblk > min_blocks(8)
        served = f"{B * nblk} blocks of 3200, above 8/16 per CU = {min_blocks(8)}"
        if T == 3201:
            assert ws_bytes(B, T, F, 801, 320, 0, need_dx) == plan4k_static_bytes(B, T, F, need_dx)
    else:
        B = 2
        assert B * nblk < min_blocks(8)
        served = f"{B * nblk} blocks of 3200, below 8/16 per CU = {min_blocks(8)}"
        if T == 3201:
            assert ws_bytes(B, T, F, 801, 320, 0, need_dx) != plan4k_static_bytes(B, T, F, need_dx)
            assert_not_the_staged_workspace(B, T, F, 801, 320, need_dx)
    edge_case("5-static-32k-" + route, F, 801, 320, T, B, pcen, seed=2005, need_dx=need_dx, served=served)


# ---- 6. run-time geometry on 2048-sample blocks: an even and an odd window
# (the plan rounds 2048 - K + 1 down to whole 64-sample rows -- leaf_fft.hpp, fft_block_len -- so L = 1472 / 1408; the unrounded
# 2048 - K + 1 = 1497 / 1448 and its neighbours stay in the lattice as ragged second blocks)
RUNTIME_2048 = [(552, 220, (2048 - 552 + 1) // 64 * 64), (601, 240, (2048 - 601 + 1) // 64 * 64)]
RUNTIME_2048_CASES = [pytest.param(K, hop, L, *p.values, id=f"K{K}-{p.id}") for K, hop, L in RUNTIME_2048
                      for p in lattice_params(K, hop, L, extra=(2048 - K, 2048 - K + 1, 2048 - K + 2, 2 * (2048 - K + 1), 2 * (2048 - K + 1) + 1))]


@pytest.mark.parametrize("route", ["workgroup", "workgroup-dx", "2-clips", "2-clips-dx"])
@pytest.mark.parametrize("K,hop,L,T,pcen", RUNTIME_2048_CASES)
def test_runtime_geometry_2048(K, hop, L, T, pcen, route):
    F, nblk = 4, -(-T // L)
    need_dx = route.endswith("-dx")
    if route.startswith("workgroup"):
        B = clips_above(10, nblk)
        assert B * nblk > min_blocks(10)
        served = f"{B * nblk} blocks of {L}, above 10/16 per CU = {min_blocks(10)}"
    else:
        B = 2
        assert B * nblk < min_blocks(10)
        served = f"{B * nblk} blocks of {L}, below 10/16 per CU = {min_blocks(10)}"
    if T == L + 1:
        assert_not_the_staged_workspace(B, T, F, K, hop, need_dx)
    edge_case(f"6-runtime-2048-K{K}-" + route, F, K, hop, T, B, pcen, seed=2006 + K, need_dx=need_dx, served=served)


# ---- 7. run-time geometry on 4096-sample blocks
RUNTIME_4096 = [(1201, 480, (4096 - 1201 + 1) & ~1), (833, 333, (4096 - 833 + 1) & ~1)]
RUNTIME_4096_CASES = [pytest.param(K, hop, L, *p.values, id=f"K{K}-{p.id}") for K, hop, L in RUNTIME_4096 for p in lattice_params(K, hop, L)]


@pytest.mark.parametrize("K,hop,L,T,pcen", RUNTIME_4096_CASES)
def test_runtime_geometry_4096(K, hop, L, T, pcen):
    F, nblk = 3, -(-T // L)
    B = clips_above(8, nblk)
    assert B * nblk > min_blocks(8)
    if T == L + 1:
        assert_not_the_staged_workspace(B, T, F, K, hop)
    edge_case(f"7-runtime-4096-K{K}", F, K, hop, T, B, pcen, seed=2007 + K,
              served=f"{B * nblk} blocks of {L}, above 8/16 per CU = {min_blocks(8)}")


# ---- 8. MFMA and staged, forced (no block length of their own: the 2048-sample plan's 2048 - K + 1 places the long clips)
@pytest.mark.parametrize("route", ["mfma", "staged-dx"])
@pytest.mark.parametrize("T,pcen", lattice_params(31, 50, 2048 - 31 + 1))
def test_forced_mfma_and_staged(T, pcen, route):
    from leaf_pytorch_amd import _native
    F, B = 8, 2
    fl = _native.FLAG_PCEN if pcen else 0
    if T == 2048 - 31 + 2:
        assert_not_the_staged_workspace(B, T, F, 31, 50, flags=fl | _native.FLAG_BWD_MFMA)
    if route == "mfma":
        edge_case("8-forced-mfma", F, 31, 50, T, B, pcen, seed=2008, forced={"mfma": True}, served="mfma=True")
    else:
        edge_case("8-forced-staged-dx", F, 31, 50, T, B, pcen, seed=2008, need_dx=True, forced={"staged": True}, served="staged=True")
