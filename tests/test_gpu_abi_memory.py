"""The C ABI's memory contract, raw through ctypes: which bytes a call touches.

Every buffer handed to the library here comes from tests/guarded.py: exactly the size the header asks for (the workspace: exactly
what the size query answers), a 4096-byte guard pattern on both sides, read-only inputs compared with a copy taken before the call.
Each case runs three times --

  1. CLEAN     workspace zero-filled, outputs pre-filled with 0xFF bytes (a NaN as float32 / bfloat16): rc 0, guards intact, no
               0xFF word left in an output (every element was written), values against the fp64 oracle;
  2. POISONED  the same call with the workspace filled with 0xFF: bit-identical outputs (nothing is read before the call wrote it);
  3. STALE     another case of the same family (one clip more, longer clips, other data) runs on the same workspace memory, then
               this case again without clearing: bit-identical outputs (nothing a previous call left is taken for this call's);

-- and once with `workspace_bytes` one word short: LEAF_ERR_WORKSPACE, nothing touched.  The alignment cases put every buffer the
kernels reach with one-element accesses at the minimum include/leaf_hip.h promises (4 bytes past a 4096-byte boundary; 2 for
bfloat16 / int16 buffers) and ask for the bits of the aligned call; `workspace` and `tables` need 16 bytes and are refused below
that without a launch (tests/test_host_abi_alignment.py, no GPU).  The only wait on global memory in the library is the seam ticket
of the split small-batch kernel (leaf_fft_small.hpp): the first half of the same launch stores the 64-bit per-launch ticket the second
half polls for, so a poisoned or stale slot is never taken for it."""
import ctypes
import math

import pytest
import torch

from conftest import rel_err
from guarded import guarded, guarded_tensor, unchanged
from helpers import assert_grad_close
from oracle import leaf_oracle as lo
from leaf_pytorch_amd import _native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REL_TOL = 2e-5                                  # tests/test_gpu_parity.py: the float path's bound against the oracle
BF16_TOL = 2 ** -8                              # test_bf16_io_extension_matches_fp32_path_within_bf16_rounding
GRAD_TOL = 1e-4                                 # tests/test_gpu_backward.py
N = _native
SEL = {N.ALGO_AUTO: "auto", N.ALGO_STAGED: "staged", N.ALGO_MFMA: "mfma", N.ALGO_FFT: "fft", N.ALGO_FFT_WG: "fft_wg",
       N.ALGO_FFT_SMALL: "fft_small"}
PARAM_KEYS = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
              "_compression.root", "_compression.ema._weights"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    N.load()


def n_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def sync():
    torch.cuda.synchronize()


# ---- cases ---------------------------------------------------------------------------------------------------------------------
class Fwd:
    """One forward case: geometry, selector (+ option bits), flags, shape, entry point."""

    def __init__(self, name, K, hop, F, B, T, algo, flags=N.FLAG_PCEN, entry="forward", init="random", reserve_leave=0, loud=False,
                 seed=0):
        self.name, self.K, self.hop, self.F, self.B, self.T = name, K, hop, F, B, T
        self.algo, self.flags, self.entry, self.init, self.reserve_leave, self.loud, self.seed = algo, flags, entry, init, reserve_leave, loud, seed

    @property
    def pcen(self):
        return bool(self.flags & N.FLAG_PCEN)

    @property
    def xdtype(self):
        return torch.bfloat16 if self.flags & N.FLAG_IO_BF16 else torch.int16 if self.flags & N.FLAG_X_PCM16 else torch.float32

    @property
    def odtype(self):
        return torch.bfloat16 if self.flags & N.FLAG_IO_BF16 else torch.float32

    def algo_bits(self):
        return self.algo | (N.algo_reserve_cus(n_cus() - self.reserve_leave) if self.reserve_leave else 0)

    def pair(self):
        return (self.K, self.hop, SEL[self.algo & 0xff])

    def other(self):
        """The case whose leftovers the STALE call runs on: the same family, one clip more, longer clips, other data."""
        return Fwd(self.name + "/other", self.K, self.hop, self.F, self.B + 1, self.T + 1603, self.algo, self.flags, self.entry,
                   self.init, self.reserve_leave, self.loud, self.seed + 1000)


PC, OFF, LOG, BF, PCM, PEAK = N.FLAG_PCEN, 0, N.FLAG_LOG1P, N.FLAG_IO_BF16, N.FLAG_X_PCM16, N.FLAG_PEAKNORM
WG, FFT, SMALL, MFMA, STAGED, AUTO = N.ALGO_FFT_WG, N.ALGO_FFT, N.ALGO_FFT_SMALL, N.ALGO_MFMA, N.ALGO_STAGED, N.ALGO_AUTO
FULL, SFIN = N.ALGO_FULL_TRANSFORMS, N.ALGO_STREAM_FINALIZE

FORWARD_CASES = [
    # one-launch small-batch kernel: one block; two workgroups per (clip, filter) with the seam pairs; two rounds of workgroups
    *[Fwd(f"small-{K}-B{B}", K, hop, 40, B, T, SMALL, init="default" if K == 401 else "random", seed=B)
      for K, hop in ((401, 160), (201, 80)) for B, T in ((1, 1601), (2, 4801), (7, 1600))],
    # per-wave overlap-save kernel
    Fwd("fft-401", 401, 160, 7, 2, 4801, FFT), Fwd("fft-401-one-sample", 401, 160, 7, 1, 1, FFT),
    Fwd("fft-552-even", 552, 220, 7, 2, 3000, FFT), Fwd("fft-1217-three-slots", 1217, 300, 7, 2, 2500, FFT),
    # workgroup kernel, static 16 kHz instance at the default initialisation (band tasks)
    Fwd("wg-401", 401, 160, 40, 3, 4801, WG, init="default"), Fwd("wg-401-full", 401, 160, 40, 3, 4801, WG | FULL, init="default"),
    Fwd("wg-401-straddle", 401, 160, 40, 5, 3300, WG, init="default", reserve_leave=2),
    Fwd("wg-401-stream", 401, 160, 40, 3, 4801, WG | SFIN, init="default"),
    Fwd("wg-401-peaknorm", 401, 160, 40, 3, 4801, WG, PC | PEAK, init="default", loud=True),
    Fwd("wg-401-pcen-off", 401, 160, 40, 3, 4801, WG, OFF, init="default"),
    Fwd("wg-401-log1p", 401, 160, 40, 3, 4801, WG, LOG, init="default"),
    Fwd("wg-401-bf16", 401, 160, 40, 3, 4801, WG, PC | BF, init="default"),
    Fwd("wg-401-pcm16", 401, 160, 40, 3, 4801, WG, PC | PCM, init="default"),
    Fwd("wg-201", 201, 80, 12, 3, 4801, WG),
    # 4096-sample static instance
    Fwd("wg4k-801", 801, 320, 12, 2, 3201, WG), Fwd("wg4k-801-ragged", 801, 320, 12, 3, 7000, WG),
    Fwd("wg4k-801-f80", 801, 320, 80, 2, 3201, WG, init="default"),
    # run-time geometry, 2048- and 4096-sample plans
    Fwd("wgg-552", 552, 220, 7, 2, 5000, WG), Fwd("wgg-300", 300, 75, 7, 2, 5000, WG),
    Fwd("wgg4k-833", 833, 333, 6, 2, 5000, WG), Fwd("wgg4k-2049", 2049, 800, 6, 2, 5000, WG),
    # MFMA (K < hop), staged.  (64 taps at hop 7: leaf_workspace_bytes(..., LEAF_ALGO_MFMA) answers 0 -- no MFMA plan at a hop
    # of 7 -- so the geometry runs under AUTO, which takes the staged kernels there.)
    Fwd("mfma-401", 401, 160, 17, 2, 2400, MFMA), Fwd("mfma-31", 31, 50, 17, 2, 400, MFMA), Fwd("auto-64-staged", 64, 7, 17, 2, 300, AUTO),
    Fwd("staged-101", 101, 40, 5, 2, 777, STAGED),
    # AUTO: the size it asks for is the size the kernel it picks uses
    Fwd("auto-B1", 401, 160, 40, 1, 4801, AUTO, init="default"), Fwd("auto-B3", 401, 160, 40, 3, 4801, AUTO, init="default"),
    # leaf_forward_save_f32: pooled_raw guarded and fully written
    Fwd("save-fft-401", 401, 160, 7, 2, 4801, FFT, entry="save"), Fwd("save-fft-1217", 1217, 300, 7, 2, 2500, FFT, entry="save"),
    Fwd("save-wg-401", 401, 160, 40, 3, 4801, WG, entry="save", init="default"),
    Fwd("save-wg-401-straddle", 401, 160, 40, 5, 3300, WG, entry="save", init="default", reserve_leave=2),
    Fwd("save-wg4k-801", 801, 320, 12, 2, 3201, WG, entry="save"),
    Fwd("save-mfma-401", 401, 160, 17, 2, 2400, MFMA, entry="save"), Fwd("save-mfma-31", 31, 50, 17, 2, 400, MFMA, entry="save"),
    Fwd("save-small-401", 401, 160, 40, 2, 4801, SMALL, entry="save", init="default"),
    # frozen-parameter tables
    Fwd("prepared-401", 401, 160, 40, 3, 4801, FFT, entry="prepared", init="default"),
]
# the (K, hop, selector) pairs the matrix must have run: a pair missing from a complete run of this file fails it
EXPECTED_PAIRS = {
    (401, 160, "fft_small"), (201, 80, "fft_small"),
    (401, 160, "fft"), (552, 220, "fft"), (1217, 300, "fft"),
    (401, 160, "fft_wg"), (201, 80, "fft_wg"), (801, 320, "fft_wg"), (552, 220, "fft_wg"), (300, 75, "fft_wg"), (833, 333, "fft_wg"),
    (2049, 800, "fft_wg"),
    (401, 160, "mfma"), (31, 50, "mfma"), (64, 7, "auto"),
    (101, 40, "staged"),
    (401, 160, "auto"),
}
RAN = set()


def make_params(F, K, hop, pcen, init, seed):
    gen = torch.Generator().manual_seed(1000 + seed)
    geo = lo.LeafGeometry(F, 0, K, hop, *lo.same_padding(K))
    if init == "default":                                   # the mel initialisation at the sample rate of the geometry
        rate = {401: 16000, 801: 32000}[K]
        return lo.default_params(lo.LeafGeometry(F, rate, K, hop, *lo.same_padding(K)), pcen), geo
    kernel = torch.stack([0.1 + torch.rand(F, generator=gen) * (math.pi - 0.2), 3.0 + torch.rand(F, generator=gen) * K / 4], dim=1)
    params = lo.default_params(geo, pcen, kernel=kernel)
    return {k: v * (1 + 0.1 * (2 * torch.rand(v.shape, generator=gen) - 1)) for k, v in params.items()}, geo


def make_x(c):
    gen = torch.Generator().manual_seed(c.seed)
    if c.xdtype == torch.int16:
        return torch.randint(-32768, 32768, (c.B, c.T), generator=gen, dtype=torch.int32).to(torch.int16)
    x = 2 * torch.rand(c.B, c.T, generator=gen) - 1
    if c.loud:
        x[0] *= 3.0                                         # one loud clip: its scale in the workspace's tail is not 1
    return x.to(c.xdtype)


def oracle_forward(c, x, params, geo):
    x64 = x.double() / 32768 if x.dtype == torch.int16 else x.double()
    x64 = x64[:, None, :]
    if c.flags & PEAK and x.dtype != torch.int16:
        x64 = lo.peak_normalize(x64)
    ref = lo.leaf_forward(x64, {k: v.double() for k, v in params.items()}, geo, c.pcen, torch.float64)
    if c.flags & LOG and not c.pcen:
        ref = torch.log1p(ref)
    return ref.float()


def param_buffers(params, pcen, off=0):
    keys = PARAM_KEYS if pcen else PARAM_KEYS[:3]
    bufs = [guarded_tensor(params[k].float(), off) for k in keys]
    return bufs, [b.ptr for b in bufs] + [None] * (7 - len(bufs))


def forward_need(lib, c):
    if c.entry == "prepared":                               # sized by leaf_workspace_bytes(..., LEAF_ALGO_FFT)
        return lib.leaf_workspace_bytes(c.B, c.T, c.F, c.K, c.hop, N.ALGO_FFT)
    return lib.leaf_workspace_bytes(c.B, c.T, c.F, c.K, c.hop, c.algo_bits())


def forward_call(lib, c, x, params, ws, ws_bytes, off=0, tables=None):
    """One call: fresh guarded buffers around everything but the workspace.  Returns rc and the outputs' bytes."""
    TP = lib.leaf_num_frames(c.T, c.K, c.hop)
    small = 2 if x.element_size() == 2 else 4
    xg = guarded_tensor(x, min(off, small) if off else 0)
    pb, pp = param_buffers(params, c.pcen, off)
    osz = 2 if c.odtype == torch.bfloat16 else 4
    out = guarded(c.B * c.F * TP * osz, 0xFF, min(off, osz) if off else 0)
    raw = guarded(c.B * c.F * TP * 4, 0xFF, off) if c.entry == "save" else None
    common = (c.F, c.K, c.hop, c.flags)
    if c.entry == "prepared":
        rc = lib.leaf_forward_prepared_f32(xg.ptr, c.B, c.T, tables.ptr, tables.nbytes, *pp[2:], *common, out.ptr, ws.ptr, ws_bytes, None)
    elif c.entry == "save":
        rc = lib.leaf_forward_save_f32(xg.ptr, c.B, c.T, *pp, *common, c.algo_bits(), out.ptr, raw.ptr, ws.ptr, ws_bytes, None)
    else:
        rc = lib.leaf_forward_f32(xg.ptr, c.B, c.T, *pp, *common, c.algo_bits(), out.ptr, ws.ptr, ws_bytes, None)
    sync()
    what = f"{c.name} (off={off})"
    unchanged(xg, what + " x")
    for b in pb:
        unchanged(b, what + " parameter")
    out.check(what + " out")
    ws.check(what + " workspace")
    if raw is not None:
        raw.check(what + " pooled_raw")
    if tables is not None:
        unchanged(tables, what + " tables")
    return rc, out.cpu(torch.int16 if osz == 2 else torch.int32, (c.B, c.F, TP)), (raw.cpu(torch.int32, (c.B, c.F, TP)) if raw else None)


def prepare_tables(lib, c, params, fill):
    tb = lib.leaf_fft_tables_bytes(c.F, c.K, c.hop)
    assert tb > 0
    t = guarded(tb, fill)
    pb, pp = param_buffers(params, False)
    assert lib.leaf_fft_prepare_tables_f32(pp[0], pp[1], c.F, c.K, c.hop, t.ptr, tb, None) == 0
    sync()
    t.check(c.name + " tables (prepare)")
    for b in pb:
        unchanged(b, c.name + " parameter (prepare)")
    t.before = t.bytes().clone()
    return t


def as_values(bits, dtype):
    return bits.view(dtype).float() if dtype == torch.bfloat16 else bits.view(torch.float32)


def three_calls(lib, c, off=0):
    """CLEAN / POISONED / STALE on one workspace allocation; returns the clean call's output bits (out, pooled_raw)."""
    params, geo = make_params(c.F, c.K, c.hop, c.pcen, c.init, c.seed)
    x = make_x(c)
    need = forward_need(lib, c)
    assert need > 0, f"{c.name}: the size query answers 0 (no kernel for this selector and geometry)"
    o = c.other()
    o_need = forward_need(lib, o)
    assert o_need > 0, o.name
    ws = guarded(need, 0x00, capacity=max(need, o_need))
    tables = prepare_tables(lib, c, params, 0x00) if c.entry == "prepared" else None
    # 1. clean
    rc, out1, raw1 = forward_call(lib, c, x, params, ws, need, off, tables)
    assert rc == 0, f"{c.name}: {N.load().leaf_status_string(rc)}"
    assert not bool((out1 == -1).any()), f"{c.name}: {int((out1 == -1).sum())} elements of out were never written"
    if raw1 is not None:
        assert not bool((raw1 == -1).any()), f"{c.name}: {int((raw1 == -1).sum())} elements of pooled_raw were never written"
    # 2. poisoned (the frozen-parameter tables too: prepared into a 0xFF-filled buffer)
    ws.fill(0xFF)
    tables2 = prepare_tables(lib, c, params, 0xFF) if c.entry == "prepared" else None
    rc, out2, raw2 = forward_call(lib, c, x, params, ws, need, off, tables2)
    assert rc == 0 and torch.equal(out2, out1), f"{c.name}: the output depends on what the workspace held before the call (0xFF fill)"
    assert raw1 is None or torch.equal(raw2, raw1), f"{c.name}: pooled_raw depends on the workspace's previous contents"
    # 3. stale: another case of the family on the same memory, then this one without clearing
    po, _ = make_params(o.F, o.K, o.hop, o.pcen, o.init, o.seed)
    ws.relayout(o_need)
    ot = prepare_tables(lib, o, po, 0x00) if o.entry == "prepared" else None
    rc, _, _ = forward_call(lib, o, make_x(o), po, ws, o_need, 0, ot)
    assert rc == 0, o.name
    ws.relayout(need)
    rc, out3, raw3 = forward_call(lib, c, x, params, ws, need, off, tables)
    assert rc == 0 and torch.equal(out3, out1), f"{c.name}: the output depends on what another call left in the workspace"
    assert raw1 is None or torch.equal(raw3, raw1), f"{c.name}: pooled_raw depends on what another call left in the workspace"
    return (c, x, params, geo, need), out1, raw1


@pytest.mark.parametrize("c", FORWARD_CASES, ids=[c.name for c in FORWARD_CASES])
def test_forward_touches_only_its_buffers_and_reads_nothing_stale(c):
    lib = N.load()
    (c, x, params, geo, need), out1, raw1 = three_calls(lib, c)
    if (c.algo & 0xff) == AUTO:
        picked = lib.leaf_auto_algo(c.B, c.T, c.F, c.K, c.hop)
        assert need == lib.leaf_workspace_bytes(c.B, c.T, c.F, c.K, c.hop, picked), "AUTO asks for another size than the kernel it picks"
    ref = oracle_forward(c, x, params, geo)
    got = as_values(out1, c.odtype)
    tol = BF16_TOL if c.odtype == torch.bfloat16 else REL_TOL
    err = rel_err(got, ref)
    print(f"{c.name}: workspace {need} bytes, rel err {err:.3e} (bound {tol:.1e})")
    assert err < tol, f"{c.name}: rel err {err:.3e}"
    if raw1 is not None:
        # pooled_raw = bias + pooled energy before the 1e-5 floor: the oracle's pooled stage wherever that is above the floor
        x64 = (x.double() / 32768 if x.dtype == torch.int16 else x.double())[:, None, :]
        _, st = lo.leaf_forward(x64, {k: v.double() for k, v in params.items()}, geo, c.pcen, torch.float64, True)
        pooled = st["pooled"].float()
        rawv = raw1.view(torch.float32)
        assert rel_err(rawv.clamp_min(1e-5), pooled) < REL_TOL, f"{c.name}: pooled_raw rel err {rel_err(rawv.clamp_min(1e-5), pooled):.3e}"
    # one word short: refused, nothing touched
    ws = guarded(need - 4, 0x5A)
    tables = prepare_tables(lib, c, params, 0x00) if c.entry == "prepared" else None
    rc, out, raw = forward_call(lib, c, x, params, ws, need - 4, 0, tables)
    if c.entry == "prepared":
        # INTEGRATION.md (ABI 3): a workspace below the documented size still works down to the partial sums -- the call then has no
        # room for the edge tables of the band tasks and runs full transforms (~1e-6 from the band result): inside its guards
        assert rc == 0 and not bool((out == -1).any()) and rel_err(as_values(out, c.odtype), ref) < REL_TOL
    else:
        assert rc == -3, f"{c.name}: workspace one word short answered {rc}"
        assert bool((out == -1).all()) and (raw is None or bool((raw == -1).all())) and bool((ws.bytes() == 0x5A).all())
    RAN.add(c.pair())


def test_every_expected_selector_ran(request):
    assert {c.pair() for c in FORWARD_CASES} == EXPECTED_PAIRS
    selected = {i.name for i in request.session.items}
    whole = all(f"test_forward_touches_only_its_buffers_and_reads_nothing_stale[{c.name}]" in selected for c in FORWARD_CASES)
    if whole:                                               # (a -k selection runs what it selects; the complete file owes every pair)
        assert RAN == EXPECTED_PAIRS, f"not run: {sorted(EXPECTED_PAIRS - RAN)}"


@pytest.mark.parametrize("F,K,hop,values", [(40, 401, 160, {256, 512, 2048}), (80, 801, 320, {512, 4096})], ids=["16k", "32k"])
def test_band_classes_workspace_is_the_documented_size(F, K, hop, values):
    lib = N.load()
    need = max(lib.leaf_fft_tables_bytes(F, K, hop), lib.leaf_workspace_bytes(1, 8192, F, K, hop, N.ALGO_FFT_WG))
    params, _ = make_params(F, K, hop, False, "default", 0)
    got = []
    for fill in (0x00, 0xFF):
        ws = guarded(need, fill)
        cls = guarded(F * 4, 0xFF)
        pb, pp = param_buffers(params, False)
        rc = lib.leaf_band_classes_f32(pp[0], pp[1], pp[2], F, K, hop, cls.ptr, ws.ptr, need, None)
        sync()
        assert rc == 0, rc
        ws.check("band_classes workspace")
        cls.check("classes")
        for b in pb:
            unchanged(b, "band_classes parameter")
        got.append(cls.cpu(torch.int32))
    assert set(got[0].tolist()) <= values, sorted(set(got[0].tolist()))
    assert torch.equal(got[0], got[1]), "the classes depend on what the workspace held before the call"


# ---- backward --------------------------------------------------------------------------------------------------------------------
class Bwd:
    def __init__(self, name, K, hop, F, B, T, flags=PC, dx=False, raw=True, seed=0, cu_sixteenths=0, block_len=0):
        self.name, self.K, self.hop, self.F, self.B, self.T, self.flags, self.dx, self.raw, self.seed = name, K, hop, F, B, T, flags, dx, raw, seed
        self.cu_sixteenths, self.block_len = cu_sixteenths, block_len

    pcen = Fwd.pcen
    xdtype = Fwd.xdtype

    @property
    def iodtype(self):
        return torch.bfloat16 if self.flags & BF else torch.float32

    def batch(self):
        if not self.cu_sixteenths:
            return self.B
        # past the dispatcher's threshold for the workgroup backward of the family, as tests/test_gpu_pcm16.py::WG_BWD_PATHS sizes it
        nblk = -(-self.T // self.block_len)
        need = -(-n_cus() * self.cu_sixteenths // 16)
        return -(-need // nblk) + 1

    def other(self):
        o = Bwd(self.name + "/other", self.K, self.hop, self.F, self.batch() + 1, self.T + 777, self.flags, self.dx, self.raw, self.seed + 1000)
        return o


BST, BMF, BFULL = N.FLAG_BWD_STAGED, N.FLAG_BWD_MFMA, N.FLAG_BWD_FULL_TRANSFORMS
BACKWARD_CASES = [
    # (401, 160) F = 40: few blocks (one wave per block) and more
    Bwd("b401", 401, 160, 40, 2, 2400), Bwd("b401-dx-recompute", 401, 160, 40, 2, 2400, dx=True, raw=False),
    Bwd("b401-log1p-dx", 401, 160, 40, 2, 2400, LOG, dx=True), Bwd("b401-T4801", 401, 160, 40, 3, 4801, raw=False),
    Bwd("b401-T4801-dx", 401, 160, 40, 3, 4801, dx=True), Bwd("b401-bf16-dx", 401, 160, 40, 2, 2400, PC | BF, dx=True),
    Bwd("b401-pcm16", 401, 160, 40, 2, 2400, PC | PCM, raw=False), Bwd("b401-staged-dx", 401, 160, 40, 2, 2400, PC | BST, dx=True),
    Bwd("b401-mfma", 401, 160, 40, 2, 2400, PC | BMF), Bwd("b401-full", 401, 160, 40, 3, 4801, PC | BFULL),
    Bwd("b401-full-dx", 401, 160, 40, 2, 2400, PC | BFULL, dx=True, raw=False),
    # (801, 320) F = 12
    Bwd("b801", 801, 320, 12, 2, 3201), Bwd("b801-dx-recompute", 801, 320, 12, 2, 3201, dx=True, raw=False),
    Bwd("b801-log1p-full", 801, 320, 12, 2, 3201, LOG | BFULL), Bwd("b801-bf16", 801, 320, 12, 2, 3201, PC | BF, dx=True),
    # (552, 220) F = 6: run-time geometry (16-bit input: the widened copy in the workspace)
    Bwd("b552", 552, 220, 6, 2, 3000), Bwd("b552-dx-recompute", 552, 220, 6, 2, 3000, dx=True, raw=False),
    Bwd("b552-log1p", 552, 220, 6, 2, 3000, LOG, raw=False), Bwd("b552-bf16", 552, 220, 6, 2, 3000, PC | BF),
    Bwd("b552-pcm16", 552, 220, 6, 2, 3000, PC | PCM),
    # (833, 333) F = 6: beyond the 2048-sample plan's dL/dx
    Bwd("b833", 833, 333, 6, 2, 5000), Bwd("b833-dx", 833, 333, 6, 2, 5000, dx=True, raw=False), Bwd("b833-pcm16-log1p", 833, 333, 6, 2, 5000, LOG | PCM),
    # (31, 50) F = 8: MFMA, staged
    Bwd("b31", 31, 50, 8, 2, 400), Bwd("b31-dx", 31, 50, 8, 2, 400, dx=True, raw=False), Bwd("b31-bf16-log1p", 31, 50, 8, 2, 400, LOG | BF),
    Bwd("b31-staged", 31, 50, 8, 2, 400, PC | BST, raw=False),
    # the workgroup-per-block backwards: the batch sized from the device's CU count
    Bwd("b401-workgroup", 401, 160, 12, 0, 7000, cu_sixteenths=6, block_len=2048 - 401 + 1),
    Bwd("b801-workgroup-4096", 801, 320, 12, 0, 7000, cu_sixteenths=8, block_len=3200),
]


def backward_data(c, B):
    gen = torch.Generator().manual_seed(c.seed + 7)
    params, geo = make_params(c.F, c.K, c.hop, c.pcen, "random", c.seed)
    if c.xdtype == torch.int16:
        x = torch.randint(-32768, 32768, (B, c.T), generator=gen, dtype=torch.int32).to(torch.int16)
    else:
        x = torch.randn(B, c.T, generator=gen).to(c.xdtype)
    TP = (c.T - 1) // c.hop + 1
    go = torch.randn(B, c.F, TP, generator=gen).to(c.iodtype)
    return params, geo, x, go


def backward_call(lib, c, B, x, params, go, raw_bits, ws, ws_bytes, off=0):
    small = 2 if x.element_size() == 2 else 4
    io = 2 if c.iodtype == torch.bfloat16 else 4
    xg = guarded_tensor(x, min(off, small) if off else 0)
    gog = guarded_tensor(go, min(off, io) if off else 0)
    rawg = guarded_tensor(raw_bits, off) if raw_bits is not None else None
    pb, pp = param_buffers(params, c.pcen, off)
    ng = 7 if c.pcen else 3
    grads = [guarded((2 if i == 0 else 1) * c.F * 4, 0xFF, off) for i in range(ng)]
    gx = guarded(B * c.T * io, 0xFF, min(off, io) if off else 0) if c.dx else None
    rc = lib.leaf_backward_f32(xg.ptr, B, c.T, *pp, c.F, c.K, c.hop, c.flags, gog.ptr, rawg.ptr if rawg else None,
                               *[g.ptr for g in grads], *([None] * (7 - ng)), gx.ptr if gx else None, ws.ptr, ws_bytes, None)
    sync()
    what = f"{c.name} (off={off})"
    for g, n in [(xg, "x"), (gog, "grad_out")] + ([(rawg, "pooled_raw")] if rawg else []) + [(b, "parameter") for b in pb]:
        unchanged(g, f"{what} {n}")
    for g in grads:
        g.check(what + " parameter gradient")
    ws.check(what + " workspace")
    if gx:
        gx.check(what + " g_x")
    return rc, [g.cpu(torch.int32) for g in grads], (gx.cpu(torch.int16 if io == 2 else torch.int32, (B, c.T)) if gx else None)


def saved_pooled(lib, c, B, x, params):
    """pooled_raw of leaf_forward_save_f32 for the same flags (guarded buffers, AUTO)."""
    f = Fwd(c.name + "/fwd", c.K, c.hop, c.F, B, c.T, AUTO, c.flags & (PC | LOG | BF | PCM), entry="save")
    need = lib.leaf_workspace_bytes(B, c.T, c.F, c.K, c.hop, AUTO)
    rc, _, raw = forward_call(lib, f, x, params, guarded(need, 0xFF), need)
    assert rc == 0, rc
    return raw


def backward_three_calls(lib, c, off=0):
    B = c.batch()
    params, geo, x, go = backward_data(c, B)
    need = lib.leaf_backward_workspace_bytes(B, c.T, c.F, c.K, c.hop, c.flags, int(c.dx))
    o = c.other()
    o_need = lib.leaf_backward_workspace_bytes(o.B, o.T, o.F, o.K, o.hop, o.flags, int(o.dx))
    assert need > 0 and o_need > 0
    raw = saved_pooled(lib, c, B, x, params) if c.raw else None
    ws = guarded(need, 0x00, capacity=max(need, o_need))
    rc, g1, gx1 = backward_call(lib, c, B, x, params, go, raw, ws, need, off)
    assert rc == 0, f"{c.name}: {rc}"
    for i, g in enumerate(g1):
        assert not bool((g == -1).any()), f"{c.name}: {PARAM_KEYS[i]}: {int((g == -1).sum())} gradient entries never written (or accumulated into)"
    if gx1 is not None:
        assert not bool((gx1 == -1).any()), f"{c.name}: {int((gx1 == -1).sum())} entries of g_x never written"
    ws.fill(0xFF)
    rc, g2, gx2 = backward_call(lib, c, B, x, params, go, raw, ws, need, off)
    assert rc == 0
    for i in range(len(g1)):
        assert torch.equal(g2[i], g1[i]), f"{c.name}: {PARAM_KEYS[i]} depends on what the workspace held before the call (0xFF fill)"
    assert gx1 is None or torch.equal(gx2, gx1), f"{c.name}: g_x depends on what the workspace held before the call"
    po, _, xo, goo = backward_data(o, o.B)
    ws.relayout(o_need)
    rc, _, _ = backward_call(lib, o, o.B, xo, po, goo, None, ws, o_need)
    assert rc == 0, o.name
    ws.relayout(need)
    rc, g3, gx3 = backward_call(lib, c, B, x, params, go, raw, ws, need, off)
    assert rc == 0
    for i in range(len(g1)):
        assert torch.equal(g3[i], g1[i]), f"{c.name}: {PARAM_KEYS[i]} depends on what another call left in the workspace"
    assert gx1 is None or torch.equal(gx3, gx1), f"{c.name}: g_x depends on what another call left in the workspace"
    return (B, params, geo, x, go, need, raw), g1, gx1


@pytest.mark.parametrize("c", BACKWARD_CASES, ids=[c.name for c in BACKWARD_CASES])
def test_backward_touches_only_its_buffers_and_reads_nothing_stale(c):
    from test_gpu_backward import oracle_grads
    lib = N.load()
    (B, params, geo, x, go, need, raw), g1, gx1 = backward_three_calls(lib, c)
    x64 = (x.double() / 32768 if x.dtype == torch.int16 else x.double())[:, None, :]
    if c.flags & LOG and not c.pcen:
        p64 = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
        xr = x64.clone().requires_grad_(c.dx)
        torch.log1p(lo.leaf_forward(xr, p64, geo, False, torch.float64)).backward(go.double())
        ref, ref_dx = {k: v.grad for k, v in p64.items()}, (xr.grad if c.dx else None)
    else:
        ref, ref_dx, _ = oracle_grads(x64, params, geo, c.pcen, go.double(), c.dx)
    ctx = f"({c.name} B={B} workspace {need} bytes)"
    print(ctx)
    for i, g in enumerate(g1):
        assert_grad_close(PARAM_KEYS[i], g.view(torch.float32).reshape(ref[PARAM_KEYS[i]].shape), ref[PARAM_KEYS[i]], ctx, col_tol=GRAD_TOL)
    if c.dx:
        # bfloat16 g_x is rounded to nearest even on the way out: eight significant bits, so up to half an ulp = 2^-8 of the
        # entry (the figure test_bf16_io_extension_matches_fp32_path_within_bf16_rounding uses), on top of the float bound
        tol = GRAD_TOL + (BF16_TOL if c.iodtype == torch.bfloat16 else 0.0)
        assert_grad_close("x", as_values(gx1, c.iodtype).reshape(ref_dx.shape), ref_dx, ctx, col_tol=tol, entrywise=False)
    # one word short: refused, nothing touched
    ws = guarded(need - 4, 0x5A)
    rc, g, gx = backward_call(lib, c, B, x, params, go, raw, ws, need - 4)
    assert rc == -3, rc
    assert all(bool((t == -1).all()) for t in g) and (gx is None or bool((gx == -1).all())) and bool((ws.bytes() == 0x5A).all())


# ---- alignment at the contract's minimum --------------------------------------------------------------------------------------------
# one case per family: x, out, pooled_raw, grad_out, g_x, the parameters and their gradients 4 bytes past a 4096-byte boundary (2 for
# bfloat16 / int16 buffers) -- every access the kernels make to them is one element wide (alignment table) -- give
# the bits of the aligned call.  workspace / tables stay aligned: below 16 bytes they are refused (tests/test_host_abi_alignment.py).
ALIGN_FWD = ["small-401-B2", "fft-401", "fft-552-even", "wg-401", "wg-401-straddle", "wg-401-bf16", "wg-401-pcm16", "wg-201", "wg4k-801",
             "wgg-552", "wgg4k-833", "mfma-401", "mfma-31", "staged-101", "save-wg-401", "save-mfma-401", "prepared-401"]
ALIGN_BWD = ["b401", "b401-T4801-dx", "b401-bf16-dx", "b401-pcm16", "b401-staged-dx", "b401-mfma", "b801-dx-recompute", "b552-bf16", "b833",
             "b31-dx"]


@pytest.mark.parametrize("name", ALIGN_FWD)
def test_forward_at_the_minimum_alignment_gives_the_aligned_bits(name):
    c = next(c for c in FORWARD_CASES if c.name == name)
    lib = N.load()
    params, geo = make_params(c.F, c.K, c.hop, c.pcen, c.init, c.seed)
    x = make_x(c)
    need = forward_need(lib, c)
    outs = []
    for off in (0, 4):
        tables = prepare_tables(lib, c, params, 0x00) if c.entry == "prepared" else None
        rc, out, raw = forward_call(lib, c, x, params, guarded(need, 0xFF), need, off, tables)
        assert rc == 0, (name, off, rc)
        outs.append((out, raw))
    assert torch.equal(outs[0][0], outs[1][0]), f"{name}: out differs at the minimum alignment"
    assert outs[0][1] is None or torch.equal(outs[0][1], outs[1][1]), f"{name}: pooled_raw differs at the minimum alignment"


@pytest.mark.parametrize("name", ALIGN_BWD)
def test_backward_at_the_minimum_alignment_gives_the_aligned_bits(name):
    c = next(c for c in BACKWARD_CASES if c.name == name)
    lib = N.load()
    B = c.batch()
    params, geo, x, go = backward_data(c, B)
    need = lib.leaf_backward_workspace_bytes(B, c.T, c.F, c.K, c.hop, c.flags, int(c.dx))
    raw = saved_pooled(lib, c, B, x, params) if c.raw else None
    res = []
    for off in (0, 4):
        rc, g, gx = backward_call(lib, c, B, x, params, go, raw, guarded(need, 0xFF), need, off)
        assert rc == 0, (name, off, rc)
        res.append((g, gx))
    for i in range(len(res[0][0])):
        assert torch.equal(res[0][0][i], res[1][0][i]), f"{name}: {PARAM_KEYS[i]} differs at the minimum alignment"
    assert res[0][1] is None or torch.equal(res[0][1], res[1][1]), f"{name}: g_x differs at the minimum alignment"


# ---- stage entry points --------------------------------------------------------------------------------------------------------------
def _run(lib, fn, inputs, outputs, call, ws_need=0, off=0, ws_fill=0x00):
    """inputs: {name: tensor}; outputs: {name: (shape)} float32.  `call(ptr_of, ws_ptr, ws_bytes)` makes the call."""
    ins = {k: guarded_tensor(v, off) for k, v in inputs.items() if v is not None}
    outs = {k: guarded(int(math.prod(s)) * 4, 0xFF, off) for k, s in outputs.items()}
    ws = guarded(ws_need, ws_fill) if ws_need else None
    ptr = lambda k: (ins.get(k) or outs[k]).ptr if (k in ins or k in outs) else None
    rc = call(ptr, ws.ptr if ws else None, ws_need)
    sync()
    assert rc == 0, (fn, rc)
    for k, g in ins.items():
        unchanged(g, f"{fn} {k}")
    for k, g in outs.items():
        g.check(f"{fn} {k}")
    if ws:
        ws.check(f"{fn} workspace")
    res = {k: g.cpu(torch.int32, outputs[k]) for k, g in outs.items()}
    for k, t in res.items():
        assert not bool((t == -1).any()), f"{fn}: {int((t == -1).sum())} elements of {k} never written"
    return res


def _stage(lib, fn, inputs, outputs, call, ws_need=0):
    """clean, poisoned workspace, minimum alignment: the same bits; a workspace one word short is refused."""
    a = _run(lib, fn, inputs, outputs, call, ws_need)
    b = _run(lib, fn, inputs, outputs, call, ws_need, ws_fill=0xFF)
    m = _run(lib, fn, inputs, outputs, call, ws_need, off=4, ws_fill=0xFF)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{fn}: {k} depends on what the workspace held before the call"
        assert torch.equal(a[k], m[k]), f"{fn}: {k} differs at the minimum alignment"
    if ws_need:
        ws = guarded(ws_need - 4, 0x5A)
        ins = {k: guarded_tensor(v) for k, v in inputs.items() if v is not None}
        outs = {k: guarded(int(math.prod(s)) * 4, 0xFF) for k, s in outputs.items()}
        ptr = lambda k: (ins.get(k) or outs[k]).ptr if (k in ins or k in outs) else None
        assert call(ptr, ws.ptr, ws_need - 4) == -3, fn
        sync()
        assert all(bool((g.bytes() == 0xFF).all()) for g in outs.values()) and bool((ws.bytes() == 0x5A).all())
    return {k: v.view(torch.float32) for k, v in a.items()}


@pytest.mark.parametrize("K", [64, 101])
def test_stage_entry_points(K):
    """Each stage entry point once at B = 2, F = 5, T = 333 (hop 40): guards, full overwrite, independence from the workspace's
    contents, minimum alignment, and values against the oracle's stage functions in fp64 (tolerances: test_stage_modules_match_oracle,
    _submodule_chain)."""
    lib = N.load()
    B, F, T, hop = 2, 5, 333, 40
    TP = lib.leaf_num_frames(T, K, hop)
    gen = torch.Generator().manual_seed(K)
    d = torch.float64
    kernel = torch.stack([0.1 + torch.rand(F, generator=gen) * (math.pi - 0.2), 3.0 + torch.rand(F, generator=gen) * K / 4], dim=1)
    pool_w = 0.4 * (1 + 0.2 * (torch.rand(F, generator=gen) - 0.5))
    pool_b = 1.0 + 0.1 * torch.rand(F, generator=gen)
    alpha, delta, root = (torch.full((F,), v) * (1 + 0.05 * (torch.rand(F, generator=gen) - 0.5)) for v in (0.9, 1.5, 2.5))
    ema_w = 0.06 * (1 + 0.3 * torch.rand(F, generator=gen))
    x = torch.randn(B, T, generator=gen)
    # ---- fp64 chain with autograd
    k64, x64, w64, b64 = kernel.to(d).requires_grad_(True), x.to(d)[:, None, :].requires_grad_(True), pool_w.to(d).requires_grad_(True), pool_b.to(d).requires_grad_(True)
    hr, hi = lo.gabor_taps(lo.constrain_gabor(k64, K), K)
    y64 = lo.gabor_filterbank(x64, hr, hi)
    # taps / windows
    taps = _stage(lib, "gabor_taps", {"kernel": kernel}, {"taps": (2 * F, K)}, lambda p, w, n: lib.leaf_gabor_taps_f32(p("kernel"), F, K, p("taps"), None))["taps"]
    ref_taps = torch.stack([hr, hi], dim=1).reshape(2 * F, K).detach()
    assert float((taps.double() - ref_taps).abs().max()) < 1e-7
    win = _stage(lib, "lowpass_window", {"pool_w": pool_w}, {"window": (F, K)}, lambda p, w, n: lib.leaf_lowpass_window_f32(p("pool_w"), F, K, p("window"), None))["window"]
    g64 = lo.lowpass_window(w64, K)
    assert float((win.double() - g64.detach()).abs().max()) < 2e-6
    # conv, squared modulus, pooling
    y = _stage(lib, "gabor_conv", {"x": x, "kernel": kernel}, {"y": (B, 2 * F, T)},
               lambda p, w, n: lib.leaf_gabor_conv_f32(p("x"), B, T, p("kernel"), F, K, p("y"), w, n, None), ws_need=2 * F * K * 4)["y"]
    scale = float(y64.detach().abs().max())
    assert float((y.double() - y64.detach()).abs().max()) / scale < 5e-6
    e = _stage(lib, "squared_modulus", {"y": y}, {"e": (B, F, T)}, lambda p, w, n: lib.leaf_squared_modulus_f32(p("y"), B, F, T, p("e"), None))["e"]
    e64 = lo.squared_modulus(y64)
    assert float((e.double() - e64.detach()).abs().max()) / float(e64.detach().abs().max()) < 5e-6
    pooled = _stage(lib, "gaussian_lowpass", {"e": e, "pool_w": pool_w, "pool_b": pool_b}, {"pooled": (B, F, TP)},
                    lambda p, w, n: lib.leaf_gaussian_lowpass_f32(p("e"), B, F, T, p("pool_w"), p("pool_b"), K, hop, p("pooled"), w, n, None),
                    ws_need=F * K * 4)["pooled"]
    p64 = lo.gaussian_pool(e64, g64, b64, hop)
    assert rel_err(pooled, p64.detach().float()) < REL_TOL
    # EMA, PCEN (floor 1e-6 as in _submodule_chain)
    a64, d64, r64, s64 = (t.to(d).requires_grad_(True) for t in (alpha, delta, root, ema_w))
    m64 = lo.ema_scan(p64, s64)
    ema = _stage(lib, "ema", {"p": pooled, "ema_w": ema_w}, {"ema": (B, F, TP)}, lambda p, w, n: lib.leaf_ema_f32(p("p"), B, F, TP, p("ema_w"), p("ema"), None))["ema"]
    assert rel_err(ema, m64.detach().float()) < REL_TOL
    pc_in = {"p": pooled, "alpha": alpha, "delta": delta, "root": root, "ema_w": ema_w}
    out = _stage(lib, "pcen", pc_in, {"out": (B, F, TP)},
                 lambda p, w, n: lib.leaf_pcen_f32(p("p"), B, F, TP, p("alpha"), p("delta"), p("root"), p("ema_w"), 1e-6, p("out"), None))["out"]
    a_, ir, dd = a64.clamp(max=1.0).reshape(1, -1, 1), (1.0 / r64.clamp(min=1.0)).reshape(1, -1, 1), d64.reshape(1, -1, 1)
    o64 = (p64 / (1e-6 + m64) ** a_ + dd) ** ir - dd ** ir
    assert rel_err(out, o64.detach().float()) < REL_TOL
    # the stream entry point: a stream of 38 floored frames fed as one frame, then 37, the state handed in and out; equal to the
    # fp64 recurrence over the whole stream frame for frame
    ps = 1e-5 + 2 * torch.rand(B, F, 38, generator=gen)
    m64 = lo.ema_scan(ps.to(d), s64.detach())
    o64 = (ps.to(d) / (1e-6 + m64) ** a_.detach() + dd.detach()) ** ir.detach() - dd.detach() ** ir.detach()
    state = None
    for a, n in ((0, 1), (1, 37)):
        chunk = ps[:, :, a:a + n].contiguous()
        ins = dict(pc_in, p=chunk, ema_in=state)
        r = _stage(lib, f"pcen_stream[n={n}]", ins, {"out": (B, F, n), "ema_out": (B, F)},
                   lambda p, w, nn: lib.leaf_pcen_stream_f32(p("p"), B, F, n, p("alpha"), p("delta"), p("root"), p("ema_w"), 1e-6, 0, p("ema_in"),
                                                            p("ema_out"), p("out"), None))
        assert rel_err(r["out"], o64.detach().float()[:, :, a:a + n]) < REL_TOL
        assert rel_err(r["ema_out"], m64.detach().float()[:, :, a + n - 1]) < REL_TOL
        state = r["ema_out"]
    # peak normalisation: one loud clip
    xl = x.clone()
    xl[1] *= 3.0
    pn = _stage(lib, "peak_normalize", {"x": xl}, {"out": (B, T)}, lambda p, w, n: lib.leaf_peak_normalize_f32(p("x"), B, T, p("out"), None))["out"]
    assert torch.allclose(pn, lo.peak_normalize(xl), rtol=2e-7, atol=0)
    # ---- stage backwards against fp64 autograd, workspace exactly leaf_stage_backward_workspace_bytes
    gy = torch.randn(B, 2 * F, T, generator=gen)
    ge = torch.randn(B, F, T, generator=gen)
    gp = torch.randn(B, F, TP, generator=gen)
    sz = lambda stage, t, k, h: lib.leaf_stage_backward_workspace_bytes(stage, B, t, F, k, h)
    r = _stage(lib, "gabor_conv_backward", {"x": x, "kernel": kernel, "grad_y": gy}, {"g_kernel": (F, 2), "g_x": (B, T)},
               lambda p, w, n: lib.leaf_gabor_conv_backward_f32(p("x"), B, T, p("kernel"), F, K, p("grad_y"), p("g_kernel"), p("g_x"), w, n, None),
               ws_need=sz(N.STAGE_GABOR_CONV, T, K, 1))
    gk, gxr = torch.autograd.grad(y64, (k64, x64), gy.to(d), retain_graph=True)
    assert_grad_close("kernel", r["g_kernel"], gk, "(gabor_conv_backward)")
    assert_grad_close("x", r["g_x"], gxr, "(gabor_conv_backward)", entrywise=False)
    r = _stage(lib, "squared_modulus_backward", {"y": y, "grad_e": ge}, {"grad_y": (B, 2 * F, T)},
               lambda p, w, n: lib.leaf_squared_modulus_backward_f32(p("y"), p("grad_e"), B, F, T, p("grad_y"), None))
    yl = y.double().requires_grad_(True)
    assert_grad_close("y", r["grad_y"], torch.autograd.grad(lo.squared_modulus(yl), yl, ge.to(d))[0], "(squared_modulus_backward)", entrywise=False)
    r = _stage(lib, "gaussian_lowpass_backward", {"e": e, "grad_pooled": gp, "pool_w": pool_w}, {"g_e": (B, F, T), "g_pool_w": (F,), "g_pool_b": (F,)},
               lambda p, w, n: lib.leaf_gaussian_lowpass_backward_f32(p("e"), p("grad_pooled"), B, F, T, p("pool_w"), K, hop, p("g_e"), p("g_pool_w"),
                                                                      p("g_pool_b"), w, n, None), ws_need=sz(N.STAGE_LOWPASS, T, K, hop))
    el = e.double().requires_grad_(True)
    wl, bl = pool_w.to(d).requires_grad_(True), pool_b.to(d).requires_grad_(True)
    ge_r, gw_r, gb_r = torch.autograd.grad(lo.gaussian_pool(el, lo.lowpass_window(wl, K), bl, hop), (el, wl, bl), gp.to(d))
    assert_grad_close("e", r["g_e"], ge_r, "(gaussian_lowpass_backward)", entrywise=False)
    assert_grad_close("pool_w", r["g_pool_w"], gw_r, "(gaussian_lowpass_backward)")
    assert_grad_close("pool_b", r["g_pool_b"], gb_r, "(gaussian_lowpass_backward)")
    r = _stage(lib, "ema_backward", {"p": pooled, "grad_ema": gp, "ema_w": ema_w}, {"g_p": (B, F, TP), "g_ema_w": (F,)},
               lambda p, w, n: lib.leaf_ema_backward_f32(p("p"), p("grad_ema"), B, F, TP, p("ema_w"), p("g_p"), p("g_ema_w"), w, n, None),
               ws_need=sz(N.STAGE_EMA, TP, 1, 1))
    pl = pooled.double().requires_grad_(True)
    sl = ema_w.to(d).requires_grad_(True)
    gp_r, gs_r = torch.autograd.grad(lo.ema_scan(pl, sl), (pl, sl), gp.to(d))
    assert_grad_close("p", r["g_p"], gp_r, "(ema_backward)", entrywise=False)
    assert_grad_close("ema_w", r["g_ema_w"], gs_r, "(ema_backward)")
    r = _stage(lib, "pcen_backward", dict(pc_in, grad_out=gp), {"g_p": (B, F, TP), "g_alpha": (F,), "g_delta": (F,), "g_root": (F,), "g_ema_w": (F,)},
               lambda p, w, n: lib.leaf_pcen_backward_f32(p("p"), p("grad_out"), B, F, TP, p("alpha"), p("delta"), p("root"), p("ema_w"), 1e-6, p("g_p"),
                                                          p("g_alpha"), p("g_delta"), p("g_root"), p("g_ema_w"), w, n, None),
               ws_need=sz(N.STAGE_PCEN, TP, 1, 1))
    al, dl, rl, sl = (t.to(d).requires_grad_(True) for t in (alpha, delta, root, ema_w))
    ml = lo.ema_scan(pl, sl)
    ol = (pl / (1e-6 + ml) ** al.clamp(max=1.0).reshape(1, -1, 1) + dl.reshape(1, -1, 1)) ** (1.0 / rl.clamp(min=1.0)).reshape(1, -1, 1) \
        - dl.reshape(1, -1, 1) ** (1.0 / rl.clamp(min=1.0)).reshape(1, -1, 1)
    refs = torch.autograd.grad(ol, (pl, al, dl, rl, sl), gp.to(d))
    assert_grad_close("p", r["g_p"], refs[0], "(pcen_backward)", entrywise=False)
    for name, ref in zip(("g_alpha", "g_delta", "g_root", "g_ema_w"), refs[1:]):
        assert_grad_close(name, r[name], ref, "(pcen_backward)")
