"""Forward parity at clip-length edges for every kernel family (the forward's counterpart of tests/test_gpu_backward_edges.py).

Every forward family, forced through its selector (`m._algo`; AUTO thresholds are not involved), on the lattice of clip lengths
T in {1, 2, 3, h-1, h, h+1, padL, padL+1, K-1, K, K+1, L-1, L, L+1, 2L, 2L+1, 5L+3} plus the family's extras (h the hop, padL the left
padding, L the block length of the family's plan; tests/forward_edges_cases.py holds the groups, the lattices and the seeded draws,
tests/test_host_forward_edges.py their conditioning: the float32 oracle within 5e-6 of the fp64 one at every case).  A forward that
indexes one sample or one frame past a clip end at such a length fails here.  Every case asserts

  1. the oracle's shape, finite values and rel_err(out, fp64 oracle) < REL_TOL = 2e-5 elementwise (the suite's REL_TOL / BAND_TOL);
  2. bit-exact clip independence: the batch flipped along B gives the flipped bits;
  3. workgroup kernels (families 3 - 7): whole clips per workgroup (a), one block per workgroup with the row kernel (b), five clips
     straddling three workgroups (c) and the streaming finalize give the same bits clip for clip; the per-wave kernel on the same
     clips stays within 1e-5 (tests/test_gpu_parity.py, test_workgroup_kernel_static_geometries);
  4. band families (3, 5): band tasks within BAND_VS_FULL = 5e-6 of the full transforms (tests/test_gpu_band.py), and not their bits
     from T >= K on;
  5. the training forward (families 1 - 7, save_raw=True) at bound 1, its pre-floor pooled tensor at REL_TOL relative to
     max(|ref|, 1e-5) -- the pooling floor, below which no result depends on the value.  (The suite asserts `out` of the training
     forward equal to the inference call's bits for the small-batch kernel only, which is not among these families.)
  6. sample kinds (families 3 - 5): int16 PCM gives the bits of the float32 call on x / 32768 (tests/test_gpu_pcm16.py); bfloat16
     I/O the float32 call's result rounded to bfloat16, within 2^-8 of the oracle (test_bf16_io_extension_matches_fp32_path...).

Every case prints its figures; with LEAF_FWD_EDGE_LOG set they are appended there as JSON lines (profiles/forward_edges.txt).

Found with this file and fixed: nothing.  All 449 cases pass on an MI355X (256 CUs) against the kernels as they stood.  Worst rel_err
against the fp64 oracle per family (profiles/forward_edges.txt): 1: 6.3e-7, 2: 5.9e-7, 3: 9.2e-7, 4: 8.8e-7, 5: 7.1e-7, 6: 8.2e-7,
7: 7.3e-7, 8: 1.0e-6, 9: 1.3e-6, 10: 8.8e-7 -- all at PCEN-on cases, most at the longest clip; band tasks against full transforms
6.0e-7 (family 3) and 4.2e-7 (family 5); workgroup against per-wave kernel 6.0e-7; pooled_raw of the training forward 5.3e-7.  The
host test's conditioning figures for the same cases are 0.9e-6 .. 4.0e-6, so the kernels sit below the float32 oracle's own error."""
import json
import os

import pytest
import torch

import forward_edges_cases as fe
from conftest import rel_err
from helpers import make_leaf
from oracle import leaf_oracle as lo
from leaf_pytorch_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 2e-5                    # tests/test_gpu_parity.py REL_TOL, tests/test_gpu_band.py BAND_TOL
BAND_VS_FULL = 5e-6               # tests/test_gpu_band.py
WG_VS_PER_WAVE = 1e-5             # tests/test_gpu_parity.py, test_workgroup_kernel_static_geometries
BF16_TOL = 2 ** -8                # tests/test_gpu_parity.py, test_bf16_io_extension_matches_fp32_path_within_bf16_rounding
FLOOR_POOLED = 1e-5               # frontend.py:84
WG, FULL, SF = _native.ALGO_FFT_WG, _native.ALGO_FULL_TRANSFORMS, _native.ALGO_STREAM_FINALIZE
NAMES = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha", "_compression.delta",
         "_compression.root", "_compression.ema._weights"]
_LOG = os.environ.get("LEAF_FWD_EDGE_LOG")
RAN = set()                       # families of the table that ran
RAN_SMALL = set()                 # forms of the small-batch kernel that ran, as the workspace size says


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_extension():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    _native.load()


def n_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def cus(n):
    """algo bits that leave the call `n` CUs (n workgroups), 0: all of them (tests/test_gpu_band.py, for the device's own CU count)."""
    if not n:
        return 0
    assert 0 < n <= n_cus() and n_cus() - n < 256, (n, n_cus())
    return _native.algo_reserve_cus(n_cus() - n)


def ws_bytes(B, T, F, K, hop, algo):
    return _native.load().leaf_workspace_bytes(B, T, F, K, hop, algo)


def run(m, x, algo):
    m._algo = algo
    with torch.no_grad():
        out = m(x.to(DEV))
    torch.cuda.synchronize()
    return out.cpu()


def record(g, T, pcen, what, value):
    print(f"{g.name} T={T} pcen={pcen}: {what} {value:.3e}")
    if _LOG:
        with open(_LOG, "a") as fh:
            fh.write(json.dumps({"family": g.family, "group": g.name, "T": T, "pcen": pcen, "what": what, "value": value}) + "\n")


_LAST = {}


def drawn_with_reference(g, T, pcen):
    """The case's draw and its fp64 reference (with the pre-floor pooled tensor), computed once."""
    key = (g.name, T, pcen)
    if _LAST.get("key") != key:
        geo, params, x = fe.draw(g, T, pcen)
        _LAST.update(key=key, value=(geo, params, x, *fe.oracle(x, params, geo, pcen, stages=True)))
    return _LAST["value"]


def against_oracle(g, T, pcen, out, ref, what):
    assert out.dtype == torch.float32 and out.shape == ref.shape, (g.name, T, what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), (g.name, T, pcen, what)
    e = rel_err(out, ref)
    record(g, T, pcen, what + " vs fp64 oracle", e)
    assert e < REL_TOL, f"{g.name} T={T} pcen={pcen} {what}: {e:.3e} from the fp64 oracle (bound {REL_TOL:.0e})"


def native_args(params, pcen):
    return [params[k].to(DEV) for k in NAMES[:3]] + ([params[k].to(DEV) for k in NAMES[3:]] if pcen else [None] * 4)


def training_forward(g, T, pcen, params, x, ref, ref_raw, algo):
    out, raw = _native.leaf_forward(x.to(DEV), *native_args(params, pcen), g.K, g.hop, pcen=pcen, algo=algo, save_raw=True)
    torch.cuda.synchronize()
    against_oracle(g, T, pcen, out.cpu(), ref, "training forward")
    raw = raw.cpu()
    assert raw.dtype == torch.float32 and raw.shape == ref_raw.shape and torch.isfinite(raw).all(), (g.name, T)
    e = float(((raw.double() - ref_raw).abs() / ref_raw.abs().clamp_min(FLOOR_POOLED)).max())
    record(g, T, pcen, "pooled_raw vs fp64 oracle", e)
    assert e < REL_TOL, f"{g.name} T={T} pcen={pcen}: pooled_raw {e:.3e} from the oracle's pre-floor pooled stage (bound {REL_TOL:.0e})"


def plan_block_len(g):
    """The block length of the plan the library reports for the group's geometry, None where it reports none: the 2048-sample plan at
    a handful of blocks, the 4096-sample one at a batch AUTO hands to the workgroup kernel (leaf_fft_plan_info reports what AUTO runs)."""
    if g.family in (5, 7):
        assert 64 * 8 >= n_cus() * 7 // 16                      # leaf_kernels.hip, fft_wg_min_blocks
        info = _native.fft_plan_info(64, 8 * 4096, 8, g.K, g.hop)
        assert info is not None and info["fft_n"] == 4096, (g.name, info)
        return info["block_len"]
    if g.family in (9, 10):
        return None
    info = _native.fft_plan_info(4, 8 * 4096, 8, g.K, g.hop)
    assert info is not None and info["fft_n"] == 2048, (g.name, info)
    return info["block_len"]


def edge_case(g, T, pcen):
    """One (group, T, pcen): every assertion of the module's docstring that applies to the group's family."""
    sel = getattr(_native, g.selector)
    K, hop, L, F, B = g.K, g.hop, g.L, g.F, g.B
    geo, params, x, ref, ref_raw = drawn_with_reference(g, T, pcen)
    assert x.shape == (B, 1, T) and ref.shape == (B, F, (T - 1) // hop + 1)
    m = make_leaf(F, K, hop, pcen, params, DEV)
    nblk = -(-T // L)
    wg = g.family in (3, 4, 5, 6, 7)
    base = sel
    if wg:
        base = sel | cus(B)                                     # (a) whole clips per workgroup
    elif g.shape == "pair":                                    # B F <= 60 here: between half and twice the CALL's CUs, the rest reserved
        base = sel | cus(fe.SMALL_CUS)                          # (make_small_plan sizes both forms by the CUs the call may fill)
    assert ws_bytes(B, T, F, K, hop, base) > 0, f"{g.name}: {g.selector} does not serve B={B} T={T} F={F}"
    if g.family == 8:                                           # which form runs: the workspace says (make_small_plan adds carry_floats for SPLIT)
        call_cus = fe.SMALL_CUS if g.shape == "pair" else n_cus()
        if g.shape == "split":
            assert 2 * B * F <= n_cus()
        else:
            assert call_cus / 2 < B * F <= 2 * call_cus
        split = fe.small_is_split(B, F, T, L, call_cus)
        assert split == (g.shape == "split" and T >= L + 1), (g.name, T)
        assert ws_bytes(B, T, F, K, hop, base) == fe.small_workspace_bytes(B, F, split), (g.name, T, split)
        assert fe.small_workspace_bytes(B, F, True) - fe.small_workspace_bytes(B, F, False) == 4 * (-(-4 * B * F // 64) * 64)
        if nblk >= 2:
            RAN_SMALL.add("split" if split else "pair")
    if g.band:
        cls = _native.band_classes(params[NAMES[0]].to(DEV), params[NAMES[1]].reshape(-1).to(DEV), K, hop, params[NAMES[2]].to(DEV)).cpu().tolist()
        assert any(c not in (2048, 4096) for c in cls), (g.name, cls)

    out = run(m, x, base)
    against_oracle(g, T, pcen, out, ref, g.selector)
    assert torch.equal(run(m, x.flip(0), base).flip(0), out), f"{g.name} T={T}: clip independence, bit-exact"       # 2.

    if wg:
        outs = {"band" if g.band else "default": (0, out)}
        if g.band:
            full = run(m, x, base | FULL)
            against_oracle(g, T, pcen, full, ref, "full transforms")
            d = rel_err(out, full)
            record(g, T, pcen, "band vs full transforms", d)
            assert d < BAND_VS_FULL, f"{g.name} T={T} pcen={pcen}: band tasks {d:.3e} from the full transforms (bound {BAND_VS_FULL:.0e})"
            if T >= K:
                assert not torch.equal(out, full), f"{g.name} T={T}: the band tasks did not run"
            outs["full"] = (FULL, full)
        if T in fe.seam_subset(L):                              # 3.
            assert B == 5 and B * nblk <= n_cus()
            for what, (bits, want) in outs.items():
                dealings = {"(b) one block per workgroup": sel | bits, "(c) five clips on three workgroups": sel | bits | cus(3)}
                if g.family in (3, 4, 5):
                    dealings["streaming finalize"] = sel | bits | SF | cus(B)
                for name, algo in dealings.items():
                    assert ws_bytes(B, T, F, K, hop, algo) > 0
                    assert torch.equal(run(m, x, algo), want), f"{g.name} T={T} pcen={pcen} {what}: {name} against (a), bit for bit"
        if K <= 1217:                                           # (the per-wave kernel's plan ends there: make_fft_plan)
            assert ws_bytes(B, T, F, K, hop, _native.ALGO_FFT) > 0
            pw = run(m, x, _native.ALGO_FFT)
            for what, (_, o) in outs.items():
                d = rel_err(o, pw)
                record(g, T, pcen, f"{what} vs per-wave kernel", d)
                assert d < WG_VS_PER_WAVE, f"{g.name} T={T} pcen={pcen} {what}: {d:.3e} from the per-wave kernel (bound {WG_VS_PER_WAVE:.0e})"
        else:
            assert ws_bytes(B, T, F, K, hop, _native.ALGO_FFT) == 0

    if g.family <= 7 and T in fe.train_subset(hop, L):          # 5.
        training_forward(g, T, pcen, params, x, ref, ref_raw, base)

    if g.family in (3, 4, 5) and T in fe.kinds_subset(hop, L):  # 6.
        x16 = torch.randint(-32768, 32768, (B, 1, T), generator=torch.Generator().manual_seed(g.seed + T), dtype=torch.int32).to(torch.int16)
        got, want = run(m, x16, base), run(m, x16.float() / 32768, base)
        assert got.dtype == torch.float32 and torch.equal(got, want), f"{g.name} T={T} pcen={pcen}: int16 PCM against x / 32768, bit for bit"
        xb = x.to(torch.bfloat16)
        ob, of = run(m, xb, base), run(m, xb.float(), base)
        assert ob.dtype == torch.bfloat16 and ob.shape == of.shape
        assert torch.equal(ob, of.to(torch.bfloat16)), f"{g.name} T={T} pcen={pcen}: bfloat16 I/O against the float32 call rounded"
        e = rel_err(ob.float(), lo.leaf_forward(xb.float(), params, geo, pcen, torch.float32))
        record(g, T, pcen, "bfloat16 I/O vs oracle", e)
        assert e < BF16_TOL, f"{g.name} T={T} pcen={pcen}: bfloat16 I/O {e:.3e} from the oracle (bound 2^-8)"
    m._algo = _native.ALGO_AUTO
    RAN.add(g.family)


def cases_of(family):
    return [pytest.param(g, T, pcen, id=f"{g.name}-{fe.case_id(T, pcen)}") for g, T, pcen in fe.all_cases() if g.family == family]


def test_lattice_restates_the_plans_block_lengths():
    """L is a literal per group (tests/forward_edges_cases.py); the plan's own figure where the library reports the plan that runs."""
    reported = 0
    for g in fe.GROUPS:
        assert g.L == fe.expected_block_len(g), g.name
        got = plan_block_len(g) if g.family != 8 else _native.fft_plan_info(4, 8 * 4096, 8, g.K, g.hop)["block_len"]
        if got is not None:
            assert got == g.L, (g.name, got, g.L)
            reported += 1
    assert reported == sum(1 for g in fe.GROUPS if g.family not in (9, 10))
    slots = {K: _native.fft_plan_info(4, 8 * 4096, 8, K, hop)["slots"] for K, hop in ((552, 220), (601, 240), (1216, 300))}
    assert slots == {552: 2, 601: 2, 1216: 3}, slots


# ---- 1. per-wave kernel, static instances
@pytest.mark.parametrize("g,T,pcen", cases_of(1))
def test_per_wave_static(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 2. per-wave kernel, generic instances: odd window, even window, three slots
@pytest.mark.parametrize("g,T,pcen", cases_of(2))
def test_per_wave_generic(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 3. workgroup kernel, static 16 kHz: band tasks and full transforms
@pytest.mark.parametrize("g,T,pcen", cases_of(3))
def test_workgroup_static_16k_band_and_full(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 4. workgroup kernel, static 8 kHz
@pytest.mark.parametrize("g,T,pcen", cases_of(4))
def test_workgroup_static_8k(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 5. workgroup kernel, static 32 kHz on 4096-sample blocks: band tasks and full transforms
@pytest.mark.parametrize("g,T,pcen", cases_of(5))
def test_workgroup_static_32k_band_and_full(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 6. workgroup kernel, run-time geometry on 2048-sample blocks
@pytest.mark.parametrize("g,T,pcen", cases_of(6))
def test_workgroup_runtime_geometry_2048(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 7. workgroup kernel, run-time geometry on 4096-sample blocks
@pytest.mark.parametrize("g,T,pcen", cases_of(7))
def test_workgroup_runtime_geometry_4096(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 8. one-launch small-batch kernel: SPLIT and one workgroup per (clip, filter)
@pytest.mark.parametrize("g,T,pcen", cases_of(8))
def test_small_batch_split_and_pair(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 9. MFMA: noff_t 1, 3, 6 and the even window
@pytest.mark.parametrize("g,T,pcen", cases_of(9))
def test_mfma(g, T, pcen):
    edge_case(g, T, pcen)


# ---- 10. staged, reduced lattice
@pytest.mark.parametrize("g,T,pcen", cases_of(10))
def test_staged(g, T, pcen):
    edge_case(g, T, pcen)


def test_every_family_of_the_table_ran():
    """Every family of the table ran a case, and both forms of the small-batch kernel.  (Run on its own, or with a selection that left
    a family out, this test runs T = L + 1 of the groups that have not run.)"""
    for g in fe.GROUPS:
        if g.family not in RAN or (g.family == 8 and g.shape not in RAN_SMALL):
            edge_case(g, g.L + 1, True)
    assert RAN == set(fe.FAMILIES), sorted(RAN)
    assert RAN_SMALL == {"split", "pair"}, sorted(RAN_SMALL)
