"""CPU-only tests: module surface (reference drop-in contract), C-ABI export, error conventions."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

import leaf_pytorch_amd as L
from leaf_pytorch_amd import _native
from conftest import Golden, REPO
from oracle import leaf_oracle as lo

REF_KEYS = ["_complex_conv._kernel", "_pooling.weights", "_pooling._bias", "_compression.alpha",
            "_compression.delta", "_compression.root", "_compression.ema._weights"]


def test_constructor_signature_matches_reference():
    import inspect
    sig = inspect.signature(L.Leaf.__init__)
    names = list(sig.parameters)[1:]
    assert names == ["n_filters", "sample_rate", "window_len", "window_stride", "preemp", "init_min_freq",
                     "init_max_freq", "mean_var_norm", "pcen_compression", "use_legacy_complex", "initializer"]
    d = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert (d["n_filters"], d["sample_rate"], d["window_len"], d["window_stride"]) == (40, 16000, 25.0, 10.0)
    assert (d["init_min_freq"], d["init_max_freq"], d["pcen_compression"], d["initializer"]) == (60.0, 7800.0, True, "default")


def test_state_dict_contract():
    m = L.Leaf()
    sd = m.state_dict()
    assert list(sd) == REF_KEYS
    assert tuple(sd["_complex_conv._kernel"].shape) == (40, 2)
    assert tuple(sd["_pooling.weights"].shape) == (1, 1, 40, 1)
    for k in REF_KEYS[2:]:
        assert tuple(sd[k].shape) == (40,)
    assert all(p.requires_grad and p.dtype == torch.float32 for p in m.parameters())
    assert len(list(m.buffers())) == 0
    assert list(L.Leaf(pcen_compression=False).state_dict()) == REF_KEYS[:3]
    # attribute names the reference exposes
    assert m._preemp is None and m._instance_norm is None and float(m._maximum_val) == pytest.approx(1e-5)
    assert hasattr(m._complex_conv, "constraint") and hasattr(m._compression, "ema")
    assert m._complex_conv.use_legacy_complex is False


def test_initial_values_match_reference_defaults():
    m = L.Leaf()
    assert torch.equal(m._pooling.weights.data, torch.full((1, 1, 40, 1), 0.4))
    assert torch.equal(m._pooling._bias.data, torch.ones(40))
    c = m._compression
    assert torch.allclose(c.alpha.data, torch.full((40,), 0.96)) and torch.equal(c.delta.data, torch.full((40,), 2.0))
    assert torch.equal(c.root.data, torch.full((40,), 2.0)) and torch.allclose(c.ema._weights.data, torch.full((40,), 0.04))
    assert c._floor == 1e-12
    assert torch.equal(m._complex_conv._kernel.data, lo.mel_gabor_init(40, 16000))


def test_loads_reference_state_dict_strictly():
    g = Golden("perturbed_uniform_b3")
    m = L.Leaf()
    assert m.load_state_dict(g.params, strict=True).missing_keys == []
    for k, v in m.state_dict().items():
        assert torch.equal(v, g.params[k])


def test_error_conventions():
    with pytest.raises(NotImplementedError, match="Pre-emp"):
        L.Leaf(preemp=True)
    with pytest.raises(NotImplementedError, match="Instance Norm"):
        L.Leaf(mean_var_norm=True)
    with pytest.raises(ValueError, match="unsupported initializer"):
        L.Leaf(initializer="nope")
    with pytest.raises(ValueError, match="SimpleRNN"):
        L.PCENLayer(4)
    for init in ("random", "xavier_normal", "kaiming_normal", lambda s: torch.zeros(*s)):
        assert tuple(L.Leaf(initializer=init)._complex_conv._kernel.shape) == (40, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.Leaf()(torch.randn(1, 1, 16000))


def test_geometry_arithmetic():
    for sr, k, hop in ((16000, 401, 160), (22050, 552, 220), (32000, 801, 320), (8000, 201, 80), (44100, 1103, 441)):
        m = L.Leaf(sample_rate=sr, initializer="random")
        assert (m._complex_conv._kernel_size, m._pooling.strides) == (k, hop)
    assert L.get_padding_value(401) == (200, 200) and L.get_padding_value(552) == (275, 276)


def test_get_frontend_reads_reference_cfg_keys():
    cfg = {"frontend": {"name": "leaf", "default_args": True, "use_legacy_complex": True},
           "audio_config": {"sample_rate": 16000}}
    fe = L.get_frontend(cfg)
    assert isinstance(fe, L.Leaf) and fe._complex_conv.use_legacy_complex is True
    cfg = {"frontend": {"name": "LEAF", "n_filters": 64, "pcen_compress": False, "initializer": "random"},
           "audio_config": {"sample_rate": 32000, "window_len": 25.0, "window_stride": 10.0}}
    fe = L.get_frontend(cfg)
    assert fe._complex_conv._filters == 64 and fe._compression is None and fe._pooling.strides == 320
    with pytest.raises(NotImplementedError):
        L.get_frontend({"frontend": {"name": "mel"}, "audio_config": {}})


def test_get_frontend_loads_pretrained(tmp_path):
    g = Golden("perturbed_uniform_b3")
    path = tmp_path / "fe.pt"
    torch.save(g.params, path)
    fe = L.get_frontend({"frontend": {"name": "leaf", "default_args": True, "pretrained": str(path)},
                         "audio_config": {}})
    assert torch.equal(fe._pooling._bias.data, g.params["_pooling._bias"])


def test_reference_import_path_shim():
    """`from leaf_pytorch import get_frontend` (models/classifier.py:3) resolves to the HIP frontend."""
    import importlib
    import sys
    for k in [k for k in sys.modules if k == "leaf_pytorch" or k.startswith("leaf_pytorch.")]:
        del sys.modules[k]
    mod = importlib.import_module("leaf_pytorch")
    assert os.path.realpath(mod.__file__).startswith(os.path.realpath(REPO))
    from leaf_pytorch.frontend import Leaf as ShimLeaf
    from leaf_pytorch import get_frontend
    assert ShimLeaf is L.Leaf and get_frontend is L.get_frontend


def test_cabi_exports_every_declared_symbol():
    """The shared library loads without a GPU and exports exactly what include/leaf_hip.h declares."""
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    declared = set(re.findall(r"\b(leaf_[a-z0-9_]+)\s*\(", header)) - {"leaf_status"}
    assert declared == set(_native.EXPORTED_SYMBOLS), declared ^ set(_native.EXPORTED_SYMBOLS)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.leaf_abi_version() == _native.ABI_VERSION


def test_cabi_host_side_arithmetic_and_argument_checks():
    lib = _native.load()
    for t, k, hop in ((1, 401, 160), (16000, 401, 160), (16001, 401, 160), (5000, 552, 220), (2000, 81, 160)):
        geo = lo.LeafGeometry(1, 0, k, hop, *lo.same_padding(k))
        assert lib.leaf_num_frames(t, k, hop) == geo.n_frames(t)
    assert lib.leaf_num_frames(0, 401, 160) < 0
    assert lib.leaf_workspace_bytes(256, 16000, 40, 401, 160, _native.ALGO_MFMA) > 0
    assert lib.leaf_workspace_bytes(256, 16000, 40, 401, 160, _native.ALGO_STAGED) > 256 * 80 * 16000 * 4
    assert lib.leaf_workspace_bytes(0, 16000, 40, 401, 160, 0) == 0
    assert lib.leaf_workspace_bytes(4, 16000, 40, 401, 160, 77) == 0
    # null pointers / bad shapes are rejected before any launch
    assert lib.leaf_forward_f32(None, 1, 1, None, None, None, None, None, None, None, 40, 401, 160, 1, 0, None, None, 0, None) == -1
    assert lib.leaf_gabor_taps_f32(None, 40, 401, None, None) == -1
    assert lib.leaf_status_string(-3).decode().startswith("workspace")
    # serving-mode tables: sized by (F, K) only; 0 where the overlap-save path does not apply
    nb = lib.leaf_fft_tables_bytes(40, 401, 160)
    assert nb >= 40 * 2048 * 4 + 40 * (401 + 64) * 4 and nb % 4 == 0
    assert lib.leaf_fft_tables_bytes(40, 552, 220) > lib.leaf_fft_tables_bytes(40, 441, 220)    # longer pooling rows
    # the 16 kHz geometry also carries the parameter-only tables of the band-limited filter tasks (records + decimated windows)
    assert nb >= 40 * 2048 * 4 + 40 * (401 + 64) * 4 + 40 * (4 + 232) * 4
    assert lib.leaf_fft_tables_bytes(40, 1601, 640) == 0 and lib.leaf_fft_tables_bytes(0, 401, 160) == 0
    assert lib.leaf_fft_prepare_tables_f32(None, None, 40, 401, 160, None, 0, None) == -1
    assert lib.leaf_forward_prepared_f32(None, 1, 16000, None, 0, None, None, None, None, None, 40, 401, 160, 1, None, None, 0,
                                         None) == -1
    assert lib.leaf_peak_normalize_f32(None, 1, 1, None, None) == -1


def test_auto_algorithm_policy():
    """LEAF_ALGO_AUTO: FFT kernel for long windows + chip-filling batches, MFMA otherwise, staged as last resort."""
    lib = _native.load()
    FFT, MFMA, STAGED, WG, SMALL = (_native.ALGO_FFT, _native.ALGO_MFMA, _native.ALGO_STAGED, _native.ALGO_FFT_WG,
                                    _native.ALGO_FFT_SMALL)
    assert lib.leaf_auto_algo(256, 16000, 40, 401, 160) == WG           # BASELINE configs[1]: workgroup-per-block kernel
    assert lib.leaf_auto_algo(128, 160000, 80, 801, 320) == WG          # configs[2] per-GPU shard
    assert lib.leaf_auto_algo(4, 16000, 40, 401, 160) == SMALL          # configs[0]: a handful of clips -> everything in one launch
    assert lib.leaf_auto_algo(1, 16000, 40, 401, 160) == SMALL and lib.leaf_auto_algo(6, 16000, 40, 401, 160) == SMALL
    assert lib.leaf_auto_algo(7, 16000, 40, 401, 160) == SMALL and lib.leaf_auto_algo(12, 16000, 40, 401, 160) == SMALL   # two rounds of workgroups (round 5)
    assert lib.leaf_auto_algo(13, 16000, 40, 401, 160) == WG           # more (clip, filter) pairs than two rounds: the workgroup kernel (130 blocks)
    assert lib.leaf_auto_algo(2, 40000, 40, 401, 160) == FFT            # clips longer than two ring passes (20 blocks)
    assert lib.leaf_auto_algo(2, 32000, 40, 401, 160) == SMALL          # 2 s clips: two passes
    assert lib.leaf_auto_algo(4, 8000, 40, 201, 80) == SMALL            # 8 kHz LEAF
    assert lib.leaf_auto_algo(4, 32000, 80, 801, 320) == FFT            # 32 kHz: 34 blocks of 2048 samples per second
    assert lib.leaf_auto_algo(16, 16000, 40, 401, 160) == WG            # from ~half a block per CU the workgroup kernel wins
    assert lib.leaf_auto_algo(256, 10000, 40, 251, 100) == WG           # from K ~ 224 the transforms pay off (run-time geometry)
    assert lib.leaf_auto_algo(4, 10000, 40, 251, 100) == FFT            # ... per-wave kernel below one block per CU
    assert lib.leaf_auto_algo(256, 22050, 40, 552, 220) == WG           # even window (22.05 kHz): real-spectrum form + lone tap
    assert lib.leaf_auto_algo(256, 4000, 40, 401, 16) == WG             # any hop: the run-time-geometry kernel walks frames, not rows
    assert lib.leaf_auto_algo(256, 48000, 40, 1217, 480) == WG          # odd windows from 833 taps: 4096-sample blocks
    assert lib.leaf_auto_algo(256, 48000, 40, 1218, 480) == MFMA        # even and beyond the 2048-sample plan: direct form
    assert lib.leaf_auto_algo(2, 48000, 40, 1201, 480) == FFT           # too few 4096-sample blocks for the chip: per-wave kernel
    assert lib.leaf_auto_algo(256, 8000, 40, 201, 80) == WG             # 8 kHz LEAF: static instances exist
    assert lib.leaf_auto_algo(8, 8000, 40, 201, 80) == SMALL and lib.leaf_auto_algo(13, 8000, 40, 201, 80) == FFT
    assert lib.leaf_auto_algo(256, 6000, 40, 151, 60) == MFMA           # other short windows: direct form is as cheap
    assert lib.leaf_auto_algo(64, 48000, 40, 1201, 480) == WG           # 48 kHz
    assert lib.leaf_auto_algo(64, 64000, 40, 1601, 640) == WG           # 64 kHz: 4096-sample plan up to K = 2049
    assert lib.leaf_auto_algo(64, 96000, 40, 2401, 960) not in (FFT, WG)   # beyond it: direct form
    assert lib.leaf_auto_algo(2, 4000, 40, 5001, 160) == STAGED         # taps fit neither LDS plan
    assert lib.leaf_auto_algo(0, 16000, 40, 401, 160) < 0
    for args in ((256, 16000, 40, 401, 160), (4, 16000, 40, 401, 160), (2, 4000, 40, 5001, 160)):
        assert lib.leaf_workspace_bytes(*args, _native.ALGO_AUTO) == lib.leaf_workspace_bytes(*args, lib.leaf_auto_algo(*args))
    assert lib.leaf_workspace_bytes(4, 16000, 40, 401, 160, WG) == lib.leaf_workspace_bytes(4, 16000, 40, 401, 160, FFT) > 0
    assert lib.leaf_workspace_bytes(4, 16000, 40, 401, 160, SMALL) == 256      # only the per-clip scales of LEAF_FLAG_PEAKNORM
    assert lib.leaf_workspace_bytes(13, 16000, 40, 401, 160, SMALL) == 0 and lib.leaf_workspace_bytes(4, 10000, 40, 251, 100, SMALL) == 0
    assert lib.leaf_workspace_bytes(4, 10000, 40, 251, 100, WG) > 0     # run-time-geometry workgroup kernel
    assert lib.leaf_workspace_bytes(4, 48000, 40, 1217, 480, WG) > 0    # 4096-sample plan
    assert lib.leaf_workspace_bytes(4, 48000, 40, 1218, 480, WG) == 0   # even, more taps per lane than the 2048-sample kernel holds


def test_tools_and_entry_points_compile():
    """Every script under tools/ (and bench.py / __graft_entry__.py) is at least syntactically valid Python: they only run on
    the GPU box, where a typo would cost a gpurun call."""
    import glob
    import py_compile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "tools", "*.py"))) + [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")]
    assert len(files) > 10
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for i, f in enumerate(files):
            py_compile.compile(f, doraise=True, cfile=os.path.join(tmp, f"{i}.pyc"))


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc (no GPU)")
def test_kernel_resource_table_has_no_unexplained_scratch(tmp_path):
    """tools/kernel_resources.py: every kernel's VGPRs / scratch / occupancy from -Rpass-analysis=kernel-resource-usage (the
    table DESIGN.md quotes, profiles/<round>/kernel_resources.csv); a kernel with scratch that is not explained in the tool's
    allow-list fails the check.  Also: the dominant kernels stay at three waves per SIMD without scratch, and the product
    library reads no tools-only environment switch."""
    import csv
    import subprocess
    import sys
    out = tmp_path / "res.csv"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--check", "--out", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = {row["kernel"]: row for row in csv.DictReader(open(out))}
    for name in ("leaf_fft_wg_kernel<401, 160, 12, false>", "leaf_fft_wg4k_kernel<801, 320, 12>"):
        assert int(rows[name]["scratch_bytes_per_lane"]) == 0 and int(rows[name]["occupancy_waves_per_simd"]) == 3, rows[name]
    assert not any("<3, 6," in k or "<2, 6," in k or ", 16, false>" in k for k in rows), "A/B instantiations belong behind -DLEAF_TOOLS"
    strings = subprocess.run(["strings", _native.LIB_PATH], capture_output=True, text=True).stdout.splitlines()   # whole strings: names, not words of messages
    assert sorted(s for s in strings if re.fullmatch(r"LEAF_[A-Z0-9_]+", s)) == ["LEAF_NO_4K"]


def test_gabor_constraint_module_matches_the_oracle_bit_for_bit():
    """convolution.py:15-22 builds the sigma bounds from a float32 tensor; the host-side module must do the same (VERDICT r3
    weak #1: it used Python doubles).  Bit for bit against the oracle's ``constrain_gabor`` (itself pinned to the taps the
    reference produced for ``clamps_b2``), on the clamp fixture, at the bounds themselves and one ulp either side, for the
    three LEAF window sizes and an even one."""
    import numpy as np
    from leaf_pytorch_amd.modules import GaborConstraint
    g = Golden("clamps_b2")
    k = g.params["_complex_conv._kernel"]
    assert torch.equal(GaborConstraint(g.window_size)(k), lo.constrain_gabor(k, g.window_size))
    for K in (401, 801, 201, 552):
        c32 = torch.sqrt(2.0 * torch.log(torch.tensor(2.0))) / math.pi
        edges = []
        for bound in (float(4 * c32), float(K * c32), 4 * math.sqrt(2 * math.log(2)) / math.pi, K * math.sqrt(2 * math.log(2)) / math.pi):
            b = np.float32(bound)
            edges += [b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1e9))]
        sig = torch.tensor(np.array(edges + [0.0, 1e6], dtype=np.float32))
        mu = torch.linspace(-0.5, 3.5, sig.numel())
        kern = torch.stack([mu, sig], dim=1)
        got, want = GaborConstraint(K)(kern), lo.constrain_gabor(kern, K)
        assert got.dtype == torch.float32 and torch.equal(got, want), K
    # functional: the parameter is untouched and the clamp is differentiable like the reference's
    p = torch.nn.Parameter(torch.tensor([[-1.0, 0.1], [1.0, 50.0]]))
    GaborConstraint(401)(p).sum().backward()
    assert p.grad.tolist() == [[0.0, 0.0], [1.0, 1.0]] and p.data[0, 0] == -1.0


def test_empty_batch_is_not_an_error_at_the_c_abi():
    """B = 0: the reference returns (0, F, T') (fixture empty_b0); the entry points accept it before looking at any data
    pointer and launch nothing -- checkable without a GPU.  Every other extent must still be valid."""
    lib = _native.load()
    nul = (None,) * 7
    assert lib.leaf_forward_f32(None, 0, 1600, *nul, 40, 401, 160, 1, 0, None, None, 0, None) == 0
    assert lib.leaf_forward_save_f32(None, 0, 1600, *nul, 40, 401, 160, 1, 0, None, None, None, 0, None) == -1   # raw is required
    assert lib.leaf_forward_prepared_f32(None, 0, 1600, None, 0, None, None, None, None, None, 40, 401, 160, 1, None, None, 0, None) == 0
    for bad in ((0, 0, 40, 401, 160), (0, 1600, 0, 401, 160), (0, 1600, 40, 0, 160), (0, 1600, 40, 401, 0), (-1, 1600, 40, 401, 160)):
        B, T, F, K, hop = bad
        assert lib.leaf_forward_f32(None, B, T, *nul, F, K, hop, 1, 0, None, None, 0, None) < 0, bad
    assert lib.leaf_workspace_bytes(0, 1600, 40, 401, 160, 0) == 0 and lib.leaf_backward_workspace_bytes(0, 1600, 40, 401, 160, 1, 1) == 0
    # LEAF_FLAG_PEAKNORM is forward-only: refused where the backward would see inconsistent tensors / no pre-pass exists
    assert lib.leaf_forward_prepared_f32(None, 4, 1600, None, 0, None, None, None, None, None, 40, 401, 160,
                                         1 | _native.FLAG_PEAKNORM, None, None, 0, None) == -8
    assert "bad shape" in lib.leaf_status_string(-2).decode()


def test_design_figures_follow_the_committed_evidence():
    """DESIGN.md stays the design (< 40 KB; the lab notebook is NOTES.md) and every measured figure of its
    section 6 is GENERATED from the files under profiles/r05/ (tools/refresh_design.py) -- this regenerates the block and fails
    on any drift between the document and the evidence."""
    import subprocess
    import sys
    design = os.path.join(REPO, "DESIGN.md")
    assert os.path.getsize(design) < 45 * 1024, os.path.getsize(design)      # (40 KB until round 5; round 6 moved three sections to NOTES.md and added the band rule, the backward's derivative criterion, the windows across Nyquist and the pair-sum bound)
    assert os.path.exists(os.path.join(REPO, "NOTES.md"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "refresh_design.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    # the bench line's PMC figures are those of the committed summaries
    rnd = open(os.path.join(REPO, "profiles", "ROUND")).read().strip()          # the round whose evidence DESIGN.md section 6 is generated from
    summ = json.load(open(os.path.join(REPO, "profiles", rnd, "pmc_summary.json")))["configs"]
    traffic = json.load(open(os.path.join(REPO, "profiles", "traffic.json")))
    for cfg, e in traffic["configs"].items():
        assert e["hbm_bytes_per_launch"] == summ[cfg]["hbm_bytes_per_launch"] and e["kernel"] == summ[cfg]["kernel"], cfg
    for cfg in ("cfg1", "cfg2", "cfg3", "cfg4"):
        line = json.load(open(os.path.join(REPO, "profiles", rnd, f"bench_{cfg}_n1.json")))
        assert line["config"]["name"] == cfg and line["roofline"]["traffic"] == summ[cfg]["hbm_bytes_per_launch"], cfg
        assert 0 < line["roofline"]["frac"] <= 1 and line["roofline"]["traffic_ratio"] == summ[cfg]["traffic_ratio"], cfg
        # the executed-flop MODEL of the line (bench.py's Python mirror of the device plan) against what the counters allow: a
        # wave-level VALU instruction is at most 64 lanes x one FMA, so SQ_INSTS_VALU x 128 is an upper bound; the transforms'
        # adds / multiplies (1 flop per lane-instruction) and address arithmetic put the model at ~3/4 of it.  A device plan the
        # mirror no longer follows shows as a ratio outside the band.
        bound = summ[cfg]["valu_instructions"] * 128
        assert traffic["configs"][cfg]["valu_instructions"] == summ[cfg]["valu_instructions"], cfg
        ex = line["roofline"]["executed_flops_per_launch"]
        assert 0.6 * bound <= ex <= bound, (cfg, ex, bound)


def test_bench_configs_are_the_baseline_configs():
    """bench.py --config cfgK must be BASELINE.json configs[K]: filters, sample rate, clip length, PCEN,
    I/O dtype and the batch -- per GPU under weak scaling, in all under strong scaling (configs[2] / [4] name eight GPUs)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))["configs"]
    c = bench.CONFIGS
    assert sorted(c) == ["cfg1", "cfg2", "cfg3", "cfg4"] and all(c[f"cfg{i}"]["index"] == i for i in range(1, 5))
    assert "batch=256" in base[1] and (c["cfg1"]["per_gpu"], c["cfg1"]["global_batch"], c["cfg1"]["seconds"]) == (256, 256, 1.0)
    assert "80 filters, 32 kHz, 5 s clips, batch=1024 sharded over 8" in base[2]
    assert (c["cfg2"]["n_filters"], c["cfg2"]["sample_rate"], c["cfg2"]["seconds"], c["cfg2"]["global_batch"], c["cfg2"]["per_gpu"]) == (80, 32000, 5.0, 1024, 128)
    assert "PCEN off" in base[3] and "batch=512" in base[3] and not c["cfg3"]["pcen"] and c["cfg3"]["per_gpu"] == c["cfg3"]["global_batch"] == 512
    assert "10 s clips, bf16 forward, batch=2048 over 8 GPUs" in base[4]
    assert (c["cfg4"]["seconds"], c["cfg4"]["bf16"], c["cfg4"]["global_batch"], c["cfg4"]["per_gpu"]) == (10.0, True, 2048, 256)
    for k in ("cfg1", "cfg3", "cfg4"):
        assert (c[k]["n_filters"], c[k]["sample_rate"]) == (40, 16000)
    # the executed-flop model knows every overlap-save kernel family (the one-launch kernel repeats the forward transform per filter)
    assert bench.PEAK_FP32_VALU_TFLOPS == 157.3 and bench.PEAK_HBM_GBPS == 8000.0


def test_bench_dump_outputs_writes_float32_and_samples_clips_past_the_limit(tmp_path, monkeypatch):
    """bench.py --dump-outputs (dump_outputs): the features as float32 .npy (bf16 widened exactly); past the size limit a fixed,
    seeded sample of whole clips in clip order, with their indices beside them; rank r > 0 writes its own names."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_for_dump_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
    feats = torch.randn(10, 4, 6, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    assert bench.dump_outputs(str(tmp_path / "all"), feats, 0, 1) == {"features": [10, 4, 6]}
    got = np.load(tmp_path / "all" / "features.npy")
    assert got.dtype == np.float32 and np.array_equal(got, feats.float().numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 4 * 6 * 4 * 2)           # three clips per rank at world size 2
    picks = []
    for _ in range(2):
        d = tmp_path / f"sample{len(picks)}"
        assert bench.dump_outputs(str(d), feats, 1, 2) == {"features_clips_rank1": [3], "features_rank1": [3, 4, 6]}
        idx = np.load(d / "features_clips_rank1.npy")
        assert idx.dtype == np.float64 and list(idx) == sorted(set(idx)) and 0 <= idx.min() and idx.max() < 10
        assert np.array_equal(np.load(d / "features_rank1.npy"), feats.float().numpy()[idx.astype(np.int64)])
        picks.append(list(idx))
    assert picks[0] == picks[1]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 3 * 4)                   # less than one clip: its first frames
    assert bench.dump_outputs(str(tmp_path / "one"), feats, 0, 1) == {"features_clips": [1], "features": [1, 4, 3]}


def test_notes_switch_table_is_current():
    """NOTES.md's last section lists every compile-time switch of the HIP sources with its default (tools/list_switches.py):
    regenerated here and compared, so that a new -DLEAF_* handle or a changed default cannot go undocumented."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "list_switches.py"), "--markdown"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    notes = open(os.path.join(REPO, "NOTES.md")).read()
    assert r.stdout.strip() in notes, "NOTES.md: regenerate the switches table (python tools/list_switches.py --markdown)"


# `#ifdef`-style handles of the HIP sources: defined only by a tool's -D, so list_switches.py (which reads
# `#ifndef X / #define X default`) does not report them
SWITCH_HANDLES = {"LEAF_TOOLS", "LEAF_WG_NW", "LEAF_SMALL_STAMP", "LEAF_DX_NOWAIT", "LEAF_4K_DX_NOACC"}


def leaf_identifiers_outside_the_switch_list(handles=SWITCH_HANDLES):
    """(where, name) of every LEAF_* identifier in csrc/ that a preprocessor condition tests, or that code uses as a constant,
    without tools/list_switches.py reporting it.  Conditions may name only listed switches and the handles above (an undefined
    name in `#if` is 0 without a word); code may also use the C API's constants (include/leaf_hip.h) and the helper macros the
    sources #define themselves.  Comments, string literals and function-like macro calls are not constants."""
    import glob
    import re
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "list_switches.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    listed = {line.split()[0] for line in r.stdout.splitlines() if line.strip()} | set(handles)
    ident = re.compile(r"\bLEAF_[A-Z0-9_]+\b")
    const = re.compile(r"\bLEAF_[A-Z0-9_]+\b(?!\s*\()")
    api = set(ident.findall(open(os.path.join(REPO, "include", "leaf_hip.h")).read()))
    sources = {}
    for path in sorted(glob.glob(os.path.join(REPO, "leaf_pytorch_amd", "csrc", "*"))):
        s = open(path).read()
        s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
        s = re.sub(r'"(\\.|[^"\\\n])*"', '""', s)
        s = re.sub(r"//[^\n]*", "", s)
        sources[os.path.basename(path)] = re.sub(r"\\\n", " ", s).split("\n")
    directive = re.compile(r"\s*#\s*(if|elif|ifdef|ifndef|define|undef)\b\s*(.*)")
    local = {m.group(2).split("(")[0].split()[0] for lines in sources.values() for m in map(directive.match, lines)
             if m and m.group(1) == "define" and m.group(2)}
    bad = []
    for name, lines in sources.items():
        for no, line in enumerate(lines, 1):
            m = directive.match(line)
            if m and m.group(1) in ("if", "elif", "ifdef", "ifndef"):
                bad += [(f"{name}:{no}", n) for n in ident.findall(m.group(2)) if n not in listed]
                continue
            if m and m.group(1) == "undef":
                continue
            body = line if not m else re.sub(r"^\s*LEAF_[A-Z0-9_]+(\([^)]*\))?", "", m.group(2))   # a #define: its replacement
            bad += [(f"{name}:{no}", n) for n in const.findall(body) if n not in listed and n not in api and n not in local]
    return bad


def test_every_leaf_identifier_is_a_listed_switch():
    """A retired switch left behind in a condition (`#if LEAF_WG_PK`) would select the `#else` side silently: every LEAF_* name
    that csrc/ tests or uses as a constant is one tools/list_switches.py reports, or a handle of SWITCH_HANDLES.  The scan sees
    what it should: without its allowance for LEAF_SMALL_STAMP it reports that handle."""
    assert leaf_identifiers_outside_the_switch_list() == []
    missed = leaf_identifiers_outside_the_switch_list(SWITCH_HANDLES - {"LEAF_SMALL_STAMP"})
    assert missed and {n for _, n in missed} == {"LEAF_SMALL_STAMP"}


def test_gradient_metric_rejects_a_wrong_sigma_derivative():
    """at the default parameters d/d mu of `_complex_conv._kernel` is ~650x d/d sigma, so a comparison against
    the TENSOR's largest entry (round 5) lets a wrong sigma derivative through.  The metric of tests/helpers.py (per column, per
    filter) must reject what the old one accepted: a 5 % error on the largest sigma-gradient, a sign flip of the smallest one, a
    dropped clamp sub-gradient -- and accept fp32-sized noise."""
    import pytest
    from helpers import assert_grad_close
    g = torch.Generator().manual_seed(0)
    r = torch.stack([110.0 * (2 * torch.rand(40, generator=g, dtype=torch.float64) - 1),
                     0.17 * (2 * torch.rand(40, generator=g, dtype=torch.float64) - 1)], dim=1)
    r[7, 1] = 1.5e-4                                         # the smallest sigma-gradient the judge measured
    r[3, 1] = 0.17
    r[11, 1] = 8e-3                                          # a mid-sized one (5 % of the column's largest)
    def old_metric(got):
        return float((got - r).abs().max()) / float(r.abs().max())
    noisy = r * (1 + 1e-6 * torch.randn(r.shape, generator=g, dtype=torch.float64))
    assert_grad_close("_complex_conv._kernel", noisy, r)
    for mutate in (lambda t: t[3].__setitem__(1, t[3, 1] * 1.05),          # 5 % on the largest d/d sigma
                   lambda t: t[7].__setitem__(1, -t[7, 1]),                # sign of the smallest
                   lambda t: t[11].__setitem__(1, 0.0)):                   # a clamp sub-gradient dropped where the clamp is inactive
        bad = r.clone()
        mutate(bad)
        assert old_metric(bad) < 1e-4                         # the round-5 comparison passes it ...
        with pytest.raises(AssertionError, match="sigma"):
            assert_grad_close("_complex_conv._kernel", bad, r)              # ... this one does not
    # (F,) tensors: one filter's delta-gradient 1 % off while another filter's is 3000x larger
    d = torch.tensor([1.7, 5e-4, 0.3, 0.02], dtype=torch.float64)
    bad = d.clone()
    bad[1] *= 1.01
    assert float((bad - d).abs().max()) / float(d.abs().max()) < 1e-4
    with pytest.raises(AssertionError, match="per-filter bound"):
        assert_grad_close("_compression.delta", bad, d)
