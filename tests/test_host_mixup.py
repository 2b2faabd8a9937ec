"""Host-side contract of waveform mixup (the leaf_*_mix_f32 entries, ``Leaf.forward_mixup``, ``transforms.Mixup``): what the header
declares and the library exports, the refusals that answer before any launch (dummy host pointers: no GPU is needed), the Python
layers' argument checks, and the fp32 definition of a mixed sample against the reference's own ``do_mixup`` on a committed fixture."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from leaf_pytorch_amd import Leaf, _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "mixup", "mixup_b6.npz")
ENTRIES = ("leaf_mixup_f32", "leaf_forward_mix_workspace_bytes", "leaf_forward_mix_f32", "leaf_forward_save_mix_f32",
           "leaf_backward_mix_workspace_bytes", "leaf_backward_mix_f32")
B, T, F, K, HOP = 2, 2400, 40, 401, 160


def mix_definition(x, perm, lam):
    """The definition in include/leaf_hip.h, in torch fp32 (eager ops round separately: no fused multiply-add)."""
    lam = lam.to(torch.float32).view(-1, *([1] * (x.dim() - 1)))
    om = 1 - lam
    return x * lam + x[perm.long()] * om


def _even():
    host = (ctypes.c_char * 4096)()
    base = ctypes.addressof(host)
    return host, ctypes.c_void_p(base + (-base) % 64)


def test_header_declares_the_entries_and_the_abi_version_stays():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\(", header), name
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _native.ABI_VERSION == 6 and _native.load().leaf_abi_version() == 6


def test_library_exports_the_entries_and_ctypes_knows_their_signatures():
    lib = _native.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ENTRIES:
        assert name in exported, name
        assert name in _native._SIGNATURES and name in _native.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes == _native._SIGNATURES[name][1] and fn.restype == _native._SIGNATURES[name][0]
    # header and exported symbols stay equal: everything the header declares is registered, and the other way round
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char\*)\s+(leaf_\w+)\(", header, flags=re.M))
    assert declared == set(_native._SIGNATURES)
    assert {s for s in exported if s.startswith("leaf_")} >= declared


def test_workspace_queries_answer_for_the_new_entries():
    lib = _native.load()
    # a selector that mixes in its loads needs nothing more; one that does not adds the mixed fp32 copy
    wg, fft, mfma = _native.ALGO_FFT_WG, _native.ALGO_FFT, _native.ALGO_MFMA
    for algo in (wg, fft):                                     # static 16 kHz geometry: workgroup and per-wave kernels mix in their loads
        assert lib.leaf_forward_mix_workspace_bytes(5, 4001, F, K, HOP, algo) == lib.leaf_workspace_bytes(5, 4001, F, K, HOP, algo) > 0
    extra = lib.leaf_forward_mix_workspace_bytes(5, 4001, F, K, HOP, mfma) - lib.leaf_workspace_bytes(5, 4001, F, K, HOP, mfma)
    assert 5 * 4001 * 4 <= extra <= 5 * 4001 * 4 + 2 * 256
    pc = _native.FLAG_PCEN
    # backward: nothing extra on the static overlap-save paths and the 4096-sample plan; the copy on run-time geometry, MFMA, staged
    for (b, t, f, k, h) in ((5, 4001, F, K, HOP), (300, 16000, F, K, HOP), (64, 7000, 12, 801, 320), (64, 7000, 6, 833, 333)):
        assert lib.leaf_backward_mix_workspace_bytes(b, t, f, k, h, pc) == lib.leaf_backward_workspace_bytes(b, t, f, k, h, pc, 0) > 0
    for (b, t, f, k, h, fl) in ((5, 4001, 12, 552, 220, pc), (5, 4001, F, K, HOP, pc | _native.FLAG_BWD_MFMA), (3, 1501, 8, K, HOP, pc | _native.FLAG_BWD_STAGED)):
        assert lib.leaf_backward_mix_workspace_bytes(b, t, f, k, h, fl) >= lib.leaf_backward_workspace_bytes(b, t, f, k, h, fl, 0) + b * t * 4
    assert lib.leaf_forward_mix_workspace_bytes(0, 4001, F, K, HOP, wg) == 0            # the empty batch, as the plain queries


def test_unsupported_combinations_are_refused_before_anything_else():
    lib = _native.load()
    keep, p = _even()
    fwd = lambda flags: lib.leaf_forward_mix_f32(p, p, p, B, T, p, p, p, p, p, p, p, F, K, HOP, flags, 0, p, p, 0, None)
    save = lambda flags: lib.leaf_forward_save_mix_f32(p, p, p, B, T, p, p, p, p, p, p, p, F, K, HOP, flags, 0, p, p, p, 0, None)
    bwd = lambda flags, gx=None: lib.leaf_backward_mix_f32(p, p, p, B, T, p, p, p, p, p, p, p, F, K, HOP, flags, p, None, p, p, p, p, p, p,
                                                          p, gx, p, 0, None)
    pc = _native.FLAG_PCEN
    for call in (fwd, save, bwd):
        assert call(pc | _native.FLAG_IO_BF16) == -8
        assert call(pc | _native.FLAG_PEAKNORM) == -8
        assert call(pc) == -3                                  # accepted: the 0-byte workspace is what is refused next
        assert call(pc | _native.FLAG_X_PCM16) == -3
    assert bwd(pc, gx=p) == -8                                 # dL/dx under mixup: not built
    assert lib.leaf_forward_mix_f32(p, None, p, B, T, p, p, p, p, p, p, p, F, K, HOP, pc, 0, p, p, 0, None) == -1
    assert lib.leaf_forward_mix_f32(p, p, None, B, T, p, p, p, p, p, p, p, F, K, HOP, pc, 0, p, p, 0, None) == -1
    assert lib.leaf_mixup_f32(p, B, T, p, p, _native.FLAG_IO_BF16, p, None) == -8
    assert lib.leaf_mixup_f32(p, B, T, None, p, 0, p, None) == -1
    assert "mixup" in lib.leaf_status_string(-8).decode()


def test_forward_mixup_on_a_cpu_tensor_raises_like_forward():
    m = Leaf()
    x = torch.zeros(2, 1, 800)
    with pytest.raises(RuntimeError) as plain:
        m(x)
    with pytest.raises(RuntimeError) as mixed:
        m.forward_mixup(x, [1, 0], torch.tensor([0.5, 0.5]))
    assert "runs only on an AMD GPU" in str(plain.value) and "runs only on an AMD GPU" in str(mixed.value)


def test_a_cpu_perm_with_an_index_out_of_range_raises_value_error():
    dev = torch.device("cpu")                      # mix_args only places tensors: no launch, so the CPU serves as "the device" here
    lam = torch.tensor([0.3, 0.7, 0.5])
    for bad in ([0, 1, 3], [-1, 0, 1], torch.tensor([2, 2, 5])):
        with pytest.raises(ValueError, match="outside"):
            _native.mix_args(bad, lam, 3, dev)
    with pytest.raises(ValueError):
        _native.mix_args([0, 1], lam, 3, dev)                                  # one entry per clip
    with pytest.raises(TypeError):
        _native.mix_args(torch.tensor([0.0, 1.0, 2.0]), lam, 3, dev)
    perm, lam32 = _native.mix_args(torch.tensor([2, 0, 1], dtype=torch.int64), lam, 3, dev)
    assert perm.dtype == torch.int32 and perm.tolist() == [2, 0, 1] and lam32.dtype == torch.float32


def test_the_definition_reproduces_the_reference_fixture_bit_for_bit():
    d = np.load(FIXTURE)
    x, perm, lam = torch.from_numpy(d["x"]), torch.from_numpy(d["perm"]), torch.from_numpy(d["lam"])
    assert x.shape == (6, 1, 64) and sorted(perm.tolist()) == list(range(6))
    assert torch.equal(mix_definition(x, perm, lam), torch.from_numpy(d["mixed_x"]))
    # the same three roundings spelled out per sample in numpy float32 (no expression-level fusion possible)
    xn, ln = d["x"], d["lam"].astype(np.float32)
    om = (np.float32(1) - ln).astype(np.float32)
    want = ((xn * ln[:, None, None]).astype(np.float32) + (xn[d["perm"]] * om[:, None, None]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(want, d["mixed_x"])
    y = torch.from_numpy(d["y"])
    assert torch.equal(y * lam.view(6, 1) + y[perm] * (1 - lam.view(6, 1)), torch.from_numpy(d["mixed_y"]))
    # the draws are the reference's: Beta(alpha, alpha) from numpy's RandomState(random_seed)
    again = torch.from_numpy(np.random.RandomState(int(d["random_seed"])).beta(float(d["alpha"]), float(d["alpha"]), 6)).float()
    assert torch.equal(again, lam)


@pytest.mark.skipif(not os.path.isdir(os.environ.get("LEAF_REFERENCE", "/root/reference")), reason="the reference checkout is not on this machine")
def test_fixture_recipe_reproduces_the_committed_fixture():
    r = subprocess.run([os.sys.executable, os.path.join(REPO, "tests", "golden", "make_golden_mixup.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
