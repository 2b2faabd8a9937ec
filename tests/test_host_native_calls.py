"""CPU-only: the Python host layer asks of the C ABI what tests/golden/native_calls.json recorded (tests/golden/make_golden_native_calls.py).

The wrappers of ``_native`` and the ctypes route of ``Leaf.forward`` / ``Leaf.forward_mixup`` are driven with CPU tensors against a
recording stand-in for the library: the entry reached, every integer and float argument, the tensor behind every pointer (role, dtype,
shape, contiguity, offset), what the call returned and every refusal's text must equal the record.  Nothing is launched."""
import importlib.util
import json
import os

import pytest
import torch

from leaf_pytorch_amd import _native
from conftest import GOLDEN_DIR


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load("make_golden_native_calls")


@pytest.fixture(scope="module")
def table():
    t = gen.load_table()
    assert t["small_limit"] == gen.SMALL_LIMIT
    return t["cases"]


@pytest.fixture(scope="module")
def replayed():
    return json.loads(json.dumps(gen.replay(_native)))       # (tuples -> lists, as the table was written)


def _skip_if_other_cus():
    plan = _load("make_golden_plan_table")
    with open(os.path.join(GOLDEN_DIR, "plan_table.json")) as fh:
        cus = json.load(fh)["cus"]
    if torch.cuda.is_available() and plan.device_cus() != cus:
        pytest.skip(f"the workspace sizes in the table are those of {cus} CUs, this device has {plan.device_cus()}")


def test_every_recorded_case_is_replayed(table, replayed):
    assert sorted(replayed) == sorted(table)
    assert len(table) > 500 and sum(len(r["calls"]) for r in table.values()) > 300


@pytest.mark.parametrize("group", ["forward", "forward_mix", "forward-out", "backward", "backward_mix", "profiled", "prepared", "sliced", "stage",
                                   "frontend"])
def test_host_layer_makes_the_recorded_calls(group, table, replayed):
    _skip_if_other_cus()
    names = [n for n in table if n.split("/")[0] == group and n not in gen.CHANGED_ON_PURPOSE]
    assert names
    diff = [(n, table[n], replayed[n]) for n in names if table[n] != replayed[n]]
    assert not diff, f"{len(diff)} of {len(names)} cases changed; first (case, recorded, now): {diff[0]}"


CLIP_CASES = ("sliced/forward/clip-beyond-one-call", "sliced/backward/clip-beyond-one-call", "sliced/batch_slices/clip-beyond-one-call")
# what one unpacker and one gatherer for every wrapper changed: case -> (what the parent did, the refusal now)
SHARED_PIECE_CASES = {
    "backward/bad-alpha-dtype": ("pcen param must be float32, got torch.float64", "alpha must be float32, got torch.float64"),
    "backward_mix/bad-alpha-dtype": ("pcen param must be float32, got torch.float64", "alpha must be float32, got torch.float64"),
    "profiled/bad-alpha-dtype": ("pcen param must be float32, got torch.float64", "alpha must be float32, got torch.float64"),
    "prepared/bad-alpha-dtype": ("pcen param must be float32, got torch.float64", "alpha must be float32, got torch.float64"),
    "backward/two-channels": (None, "expected input of shape (B,1,T), got (2, 2, 2400)"),       # (the parent took channel 0)
    "profiled/two-channels": (None, "expected input of shape (B,1,T), got (2, 2, 2400)"),
    "backward/bad-alpha-and-grad_out": ("grad_out must be float32, got torch.float64", "alpha must be float32, got torch.float64"),
    "forward-out/bad-alpha-and-out/auto-staged": ("out must be a contiguous (2, 17, 43) tensor on cpu matching the input dtype (float32; "
                                                  "bfloat16 for bfloat16 x)", "alpha must be float32, got torch.float64"),
}


def test_the_intended_differences_are_these_and_no_others(table, replayed):
    assert set(gen.CHANGED_ON_PURPOSE) == set(CLIP_CASES) | set(SHARED_PIECE_CASES)
    # a single clip of T >= 2^31 samples recursed until RecursionError (batch_slices handed the clip back as its own slice); it is
    # refused with the sentence csrc/torch_binding.cpp uses
    assert table["sliced/forward/clip-beyond-one-call"]["raises"] == table["sliced/backward/clip-beyond-one-call"]["raises"] == "RecursionError"
    for name in CLIP_CASES:
        now = replayed[name]
        assert now["calls"] == [] and now["raises"] == "RuntimeError", name
        assert now["message"] == "a clip of 6000 samples is beyond the C ABI's 32-bit sample index", name
    with pytest.raises(RuntimeError, match="a clip of 2147483648 samples is beyond the C ABI's 32-bit sample index"):
        _native.batch_slices(1, 1 << 31)
    assert _native.batch_slices(1, (1 << 31) - 1) == [(0, 1)] and _native.CALL_SAMPLES == 1 << 31
    for name, (before, after) in SHARED_PIECE_CASES.items():
        assert table[name].get("message") == before and (before is not None or len(table[name]["calls"]) == 1), name
        now = replayed[name]
        assert now["calls"] == [] and now["raises"] == "RuntimeError" and now["message"] == after, (name, now)


def test_frontend_cases_cover_the_ctypes_autograd_route(table):
    """What the second half of the table must hold: both calls, under no_grad and in training with a given grad_out, reach the entries
    with the flags recorded; x.grad of a plain float32 call has x's shape; a mixed call refuses x.requires_grad in today's words."""
    entries = lambda n: [c.split("(")[0] for c in table[n]["calls"]]
    assert entries("frontend/forward/no_grad/default/f32") == ["leaf_forward_f32"]
    assert entries("frontend/forward/train/default/f32") == ["leaf_forward_save_f32", "leaf_backward_f32"]
    assert entries("frontend/forward_mixup/no_grad/default/i16") == ["leaf_forward_mix_f32"]
    assert entries("frontend/forward_mixup/train/default/i16") == ["leaf_forward_save_mix_f32", "leaf_backward_mix_f32"]
    assert entries("frontend/forward/no_grad/cache-tables") == ["leaf_fft_prepare_tables_f32", "leaf_forward_prepared_f32"]
    r = table["frontend/forward/x-requires-grad"]
    assert r["returns"][1] == "f32[3,1,2400]" and r["calls"][1].split(", ")[-4] == "ret1:f32[3,2400]"     # g_x is x.grad
    assert table["frontend/forward/train/default/f32"]["returns"][1] is None
    r = table["frontend/forward_mixup/x-requires-grad"]
    assert r["raises"] == "RuntimeError" and r["message"].startswith("Leaf.forward_mixup: x.requires_grad is not supported") and not r["calls"]
