"""CPU-only: the host dispatch answers what tests/golden/plan_table.json recorded (tests/golden/make_golden_plan_table.py).

The plan makers, the selector resolution and the workspace sizes are pure host functions: this replays a few thousand
queries across every threshold they have (batch, window, clip length, filter count, selector, option bits, backward flags)
and compares status codes and sizes.  Nothing is launched."""
import importlib.util
import json
import os

import pytest
import torch

from leaf_pytorch_amd import _native
from conftest import GOLDEN_DIR


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_plan_table", os.path.join(GOLDEN_DIR, "make_golden_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_plan_table_matches_the_recorded_dispatch():
    gen = _generator()
    with open(os.path.join(GOLDEN_DIR, "plan_table.json")) as fh:
        table = json.load(fh)
    if torch.cuda.is_available() and gen.device_cus() != table["cus"]:
        pytest.skip(f"the table was recorded for {table['cus']} CUs, this device has {gen.device_cus()}: the plans follow the CU count")
    got = gen.replay(_native.load(), table["grid"])
    assert sorted(got) == sorted(table["answers"])
    assert gen.n_answers(got) > 3000
    for name, want in table["answers"].items():
        assert len(got[name]) == len(want), name
        diff = [(i, w, g) for i, (w, g) in enumerate(zip(want, got[name])) if w != g]
        assert not diff, f"{name}: {len(diff)} of {len(want)} answers changed; first (index, recorded, now): {diff[:5]}"
