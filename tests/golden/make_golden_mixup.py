#!/usr/bin/env python3
"""Fixture for waveform mixup, recorded from the reference's own ``do_mixup`` (utilities/data/mixup.py).

    python tests/golden/make_golden_mixup.py            # rewrites tests/golden/mixup/mixup_b6.npz (a directory of its own: every .npz directly under tests/golden/ is a frontend fixture)
    python tests/golden/make_golden_mixup.py --check    # regenerates in memory and compares bit for bit

Run where the reference checkout exists (LEAF_REFERENCE, default /root/reference); the tests only read the .npz.  The fixture is
data only: inputs (6,1,64) float32, multilabel targets (6,5), what do_mixup returned for them (mixed_x, mixed_y), and the two
random draws it made -- ``lam`` (numpy RandomState(random_seed).beta, recovered by re-seeding) and ``perm`` (torch.randperm,
recovered by re-seeding torch's generator to the state do_mixup saw).  Amplitudes stay where no product is subnormal."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LEAF_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "mixup", "mixup_b6.npz")
SEED, B, T, CLASSES, ALPHA, RANDOM_SEED = 20260, 6, 64, 5, 1.0, 1233


def generate():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_mixup", os.path.join(REF, "utilities", "data", "mixup.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = torch.Generator().manual_seed(SEED)
    x = (2 * torch.rand(B, 1, T, generator=g) - 1) * 0.9
    x[x.abs() < 1e-3] = 0.25                                 # no product near the subnormal range
    y = (torch.rand(B, CLASSES, generator=g) < 0.4).float()
    torch.manual_seed(SEED + 1)                              # the global generator do_mixup's randperm draws from
    mixed_x, mixed_y, _, _ = ref.do_mixup(x, y, alpha=ALPHA, random_seed=RANDOM_SEED, mode="multilabel")
    torch.manual_seed(SEED + 1)
    perm = torch.randperm(B)
    lam = torch.from_numpy(np.random.RandomState(RANDOM_SEED).beta(ALPHA, ALPHA, B)).float()
    assert torch.equal(mixed_x, x * lam.view(B, 1, 1) + x[perm] * (1 - lam.view(B, 1, 1))), "recovered draws do not reproduce do_mixup"
    return {"x": x.numpy(), "y": y.numpy(), "perm": perm.numpy().astype(np.int64), "lam": lam.numpy(), "mixed_x": mixed_x.numpy(),
            "mixed_y": mixed_y.numpy(), "alpha": np.float64(ALPHA), "random_seed": np.int64(RANDOM_SEED),
            "torch_seed": np.int64(SEED + 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixture bit for bit")
    args = ap.parse_args()
    data = generate()
    if args.check:
        old = np.load(OUT)
        bad = [k for k in data if k not in old or not np.array_equal(np.asarray(data[k]), old[k])]
        if bad or set(old.files) != set(data):
            sys.exit(f"mixup_b6.npz differs from the reference's output: {bad}")
        print("mixup_b6.npz: identical")
        return
    np.savez(OUT, **data)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
