#!/usr/bin/env python3
"""Records tests/golden/tail_rows/<name>.npz: the outputs of the cases tests/tail_rows_cases.py lists under GOLDEN, from the library
that is built in the tree.  They were recorded on an MI355X from the commit BEFORE the row-owned tail (the tile finalize in the
workgroup kernel's tail) and are held exactly by tests/test_gpu_tail_rows.py: run this only from a commit whose bits are the reference.

    python tests/golden/make_golden_tail_rows.py [output directory]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import tail_rows_cases as C  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tail_rows")
    os.makedirs(out_dir, exist_ok=True)
    for name, sr, F, tp, B, G, mode in C.GOLDEN:
        K, hop = C.GEOMETRY[sr]
        x, params = C.inputs(F, K, hop, tp, B, mode, C.golden_seed(name))
        out, raw = C.forward(x, params, K, hop, mode, C.N.ALGO_FFT_WG | C.grid_bits(G))
        arrays = {"out": out.view(torch.int16).numpy() if out.dtype == torch.bfloat16 else out.numpy()}
        if raw is not None:
            arrays["raw"] = raw.numpy()
        np.savez(os.path.join(out_dir, name + ".npz"), **arrays)
        print(f"{name}: out {tuple(out.shape)} {out.dtype}, finite {bool(torch.isfinite(out.float()).all())}")


if __name__ == "__main__":
    main()
