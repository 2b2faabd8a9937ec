#!/usr/bin/env python3
"""Fixture for the host dispatch: what the plan / size queries of the C ABI answer over a grid that crosses every threshold.

    python tests/golden/make_golden_plan_table.py            # rewrites tests/golden/plan_table.json from the built library
    python tests/golden/make_golden_plan_table.py --check    # recomputes in memory and compares

The queries are pure host functions (status codes and sizes; nothing is launched), so the table is taken without a GPU.  It pins
the dispatch decisions of the commit it was taken on: regenerate it ONLY when a decision is meant to change, never to make a
refactor pass.  The answers depend on the device's CU count (256 without a visible device, which is also an MI355X's count);
the fixture records the count it was taken with.  The fixture holds the grid AND the answers: tests/test_host_plan_table.py
replays it with `replay()` below and needs nothing else from this file."""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
OUT = os.path.join(HERE, "plan_table.json")

# (K, hop): the three static geometries, then run-time geometries odd and even, across the 224-tap, 833-tap and 1217-tap thresholds
GEOMETRIES = [(401, 160), (801, 320), (201, 80), (552, 220), (1103, 441), (1201, 480), (2049, 800), (223, 89), (224, 90), (64, 25)]
BATCHES_ALL = [0, 1, 4, 7, 8, 11, 12, 24, 111, 112, 113, 256]      # 112 blocks: where AUTO takes the workgroup kernels (7/16 per CU)
FILTERS_ALL = [1, 40, 80, 300]                                       # 300 > kBandMaxFilters
SELECTORS = [0, 1, 2, 3, 4, 5, 9]                                    # 9: invalid
RESERVE = [0, 8 << 16, 200 << 16]                                    # LEAF_ALGO_RESERVE_CUS(k)
OPTION_BITS = [1 << 25, 1 << 26, 1 << 27]                            # STREAM_FINALIZE, FULL_TRANSFORMS, STRICT_BAND_CLASSES
PCEN, IO_BF16, BWD_STAGED, BWD_MFMA, BWD_FULL, X_PCM16, OUT_BF16 = 0x1, 0x4, 0x8, 0x10, 0x40, 0x100, 0x200
BWD_FLAGS = [0, PCEN | BWD_FULL | OUT_BF16, BWD_STAGED, BWD_MFMA, IO_BF16, X_PCM16, BWD_MFMA | IO_BF16, BWD_STAGED | X_PCM16]


def block_len(K):
    """samples an overlap-save block advances by: 2048-point blocks up to 1217 taps, 4096-point blocks beyond"""
    return 2048 - K + 1 if K <= 1217 else (4096 - K + 1) & ~1


def clip_lengths(K, hop):
    L = block_len(K)
    return [1, 159, L - 1, L, L + 1, 500 * hop]                          # one block +- 1; 500 frames: 5 s


def sized_shapes(K, hop):
    """The size queries answer ~120 questions per shape, so they see every value of each axis, not the full cross: every batch at a
    1 s clip (ten 2048-sample blocks: 11 / 12 clips straddle the 112-block threshold), every clip length at one clip and at 112,
    every filter count at 1 and 12 clips."""
    Ts, sec = clip_lengths(K, hop), 100 * hop
    shapes = [(B, sec, 40) for B in BATCHES_ALL] + [(B, T, 40) for B in (1, 112) for T in Ts] + \
             [(B, sec, F) for B in (1, 12) for F in FILTERS_ALL if F != 40]
    return [[B, T, F, K, hop] for B, T, F in shapes]


def grid():
    return {
        "geometries": [list(g) for g in GEOMETRIES],
        "auto": {"B": BATCHES_ALL, "F": FILTERS_ALL, "T": {f"{K}/{hop}": clip_lengths(K, hop) for K, hop in GEOMETRIES}},
        "sized": [s for K, hop in GEOMETRIES for s in sized_shapes(K, hop)],
        "selectors": SELECTORS,
        "options": RESERVE + OPTION_BITS,                      # every selector is crossed with every option
        "bwd_flags": BWD_FLAGS,
        "stages": [0, 1, 2, 3, 4, 5],
    }


def _auto_shapes(g):
    for K, hop in g["geometries"]:
        for B in g["auto"]["B"]:
            for T in g["auto"]["T"][f"{K}/{hop}"]:
                for F in g["auto"]["F"]:
                    yield B, T, F, K, hop


def rle(values):
    """runs of equal answers as [value, count]; a single answer as itself (the fixture stays small enough to read and to diff)"""
    out = []
    for v in values:
        if out and isinstance(out[-1], list) and len(out[-1]) == 2 and isinstance(out[-1][1], int) and out[-1][0] == v and not isinstance(v, list):
            out[-1][1] += 1
        elif out and out[-1] == v and not isinstance(v, list):
            out[-1] = [v, 2]
        else:
            out.append(v)
    return out


def replay(lib, g):
    """every answer of the grid `g`, in the order the fixture stores them"""
    info = (ctypes.c_int * 8)()
    out = {"auto_algo": [], "fft_plan_info": [], "workspace_bytes": [], "forward_mix_workspace_bytes": [],
           "backward_workspace_bytes": [], "backward_mix_workspace_bytes": [], "fft_tables_bytes": [],
           "stage_backward_workspace_bytes": []}
    for s in _auto_shapes(g):
        out["auto_algo"].append(lib.leaf_auto_algo(*s))
    for s in g["sized"]:
        rc = lib.leaf_fft_plan_info(*s, info)
        out["fft_plan_info"].append(list(info) if rc == 0 else rc)
        for sel in g["selectors"]:
            for opt in g["options"]:
                out["workspace_bytes"].append(lib.leaf_workspace_bytes(*s, sel | opt))
            for opt in g["options"]:
                out["forward_mix_workspace_bytes"].append(lib.leaf_forward_mix_workspace_bytes(*s, sel | opt))
        for need_dx in (0, 1):
            for flags in g["bwd_flags"]:
                out["backward_workspace_bytes"].append(lib.leaf_backward_workspace_bytes(*s, flags, need_dx))
        for flags in g["bwd_flags"]:
            out["backward_mix_workspace_bytes"].append(lib.leaf_backward_mix_workspace_bytes(*s, flags))
        B, T, F, K, hop = s
        for stage in g["stages"]:
            out["stage_backward_workspace_bytes"].append(lib.leaf_stage_backward_workspace_bytes(stage, B, T, F, K, hop))
    for K, hop in g["geometries"]:
        for F in g["auto"]["F"] + [0]:
            out["fft_tables_bytes"].append(lib.leaf_fft_tables_bytes(F, K, hop))
    return {k: v if k == "fft_plan_info" else rle(v) for k, v in out.items()}


def device_cus():
    """the count the library sizes its grids for: the visible device's, 256 without one"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def n_answers(answers):
    return sum(v[1] if isinstance(v, list) and k != "fft_plan_info" else 1 for k, vs in answers.items() for v in vs)


def generate():
    from leaf_pytorch_amd import _native
    if os.environ.get("LEAF_PLAN_TABLE_LIB"):                # another build of the library (the commit the table is to pin)
        _native.LIB_PATH = os.path.abspath(os.environ["LEAF_PLAN_TABLE_LIB"])
    g = grid()
    return {"cus": device_cus(), "grid": g, "answers": replay(_native.load(), g)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    table = generate()
    if args.check:
        with open(OUT) as fh:
            assert json.load(fh) == table, "plan_table.json differs from what the built library answers"
        print("plan_table.json matches")
        return
    with open(OUT, "w") as fh:
        fh.write("{\n")
        fh.write(f' "cus": {table["cus"]},\n "grid": {json.dumps(table["grid"], separators=(",", ":"))},\n "answers": {{\n')
        fh.write(",\n".join(f'  "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in table["answers"].items()))
        fh.write("\n }\n}\n")
    print(f"wrote {OUT}: {n_answers(table['answers'])} answers, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
