#!/usr/bin/env python3
"""Host cost of the ctypes wrappers (leaf_forward, leaf_backward, leaf_forward_mix) of this checkout against another ``_native.py``.

No GPU and no launch: CPU tensors, ``require_hip`` / the device guard / ``stream_ptr`` set aside, and a stand-in library whose
stream-taking entries return 0 (the host-only size queries go to the real library).  The two files alternate, ``--repeats`` times
``--calls`` calls each; the bound of profiles/native_binding_refactor.txt is "this checkout's median within the other's spread".

    git show <commit>:leaf_pytorch_amd/_native.py > /tmp/other_native.py
    taskset -c 3 python tools/native_host_cost.py --other /tmp/other_native.py [--parameters]"""
import argparse
import contextlib
import os
import statistics
import sys
import time
import types
from unittest import mock

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from leaf_pytorch_amd import _native as new  # noqa: E402


class _Lib:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.endswith("_bytes") or name in ("leaf_num_frames", "leaf_auto_algo", "leaf_status_string"):
            return getattr(self._real, name)
        return lambda *a: 0


@contextlib.contextmanager
def stubbed(native):
    lib = _Lib(native.load())
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(native, "require_hip", lambda x, who: None))
        st.enter_context(mock.patch.object(native, "stream_ptr", lambda device: None))
        st.enter_context(mock.patch.object(native, "load", lambda: lib))
        st.enter_context(mock.patch.object(torch.cuda, "device", lambda device: contextlib.nullcontext()))
        yield


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="a _native.py of another commit")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--parameters", action="store_true", help="the seven parameters as nn.Parameter under no_grad, as Leaf hands them over")
    a = ap.parse_args()
    old = types.ModuleType("leaf_pytorch_amd._native")
    old.__file__, old.__package__ = new.__file__, "leaf_pytorch_amd"
    exec(compile(open(a.other).read(), a.other, "exec"), old.__dict__)
    torch.set_num_threads(1)
    torch.set_grad_enabled(False)
    B, T, F, K, hop = 2, 2400, 40, 401, 160
    x, go = torch.zeros(B, 1, T), torch.zeros(B, F, 15)
    prm = [torch.zeros(F, 2), torch.zeros(1, 1, F, 1), torch.zeros(F)] + [torch.ones(F) for _ in range(4)]
    if a.parameters:
        prm = [torch.nn.Parameter(p) for p in prm]
    perm, lam = torch.tensor([1, 0], dtype=torch.int32), torch.tensor([0.25, 0.5])
    calls = {"leaf_forward": lambda n: n.leaf_forward(x, *prm, K, hop),
             "leaf_backward": lambda n: n.leaf_backward(x, *prm, K, hop, go),
             "leaf_forward_mix": lambda n: n.leaf_forward_mix(x, perm, lam, *prm, K, hop)}
    for name, fn in calls.items():
        us = {"other": [], "this": []}
        for r in range(a.repeats + 1):                       # (the first round warms up)
            for tag, native in (("other", old), ("this", new))[::1 if r % 2 == 0 else -1]:
                with stubbed(native):
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn(native)
                    dt = (time.perf_counter() - t0) / a.calls * 1e6
                if r:
                    us[tag].append(dt)
        o, n = sorted(us["other"]), sorted(us["this"])
        med = statistics.median(n)
        print(f"{name:18s} other {' '.join(f'{v:.2f}' for v in o)}   median {statistics.median(o):.2f}")
        print(f"{'':18s} this  {' '.join(f'{v:.2f}' for v in n)}   median {med:.2f}   "
              f"{'within' if o[0] <= med <= o[-1] else 'below' if med < o[0] else 'ABOVE'} the other's spread")


if __name__ == "__main__":
    main()
