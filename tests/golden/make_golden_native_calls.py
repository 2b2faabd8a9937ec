"""Records what the Python host layer (leaf_pytorch_amd/_native.py, frontend.py) asks of the C ABI: tests/golden/native_calls.json.

No GPU: the wrappers are driven with CPU tensors.  ``require_hip``, the device guard and ``stream_ptr`` are set aside, and the loaded
library is replaced by a recording stand-in: host-only queries (``leaf_num_frames``, the ``*_bytes`` functions, ``leaf_auto_algo``,
``leaf_fft_plan_info``) are forwarded to the real library, every entry that takes a stream is NOT called -- it is recorded and
answered with 0.  A record holds the entry's name, every integer and float argument, and for every pointer argument None or the
tensor it points into: which input by name, ``ret<i>`` for the i-th returned tensor, ``tmp`` for anything else the wrapper
allocated (workspace, contiguous or widened copies), with dtype, shape, contiguity and the byte offset into it (``Recorder.finish``).
A case also records what the wrapper returned (dtype and shape of each element) or the exception it raised.

    python tests/golden/make_golden_native_calls.py --commit <the commit checked out>

writes the table from the checked-out package.  tests/test_host_native_calls.py replays ``cases()`` through the checked-out code and
demands equality record for record, except for ``CHANGED_ON_PURPOSE``.  The committed table was recorded once from the commit before
the host layer was refactored (profiles/native_binding_refactor.txt says how).  The "sliced" cases lower ``_native.CALL_SAMPLES``, the
sample limit of one C-ABI call, to ``SMALL_LIMIT``, here and in the test alike."""
import argparse
import contextlib
import ctypes
import importlib
import json
import os
import sys
from unittest import mock

import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_leaves

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "native_calls.json")
SMALL_LIMIT = 5000                      # stands in for 2^31 samples per C-ABI call in the "sliced" cases
HOST_ONLY = ("leaf_abi_version", "leaf_status_string", "leaf_num_frames", "leaf_auto_algo", "leaf_fft_plan_info", "leaf_stream_history_samples")
# the intended differences to the recorded table: a single clip beyond one C-ABI call used to recurse until RecursionError; and what one
# unpacker and one gatherer for every wrapper changed (see _native_cases)
CHANGED_ON_PURPOSE = ("sliced/forward/clip-beyond-one-call", "sliced/backward/clip-beyond-one-call", "sliced/batch_slices/clip-beyond-one-call",
                      "backward/bad-alpha-dtype", "backward_mix/bad-alpha-dtype", "profiled/bad-alpha-dtype", "prepared/bad-alpha-dtype",
                      "backward/two-channels", "profiled/two-channels", "backward/bad-alpha-and-grad_out",
                      "forward-out/bad-alpha-and-out/auto-staged")


class Recorder(TorchDispatchMode):
    """Remembers every tensor allocated while a case runs (so that a pointer can be traced back to one) and every C-ABI call."""

    def __init__(self):
        super().__init__()
        self.calls, self.allocs, self.names = [], {}, {}

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in tree_leaves(out):
            if isinstance(t, torch.Tensor) and t.device.type == "cpu":
                self.allocs.setdefault(t.untyped_storage().data_ptr(), t)      # (kept alive: no address is used twice)
        return out

    def name(self, **tensors):
        for n, t in tensors.items():
            if t is not None and t.device.type == "cpu" and t.untyped_storage().data_ptr():
                base = t.untyped_storage().data_ptr()
                self.allocs[base], self.names[base] = t, n
        return tuple(tensors.values())

    def describe(self, a):
        if isinstance(a, ctypes.c_void_p):
            a = a.value
            if a is None:
                return None
            for base, t in self.allocs.items():
                if base and base <= a < base + max(t.untyped_storage().nbytes(), 1):
                    return {"of": base, "dtype": str(t.dtype), "shape": list(t.shape), "contig": t.is_contiguous(), "off": a - base}
            return {"of": "unknown", "dtype": "torch.?", "shape": [], "contig": True, "off": a}
        if isinstance(a, ctypes.Array):
            return f"{type(a)._type_.__name__}[{len(a)}]"
        if isinstance(a, bool):
            return int(a)
        assert a is None or isinstance(a, (int, float, str)), type(a)
        return a

    def finish(self, ret):
        """Pointer descriptions get their role: an input's name, ret<i>, or tmp."""
        elems = ret if isinstance(ret, (tuple, list)) else (ret,)
        rets = {t.untyped_storage().data_ptr(): f"ret{i}" for i, t in enumerate(elems) if isinstance(t, torch.Tensor) and t.device.type == "cpu"}
        for _, args in self.calls:
            for d in args:
                if isinstance(d, dict) and isinstance(d["of"], int):
                    d["of"] = self.names.get(d["of"]) or rets.get(d["of"]) or "tmp"
        # a named input is described once per case ("in": {"x": "i16[5,1,2400]"}; a trailing "s": strided) and a pointer into it is its
        # name, plus the byte offset where there is one ("x+9600"); any other tensor is described in place ("ret0:f32[2,40,15]")
        legend = {}

        def short(d):
            if not isinstance(d, dict):
                return d
            desc = _DTYPES.get(d["dtype"], d["dtype"]) + str(d["shape"]).replace(" ", "") + ("" if d["contig"] else "s")
            if d["of"] in self.names.values():
                legend[d["of"]] = desc
                desc = d["of"]
            else:
                desc = f'{d["of"]}:{desc}'
            return desc + (f'+{d["off"]}' if d["off"] else "")
        return [f'{name}({", ".join(str(short(d)) for d in args)})' for name, args in self.calls], legend     # one string per call


_DTYPES = {"torch.float32": "f32", "torch.bfloat16": "bf16", "torch.int16": "i16", "torch.int32": "i32", "torch.uint8": "u8"}


def _shape_of(v):
    if isinstance(v, torch.Tensor):
        return _DTYPES.get(str(v.dtype), str(v.dtype)) + str(list(v.shape)).replace(" ", "")
    if isinstance(v, (tuple, list)):
        return [_shape_of(e) for e in v]
    return v if v is None or isinstance(v, (int, float)) else type(v).__name__


class _Lib:
    def __init__(self, real, rec):
        self._real, self._rec = real, rec

    def __getattr__(self, name):
        if name in HOST_ONLY or name.endswith("_bytes"):
            return getattr(self._real, name)

        def entry(*args):
            self._rec.calls.append([name, [self._rec.describe(a) for a in args]])
            return 0
        return entry


@contextlib.contextmanager
def recording(native, rec, limit=None):
    real = native.load()
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(native, "require_hip", lambda x, who: None))
        st.enter_context(mock.patch.object(native, "stream_ptr", lambda device: "stream"))
        st.enter_context(mock.patch.object(native, "load", lambda: lib))
        st.enter_context(mock.patch.object(native, "_lib", None))
        st.enter_context(mock.patch.object(torch.cuda, "device", lambda device: contextlib.nullcontext()))
        if limit is not None:
            st.enter_context(mock.patch.object(native, "CALL_SAMPLES", limit))
        lib = _Lib(real, rec)
        st.enter_context(rec)
        yield


def run_case(native, fn, limit=None):
    rec = Recorder()
    ret, err = None, None
    with recording(native, rec, limit):
        try:
            ret = fn(native, rec)
        except Exception as e:                    # a refusal is part of the record
            err = {"raises": type(e).__name__, "message": str(e)}
    calls, legend = rec.finish(ret)
    return {"calls": calls, **({"in": legend} if legend else {}), **(err if err is not None else {"returns": _shape_of(ret)})}


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
DEFAULT = (2, 2400, 40, 401, 160)        # B, T, F, K, hop: the 16 kHz window, a fused path under AUTO
STAGED = (2, 300, 17, 64, 7)             # a window no fused plan covers: AUTO resolves to the staged kernels
RUNTIME = (3, 700, 8, 101, 40)           # a run-time geometry
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "i16": torch.int16}


def wave(B, T, dtype, layout="b1t"):
    if layout == "b1t":
        return torch.zeros(B, 1, T, dtype=dtype)
    if layout == "bt":
        return torch.zeros(B, T, dtype=dtype)
    assert layout == "strided"
    return torch.zeros(B, 1, 2 * T, dtype=dtype)[:, :, ::2]


def params(F, pcen=True, shared_ema=False):
    p = [torch.zeros(F, 2), torch.zeros(1, 1, F, 1), torch.zeros(F)]
    p += [torch.ones(F), torch.ones(F), torch.ones(F), torch.ones(1 if shared_ema else F)] if pcen else [None] * 4
    return p


PARAM_NAMES = ("kernel", "pool_w", "pool_b", "alpha", "delta", "root", "ema_w")


def _frames(native, T, K, hop):
    return native.load().leaf_num_frames(T, K, hop)


def _forward(geom, dtype="f32", layout="b1t", pcen=True, mix=False, out=None, prm=None, **kw):
    """A case: leaf_forward / leaf_forward_mix.  ``out``: a function (B, F, TP) -> tensor."""
    B, T, F, K, hop = geom

    def case(native, rec):
        (x,) = rec.name(x=wave(B, T, DTYPES[dtype], layout))
        p = rec.name(**dict(zip(PARAM_NAMES, prm(F) if prm else params(F, pcen))))
        if mix:
            perm, lam = rec.name(perm=torch.arange(B - 1, -1, -1), lam=torch.full((B,), 0.25))
            return native.leaf_forward_mix(x, perm, lam, *p, K, hop, pcen=pcen, **kw)
        if out is not None:
            (o,) = rec.name(out=out(B, F, _frames(native, T, K, hop)))
            return native.leaf_forward(x, *p, K, hop, pcen=pcen, out=o, **kw)
        return native.leaf_forward(x, *p, K, hop, pcen=pcen, **kw)
    return case


def _backward(geom, dtype="f32", layout="b1t", pcen=True, mix=False, go_dtype=None, raw=False, go_shape=None, prm=None, channels=1, **kw):
    B, T, F, K, hop = geom

    def case(native, rec):
        TP = _frames(native, T, K, hop)
        (x,) = rec.name(x=wave(B, T, DTYPES[dtype], layout) if channels == 1 else torch.zeros(B, channels, T))
        p = rec.name(**dict(zip(PARAM_NAMES, prm(F) if prm else params(F, pcen))))
        gdt = go_dtype or (torch.bfloat16 if dtype == "bf16" or kw.get("out_bf16") else torch.float32)
        (go,) = rec.name(grad_out=torch.zeros(go_shape or (B, F, TP), dtype=gdt))
        (pr,) = rec.name(pooled_raw=torch.zeros(B, F, TP) if raw else None)
        if mix:
            perm, lam = rec.name(perm=torch.arange(B - 1, -1, -1), lam=torch.full((B,), 0.25))
            return native.leaf_backward_mix(x, perm, lam, *p, K, hop, go, pcen=pcen, pooled_raw=pr, **kw)
        return native.leaf_backward(x, *p, K, hop, go, pcen=pcen, pooled_raw=pr, **kw)
    return case


def _with(geom, **over):
    g = dict(zip(("B", "T", "F", "K", "hop"), geom))
    g.update(over)
    return tuple(g[k] for k in ("B", "T", "F", "K", "hop"))


def _native_cases():
    c = {}
    f32, bf16 = torch.float32, torch.bfloat16
    modes = (("off", {"pcen": False}), ("log1p", {"pcen": False, "log1p": True}))
    geoms = ((DEFAULT, "default"), (STAGED, "auto-staged"), (_with(DEFAULT, B=0), "empty"))
    # forward: dtype x layout, compression, save_raw x out_bf16 on a fused path, on what AUTO hands to the staged kernels, at B == 0
    for dt in DTYPES:
        for layout in ("b1t", "bt", "strided"):
            c[f"forward/{dt}/{layout}/pcen"] = _forward(DEFAULT, dt, layout)
            c[f"forward_mix/{dt}/{layout}"] = _forward(DEFAULT, dt, layout, mix=True)
        for mode, kw in modes:
            c[f"forward/{dt}/b1t/{mode}"] = _forward(DEFAULT, dt, **kw)
        for geom, gname in geoms:
            for save, ob in ((False, False), (True, True)) + (((False, True), (True, False)) if gname != "empty" else ()):
                tag = f"{dt}/{gname}/{'save' if save else 'plain'}/{'out_bf16' if ob else 'follow'}"
                c[f"forward/{tag}"] = _forward(geom, dt, save_raw=save, out_bf16=ob)
                if dt != "bf16" and save == ob:
                    c[f"forward_mix/{tag}"] = _forward(geom, dt, mix=True, save_raw=save, out_bf16=ob)
            c[f"forward/{dt}/{gname}/peaknorm"] = _forward(geom, dt, peak_normalize=True)
        c[f"forward/{dt}/empty/peaknorm-save"] = _forward(_with(DEFAULT, B=0), dt, peak_normalize=True, save_raw=True)
    for mode, kw in modes + (("pcen-log1p-ignored", {"log1p": True}),):
        c[f"forward_mix/i16/{mode}/save"] = _forward(RUNTIME, "i16", mix=True, save_raw=True, **kw)
    # selectors and option bits
    for sel in (1, 2, 3, 4, 5, 9):
        c[f"forward/f32/selector{sel}"] = _forward(DEFAULT, algo=sel)
    for dt in DTYPES:
        c[f"forward/{dt}/selector1/out_bf16-save"] = _forward(DEFAULT, dt, algo=1, out_bf16=True, save_raw=True)
        c[f"forward_mix/{dt}/selector1/out_bf16"] = _forward(DEFAULT, dt, mix=True, algo=1, out_bf16=True)
    c["forward/f32/selector9/out_bf16-save"] = _forward(DEFAULT, algo=9, out_bf16=True, save_raw=True)
    c["forward_mix/f32/selector9/out_bf16"] = _forward(DEFAULT, mix=True, algo=9, out_bf16=True)
    c["forward/f32/option-bits"] = lambda n, r: _forward(DEFAULT, algo=n.ALGO_FFT_WG | n.ALGO_FULL_TRANSFORMS | n.algo_reserve_cus(8))(n, r)
    c["forward/i16/staged-with-option-bits"] = lambda n, r: _forward(DEFAULT, "i16", algo=n.ALGO_STAGED | n.ALGO_STRICT_BAND_CLASSES)(n, r)
    c["forward_mix/f32/option-bits"] = lambda n, r: _forward(DEFAULT, mix=True, algo=n.ALGO_FFT | n.ALGO_NO_TABLE_CACHE)(n, r)
    c["forward/f32/runtime-geometry"] = _forward(RUNTIME)
    # out=: valid and wrong in each way, on the direct path, the narrow-on-host path and the empty batch
    outs = {"valid-f32": lambda *s: torch.zeros(s), "valid-bf16": lambda *s: torch.zeros(s, dtype=bf16),
            "wrong-shape": lambda b, f, tp: torch.zeros(b, f, tp + 1), "wrong-shape-bf16": lambda b, f, tp: torch.zeros(b, f + 1, tp, dtype=bf16),
            "strided": lambda b, f, tp: torch.zeros(b, f, 2 * tp)[:, :, ::2], "strided-bf16": lambda b, f, tp: torch.zeros(b, f, 2 * tp, dtype=bf16)[:, :, ::2],
            "wrong-device": lambda *s: torch.zeros(s, device="meta"), "wrong-device-bf16": lambda *s: torch.zeros(s, dtype=bf16, device="meta")}
    for oname, make in outs.items():
        for geom, gname in geoms:
            for dt, ob in (("f32", False), ("i16", True)) + ((("f32", True), ("bf16", False)) if geom is DEFAULT else ()):
                c[f"forward-out/{oname}/{gname}/{dt}/{'out_bf16' if ob else 'follow'}"] = _forward(geom, dt, out=make, out_bf16=ob)
        c[f"forward-out/{oname}/save"] = _forward(DEFAULT, out=make, save_raw=True)
        c[f"forward-out/{oname}/auto-staged/save-out_bf16"] = _forward(STAGED, "i16", out=make, save_raw=True, out_bf16=True)
    # refusals of the inputs
    for name, shape in (("b2t", (2, 2, 2400)), ("1d", (2400,)), ("4d", (2, 1, 1, 2400)), ("too-short", (2, 1, 0))):
        def bad(native, rec, shape=shape, mix=False):
            x = torch.zeros(shape)
            p = params(40)
            if mix:
                return native.leaf_forward_mix(x, torch.zeros(shape[0], dtype=torch.int64), torch.zeros(shape[0]), *p, 401, 160)
            return native.leaf_forward(x, *p, 401, 160)
        c[f"forward/bad-shape/{name}"] = bad
        c[f"forward_mix/bad-shape/{name}"] = lambda n, r, bad=bad: bad(n, r, mix=True)

    def bad_param(which, how):
        def prm(F):
            p = params(F)
            i = PARAM_NAMES.index(which)
            p[i] = p[i].double() if how == "dtype" else p[i].to("meta")
            return p
        return prm
    for which in PARAM_NAMES:
        for how in ("dtype", "device"):
            c[f"forward/bad-{which}-{how}"] = _forward(DEFAULT, prm=bad_param(which, how))
    c["forward_mix/bad-kernel-dtype"] = _forward(DEFAULT, mix=True, prm=bad_param("kernel", "dtype"))
    c["forward_mix/bad-ema_w-device"] = _forward(DEFAULT, mix=True, prm=bad_param("ema_w", "device"))
    c["forward/f64-x"] = lambda n, r: n.leaf_forward(torch.zeros(2, 1, 2400, dtype=torch.float64), *params(40), 401, 160)
    c["forward_mix/f64-x"] = lambda n, r: n.leaf_forward_mix(torch.zeros(2, 1, 2400, dtype=torch.float64), [1, 0], [0.5, 0.5], *params(40), 401, 160)
    c["forward_mix/bad-perm"] = lambda n, r: n.leaf_forward_mix(torch.zeros(2, 1, 2400), [0, 2], [0.5, 0.5], *params(40), 401, 160)
    c["forward_mix/bad-lam"] = lambda n, r: n.leaf_forward_mix(torch.zeros(2, 1, 2400), [0, 1], torch.zeros(2, dtype=torch.float64), *params(40), 401, 160)
    # backward: every flag, with and without dL/dx
    flags = ("staged", "mfma", "full_transforms", "strict_band_classes", "log1p")
    for fl in flags:
        for pcen in (True, False):
            tag = f"{'pcen' if pcen else 'off'}/nodx/{fl}"
            c[f"backward/f32/{tag}"] = _backward(DEFAULT, pcen=pcen, **{fl: True})
            c[f"backward_mix/f32/{tag[:-len(fl) - 6]}/{fl}"] = _backward(DEFAULT, pcen=pcen, mix=True, **{fl: True})
    for dt in DTYPES:
        for pcen in (True, False):
            for need_dx in (False, True):
                tag = f"{dt}/{'pcen' if pcen else 'off'}/{'dx' if need_dx else 'nodx'}"
                c[f"backward/{tag}"] = _backward(DEFAULT, dt, pcen=pcen, need_dx=need_dx)
                if pcen:
                    c[f"backward/{tag}/raw-out_bf16"] = _backward(DEFAULT, dt, need_dx=need_dx, raw=True, out_bf16=True)
                    c[f"backward/{tag}/all-flags"] = _backward(DEFAULT, dt, need_dx=need_dx, raw=True, **{fl: True for fl in flags})
            if dt != "bf16":
                tag = f"{dt}/{'pcen' if pcen else 'off'}"
                c[f"backward_mix/{tag}"] = _backward(DEFAULT, dt, pcen=pcen, mix=True)
                c[f"backward_mix/{tag}/raw-out_bf16"] = _backward(RUNTIME, dt, pcen=pcen, mix=True, raw=True, out_bf16=True)
                c[f"backward_mix/{tag}/all-flags"] = _backward(DEFAULT, dt, pcen=pcen, mix=True, raw=True, **{fl: True for fl in flags})
        for layout in ("bt", "strided"):
            c[f"backward/{dt}/{layout}"] = _backward(DEFAULT, dt, layout, need_dx=dt != "i16")
            c[f"backward_mix/{dt}/{layout}"] = _backward(DEFAULT, dt, layout, mix=True)
        for ob in (False, True):
            for need_dx in (False, True):
                c[f"backward/{dt}/empty/{'out_bf16' if ob else 'follow'}/{'dx' if need_dx else 'nodx'}"] = _backward(_with(DEFAULT, B=0), dt, need_dx=need_dx, out_bf16=ob)
            c[f"backward_mix/{dt}/empty/{'out_bf16' if ob else 'follow'}"] = _backward(_with(DEFAULT, B=0), dt, mix=True, out_bf16=ob, pcen=not ob)
        # grad_out of the wrong dtype, each way round, and of the wrong shape
        for gname, gdt in (("f32", f32), ("bf16", bf16), ("f64", torch.float64)):
            for ob in (False, True):
                c[f"backward/{dt}/grad_out-{gname}/{'out_bf16' if ob else 'follow'}"] = _backward(DEFAULT, dt, go_dtype=gdt, out_bf16=ob)
                if dt == "f32":
                    c[f"backward_mix/{dt}/grad_out-{gname}/{'out_bf16' if ob else 'follow'}"] = _backward(DEFAULT, dt, mix=True, go_dtype=gdt, out_bf16=ob)
        c[f"backward/{dt}/grad_out-shape"] = _backward(DEFAULT, dt, go_shape=(2, 40, 16))
    c["backward_mix/i16/grad_out-shape"] = _backward(DEFAULT, "i16", mix=True, go_shape=(2, 40, 16))
    c["backward_mix/bad-shape"] = lambda n, r: n.leaf_backward_mix(torch.zeros(2, 2, 2400), [1, 0], [0.5, 0.5], *params(40), 401, 160, torch.zeros(2, 40, 15))

    # profiled and prepared
    def profiled(dt, layout="b1t", prm=None, channels=1, **kw):
        def case(native, rec):
            B, T, F, K, hop = DEFAULT
            (x,) = rec.name(x=wave(B, T, DTYPES[dt], layout) if channels == 1 else torch.zeros(B, channels, T))
            p = rec.name(**dict(zip(PARAM_NAMES, prm(F) if prm else params(F, kw.get("pcen", True)))))
            return native.leaf_forward_profiled(x, *p, K, hop, algo=native.ALGO_FFT_WG, **kw)
        return case

    def prepared(dt, layout="b1t", ob=False, out=None, B=DEFAULT[0], prm=None, **kw):
        def case(native, rec):
            _, T, F, K, hop = DEFAULT
            (x,) = rec.name(x=wave(B, T, DTYPES[dt], layout))
            p = rec.name(**dict(zip(PARAM_NAMES, prm(F) if prm else params(F, kw.get("pcen", True)))))
            (tables,) = rec.name(tables=torch.zeros(native.load().leaf_fft_tables_bytes(F, K, hop), dtype=torch.uint8))
            (o,) = rec.name(out=None if out is None else out(B, F, _frames(native, T, K, hop)))
            return native.leaf_forward_prepared(x, tables, *p[2:], F, K, hop, out=o, out_bf16=ob, **kw)
        return case
    for dt in DTYPES:
        for layout in ("b1t", "bt", "strided"):
            c[f"profiled/{dt}/{layout}/pcen"] = profiled(dt, layout)
            c[f"prepared/{dt}/{layout}/pcen/follow"] = prepared(dt, layout)
        c[f"prepared/{dt}/b1t/pcen/out_bf16"] = prepared(dt, ob=True)
    for mode, kw in modes:
        c[f"profiled/f32/b1t/{mode}"] = profiled("f32", **kw)
        c[f"prepared/i16/b1t/{mode}/out_bf16"] = prepared("i16", ob=True, **kw)
    c["prepared/out-given"] = prepared("f32", out=lambda *s: torch.zeros(s))
    c["prepared/out-given-bf16"] = prepared("i16", ob=True, out=lambda *s: torch.zeros(s, dtype=bf16))
    c["prepared/empty"] = prepared("f32", B=0)
    c["prepared/bad-shape"] = lambda n, r: n.leaf_forward_prepared(torch.zeros(2, 2, 2400), torch.zeros(8, dtype=torch.uint8), *params(40)[2:], 40, 401, 160)
    # what the shared unpacker and gatherer changed on purpose (CHANGED_ON_PURPOSE): a wrong PCEN parameter is named by every wrapper,
    # a (B,C,T) waveform is refused by every wrapper, the parameters answer before grad_out and before the narrow-on-host path's out
    bad_alpha = bad_param("alpha", "dtype")
    c["backward/bad-alpha-dtype"] = _backward(DEFAULT, prm=bad_alpha)
    c["backward_mix/bad-alpha-dtype"] = _backward(DEFAULT, mix=True, prm=bad_alpha)
    c["profiled/bad-alpha-dtype"] = profiled("f32", prm=bad_alpha)
    c["prepared/bad-alpha-dtype"] = prepared("f32", prm=bad_alpha)
    c["backward/two-channels"] = _backward(DEFAULT, channels=2)
    c["profiled/two-channels"] = profiled("f32", channels=2)
    c["backward/bad-alpha-and-grad_out"] = _backward(DEFAULT, prm=bad_alpha, go_dtype=torch.float64)
    c["forward-out/bad-alpha-and-out/auto-staged"] = _forward(STAGED, out=lambda *s: torch.zeros(s), out_bf16=True, prm=bad_alpha)
    c["profiled/default-algo"] = lambda n, r: n.leaf_forward_profiled(torch.zeros(2, 1, 2400), *params(40), 401, 160)
    return c


def _sliced_cases():
    """Run with the sample limit of one C-ABI call at SMALL_LIMIT."""
    c = {}
    big = _with(DEFAULT, B=3)            # 3 x 2400 >= 5000: a slice of two clips and one of one
    for dt in DTYPES:
        for save, ob in ((False, False), (True, True)):
            c[f"sliced/forward/{dt}/{'save' if save else 'plain'}/{'out_bf16' if ob else 'follow'}"] = _forward(big, dt, save_raw=save, out_bf16=ob)
        c[f"sliced/forward/{dt}/staged"] = _forward(big, dt, algo=1, out_bf16=dt == "i16")
        c[f"sliced/forward/{dt}/out-given"] = _forward(big, dt, out=lambda *s, dt=dt: torch.zeros(s, dtype=torch.bfloat16 if dt == "bf16" else torch.float32))
        c[f"sliced/backward/{dt}"] = _backward(big, dt, need_dx=dt != "i16", raw=True, pcen=dt != "bf16", log1p=True)
        c[f"sliced/backward/{dt}/out_bf16"] = _backward(big, dt, out_bf16=True, strict_band_classes=True)
        if dt != "bf16":
            c[f"sliced/forward_mix/{dt}"] = _forward(big, dt, mix=True)
            c[f"sliced/backward_mix/{dt}"] = _backward(big, dt, mix=True)
            c[f"sliced/mixup/{dt}"] = lambda n, r, dt=dt: n.mixup(torch.zeros(3, 1, 2400, dtype=DTYPES[dt]), [0, 1, 2], torch.zeros(3))
    c["sliced/forward/strided-peaknorm"] = _forward(big, layout="strided", peak_normalize=True)
    c["sliced/batch_slices"] = lambda n, r: [list(s) for s in n.batch_slices(5, 2400)] + [list(s) for s in n.batch_slices(7, 1000)]
    long_clip = _with(DEFAULT, B=3, T=6000)
    c["sliced/forward/clip-beyond-one-call"] = _forward(long_clip)
    c["sliced/backward/clip-beyond-one-call"] = _backward(long_clip)
    c["sliced/batch_slices/clip-beyond-one-call"] = lambda n, r: [list(s) for s in n.batch_slices(3, 6000)]
    return c


def _stage_cases():
    c = {}
    F, K, hop, T = 5, 33, 8, 300
    for B in (2, 0):
        TP = -(-T // hop)
        b = f"B{B}"
        for shared in (False, True):
            s = "shared" if shared else "per-channel"

            def prm(rec, shared=shared):
                return rec.name(alpha=torch.ones(F), delta=torch.ones(F), root=torch.ones(F), ema_w=torch.ones(1) if shared else torch.ones(F))
            c[f"stage/ema/{s}/{b}"] = lambda n, r, B=B, prm=prm: n.ema(*r.name(p=torch.zeros(B, F, TP)), prm(r)[3])
            c[f"stage/pcen/{s}/{b}"] = lambda n, r, B=B, prm=prm: n.pcen(*r.name(p=torch.zeros(B, F, TP)), *prm(r), 1e-12)
            c[f"stage/ema_backward/{s}/{b}"] = lambda n, r, B=B, prm=prm: n.ema_backward(*r.name(p=torch.zeros(B, F, TP)), prm(r)[3], *r.name(grad_ema=torch.zeros(B, F, TP)))
            c[f"stage/pcen_backward/{s}/{b}"] = lambda n, r, B=B, prm=prm: n.pcen_backward(*r.name(p=torch.zeros(B, F, TP)), *prm(r), 1e-12, *r.name(grad_out=torch.zeros(B, F, TP)))
            c[f"stage/pcen_stream/{s}/{b}"] = lambda n, r, B=B, prm=prm: n.pcen_stream(*r.name(p=torch.zeros(B, F, 7)), *prm(r), 1e-12, *r.name(ema_state=torch.zeros(B, F)))
        c[f"stage/pcen_stream/first/{b}"] = lambda n, r, B=B: n.pcen_stream(*r.name(p=torch.zeros(B, F, 7), alpha=torch.ones(F), delta=torch.ones(F), root=torch.ones(F), ema_w=torch.ones(F)), 1e-12)
        c[f"stage/pcen_stream/no-pcen-log1p/{b}"] = lambda n, r, B=B: n.pcen_stream(*r.name(p=torch.zeros(B, F, 7)), None, None, None, None, 1e-5, log1p=True)
        c[f"stage/gabor_conv/{b}"] = lambda n, r, B=B: n.gabor_conv(*r.name(x=torch.zeros(B, 1, T), kernel=torch.zeros(F, 2)), K)
        c[f"stage/squared_modulus/{b}"] = lambda n, r, B=B: n.squared_modulus(*r.name(y=torch.zeros(B, 2 * F, T)))
        c[f"stage/gaussian_lowpass/{b}"] = lambda n, r, B=B: n.gaussian_lowpass(*r.name(e=torch.zeros(B, F, T), pool_w=torch.zeros(1, 1, F, 1), pool_b=torch.zeros(F)), K, hop)
        c[f"stage/gaussian_lowpass/no-bias/{b}"] = lambda n, r, B=B: n.gaussian_lowpass(*r.name(e=torch.zeros(B, F, T), pool_w=torch.zeros(1, 1, F, 1)), None, K, hop)
        for dk in (True, False):
            for dx in (True, False):
                c[f"stage/gabor_conv_backward/dk{int(dk)}-dx{int(dx)}/{b}"] = lambda n, r, B=B, dk=dk, dx=dx: n.gabor_conv_backward(
                    *r.name(x=torch.zeros(B, 1, T), kernel=torch.zeros(F, 2)), K, *r.name(grad_y=torch.zeros(B, 2 * F, T)), need_dk=dk, need_dx=dx)
        c[f"stage/squared_modulus_backward/{b}"] = lambda n, r, B=B: n.squared_modulus_backward(*r.name(y=torch.zeros(B, 2 * F, T), grad_e=torch.zeros(B, F, T)))
        for need in ((True, True, True), (False, True, False), (True, False, True), (False, False, False)):
            c[f"stage/gaussian_lowpass_backward/{''.join(str(int(v)) for v in need)}/{b}"] = lambda n, r, B=B, need=need: n.gaussian_lowpass_backward(
                *r.name(e=torch.zeros(B, F, T), pool_w=torch.zeros(1, 1, F, 1)), K, hop, *r.name(grad_pooled=torch.zeros(B, F, TP)),
                need_de=need[0], need_dw=need[1], need_db=need[2])
        for shape in ((B, 1, T), (B, T), (B, 2, T)):
            c[f"stage/peak_normalize/{len(shape)}d-{shape[1]}/{b}"] = lambda n, r, shape=shape: n.peak_normalize(*r.name(x=torch.zeros(shape)))
        c[f"stage/peak_normalize/out-given/{b}"] = lambda n, r, B=B: n.peak_normalize(*r.name(x=torch.zeros(B, 1, T), out=torch.zeros(B, T)))
        c[f"stage/peak_normalize/out-wrong/{b}"] = lambda n, r, B=B: n.peak_normalize(*r.name(x=torch.zeros(B, 1, T), out=torch.zeros(B, T, dtype=torch.bfloat16)))
        for dt in ("f32", "i16"):
            c[f"stage/mixup/{dt}/{b}"] = lambda n, r, B=B, dt=dt: n.mixup(*r.name(x=torch.zeros(B, 1, T, dtype=DTYPES[dt]), perm=torch.arange(B), lam=torch.zeros(B)))
    c["stage/mixup/bf16"] = lambda n, r: n.mixup(torch.zeros(2, 1, T, dtype=torch.bfloat16), [0, 1], [0.0, 1.0])
    c["stage/mixup/bt-sequences"] = lambda n, r: n.mixup(*r.name(x=torch.zeros(2, T)), [1, 0], [0.0, 1.0])
    c["stage/gabor_conv/bad-shape"] = lambda n, r: n.gabor_conv(torch.zeros(2, T), torch.zeros(F, 2), K)
    c["stage/squared_modulus/odd-channels"] = lambda n, r: n.squared_modulus(torch.zeros(2, 5, T))
    c["stage/ema/bad-dtype"] = lambda n, r: n.ema(torch.zeros(2, F, 4, dtype=torch.float64), torch.ones(F))
    c["stage/gabor_taps"] = lambda n, r: n.gabor_taps(*r.name(kernel=torch.zeros(F, 2)), K)
    c["stage/lowpass_window"] = lambda n, r: n.lowpass_window(*r.name(pool_w=torch.zeros(1, 1, F, 1)), K)
    c["stage/prepare_tables/default"] = lambda n, r: n.prepare_tables(*r.name(kernel=torch.zeros(40, 2), pool_w=torch.zeros(1, 1, 40, 1)), 401, 160)
    c["stage/prepare_tables/not-covered"] = lambda n, r: n.prepare_tables(*r.name(kernel=torch.zeros(17, 2), pool_w=torch.zeros(1, 1, 17, 1)), 64, 7)
    c["stage/band_classes/strict"] = lambda n, r: n.band_classes(*r.name(kernel=torch.zeros(40, 2), pool_w=torch.zeros(1, 1, 40, 1)), 401, 160)
    c["stage/band_classes/bias-aware"] = lambda n, r: n.band_classes(*r.name(kernel=torch.zeros(40, 2), pool_w=torch.zeros(1, 1, 40, 1)), 401, 160,
                                                                       *r.name(pool_b=torch.zeros(40)))

    def stream(native, rec, pcen=True, pcm=False):
        B, F_, K_, hop_ = 2, 40, 401, 160
        flags = (native.FLAG_PCEN if pcen else native.FLAG_LOG1P) | (native.FLAG_X_PCM16 if pcm else 0)
        state = native.stream_state(B, F_, K_, hop_, flags, torch.device("cpu"))
        (chunk, state, out) = rec.name(chunk=torch.zeros(B, 4000, dtype=torch.int16 if pcm else torch.float32), state=state, out=torch.zeros(B, F_, 3))
        p = rec.name(**dict(zip(PARAM_NAMES, [t if t is None else t.reshape(-1) if t.dim() == 4 else t for t in params(F_, pcen)])))
        at = 100
        native.stream_step(chunk.data_ptr() + at * chunk.element_size(), B, 480, chunk.stride(0), state, 200, 1, 0, 1, 3, True, p, F_, K_, hop_, flags,
                           out.data_ptr(), torch.device("cpu"))
        return state
    c["stage/stream_step/pcen"] = stream
    c["stage/stream_step/log1p-pcm"] = lambda n, r: stream(n, r, pcen=False, pcm=True)
    c["stage/stream_state/not-covered"] = lambda n, r: n.stream_state(2, 17, 64, 7, 0, torch.device("cpu"))
    return c


# ---- frontend.py over the ctypes route (the ops library masked off) --------------------------------------------------------------
def _frontend_cases():
    c = {}

    def module(pcen=True, setup=None):
        from leaf_pytorch_amd import Leaf
        m = Leaf(pcen_compression=pcen)
        return setup(m) if setup else m

    def name_params(rec, m):
        pc = m._compression
        rec.name(kernel=m._complex_conv._kernel, pool_w=m._pooling.weights, pool_b=m._pooling._bias,
                 **({} if pc is None else dict(alpha=pc.alpha, delta=pc.delta, root=pc.root, ema_w=pc.ema._weights)))

    def call(mix, train, dt="f32", pcen=True, setup=None, x_grad=False, geom=(3, 2400), go_bf16=False):
        def case(native, rec):
            m = module(pcen, setup)
            name_params(rec, m)
            (x,) = rec.name(x=wave(geom[0], geom[1], DTYPES[dt]).requires_grad_(x_grad))
            extra = rec.name(perm=torch.tensor([0, 2, 1]), lam=torch.tensor([0.0, 1.0, 0.3])) if mix else ()
            fn = m.forward_mixup if mix else m.forward
            if not train:
                with torch.no_grad():
                    return fn(x, *extra)
            out = fn(x, *extra)
            (go,) = rec.name(grad_out=torch.zeros(out.shape, dtype=out.dtype))
            out.backward(go)
            return [out, x.grad] + [p.grad for p in m.parameters()]
        return case

    def strict(m):
        m._algo |= 1 << 27               # LEAF_ALGO_STRICT_BAND_CLASSES: the autograd function hands it to the backward as a flag
        return m

    setups = {"default": None, "bf16-features": lambda m: m.output_dtype(torch.bfloat16), "full-transforms": lambda m: m.full_transforms()}
    for mix in (False, True):
        who = "forward_mixup" if mix else "forward"
        for train in (False, True):
            how = "train" if train else "no_grad"
            for sname, setup in setups.items():
                for dt in ("f32", "i16") if sname != "full-transforms" else ("f32",):
                    c[f"frontend/{who}/{how}/{sname}/{dt}"] = call(mix, train, dt, setup=setup)
            c[f"frontend/{who}/{how}/log1p"] = call(mix, train, pcen=False, setup=lambda m: m.log_compression())
            c[f"frontend/{who}/{how}/no-compression"] = call(mix, train, pcen=False)
            c[f"frontend/{who}/{how}/strict-band-classes"] = call(mix, train, setup=strict)
            c[f"frontend/{who}/{how}/fused-peaknorm"] = call(mix, train, setup=lambda m: m.fuse_peak_normalization())
        c[f"frontend/{who}/x-requires-grad"] = call(mix, True, x_grad=True)
    c["frontend/forward/no_grad/bf16-x"] = call(False, False, "bf16")
    c["frontend/forward/train/bf16-x"] = call(False, True, "bf16")
    c["frontend/forward_mixup/bf16-x"] = call(True, False, "bf16")
    c["frontend/forward/no_grad/fused-peaknorm/workgroup"] = call(False, False, setup=lambda m: m.fuse_peak_normalization(), geom=(24, 16000))
    c["frontend/forward/no_grad/cache-tables"] = call(False, False, setup=lambda m: m.cache_tables(), geom=(24, 16000))
    c["frontend/forward/no_grad/cache-tables/bf16-features-i16"] = call(False, False, "i16", setup=lambda m: m.cache_tables().output_dtype(torch.bfloat16), geom=(24, 16000))
    c["frontend/forward/no_grad/cache-tables/small-batch"] = call(False, False, setup=lambda m: m.cache_tables())
    c["frontend/forward/train/cache-tables"] = call(False, True, setup=lambda m: m.cache_tables(), geom=(24, 16000))
    return c


def cases():
    """name -> (case, sample limit or None, drives frontend.py)"""
    out = {n: (f, None, False) for n, f in {**_native_cases(), **_stage_cases()}.items()}
    out.update({n: (f, SMALL_LIMIT, False) for n, f in _sliced_cases().items()})
    out.update({n: (f, None, True) for n, f in _frontend_cases().items()})
    return out


def replay(native, only=None):
    """Every case's record.  Frontend cases run the installed package (its ``_native`` must be ``native``) with the ops library masked."""
    from leaf_pytorch_amd import _ops
    got = {}
    for name, (fn, limit, frontend) in cases().items():
        if only is not None and name not in only:
            continue
        if frontend:
            assert native is sys.modules["leaf_pytorch_amd._native"]
            with mock.patch.object(_ops, "available", lambda: False):
                got[name] = run_case(native, fn, limit)
        else:
            got[name] = run_case(native, fn, limit)
    return got


def load_table():
    with open(TABLE) as fh:
        t = json.load(fh)
    for r in t["cases"].values():
        if "in" in r:
            r["in"] = t["inputs"][r["in"]]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="", help="the commit the wrappers are recorded from (kept in the table)")
    a = ap.parse_args()
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    native = importlib.import_module("leaf_pytorch_amd._native")
    got = replay(native)
    legends = sorted({json.dumps(r["in"], sort_keys=True) for r in got.values() if "in" in r})      # most cases share their inputs: kept once
    for r in got.values():
        if "in" in r:
            r["in"] = legends.index(json.dumps(r["in"], sort_keys=True))
    with open(TABLE, "w") as fh:
        json.dump({"recorded_from": a.commit, "small_limit": SMALL_LIMIT, "inputs": [json.loads(l) for l in legends], "cases": got}, fh,
                  separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print(f"{len(got)} cases, {sum(len(r['calls']) for r in got.values())} C-ABI calls, {os.path.getsize(TABLE)} bytes -> {TABLE}")


if __name__ == "__main__":
    main()
