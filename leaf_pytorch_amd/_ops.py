"""Dispatcher ops ``torch.ops.leaf_amd.{forward, forward_train, backward, backward_head}`` (csrc/torch_binding.cpp: a thin torch
extension over the C ABI of include/leaf_hip.h) plus what only Python can attach to them: the fake (meta) kernels
``torch.compile`` / ``torch.export`` need to propagate shapes, and the autograd formula of the training forward, which picks the
full or the head-only backward by what needs a gradient (``backward_route``).

``Leaf.forward`` goes through these ops, so a model containing the frontend compiles without a graph break and an eager
call costs one dispatcher hop.  There is no fallback: the ops exist only for HIP tensors and fail loudly otherwise.
"""
from __future__ import annotations

import os
import subprocess
import sysconfig
import threading
from typing import Optional

import torch

from . import _native

OPS_LIB_PATH = os.path.join(_native._PKG_DIR, "_leaf_torch_ops.so")
OPS_SRC_PATH = os.path.join(_native._PKG_DIR, "csrc", "torch_binding.cpp")
_loaded = False
_load_lock = threading.Lock()


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/torch_binding.cpp (plain C++, g++) against the torch headers and libleaf_hip.so, in-tree."""
    from torch.utils import cpp_extension as ce
    deps = [OPS_SRC_PATH, os.path.join(_native.INCLUDE_DIR, "leaf_hip.h")]
    if not force and os.path.exists(OPS_LIB_PATH) and os.path.getmtime(OPS_LIB_PATH) >= max(os.path.getmtime(d) for d in deps):
        return OPS_LIB_PATH
    _native.build()                                          # links against libleaf_hip.so
    tl = os.path.join(os.path.dirname(torch.__file__), "lib")
    inc = ce.include_paths() + ["/opt/rocm/include", _native.INCLUDE_DIR, sysconfig.get_paths()["include"]]
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-DUSE_ROCM", "-D__HIP_PLATFORM_AMD__",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}"] + [f"-I{i}" for i in inc] + [
           OPS_SRC_PATH, "-o", OPS_LIB_PATH + ".tmp", f"-L{tl}", "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip",
           f"-L{_native._PKG_DIR}", "-lleaf_hip", "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{tl}"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(OPS_LIB_PATH + ".tmp", OPS_LIB_PATH)
    return OPS_LIB_PATH


def load() -> None:
    """Register the ops (idempotent).  Raises if the extension has not been built -- no fallback."""
    global _loaded
    if _loaded:
        return
    # The first call may come from several threads at once (nn.DataParallel replicas call Leaf.forward concurrently, and
    # dlopen releases the GIL): register exactly once.
    with _load_lock:
        if _loaded:
            return
        if not os.path.exists(OPS_LIB_PATH):
            raise RuntimeError(f"{OPS_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        _native.load()
        torch.ops.load_library(OPS_LIB_PATH)
        _register_python_side()
        _loaded = True


def available() -> bool:
    return _loaded or os.path.exists(OPS_LIB_PATH)


def _frames(T: int, K: int, hop: int) -> int:
    pad_l, pad_r = K // 2 + K % 2 - 1, K // 2                 # utils.py:5-10
    return (T + pad_l + pad_r - K) // hop + 1


def _out_dtype(x: torch.Tensor, out_bf16: bool = False) -> torch.dtype:
    """Feature dtype for a waveform: bfloat16 clips give bfloat16 features, int16 PCM (like float32) gives float32 -- or bfloat16
    when the call asks for it (``out_bf16``: LEAF_FLAG_OUT_BF16)."""
    return torch.bfloat16 if x.dtype == torch.bfloat16 or out_bf16 else torch.float32


def backward_route(need_kernel: bool, need_pool_w: bool, need_x: bool, create_graph: bool) -> str:
    """Which backward a training forward gets: ``"head"`` -- leaf_amd::backward_head, the gradients of the pooling bias and the PCEN
    vectors from the saved pre-floor pooled tensor alone, one launch -- exactly when neither the Gabor kernel, nor the pooling width,
    nor the waveform needs a gradient and no graph of the backward is asked for; ``"full"`` (leaf_amd::backward) otherwise.

    The forward decides what it saves from the three needs (``create_graph`` is not known before the backward runs): on the head
    route that is the pooled tensor and the PCEN vectors -- no waveform, no ``perm`` / ``lam``, no kernel, no pooling width."""
    return "full" if (need_kernel or need_pool_w or need_x or create_graph) else "head"


def _register_family(mixed: bool) -> None:
    """Fake kernels and the autograd formula of one family of three ops: forward / forward_train / backward, or (``mixed``) the
    same three with (perm, lam) behind x -- waveform mixup, parameter gradients only."""
    sfx = "_mix" if mixed else ""
    lead = 3 if mixed else 1                                     # x [, perm, lam] in front of the seven parameters

    def feat_dtype(x, out_bf16):                                 # (a mixed call takes no bfloat16 waveform)
        return (torch.bfloat16 if out_bf16 else torch.float32) if mixed else _out_dtype(x, out_bf16)

    @torch.library.register_fake(f"leaf_amd::forward{sfx}")
    def _(*args, out_bf16=False):
        x, kernel, (K, hop) = args[0], args[lead], args[lead + 7:lead + 9]
        return x.new_empty((x.shape[0], kernel.shape[0], _frames(x.shape[-1], K, hop)), dtype=feat_dtype(x, out_bf16))

    @torch.library.register_fake(f"leaf_amd::forward_train{sfx}")
    def _(*args, out_bf16=False):
        x, kernel, (K, hop) = args[0], args[lead], args[lead + 7:lead + 9]
        shape = (x.shape[0], kernel.shape[0], _frames(x.shape[-1], K, hop))
        return x.new_empty(shape, dtype=feat_dtype(x, out_bf16)), x.new_empty(shape, dtype=torch.float32)

    @torch.library.register_fake(f"leaf_amd::backward{sfx}")
    def _(*args, out_bf16=False):
        x, (kernel, pool_w, pool_b, alpha) = args[0], args[lead:lead + 4]
        pc = kernel.shape[0] if alpha is not None else 0
        e = lambda *s: kernel.new_empty(s)
        grads = [torch.empty_like(kernel), torch.empty_like(pool_w), torch.empty_like(pool_b), e(pc), e(pc), e(pc), e(pc)]
        if mixed:
            return grads
        need_dx = args[lead + 11]
        return grads + [torch.empty_like(x) if need_dx else e(0)]    # (g_x in the dtype of x: bfloat16 for bfloat16 I/O)

    def setup_context(ctx, inputs, keyword_only_inputs, output):
        kernel, pool_w, pool_b, alpha, delta, root, ema_w, K, hop, algo, log1p = inputs[lead:]
        _, raw = output
        ctx.pcen = alpha is not None
        ctx.out_bf16 = bool(keyword_only_inputs["out_bf16"])     # the features left in bfloat16: their gradient arrives in bfloat16
        ctx.log1p = bool(log1p) and not ctx.pcen                 # (ignored with PCEN on, as in the forward)
        ctx.geom = (K, hop)
        ctx.full = bool(algo & _native.ALGO_FULL_TRANSFORMS)     # Leaf.full_transforms(): no band tasks in the backward either
        ctx.strict = bool(algo & _native.ALGO_STRICT_BAND_CLASSES)
        need = ctx.needs_input_grad
        ctx.route = "full" if algo & _native.OPT_FULL_BACKWARD else backward_route(need[lead], need[lead + 1], need[0] or (mixed and need[2]), False)
        if ctx.route == "head":
            # nothing of the waveform side reaches the backward: not x, not (perm, lam), not the filterbank
            ctx.grad_bf16 = ctx.out_bf16 or inputs[0].dtype == torch.bfloat16     # (a bfloat16 waveform: bfloat16 features)
            ctx.save_for_backward(pool_b, raw, *([alpha, delta, root, ema_w] if ctx.pcen else []))
            return
        ctx.save_for_backward(*inputs[:lead], kernel, pool_w, pool_b, raw, *([alpha, delta, root, ema_w] if ctx.pcen else []))

    def backward_head(ctx, grad_out):
        pool_b, raw, *pc = ctx.saved_tensors
        # Under create_graph=True (grad mode is on in here) the same op runs: its own autograd formula (_second_order.py) gives the
        # gradients of these gradients from the pooled tensor, which is all they depend on with the filterbank and x constant.
        gpb, *gpc = torch.ops.leaf_amd.backward_head(raw, grad_out.contiguous(), pool_b, *(pc or (None,) * 4),
                                                     _native.FLAG_LOG1P if ctx.log1p else 0, out_bf16=ctx.grad_bf16)
        return (*(None,) * (lead + 2), gpb, *(gpc if ctx.pcen else (None,) * 4), None, None, None, None)   # (one per positional input)

    def backward(ctx, grad_out, grad_raw):
        if ctx.route == "head":
            return backward_head(ctx, grad_out)
        K, hop = ctx.geom
        saved = ctx.saved_tensors
        kernel, pool_w, pool_b, raw = saved[lead:lead + 4]
        alpha, delta, root, ema_w = saved[lead + 4:] if ctx.pcen else (None,) * 4
        flags = _native.backward_flags(full_transforms=ctx.full, strict_band_classes=ctx.strict, log1p=ctx.log1p)   # (the op adds PCEN and the dtype bits)
        params = (kernel, pool_w, pool_b, alpha, delta, root, ema_w, K, hop, grad_out.contiguous(), raw)
        if mixed:
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
                raise RuntimeError("leaf_amd::forward_train_mix has no gradient for x or lam: the mixed waveform is data "
                                   "(dL/dx under mixup is a scatter over perm and is not built)")
            grads, gx = torch.ops.leaf_amd.backward_mix(*saved[:lead], *params, flags, out_bf16=ctx.out_bf16), None
        else:
            need_dx = ctx.needs_input_grad[0]
            *grads, gx = torch.ops.leaf_amd.backward(saved[0], *params, need_dx, flags,
                                                     out_bf16=ctx.out_bf16)   # (the bfloat16 grad_out goes straight in)
            gx = gx if need_dx else None
        gk, gpw, gpb, *pc = grads
        return (gx, *(None,) * (lead - 1), gk, gpw, gpb, *(pc if ctx.pcen else (None,) * 4), None, None, None, None)   # (one per positional input)

    torch.library.register_autograd(f"leaf_amd::forward_train{sfx}", backward, setup_context=setup_context)


def _register_head() -> None:
    @torch.library.register_fake("leaf_amd::backward_head")
    def _(pooled_raw, grad_out, pool_b, alpha, delta, root, ema_w, flags, out_bf16=False):
        pc = pooled_raw.shape[1] if alpha is not None else 0
        e = lambda *s: pooled_raw.new_empty(s, dtype=torch.float32)
        return [e(*pool_b.shape), e(pc), e(pc), e(pc), e(pc)]


def _register_python_side() -> None:
    _register_head()
    _register_family(mixed=False)
    _register_family(mixed=True)
    from . import _second_order
    _second_order.register()                  # gradients of gradients: leaf_amd::backward's own autograd formula


def forward(x, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int, log1p: bool = False,
            algo: int = _native.ALGO_AUTO, out_bf16: bool = False) -> torch.Tensor:
    return torch.ops.leaf_amd.forward(x, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K, hop, log1p, algo, out_bf16=out_bf16)


def forward_train(x, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int,
                  algo: int = _native.ALGO_AUTO, log1p: bool = False, out_bf16: bool = False) -> torch.Tensor:
    return torch.ops.leaf_amd.forward_train(x, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K, hop, algo, log1p, out_bf16=out_bf16)[0]


def forward_mix(x, perm, lam, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int, log1p: bool = False,
                algo: int = _native.ALGO_AUTO, out_bf16: bool = False) -> torch.Tensor:
    return torch.ops.leaf_amd.forward_mix(x, perm, lam, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K, hop, log1p, algo, out_bf16=out_bf16)


def forward_train_mix(x, perm, lam, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K: int, hop: int,
                      algo: int = _native.ALGO_AUTO, log1p: bool = False, out_bf16: bool = False) -> torch.Tensor:
    return torch.ops.leaf_amd.forward_train_mix(x, perm, lam, kernel, pool_w, pool_b, alpha, delta, root, ema_w, K, hop, algo, log1p,
                                                out_bf16=out_bf16)[0]
