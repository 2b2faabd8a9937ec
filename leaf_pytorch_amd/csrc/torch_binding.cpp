// torch_binding.cpp -- the "thin torch cpp_extension" over the C ABI (include/leaf_hip.h): registers the fused forward,
// the training forward and the backward as dispatcher ops in the `leaf_amd` namespace, so that
//   * a model containing leaf_pytorch_amd.Leaf traces under torch.compile / torch.export without a graph break
//     (fake kernels + the autograd formula are attached from Python, leaf_pytorch_amd/_ops.py), and
//   * an eager call costs one dispatcher hop instead of ~20 ctypes argument conversions.
// No arithmetic lives here: tensors are checked, outputs and the scratch workspace come from the caching allocator, the
// current HIP stream is handed through, and the matching C-ABI entry point does the work (no fallback of any kind).
// Plain C++ (compiled with g++ against the torch headers); reference counterpart: leaf_pytorch/frontend.py:78-89 and
// what autograd derives for it.
#include <algorithm>
#include <list>
#include <mutex>
#include <tuple>

#include <torch/library.h>
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>      // PyTorch-ROCm presents HIP devices under the "cuda" device type
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPGraphsC10Utils.h>

#include "leaf_hip.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

const float* fptr(const Tensor& t) { return t.data_ptr<float>(); }
const float* fptr(const OptTensor& t) { return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr; }

Tensor dev_f32(const Tensor& t, const char* name, const c10::Device& dev) {
    TORCH_CHECK(t.device() == dev, name, " is on ", t.device(), ", expected ", dev);
    TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32, got ", t.scalar_type());
    return t.contiguous();
}
OptTensor dev_f32(const OptTensor& t, const char* name, const c10::Device& dev) {
    if (!t.has_value() || !t->defined()) return c10::nullopt;
    return dev_f32(*t, name, dev);
}

void check_status(int rc, const char* what) {
    TORCH_CHECK(rc == LEAF_OK, what, " failed: ", leaf_status_string(rc), " (status ", rc, ")");
}

// (B,1,T) or (B,T) -> contiguous (B,T) view of the waveform
Tensor waveform_2d(const Tensor& x) {
    TORCH_CHECK(x.is_cuda(), "leaf_amd: input is on '", x.device(),
                "'. leaf_pytorch_amd runs only on an AMD GPU through its HIP kernels; there is no CPU path in the product");
    TORCH_CHECK(x.dim() == 2 || (x.dim() == 3 && x.size(1) == 1), "expected input of shape (B,1,T), got ", x.sizes());
    return (x.dim() == 3 ? x.select(1, 0) : x).contiguous();
}

// Slices of whole clips for batches beyond one C-ABI call (B * T < 2^31 per call): as few calls as possible, balanced.
struct BatchSlices { int64_t per_call, calls; };
BatchSlices batch_slices(int64_t B, int64_t T) {
    const int64_t most = std::max<int64_t>(1, ((int64_t(1) << 31) - 1) / std::max<int64_t>(T, 1));
    const int64_t calls = std::max<int64_t>(1, (B + most - 1) / most);
    return {(B + calls - 1) / calls, calls};
}

struct Params {
    Tensor kernel, pool_w, pool_b;
    OptTensor alpha, delta, root, ema_w;
    bool pcen;
};
Params gather(const Tensor& kernel, const Tensor& pool_w, const Tensor& pool_b, const OptTensor& alpha, const OptTensor& delta,
              const OptTensor& root, const OptTensor& ema_w, const c10::Device& dev) {
    Params p;
    p.kernel = dev_f32(kernel, "kernel", dev);
    p.pool_w = dev_f32(pool_w.reshape({-1}), "pool_w", dev);
    p.pool_b = dev_f32(pool_b, "pool_b", dev);
    p.pcen = alpha.has_value() && alpha->defined();
    if (p.pcen) {
        p.alpha = dev_f32(alpha, "alpha", dev); p.delta = dev_f32(delta, "delta", dev);
        p.root = dev_f32(root, "root", dev); p.ema_w = dev_f32(ema_w, "ema_w", dev);
        TORCH_CHECK(p.delta && p.root && p.ema_w, "PCEN needs alpha, delta, root and ema_w");
    }
    return p;
}

// ---- One forward and one backward serve the plain ops and the waveform-mixup ops (leaf_hip.h: the *_mix_* entries), which are the same
// code with (perm, lam) present: the ops on x * lam + x[perm] * (1 - lam), the mix done inside the kernels' loads where the family
// has one.  What a mixed call does differently: x float32 or int16 PCM only (no bfloat16 waveform); perm int32 [B] and lam float32 [B]
// on x's device (the Python layer converts and validates, leaf_pytorch_amd/_native.py: mix_args); ONE C-ABI call -- a mixed batch
// cannot be sliced (a clip's partner may sit in another slice), so B * T >= 2^31 is refused; no g_x.
struct Mix { const Tensor& perm; const Tensor& lam; };
struct Call {
    Tensor x2, perm, lam;          // perm / lam: defined for a mixed call only
    bool mixed, io_bf16, pcm16;
    int64_t B;
    int T, F, TP;
};
Call make_call(const Tensor& x, const Mix* mix, const Params& p, int64_t K, int64_t hop, bool check_frames) {
    Call c;
    c.x2 = waveform_2d(x);
    c.mixed = mix != nullptr;
    c.io_bf16 = c.x2.scalar_type() == at::kBFloat16;
    c.pcm16 = c.x2.scalar_type() == at::kShort;                // 16-bit PCM in (a sample v means v / 32768), float32 out
    c.B = c.x2.size(0);
    if (mix) {
        TORCH_CHECK(c.x2.scalar_type() == at::kFloat || c.pcm16,
                    "mixup is defined in float32 on a float32 or int16 (PCM) waveform, got ", c.x2.scalar_type());
        TORCH_CHECK(c.x2.size(1) < (int64_t(1) << 31) && c.B * c.x2.size(1) < (int64_t(1) << 31),
                    "a mixed batch goes through one C-ABI call: B * T must stay below 2^31, got ", c.B, " x ", c.x2.size(1));
    } else {
        TORCH_CHECK(c.io_bf16 || c.pcm16 || c.x2.scalar_type() == at::kFloat,
                    "x must be float32 (or bfloat16 for the bf16-I/O extension, or int16 PCM), got ", c.x2.scalar_type());
        TORCH_CHECK(c.x2.size(1) < (int64_t(1) << 31), "a clip of ", c.x2.size(1), " samples is beyond the C ABI's 32-bit sample index");
    }
    c.T = (int)c.x2.size(1); c.F = (int)p.kernel.size(0);
    c.TP = leaf_num_frames(c.T, (int)K, (int)hop);
    if (check_frames) TORCH_CHECK(c.TP >= 1 && c.F >= 1, "bad shape B=", c.B, " T=", c.T, " F=", c.F, " K=", K, " hop=", hop);
    if (mix) {
        TORCH_CHECK(mix->perm.device() == c.x2.device() && mix->perm.scalar_type() == at::kInt && mix->perm.numel() == c.B,
                    "perm must be int32 with one entry per clip on ", c.x2.device());
        c.perm = mix->perm.reshape({-1}).contiguous();
        c.lam = dev_f32(mix->lam.reshape({-1}), "lam", c.x2.device());
        TORCH_CHECK(c.lam.numel() == c.B, "lam must have one entry per clip");
    }
    return c;
}
// Slices of the batch, one C-ABI call each.  The C ABI indexes the samples of ONE call with 32 bits and refuses B * T >= 2^31
// (LEAF_ERR_BAD_SHAPE); the reference's conv1d takes any batch (frontend.py:78-89).  Clips are independent, so a larger batch goes
// through in balanced slices of whole clips into the one preallocated output: the bits of a clip do not depend on its slice (within
// one kernel family; the slices are far beyond every AUTO threshold).  A mixed batch is one slice (make_call has refused the rest).
BatchSlices call_slices(const Call& c) { return c.mixed ? BatchSlices{c.B, 1} : batch_slices(c.B, c.T); }
// element offset into a float32 / bfloat16 / int16 I/O tensor, as the C ABI's float pointer
float* io_at(const Tensor& t, size_t elems) {
    return reinterpret_cast<float*>(static_cast<char*>(t.data_ptr()) + elems * (size_t)t.element_size());
}

// ---- The table caches of the no-grad forward (leaf_hip.h: leaf_forward_cached_f32).  A small per-process LRU of zero-filled device
// buffers; the key only FINDS a candidate buffer -- whether its tables are valid is decided on the device, by content, in the table
// launch of every call.  The stream is part of the key so that two streams never share a buffer.  The list is never destroyed (a
// static destructor would free device memory after the runtime has gone).
struct TableCaches {
    using Key = std::tuple<int, int64_t, const void*, const void*, int, int, int, int>;   // device, stream, kernel, pool_w, F, K, hop, T
    static constexpr size_t kEntries = 8;
    std::mutex mu;
    std::list<std::pair<Key, Tensor>> lru;                     // most recently used first
    int64_t cached_calls = 0, created = 0;
    Tensor get(const Key& key, size_t bytes, const at::TensorOptions& byte_opt) {
        std::lock_guard<std::mutex> lock(mu);
        ++cached_calls;
        for (auto it = lru.begin(); it != lru.end(); ++it)
            if (it->first == key && (size_t)it->second.numel() == bytes) {
                lru.splice(lru.begin(), lru, it);
                return lru.front().second;
            }
        lru.emplace_front(key, at::zeros({(int64_t)bytes}, byte_opt));
        ++created;
        if (lru.size() > kEntries) lru.pop_back();
        return lru.front().second;
    }
};
TableCaches& table_caches() {
    static TableCaches* c = new TableCaches();
    return *c;
}
// [buffers held, calls sent through leaf_forward_cached_f32, buffers created] -- for tests and tools
std::vector<int64_t> op_table_cache_info() {
    TableCaches& c = table_caches();
    std::lock_guard<std::mutex> lock(c.mu);
    return {(int64_t)c.lru.size(), c.cached_calls, c.created};
}

// out_bf16 (LEAF_FLAG_OUT_BF16): bfloat16 features from a float32 or int16 waveform, narrowed where the kernels store them; an explicit
// argument of the ops, never inferred from a tensor (redundant for a bfloat16 x)
Tensor forward_impl(const Tensor& x, const Mix* mix, const Params& p, int64_t K, int64_t hop, bool log1p, int64_t algo, Tensor* raw,
                    bool out_bf16) {
    const Call c = make_call(x, mix, p, K, hop, /*check_frames=*/true);
    const int64_t B = c.B;
    const int T = c.T, F = c.F, TP = c.TP;
    out_bf16 = out_bf16 && !c.io_bf16;
    const auto f32_opt = c.x2.options().dtype(at::kFloat);
    const auto out_opt = f32_opt.dtype(c.io_bf16 || out_bf16 ? at::kBFloat16 : at::kFloat);
    if (raw) *raw = at::empty({B, F, TP}, f32_opt);
    // the empty batch: the reference returns (0, F, T') (frontend.py:78-89 -> convolution.py:97); nothing is launched
    if (B == 0) return at::empty({0, F, TP}, out_opt);
    int flags = (c.io_bf16 ? LEAF_FLAG_IO_BF16 : 0) | (c.pcm16 ? LEAF_FLAG_X_PCM16 : 0) | (out_bf16 ? LEAF_FLAG_OUT_BF16 : 0) |
                (p.pcen ? LEAF_FLAG_PCEN : (log1p ? LEAF_FLAG_LOG1P : 0));
    // call options travelling in the upper bits of the op's `algo` argument (the schema stays as it is): bit 24 = the
    // PeakNormalization prologue folded into the forward (LEAF_FLAG_PEAKNORM; inference only, the plain ops only)
    constexpr int64_t kOptPeakNorm = int64_t(1) << 24;
    algo &= ~(int64_t(1) << 29);                               // OPT_FULL_BACKWARD: read by the autograd formula (_ops.py) alone
    if (!c.mixed && (algo & kOptPeakNorm)) {
        TORCH_CHECK(!raw, "the fused PeakNormalization prologue is forward-only");
        if (!c.pcm16) flags |= LEAF_FLAG_PEAKNORM;              // (|v / 32768| <= 1: nothing to normalise, nothing launched)
        algo &= ~kOptPeakNorm;
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(c.x2.device());
    auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(c.x2.device().index());
    const BatchSlices sl = call_slices(c);
    const int last = (int)(B - (sl.calls - 1) * sl.per_call);
    bool pcm16_staged = false, bf16_staged = false;
    if (c.pcm16 || out_bf16) {
        // the staged forward reads and writes float32 only (LEAF_ERR_UNSUPPORTED from the C ABI): where the call lands on it, each
        // slice of an int16 batch is converted below -- the same values, v / 32768 exactly (a mixed call: mixup_kernel widens) -- and
        // bfloat16 features are narrowed from its float32 result at the end (the same rounding, the same bits)
        int sel = (int)(algo & 0xff);
        if (sel == LEAF_ALGO_AUTO) sel = leaf_auto_algo((int)std::min<int64_t>(B, sl.per_call), T, F, (int)K, (int)hop);
        pcm16_staged = c.pcm16 && !c.mixed && sel == LEAF_ALGO_STAGED;
        bf16_staged = out_bf16 && sel == LEAF_ALGO_STAGED;
        if (pcm16_staged) flags &= ~LEAF_FLAG_X_PCM16;
        if (bf16_staged) flags &= ~LEAF_FLAG_OUT_BF16;
    }
    Tensor out = at::empty({B, F, TP}, bf16_staged ? f32_opt : out_opt);
    // One workspace, sized for the largest slice, serves the stream-ordered calls in turn.
    auto ws_bytes = [&](int nb) {
        return c.mixed ? leaf_forward_mix_workspace_bytes(nb, T, F, (int)K, (int)hop, (int)algo) : leaf_workspace_bytes(nb, T, F, (int)K, (int)hop, (int)algo);
    };
    Tensor ws = at::empty({(int64_t)std::max<size_t>({ws_bytes((int)sl.per_call), ws_bytes(last), size_t(4)})}, f32_opt.dtype(at::kByte));
    void* wsp = ws.data_ptr();
    const size_t wsn = (size_t)ws.numel();
    const float *pk = fptr(p.kernel), *pw = fptr(p.pool_w), *pb = fptr(p.pool_b), *pa = fptr(p.alpha), *pd = fptr(p.delta), *pr = fptr(p.root),
                *pe = fptr(p.ema_w);
    // The no-grad forward keeps the tables of the 2048-sample plan in a self-validating cache (leaf_forward_cached_f32).  Not while the
    // stream is being captured (a captured graph must not allocate or depend on a buffer of this list), not on the training forward, not
    // for a mixed or peak-normalised call, not with LEAF_ALGO_NO_TABLE_CACHE: those take today's path.  (Fake and meta tensors never
    // reach this function: their kernels are registered from Python.)
    const bool cacheable = !raw && !c.mixed && !(flags & LEAF_FLAG_PEAKNORM) && !(algo & LEAF_ALGO_NO_TABLE_CACHE) && !pcm16_staged &&
                           c10::hip::currentStreamCaptureStatusMayInitCtx() == c10::hip::CaptureStatus::None;
    const size_t cache_bytes = cacheable ? leaf_table_cache_bytes(F, (int)K, (int)hop, T) : 0;
    for (int64_t b0 = 0; b0 < B; b0 += sl.per_call) {
        const int nb = (int)std::min<int64_t>(sl.per_call, B - b0);
        Tensor cache;                                           // only where the slice lands on a kernel of the 2048-sample plan
        if (cache_bytes) {
            int sel = (int)(algo & 0xff), info[8] = {0};
            if (sel == LEAF_ALGO_AUTO) sel = leaf_auto_algo(nb, T, F, (int)K, (int)hop);
            const bool plan4k = sel == LEAF_ALGO_FFT_WG && leaf_fft_plan_info(nb, T, F, (int)K, (int)hop, info) == LEAF_OK && info[0] != 2048;
            if ((sel == LEAF_ALGO_FFT || sel == LEAF_ALGO_FFT_WG) && !plan4k)
                cache = table_caches().get(TableCaches::Key{(int)c.x2.device().index(), (int64_t)stream.id(), pk, pw, F, (int)K, (int)hop, T},
                                           cache_bytes, f32_opt.dtype(at::kByte));
        }
        Tensor xs;                                              // one slice of an int16 batch as float32, for the staged forward
        if (pcm16_staged) xs = c.x2.narrow(0, b0, nb).to(at::kFloat).mul_(1.0 / 32768.0);
        const float* xin = pcm16_staged ? xs.data_ptr<float>() : io_at(c.x2, (size_t)b0 * T);
        float* o = io_at(out, (size_t)b0 * F * TP);
        float* r = raw ? raw->data_ptr<float>() + (size_t)b0 * F * TP : nullptr;
        if (c.mixed && raw)
            check_status(leaf_forward_save_mix_f32(xin, c.perm.data_ptr<int>(), fptr(c.lam), nb, T, pk, pw, pb, pa, pd, pr, pe, F, (int)K, (int)hop,
                                                   flags, (int)algo, o, r, wsp, wsn, stream.stream()), "leaf_forward_save_mix_f32");
        else if (c.mixed)
            check_status(leaf_forward_mix_f32(xin, c.perm.data_ptr<int>(), fptr(c.lam), nb, T, pk, pw, pb, pa, pd, pr, pe, F, (int)K, (int)hop,
                                              flags, (int)algo, o, wsp, wsn, stream.stream()), "leaf_forward_mix_f32");
        else if (cache.defined())
            check_status(leaf_forward_cached_f32(xin, nb, T, pk, pw, pb, pa, pd, pr, pe, F, (int)K, (int)hop, flags, (int)algo, o, wsp, wsn,
                                                 cache.data_ptr(), (size_t)cache.numel(), stream.stream()), "leaf_forward_cached_f32");
        else if (raw)
            check_status(leaf_forward_save_f32(xin, nb, T, pk, pw, pb, pa, pd, pr, pe, F, (int)K, (int)hop, flags, (int)algo, o, r, wsp, wsn,
                                               stream.stream()), "leaf_forward_save_f32");
        else
            check_status(leaf_forward_f32(xin, nb, T, pk, pw, pb, pa, pd, pr, pe, F, (int)K, (int)hop, flags, (int)algo, o, wsp, wsn,
                                          stream.stream()), "leaf_forward_f32");
    }
    return bf16_staged ? out.to(at::kBFloat16) : out;
}

// What autograd derives for frontend.py:78-89: (g_kernel, g_pool_w, g_pool_b, g_alpha, g_delta, g_root, g_ema_w[, g_x]); the PCEN
// entries are empty tensors without PCEN; the plain op appends g_x (empty unless need_dx), a mixed call has none.  `flags` are C-ABI
// flags (LEAF_FLAG_BWD_*, and LEAF_FLAG_LOG1P for the backward of the log1p-compressed forward); LEAF_FLAG_PCEN and
// LEAF_FLAG_IO_BF16 / LEAF_FLAG_X_PCM16 follow from the tensors.  bfloat16 x: grad_out is bfloat16 too, g_x comes back in
// bfloat16, the parameter gradients and pooled_raw are float32.  int16 x (PCM): grad_out float32, need_dx refused.
// out_bf16 (LEAF_FLAG_OUT_BF16): grad_out alone is bfloat16, for a float32 (g_x float32) or int16 x.
std::vector<Tensor> backward_impl(const Tensor& x, const Mix* mix, const Params& p, const Tensor& pool_w, int64_t K, int64_t hop,
                                  const Tensor& grad_out, const OptTensor& pooled_raw, bool need_dx, int64_t flags, bool out_bf16) {
    const Call c = make_call(x, mix, p, K, hop, /*check_frames=*/mix != nullptr);
    TORCH_CHECK(!(c.pcm16 && need_dx), "an int16 (PCM) input has no gradient: need_dx needs a float32 or bfloat16 x");
    const int64_t B = c.B;
    const int T = c.T, F = c.F, TP = c.TP;
    out_bf16 = out_bf16 && !c.io_bf16;
    Tensor go;
    if (c.io_bf16 || out_bf16) {                              // a bfloat16 grad_out goes straight in: widened where the kernels read it
        TORCH_CHECK(grad_out.device() == c.x2.device(), "grad_out is on ", grad_out.device(), ", expected ", c.x2.device());
        TORCH_CHECK(grad_out.scalar_type() == at::kBFloat16, c.io_bf16 ? "grad_out must be bfloat16 when x is bfloat16, got " : "grad_out must be bfloat16 with out_bf16=True, got ",
                    grad_out.scalar_type());
        go = grad_out.contiguous();
    } else {
        go = dev_f32(grad_out, "grad_out", c.x2.device());
    }
    TORCH_CHECK(go.dim() == 3 && go.size(0) == B && go.size(1) == F && go.size(2) == TP, "grad_out has shape ", go.sizes(),
                ", expected (", B, ",", F, ",", TP, ")");
    OptTensor raw = dev_f32(pooled_raw, "pooled_raw", c.x2.device());
    c10::hip::HIPGuardMasqueradingAsCUDA guard(c.x2.device());
    auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(c.x2.device().index());
    auto opt = c.x2.options().dtype(at::kFloat);              // parameter gradients are float32 whatever the I/O type
    Tensor gk = at::empty_like(p.kernel), gpw = at::empty_like(p.pool_w), gpb = at::empty_like(p.pool_b);
    Tensor ga = at::empty({p.pcen ? F : 0}, opt), gd = at::empty({p.pcen ? F : 0}, opt), gr = at::empty({p.pcen ? F : 0}, opt),
           gw = at::empty({p.pcen ? F : 0}, opt);
    Tensor gx = need_dx ? at::empty_like(c.x2) : at::empty({0}, opt);
    auto result = [&]() {
        std::vector<Tensor> g{gk, gpw.reshape(pool_w.sizes()), gpb, ga, gd, gr, gw};
        if (!c.mixed) g.push_back(need_dx ? gx.reshape(x.sizes()) : gx);
        return g;
    };
    if (B == 0) {                                             // the sum over no clips (C ABI: zero-fills, launches nothing else)
        for (Tensor* g : {&gk, &gpw, &gpb, &ga, &gd, &gr, &gw}) g->zero_();
        return result();
    }
    const int fl = ((int)flags & ~(LEAF_FLAG_PCEN | LEAF_FLAG_IO_BF16 | LEAF_FLAG_X_PCM16 | LEAF_FLAG_OUT_BF16)) | (p.pcen ? LEAF_FLAG_PCEN : 0) |
                   (c.io_bf16 ? LEAF_FLAG_IO_BF16 : 0) | (c.pcm16 ? LEAF_FLAG_X_PCM16 : 0) | (out_bf16 ? LEAF_FLAG_OUT_BF16 : 0);
    // B * T >= 2^31: slices of whole clips as in the forward; the parameter gradients of the slices are added in slice order
    // (a fixed order: the step stays bit-reproducible), dL/dx is written slice by slice
    const BatchSlices sl = call_slices(c);
    const int last = (int)(B - (sl.calls - 1) * sl.per_call);
    auto ws_bytes = [&](int nb) {
        return c.mixed ? leaf_backward_mix_workspace_bytes(nb, T, F, (int)K, (int)hop, fl)
                       : leaf_backward_workspace_bytes(nb, T, F, (int)K, (int)hop, fl, need_dx ? 1 : 0);
    };
    Tensor ws = at::empty({(int64_t)std::max<size_t>({ws_bytes((int)sl.per_call), ws_bytes(last), size_t(4)})}, opt.dtype(at::kByte));
    Tensor tk, tpw, tpb, ta, td, tr, tw;
    if (sl.calls > 1) {
        tk = at::empty_like(gk); tpw = at::empty_like(gpw); tpb = at::empty_like(gpb);
        ta = at::empty_like(ga); td = at::empty_like(gd); tr = at::empty_like(gr); tw = at::empty_like(gw);
    }
    for (int64_t b0 = 0; b0 < B; b0 += sl.per_call) {
        const int nb = (int)std::min<int64_t>(sl.per_call, B - b0);
        const bool first = b0 == 0;
        Tensor &k_ = first ? gk : tk, &pw_ = first ? gpw : tpw, &pb_ = first ? gpb : tpb, &a_ = first ? ga : ta, &d_ = first ? gd : td,
               &r_ = first ? gr : tr, &w_ = first ? gw : tw;
        const float* rawp = raw ? fptr(raw) + (size_t)b0 * F * TP : nullptr;
        float *pa = p.pcen ? a_.data_ptr<float>() : nullptr, *pd = p.pcen ? d_.data_ptr<float>() : nullptr,
              *pr = p.pcen ? r_.data_ptr<float>() : nullptr, *pw = p.pcen ? w_.data_ptr<float>() : nullptr;
        if (c.mixed)
            check_status(leaf_backward_mix_f32(io_at(c.x2, (size_t)b0 * T), c.perm.data_ptr<int>(), fptr(c.lam), nb, T, fptr(p.kernel),
                                               fptr(p.pool_w), fptr(p.pool_b), fptr(p.alpha), fptr(p.delta), fptr(p.root), fptr(p.ema_w), F,
                                               (int)K, (int)hop, fl, io_at(go, (size_t)b0 * F * TP), rawp, k_.data_ptr<float>(),
                                               pw_.data_ptr<float>(), pb_.data_ptr<float>(), pa, pd, pr, pw, nullptr, ws.data_ptr(),
                                               (size_t)ws.numel(), stream.stream()), "leaf_backward_mix_f32");
        else
            check_status(leaf_backward_f32(io_at(c.x2, (size_t)b0 * T), nb, T, fptr(p.kernel), fptr(p.pool_w), fptr(p.pool_b), fptr(p.alpha),
                                           fptr(p.delta), fptr(p.root), fptr(p.ema_w), F, (int)K, (int)hop, fl,
                                           io_at(go, (size_t)b0 * F * TP), rawp, k_.data_ptr<float>(), pw_.data_ptr<float>(),
                                           pb_.data_ptr<float>(), pa, pd, pr, pw, need_dx ? io_at(gx, (size_t)b0 * T) : nullptr,
                                           ws.data_ptr(), (size_t)ws.numel(), stream.stream()), "leaf_backward_f32");
        if (!first) {
            gk.add_(tk); gpw.add_(tpw); gpb.add_(tpb);
            if (p.pcen) { ga.add_(ta); gd.add_(td); gr.add_(tr); gw.add_(tw); }
        }
    }
    return result();
}

// The head-only backward (leaf_hip.h: leaf_backward_head_f32): (g_pool_b, g_alpha, g_delta, g_root, g_ema_w) from the saved pre-floor
// pooled tensor and grad_out alone -- what a Leaf whose Gabor kernel and pooling width are frozen needs.  pool_b gives the shape and
// the device of its gradient, nothing else; the PCEN entries are empty tensors without PCEN.  `flags`: LEAF_FLAG_LOG1P (PCEN off);
// LEAF_FLAG_PCEN follows from the tensors.  out_bf16: grad_out is bfloat16 (bfloat16 features, from whatever waveform).
// B * F * T' >= 2^31: slices over B, the gradients of the slices added in slice order.
std::vector<Tensor> op_backward_head(const Tensor& pooled_raw, const Tensor& grad_out, const Tensor& pool_b, const OptTensor& alpha,
                                     const OptTensor& delta, const OptTensor& root, const OptTensor& ema_w, int64_t flags, bool out_bf16) {
    TORCH_CHECK(pooled_raw.is_cuda(), "leaf_amd::backward_head: pooled_raw is on '", pooled_raw.device(),
                "'. leaf_pytorch_amd runs only on an AMD GPU through its HIP kernels; there is no CPU path in the product");
    const auto dev = pooled_raw.device();
    TORCH_CHECK(pooled_raw.dim() == 3, "pooled_raw must be (B, F, T'), got ", pooled_raw.sizes());
    const Tensor raw = dev_f32(pooled_raw, "pooled_raw", dev);
    const int64_t B = raw.size(0), F = raw.size(1), TP = raw.size(2);
    TORCH_CHECK(F >= 1 && TP >= 1 && F * TP < (int64_t(1) << 31), "bad shape B=", B, " F=", F, " T'=", TP);
    Tensor go;
    if (out_bf16) {
        TORCH_CHECK(grad_out.device() == dev, "grad_out is on ", grad_out.device(), ", expected ", dev);
        TORCH_CHECK(grad_out.scalar_type() == at::kBFloat16, "grad_out must be bfloat16 with out_bf16=True, got ", grad_out.scalar_type());
        go = grad_out.contiguous();
    } else {
        go = dev_f32(grad_out, "grad_out", dev);
    }
    TORCH_CHECK(go.sizes() == raw.sizes(), "grad_out has shape ", go.sizes(), ", expected ", raw.sizes());
    TORCH_CHECK(pool_b.device() == dev && pool_b.numel() == F, "pool_b must hold one bias per filter on ", dev);
    const bool pcen = alpha.has_value() && alpha->defined();
    OptTensor a, d, r, w;
    if (pcen) {
        a = dev_f32(alpha, "alpha", dev); d = dev_f32(delta, "delta", dev); r = dev_f32(root, "root", dev); w = dev_f32(ema_w, "ema_w", dev);
        TORCH_CHECK(d && r && w, "PCEN needs alpha, delta, root and ema_w");
        TORCH_CHECK(a->numel() == F && d->numel() == F && r->numel() == F && w->numel() == F, "the PCEN vectors must hold one entry per filter");
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index());
    auto opt = raw.options();
    const int64_t np = pcen ? F : 0;
    Tensor gb = at::empty(pool_b.sizes(), opt), ga = at::empty({np}, opt), gd = at::empty({np}, opt), gr = at::empty({np}, opt),
           gw = at::empty({np}, opt);
    if (B == 0) {
        for (Tensor* g : {&gb, &ga, &gd, &gr, &gw}) g->zero_();
        return {gb, ga, gd, gr, gw};
    }
    const int fl = (pcen ? LEAF_FLAG_PCEN : ((int)flags & LEAF_FLAG_LOG1P)) | (out_bf16 ? LEAF_FLAG_OUT_BF16 : 0);
    const BatchSlices sl = batch_slices(B, F * TP);
    const int last = (int)(B - (sl.calls - 1) * sl.per_call);
    auto ws_bytes = [&](int nb) { return leaf_backward_head_workspace_bytes(nb, (int)TP, (int)F, fl); };
    Tensor ws = at::empty({(int64_t)std::max<size_t>({ws_bytes((int)sl.per_call), ws_bytes(last), size_t(4)})}, opt.dtype(at::kByte));
    Tensor tb, ta, td, tr, tw;
    if (sl.calls > 1) {
        tb = at::empty_like(gb); ta = at::empty_like(ga); td = at::empty_like(gd); tr = at::empty_like(gr); tw = at::empty_like(gw);
    }
    for (int64_t b0 = 0; b0 < B; b0 += sl.per_call) {
        const int nb = (int)std::min<int64_t>(sl.per_call, B - b0);
        const bool first = b0 == 0;
        Tensor &b_ = first ? gb : tb, &a_ = first ? ga : ta, &d_ = first ? gd : td, &r_ = first ? gr : tr, &w_ = first ? gw : tw;
        check_status(leaf_backward_head_f32(fptr(raw) + (size_t)b0 * F * TP, io_at(go, (size_t)b0 * F * TP), nb, (int)TP, (int)F, fptr(a),
                                            fptr(d), fptr(r), fptr(w), fl, b_.data_ptr<float>(), pcen ? a_.data_ptr<float>() : nullptr,
                                            pcen ? d_.data_ptr<float>() : nullptr, pcen ? r_.data_ptr<float>() : nullptr,
                                            pcen ? w_.data_ptr<float>() : nullptr, ws.data_ptr(), (size_t)ws.numel(), stream.stream()),
                     "leaf_backward_head_f32");
        if (!first) {
            gb.add_(tb);
            if (pcen) { ga.add_(ta); gd.add_(td); gr.add_(tr); gw.add_(tw); }
        }
    }
    return {gb, ga, gd, gr, gw};
}

// ---- the six ops: leaf_amd::forward -- frontend.py:78-89 (inference / no-grad); forward_train -- the same, additionally returning
// the pre-floor pooled tensor the backward consumes; backward; and the three on the mixed batch (forward_mix, forward_train_mix,
// backward_mix: the seven parameter gradients, no dL/dx)
#define LEAF_PARAM_ARGS const Tensor &kernel, const Tensor &pool_w, const Tensor &pool_b, const OptTensor &alpha, const OptTensor &delta, \
                        const OptTensor &root, const OptTensor &ema_w
#define LEAF_GATHER gather(kernel, pool_w, pool_b, alpha, delta, root, ema_w, x.device())
Tensor op_forward(const Tensor& x, LEAF_PARAM_ARGS, int64_t K, int64_t hop, bool log1p, int64_t algo, bool out_bf16) {
    return forward_impl(x, nullptr, LEAF_GATHER, K, hop, log1p, algo, nullptr, out_bf16);
}
std::tuple<Tensor, Tensor> op_forward_train(const Tensor& x, LEAF_PARAM_ARGS, int64_t K, int64_t hop, int64_t algo, bool log1p, bool out_bf16) {
    Tensor raw;
    Tensor out = forward_impl(x, nullptr, LEAF_GATHER, K, hop, log1p, algo, &raw, out_bf16);
    return {out, raw};
}
std::vector<Tensor> op_backward(const Tensor& x, LEAF_PARAM_ARGS, int64_t K, int64_t hop, const Tensor& grad_out, const OptTensor& pooled_raw,
                                bool need_dx, int64_t flags, bool out_bf16) {
    return backward_impl(x, nullptr, LEAF_GATHER, pool_w, K, hop, grad_out, pooled_raw, need_dx, flags, out_bf16);
}
Tensor op_forward_mix(const Tensor& x, const Tensor& perm, const Tensor& lam, LEAF_PARAM_ARGS, int64_t K, int64_t hop, bool log1p,
                      int64_t algo, bool out_bf16) {
    const Mix mix{perm, lam};
    return forward_impl(x, &mix, LEAF_GATHER, K, hop, log1p, algo, nullptr, out_bf16);
}
std::tuple<Tensor, Tensor> op_forward_train_mix(const Tensor& x, const Tensor& perm, const Tensor& lam, LEAF_PARAM_ARGS, int64_t K,
                                                int64_t hop, int64_t algo, bool log1p, bool out_bf16) {
    const Mix mix{perm, lam};
    Tensor raw;
    Tensor out = forward_impl(x, &mix, LEAF_GATHER, K, hop, log1p, algo, &raw, out_bf16);
    return {out, raw};
}
std::vector<Tensor> op_backward_mix(const Tensor& x, const Tensor& perm, const Tensor& lam, LEAF_PARAM_ARGS, int64_t K, int64_t hop,
                                    const Tensor& grad_out, const OptTensor& pooled_raw, int64_t flags, bool out_bf16) {
    const Mix mix{perm, lam};
    return backward_impl(x, &mix, LEAF_GATHER, pool_w, K, hop, grad_out, pooled_raw, /*need_dx=*/false, flags, out_bf16);
}
#undef LEAF_PARAM_ARGS
#undef LEAF_GATHER

}  // namespace

TORCH_LIBRARY(leaf_amd, m) {
    m.def("forward(Tensor x, Tensor kernel, Tensor pool_w, Tensor pool_b, Tensor? alpha, Tensor? delta, Tensor? root, "
          "Tensor? ema_w, int K, int hop, bool log1p, int algo, *, bool out_bf16=False) -> Tensor");
    m.def("forward_train(Tensor x, Tensor kernel, Tensor pool_w, Tensor pool_b, Tensor? alpha, Tensor? delta, Tensor? root, "
          "Tensor? ema_w, int K, int hop, int algo, bool log1p=False, *, bool out_bf16=False) -> (Tensor, Tensor)");
    m.def("backward(Tensor x, Tensor kernel, Tensor pool_w, Tensor pool_b, Tensor? alpha, Tensor? delta, Tensor? root, "
          "Tensor? ema_w, int K, int hop, Tensor grad_out, Tensor? pooled_raw, bool need_dx, int flags, *, bool out_bf16=False) -> Tensor[]");
    m.def("forward_mix(Tensor x, Tensor perm, Tensor lam, Tensor kernel, Tensor pool_w, Tensor pool_b, Tensor? alpha, Tensor? delta, "
          "Tensor? root, Tensor? ema_w, int K, int hop, bool log1p, int algo, *, bool out_bf16=False) -> Tensor");
    m.def("forward_train_mix(Tensor x, Tensor perm, Tensor lam, Tensor kernel, Tensor pool_w, Tensor pool_b, Tensor? alpha, "
          "Tensor? delta, Tensor? root, Tensor? ema_w, int K, int hop, int algo, bool log1p=False, *, bool out_bf16=False) -> (Tensor, Tensor)");
    m.def("backward_mix(Tensor x, Tensor perm, Tensor lam, Tensor kernel, Tensor pool_w, Tensor pool_b, Tensor? alpha, Tensor? delta, "
          "Tensor? root, Tensor? ema_w, int K, int hop, Tensor grad_out, Tensor? pooled_raw, int flags, *, bool out_bf16=False) -> Tensor[]");
    m.def("backward_head(Tensor pooled_raw, Tensor grad_out, Tensor pool_b, Tensor? alpha, Tensor? delta, Tensor? root, Tensor? ema_w, "
          "int flags, *, bool out_bf16=False) -> Tensor[]");
    m.def("table_cache_info() -> int[]", &op_table_cache_info);
}

// HIP tensors dispatch under the CUDA key in PyTorch-ROCm
TORCH_LIBRARY_IMPL(leaf_amd, CUDA, m) {
    m.impl("forward", &op_forward);
    m.impl("forward_train", &op_forward_train);
    m.impl("backward", &op_backward);
    m.impl("forward_mix", &op_forward_mix);
    m.impl("forward_train_mix", &op_forward_train_mix);
    m.impl("backward_mix", &op_backward_mix);
    m.impl("backward_head", &op_backward_head);
}
