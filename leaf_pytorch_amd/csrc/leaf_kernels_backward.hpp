// leaf_kernels_backward.hpp -- the staged backward's kernels (pooling and convolution transposes, chain to (mu, sigma)) and the
// reductions behind the tap-gradient GEMM of leaf_backward.hpp
// Included by leaf_kernels.hip only: kernels (see leaf_kernels_tables.hpp).
#pragma once
#include "leaf_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// backward (staged, correctness-first): gradients of a scalar loss w.r.t. the seven parameters (and
// optionally x) given dL/d out.  Every forward intermediate is recomputed on the device with the staged
// kernels above; nothing is kept from the forward call.  Mirrors what autograd derives for the reference
// graph (frontend.py:78-89), including its clamp sub-gradients:
//   torch.clamp  -> gradient passes where lo <= x <= hi          (convolution.py:19-20, impulse_responses.py:75,
//                                                                  postprocessing.py:14)
//   torch.min/max against a scalar tensor -> the selected side; an exact tie splits 1/2 (postprocessing.py:63-64)
//   torch.maximum(p, 1e-5)               -> passes where p > 1e-5 (frontend.py:84)
// ---------------------------------------------------------------------------------------------

// d e[b,f,n] = sum_m g[f][n + padL - m hop] * gpre[b,f,m]  (transpose of pooling.py:41), then
// dy[b,2f,n] = 2 y_re de, dy[b,2f+1,n] = 2 y_im de written over y  (frontend.py:15-19).
__global__ void pool_bwd_dy_kernel(float* __restrict__ y, const float* __restrict__ g, const float* __restrict__ gpre,
                                   int F, int T, int TP, int K, int hop, int padL) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y, b = blockIdx.z;
    if (n >= T) return;
    const float* w = g + (size_t)f * K;
    const float* gp = gpre + ((size_t)b * F + f) * TP;
    const int np = n + padL;
    const int m_hi = min(TP - 1, np / hop);
    const int m_lo = max(0, (np - K + hop) / hop);          // smallest m with np - m*hop <= K-1
    float de = 0.0f;
    for (int m = m_lo; m <= m_hi; ++m) {
        const int j = np - m * hop;
        if (j >= 0 && j < K) de = fmaf(w[j], gp[m], de);
    }
    const size_t ire = ((size_t)b * 2 * F + 2 * f) * T + n;
    y[ire] *= 2.0f * de;
    y[ire + T] *= 2.0f * de;
}

// dg[f][j] = sum_{b,m} gpre[b,f,m] * ez[b,f,m hop + j - padL]
__global__ void pool_bwd_dg_kernel(const float* __restrict__ e, const float* __restrict__ gpre, int B, int F, int T, int TP,
                                   int K, int hop, int padL, float* __restrict__ dg) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (j >= K) return;
    float acc = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float* eb = e + ((size_t)b * F + f) * T;
        const float* gp = gpre + ((size_t)b * F + f) * TP;
        for (int m = 0; m < TP; ++m) {
            const int n = m * hop + j - padL;
            if (n >= 0 && n < T) acc = fmaf(gp[m], eb[n], acc);
        }
    }
    dg[(size_t)f * K + j] = acc;
}

// dtaps partial per clip: part[b][c][j] = sum_n dy[b,c,n] * xz[b, n + j - padL]   (transpose of convolution.py:97 w.r.t. weights)
__global__ void dtaps_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x, int T, int C, int K, int padL,
                                     float* __restrict__ part) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (j >= K) return;
    const float* d = dy + ((size_t)b * C + c) * T;
    const float* xb = x + (size_t)b * T;
    const int off = j - padL;
    const int n0 = max(0, -off), n1 = min(T, T - off);
    float acc = 0.0f;
    for (int n = n0; n < n1; ++n) acc = fmaf(d[n], xb[n + off], acc);
    part[((size_t)b * C + c) * K + j] = acc;
}

// One block per filter: sum the per-clip tap gradients over the batch and chain them through the Gabor formula
// (impulse_responses.py:5-16) to (mu, sigma):  d hr/d mu = -t hi, d hi/d mu = t hr, d h/d sigma = h (t^2/s^3 - 1/s).
__global__ void dkernel_kernel(const float* __restrict__ part, const float* __restrict__ taps,
                               const float* __restrict__ kernel, int B, int F, int K, GaborBounds bd,
                               float* __restrict__ g_kernel) {
    __shared__ float red[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const float mu_raw = kernel[2 * f], sg_raw = kernel[2 * f + 1];
    const float sg = fminf(fmaxf(sg_raw, bd.sigma_lo), bd.sigma_hi);
    float a_mu = 0.0f, a_sg = 0.0f;
    for (int j = tid; j < K; j += 256) {
        float dre = 0.0f, dim = 0.0f;
        for (int b = 0; b < B; ++b) {
            dre += part[((size_t)b * 2 * F + 2 * f) * K + j];
            dim += part[((size_t)b * 2 * F + 2 * f + 1) * K + j];
        }
        const float t = (float)(j - K / 2);
        const float hr = taps[(size_t)(2 * f) * K + j], hi = taps[(size_t)(2 * f + 1) * K + j];
        a_mu += t * (dim * hr - dre * hi);
        a_sg += (dre * hr + dim * hi) * (t * t / (sg * sg * sg) - 1.0f / sg);
    }
    float out2[2];
    float vals[2] = {a_mu, a_sg};
    for (int q = 0; q < 2; ++q) {
        red[tid] = vals[q];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        out2[q] = red[0];
        __syncthreads();
    }
    if (tid == 0) {
        g_kernel[2 * f] = (mu_raw >= 0.0f && mu_raw <= 3.14159274101257324f) ? out2[0] : 0.0f;
        g_kernel[2 * f + 1] = (sg_raw >= bd.sigma_lo && sg_raw <= bd.sigma_hi) ? out2[1] : 0.0f;
    }
}

// dx[b,i] = sum_c sum_j taps[c][j] * dy[b,c,i - j + padL]
__global__ void dx_kernel(const float* __restrict__ dy, const float* __restrict__ taps, int T, int C, int K, int padL,
                          void* __restrict__ dx, int out_bf16 = 0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= T) return;
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float* d = dy + ((size_t)b * C + c) * T;
        const float* w = taps + (size_t)c * K;
        const int j0 = max(0, i + padL - (T - 1)), j1 = min(K, i + padL + 1);
        for (int j = j0; j < j1; ++j) acc = fmaf(w[j], d[i + padL - j], acc);
    }
    io_store(dx, (size_t)b * T + i, out_bf16, acc);
}

// sum the per-workgroup partial dH slabs: out[i] = sum_w part[w][i]
__global__ void dh_reduce_kernel(const float* __restrict__ part, int nparts, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = 0.0f;
    for (int w = 0; w < nparts; ++w) acc += part[(size_t)w * n + i];
    out[i] = acc;
}

// One block per filter: sum the workgroup partials of dH and chain through the Gabor formula using the tap table
// itself (W = h * scale, and the scale cancels): d mu = sum_kk kk (dH_im W_re - dH_re W_im),
// d sigma = sum_kk (dH_re W_re + dH_im W_im) (kk^2/s^3 - 1/s); clamp sub-gradients as torch.clamp.
__global__ void dkernel_fused_kernel(const float* __restrict__ dHpart, int nparts, int Rp, const float* __restrict__ W,
                                     int R, int FP, const int* __restrict__ col_of, const float* __restrict__ kernel,
                                     int F, GaborBounds bd, float* __restrict__ g_kernel) {
    (void)F;
    __shared__ float red[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int c = col_of[f];
    const float mu_raw = kernel[2 * f], sg_raw = kernel[2 * f + 1];
    const float sg = fminf(fmaxf(sg_raw, bd.sigma_lo), bd.sigma_hi);
    float a_mu = 0.0f, a_sg = 0.0f;
    for (int kk = tid; kk < R; kk += 256) {
        float dre = 0.0f, dim = 0.0f;
        for (int w = 0; w < nparts; ++w) {
            const float* row = dHpart + ((size_t)w * Rp + kk) * (2 * FP);
            dre += row[c];
            dim += row[FP + c];
        }
        const float wre = W[(size_t)kk * (2 * FP) + c], wim = W[(size_t)kk * (2 * FP) + FP + c];
        const float t = (float)kk;
        a_mu += t * (dim * wre - dre * wim);
        a_sg += (dre * wre + dim * wim) * (t * t / (sg * sg * sg) - 1.0f / sg);
    }
    float res[2];
    const float vals[2] = {a_mu, a_sg};
    for (int q = 0; q < 2; ++q) {
        red[tid] = vals[q];
        __syncthreads();
        for (int s2 = 128; s2 > 0; s2 >>= 1) {
            if (tid < s2) red[tid] += red[tid + s2];
            __syncthreads();
        }
        res[q] = red[0];
        __syncthreads();
    }
    if (tid == 0) {
        g_kernel[2 * f] = (mu_raw >= 0.0f && mu_raw <= 3.14159274101257324f) ? res[0] : 0.0f;
        g_kernel[2 * f + 1] = (sg_raw >= bd.sigma_lo && sg_raw <= bd.sigma_hi) ? res[1] : 0.0f;
    }
}

}  // namespace
