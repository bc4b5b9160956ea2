// Loss kernels of the training step (train_or_resume.py:116-119, 435-438): CrossEntropy(ignore_index), MSE and the
// Feature-Affinity loss (models/losses/FALoss.py), plus the SGD update and the NaN check.  All HBM-bound or tiny.
#include "common.h"
#include <algorithm>

namespace dsrl {

__device__ inline double block_sum_d(double v, double* sh) {     // sh: 4 doubles
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// ---------------------------------------------------------------------------------------------- cross entropy
// A block stages 256 pixels x C logits through LDS (contiguous global reads), one thread per pixel.
// CW = true (the *_w_kernel entry of each body below): nn.CrossEntropyLoss(weight=): `wtab` is the 256-float class-weight table indexed by the label byte
// (entries >= C are zero, so no label can index past it), a pixel's term is (double)w[t] * (double)nll and the mean's denominator is D = sum n_c w_c,
// left by ce_weight_sum_kernel where the unweighted kernels leave the pixel count.  The CW = false bodies are the kernels as they were.
// FL = true (the *_f_kernel entries): focal cross entropy, a pixel's term is (double)w[t] * (double)(q^gamma nll) and its gradient scale
// (w[t] * mod) * (1 / D), both from focal_pixel (common.h) on exp_nonpos terms; D, the flags and the staging are those of the weighted bodies.
// SM = true (the *_s_kernel entries): label-smoothed cross entropy, a pixel's term and its gradient row come from smooth_pixel / smooth_grad (common.h),
// which read all C logits and all C weights of the pixel; W = sum_{c < C} w_c is summed once per block, c ascending, before the pixel loop.
// RX = true (the *_r_kernel entries): boundary label relaxation: the pixel's class-set word is read beside its label byte, cleaned
// by relax_set, and the term and the gradient row come from relax_pixel / relax_grad (common.h) on exp_nonpos terms.
template <bool CW, bool FL = false, bool SM = false, bool RX = false>
__device__ __forceinline__ void ce_fwd_body(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                            int ignore_index, const float* __restrict__ wtab, double* __restrict__ part, float gamma = 0.f, float eps = 0.f,
                                            const unsigned* __restrict__ mask = nullptr) {
    static_assert(!FL || CW, "the focal loss runs on the weighted machinery");
    static_assert(!SM || (CW && !FL), "label smoothing runs on the weighted machinery and has no focal form");
    static_assert(!RX || (CW && !FL && !SM), "label relaxation runs on the weighted machinery alone");
    extern __shared__ float tile[];         // [256][C]
    __shared__ double shd[4];
    double loss = 0.0, cnt = 0.0;
    float Wsum = 0.f;
    if (SM) for (int c = 0; c < C; ++c) Wsum += wtab[c];
    for (long long p0 = (long long)blockIdx.x * 256; p0 < P; p0 += (long long)gridDim.x * 256) {
        const int np = (int)min(256ll, P - p0);
        __syncthreads();
        for (int t = threadIdx.x; t < np * C; t += 256) { const int r = t / C, c = t - r * C; tile[t] = logits[(p0 + r) * ld + c]; }
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int tg = target[p0 + threadIdx.x];
            if (tg != ignore_index) {
                const float* v = tile + threadIdx.x * C;
                float m = v[0];
                for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
                if (SM) {
                    float s = 0.f;
                    for (int c = 0; c < C; ++c) s += exp_nonpos(v[c] - m);
                    double val; float sub_t, inv;
                    smooth_pixel<true>(v, wtab, C, tg, m, s, eps, Wsum, 0.f, val, sub_t, inv);
                    loss += tg < C ? val : __builtin_nan("");
                } else if (RX) {
                    float s = 0.f;
                    for (int c = 0; c < C; ++c) s += exp_nonpos(v[c] - m);
                    float mS, inv, invz, term;
                    relax_pixel<0, true>(v, C, relax_set(mask[p0 + threadIdx.x], tg, C), m, s, 0.f, mS, inv, invz, term);
                    loss += (double)wtab[tg] * (double)(tg < C ? term : __builtin_nanf(""));
                } else if (FL) {
                    float s = 0.f, so = 0.f;
                    for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; so += c == tg ? 0.f : e; }
                    const float vt = v[min(tg, C - 1)];
                    float fl, mod;
                    focal_pixel(m, vt, exp_nonpos(vt - m), s, so, gamma, fl, mod);
                    loss += (double)wtab[tg] * (double)(tg < C ? fl : __builtin_nanf(""));
                } else {
                    float s = 0.f;
                    for (int c = 0; c < C; ++c) s += expf(v[c] - m);
                    // a label outside [0, C) that is not ignore_index: torch's CrossEntropyLoss asserts; here it poisons the loss (as ce_fused_kernel does)
                    const float vt = tg < C ? v[tg] : __builtin_nanf("");
                    if (CW) loss += (double)wtab[tg] * (double)(m + logf(s) - vt);
                    else loss += (double)(m + logf(s) - vt);
                }
                cnt += 1.0;
            }
        }
    }
    const double l = block_sum_d(loss, shd);
    const double n = block_sum_d(cnt, shd);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = l; part[2 * blockIdx.x + 1] = n; }
}
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                      int ignore_index, double* __restrict__ part) {
    ce_fwd_body<false>(logits, ld, target, P, C, ignore_index, nullptr, part);
}
__global__ __launch_bounds__(256) void ce_fwd_w_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, double* __restrict__ part) {
    ce_fwd_body<true>(logits, ld, target, P, C, ignore_index, wtab, part);
}
__global__ __launch_bounds__(256) void ce_fwd_f_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, float gamma, double* __restrict__ part) {
    ce_fwd_body<true, true>(logits, ld, target, P, C, ignore_index, wtab, part, gamma);
}
__global__ __launch_bounds__(256) void ce_fwd_s_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, float eps, double* __restrict__ part) {
    ce_fwd_body<true, false, true>(logits, ld, target, P, C, ignore_index, wtab, part, 0.f, eps);
}
__global__ __launch_bounds__(256) void ce_fwd_r_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, const unsigned* __restrict__ mask,
                                                        double* __restrict__ part) {
    ce_fwd_body<true, false, false, true>(logits, ld, target, P, C, ignore_index, wtab, part, 0.f, 0.f, mask);
}
__global__ __launch_bounds__(256) void ce_finalize_kernel(const double* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ double shd[4];
    double l = 0, n = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { l += part[2 * i]; n += part[2 * i + 1]; }
    l = block_sum_d(l, shd); n = block_sum_d(n, shd);
    if (threadIdx.x == 0) {
        out[0] = (float)(l / n);        // 0/0 = NaN when every pixel is ignored, as torch
        out[1] = (float)n;
    }
}
// weighted: out[1] already holds D (ce_weight_sum_kernel); out[0] = sum w nll / D, 0/0 = NaN when every live pixel has weight 0, as torch
__global__ __launch_bounds__(256) void ce_finalize_w_kernel(const double* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ double shd[4];
    double l = 0;
    for (int i = threadIdx.x; i < nb; i += 256) l += part[2 * i];
    l = block_sum_d(l, shd);
    if (threadIdx.x == 0) out[0] = (float)(l / (double)out[1]);
}
template <bool CW, bool FL = false, bool SM = false, bool RX = false>
__device__ __forceinline__ void ce_bwd_body(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                            int ignore_index, const float* __restrict__ wtab, const float* __restrict__ loss_out,
                                            const float* __restrict__ grad_out, float* __restrict__ dl, int lddl, float gamma = 0.f, float eps = 0.f,
                                            const unsigned* __restrict__ mask = nullptr) {
    static_assert(!FL || CW, "the focal loss runs on the weighted machinery");
    static_assert(!SM || (CW && !FL), "label smoothing runs on the weighted machinery and has no focal form");
    static_assert(!RX || (CW && !FL && !SM), "label relaxation runs on the weighted machinery alone");
    extern __shared__ float tile[];
    const float scale = grad_out[0] / loss_out[1];
    float Wsum = 0.f;
    __shared__ float sub_s[SM ? 64 : 1];    // SM: smooth_sub of every class (C <= 60), published by the first barrier of the pixel loop
    if (SM) {
        for (int c = 0; c < C; ++c) Wsum += wtab[c];
        if ((int)threadIdx.x < C) sub_s[threadIdx.x] = smooth_sub(eps, C, wtab[threadIdx.x], scale);
    }
    for (long long p0 = (long long)blockIdx.x * 256; p0 < P; p0 += (long long)gridDim.x * 256) {
        const int np = (int)min(256ll, P - p0);
        __syncthreads();
        for (int t = threadIdx.x; t < np * C; t += 256) { const int r = t / C, c = t - r * C; tile[t] = logits[(p0 + r) * ld + c]; }
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int tg = target[p0 + threadIdx.x];
            float* v = tile + threadIdx.x * C;
            if (tg != ignore_index) {
                float m = v[0];
                for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
                const bool bad = tg >= C;             // label outside [0, C), not ignored: a NaN gradient row, as the loss
                if (SM) {
                    float s = 0.f;
                    for (int c = 0; c < C; ++c) s += exp_nonpos(v[c] - m);
                    double val; float sub_t, inv;
                    smooth_pixel<false>(v, wtab, C, tg, m, s, eps, Wsum, scale, val, sub_t, inv);
                    for (int c = 0; c < C; ++c) v[c] = bad ? __builtin_nanf("") : smooth_grad(exp_nonpos(v[c] - m), inv, c == tg, sub_t, sub_s[c]);
                } else if (RX) {
                    float s = 0.f;
                    for (int c = 0; c < C; ++c) s += exp_nonpos(v[c] - m);
                    const unsigned S = relax_set(mask[p0 + threadIdx.x], tg, C);
                    float mS, inv, invz, term;
                    relax_pixel<0, false>(v, C, S, m, s, wtab[tg] * scale, mS, inv, invz, term);
                    for (int c = 0; c < C; ++c)
                        v[c] = bad ? __builtin_nanf("") : relax_grad(exp_nonpos(v[c] - m), inv, (S >> c) & 1u, v[c], mS, invz);
                } else if (FL) {
                    const float vt = v[min(tg, C - 1)];
                    float s = 0.f, so = 0.f;
                    for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; so += c == tg ? 0.f : e; v[c] = e; }
                    float fl, mod;
                    focal_pixel(m, vt, exp_nonpos(vt - m), s, so, gamma, fl, mod);
                    const float sc = (wtab[tg] * mod) * scale;
                    const float inv = 1.f / s;
                    for (int c = 0; c < C; ++c) v[c] = bad ? __builtin_nanf("") : (v[c] * inv - (c == tg ? 1.f : 0.f)) * sc;
                } else {
                    float s = 0.f;
                    for (int c = 0; c < C; ++c) s += expf(v[c] - m);
                    const float inv = 1.f / s;
                    const float sc = CW ? wtab[tg] * scale : scale;
                    for (int c = 0; c < C; ++c) v[c] = bad ? __builtin_nanf("") : (expf(v[c] - m) * inv - (c == tg ? 1.f : 0.f)) * sc;
                }
            } else {
                for (int c = 0; c < C; ++c) v[c] = 0.f;
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < np * C; t += 256) { const int r = t / C, c = t - r * C; dl[(p0 + r) * lddl + c] = tile[t]; }
    }
}
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                      int ignore_index, const float* __restrict__ loss_out, const float* __restrict__ grad_out,
                                                      float* __restrict__ dl, int lddl) {
    ce_bwd_body<false>(logits, ld, target, P, C, ignore_index, nullptr, loss_out, grad_out, dl, lddl);
}
__global__ __launch_bounds__(256) void ce_bwd_w_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, const float* __restrict__ loss_out,
                                                        const float* __restrict__ grad_out, float* __restrict__ dl, int lddl) {
    ce_bwd_body<true>(logits, ld, target, P, C, ignore_index, wtab, loss_out, grad_out, dl, lddl);
}
__global__ __launch_bounds__(256) void ce_bwd_f_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, float gamma, const float* __restrict__ loss_out,
                                                        const float* __restrict__ grad_out, float* __restrict__ dl, int lddl) {
    ce_bwd_body<true, true>(logits, ld, target, P, C, ignore_index, wtab, loss_out, grad_out, dl, lddl, gamma);
}
__global__ __launch_bounds__(256) void ce_bwd_s_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, float eps, const float* __restrict__ loss_out,
                                                        const float* __restrict__ grad_out, float* __restrict__ dl, int lddl) {
    ce_bwd_body<true, false, true>(logits, ld, target, P, C, ignore_index, wtab, loss_out, grad_out, dl, lddl, 0.f, eps);
}
__global__ __launch_bounds__(256) void ce_bwd_r_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const float* __restrict__ wtab, const unsigned* __restrict__ mask,
                                                        const float* __restrict__ loss_out, const float* __restrict__ grad_out, float* __restrict__ dl, int lddl) {
    ce_bwd_body<true, false, false, true>(logits, ld, target, P, C, ignore_index, wtab, loss_out, grad_out, dl, lddl, 0.f, 0.f, mask);
}

// ---------------------------------------------------------------------------------------------- fused loss pass
// One pass over the logits instead of two: the kernel computes the per-pixel CE terms AND writes d(CE)/d(logits) for an upstream
// gradient of 1 (the loss is the root of the backward pass), checks the logits for NaN on the way (the reference's per-output NaN
// asserts, train_or_resume.py:426-433) and stages 256 pixels x C logits through LDS with 16-byte accesses when the tensor is dense.
// The mean's denominator (pixels that are not ignored) comes from a pre-pass over the uint8 target (4 MB at 8 x 512 x 1024).
constexpr int kCountBlocks = 256;
__global__ __launch_bounds__(256) void count_valid_kernel(const unsigned char* __restrict__ target, long long P, int ignore_index, unsigned* __restrict__ part) {
    __shared__ unsigned sh[4];
    unsigned n = 0;
    // 16 labels per load; the head up to the first 16-byte boundary and the tail are counted byte by byte by block 0
    const long long head = min(P, (long long)((16 - ((uintptr_t)target & 15)) & 15));
    const long long nv = (P - head) >> 4;
    const uint4* v = reinterpret_cast<const uint4*>(target + head);
    const unsigned ig = (unsigned)ignore_index & 0xffu;
    const bool can_match = ignore_index >= 0 && ignore_index <= 255;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long long)gridDim.x * 256) {
        const uint4 q = v[e];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int b = 0; b < 4; ++b) n += (!can_match || ((w[u] >> (8 * b)) & 0xffu) != ig) ? 1u : 0u;
    }
    if (blockIdx.x == 0) {
        for (long long e = threadIdx.x; e < head; e += 256) n += (target[e] != ignore_index) ? 1u : 0u;
        for (long long e = head + (nv << 4) + threadIdx.x; e < P; e += 256) n += (target[e] != ignore_index) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
// ---------------------------------------------------------------------------------------------- class histogram, weighted denominator
// Labels (through `lut` when given) -> 256 bins.  16 labels per load, per-wave LDS bins (a road-heavy label map sends most lanes of a wave to one
// bin; four sets keep the waves of a block apart), the head up to the first 16-byte boundary and the tail byte by byte by block 0.  The bins leave as
// 64-bit atomics into `counts` (accumulated: dsrl_class_histogram) or as the block's own row of `part` [gridDim.x][256] (nothing to zero, merged in
// integers by ce_weight_sum_kernel) - exact and independent of the block order either way.
constexpr int kHistBlocks = 256;
__global__ __launch_bounds__(256) void class_hist_kernel(const unsigned char* __restrict__ labels, long long P, const unsigned char* __restrict__ lut,
                                                          unsigned long long* __restrict__ counts, unsigned* __restrict__ part) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned char slut[256];
    for (int t = threadIdx.x; t < 4 * 256; t += 256) (&hist[0][0])[t] = 0u;
    slut[threadIdx.x] = lut ? lut[threadIdx.x] : (unsigned char)threadIdx.x;
    __syncthreads();
    unsigned* h = hist[threadIdx.x >> 6];
    const long long head = min(P, (long long)((16 - ((uintptr_t)labels & 15)) & 15));
    const long long nv = (P - head) >> 4;
    const uint4* v = reinterpret_cast<const uint4*>(labels + head);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long long)gridDim.x * 256) {
        const uint4 q = v[e];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int b = 0; b < 4; ++b) atomicAdd(&h[slut[(w[u] >> (8 * b)) & 0xffu]], 1u);
    }
    if (blockIdx.x == 0) {
        for (long long e = threadIdx.x; e < head; e += 256) atomicAdd(&h[slut[labels[e]]], 1u);
        for (long long e = head + (nv << 4) + threadIdx.x; e < P; e += 256) atomicAdd(&h[slut[labels[e]]], 1u);
    }
    __syncthreads();
    const unsigned n = hist[0][threadIdx.x] + hist[1][threadIdx.x] + hist[2][threadIdx.x] + hist[3][threadIdx.x];
    if (part) part[(long long)blockIdx.x * 256 + threadIdx.x] = n;
    else if (n) atomicAdd(&counts[threadIdx.x], (unsigned long long)n);
}
// D = fp32(sum over c ascending of (double)n_c * (double)w_c), n_c the pixels of class c that are not ignore_index: integer counts, one rounding.
// Classes [0, C) only: whatever a caller's table holds from C on cannot change D.
__global__ __launch_bounds__(256) void ce_weight_sum_kernel(const unsigned* __restrict__ part, int nb, int C, int ignore_index, const float* __restrict__ wtab,
                                                             float* __restrict__ d_out) {
    __shared__ double term[256];
    unsigned long long n = 0;
    for (int b = 0; b < nb; ++b) n += part[b * 256 + threadIdx.x];
    term[threadIdx.x] = ((int)threadIdx.x == ignore_index || (int)threadIdx.x >= C) ? 0.0 : (double)n * (double)wtab[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        double d = 0.0;
        for (int c = 0; c < C; ++c) d += term[c];
        d_out[0] = (float)d;
    }
}

template <bool CW, bool FL = false, bool SM = false, bool RX = false>
__device__ __forceinline__ void ce_fused_body(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                              int ignore_index, const unsigned* __restrict__ cnt_part, const float* __restrict__ wtab,
                                              const float* __restrict__ wsum, float* __restrict__ dl, int lddl,
                                              double* __restrict__ part, int* __restrict__ nan_flag, int vec_in, int vec_out, float gamma = 0.f,
                                              float eps = 0.f, const unsigned* __restrict__ mask = nullptr) {
    static_assert(!FL || CW, "the focal loss runs on the weighted machinery");
    static_assert(!SM || (CW && !FL), "label smoothing runs on the weighted machinery and has no focal form");
    static_assert(!RX || (CW && !FL && !SM), "label relaxation runs on the weighted machinery alone");
    extern __shared__ __attribute__((aligned(16))) float tile[];         // [256][C]
    __shared__ double shd[4];
    __shared__ float sh_scale;
    if (!CW) {
        static_assert(kCountBlocks == 256, "one partial count per thread");
        const double n = block_sum_d((double)cnt_part[threadIdx.x], shd);       // exact: counts < 2^53
        if (threadIdx.x == 0) sh_scale = 1.f / (float)n;        // n = 0: every pixel ignored, the loss is 0/0 = NaN as in torch and no gradient element uses the scale
    }
    __syncthreads();
    const float scale = CW ? 1.f / wsum[0] : sh_scale;      // CW: 1 / D; per pixel sc = w[t] * (1 / D)
    double loss = 0.0, cnt = 0.0;
    bool bad = false, bad_label = false;
    float Wsum = 0.f;
    __shared__ float sub_s[SM ? 64 : 1];    // SM: smooth_sub of every class (C <= 60), published by the first barrier of the pixel loop
    if (SM) {
        for (int c = 0; c < C; ++c) Wsum += wtab[c];
        if ((int)threadIdx.x < C) sub_s[threadIdx.x] = smooth_sub(eps, C, wtab[threadIdx.x], scale);
    }
    for (long long p0 = (long long)blockIdx.x * 256; p0 < P; p0 += (long long)gridDim.x * 256) {
        const int np = (int)min(256ll, P - p0);
        const int nf = np * C;
        __syncthreads();
        if (vec_in) {           // dense rows: 256 pixels are one contiguous run that starts on a 16-byte boundary
            const float4* src = reinterpret_cast<const float4*>(logits + p0 * C);
            for (int t = threadIdx.x; t < (nf >> 2); t += 256) reinterpret_cast<float4*>(tile)[t] = src[t];
            for (int t = (nf & ~3) + threadIdx.x; t < nf; t += 256) tile[t] = logits[p0 * C + t];
        } else {
            for (int t = threadIdx.x; t < nf; t += 256) { const int r = t / C, c = t - r * C; tile[t] = logits[(p0 + r) * ld + c]; }
        }
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int tg = target[p0 + threadIdx.x];
            bad_label |= tg != ignore_index && (tg < 0 || tg >= C);     // torch's CrossEntropyLoss asserts on such a target: here it poisons the loss and raises flag bit 1
            float* v = tile + threadIdx.x * C;
            float m = v[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
            const float vt = v[max(min(tg == ignore_index ? 0 : tg, C - 1), 0)];
            float s = 0.f, so = 0.f;
            if (SM || RX) {                     // the tile keeps the logits: smooth_pixel / relax_pixel read them once s is known
                for (int c = 0; c < C; ++c) s += exp_nonpos(v[c] - m);
            } else if (FL) {                    // so: the sum without the target's term, in the same order
                for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; so += c == tg ? 0.f : e; v[c] = e; }
            } else {
                for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; v[c] = e; }   // the tile keeps exp(v - m): one exp per logit
            }
            bad |= !(s == s);                   // any NaN logit poisons the sum (fmaxf alone would skip it)
            if (SM) {
                if (tg != ignore_index) {
                    double val; float sub_t, inv;
                    smooth_pixel<true>(v, wtab, C, tg, m, s, eps, Wsum, scale, val, sub_t, inv);
                    loss += val;
                    cnt += 1.0;
                    // the second exp_nonpos of a logit has the bits of the first: the row equals the one convt2x2_bwd_dma_kernel forms from registers
                    if (dl) for (int c = 0; c < C; ++c) v[c] = smooth_grad(exp_nonpos(v[c] - m), inv, c == tg, sub_t, sub_s[c]);
                } else if (dl) {
                    for (int c = 0; c < C; ++c) v[c] = 0.f;
                }
            } else if (RX) {
                if (tg != ignore_index) {
                    const unsigned S = relax_set(mask[p0 + threadIdx.x], tg, C);
                    float mS, inv, invz, term;
                    const float wt = wtab[tg];
                    relax_pixel<0, true>(v, C, S, m, s, wt * scale, mS, inv, invz, term);
                    loss += (double)wt * (double)term;
                    cnt += 1.0;
                    if (dl) for (int c = 0; c < C; ++c) v[c] = relax_grad(exp_nonpos(v[c] - m), inv, (S >> c) & 1u, v[c], mS, invz);
                } else if (dl) {
                    for (int c = 0; c < C; ++c) v[c] = 0.f;
                }
            } else if (tg != ignore_index) {
                const float wt = CW ? wtab[tg] : 1.f;
                float mod = 1.f;
                if (FL) {
                    float fl;
                    focal_pixel(m, vt, exp_nonpos(vt - m), s, so, gamma, fl, mod);
                    loss += (double)wt * (double)fl;
                }
                else if (CW) loss += (double)wt * (double)(m + logf(s) - vt);
                else loss += (double)(m + logf(s) - vt);
                cnt += 1.0;
                if (dl) {
                    const float sc = FL ? (wt * mod) * scale : CW ? wt * scale : scale;
                    const float inv = sc / s;
                    for (int c = 0; c < C; ++c) v[c] = v[c] * inv - (c == tg ? sc : 0.f);
                }
            } else if (dl) {
                for (int c = 0; c < C; ++c) v[c] = 0.f;
            }
        }
        if (dl) {
            __syncthreads();
            if (vec_out) {
                float4* dst = reinterpret_cast<float4*>(dl + p0 * C);
                for (int t = threadIdx.x; t < (nf >> 2); t += 256) dst[t] = reinterpret_cast<const float4*>(tile)[t];
                for (int t = (nf & ~3) + threadIdx.x; t < nf; t += 256) dl[p0 * C + t] = tile[t];
            } else {
                for (int t = threadIdx.x; t < nf; t += 256) { const int r = t / C, c = t - r * C; dl[(p0 + r) * lddl + c] = tile[t]; }
            }
        }
    }
    if (bad_label) loss = __builtin_nan("");
    const double l = block_sum_d(loss, shd);
    const double n = block_sum_d(cnt, shd);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = l; part[2 * blockIdx.x + 1] = n; }
    if (nan_flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
    if (nan_flag && __any(bad_label) && (threadIdx.x & 63) == 0) atomicOr(nan_flag, 2);
}
__global__ __launch_bounds__(256) void ce_fused_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                        int ignore_index, const unsigned* __restrict__ cnt_part, float* __restrict__ dl, int lddl,
                                                        double* __restrict__ part, int* __restrict__ nan_flag, int vec_in, int vec_out) {
    ce_fused_body<false>(logits, ld, target, P, C, ignore_index, cnt_part, nullptr, nullptr, dl, lddl, part, nan_flag, vec_in, vec_out);
}
__global__ __launch_bounds__(256) void ce_fused_w_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                          int ignore_index, const float* __restrict__ wtab, const float* __restrict__ wsum,
                                                          float* __restrict__ dl, int lddl, double* __restrict__ part, int* __restrict__ nan_flag,
                                                          int vec_in, int vec_out) {
    ce_fused_body<true>(logits, ld, target, P, C, ignore_index, nullptr, wtab, wsum, dl, lddl, part, nan_flag, vec_in, vec_out);
}
__global__ __launch_bounds__(256) void ce_fused_f_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                          int ignore_index, const float* __restrict__ wtab, float gamma, const float* __restrict__ wsum,
                                                          float* __restrict__ dl, int lddl, double* __restrict__ part, int* __restrict__ nan_flag,
                                                          int vec_in, int vec_out) {
    ce_fused_body<true, true>(logits, ld, target, P, C, ignore_index, nullptr, wtab, wsum, dl, lddl, part, nan_flag, vec_in, vec_out, gamma);
}
__global__ __launch_bounds__(256) void ce_fused_s_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                          int ignore_index, const float* __restrict__ wtab, float eps, const float* __restrict__ wsum,
                                                          float* __restrict__ dl, int lddl, double* __restrict__ part, int* __restrict__ nan_flag,
                                                          int vec_in, int vec_out) {
    ce_fused_body<true, false, true>(logits, ld, target, P, C, ignore_index, nullptr, wtab, wsum, dl, lddl, part, nan_flag, vec_in, vec_out, 0.f, eps);
}
__global__ __launch_bounds__(256) void ce_fused_r_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                          int ignore_index, const float* __restrict__ wtab, const unsigned* __restrict__ mask,
                                                          const float* __restrict__ wsum, float* __restrict__ dl, int lddl, double* __restrict__ part,
                                                          int* __restrict__ nan_flag, int vec_in, int vec_out) {
    ce_fused_body<true, false, false, true>(logits, ld, target, P, C, ignore_index, nullptr, wtab, wsum, dl, lddl, part, nan_flag, vec_in, vec_out, 0.f, 0.f, mask);
}
// MSE forward and backward in one pass: partial sums of (a-b)^2 and da = (a-b) * 2 * grad_scale / n; NaN check of `a`
__global__ __launch_bounds__(256) void mse_fused_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, float sc, float* __restrict__ da,
                                                         double* __restrict__ part, int* __restrict__ nan_flag, int vec) {
    __shared__ double shd[4];
    double s = 0.0;
    bool bad = false;
    if (vec) {
        const long long n4 = n >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(a); const float4* b4 = reinterpret_cast<const float4*>(b); float4* d4 = reinterpret_cast<float4*>(da);
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long long)gridDim.x * 256) {
            const float4 x = a4[e], y = b4[e];
            const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
            bad |= !(x.x == x.x) | !(x.y == x.y) | !(x.z == x.z) | !(x.w == x.w);
            s += (double)(d0 * d0) + (double)(d1 * d1) + (double)(d2 * d2) + (double)(d3 * d3);
            if (da) d4[e] = make_float4(d0 * sc, d1 * sc, d2 * sc, d3 * sc);
        }
        for (long long e = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
            const float d = a[e] - b[e];
            bad |= !(a[e] == a[e]);
            s += (double)(d * d);
            if (da) da[e] = d * sc;
        }
    } else {
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
            const float d = a[e] - b[e];
            bad |= !(a[e] == a[e]);
            s += (double)(d * d);
            if (da) da[e] = d * sc;
        }
    }
    const double t = block_sum_d(s, shd);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
    if (nan_flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
}
// vals = {CE, w1 * MSE, w2 * FA, their sum, NaN flag}: the five scalars one iteration reads back (train_or_resume.py:435-438, 457-460)
__global__ void loss_mix_kernel(const float* __restrict__ ce, const float* __restrict__ mse, const float* __restrict__ fa, float w1, float w2,
                                const int* __restrict__ nan_flag, float* __restrict__ vals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float c = ce[0], m = mse ? w1 * mse[0] : 0.f, f = fa ? w2 * fa[0] : 0.f;
        vals[0] = c; vals[1] = m; vals[2] = f; vals[3] = c + m + f; vals[4] = nan_flag ? (float)nan_flag[0] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------- MSE
__global__ __launch_bounds__(256) void mse_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, double* __restrict__ part) {
    __shared__ double shd[4];
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const float d = a[e] - b[e];
        s += (double)(d * d);
    }
    const double t = block_sum_d(s, shd);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void mse_finalize_kernel(const double* __restrict__ part, int nb, long long n, float* __restrict__ out) {
    __shared__ double shd[4];
    double s = 0;
    for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
    s = block_sum_d(s, shd);
    if (threadIdx.x == 0) out[0] = (float)(s / (double)n);
}
__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, const float* __restrict__ grad_out,
                                                       float* __restrict__ da) {
    const float sc = 2.f * grad_out[0] / (float)n;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) da[e] = (a[e] - b[e]) * sc;
}

// ---------------------------------------------------------------------------------------------- FA loss
// One block per (b,c) slice pair.  Per map: k x k average pooling -> X (h' x w'), G = X^T X in fp64, the dominant
// eigenpair of G by repeated squaring (20 squarings = power 2^20: converged for any spectral gap a float can
// resolve; the eigenvalue is then the Rayleigh quotient on the original G), sigma_1 = sqrt(lambda), S = G/lambda.
constexpr int FA_MAXW = 32, FA_MAXH = 64, FA_SQUARINGS = 20;

struct FaSmem {
    double g0[FA_MAXW * FA_MAXW];
    double ga[FA_MAXW * FA_MAXW];
    double gb[FA_MAXW * FA_MAXW];
    double red[4];
    double vec[FA_MAXW];
    float x[FA_MAXH * FA_MAXW];
    float s1[FA_MAXW * FA_MAXW];
    float s2[FA_MAXW * FA_MAXW];
    float u[FA_MAXH];
    float scal[4];
};

// k x k average pooling of one map into X (hp x wp).  The usual case (k = 8, unit column stride, 16-byte aligned rows) uses T = 1, 2, 4 or 8
// consecutive lanes per cell - as many as 256 threads allow - each summing k / T rows with two independent 16-byte loads per row (all loads
// of a thread are in flight together; the per-cell loop of 64 dependent scalar loads this replaces took ~30 us per map), the lane partials
// combined by a fixed xor tree: deterministic.
__device__ void fa_pool(const float* __restrict__ fm, long long sh_, long long sw_, int hp, int wp, int k, float* X) {
    const float inv = 1.f / (float)(k * k);
    const int ncells = hp * wp;
    if (k == 8 && sw_ == 1 && (sh_ & 3) == 0 && ((uintptr_t)fm & 15) == 0) {
        int T = 1;
        while (T < 8 && ncells * (T * 2) <= 256) T *= 2;
        const int sub = threadIdx.x & (T - 1), per = 256 / T;
        for (int c0 = 0; c0 < ncells; c0 += per) {
            const int cell = c0 + (int)(threadIdx.x / T);
            float s = 0.f;
            if (cell < ncells) {
                const int i = cell / wp, j = cell - i * wp;
                const float* base = fm + (long long)(i * 8) * sh_ + j * 8;
                float4 v[8][2];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (r < 8 / T) {
                        const float* row = base + (long long)(sub + r * T) * sh_;
                        v[r][0] = *reinterpret_cast<const float4*>(row); v[r][1] = *reinterpret_cast<const float4*>(row + 4);
                    }
                }
#pragma unroll
                for (int r = 0; r < 8; ++r)
                    if (r < 8 / T) s += ((v[r][0].x + v[r][0].y) + (v[r][0].z + v[r][0].w)) + ((v[r][1].x + v[r][1].y) + (v[r][1].z + v[r][1].w));
            }
            for (int o = 1; o < T; o <<= 1) s += __shfl_xor(s, o, 64);
            if (cell < ncells && sub == 0) X[cell] = s * inv;
        }
    } else {
        for (int cell = threadIdx.x; cell < ncells; cell += 256) {
            const int i = cell / wp, j = cell - i * wp;
            float s = 0.f;
            for (int r = 0; r < k; ++r)
                for (int q = 0; q < k; ++q) s += fm[(long long)(i * k + r) * sh_ + (long long)(j * k + q) * sw_];
            X[cell] = s * inv;
        }
    }
    __syncthreads();
}

// wave-wide helpers on doubles: every lane of the wave takes part (wp <= 32 values sit in lanes 0..wp-1, the others carry neutral elements)
__device__ __forceinline__ double shfl_xor_d(double v, int o) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl_xor((int)(b & 0xffffffffll), o, 64), hi = __shfl_xor((int)(b >> 32), o, 64);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave32_max_d(double v) {        // all 64 lanes receive the result (lanes >= wp carry the neutral element)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, shfl_xor_d(v, o));
    return v;
}
__device__ __forceinline__ double wave32_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_d(v, o);
    return v;
}

// leaves: sm.g0 = G, sm.vec = unit dominant eigenvector, returns lambda (double, uniform).  Round 3: nothing in the loop is serial any more - the
// largest diagonal entry, the best column, the norm and the Rayleigh quotient used to be loops of wp dependent LDS reads in EVERY thread (the
// kernel took 100 us for two 16x16 problems per slice); they are wave reductions over lanes 0..wp-1 now, done redundantly by each wave.
__device__ double fa_top_eig(FaSmem& sm, int hp, int wp) {
    const int nn = wp * wp, lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < nn; e += 256) {
        const int a = e / wp, b = e - a * wp;
        double s = 0.0;
        for (int i = 0; i < hp; ++i) s += (double)sm.x[i * wp + a] * (double)sm.x[i * wp + b];
        sm.g0[e] = s; sm.ga[e] = s;
    }
    __syncthreads();
    double* cur = sm.ga; double* nxt = sm.gb;
    for (int it = 0; it < FA_SQUARINGS; ++it) {
        // normalise by the largest diagonal entry (G is PSD: max |entry| sits on the diagonal)
        const double mx = wave32_max_d(lane < wp ? cur[lane * wp + lane] : 0.0);
        if (!(mx > 0.0)) break;             // all-zero (or NaN) map: lambda = 0 -> S = 0/0 = NaN exactly like the reference
        const double inv = 1.0 / mx;
        for (int e = threadIdx.x; e < nn; e += 256) {
            const int a = e / wp, b = e - a * wp;
            double s = 0.0;
            for (int q = 0; q < wp; ++q) s += (cur[a * wp + q] * inv) * (cur[q * wp + b] * inv);
            nxt[e] = s;
        }
        __syncthreads();
        double* t = cur; cur = nxt; nxt = t;
    }
    // dominant eigenvector ~ the column of G^(2^s) with the largest diagonal entry (the first such column)
    const double dg = lane < wp ? cur[lane * wp + lane] : -1.0;
    const double bd = wave32_max_d(dg);
    const unsigned long long hit = __ballot(lane < wp && dg == bd);
    const int best = hit ? __builtin_ctzll(hit) : 0;
    const double col = lane < wp ? cur[lane * wp + best] : 0.0;
    const double nrm = sqrt(wave32_sum_d(col * col));
    if ((int)threadIdx.x < wp) sm.vec[threadIdx.x] = nrm > 0.0 ? col / nrm : (threadIdx.x == 0 ? 1.0 : 0.0);
    __syncthreads();
    double row = 0.0;                        // Rayleigh quotient on the original G: lane a holds v_a (G v)_a
    if (lane < wp) {
        for (int b = 0; b < wp; ++b) row += sm.g0[lane * wp + b] * sm.vec[b];
        row *= sm.vec[lane];
    }
    return wave32_sum_d(row);
}

// One (slice, map) per block (round 3: the two maps of a slice used to run one after the other in one block): pooled map -> G = X^T X -> lambda,
// v1 -> S = G / lambda, and what the backward pass needs, into `saved` [S1 n][S2 n][sigma1, sigma2][u1 hp][v1 wp][u2 hp][v2 wp].
__global__ __launch_bounds__(256) void fa_sim_kernel(const float* __restrict__ fm1, const float* __restrict__ fm2, int C, int hp, int wp, int k,
                                                      long long sb, long long sc, long long sh_, long long sw_, float* __restrict__ saved, long long saved_stride) {
    __shared__ FaSmem sm;
    const int slice = blockIdx.x, map = blockIdx.y, b = slice / C, c = slice - b * C;
    const int n = wp * wp;
    float* sv = saved + (long long)slice * saved_stride;
    const float* fm = (map == 0 ? fm1 : fm2) + b * sb + c * sc;
    fa_pool(fm, sh_, sw_, hp, wp, k, sm.x);
    const double lam = fa_top_eig(sm, hp, wp);
    const double sigma = sqrt(lam);
    for (int e = threadIdx.x; e < n; e += 256) sv[map * n + e] = (float)(sm.g0[e] / lam);
    float* uv = sv + 2 * n + 2 + map * (hp + wp);
    for (int i = threadIdx.x; i < hp; i += 256) {
        double s = 0.0;
        for (int a = 0; a < wp; ++a) s += (double)sm.x[i * wp + a] * sm.vec[a];
        uv[i] = (float)(s / sigma);
    }
    if ((int)threadIdx.x < wp) uv[hp + threadIdx.x] = (float)sm.vec[threadIdx.x];
    if (threadIdx.x == 0) sv[2 * n + map] = (float)sigma;
}
// all pairs |S1_i - S2_j| of one slice, rows i dealt over kFaPairBlocks blocks; one fp64 partial per block (summed in a fixed order by fa_finalize_kernel)
constexpr int kFaPairBlocks = 8;
__global__ __launch_bounds__(256) void fa_pairs_kernel(const float* __restrict__ saved, long long saved_stride, int n, int reduction,
                                                        float* __restrict__ out_none, double* __restrict__ part) {
    __shared__ float s2[FA_MAXW * FA_MAXW];
    __shared__ double red[4];
    const int slice = blockIdx.x, chunk = blockIdx.y;
    const float* sv = saved + (long long)slice * saved_stride;
    for (int e = threadIdx.x; e < n; e += 256) s2[e] = sv[n + e];
    __syncthreads();
    const int per = (n + kFaPairBlocks - 1) / kFaPairBlocks, i0 = chunk * per, i1 = min(n, i0 + per);
    double acc = 0.0;
    // a row is shared by 8 lanes (j = sub, sub + 8, ...: 32 rows per pass over 256 threads), so that even n = 256 keeps every thread busy
    const int sub = threadIdx.x & 7;
    for (int i = i0 + (int)(threadIdx.x >> 3); i < i1; i += 32) {
        const float a = sv[i];
        float s = 0.f;
        if (reduction == 2) {
            float* o = out_none + ((long long)slice * n + i) * n;
            for (int j = sub; j < n; j += 8) o[j] = fabsf(a - s2[j]);
        } else {
            for (int j = sub; j < n; j += 8) s += fabsf(a - s2[j]);
        }
        acc += (double)s;
    }
    const double tot = block_sum_d(acc, red);
    if (threadIdx.x == 0) part[slice * kFaPairBlocks + chunk] = tot;
}
__global__ void fa_finalize_kernel(const double* __restrict__ part, int nslices, int n, int reduction, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < nslices * kFaPairBlocks; ++i) s += part[i];
        out[0] = (float)(reduction == 0 ? s / ((double)nslices * n * n) : s);
    }
}

__global__ __launch_bounds__(256) void fa_bwd_kernel(const float* __restrict__ fm1, const float* __restrict__ fm2, int nslices, int C, int H, int W, int hp, int wp, int k,
                                                      long long sb, long long sc, long long sh_, long long sw_, int reduction,
                                                      const float* __restrict__ grad_out, const float* __restrict__ saved, long long saved_stride,
                                                      float* __restrict__ d1, float* __restrict__ d2) {
    __shared__ float X[FA_MAXH * FA_MAXW];
    __shared__ float S1[FA_MAXW * FA_MAXW], S2[FA_MAXW * FA_MAXW], dS[FA_MAXW * FA_MAXW];
    __shared__ float dXn[FA_MAXH * FA_MAXW];
    __shared__ double red[4];
    const int slice = blockIdx.x, b = slice / C, c = slice - b * C;
    const int n = wp * wp;
    const float* sv = saved + (long long)slice * saved_stride;
    for (int e = threadIdx.x; e < n; e += 256) { S1[e] = sv[e]; S2[e] = sv[n + e]; }
    __syncthreads();
    const float scale = grad_out[0] * (reduction == 0 ? (float)(1.0 / ((double)nslices * n * n)) : 1.f);
    {
        const int map = blockIdx.y;            // round 3: the two maps of a slice in two blocks
        // dS_map
        for (int e = threadIdx.x; e < n; e += 256) {
            int cnt = 0;
            if (map == 0) { const float a = S1[e]; for (int j = 0; j < n; ++j) { const float d = a - S2[j]; cnt += (d > 0.f) - (d < 0.f); } }
            else { const float v = S2[e]; for (int i = 0; i < n; ++i) { const float d = S1[i] - v; cnt -= (d > 0.f) - (d < 0.f); } }
            dS[e] = scale * (float)cnt;
        }
        const float* fm = (map == 0 ? fm1 : fm2) + b * sb + c * sc;
        fa_pool(fm, sh_, sw_, hp, wp, k, X);        // ends with a barrier (dS complete too)
        const float sigma = sv[2 * n + map];
        const float* u1 = sv + 2 * n + 2 + map * (hp + wp);
        const float* v1 = u1 + hp;
        // dXn = (X/sigma) (dS + dS^T);  dot = sum dXn * X
        double dot = 0.0;
        for (int e = threadIdx.x; e < hp * wp; e += 256) {
            const int i = e / wp, a = e - i * wp;
            float s = 0.f;
            for (int q = 0; q < wp; ++q) s += X[i * wp + q] * (dS[q * wp + a] + dS[a * wp + q]);
            s /= sigma;
            dXn[e] = s;
            dot += (double)s * (double)X[e];
        }
        const double tot = block_sum_d(dot, red);
        const float dsigma = (float)(-tot / ((double)sigma * (double)sigma));
        float* dst = (map == 0 ? d1 : d2) + (long long)slice * H * W;
        const float invk2 = 1.f / (float)(k * k);
        for (int e = threadIdx.x; e < H * W; e += 256) {
            const int h = e / W, w = e - h * W;
            const int i = h / k, a = w / k;
            float v = 0.f;
            if (i < hp && a < wp) v = (dXn[i * wp + a] / sigma + dsigma * u1[i] * v1[a]) * invk2;
            dst[e] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- SGD, NaN check
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long n,
                                                   float lr, float mom, float wd, float gscale) {
    const long long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g); float4* b4 = reinterpret_cast<float4*>(buf);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        float4 pv = p4[e]; const float4 gv = g4[e]; float4 bv = b4[e];
        bv.x = mom * bv.x + fmaf(wd, pv.x, gv.x * gscale); pv.x -= lr * bv.x;
        bv.y = mom * bv.y + fmaf(wd, pv.y, gv.y * gscale); pv.y -= lr * bv.y;
        bv.z = mom * bv.z + fmaf(wd, pv.z, gv.z * gscale); pv.z -= lr * bv.z;
        bv.w = mom * bv.w + fmaf(wd, pv.w, gv.w * gscale); pv.w -= lr * bv.w;
        p4[e] = pv; b4[e] = bv;
    }
    for (long long e = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const float d = fmaf(wd, p[e], g[e] * gscale);
        const float bv = mom * buf[e] + d;
        buf[e] = bv; p[e] -= lr * bv;
    }
}
// the same update with the four hyper-parameters read from device memory (a captured launch follows the LR schedule without re-capture)
__global__ __launch_bounds__(256) void sgd_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long n,
                                                       const float* __restrict__ hyper) {
    const float lr = hyper[0], mom = hyper[1], wd = hyper[2], gscale = hyper[3];
    const long long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g); float4* b4 = reinterpret_cast<float4*>(buf);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        float4 pv = p4[e]; const float4 gv = g4[e]; float4 bv = b4[e];
        bv.x = mom * bv.x + fmaf(wd, pv.x, gv.x * gscale); pv.x -= lr * bv.x;
        bv.y = mom * bv.y + fmaf(wd, pv.y, gv.y * gscale); pv.y -= lr * bv.y;
        bv.z = mom * bv.z + fmaf(wd, pv.z, gv.z * gscale); pv.z -= lr * bv.z;
        bv.w = mom * bv.w + fmaf(wd, pv.w, gv.w * gscale); pv.w -= lr * bv.w;
        p4[e] = pv; b4[e] = bv;
    }
    for (long long e = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const float d = fmaf(wd, p[e], g[e] * gscale);
        const float bv = mom * buf[e] + d;
        buf[e] = bv; p[e] -= lr * bv;
    }
}
// The same update over a SEGMENT table that covers the arena (round 5): row {first float, floats (multiple of 4, first float 16-byte aligned), address of an
// amax record or 0}.  A segment lies inside ONE parameter; for the conv filters the block also leaves max |p| of the values it has just written in the
// filter's record (bit patterns, atomicMax: order-independent, so the record equals what dsrl_conv2d_filters_amax_batched measures) - the per-step filter pass
// then starts with the split instead of another 232 MB sweep over the parameters the optimiser wrote a moment ago.  One block per segment.
__global__ __launch_bounds__(256) void sgd_dev_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                                const long long* __restrict__ table, const float* __restrict__ hyper) {
    const float lr = hyper[0], mom = hyper[1], wd = hyper[2], gscale = hyper[3];
    const long long* row = table + 3ll * blockIdx.x;
    const long long off = row[0];
    const int n4 = (int)(row[1] >> 2);
    unsigned* rec = reinterpret_cast<unsigned*>(row[2]);
    float4* p4 = reinterpret_cast<float4*>(p + off); const float4* g4 = reinterpret_cast<const float4*>(g + off); float4* b4 = reinterpret_cast<float4*>(buf + off);
    unsigned m = 0u;
    for (int e = threadIdx.x; e < n4; e += 256) {
        float4 pv = p4[e]; const float4 gv = g4[e]; float4 bv = b4[e];
        bv.x = mom * bv.x + fmaf(wd, pv.x, gv.x * gscale); pv.x -= lr * bv.x;
        bv.y = mom * bv.y + fmaf(wd, pv.y, gv.y * gscale); pv.y -= lr * bv.y;
        bv.z = mom * bv.z + fmaf(wd, pv.z, gv.z * gscale); pv.z -= lr * bv.z;
        bv.w = mom * bv.w + fmaf(wd, pv.w, gv.w * gscale); pv.w -= lr * bv.w;
        p4[e] = pv; b4[e] = bv;
        m = abs_bits4(m, pv.x, pv.y, pv.z, pv.w);
    }
    amax_publish(m, rec);           // every thread of the block reaches it; a null record publishes nothing
}
__global__ __launch_bounds__(256) void nan_check_kernel(const float* __restrict__ x, long long n, int* __restrict__ flag) {
    bool bad = false;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) bad |= (x[e] != x[e]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// ---------------------------------------------------------------------------------------------- validation metrics
// CM: the confusion matrix cmh[t * C + p] beside the table, in dynamic LDS behind the staged logits (C <= kSegMetricsCmMaxC keeps both under 64 KB);
// `counts` may then be null.
constexpr int kSegMetricsCmMaxC = 48;
template <bool CM>
__global__ __launch_bounds__(256) void seg_metrics_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                           int ignore_index, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ cm) {
    extern __shared__ float tile[];                     // [256][C] logits; CM: then [C][C] unsigned bins
    __shared__ unsigned hist[3 * 64 + 2];
    unsigned* cmh = reinterpret_cast<unsigned*>(tile + 256 * C);
    for (int t = threadIdx.x; t < 3 * C + 2; t += 256) hist[t] = 0u;
    if (CM)
        for (int t = threadIdx.x; t < C * C; t += 256) cmh[t] = 0u;
    for (long long p0 = (long long)blockIdx.x * 256; p0 < P; p0 += (long long)gridDim.x * 256) {
        const int np = (int)min(256ll, P - p0);
        __syncthreads();
        for (int t = threadIdx.x; t < np * C; t += 256) { const int r = t / C, c = t - r * C; tile[t] = logits[(p0 + r) * ld + c]; }
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int tg = target[p0 + threadIdx.x];
            if (tg != ignore_index && tg < C) {
                const float* v = tile + threadIdx.x * C;
                int best = 0; float bv = v[0];
                for (int c = 1; c < C; ++c) if (v[c] > bv) { bv = v[c]; best = c; }     // first maximum, as torch.argmax
                atomicAdd(&hist[best], 1u);
                atomicAdd(&hist[2 * C + tg], 1u);
                atomicAdd(&hist[3 * C + 1], 1u);
                if (best == tg) { atomicAdd(&hist[C + tg], 1u); atomicAdd(&hist[3 * C], 1u); }
                if (CM) atomicAdd(&cmh[tg * C + best], 1u);
            }
        }
    }
    __syncthreads();
    if (!CM || counts != nullptr)
        for (int t = threadIdx.x; t < 3 * C + 2; t += 256) if (hist[t]) atomicAdd(&counts[t], (unsigned long long)hist[t]);
    if (CM)
        for (int t = threadIdx.x; t < C * C; t += 256) if (cmh[t]) atomicAdd(&cm[t], (unsigned long long)cmh[t]);
}

// ---------------------------------------------------------------------------------------------- confusion matrix of two class maps
// cm[t * C + p] += 1 for every pixel whose target t is counted (t != ignore_index, t < C) and whose predicted class p is < C; a p >= C on a counted
// pixel raises bit 1 of nan_flag instead.  16 pixels of each map per iteration in 16-byte loads, whatever byte either map starts at (block 0 takes
// the head up to the target's first 16-byte boundary and the tail byte by byte).  LDS bins per wave
// (kCmCopies sets when C * C <= kCmCopyBins, else one), merged and flushed once per block as 64-bit atomics: exact and order independent.
constexpr int kCmBlocks = 512;
constexpr int kCmMaxC = 64;
constexpr int kCmCopyBins = 1024, kCmCopies = 4;
constexpr long long kCmLaunchPixels = 1ll << 40;        // per block <= 2^31 + 2^12 pixels: no 32-bit LDS bin can wrap
// A lane's 16 pixels are consecutive: a run of equal (t, p) pairs leaves as ONE LDS atomic of its length, so a map that is one class over most pixels
// does not serialise a wave on one bin.  k < 0: a pixel that is not counted.
struct CmRun {
    int key = -1;
    unsigned n = 0u;
    __device__ __forceinline__ void flush(unsigned* h) { if (n) atomicAdd(&h[key], n); n = 0u; }
    __device__ __forceinline__ void add(unsigned* h, int k) {
        if (k != key) { flush(h); key = k; }
        n += k >= 0 ? 1u : 0u;
    }
};
__device__ __forceinline__ int cm_key(unsigned t, unsigned p, int C, int ignore_index, bool& bad) {
    const bool live = (int)t != ignore_index && (int)t < C;
    bad |= live && (int)p >= C;
    return (live && (int)p < C) ? (int)t * C + (int)p : -1;
}
__global__ __launch_bounds__(256) void confusion_matrix_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ target, long long P, int C,
                                                                int ignore_index, int copies, unsigned long long* __restrict__ cm, int* __restrict__ nan_flag) {
    extern __shared__ unsigned cmbins[];                // [copies][C * C]
    const int bins = C * C;
    for (int t = threadIdx.x; t < copies * bins; t += 256) cmbins[t] = 0u;
    __syncthreads();
    unsigned* h = cmbins + (copies > 1 ? (int)(threadIdx.x >> 6) * bins : 0);
    bool bad = false;
    CmRun run;
    // The body starts at the target's first 16-byte boundary.  pred + head is `m` bytes past a boundary of its own: its 16 pixels come from the two
    // aligned quads that hold them (both hold a pixel of the map, so neither load leaves the 16-byte granules the map occupies), shifted together.
    const long long head = min(P, (long long)((16 - ((uintptr_t)target & 15)) & 15));
    const long long nv = (P - head) >> 4;
    const int m = (int)((uintptr_t)(pred + head) & 15), q = m >> 2, r = m & 3;
    const uint4* pv = reinterpret_cast<const uint4*>(pred + head - m);
    const uint4* tv = reinterpret_cast<const uint4*>(target + head);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long long)gridDim.x * 256) {
        const uint4 qt = tv[e], lo = pv[e];
        unsigned wp[4] = {lo.x, lo.y, lo.z, lo.w};
        if (m) {
            const uint4 hi = pv[e + 1];
            const unsigned w[9] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w, 0u};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned a = q == 0 ? w[u] : q == 1 ? w[u + 1] : q == 2 ? w[u + 2] : w[u + 3];
                const unsigned b = q == 0 ? w[u + 1] : q == 1 ? w[u + 2] : q == 2 ? w[u + 3] : w[u + 4];
                wp[u] = __builtin_amdgcn_alignbyte(b, a, (unsigned)r);          // bytes r .. r + 3 of {b : a}
            }
        }
        const unsigned wt[4] = {qt.x, qt.y, qt.z, qt.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int b = 0; b < 4; ++b) run.add(h, cm_key((wt[u] >> (8 * b)) & 0xffu, (wp[u] >> (8 * b)) & 0xffu, C, ignore_index, bad));
    }
    run.flush(h);
    if (blockIdx.x == 0) {          // scalar head and tail
        for (long long e = threadIdx.x; e < head; e += 256) run.add(h, cm_key(target[e], pred[e], C, ignore_index, bad));
        for (long long e = head + (nv << 4) + threadIdx.x; e < P; e += 256) run.add(h, cm_key(target[e], pred[e], C, ignore_index, bad));
    }
    run.flush(h);
    if (nan_flag != nullptr && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(nan_flag, 2);
    __syncthreads();
    for (int t = threadIdx.x; t < bins; t += 256) {
        unsigned n = cmbins[t];
        for (int c = 1; c < copies; ++c) n += cmbins[c * bins + t];
        if (n) atomicAdd(&cm[t], (unsigned long long)n);
    }
}

// ---------------------------------------------------------------------------------------------- batch preparation
__device__ inline void ac_src_f(int dst, float scale, int n_in, int& i0, int& ip, float& l1) {
    const float r = scale * (float)dst;
    i0 = min((int)r, n_in - 1); ip = (i0 < n_in - 1) ? 1 : 0; l1 = r - (float)i0;
}
__global__ __launch_bounds__(256) void prepare_image_kernel(const unsigned char* __restrict__ rgb, float* __restrict__ out, int N, int Hs, int Ws, int Ho, int Wo, int Cout,
                                                             float sh, float sw, float m0, float m1, float m2, float i0s, float i1s, float i2s) {
    const long long total = (long long)N * Ho * Wo;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int wo = (int)(e % Wo); const long long t = e / Wo; const int ho = (int)(t % Ho); const long long n = t / Ho;
        int h0, hp, w0, wp; float lh, lw;
        ac_src_f(ho, sh, Hs, h0, hp, lh); ac_src_f(wo, sw, Ws, w0, wp, lw);
        const unsigned char* b = rgb + ((n * Hs + h0) * Ws + w0) * 3;
        const long long dw_ = (long long)wp * 3, dh_ = (long long)hp * Ws * 3;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x00 = b[c], x01 = b[dw_ + c], x10 = b[dh_ + c], x11 = b[dh_ + dw_ + c];
            v[c] = (1.f - lh) * ((1.f - lw) * x00 + lw * x01) + lh * ((1.f - lw) * x10 + lw * x11);
        }
        float* o = out + e * Cout;
        o[0] = (v[0] * (1.f / 255.f) - m0) * i0s; o[1] = (v[1] * (1.f / 255.f) - m1) * i1s; o[2] = (v[2] * (1.f / 255.f) - m2) * i2s;
        if (Cout == 4) o[3] = 0.f;
    }
}
__global__ __launch_bounds__(256) void prepare_target_kernel(const unsigned char* __restrict__ labels, const unsigned char* __restrict__ lut, unsigned char* __restrict__ target,
                                                              int N, int Hs, int Ws, int Ho, int Wo) {
    const long long total = (long long)N * Ho * Wo;
    const float sh = (float)Hs / (float)Ho, sw = (float)Ws / (float)Wo;             // torch 'nearest': src = floor(dst * in/out)
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int wo = (int)(e % Wo); const long long t = e / Wo; const int ho = (int)(t % Ho); const long long n = t / Ho;
        const int hs = min((int)floorf((float)ho * sh), Hs - 1), ws = min((int)floorf((float)wo * sw), Ws - 1);
        target[e] = lut[labels[(n * Hs + hs) * Ws + ws]];
    }
}

static int loss_blocks(long long work) { return (int)std::max<long long>(1, std::min<long long>(1024, ceil_div(work, 256))); }

}  // namespace dsrl
using namespace dsrl;

extern "C" size_t dsrl_mse_workspace_bytes(int64_t n) { return (size_t)loss_blocks(n / 4 + 1) * sizeof(double); }
extern "C" int dsrl_mse_fwd(const float* a, const float* b, int64_t n, float* loss_out, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(a && b && loss_out && ws && n > 0, DSRL_E_BADARG, "mse_fwd: bad arguments");
    DSRL_REQUIRE(ws_bytes >= dsrl_mse_workspace_bytes(n), DSRL_E_WORKSPACE, "mse_fwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int nb = loss_blocks(n / 4 + 1);
    hipLaunchKernelGGL(mse_fwd_kernel, dim3(nb), dim3(256), 0, st, a, b, (long long)n, (double*)ws);
    if (int e = launch_status("mse_fwd_kernel")) return e;
    hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nb, (long long)n, loss_out);
    return launch_status("mse_finalize_kernel");
}
extern "C" int dsrl_mse_bwd(const float* a, const float* b, int64_t n, const float* grad_out, float* da, dsrl_stream_t stream) {
    DSRL_REQUIRE(a && b && grad_out && da && n > 0, DSRL_E_BADARG, "mse_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(mse_bwd_kernel, dim3((unsigned)std::min<long long>(ceil_div(n, 1024), 8192)), dim3(256), 0, st, a, b, (long long)n, grad_out, da);
    return launch_status("mse_bwd_kernel");
}

// ---- cross entropy: nn.CrossEntropyLoss(weight, ignore_index, label_smoothing=) and the focal loss.  Four kinds (CeVariant, common.h): plain,
// class-weighted, focal = weighted with one more per-pixel factor (focal_pixel), label-smoothed = weighted plus the smoothing term over all
// classes (smooth_pixel).  The twelve entry points check their gamma or eps, make their CeVariant and hand over to ONE host body per family
// (ce_fwd_any, ce_bwd_any, ce_fused_any): every check, workspace layout and launch decision is written once.
// Every kind but plain starts with the same pre-pass (per-block integer histograms of the labels, then D = sum n_c w_c in one block, left in
// loss_out[1]), so D is the same bits in all of them, and ends with the finalize that divides by D.
static int hist_blocks(long long P) { return (int)std::max<long long>(1, std::min<long long>(kHistBlocks, ceil_div(P, 4096))); }
static constexpr size_t kWeightSumBytes = (size_t)kHistBlocks * 256 * sizeof(unsigned);
size_t dsrl::ce_weight_sum_bytes() { return kWeightSumBytes; }
int dsrl::launch_ce_weight_sum(const unsigned char* target, long long P, int C, int ignore_index, const float* weights, float* d_out, void* ws, hipStream_t st) {
    const int nb = hist_blocks(P);
    hipLaunchKernelGGL(class_hist_kernel, dim3(nb), dim3(256), 0, st, target, P, (const unsigned char*)nullptr, (unsigned long long*)nullptr, (unsigned*)ws);
    if (int e = launch_status("class_hist_kernel")) return e;
    hipLaunchKernelGGL(ce_weight_sum_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)ws, nb, C, ignore_index, weights, d_out);
    return launch_status("ce_weight_sum_kernel");
}
int dsrl::launch_ce_finalize(CeVariant::Kind kind, const double* part, int nb, float* loss_out, hipStream_t st) {
    if (kind == CeVariant::kPlain) {
        hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, part, nb, loss_out);
        return launch_status("ce_finalize_kernel");
    }
    hipLaunchKernelGGL(ce_finalize_w_kernel, dim3(1), dim3(256), 0, st, part, nb, loss_out);
    return launch_status("ce_finalize_w_kernel");
}
// workspaces: two doubles per loss block, then the histograms of the pre-pass (every kind but plain) or, for the plain fused pass, the pixel
// counts of count_valid_kernel
static size_t ce_ws_bytes(int64_t P, bool plain) { return (size_t)2 * loss_blocks(P) * sizeof(double) + (plain ? 0 : kWeightSumBytes); }
static size_t ce_fused_ws_bytes(int64_t P, bool plain) {
    return (size_t)2 * loss_blocks(P) * sizeof(double) + (plain ? kCountBlocks * sizeof(unsigned) : kWeightSumBytes);
}
extern "C" size_t dsrl_ce_workspace_bytes(int64_t P) { return ce_ws_bytes(P, true); }
extern "C" size_t dsrl_ce_w_workspace_bytes(int64_t P) { return ce_ws_bytes(P, false); }
extern "C" size_t dsrl_ce_f_workspace_bytes(int64_t P) { return ce_ws_bytes(P, false); }
extern "C" size_t dsrl_ce_s_workspace_bytes(int64_t P) { return ce_ws_bytes(P, false); }
extern "C" size_t dsrl_ce_r_workspace_bytes(int64_t P) { return ce_ws_bytes(P, false); }
extern "C" size_t dsrl_ce_fused_workspace_bytes(int64_t P) { return ce_fused_ws_bytes(P, true); }
extern "C" size_t dsrl_ce_fused_w_workspace_bytes(int64_t P) { return ce_fused_ws_bytes(P, false); }
extern "C" size_t dsrl_ce_fused_f_workspace_bytes(int64_t P) { return ce_fused_ws_bytes(P, false); }
extern "C" size_t dsrl_ce_fused_s_workspace_bytes(int64_t P) { return ce_fused_ws_bytes(P, false); }
extern "C" size_t dsrl_ce_fused_r_workspace_bytes(int64_t P) { return ce_fused_ws_bytes(P, false); }

static int ce_fwd_any(const CeVariant& v, const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float* loss_out,
                      void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    const char* sfx = v.suffix();
    DSRL_REQUIRE(logits && target && v.table_ok() && loss_out && ws && P > 0 && C > 0 && C <= v.max_classes() && ld >= C, DSRL_E_BADARG,
                 "ce_fwd%s: bad arguments (C=%d)", sfx, C);
    if (v.plain()) DSRL_REQUIRE(ws_bytes >= ce_ws_bytes(P, true), DSRL_E_WORKSPACE, "ce_fwd: workspace too small");
    else DSRL_REQUIRE(ws_bytes >= ce_ws_bytes(P, false) && ((uintptr_t)ws % 8) == 0, DSRL_E_WORKSPACE, "ce_fwd%s: workspace too small or misaligned", sfx);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int nb = loss_blocks(P);
    double* part = (double*)ws;
    if (!v.plain())
        if (int e = launch_ce_weight_sum(target, (long long)P, C, ignore_index, v.weights, loss_out + 1, part + 2 * nb, st)) return e;
    const dim3 grid(nb), block(256);
    const size_t lds = (size_t)256 * C * sizeof(float);
    switch (v.kind) {
    case CeVariant::kPlain: hipLaunchKernelGGL(ce_fwd_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, part); break;
    case CeVariant::kWeighted: hipLaunchKernelGGL(ce_fwd_w_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, part); break;
    case CeVariant::kFocal: hipLaunchKernelGGL(ce_fwd_f_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.gamma, part); break;
    case CeVariant::kSmoothed: hipLaunchKernelGGL(ce_fwd_s_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.eps, part); break;
    case CeVariant::kRelaxed: hipLaunchKernelGGL(ce_fwd_r_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.mask, part); break;
    default: break;         // (kDice, kLovasz: no entry point of this family makes them)
    }
    static const char* const kernel[] = {"ce_fwd_kernel", "ce_fwd_w_kernel", "ce_fwd_f_kernel", "ce_fwd_s_kernel", "", "", "ce_fwd_r_kernel"};
    if (int e = launch_status(kernel[v.kind])) return e;
    return launch_ce_finalize(v.kind, part, nb, loss_out, st);
}
static int ce_bwd_any(const CeVariant& v, const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* loss_out,
                      const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream) {
    DSRL_REQUIRE(logits && target && v.table_ok() && loss_out && grad_out && dlogits && P > 0 && C > 0 && C <= v.max_classes() && ld >= C && lddl >= C, DSRL_E_BADARG,
                 "ce_bwd%s: bad arguments", v.suffix());
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const dim3 grid((unsigned)std::min<long long>(ceil_div(P, 256), 8192)), block(256);
    const size_t lds = (size_t)256 * C * sizeof(float);
    switch (v.kind) {
    case CeVariant::kPlain:
        hipLaunchKernelGGL(ce_bwd_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, loss_out, grad_out, dlogits, lddl);
        break;
    case CeVariant::kWeighted:
        hipLaunchKernelGGL(ce_bwd_w_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, loss_out, grad_out, dlogits, lddl);
        break;
    case CeVariant::kFocal:
        hipLaunchKernelGGL(ce_bwd_f_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.gamma, loss_out, grad_out,
                           dlogits, lddl);
        break;
    case CeVariant::kSmoothed:
        hipLaunchKernelGGL(ce_bwd_s_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.eps, loss_out, grad_out,
                           dlogits, lddl);
        break;
    case CeVariant::kRelaxed:
        hipLaunchKernelGGL(ce_bwd_r_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.mask, loss_out, grad_out,
                           dlogits, lddl);
        break;
    default: break;
    }
    static const char* const kernel[] = {"ce_bwd_kernel", "ce_bwd_w_kernel", "ce_bwd_f_kernel", "ce_bwd_s_kernel", "", "", "ce_bwd_r_kernel"};
    return launch_status(kernel[v.kind]);
}
static int ce_fused_any(const CeVariant& v, const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float* dlogits, int lddl,
                        float* loss_out, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    const char* sfx = v.suffix();
    DSRL_REQUIRE(logits && target && v.table_ok() && loss_out && ws && P > 0 && C > 0 && C <= v.max_classes() && ld >= C && (!dlogits || lddl >= C), DSRL_E_BADARG,
                 "ce_fused%s: bad arguments (C=%d)", sfx, C);
    DSRL_REQUIRE(ws_bytes >= ce_fused_ws_bytes(P, v.plain()) && ((uintptr_t)ws % 8) == 0, DSRL_E_WORKSPACE, "ce_fused%s: workspace too small or misaligned", sfx);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int nb = loss_blocks(P);
    double* part = (double*)ws;
    unsigned* cnt = (unsigned*)(part + 2 * nb);         // plain: the pixel counts; the others: the histograms, and D lands in loss_out[1]
    const float* wsum = loss_out + 1;
    if (v.plain()) {
        hipLaunchKernelGGL(count_valid_kernel, dim3(kCountBlocks), dim3(256), 0, st, target, (long long)P, ignore_index, cnt);
        if (int e = launch_status("count_valid_kernel")) return e;
    } else if (int e = launch_ce_weight_sum(target, (long long)P, C, ignore_index, v.weights, loss_out + 1, cnt, st)) return e;
    const int vec_in = (ld == C && ((uintptr_t)logits % 16) == 0) ? 1 : 0;          // 256 * C floats per tile: every tile starts 16-byte aligned
    const int vec_out = (dlogits && lddl == C && ((uintptr_t)dlogits % 16) == 0) ? 1 : 0;
    const dim3 grid(nb), block(256);
    const size_t lds = (size_t)256 * C * sizeof(float);
    switch (v.kind) {
    case CeVariant::kPlain:
        hipLaunchKernelGGL(ce_fused_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, (const unsigned*)cnt, dlogits, lddl, part,
                           nan_flag, vec_in, vec_out);
        break;
    case CeVariant::kWeighted:
        hipLaunchKernelGGL(ce_fused_w_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, wsum, dlogits, lddl, part,
                           nan_flag, vec_in, vec_out);
        break;
    case CeVariant::kFocal:
        hipLaunchKernelGGL(ce_fused_f_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.gamma, wsum, dlogits, lddl,
                           part, nan_flag, vec_in, vec_out);
        break;
    case CeVariant::kSmoothed:
        hipLaunchKernelGGL(ce_fused_s_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.eps, wsum, dlogits, lddl,
                           part, nan_flag, vec_in, vec_out);
        break;
    case CeVariant::kRelaxed:
        hipLaunchKernelGGL(ce_fused_r_kernel, grid, block, lds, st, logits, ld, target, (long long)P, C, ignore_index, v.weights, v.mask, wsum, dlogits, lddl,
                           part, nan_flag, vec_in, vec_out);
        break;
    default: break;
    }
    static const char* const kernel[] = {"ce_fused_kernel", "ce_fused_w_kernel", "ce_fused_f_kernel", "ce_fused_s_kernel", "", "", "ce_fused_r_kernel"};
    if (int e = launch_status(kernel[v.kind])) return e;
    return launch_ce_finalize(v.kind, part, nb, loss_out, st);
}

// the entry points: gamma or eps first (DSRL_FOCAL_GAMMA, DSRL_LABEL_SMOOTHING), then everything else in the shared body
extern "C" int dsrl_ce_fwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float* loss_out,
                           void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    return ce_fwd_any(CeVariant{}, logits, ld, target, P, C, ignore_index, loss_out, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fwd_w(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float* loss_out,
                             void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    return ce_fwd_any(CeVariant::weighted(weights), logits, ld, target, P, C, ignore_index, loss_out, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fwd_f(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float gamma,
                             float* loss_out, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_FOCAL_GAMMA(gamma, "ce_fwd_f");
    return ce_fwd_any(CeVariant::focal(weights, gamma), logits, ld, target, P, C, ignore_index, loss_out, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fwd_s(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float eps,
                             float* loss_out, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_LABEL_SMOOTHING(eps, "ce_fwd_s");
    return ce_fwd_any(CeVariant::smoothed(weights, eps), logits, ld, target, P, C, ignore_index, loss_out, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fwd_r(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, const uint32_t* mask,
                             float* loss_out, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    return ce_fwd_any(CeVariant::relaxed(weights, mask), logits, ld, target, P, C, ignore_index, loss_out, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_bwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* loss_out,
                           const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream) {
    return ce_bwd_any(CeVariant{}, logits, ld, target, P, C, ignore_index, loss_out, grad_out, dlogits, lddl, stream);
}
extern "C" int dsrl_ce_bwd_w(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, const float* loss_out,
                             const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream) {
    return ce_bwd_any(CeVariant::weighted(weights), logits, ld, target, P, C, ignore_index, loss_out, grad_out, dlogits, lddl, stream);
}
extern "C" int dsrl_ce_bwd_f(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float gamma,
                             const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream) {
    DSRL_FOCAL_GAMMA(gamma, "ce_bwd_f");
    return ce_bwd_any(CeVariant::focal(weights, gamma), logits, ld, target, P, C, ignore_index, loss_out, grad_out, dlogits, lddl, stream);
}
extern "C" int dsrl_ce_bwd_s(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float eps,
                             const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream) {
    DSRL_LABEL_SMOOTHING(eps, "ce_bwd_s");
    return ce_bwd_any(CeVariant::smoothed(weights, eps), logits, ld, target, P, C, ignore_index, loss_out, grad_out, dlogits, lddl, stream);
}
extern "C" int dsrl_ce_bwd_r(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, const uint32_t* mask,
                             const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream) {
    return ce_bwd_any(CeVariant::relaxed(weights, mask), logits, ld, target, P, C, ignore_index, loss_out, grad_out, dlogits, lddl, stream);
}
extern "C" int dsrl_ce_fused(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float* dlogits, int lddl,
                             float* loss_out, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    return ce_fused_any(CeVariant{}, logits, ld, target, P, C, ignore_index, dlogits, lddl, loss_out, nan_flag, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fused_w(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights,
                               float* dlogits, int lddl, float* loss_out, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    return ce_fused_any(CeVariant::weighted(weights), logits, ld, target, P, C, ignore_index, dlogits, lddl, loss_out, nan_flag, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fused_f(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float gamma,
                               float* dlogits, int lddl, float* loss_out, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_FOCAL_GAMMA(gamma, "ce_fused_f");
    return ce_fused_any(CeVariant::focal(weights, gamma), logits, ld, target, P, C, ignore_index, dlogits, lddl, loss_out, nan_flag, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fused_s(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float eps,
                               float* dlogits, int lddl, float* loss_out, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_LABEL_SMOOTHING(eps, "ce_fused_s");
    return ce_fused_any(CeVariant::smoothed(weights, eps), logits, ld, target, P, C, ignore_index, dlogits, lddl, loss_out, nan_flag, ws, ws_bytes, stream);
}
extern "C" int dsrl_ce_fused_r(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, const uint32_t* mask,
                               float* dlogits, int lddl, float* loss_out, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    return ce_fused_any(CeVariant::relaxed(weights, mask), logits, ld, target, P, C, ignore_index, dlogits, lddl, loss_out, nan_flag, ws, ws_bytes, stream);
}

extern "C" int dsrl_class_histogram(const uint8_t* labels, int64_t P, const uint8_t* lut, unsigned long long* counts, dsrl_stream_t stream) {
    DSRL_REQUIRE(labels && counts && P > 0, DSRL_E_BADARG, "class_histogram: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(class_hist_kernel, dim3(hist_blocks(P)), dim3(256), 0, st, labels, (long long)P, lut, counts, (unsigned*)nullptr);
    return launch_status("class_hist_kernel");
}
extern "C" size_t dsrl_ce_weight_sum_workspace_bytes(void) { return kWeightSumBytes; }
extern "C" int dsrl_ce_weight_sum(const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights, float* d_out,
                                  void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(target && weights && d_out && ws && P > 0 && C > 0 && C <= 256, DSRL_E_BADARG, "ce_weight_sum: bad arguments (C=%d)", C);
    DSRL_REQUIRE(ws_bytes >= kWeightSumBytes && ((uintptr_t)ws % 4) == 0, DSRL_E_WORKSPACE, "ce_weight_sum: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    return launch_ce_weight_sum(target, (long long)P, C, ignore_index, weights, d_out, ws, st);
}
extern "C" int dsrl_mse_fused(const float* a, const float* b, int64_t n, float grad_scale, float* da, float* loss_out, int* nan_flag,
                              void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(a && b && loss_out && ws && n > 0, DSRL_E_BADARG, "mse_fused: bad arguments");
    DSRL_REQUIRE(ws_bytes >= dsrl_mse_workspace_bytes(n), DSRL_E_WORKSPACE, "mse_fused: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int nb = loss_blocks(n / 4 + 1);
    const int vec = (((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0 && (!da || ((uintptr_t)da % 16) == 0)) ? 1 : 0;
    hipLaunchKernelGGL(mse_fused_kernel, dim3(nb), dim3(256), 0, st, a, b, (long long)n, 2.f * grad_scale / (float)n, da, (double*)ws, nan_flag, vec);
    if (int e = launch_status("mse_fused_kernel")) return e;
    hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nb, (long long)n, loss_out);
    return launch_status("mse_finalize_kernel");
}
extern "C" int dsrl_loss_mix(const float* ce, const float* mse, const float* fa, float w1, float w2, const int* nan_flag, float* vals, dsrl_stream_t stream) {
    DSRL_REQUIRE(ce && vals, DSRL_E_BADARG, "loss_mix: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(loss_mix_kernel, dim3(1), dim3(64), 0, st, ce, mse, fa, w1, w2, nan_flag, vals);
    return launch_status("loss_mix_kernel");
}

static int fa_dims(int H, int W, int k, int& hp, int& wp) {
    DSRL_REQUIRE(k > 0, DSRL_E_BADARG, "fa_loss: subsample factor %d must be positive", k);
    DSRL_REQUIRE(H >= k && W >= k, DSRL_E_BADARG, "fa_loss: subsample factor %d larger than the %dx%d map", k, H, W);
    hp = H / k; wp = W / k;
    DSRL_REQUIRE(hp <= FA_MAXH && wp <= FA_MAXW, DSRL_E_UNSUPPORTED, "fa_loss: pooled map %dx%d exceeds %dx%d", hp, wp, FA_MAXH, FA_MAXW);
    return DSRL_OK;
}
static long long fa_saved_stride(int hp, int wp) { return 2ll * wp * wp + 2 + 2ll * (hp + wp); }
extern "C" size_t dsrl_fa_saved_floats(int B, int C, int H, int W, int k) {
    if (k <= 0) return 0;
    return (size_t)B * C * fa_saved_stride(H / k, W / k);
}
extern "C" size_t dsrl_fa_workspace_bytes(int B, int C, int H, int W, int k) { (void)H; (void)W; (void)k; return (size_t)B * C * kFaPairBlocks * sizeof(double); }

extern "C" int dsrl_fa_fwd(const float* fm1, const float* fm2, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                           int k, int reduction, float* out, float* saved, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    int hp, wp;
    if (int e = fa_dims(H, W, k, hp, wp)) return e;         // first: k > W leaves a 'none' output of no elements, whose null pointer is not the reason
    DSRL_REQUIRE(fm1 && fm2 && out && saved && ws && B > 0 && C > 0 && reduction >= 0 && reduction <= 2, DSRL_E_BADARG, "fa_fwd: bad arguments");
    DSRL_REQUIRE(ws_bytes >= dsrl_fa_workspace_bytes(B, C, H, W, k), DSRL_E_WORKSPACE, "fa_fwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(fa_sim_kernel, dim3(B * C, 2), dim3(256), 0, st, fm1, fm2, C, hp, wp, k, (long long)sb, (long long)sc, (long long)sh, (long long)sw,
                       saved, fa_saved_stride(hp, wp));
    if (int e = launch_status("fa_sim_kernel")) return e;
    hipLaunchKernelGGL(fa_pairs_kernel, dim3(B * C, kFaPairBlocks), dim3(256), 0, st, (const float*)saved, fa_saved_stride(hp, wp), wp * wp, reduction, out, (double*)ws);
    if (int e = launch_status("fa_pairs_kernel")) return e;
    if (reduction != 2) {
        hipLaunchKernelGGL(fa_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, B * C, wp * wp, reduction, out);
        return launch_status("fa_finalize_kernel");
    }
    return DSRL_OK;
}
extern "C" int dsrl_fa_bwd(const float* fm1, const float* fm2, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                           int k, int reduction, const float* grad_out, const float* saved, float* d1, float* d2, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    (void)ws; (void)ws_bytes;
    DSRL_REQUIRE(fm1 && fm2 && grad_out && saved && d1 && d2 && B > 0 && C > 0, DSRL_E_BADARG, "fa_bwd: bad arguments");
    DSRL_REQUIRE(reduction == 0 || reduction == 1, DSRL_E_UNSUPPORTED, "fa_bwd: only 'mean' and 'sum' reductions have a backward kernel");
    int hp, wp;
    if (int e = fa_dims(H, W, k, hp, wp)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(fa_bwd_kernel, dim3(B * C, 2), dim3(256), 0, st, fm1, fm2, B * C, C, H, W, hp, wp, k, (long long)sb, (long long)sc, (long long)sh, (long long)sw,
                       reduction, grad_out, saved, fa_saved_stride(hp, wp), d1, d2);
    return launch_status("fa_bwd_kernel");
}

extern "C" int dsrl_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale, dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && buf && n > 0, DSRL_E_BADARG, "sgd_step: bad arguments");
    DSRL_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)buf % 16) == 0, DSRL_E_BADARG, "sgd_step: arenas must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)std::min<long long>(ceil_div(n, 1024), 4096)), dim3(256), 0, st, p, g, buf, (long long)n, lr, momentum, weight_decay, grad_scale);
    return launch_status("sgd_kernel");
}
extern "C" int dsrl_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, const float* hyper, dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && buf && hyper && n > 0, DSRL_E_BADARG, "sgd_step_dev: bad arguments");
    DSRL_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)buf % 16) == 0, DSRL_E_BADARG, "sgd_step_dev: arenas must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(sgd_dev_kernel, dim3((unsigned)std::min<long long>(ceil_div(n, 1024), 4096)), dim3(256), 0, st, p, g, buf, (long long)n, hyper);
    return launch_status("sgd_dev_kernel");
}
extern "C" int dsrl_sgd_step_dev_segments(float* p, const float* g, float* buf, const int64_t* table, int64_t nseg, const float* hyper, dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && buf && table && hyper && nseg > 0 && nseg < (1ll << 31), DSRL_E_BADARG, "sgd_step_dev_segments: bad arguments");
    DSRL_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)buf % 16) == 0, DSRL_E_BADARG, "sgd_step_dev_segments: arenas must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(sgd_dev_segments_kernel, dim3((unsigned)nseg), dim3(256), 0, st, p, g, buf, (const long long*)table, hyper);
    return launch_status("sgd_dev_segments_kernel");
}
extern "C" int dsrl_nan_check(const float* x, int64_t n, int* flag, dsrl_stream_t stream) {
    DSRL_REQUIRE(x && flag && n > 0, DSRL_E_BADARG, "nan_check: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(nan_check_kernel, dim3((unsigned)std::min<long long>(ceil_div(n, 2048), 4096)), dim3(256), 0, st, x, (long long)n, flag);
    return launch_status("nan_check_kernel");
}

extern "C" int dsrl_seg_metrics(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index,
                                unsigned long long* counts, dsrl_stream_t stream) {
    DSRL_REQUIRE(logits && target && counts && P > 0 && C > 0 && C <= 60 && ld >= C, DSRL_E_BADARG, "seg_metrics: bad arguments (C=%d)", C);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(seg_metrics_kernel<false>, dim3(loss_blocks(P)), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, (long long)P, C,
                       ignore_index, counts, (unsigned long long*)nullptr);
    return launch_status("seg_metrics_kernel");
}
extern "C" int dsrl_seg_metrics_cm_max_classes(void) { return kSegMetricsCmMaxC; }
extern "C" int dsrl_seg_metrics_cm(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, unsigned long long* counts,
                                   unsigned long long* cm, dsrl_stream_t stream) {
    DSRL_REQUIRE(logits && target && cm && P > 0 && C > 0 && ld >= C, DSRL_E_BADARG, "seg_metrics_cm: bad arguments (C=%d)", C);
    DSRL_REQUIRE(C <= kSegMetricsCmMaxC, DSRL_E_UNSUPPORTED, "seg_metrics_cm: %d classes, the staged logits and the matrix fit the LDS up to %d", C,
                 kSegMetricsCmMaxC);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(seg_metrics_kernel<true>, dim3(loss_blocks(P)), dim3(256), ((size_t)256 * C + (size_t)C * C) * sizeof(float), st, logits, ld, target,
                       (long long)P, C, ignore_index, counts, cm);
    return launch_status("seg_metrics_kernel");
}
extern "C" int dsrl_confusion_matrix_max_classes(void) { return kCmMaxC; }
extern "C" int dsrl_confusion_matrix(const uint8_t* pred, const uint8_t* target, int64_t P, int C, int ignore_index, unsigned long long* cm, int* nan_flag,
                                     dsrl_stream_t stream) {
    DSRL_REQUIRE(pred && target && cm && P > 0 && C > 0, DSRL_E_BADARG, "confusion_matrix: bad arguments (C=%d)", C);
    DSRL_REQUIRE(C <= kCmMaxC, DSRL_E_UNSUPPORTED, "confusion_matrix: %d classes, the LDS bins hold up to %d", C, kCmMaxC);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int copies = C * C <= kCmCopyBins ? kCmCopies : 1;
    for (int64_t done = 0; done < P; done += kCmLaunchPixels) {
        const long long n = std::min<long long>(kCmLaunchPixels, P - done);
        const int nb = (int)std::max<long long>(1, std::min<long long>(kCmBlocks, ceil_div(n, 4096)));
        hipLaunchKernelGGL(confusion_matrix_kernel, dim3(nb), dim3(256), (size_t)copies * C * C * sizeof(unsigned), st, pred + done, target + done, n, C,
                           ignore_index, copies, cm, nan_flag);
        if (int e = launch_status("confusion_matrix_kernel")) return e;
    }
    return DSRL_OK;
}

extern "C" int dsrl_prepare_batch(const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut, const float* mean, const float* std_,
                                  float* img_in, float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W, dsrl_stream_t stream) {
    DSRL_REQUIRE(rgb && mean && std_ && N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, DSRL_E_BADARG, "prepare_batch: bad arguments");
    DSRL_REQUIRE((labels == nullptr) == (target == nullptr) && (labels == nullptr || lut != nullptr), DSRL_E_BADARG, "prepare_batch: labels, lut and target go together");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    auto sc = [](int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; };
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2], i0 = 1.f / std_[0], i1 = 1.f / std_[1], i2 = 1.f / std_[2];
    if (img_in) {
        hipLaunchKernelGGL(prepare_image_kernel, dim3((unsigned)std::min<long long>(ceil_div((long long)N * H * W, 256), 4096)), dim3(256), 0, st,
                           rgb, img_in, N, Hs, Ws, H, W, 4, sc(Hs, H), sc(Ws, W), m0, m1, m2, i0, i1, i2);
        if (int e = launch_status("prepare_image_kernel")) return e;
    }
    if (img_org) {
        hipLaunchKernelGGL(prepare_image_kernel, dim3((unsigned)std::min<long long>(ceil_div((long long)N * 4 * H * W, 256), 4096)), dim3(256), 0, st,
                           rgb, img_org, N, Hs, Ws, 2 * H, 2 * W, 3, sc(Hs, 2 * H), sc(Ws, 2 * W), m0, m1, m2, i0, i1, i2);
        if (int e = launch_status("prepare_image_kernel")) return e;
    }
    if (target) {
        hipLaunchKernelGGL(prepare_target_kernel, dim3((unsigned)std::min<long long>(ceil_div((long long)N * 4 * H * W, 256), 4096)), dim3(256), 0, st,
                           labels, lut, target, N, Hs, Ws, 2 * H, 2 * W);
        return launch_status("prepare_target_kernel");
    }
    return DSRL_OK;
}
