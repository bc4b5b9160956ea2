// Soft Dice loss term beside the cross entropy: loss = CE + lambda L_dice, L_dice = 1 - mean over the classes PRESENT in the call of
// (2 I_c + smooth) / (P_c + G_c + smooth), with I_c = sum_i p_ic [t_i == c], P_c = sum_i p_ic, G_c = sum_i [t_i == c] over the live pixels (label
// neither ignore_index nor >= C) and p the softmax.  The gradient of a pixel depends on the batch only through the 2 C coefficients a_c, b_c:
//     dsrl_dice_fwd   one streaming pass over the logits -> per-chunk partials of I_c, P_c (double) and G_c (integer); a one-block finish reduces them
//                     in a fixed ascending order (the chunks of a group of 64, then the groups) and writes the record {lambda L_dice, |K|, a[0..C), b[0..C)} (kDiceRecordFloats floats)
//     dsrl_dice_bwd   dlogits (+)= the Dice row of every pixel from the logits and the record (dice_pixel / dice_grad of common.h, which the
//                     ConvTranspose backward of convt_dma.hip uses too)
// No float atomics anywhere and a pixel -> chunk mapping that depends on P alone: the record has the same bits on every call.
#include "common.h"
#include <algorithm>

namespace dsrl {

constexpr int kDiceMaxChunks = 1024;            // partial sums [chunk][...]; a chunk is a run of consecutive 256-pixel tiles
constexpr int kDiceStride = 64;                 // classes per row of the partials and of the totals (C <= kDiceMaxC)
// the workspace: the totals {double I[64], double P[64], unsigned G[64]} first (what the finish leaves for a reader), then the partials
constexpr size_t kDiceTotalBytes = (size_t)kDiceStride * (2 * sizeof(double) + sizeof(unsigned));
constexpr size_t kDiceChunkBytes = (size_t)kDiceStride * (2 * sizeof(double) + sizeof(unsigned));

static int dice_tiles(long long P) { return (int)ceil_div(P, 256); }
static int dice_chunks(long long P) { return std::min(kDiceMaxChunks, dice_tiles(P)); }
static int dice_tiles_per_chunk(long long P) { return (int)ceil_div(dice_tiles(P), dice_chunks(P)); }

// The staging of ce_fused_kernel: a block takes 256 pixels x C logits through LDS (16-byte loads when the rows are dense and the base aligned), 32-bit
// indices throughout.
__device__ __forceinline__ void dice_stage(float* tile, const float* __restrict__ logits, int ld, int p0, int np, int C, int vec_in) {
    const int nf = np * C;
    if (vec_in) {               // dense rows: 256 pixels are one contiguous run that starts on a 16-byte boundary
        const float4* src = reinterpret_cast<const float4*>(logits + (size_t)p0 * C);
        for (int t = threadIdx.x; t < (nf >> 2); t += 256) reinterpret_cast<float4*>(tile)[t] = src[t];
        for (int t = (nf & ~3) + threadIdx.x; t < nf; t += 256) tile[t] = logits[(size_t)p0 * C + t];
    } else {
        for (int t = threadIdx.x; t < nf; t += 256) { const int r = t / C, c = t - r * C; tile[t] = logits[(size_t)(p0 + r) * ld + c]; }
    }
}

// ---------------------------------------------------------------------------------------------- class sums
// Block `chunk` takes the tiles [chunk * tpc, (chunk + 1) * tpc).  Per tile: one thread per pixel turns its row into p_c = e_c (1 / s) in place (zeros
// for a pixel that is not live), then the 256 threads sum the columns - thread (slot, c) the pixels slot, slot + G, ... of class c, G = 256 / C, in
// double - and carry the sums from tile to tile.  At the end the G slots of a class are added in ascending slot order.  Everything is a fixed
// function of P and C: the partials have the same bits whatever else runs.
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, int P, int C,
                                                         int ignore_index, int tpc, int ntiles, double* __restrict__ part_ip, unsigned* __restrict__ part_g,
                                                         int* __restrict__ nan_flag, int vec_in) {
    extern __shared__ __attribute__((aligned(16))) float tile[];         // [256][C]
    __shared__ int tg_s[256];
    __shared__ double red_i[256], red_p[256];
    __shared__ unsigned red_g[256];
    const int G = 256 / C;
    const int tid = threadIdx.x;
    const bool summer = tid < G * C;
    const int slot = tid / C, cls = tid - slot * C;
    double acc_i = 0.0, acc_p = 0.0;
    unsigned acc_g = 0u;
    bool bad = false;
    const int t0 = (int)blockIdx.x * tpc, t1 = min(t0 + tpc, ntiles);
    for (int tl = t0; tl < t1; ++tl) {
        const int p0 = tl * 256;
        const int np = min(256, P - p0);
        __syncthreads();
        dice_stage(tile, logits, ld, p0, np, C, vec_in);
        __syncthreads();
        if (tid < np) {
            const int tg = target[p0 + tid];
            const bool live = tg != ignore_index && tg < C;
            float* v = tile + tid * C;
            float m = v[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; v[c] = e; }
            bad |= live && !(s == s);           // any NaN logit poisons the sum (fmaxf alone would skip it)
            const float inv_s = 1.f / s;
            for (int c = 0; c < C; ++c) v[c] = live ? v[c] * inv_s : 0.f;
            tg_s[tid] = live ? tg : -1;
        }
        __syncthreads();
        if (summer) {
            for (int k = slot; k < np; k += G) {
                const double p = (double)tile[k * C + cls];
                const bool hit = tg_s[k] == cls;
                acc_p += p;
                if (hit) { acc_i += p; acc_g += 1u; }
            }
        }
    }
    red_i[tid] = acc_i; red_p[tid] = acc_p; red_g[tid] = acc_g;
    __syncthreads();
    if (tid < C) {
        double si = 0.0, sp = 0.0;
        unsigned sg = 0u;
        for (int g = 0; g < G; ++g) { si += red_i[g * C + tid]; sp += red_p[g * C + tid]; sg += red_g[g * C + tid]; }
        part_ip[(size_t)blockIdx.x * 2 * kDiceStride + tid] = si;
        part_ip[(size_t)blockIdx.x * 2 * kDiceStride + kDiceStride + tid] = sp;
        part_g[(size_t)blockIdx.x * kDiceStride + tid] = sg;
    }
    if (nan_flag && __any(bad) && (tid & 63) == 0) atomicOr(nan_flag, 1);
}

// One block of 16 x 64 threads.  Thread (g, c) adds the partials of class c over the chunks [64 g, 64 g + 64) in ascending order (the loads of a group
// are independent of its sums: one thread walking all 1024 chunks was a chain of 1024 memory latencies: 529 us for the call at 4.19 M pixels against 151 us this way); thread (0, c) then adds the 16 group
// sums in ascending g.  The order is a fixed function of the chunk index, so the totals have the same bits on every call.  The present classes are
// counted, and the coefficients are formed in double and rounded once:  den = P + G + smooth, dice = (2 I + smooth) / den,
// a = -(lambda / |K|) 2 / den, b = (lambda / |K|) (2 I + smooth) / den^2 for a class with G > 0, zeros otherwise;
// L = 1 - (sum of dice over the present classes, c ascending) / |K|, 0 when no class is present.
constexpr int kDiceFinishGroups = kDiceMaxChunks / 64;
__global__ __launch_bounds__(kDiceFinishGroups * 64) void dice_finish_kernel(const double* __restrict__ part_ip, const unsigned* __restrict__ part_g, int nchunks, int C,
                                                                            float lambda, float smooth, double* __restrict__ tot_i, double* __restrict__ tot_p,
                                                                            unsigned* __restrict__ tot_g, float* __restrict__ record) {
    __shared__ double grp_i[kDiceFinishGroups][kDiceStride], grp_p[kDiceFinishGroups][kDiceStride];
    __shared__ unsigned grp_g[kDiceFinishGroups][kDiceStride];
    __shared__ double dice_s[kDiceStride];
    __shared__ unsigned g_s[kDiceStride];
    const int c = threadIdx.x & 63, grp = threadIdx.x >> 6;
    double si = 0.0, sp = 0.0;
    unsigned sg = 0u;
    if (c < C) {
        const int b1 = min(64 * grp + 64, nchunks);
#pragma unroll 8
        for (int b = 64 * grp; b < b1; ++b) {
            si += part_ip[(size_t)b * 2 * kDiceStride + c];
            sp += part_ip[(size_t)b * 2 * kDiceStride + kDiceStride + c];
            sg += part_g[(size_t)b * kDiceStride + c];
        }
    }
    grp_i[grp][c] = si; grp_p[grp][c] = sp; grp_g[grp][c] = sg;
    __syncthreads();
    if (grp == 0) {
        si = 0.0; sp = 0.0; sg = 0u;
        for (int g = 0; g < kDiceFinishGroups; ++g) { si += grp_i[g][c]; sp += grp_p[g][c]; sg += grp_g[g][c]; }
        tot_i[c] = si; tot_p[c] = sp; tot_g[c] = sg;
        g_s[c] = sg;
    }
    __syncthreads();
    const bool lead = grp == 0;                 // the first wave holds the totals
    int K = 0;
    for (int j = 0; j < C; ++j) K += g_s[j] > 0u ? 1 : 0;
    const double lk = K ? (double)lambda / (double)K : 0.0;
    const bool present = c < C && sg > 0u;
    const double den = sp + (double)sg + (double)smooth;
    const double num = 2.0 * si + (double)smooth;
    if (lead) dice_s[c] = present ? num / den : 0.0;
    if (lead && c < C) {
        record[2 + c] = present ? (float)(-lk * 2.0 / den) : 0.f;
        record[2 + C + c] = present ? (float)(lk * num / (den * den)) : 0.f;
    }
    if (lead)
        for (int o = 2 + 2 * C + c; o < kDiceRecordFloats; o += 64) record[o] = 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int j = 0; j < C; ++j) sum += dice_s[j];
        const double L = K ? 1.0 - sum / (double)K : 0.0;
        record[0] = (float)((double)lambda * L);
        record[1] = (float)K;
    }
}

// ---------------------------------------------------------------------------------------------- gradient
// ce_fused_kernel's staging and softmax terms, then the row through dice_pixel / dice_grad.  accumulate: dl = dl + row (an ignored pixel adds +0).
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, int P, int C,
                                                        int ignore_index, const float* __restrict__ record, int accumulate, float* __restrict__ dl, int lddl,
                                                        int ntiles, int vec_in, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) float tile[];         // [256][C]
    __shared__ float a_s[kDiceStride], b_s[kDiceStride];
    const int tid = threadIdx.x;
    if (tid < kDiceStride) { a_s[tid] = tid < C ? record[2 + tid] : 0.f; b_s[tid] = tid < C ? record[2 + C + tid] : 0.f; }
    for (int tl = (int)blockIdx.x; tl < ntiles; tl += (int)gridDim.x) {
        const int p0 = tl * 256;
        const int np = min(256, P - p0);
        const int nf = np * C;
        __syncthreads();
        dice_stage(tile, logits, ld, p0, np, C, vec_in);
        __syncthreads();
        if (tid < np) {
            const int tg = target[p0 + tid];
            const bool live = tg != ignore_index && tg < C;
            float* v = tile + tid * C;
            float m = v[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; v[c] = e; }
            float inv_s, a_t, dot;
            dice_pixel<0>(v, C, s, tg, live, a_s, b_s, inv_s, a_t, dot);
            for (int c = 0; c < C; ++c) v[c] = dice_grad(v[c], inv_s, b_s[c], c == tg, a_t, dot, live);
        }
        __syncthreads();
        if (vec_out) {
            float4* dst = reinterpret_cast<float4*>(dl + (size_t)p0 * C);
            for (int t = tid; t < (nf >> 2); t += 256) {
                float4 r = reinterpret_cast<const float4*>(tile)[t];
                if (accumulate) { const float4 o = dst[t]; r.x = o.x + r.x; r.y = o.y + r.y; r.z = o.z + r.z; r.w = o.w + r.w; }
                dst[t] = r;
            }
            for (int t = (nf & ~3) + tid; t < nf; t += 256) { float* o = dl + (size_t)p0 * C + t; *o = accumulate ? *o + tile[t] : tile[t]; }
        } else {
            for (int t = tid; t < nf; t += 256) {
                const int r = t / C, c = t - r * C;
                float* o = dl + (size_t)(p0 + r) * lddl + c;
                *o = accumulate ? *o + tile[t] : tile[t];
            }
        }
    }
}

}  // namespace dsrl
using namespace dsrl;

#define DSRL_DICE_P(P, what) DSRL_REQUIRE((P) <= 0x7fffffffll - 256, DSRL_E_BADARG, what ": P = %lld does not fit the 32-bit indices", (long long)(P))
// lambda: a finite number > 0; smooth: a finite number >= 0 (a NaN fails the comparisons)
#define DSRL_DICE_SCALARS(lambda, smooth, what)                                                                                                       \
    DSRL_REQUIRE((lambda) > 0.f && (lambda) <= 3.402823466e+38f && (smooth) >= 0.f && (smooth) <= 3.402823466e+38f, DSRL_E_BADARG,                    \
                 what ": lambda = %g must be a finite number > 0 and smooth = %g a finite number >= 0", (double)(lambda), (double)(smooth))

extern "C" size_t dsrl_dice_workspace_bytes(int64_t P) {
    if (P <= 0 || P > 0x7fffffffll - 256) { set_error("dice_workspace_bytes: bad arguments (P=%lld)", (long long)P); return 0; }
    return kDiceTotalBytes + (size_t)dice_chunks(P) * kDiceChunkBytes;
}
extern "C" int dsrl_dice_fwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float lambda, float smooth, float* record,
                             int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_DICE_SCALARS(lambda, smooth, "dice_fwd");
    DSRL_REQUIRE(logits && target && record && ws && P > 0 && C > 0 && C <= kDiceMaxC && ld >= C && ((uintptr_t)record % 4) == 0, DSRL_E_BADARG,
                 "dice_fwd: bad arguments (C=%d)", C);
    DSRL_DICE_P(P, "dice_fwd");
    DSRL_REQUIRE(ws_bytes >= dsrl_dice_workspace_bytes(P) && ((uintptr_t)ws % 8) == 0, DSRL_E_WORKSPACE, "dice_fwd: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    double* tot_i = (double*)ws;
    double* tot_p = tot_i + kDiceStride;
    unsigned* tot_g = (unsigned*)(tot_p + kDiceStride);
    double* part_ip = (double*)((char*)ws + kDiceTotalBytes);
    const int nchunks = dice_chunks(P);
    unsigned* part_g = (unsigned*)(part_ip + (size_t)nchunks * 2 * kDiceStride);
    const int vec_in = (ld == C && ((uintptr_t)logits % 16) == 0) ? 1 : 0;          // 256 * C floats per tile: every tile starts 16-byte aligned
    hipLaunchKernelGGL(dice_sums_kernel, dim3(nchunks), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, (int)P, C, ignore_index,
                       dice_tiles_per_chunk(P), dice_tiles(P), part_ip, part_g, nan_flag, vec_in);
    if (int e = launch_status("dice_sums_kernel")) return e;
    hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(kDiceFinishGroups * 64), 0, st, (const double*)part_ip, (const unsigned*)part_g, nchunks, C, lambda, smooth, tot_i, tot_p,
                       tot_g, record);
    return launch_status("dice_finish_kernel");
}
extern "C" int dsrl_dice_bwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* record, int accumulate,
                             float* dlogits, int lddl, dsrl_stream_t stream) {
    DSRL_REQUIRE(logits && target && record && dlogits && P > 0 && C > 0 && C <= kDiceMaxC && ld >= C && lddl >= C && (accumulate == 0 || accumulate == 1) &&
                 ((uintptr_t)record % 4) == 0, DSRL_E_BADARG, "dice_bwd: bad arguments (C=%d)", C);
    DSRL_DICE_P(P, "dice_bwd");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int vec_in = (ld == C && ((uintptr_t)logits % 16) == 0) ? 1 : 0;
    const int vec_out = (lddl == C && ((uintptr_t)dlogits % 16) == 0) ? 1 : 0;
    const int ntiles = dice_tiles(P);
    hipLaunchKernelGGL(dice_bwd_kernel, dim3(std::min(1024, ntiles)), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, (int)P, C, ignore_index,
                       record, accumulate, dlogits, lddl, ntiles, vec_in, vec_out);
    return launch_status("dice_bwd_kernel");
}
