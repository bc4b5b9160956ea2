// Inference tail of the SSSR decoder (DSRL.py:53-69 in eval mode) as ONE launch: ConvTranspose2d k2 s2 (19 -> 19, no bias) -> BatchNorm (running
// statistics) -> ReLU -> ConvTranspose2d k2 s2 (19 -> 19, bias) -> arg-max over the classes, optionally with the validation counters of
// dsrl_seg_metrics and nn.CrossEntropyLoss(ignore_index) of the logits it never writes.
//
// Both ConvTransposes have kernel 2 / stride 2 and eval-mode BatchNorm / ReLU / Dropout are pointwise, so an input pixel owns a disjoint 4x4 patch of
// the class map: per pixel a [19] x [19 x 76] product (the 2x2 mid pixels), then four [19] x [19 x 76] products (their 2x2 logits each).  They run on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation) with the WEIGHTS as the A operand (M = 80 rows: 76 (tap, channel) pairs padded, K = 20:
// 19 channels padded) and 16 PIXELS as the N columns, so that D puts a pixel into a lane and channels into its registers:
//   lane l: pixel px = l & 15 of the wave's tile, group g = l >> 4; D register r of M-tile t is row 16 t + 4 g + r of column px.
//   stage 1: row 16 t + 4 g + r  <->  mid channel cm = 4 t + g, tap1 = r.   Lane (px, g) ends up with mid[px][tap1 = r][cm = 4 t + g], which is exactly
//            the B fragment stage 2 wants from it (B[k = 4 s + (l >> 4)][n = l & 15] for k-step s): register (t = s, r = tap1), no LDS, no shuffle.
//   stage 2: row 16 t + 4 g + r  <->  tap2 = g, class = 4 t + r.            Lane (px, g) holds all 19 logits of output pixel (px, tap1, tap2 = g) in
//            registers: the arg-max (and the softmax of the loss) is lane-local.
// A wave walks tiles of 16 consecutive input pixels (flat over N*H*W, grid-stride); per tile 25 + 4 * 25 MFMAs.  The 50 weight fragments stay in
// registers.  Class indices leave as one aligned 32-bit store per lane (4 horizontally adjacent output pixels, assembled with the lane 16 away).
#include "common.h"
#include <algorithm>
#include <limits.h>

namespace dsrl {

namespace {

constexpr int kPC = 19;                 // channels in, mid, classes
constexpr int kPT = 5;                  // M tiles of 16 rows (80 >= 76) = k-steps of 4 (20 >= 19)
constexpr int kPredMaxBlocks = 512;     // two blocks of 4 waves per CU
using f32x4_p = __attribute__((ext_vector_type(4))) float;

template <bool TGT, bool CE>
__global__ __launch_bounds__(256, 2) void sssr_tail_predict_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w1,
                                                                    const float* __restrict__ bn_mean, const float* __restrict__ bn_invstd,
                                                                    const float* __restrict__ bn_gamma, const float* __restrict__ bn_beta,
                                                                    const float* __restrict__ w2, const float* __restrict__ bias2,
                                                                    unsigned char* __restrict__ pred, const unsigned char* __restrict__ target, int ignore_index,
                                                                    unsigned long long* __restrict__ counts, double* __restrict__ part, int* __restrict__ nan_flag,
                                                                    int H, int W, long long P, int ntiles) {
    __shared__ unsigned hist[3 * kPC + 2];
    __shared__ double shd[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;
    if (TGT) {
        for (int t = tid; t < 3 * kPC + 2; t += 256) hist[t] = 0u;
        __syncthreads();
    }
    // A fragments: A[i = l & 15][k = 4 s + (l >> 4)] of M-tile t
    float a1[kPT][kPT], a2[kPT][kPT];
#pragma unroll
    for (int t = 0; t < kPT; ++t)
#pragma unroll
        for (int s = 0; s < kPT; ++s) {
            const int k = 4 * s + g;
            const int cm = 4 * t + (px >> 2), tap1 = px & 3;
            a1[t][s] = (k < kPC && cm < kPC) ? w1[(k * kPC + cm) * 4 + tap1] : 0.f;
            const int tap2 = px >> 2, cls = 4 * t + (px & 3);
            a2[t][s] = (k < kPC && cls < kPC) ? w2[(k * kPC + cls) * 4 + tap2] : 0.f;
        }
    // BatchNorm of mid channel cm = 4 t + g as bn_apply_kernel evaluates it: fmaf(v, sc, sh), sc = gamma * invstd, sh = beta - mean * sc
    float sc[kPT], sh[kPT];
#pragma unroll
    for (int t = 0; t < kPT; ++t) {
        const int cm = 4 * t + g;
        sc[t] = cm < kPC ? bn_gamma[cm] * bn_invstd[cm] : 0.f;
        sh[t] = cm < kPC ? bn_beta[cm] - bn_mean[cm] * sc[t] : 0.f;
    }
    float bv[4 * kPT];
#pragma unroll
    for (int c = 0; c < 4 * kPT; ++c) bv[c] = (bias2 != nullptr && c < kPC) ? bias2[c] : 0.f;

    const int i2 = g >> 1, j2 = g & 1;
    const long long HW = (long long)H * W;
    const int Wo = 4 * W;
    double ce_loss = 0.0, ce_cnt = 0.0;
    bool bad = false, bad_label = false;
    unsigned nanbits = 0u;

    auto xload = [&](int tile, float (&xb)[kPT]) {
        const long long p = (long long)tile * 16 + px;
#pragma unroll
        for (int s = 0; s < kPT; ++s) xb[s] = (tile < ntiles && p < P && 4 * s + g < kPC) ? x[p * ldx + 4 * s + g] : 0.f;
    };
    const int stride = (int)gridDim.x * 4;
    int tile = (int)blockIdx.x * 4 + wv;
    float xb[kPT], xn[kPT];
    xload(tile, xb);
    for (; tile < ntiles; tile += stride) {
        xload(tile + stride, xn);                   // the next tile's pixels are in flight while this one is computed
        const long long p = (long long)tile * 16 + px;
        const bool valid = p < P;
        const long long pc = valid ? p : P - 1;
        const int n = (int)(pc / HW);
        const int rem = (int)(pc - (long long)n * HW);
        const int h = rem / W, w = rem - h * W;
        const long long obase = ((long long)n * 4 * H + 4 * h) * Wo + 4 * w;        // first byte of the pixel's 4x4 patch
        unsigned tw[2] = {0u, 0u};
        if (TGT && valid) {
            tw[0] = *reinterpret_cast<const unsigned*>(target + obase + (long long)i2 * Wo);
            tw[1] = *reinterpret_cast<const unsigned*>(target + obase + (long long)(2 + i2) * Wo);
        }
        // ---- stage 1: the 2x2 mid pixels
        f32x4_p mid[kPT];
#pragma unroll
        for (int t = 0; t < kPT; ++t) mid[t] = f32x4_p{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < kPT; ++s)
#pragma unroll
            for (int t = 0; t < kPT; ++t) mid[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t][s], xb[s], mid[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < kPT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = fmaf(mid[t][r], sc[t], sh[t]);
                nanbits = max(nanbits, abs_bits(z));        // fmaxf(NaN, 0) = 0: the ReLU would hide a NaN of the input from the logits (lanes past the end hold zeros)
                mid[t][r] = fmaxf(z, 0.f);
            }
        // ---- stage 2: per mid pixel (tap1) the 2x2 logits; this lane's output pixel is (tap1, tap2 = g)
        unsigned packed = 0u;
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            f32x4_p acc[kPT];
#pragma unroll
            for (int t = 0; t < kPT; ++t) acc[t] = f32x4_p{bv[4 * t], bv[4 * t + 1], bv[4 * t + 2], bv[4 * t + 3]};
#pragma unroll
            for (int s = 0; s < kPT; ++s)
#pragma unroll
                for (int t = 0; t < kPT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[t][s], mid[s][T], acc[t], 0, 0, 0);
            float v[kPC];
#pragma unroll
            for (int c = 0; c < kPC; ++c) v[c] = acc[c >> 2][c & 3];
            int best = 0;
            float bestv = v[0];
#pragma unroll
            for (int c = 1; c < kPC; ++c)
                if (v[c] > bestv) { bestv = v[c]; best = c; }           // first maximum, as seg_metrics_kernel and torch.argmax
            packed |= (unsigned)best << (8 * T);
            if (!CE) {
#pragma unroll
                for (int c = 0; c < kPC; ++c) nanbits = max(nanbits, valid ? abs_bits(v[c]) : 0u);
            }
            if (TGT) {
                const int tg = (int)((tw[T >> 1] >> (8 * (2 * (T & 1) + j2))) & 0xffu);
                const bool lab_bad = valid && tg != ignore_index && tg >= kPC;
                bad_label |= lab_bad;
                if (counts != nullptr && valid && tg != ignore_index && tg < kPC) {
                    atomicAdd(&hist[best], 1u);
                    atomicAdd(&hist[2 * kPC + tg], 1u);
                    atomicAdd(&hist[3 * kPC + 1], 1u);
                    if (best == tg) { atomicAdd(&hist[kPC + tg], 1u); atomicAdd(&hist[3 * kPC], 1u); }
                }
                if (CE && valid) {
                    // ce_fused_kernel's arithmetic: max, exp(v - max), sum, log
                    float m = v[0];
#pragma unroll
                    for (int c = 1; c < kPC; ++c) m = fmaxf(m, v[c]);
                    const int ts = min(tg == ignore_index ? 0 : tg, kPC - 1);
                    float vt = v[0];
#pragma unroll
                    for (int c = 1; c < kPC; ++c) vt = (c == ts) ? v[c] : vt;
                    float sum = 0.f;
#pragma unroll
                    for (int c = 0; c < kPC; ++c) sum += exp_nonpos(v[c] - m);
                    bad |= !(sum == sum);               // any NaN logit poisons the sum (fmaxf alone would skip it)
                    if (tg != ignore_index) { ce_loss += (double)(m + logf(sum) - vt); ce_cnt += 1.0; }
                }
            }
        }
        // row 2 i1 + i2 of the patch, columns 2 j1 + j2: this lane has j2, the lane 16 further on has the other one; lane j2 writes row i1 = j2
        const unsigned other = (unsigned)__shfl_xor((int)packed, 16, 64);
        const unsigned b0 = j2 ? (other >> 16) & 0xffu : packed & 0xffu;
        const unsigned b1 = j2 ? (packed >> 16) & 0xffu : other & 0xffu;
        const unsigned b2 = j2 ? (other >> 24) & 0xffu : (packed >> 8) & 0xffu;
        const unsigned b3 = j2 ? (packed >> 24) & 0xffu : (other >> 8) & 0xffu;
        if (valid) *reinterpret_cast<unsigned*>(pred + obase + (long long)(2 * j2 + i2) * Wo) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
#pragma unroll
        for (int s = 0; s < kPT; ++s) xb[s] = xn[s];
    }
    bad |= nanbits > 0x7f800000u;
    if (nan_flag != nullptr && __any(bad) && lane == 0) atomicOr(nan_flag, 1);
    if (TGT && nan_flag != nullptr && __any(bad_label) && lane == 0) atomicOr(nan_flag, 2);
    if (TGT) {
        __syncthreads();
        if (counts != nullptr)
            for (int t = tid; t < 3 * kPC + 2; t += 256)
                if (hist[t]) atomicAdd(&counts[t], (unsigned long long)hist[t]);
    }
    if (CE) {
        if (bad_label) ce_loss = __builtin_nan("");     // torch asserts on such a label; here it poisons the loss, as ce_fused_kernel does
        double l = wave_sum_d(ce_loss), c = wave_sum_d(ce_cnt);
        if (lane == 0) shd[wv] = l;
        __syncthreads();
        l = shd[0] + shd[1] + shd[2] + shd[3];
        __syncthreads();
        if (lane == 0) shd[wv] = c;
        __syncthreads();
        c = shd[0] + shd[1] + shd[2] + shd[3];
        if (tid == 0) { part[2 * blockIdx.x] = l; part[2 * blockIdx.x + 1] = c; }
    }
}

// the per-block partials in block order: the same value whatever order the blocks ran in
__global__ __launch_bounds__(256) void predict_ce_finalize_kernel(const double* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ double sl[256], sn[256];
    double l = 0, n = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { l += part[2 * i]; n += part[2 * i + 1]; }
    sl[threadIdx.x] = l; sn[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sn[threadIdx.x] += sn[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(sl[0] / sn[0]);        // 0/0 = NaN when every pixel is ignored, as torch
        out[1] = (float)sn[0];
    }
}

// Fingerprint of frozen tensors (inference.FrozenOperands): one block per table row {pointer, 32-bit words}, h = sum over the words of
// (w + 1) * K * (2 i + 1) modulo 2^64 - every single-word change moves it (the factor is odd), and the sum does not depend on the order the threads
// add in.  With `expect` the block compares instead of (or besides) storing and raises `bit` in `flag` on a difference.
constexpr int kFingerprintSegWords = 32768;
__global__ __launch_bounds__(256) void fingerprint_segments_kernel(const long long* __restrict__ table, unsigned long long* __restrict__ out,
                                                                   const unsigned long long* __restrict__ expect, int* __restrict__ flag, int bit) {
    __shared__ unsigned long long sh[4];
    const unsigned* p = reinterpret_cast<const unsigned*>(table[2 * blockIdx.x]);
    const unsigned n = (unsigned)table[2 * blockIdx.x + 1];
    constexpr unsigned long long K = 0x9E3779B97F4A7C15ull;
    unsigned long long h = 0ull;
    unsigned done = 0u;
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0u) {
        const unsigned n4 = n >> 2;
        const uint4* p4 = reinterpret_cast<const uint4*>(p);
        for (unsigned i = threadIdx.x; i < n4; i += 256u) {
            const uint4 v = p4[i];
            const unsigned long long i0 = 8ull * i + 1ull;         // 2 (4 i) + 1
            h += ((unsigned long long)v.x + 1ull) * (K * i0) + ((unsigned long long)v.y + 1ull) * (K * (i0 + 2ull)) +
                 ((unsigned long long)v.z + 1ull) * (K * (i0 + 4ull)) + ((unsigned long long)v.w + 1ull) * (K * (i0 + 6ull));
        }
        done = n4 << 2;
    }
    for (unsigned i = done + threadIdx.x; i < n; i += 256u) h += ((unsigned long long)p[i] + 1ull) * (K * (2ull * i + 1ull));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += (unsigned long long)__shfl_xor((long long)h, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        h = sh[0] + sh[1] + sh[2] + sh[3];
        if (out != nullptr) out[blockIdx.x] = h;
        if (expect != nullptr && flag != nullptr && expect[blockIdx.x] != h) atomicOr(flag, bit);
    }
}

int predict_blocks(long long P) { return (int)std::max<long long>(1, std::min<long long>(kPredMaxBlocks, ceil_div(ceil_div(P, 16), 4))); }

}  // namespace

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_sssr_tail_predict_supported(int N, int H, int W, int Cin, int Cmid, int Cout) {
    if (N < 1 || H < 1 || W < 1 || Cin != kPC || Cmid != kPC || Cout != kPC) return 0;
    return (long long)N * H * W * 16 <= (long long)INT_MAX ? 1 : 0;
}

extern "C" size_t dsrl_sssr_tail_predict_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return (size_t)2 * predict_blocks((long long)N * H * W) * sizeof(double);
}

extern "C" int dsrl_sssr_tail_predict(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                      const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2, uint8_t* pred,
                                      const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws,
                                      size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(x && w1 && bn_mean && bn_invstd && bn_gamma && bn_beta && w2 && pred && N > 0 && H > 0 && W > 0, DSRL_E_BADARG,
                 "sssr_tail_predict: null pointer or empty shape");
    DSRL_REQUIRE(dsrl_sssr_tail_predict_supported(N, H, W, Cin, Cmid, Cout), DSRL_E_UNSUPPORTED,
                 "sssr_tail_predict: needs 19 -> 19 -> 19 channels and N*H*W*16 < 2^31 (got %d -> %d -> %d, %d x %d x %d)", Cin, Cmid, Cout, N, H, W);
    DSRL_REQUIRE(ldx >= Cin && ((uintptr_t)x % 4) == 0 && ((uintptr_t)pred % 4) == 0 && ((uintptr_t)target % 4) == 0, DSRL_E_BADARG,
                 "sssr_tail_predict: ldx < Cin, or x / pred / target not 4-byte aligned");
    DSRL_REQUIRE(target || (!counts && !ce_out), DSRL_E_BADARG, "sssr_tail_predict: counts / ce_out need a target");
    const long long P = (long long)N * H * W;
    const int nb = predict_blocks(P);
    DSRL_REQUIRE(!ce_out || (ws && ws_bytes >= dsrl_sssr_tail_predict_workspace_bytes(N, H, W) && ((uintptr_t)ws % 8) == 0), DSRL_E_WORKSPACE,
                 "sssr_tail_predict: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int ntiles = (int)ceil_div(P, 16);
    double* part = (double*)ws;
#define DSRL_PREDICT_LAUNCH(TGT, CE)                                                                                                                   \
    hipLaunchKernelGGL((sssr_tail_predict_kernel<TGT, CE>), dim3(nb), dim3(256), 0, st, x, ldx, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, \
                       pred, target, ignore_index, counts, part, nan_flag, H, W, P, ntiles)
    if (!target) DSRL_PREDICT_LAUNCH(false, false);
    else if (!ce_out) DSRL_PREDICT_LAUNCH(true, false);
    else DSRL_PREDICT_LAUNCH(true, true);
#undef DSRL_PREDICT_LAUNCH
    if (int e = launch_status("sssr_tail_predict_kernel")) return e;
    if (ce_out) {
        hipLaunchKernelGGL(predict_ce_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nb, ce_out);
        return launch_status("predict_ce_finalize_kernel");
    }
    return DSRL_OK;
}

extern "C" int dsrl_fingerprint_segment_words(void) { return kFingerprintSegWords; }

extern "C" int dsrl_fingerprint_segments(const int64_t* table, int64_t nseg, uint64_t* out, const uint64_t* expect, int* flag, int bit, dsrl_stream_t stream) {
    DSRL_REQUIRE(table && nseg > 0 && nseg <= INT_MAX && (out || (expect && flag)), DSRL_E_BADARG,
                 "fingerprint_segments: null table, no rows, or neither an output nor (expect, flag)");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(fingerprint_segments_kernel, dim3((unsigned)nseg), dim3(256), 0, st, (const long long*)table, (unsigned long long*)out,
                       (const unsigned long long*)expect, flag, bit);
    return launch_status("fingerprint_segments_kernel");
}
