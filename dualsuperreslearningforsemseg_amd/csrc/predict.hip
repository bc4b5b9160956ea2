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

// CAL: the calibration record of the class map against target (common.h: CalBins, in LDS beside cmh); CONF: the confidence map (N,4H,4W), one aligned
// 16-byte store per lane - the four columns of a patch row assembled with the lane 16 away, as the class bytes are.  Both take the confidence from the
// softmax denominator the loss forms (CE) or form it the same way (softmax_denominator); a patch whose input pixel held a NaN in front of the ReLU has
// NaN confidence (the ReLU hides it from the logits): in no bin, NaN in the map.  Without them the kernel is the one that does not know them.
// TEMP: temperature scaling (common.h: temperature_scale) - behind the arg-max the 19 logits in registers become v_c * beta, and the loss, the
// confidence and the calibration bins come from the scaled values through the code that is there; the class map and the counters do not change.
// (In the flip kernel each view's logits are scaled in front of that view's max / exp: the ensemble is that of the scaled model.)
template <bool TGT, bool CE, bool CM, bool CAL = false, bool CONF = false, bool TEMP = false>
__global__ __launch_bounds__(256, 2) void sssr_tail_predict_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w1,
                                                                    const float* __restrict__ bn_mean, const float* __restrict__ bn_invstd,
                                                                    const float* __restrict__ bn_gamma, const float* __restrict__ bn_beta,
                                                                    const float* __restrict__ w2, const float* __restrict__ bias2,
                                                                    unsigned char* __restrict__ pred, const unsigned char* __restrict__ target, int ignore_index,
                                                                    unsigned long long* __restrict__ counts, double* __restrict__ part, int* __restrict__ nan_flag,
                                                                    int H, int W, long long P, int ntiles, unsigned long long* __restrict__ cm,
                                                                    unsigned long long* __restrict__ cal, int B, float* __restrict__ conf, float beta) {
    static_assert(!CM || TGT, "the confusion matrix needs a target");
    static_assert(!CAL || TGT, "the calibration record needs a target");
    __shared__ unsigned hist[3 * kPC + 2];
    __shared__ unsigned cmh[CM ? kPC * kPC : 1];           // CM: cmh[t * kPC + p], per block at most what hist[3 * kPC + 1] receives
    __shared__ unsigned long long calraw[CAL ? sizeof(CalBins) / 8 : 1];
    CalBins& calb = *reinterpret_cast<CalBins*>(calraw);
    __shared__ double shd[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;
    if (TGT) {
        for (int t = tid; t < 3 * kPC + 2; t += 256) hist[t] = 0u;
        if (CM)
            for (int t = tid; t < kPC * kPC; t += 256) cmh[t] = 0u;
        if (CAL) calb.clear(B);
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
        unsigned tilebits = 0u;                     // CAL / CONF: a NaN in front of this pixel's ReLU
        float cf[4] = {0.f, 0.f, 0.f, 0.f};         // CAL / CONF: the confidence of this lane's four output pixels
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
                // fmaxf(NaN, 0) = 0: the ReLU would hide a NaN of the input from the logits (lanes past the end hold zeros)
                if (CAL || CONF) tilebits = max(tilebits, abs_bits(z));
                else nanbits = max(nanbits, abs_bits(z));
                mid[t][r] = fmaxf(z, 0.f);
            }
        // ---- stage 2: per mid pixel (tap1) the 2x2 logits; this lane's output pixel is (tap1, tap2 = g)
        // packed: the class of output pixel T in bits 0-4 of byte T.  CAL / CONF keep their flags in the free bits and mask them off below: bit 7 of
        // byte 0 = a NaN in front of this pixel's ReLU, bits 5 / 6 of byte T = pixel T is counted / is a hit (binned behind the T loop, where few
        // registers are live)
        unsigned packed = 0u;
        if (CAL || CONF) { nanbits = max(nanbits, tilebits); packed = tilebits > 0x7f800000u ? 0x80u : 0u; }
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            f32x4_p acc[kPT];
#pragma unroll
            for (int t = 0; t < kPT; ++t) acc[t] = f32x4_p{bv[4 * t], bv[4 * t + 1], bv[4 * t + 2], bv[4 * t + 3]};
            // The map-only build (no target) has no LDS traffic between two output pixels: left alone the compiler runs the next pixel's MFMAs ahead of
            // this one's softmax arithmetic and spills one register.  An empty asm statement keeps their order, as in the flip kernel: the first k-step's
            // operand passes through one that needs the class byte of the pixel before.
            float m0 = mid[0][T];
            // (The TEMP build holds one value more per pixel, beta, and spilled again: there the operand also waits for the confidence of the pixel before.)
            if (CONF && !TGT) {
                if (TEMP && T > 0) asm volatile("" : "+v"(packed), "+v"(m0), "+v"(cf[T - 1]));
                else asm volatile("" : "+v"(packed), "+v"(m0));
            }
#pragma unroll
            for (int s = 0; s < kPT; ++s)
#pragma unroll
                for (int t = 0; t < kPT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[t][s], s == 0 ? m0 : mid[s][T], acc[t], 0, 0, 0);
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
            if (TEMP) {         // softmax(beta v): the class above is that of v (beta > 0 is monotone under rounding); loss and confidence below are the scaled model's
#pragma unroll
                for (int c = 0; c < kPC; ++c) v[c] = temperature_scale(v[c], beta);
            }
            float csum = 0.f;
            if ((CAL || CONF) && !CE) csum = softmax_denominator<kPC>(v, kPC);
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
                if (CM && valid && tg != ignore_index && tg < kPC) atomicAdd(&cmh[tg * kPC + best], 1u);
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
                    if (CAL || CONF) csum = sum;
                    if (tg != ignore_index) { ce_loss += (double)(m + logf(sum) - vt); ce_cnt += 1.0; }
                }
                if (CAL || CONF) cf[T] = (packed & 0x80u) ? __builtin_nanf("") : confidence_pixel(csum);
                if (CAL && valid && tg != ignore_index && tg < kPC) packed |= (best == tg ? 0x60u : 0x20u) << (8 * T);
            } else if (CONF) {
                cf[T] = (packed & 0x80u) ? __builtin_nanf("") : confidence_pixel(csum);
            }
        }
        // row 2 i1 + i2 of the patch, columns 2 j1 + j2: this lane has j2, the lane 16 further on has the other one; lane j2 writes row i1 = j2
        const unsigned other = (unsigned)__shfl_xor((int)packed, 16, 64);
        constexpr unsigned kCls = (CAL || CONF) ? 0x1fu : 0xffu;
        const unsigned b0 = j2 ? (other >> 16) & kCls : packed & kCls;
        const unsigned b1 = j2 ? (packed >> 16) & kCls : other & kCls;
        const unsigned b2 = j2 ? (other >> 24) & kCls : (packed >> 8) & kCls;
        const unsigned b3 = j2 ? (packed >> 24) & kCls : (other >> 8) & kCls;
        if (valid) *reinterpret_cast<unsigned*>(pred + obase + (long long)(2 * j2 + i2) * Wo) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        if (CAL) {
#pragma unroll
            for (int T = 0; T < 4; ++T)
                if ((packed >> (8 * T)) & 0x20u) calb.count(cf[T], ((packed >> (8 * T)) & 0x40u) != 0u, B);
        }
        if (CONF) {
            // the same row: this lane's two columns and the two of the lane 16 away, which needs this lane's other pair
            const float s0 = __shfl_xor(j2 ? cf[0] : cf[2], 16, 64), s1 = __shfl_xor(j2 ? cf[1] : cf[3], 16, 64);
            const f32x4_p row = j2 ? f32x4_p{s0, cf[2], s1, cf[3]} : f32x4_p{cf[0], s0, cf[1], s1};
            if (valid) *reinterpret_cast<f32x4_p*>(conf + obase + (long long)(2 * j2 + i2) * Wo) = row;
        }
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
        if (CM)
            for (int t = tid; t < kPC * kPC; t += 256)
                if (cmh[t]) atomicAdd(&cm[t], (unsigned long long)cmh[t]);
        if (CAL) calb.flush(cal, B);
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

// Horizontal-flip ensemble of the same tail: x holds 2 N images, image N + n is the tail input of the MIRRORED image n, still in the mirrored frame.
// The lane of pixel p = (n, h, w) also loads pixel (N + n, h, W - 1 - w), whose 4x4 patch is the same patch of the class map mirrored left to right:
// its output pixel (tap1 = (i1, j1), tap2 = (i2, j2)) in the un-mirrored frame is view b's ((i1, 1 - j1), (i2, 1 - j2)).  Tap indices are 2 i + j, so
// stage-2 step T feeds view b's mid[.][T ^ 1] to a second set of stage-2 fragments built with tap2 ^ 1 (a2b), and the lane that holds the 19 logits of an
// output pixel of view a then holds the 19 logits of view b for the SAME pixel.  Per view: max, exp(v - max), sum; the class is the first maximum of
// ea_c / sa + eb_c / sb, the loss -(logaddexp(la_t, lb_t) - ln 2) of the two log-softmax values in log space (finite where the averaged probability
// underflows).  View a is reduced to its 19 probabilities before view b's accumulators are formed, so only one set of accumulators is live at a time.
// Counters, partials, NaN flag and the byte assembly are those of sssr_tail_predict_kernel.
template <bool TGT, bool CE, bool CM, bool CAL = false, bool CONF = false, bool TEMP = false>
__global__ __launch_bounds__(256, 2) void sssr_tail_predict_flip_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w1,
                                                                         const float* __restrict__ bn_mean, const float* __restrict__ bn_invstd,
                                                                         const float* __restrict__ bn_gamma, const float* __restrict__ bn_beta,
                                                                         const float* __restrict__ w2, const float* __restrict__ bias2,
                                                                         unsigned char* __restrict__ pred, const unsigned char* __restrict__ target,
                                                                         int ignore_index, unsigned long long* __restrict__ counts, double* __restrict__ part,
                                                                         int* __restrict__ nan_flag, int H, int W, long long P, int ntiles,
                                                                         unsigned long long* __restrict__ cm, unsigned long long* __restrict__ cal, int B,
                                                                         float* __restrict__ conf, float beta) {
    static_assert(!CM || TGT, "the confusion matrix needs a target");
    static_assert(!CAL || TGT, "the calibration record needs a target");
    __shared__ unsigned hist[3 * kPC + 2];
    __shared__ unsigned cmh[CM ? kPC * kPC : 1];           // as sssr_tail_predict_kernel
    __shared__ unsigned long long calraw[CAL ? sizeof(CalBins) / 8 : 1];
    CalBins& calb = *reinterpret_cast<CalBins*>(calraw);
    __shared__ double shd[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 15, g = lane >> 4;
    if (TGT) {
        for (int t = tid; t < 3 * kPC + 2; t += 256) hist[t] = 0u;
        if (CM)
            for (int t = tid; t < kPC * kPC; t += 256) cmh[t] = 0u;
        if (CAL) calb.clear(B);
        __syncthreads();
    }
    // Stage-2 fragments stay in registers (two sets: a2 for view a, a2b with tap2 ^ 1 for view b).  The stage-1 fragments do not fit beside them and
    // both views' mid pixels: they are re-read per tile (w1 is 5.8 KB, cache-resident; 25 loads against 250 MFMAs) through an offset the compiler
    // cannot see through, so that it does not hoist them back out of the tile loop.  Padding rows / k-steps read a clamped address and are zeroed.
    float a2[kPT][kPT], a2b[kPT][kPT];
#pragma unroll
    for (int t = 0; t < kPT; ++t)
#pragma unroll
        for (int s = 0; s < kPT; ++s) {
            const int k = 4 * s + g;
            const int tap2 = px >> 2, cls = 4 * t + (px & 3);
            a2[t][s] = (k < kPC && cls < kPC) ? w2[(k * kPC + cls) * 4 + tap2] : 0.f;
            a2b[t][s] = (k < kPC && cls < kPC) ? w2[(k * kPC + cls) * 4 + (tap2 ^ 1)] : 0.f;
        }
    // a1[t][s] = w1[((4 s + g) * 19 + 4 t + (px >> 2)) * 4 + (px & 3)]: one lane offset plus 304 s + 16 t; s = 4 needs g < 3, t = 4 needs (px >> 2) < 3
    const bool k_ok = g < 3, cm_ok = (px >> 2) < 3;
    const int gc = k_ok ? g : 0, qc = cm_ok ? (px >> 2) : 0;
    const int w1off[2][2] = {{(g * kPC + (px >> 2)) * 4 + (px & 3), (gc * kPC + (px >> 2)) * 4 + (px & 3)},
                             {(g * kPC + qc) * 4 + (px & 3), (gc * kPC + qc) * 4 + (px & 3)}};
    auto a1load = [&](float (&a1)[kPT][kPT]) {
        int o[2][2] = {{w1off[0][0], w1off[0][1]}, {w1off[1][0], w1off[1][1]}};
        asm volatile("" : "+v"(o[0][0]), "+v"(o[0][1]), "+v"(o[1][0]), "+v"(o[1][1]));
#pragma unroll
        for (int t = 0; t < kPT; ++t)
#pragma unroll
            for (int s = 0; s < kPT; ++s) {
                const float v = w1[o[t == 4][s == 4] + 304 * s + 16 * t];
                a1[t][s] = ((s < 4 || k_ok) && (t < 4 || cm_ok)) ? v : 0.f;
            }
    };
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
    unsigned tilebits = 0u;                     // CAL / CONF: a NaN in front of the ReLU of either view of the tile's pixel

    // view a: pixel p; view b: the pixel of image N + n at column W - 1 - w, i.e. p + P + (W - 1 - 2 w)
    auto xload = [&](int tile, float (&xa)[kPT], float (&xb)[kPT]) {
        const long long p = (long long)tile * 16 + px;
        const bool in = tile < ntiles && p < P;
        const long long q = in ? p + P + (W - 1 - 2 * ((int)p % W)) : 0;           // p < P <= INT_MAX / 16
#pragma unroll
        for (int s = 0; s < kPT; ++s) {
            const bool ld = in && 4 * s + g < kPC;
            xa[s] = ld ? x[p * ldx + 4 * s + g] : 0.f;
            xb[s] = ld ? x[q * ldx + 4 * s + g] : 0.f;
        }
    };
    // stage 1 of one view: the 2x2 mid pixels after BatchNorm and ReLU
    auto stage1 = [&](const float (&a1)[kPT][kPT], const float (&xv)[kPT], f32x4_p (&mid)[kPT]) {
#pragma unroll
        for (int t = 0; t < kPT; ++t) mid[t] = f32x4_p{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < kPT; ++s)
#pragma unroll
            for (int t = 0; t < kPT; ++t) mid[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t][s], xv[s], mid[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < kPT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = fmaf(mid[t][r], sc[t], sh[t]);
                // the ReLU would hide a NaN of the input from the logits (lanes past the end hold zeros)
                if (CAL || CONF) tilebits = max(tilebits, abs_bits(z));
                else nanbits = max(nanbits, abs_bits(z));
                mid[t][r] = fmaxf(z, 0.f);
            }
    };
    // stage 2 of one view for one mid pixel, reduced to what the ensemble needs: v[c] <- exp(v[c] - max) / sum; returns log_softmax(v)[ts]
    auto softmax_of = [&](const float (&aw)[kPT][kPT], const f32x4_p (&mid)[kPT], int T, int ts, const float (&b0)[4 * kPT], float (&v)[kPC]) {
        f32x4_p acc[kPT];
#pragma unroll
        for (int t = 0; t < kPT; ++t) acc[t] = f32x4_p{b0[4 * t], b0[4 * t + 1], b0[4 * t + 2], b0[4 * t + 3]};
#pragma unroll
        for (int s = 0; s < kPT; ++s)
#pragma unroll
            for (int t = 0; t < kPT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[t][s], mid[s][T], acc[t], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < kPC; ++c) v[c] = TEMP ? temperature_scale(acc[c >> 2][c & 3], beta) : acc[c >> 2][c & 3];
        float m = v[0], vt = v[0];
#pragma unroll
        for (int c = 1; c < kPC; ++c) {
            m = fmaxf(m, v[c]);
            if (CE) vt = (c == ts) ? v[c] : vt;
        }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < kPC; ++c) { v[c] = exp_nonpos(v[c] - m); sum += v[c]; }
        bad |= !(sum == sum);               // any NaN logit poisons the sum (fmaxf alone would skip it)
        const float inv = 1.f / sum;
#pragma unroll
        for (int c = 0; c < kPC; ++c) v[c] *= inv;
        return CE ? (vt - m) - logf(sum) : 0.f;
    };

    const int stride = (int)gridDim.x * 4;
    int tile = (int)blockIdx.x * 4 + wv;
    float xa[kPT], xb[kPT];
    xload(tile, xa, xb);
    for (; tile < ntiles; tile += stride) {
        float a1[kPT][kPT];
        a1load(a1);
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
        f32x4_p mid_a[kPT], mid_b[kPT];
        tilebits = 0u;
        float cf[4] = {0.f, 0.f, 0.f, 0.f};         // CAL / CONF: the confidence of this lane's four output pixels
        stage1(a1, xa, mid_a);
        stage1(a1, xb, mid_b);
        xload(tile + stride, xa, xb);               // the next tile's pixels are in flight while stage 2 of this one is computed
        unsigned packed = 0u;                       // the free bits of its bytes: as in sssr_tail_predict_kernel
        if (CAL || CONF) { nanbits = max(nanbits, tilebits); packed = tilebits > 0x7f800000u ? 0x80u : 0u; }
#pragma unroll
        for (int T = 0; T < 4; ++T) {
            int tg = 0, ts = 0;
            if (TGT) {
                tg = (int)((tw[T >> 1] >> (8 * (2 * (T & 1) + j2))) & 0xffu);
                ts = min(tg == ignore_index ? 0 : tg, kPC - 1);
            }
            float pa[kPC], pb[kPC];
            // One set of accumulators at a time.  Left alone the compiler issues the MFMAs of both views, and of the next output pixel, ahead of the
            // softmax arithmetic and spills.  Empty asm statements keep their order: each set of accumulators starts from bias values that pass through
            // one, behind a statement that needs what the previous set was reduced to (the class byte of the pixel before; view a's pa[]).
            float ba[4 * kPT], bb[4 * kPT];
#pragma unroll
            for (int c = 0; c < 4 * kPT; ++c) ba[c] = bb[c] = bv[c];
            asm volatile("" : "+v"(packed), "+v"(ba[0]), "+v"(ba[1]), "+v"(ba[2]), "+v"(ba[3]), "+v"(ba[4]), "+v"(ba[5]), "+v"(ba[6]), "+v"(ba[7]), "+v"(ba[8]),
                         "+v"(ba[9]), "+v"(ba[10]), "+v"(ba[11]), "+v"(ba[12]), "+v"(ba[13]), "+v"(ba[14]), "+v"(ba[15]), "+v"(ba[16]), "+v"(ba[17]), "+v"(ba[18]),
                         "+v"(ba[19]));
            const float la = softmax_of(a2, mid_a, T, ts, ba, pa);
            asm volatile("" : "+v"(pa[0]), "+v"(pa[1]), "+v"(pa[2]), "+v"(pa[3]), "+v"(pa[4]), "+v"(pa[5]), "+v"(pa[6]), "+v"(pa[7]), "+v"(pa[8]), "+v"(pa[9]),
                         "+v"(pa[10]), "+v"(pa[11]), "+v"(pa[12]), "+v"(pa[13]), "+v"(pa[14]), "+v"(pa[15]), "+v"(pa[16]), "+v"(pa[17]), "+v"(pa[18]));
            asm volatile("" : "+v"(bb[0]), "+v"(bb[1]), "+v"(bb[2]), "+v"(bb[3]), "+v"(bb[4]), "+v"(bb[5]), "+v"(bb[6]), "+v"(bb[7]), "+v"(bb[8]), "+v"(bb[9]),
                         "+v"(bb[10]), "+v"(bb[11]), "+v"(bb[12]), "+v"(bb[13]), "+v"(bb[14]), "+v"(bb[15]), "+v"(bb[16]), "+v"(bb[17]), "+v"(bb[18]), "+v"(bb[19]));
            const float lb = softmax_of(a2b, mid_b, T ^ 1, ts, bb, pb);
            int best = 0;
            float bestv = pa[0] + pb[0];
#pragma unroll
            for (int c = 1; c < kPC; ++c) {
                const float e = pa[c] + pb[c];
                if (e > bestv) { bestv = e; best = c; }                 // first maximum, as seg_metrics_kernel and torch.argmax
            }
            packed |= (unsigned)best << (8 * T);
            if (CAL || CONF) cf[T] = (packed & 0x80u) ? __builtin_nanf("") : confidence_flip(bestv);
            if (TGT) {
                const bool lab_bad = valid && tg != ignore_index && tg >= kPC;
                if (CAL && valid && tg != ignore_index && tg < kPC) packed |= (best == tg ? 0x60u : 0x20u) << (8 * T);
                bad_label |= lab_bad;
                if (counts != nullptr && valid && tg != ignore_index && tg < kPC) {
                    atomicAdd(&hist[best], 1u);
                    atomicAdd(&hist[2 * kPC + tg], 1u);
                    atomicAdd(&hist[3 * kPC + 1], 1u);
                    if (best == tg) { atomicAdd(&hist[kPC + tg], 1u); atomicAdd(&hist[3 * kPC], 1u); }
                }
                if (CM && valid && tg != ignore_index && tg < kPC) atomicAdd(&cmh[tg * kPC + best], 1u);
                if (CE && valid && tg != ignore_index) {
                    // log(0.5 (pa_t + pb_t)) = logaddexp(la, lb) - ln 2, in log space
                    constexpr float LN2 = 0.693147182464599609375f;
                    const float e = fmaxf(la, lb) + log1pf(exp_nonpos(-fabsf(la - lb))) - LN2;
                    ce_loss -= (double)e;
                    ce_cnt += 1.0;
                }
            }
        }
        // row 2 i1 + i2 of the patch, columns 2 j1 + j2: this lane has j2, the lane 16 further on has the other one; lane j2 writes row i1 = j2
        const unsigned other = (unsigned)__shfl_xor((int)packed, 16, 64);
        constexpr unsigned kCls = (CAL || CONF) ? 0x1fu : 0xffu;
        const unsigned b0 = j2 ? (other >> 16) & kCls : packed & kCls;
        const unsigned b1 = j2 ? (packed >> 16) & kCls : other & kCls;
        const unsigned b2 = j2 ? (other >> 24) & kCls : (packed >> 8) & kCls;
        const unsigned b3 = j2 ? (packed >> 24) & kCls : (other >> 8) & kCls;
        if (valid) *reinterpret_cast<unsigned*>(pred + obase + (long long)(2 * j2 + i2) * Wo) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        if (CAL) {
#pragma unroll
            for (int T = 0; T < 4; ++T)
                if ((packed >> (8 * T)) & 0x20u) calb.count(cf[T], ((packed >> (8 * T)) & 0x40u) != 0u, B);
        }
        if (CONF) {
            // the same row: this lane's two columns and the two of the lane 16 away, which needs this lane's other pair
            const float s0 = __shfl_xor(j2 ? cf[0] : cf[2], 16, 64), s1 = __shfl_xor(j2 ? cf[1] : cf[3], 16, 64);
            const f32x4_p row = j2 ? f32x4_p{s0, cf[2], s1, cf[3]} : f32x4_p{cf[0], s0, cf[1], s1};
            if (valid) *reinterpret_cast<f32x4_p*>(conf + obase + (long long)(2 * j2 + i2) * Wo) = row;
        }
    }
    bad |= nanbits > 0x7f800000u;
    if (nan_flag != nullptr && __any(bad) && lane == 0) atomicOr(nan_flag, 1);
    if (TGT && nan_flag != nullptr && __any(bad_label) && lane == 0) atomicOr(nan_flag, 2);
    if (TGT) {
        __syncthreads();
        if (counts != nullptr)
            for (int t = tid; t < 3 * kPC + 2; t += 256)
                if (hist[t]) atomicAdd(&counts[t], (unsigned long long)hist[t]);
        if (CM)
            for (int t = tid; t < kPC * kPC; t += 256)
                if (cmh[t]) atomicAdd(&cm[t], (unsigned long long)cmh[t]);
        if (CAL) calb.flush(cal, B);
    }
    if (CE) {
        if (bad_label) ce_loss = __builtin_nan("");     // as sssr_tail_predict_kernel
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

namespace {

// both entry points: `flip` selects the two-view kernel, whose x holds 2 N images for N class maps
int tail_predict_launch(bool flip, const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                        const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2, uint8_t* pred,
                        const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws, size_t ws_bytes,
                        unsigned long long* cm, unsigned long long* cal, int bins, float* conf, dsrl_stream_t stream, bool temp = false,
                        float beta = 1.f) {
    DSRL_REQUIRE(x && w1 && bn_mean && bn_invstd && bn_gamma && bn_beta && w2 && pred && N > 0 && H > 0 && W > 0, DSRL_E_BADARG,
                 "sssr_tail_predict: null pointer or empty shape");
    DSRL_REQUIRE(dsrl_sssr_tail_predict_supported(N, H, W, Cin, Cmid, Cout), DSRL_E_UNSUPPORTED,
                 "sssr_tail_predict: needs 19 -> 19 -> 19 channels and N*H*W*16 < 2^31 (got %d -> %d -> %d, %d x %d x %d)", Cin, Cmid, Cout, N, H, W);
    DSRL_REQUIRE(ldx >= Cin && ((uintptr_t)x % 4) == 0 && ((uintptr_t)pred % 4) == 0 && ((uintptr_t)target % 4) == 0, DSRL_E_BADARG,
                 "sssr_tail_predict: ldx < Cin, or x / pred / target not 4-byte aligned");
    DSRL_REQUIRE(target || (!counts && !ce_out && !cm && !cal), DSRL_E_BADARG, "sssr_tail_predict: counts / ce_out / cm / cal need a target");
    DSRL_REQUIRE(!cal || (bins >= 1 && bins <= kCalMaxBins && ((uintptr_t)cal % 8) == 0), DSRL_E_BADARG,
                 "sssr_tail_predict: %d calibration bins (1 to %d are possible), or cal not 8-byte aligned", bins, kCalMaxBins);
    DSRL_REQUIRE(((uintptr_t)conf % 16) == 0, DSRL_E_BADARG, "sssr_tail_predict: conf not 16-byte aligned");
    const long long P = (long long)N * H * W;
    const int nb = predict_blocks(P);
    DSRL_REQUIRE(!ce_out || (ws && ws_bytes >= dsrl_sssr_tail_predict_workspace_bytes(N, H, W) && ((uintptr_t)ws % 8) == 0), DSRL_E_WORKSPACE,
                 "sssr_tail_predict: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int ntiles = (int)ceil_div(P, 16);
    double* part = (double*)ws;
    // the _t entry points (temp) launch the TEMP builds; every other entry point launches the builds it always did
#define DSRL_PREDICT_LAUNCH_T(KERNEL, TGT, CE, CM, CAL, CONF, TEMP)                                                                                     \
    hipLaunchKernelGGL((KERNEL<TGT, CE, CM, CAL, CONF, TEMP>), dim3(nb), dim3(256), 0, st, x, ldx, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2,  \
                       pred, target, ignore_index, counts, part, nan_flag, H, W, P, ntiles, cm, cal, bins, conf, beta)
#define DSRL_PREDICT_LAUNCH(KERNEL, TGT, CE, CM, CAL, CONF)                         \
    do {                                                                            \
        if (temp) DSRL_PREDICT_LAUNCH_T(KERNEL, TGT, CE, CM, CAL, CONF, true);      \
        else DSRL_PREDICT_LAUNCH_T(KERNEL, TGT, CE, CM, CAL, CONF, false);          \
    } while (0)
    // without a record and a map: the launches of the entry points that do not know them
#define DSRL_PREDICT_PLAIN(KERNEL)                                                          \
    do {                                                                                    \
        if (!target) DSRL_PREDICT_LAUNCH(KERNEL, false, false, false, false, false);        \
        else if (cm && !ce_out) DSRL_PREDICT_LAUNCH(KERNEL, true, false, true, false, false); \
        else if (cm) DSRL_PREDICT_LAUNCH(KERNEL, true, true, true, false, false);           \
        else if (!ce_out) DSRL_PREDICT_LAUNCH(KERNEL, true, false, false, false, false);    \
        else DSRL_PREDICT_LAUNCH(KERNEL, true, true, false, false, false);                  \
    } while (0)
#define DSRL_PREDICT_EX3(KERNEL, CE, CM)                                                    \
    do {                                                                                    \
        if (cal && conf) DSRL_PREDICT_LAUNCH(KERNEL, true, CE, CM, true, true);             \
        else if (cal) DSRL_PREDICT_LAUNCH(KERNEL, true, CE, CM, true, false);               \
        else DSRL_PREDICT_LAUNCH(KERNEL, true, CE, CM, false, true);                        \
    } while (0)
#define DSRL_PREDICT_EX(KERNEL)                                                             \
    do {                                                                                    \
        if (!target) DSRL_PREDICT_LAUNCH(KERNEL, false, false, false, false, true);         \
        else if (cm && !ce_out) DSRL_PREDICT_EX3(KERNEL, false, true);                      \
        else if (cm) DSRL_PREDICT_EX3(KERNEL, true, true);                                  \
        else if (!ce_out) DSRL_PREDICT_EX3(KERNEL, false, false);                           \
        else DSRL_PREDICT_EX3(KERNEL, true, false);                                         \
    } while (0)
    if (!cal && !conf) {
        if (flip) DSRL_PREDICT_PLAIN(sssr_tail_predict_flip_kernel);
        else DSRL_PREDICT_PLAIN(sssr_tail_predict_kernel);
    } else {
        if (flip) DSRL_PREDICT_EX(sssr_tail_predict_flip_kernel);
        else DSRL_PREDICT_EX(sssr_tail_predict_kernel);
    }
#undef DSRL_PREDICT_EX
#undef DSRL_PREDICT_EX3
#undef DSRL_PREDICT_PLAIN
#undef DSRL_PREDICT_LAUNCH
#undef DSRL_PREDICT_LAUNCH_T
    if (int e = launch_status(flip ? "sssr_tail_predict_flip_kernel" : "sssr_tail_predict_kernel")) return e;
    if (ce_out) {
        hipLaunchKernelGGL(predict_ce_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nb, ce_out);
        return launch_status("predict_ce_finalize_kernel");
    }
    return DSRL_OK;
}

}  // namespace

extern "C" int dsrl_sssr_tail_predict(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                      const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2, uint8_t* pred,
                                      const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws,
                                      size_t ws_bytes, dsrl_stream_t stream) {
    return tail_predict_launch(false, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int dsrl_sssr_tail_predict_flip(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                           const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2,
                                           uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag,
                                           void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    return tail_predict_launch(true, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, nullptr, nullptr, 0, nullptr, stream);
}

// the same launches with the confusion matrix beside the counters: cm[t * Cout + p] += pixels with target t and predicted class p
extern "C" int dsrl_sssr_tail_predict_cm(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                         const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2, uint8_t* pred,
                                         const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws,
                                         size_t ws_bytes, unsigned long long* cm, dsrl_stream_t stream) {
    return tail_predict_launch(false, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, cm, nullptr, 0, nullptr, stream);
}

extern "C" int dsrl_sssr_tail_predict_flip_cm(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                              const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2,
                                              uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag,
                                              void* ws, size_t ws_bytes, unsigned long long* cm, dsrl_stream_t stream) {
    return tail_predict_launch(true, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, cm, nullptr, 0, nullptr, stream);
}

// one entry point per kernel for every optional output: cm, cal (the calibration record, int64 [3 * bins], ADDED) and conf (the confidence map) are
// nullable; with cal and conf null these are the launches above
extern "C" int dsrl_sssr_tail_predict_ex(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                         const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2, uint8_t* pred,
                                         const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws,
                                         size_t ws_bytes, unsigned long long* cm, unsigned long long* cal, int bins, float* conf, dsrl_stream_t stream) {
    return tail_predict_launch(false, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, cm, cal, bins, conf, stream);
}

extern "C" int dsrl_sssr_tail_predict_flip_ex(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                              const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2,
                                              uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag,
                                              void* ws, size_t ws_bytes, unsigned long long* cm, unsigned long long* cal, int bins, float* conf,
                                              dsrl_stream_t stream) {
    return tail_predict_launch(true, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, cm, cal, bins, conf, stream);
}

// temperature scaling applied in the tail (include/dsrl_hip.h, "temperature"): the argument list of _ex plus beta = 1 / T
extern "C" int dsrl_sssr_tail_predict_t(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                        const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2, uint8_t* pred,
                                        const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws,
                                        size_t ws_bytes, unsigned long long* cm, unsigned long long* cal, int bins, float* conf, float beta,
                                        dsrl_stream_t stream) {
    DSRL_TEMPERATURE_BETA(beta, "sssr_tail_predict_t");
    return tail_predict_launch(false, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, cm, cal, bins, conf, stream, true, beta);
}

extern "C" int dsrl_sssr_tail_predict_flip_t(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                             const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2,
                                             uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag,
                                             void* ws, size_t ws_bytes, unsigned long long* cm, unsigned long long* cal, int bins, float* conf, float beta,
                                             dsrl_stream_t stream) {
    DSRL_TEMPERATURE_BETA(beta, "sssr_tail_predict_flip_t");
    return tail_predict_launch(true, x, ldx, N, H, W, Cin, Cmid, Cout, w1, bn_mean, bn_invstd, bn_gamma, bn_beta, w2, bias2, pred, target, ignore_index,
                               counts, ce_out, nan_flag, ws, ws_bytes, cm, cal, bins, conf, stream, true, beta);
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
