// Shared host/device helpers of libdsrl_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include "../../include/dsrl_hip.h"

namespace dsrl {

// ---------------------------------------------------------------- error reporting (thread-local)
void set_error(const char* fmt, ...);
int launch_status(const char* what);

#define DSRL_REQUIRE(cond, code, ...)        \
    do {                                     \
        if (!(cond)) {                       \
            ::dsrl::set_error(__VA_ARGS__);  \
            return (code);                   \
        }                                    \
    } while (0)

// the focal entry points (dsrl_*_f) check their gamma before anything else: finite and >= 0 (a NaN fails the comparison)
#define DSRL_FOCAL_GAMMA(gamma, what) \
    DSRL_REQUIRE((gamma) >= 0.f && (gamma) <= 3.402823466e+38f, DSRL_E_BADARG, what ": gamma = %g is not a finite number >= 0", (double)(gamma))

// the label-smoothing entry points (dsrl_*_s) check their eps before anything else: 0 <= eps <= 1 (a NaN fails the comparison)
#define DSRL_LABEL_SMOOTHING(eps, what) \
    DSRL_REQUIRE((eps) >= 0.f && (eps) <= 1.f, DSRL_E_BADARG, what ": eps = %g is not a number in [0, 1]", (double)(eps))

// Binds the calling thread to the device that owns `stream` (autograd runs backward on its own thread).
int bind_stream_device(hipStream_t s);

// convt_dma.hip: ConvTranspose2d k2 s2 backward staged by LDS-DMA (19 -> 19 channels, W % 128 == 0)
bool convt_bwd_dma_supported(const void* x, const void* dy, int W, int Cin, int Cout);
int convt_bwd_dma_blocks(long long nseg, int cap);
int launch_convt_bwd_dma(const float* x, const float* w, const float* dy, float* dx, float* part, int N, int H, int W, int nblocks, hipStream_t st);

// Which cross entropy a host call asks for: plain, class-weighted, focal, label-smoothed or relaxed.  The dsrl_*_w / _f / _s / _r entry points make
// theirs with weighted() / focal() / smoothed() / relaxed(), and these hold the one normalisation rule: gamma == 0 or eps == 0 IS the weighted form, in every respect
// (kernels, messages).  Everything below the entry points takes this value and decides by kind.
struct CeVariant {
    enum Kind { kPlain, kWeighted, kFocal, kSmoothed, kDice, kLovasz, kRelaxed };
    const float* weights = nullptr;     // the 256-float class-weight table; the plain form has none
    float gamma = 0.f;                  // > 0: kFocal
    float eps = 0.f;                    // > 0: kSmoothed
    Kind kind = kPlain;
    const float* dice = nullptr;        // kDice: the record of dsrl_dice_fwd (dsrl_convt2x2_bwd_ce_d only: the weighted row plus the Dice row)
    static CeVariant weighted(const float* w) { return CeVariant{w, 0.f, 0.f, kWeighted}; }
    static CeVariant focal(const float* w, float gamma) { return gamma == 0.f ? weighted(w) : CeVariant{w, gamma, 0.f, kFocal}; }
    static CeVariant smoothed(const float* w, float eps) { return eps == 0.f ? weighted(w) : CeVariant{w, 0.f, eps, kSmoothed}; }
    const float* lovasz = nullptr;      // kLovasz: the record of dsrl_lovasz_fwd (dsrl_convt2x2_bwd_ce_l only: the weighted row plus the Lovasz row)
    int bins = 0;                       // kLovasz: K, the levels of that record
    static CeVariant diced(const float* w, const float* record) { return CeVariant{w, 0.f, 0.f, kDice, record}; }
    static CeVariant lovasz_of(const float* w, const float* record, int bins) { return CeVariant{w, 0.f, 0.f, kLovasz, nullptr, record, bins}; }
    const uint32_t* mask = nullptr;     // kRelaxed: one class-set word per pixel (dsrl_relax_mask, or any words: the consumers clean them with relax_set)
    static CeVariant relaxed(const float* w, const uint32_t* mask) {
        CeVariant v{w, 0.f, 0.f, kRelaxed};
        v.mask = mask;
        return v;
    }
    bool plain() const { return kind == kPlain; }
    int max_classes() const { return kind == kRelaxed ? 32 : 60; }          // a class set is one 32-bit word
    bool table_ok() const { return plain() || (weights != nullptr && (kind != kRelaxed || mask != nullptr)); }   // part of every entry point's argument check
    const char* suffix() const {        // of the entry point, for its messages
        return plain() ? "" : kind == kWeighted ? "_w" : kind == kFocal ? "_f" : kind == kSmoothed ? "_s" : kind == kDice ? "_d" : kind == kLovasz ? "_l" : "_r";
    }
};
// losses.hip, for the ConvTranspose forms in spatial.hip: the pre-pass of every kind but plain (D = sum n_c w_c into d_out, through `ws` of
// ce_weight_sum_bytes()) and the finalize (plain: loss / pixel count; the others: loss / D, D read from loss_out[1])
int launch_ce_weight_sum(const unsigned char* target, long long P, int C, int ignore_index, const float* weights, float* d_out, void* ws, hipStream_t st);
size_t ce_weight_sum_bytes();
int launch_ce_finalize(CeVariant::Kind kind, const double* part, int nb, float* loss_out, hipStream_t st);

// `count`: the pixel count of the plain form, D of the others
int launch_convt_bwd_dma_ce(const float* x, const float* w, const float* logits, float* dx, float* part, int N, int H, int W, int nblocks,
                            const unsigned char* target, int ignore_index, const float* count, const float* ft_g, const float* ft_w, int ft_s,
                            const CeVariant& v, hipStream_t st);

// The one way the library reads a DSRL_* environment switch (table: DESIGN.md §9).  Read at every call, never cached: tests change switches
// between calls inside one process.  knob_str: for the one switch whose value is a path (DSRL_PROF_DUMP).
static inline const char* knob_str(const char* name) { return getenv(name); }
static inline int knob(const char* name, int dflt) { const char* v = knob_str(name); return v ? atoi(v) : dflt; }

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

constexpr int kWave = 64;
constexpr int kNumCU = 256;     // MI355X
constexpr int kNumXCD = 8;

// ---------------------------------------------------------------- Philox4x32-10 (same as oracle/philox.py)
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// uniform in [0,1) for element e: word (e&3) of philox(counter = e>>2, stream), u = (word>>8) * 2^-24
__device__ inline float philox_uniform(uint64_t e, uint64_t seed, uint32_t stream) {
    uint32_t r[4];
    const uint64_t q = e >> 2;
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return (float)(r[e & 3] >> 8) * 5.9604644775390625e-08f;
}

// ---------------------------------------------------------------- exp(x) for x <= 0 (softmax terms exp(v - max))
// v_exp_f32 on t = fl(x * log2 e) with the rounding error of that product and the low part of log2 e put back to first order:
// exp(x) = 2^t * 2^r, r = (x * L2E_HI - t) + x * L2E_LO exactly (one fma each), 2^r = 1 + r ln 2 + O(r^2), |r| < 2^-23 |t|.  Six instructions instead
// of libm's ~20 (range reduction + polynomial + overflow / denormal cases, none of which a non-positive argument needs); within 2 ulp of expf for
// x in [-87, 0], 0 below (the hardware flushes the denormal result).  ce_fused_kernel and the ConvTranspose backward that forms the CE gradient
// itself (convt_dma.hip) both use it: their results are bit-identical.
// t = -inf (x = -inf: a -inf logit, or v - m overflowing; or x below -2.3e38, where the product overflows) would make r = -inf + inf = NaN:
// r = 0 there, and the result is 2^-inf = 0 as for expf.  A NaN x fails the comparison too and stays NaN through e0.
__device__ __forceinline__ float exp_nonpos(float x) {
    constexpr float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500011e-08f, LN2 = 0.693147182464599609375f;
    const float t = x * L2E_HI;
    const float r = t > -INFINITY ? fmaf(x, L2E_LO, fmaf(x, L2E_HI, -t)) : 0.f;
    const float e0 = __builtin_amdgcn_exp2f(t);
    return fmaf(e0, r * LN2, e0);
}

// ---------------------------------------------------------------- focal cross entropy, the arithmetic of one live pixel
// term_i = w[t] q^g nll, d loss / d v_c = (w[t] / D) mod (softmax_c - [c == t]), mod = q^(g-1) (q + g p nll), with q = 1 - p_t.  The caller passes
//     m = max_c v_c, vt = v_t, et = exp_nonpos(vt - m), s = sum_c e_c and so = sum_{c != t} e_c (both with c ascending, e_t taken as 0 in `so`)
// and gets fl = q^g nll and mod; the weight, 1 / D and the double accumulation stay with the kernel.  Every focal kernel (losses.hip, spatial.hip,
// convt_dma.hip) goes through this one function, so that the fused and the unfused paths round alike (the library is built with -ffp-contract=off).
//   q = so / s, never 1 - p: a confident pixel would lose all of q, and q^g with it, to cancellation.
//   nll = (m - vt) + log s, not m + log s - vt: at logits near 1e4 the latter costs an ulp(1e4), which the modulator does not tolerate.
//   q^g = 2^(g log2 q) on v_log_f32 / v_exp_f32 (1 ulp each): the error of the exponent, g |log2 q| 2^-23 relative, is weighted by q^g |log q|
//   <= 1 / (e g) in the value and in the gradient alike, i.e. below an ulp of their bounds.
//   Limits: q == 0 -> fl = 0, mod = 0 for every g > 0 (also a q below the smallest normal number, which v_log_f32 does not read: q^g underflows
//   there for g >= 1 and is below 1.1e-19 for g = 1/2); p == 0 -> p nll taken as 0, so that mod = 1 at q = 1 even where nll overflows.
__device__ __forceinline__ void focal_pixel(float m, float vt, float et, float s, float so, float gamma, float& fl, float& mod) {
    const float d = m - vt;
    const float nll = d + logf(s);
    const float q = so / s;
    const float p = et / s;
    const float l2 = __builtin_amdgcn_logf(q);                              // log2 q <= 0
    const float qg = __builtin_amdgcn_exp2f(gamma * l2);                    // q^g
    const float qg1 = __builtin_amdgcn_exp2f((gamma - 1.f) * l2);           // q^(g-1)
    const float pn = p == 0.f ? 0.f : p * nll;
    const bool zero = q < 1.17549435e-38f;                                  // (a NaN q compares false and goes through)
    fl = zero ? 0.f : qg * nll;
    mod = zero ? 0.f : qg1 * (q + gamma * pn);
}

// ---------------------------------------------------------------- label-smoothed cross entropy, the arithmetic of one live pixel
// With nl_c = (m - v_c) + log s, W = sum_{c < C} w_c and D = sum_i w[t_i]:
//     term_i = (1 - eps) w[t] nl_t + (eps / C) sum_{c < C, w_c > 0} w_c nl_c
//     d loss / d v_c = ((1 - eps) w[t] (p_c - [c == t]) + (eps / C) (p_c W - w_c)) / D = e_c inv - sub_c,
//     inv = (((1 - eps) w[t] + (eps / C) W) scale) / s,   sub_c = (([c == t] ? (1 - eps) w[t] : 0) + (eps / C) w_c) scale,   scale = 1 / D
// sub_c of a class that is not the target is ((eps / C) w_c) scale (0 + x is x) and the same for every pixel: smooth_sub, which the gradient kernels
// keep as a C-entry table in LDS, made once per block; the target's own sub_t = ((1 - eps) w[t] + (eps / C) w[t]) scale comes from smooth_pixel.
// The caller passes the pixel's C raw logits `v`, the weights `w` (the table: w[t] is read at the label byte, so a label >= C has weight 0),
// m = max_c v_c, s = sum_c exp_nonpos(v_c - m) (c ascending) and W (summed once per block, c ascending); it gets the value term (VAL builds only:
// a backward needs no log), sub_t and inv.  smooth_grad is one element of the gradient row.  Each nl_c is fp32; the products with the
// weights and their sum over the classes are double, as the accumulation over pixels is in every CE kernel (w_c nl_c of a logit near -3e38 times a
// weight above 1 leaves fp32 while the loss does not).  The accumulation over pixels and 1 / D stay with the kernel.  Every smoothing kernel
// (losses.hip, spatial.hip, convt_dma.hip) goes through these functions, so that the fused and the unfused paths round alike (the library is
// built with -ffp-contract=off).
//   nl = (m - v) + log s, never m + log s - v: m - v is exact or rounds at its own size, the other order rounds at ulp(m) in every one of C terms.
//   The sum over the classes runs in ascending c.  A class of weight 0 adds nothing to it, even where nl_c is +inf (torch forms 0 * inf = NaN there);
//   with a positive weight such a class makes the value +inf, as it is.  The target's own term is the plain product, as in the weighted kernels.
template <bool VAL>
__device__ __forceinline__ void smooth_pixel(const float* v, const float* w, int C, int tg, float m, float s, float eps, float Wsum, float scale,
                                             double& val, float& sub_t, float& inv) {
    const float epsC = eps / (float)C;
    const float omw = (1.f - eps) * w[tg];
    inv = ((omw + epsC * Wsum) * scale) / s;
    sub_t = (omw + epsC * w[tg]) * scale;
    if (VAL) {
        const float ls = logf(s);
        double sm = 0.0;
        for (int c = 0; c < C; ++c) { const float wc = w[c]; const float nl = (m - v[c]) + ls; sm += wc > 0.f ? (double)wc * (double)nl : 0.0; }
        const float nlt = (m - v[min(tg, C - 1)]) + ls;
        val = (double)omw * (double)nlt + (double)epsC * sm;
    } else {
        val = 0.0;
    }
}
__device__ __forceinline__ float smooth_sub(float eps, int C, float wc, float scale) { return ((eps / (float)C) * wc) * scale; }
__device__ __forceinline__ float smooth_grad(float e, float inv, bool hit, float sub_t, float sub_c) { return e * inv - (hit ? sub_t : sub_c); }

// ---------------------------------------------------------------- soft Dice loss term (dice.hip), the gradient row of one pixel
// The record dsrl_dice_fwd leaves in device memory: kDiceRecordFloats floats {lambda L_dice, |K|, a[0..C), b[0..C), zeros}.  With the per-class
// coefficients a_c, b_c of the batch (zero for a class without a pixel),
//     d(lambda L_dice) / d v_k = live p_k (g_k - sum_j p_j g_j),   g_j = b_j + a_j [j == t],   p_j = e_j (1 / s)
// The caller passes its softmax terms e_c = exp_nonpos(v_c - m) and s = sum_c e_c (c ascending) - what every CE kernel has in hand - the label and
// the two tables; live = the label is neither ignore_index nor >= C (such a pixel takes no part in Dice: a row of zeros).  dice_pixel forms 1 / s,
// a_t and the sum over the classes in ascending j; dice_grad is one element of the row.  CT > 0: the class count at compile time (e[] in registers,
// the loop unrolled); CT == 0: `C` at run time.  The unfused kernel (dice.hip) and the ConvTranspose backward that forms the row itself
// (convt_dma.hip) both go through these two functions, so that they round alike (the library is built with -ffp-contract=off).
constexpr int kDiceRecordFloats = 128, kDiceMaxC = 60;
template <int CT>
__device__ __forceinline__ void dice_pixel(const float* e, int C, float s, int tg, bool live, const float* a, const float* b, float& inv_s, float& a_t,
                                           float& dot) {
    const int n = CT > 0 ? CT : C;
    inv_s = 1.f / s;
    a_t = live ? a[tg] : 0.f;
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < n; ++c) d += (e[c] * inv_s) * (b[c] + (c == tg ? a_t : 0.f));
    dot = d;
}
__device__ __forceinline__ float dice_grad(float e, float inv_s, float b_c, bool hit, float a_t, float dot, bool live) {
    return live ? (e * inv_s) * ((b_c + (hit ? a_t : 0.f)) - dot) : 0.f;
}

// ---------------------------------------------------------------- Lovasz-Softmax loss term (lovasz.hip), the gradient row of one pixel
// The quantised form: the error err_c = |[c == t] - p_c| of a live pixel falls in level b = lovasz_bin(err_c, K) of K, and the loss and a valid
// subgradient follow from the integer histograms of the levels (dsrl_hip.h).  The record dsrl_lovasz_fwd leaves in device memory:
//     {lambda L, |Present|, 0, 0, gf[C][K], gb[C][K]}      gf = -(lambda / |Present|) wf,  gb = +(lambda / |Present|) wb,  zeros for an absent class
//     d(lambda L) / d v_k = live p_k (g_k - sum_j p_j g_j),   g_j = (j == t ? gf : gb)[j][b_j],   p_j = e_j (1 / s)          (j ascending)
// lovasz_bin is the ONE function that turns an error into a level: the histogram pass and every gradient path call it on the same fp32 p, so a
// pixel looks up the level it was counted in.  It returns an index in [0, K) for ANY bit pattern: x = err K; fmaxf(x, 0) is 0 for a NaN (maxnum
// returns the operand that is a number) and for every negative value or -inf; fminf(., K - 1) bounds +inf and everything above; the conversion of
// a number in [0, K - 1] is exact arithmetic; and the final & (K - 1) (K is a power of two) holds the range whatever the three steps before it gave.
// lovasz_coef is g_j of one class (one gather from the record, global memory / L2); lovasz_pixel forms 1 / s and the sum over the classes in
// ascending j, and with CT > 0 (class count at compile time, e[] in registers) keeps the C coefficients in g[] so that the row needs no second
// gather; CT == 0: `C` at run time, g unused, the caller gathers again through lovasz_coef.  A pixel that is not live reads nothing.  The unfused
// kernel (lovasz.hip) and the ConvTranspose backward (convt_dma.hip) both go through these functions, so that they round alike.
constexpr int kLovaszHeadFloats = 4, kLovaszMaxC = 60, kLovaszMinBins = 16, kLovaszMaxBins = 4096;
__host__ __device__ __forceinline__ int lovasz_bin(float err, int K) {
    const float x = fminf(fmaxf(err * (float)K, 0.f), (float)(K - 1));
    return (int)x & (K - 1);
}
__device__ __forceinline__ float lovasz_err(float p, bool hit) { return hit ? fabsf(1.f - p) : fabsf(p); }
__device__ __forceinline__ float lovasz_coef(float p, bool hit, int c, const float* __restrict__ gf, const float* __restrict__ gb, int K) {
    return (hit ? gf : gb)[c * K + lovasz_bin(lovasz_err(p, hit), K)];
}
template <int CT>
__device__ __forceinline__ void lovasz_pixel(const float* e, int C, float s, int tg, bool live, const float* __restrict__ gf, const float* __restrict__ gb,
                                             int K, float& inv_s, float* g, float& dot) {
    const int n = CT > 0 ? CT : C;
    inv_s = 1.f / s;
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < n; ++c) {
        const float p = e[c] * inv_s;
        const float gc = live ? lovasz_coef(p, c == tg, c, gf, gb, K) : 0.f;
        if (CT > 0) g[c] = gc;
        d += p * gc;
    }
    dot = d;
}
__device__ __forceinline__ float lovasz_grad(float e, float inv_s, float g_c, float dot, bool live) { return live ? (e * inv_s) * (g_c - dot) : 0.f; }

// ---------------------------------------------------------------- boundary label relaxation (relax.hip), the arithmetic of one live pixel
// The loss of a pixel asks for the probability of a SET of classes S (the classes of the labels around it, dsrl_relax_mask) instead of one label:
//     term = w[t] ((m + log s) - (m_S + log z)) = -w[t] log sum_{c in S} p_c,      d loss / d v_c = (w[t] / D) (e_c / s - g_c / z)
//     m_S = max_{c in S} v_c,   g_c = [c in S] exp_nonpos(v_c - m_S),   z = sum_{c in S} g_c (c ascending)
// The set softmax is taken relative to its OWN maximum: a set whose logits all lie 87 below the largest one has e_c = 0 for every member, and a
// -log(sum_S e_c / s) on the shared terms would be infinite where plain CE is about 100.
// relax_set is the one place a mask word becomes a set: bits of classes that do not exist are dropped and the pixel's own label is added, so no
// caller-supplied word can drop the label or name a class >= C (a label >= C has no bit: its weight is 0 and the entry point poisons the loss).
// relax_pixel gets the pixel's C raw logits `v`, m = max_c v_c, s = sum_c exp_nonpos(v_c - m) (c ascending) and sc = w[t] (1 / D) and gives m_S,
// inv = sc / s, invz = sc / z and (VAL builds) the fp32 term without its weight; relax_grad is one element of the row, e inv - g invz, with g
// recomputed from the logit (the second exp_nonpos of a logit has the bits of the first).  A member equal to m_S takes the argument 0 whatever its
// value, so that a set whose maximum is -inf has g = 1 there instead of exp(-inf + inf).  For S = {t}: m_S = v_t, g_t = exp_nonpos(0) = 1, z = 1,
// log z = 0, invz = sc: the term is (m + log s) - v_t and the row e_c (sc / s) - [c == t] sc - the operations and the bits of the weighted form.
// CT > 0: the class count at compile time (loops unrolled); CT == 0: `C` at run time.  Every relaxed kernel (losses.hip, spatial.hip, convt_dma.hip)
// goes through these functions, so that the fused and the unfused paths round alike (the library is built with -ffp-contract=off).
constexpr int kRelaxMaxC = 32, kRelaxMaxRadius = 4;
__host__ __device__ __forceinline__ unsigned relax_set(unsigned word, int tg, int C) {
    const unsigned all = C >= 32 ? 0xffffffffu : (1u << C) - 1u;
    return (word & all) | ((tg >= 0 && tg < C) ? 1u << tg : 0u);
}
__device__ __forceinline__ float relax_arg(float vc, float mS) { return vc == mS ? 0.f : vc - mS; }
template <int CT, bool VAL>
__device__ __forceinline__ void relax_pixel(const float* v, int C, unsigned S, float m, float s, float sc, float& mS, float& inv, float& invz, float& term) {
    const int n = CT > 0 ? CT : C;
    float ms = -INFINITY;
#pragma unroll
    for (int c = 0; c < n; ++c) ms = ((S >> c) & 1u) ? fmaxf(ms, v[c]) : ms;
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < n; ++c) z += ((S >> c) & 1u) ? exp_nonpos(relax_arg(v[c], ms)) : 0.f;
    mS = ms;
    inv = sc / s;
    invz = sc / z;
    term = VAL ? (m + logf(s)) - (ms + logf(z)) : 0.f;
}
__device__ __forceinline__ float relax_grad(float e, float inv, bool in_set, float vc, float mS, float invz) {
    return e * inv - (in_set ? exp_nonpos(relax_arg(vc, mS)) * invz : 0.f);
}

// ---------------------------------------------------------------- exponential moving average of the weights (ema.hip)
// The EMA record in device memory (16 bytes, 16-byte aligned).  omd = 1 - d_t of the update ABOUT to run; dsrl_ema_advance rewrites it once per step.
struct EmaRecord {
    float omd;          // 1 - d_t: all that the element kernels read
    float decay_max;    // the configured decay, d_t's limit
    uint32_t updates;   // averages formed so far (t)
    uint32_t warmup;    // non-zero: d_t = min(decay_max, (1 + t) / (10 + t))
};
// e <- d e + (1 - d) p as e + (1 - d) (p - e): one difference and one fma, so e == p stays e for every d, and the error per step is an ulp of e.
// Every EMA kernel - fused into an SGD launch or not - goes through this one function, so that the fused and the unfused paths round alike.
__device__ __forceinline__ float ema_elem(float e, float p_new, float omd) { return fmaf(omd, p_new - e, e); }

// ---------------------------------------------------------------- gradient-norm clipping (gradclip.hip)
// The clip record in device memory (64 bytes, 16-byte aligned).  dsrl_grad_clip_finish reads max_norm when it runs - a new value needs no re-capture -
// and writes everything else: the figures of the step it finished, then the running fields (since the record was made or last reset by the host).
struct GradClipRecord {
    double sumsq;       // S of the last step: the sum of squares of the gradient arena, before grad_scale
    double norm_sum;    // running: sum of the finite norms
    float norm;         // last step: grad_scale * sqrt(S), the norm of the rank-averaged gradient
    float coef;         // last step: min(1, max_norm / (norm + 1e-6)); NaN for a NaN norm
    float max_norm;     // the threshold; +inf monitors only
    float norm_max;     // running: largest finite norm
    uint32_t steps;     // running: finishes
    uint32_t clipped;   // running: finishes with a finite norm and coef < 1
    uint32_t nonfinite; // running: finishes with a NaN or infinite norm (left out of norm_sum and norm_max)
    uint32_t pad[5];
};
static_assert(sizeof(GradClipRecord) == 64, "GradClipRecord is 64 bytes");

// ---------------------------------------------------------------- AdamW (adamw.hip)
// The AdamW record in device memory (64 bytes, 16-byte aligned).  The host writes the configuration once (the floats as the kernels use them, 1 - beta
// formed from the DOUBLE beta as torch forms it: 1 - 0.999f is 4.7e-5 off 0.001; the doubles for the bias corrections, which amplify a beta error by
// t); dsrl_adamw_advance / dsrl_adamw_set_step write t and the two factors of step t, in double from t, and nothing else ever does.
struct AdamwRecord {
    float beta1, beta2;     // as float: beta2 multiplies v
    float eps;
    float ss_factor;        // 1 / (1 - beta1^t): the step size is lr times this
    float isq;              // 1 / sqrt(1 - beta2^t)
    float omb1, omb2;       // (float)(1 - beta1), (float)(1 - beta2) of the double betas
    uint32_t pad0;
    long long t;            // optimiser passes begun: the launches of a pass read the factors of THIS t (0 in a fresh record: nothing may launch yet)
    double beta1_d, beta2_d;
    uint32_t pad1[2];
};
static_assert(sizeof(AdamwRecord) == 64, "AdamwRecord is 64 bytes");
// what every element of a launch shares, formed the same way by every entry point
struct AdamwCoef { float dk, b1, w1, b2, w2, eps, ss, isq, gscale; };
__device__ __forceinline__ AdamwCoef adamw_coef(float lr, float wd, float gscale, const AdamwRecord* __restrict__ r) {
    AdamwCoef c;
    c.dk = 1.f - lr * wd;               // decoupled decay, torch's p.mul_(1 - lr * wd)
    c.b1 = r->beta1; c.w1 = r->omb1; c.b2 = r->beta2; c.w2 = r->omb2; c.eps = r->eps;
    c.ss = lr * r->ss_factor; c.isq = r->isq; c.gscale = gscale;
    return c;
}
// One element of torch.optim.AdamW (one group, no amsgrad, no maximize) on gh = g * grad_scale - scaled BEFORE the moments: eps makes the update depend
// on the gradient's scale.  m as torch's lerp - from m for a weight 1 - beta1 below 1/2, from gh above, so that beta1 = 0 gives gh itself; the choice is
// uniform over the launch -, v and both p updates with one rounding each (explicit fma: the library is built with -ffp-contract=off); square root and
// division correctly rounded: sqrtf, which hipcc lowers to v_sqrt_f32 plus the two-fma +-1 ulp correction (NOT __fsqrt_rn - without
// OCML_BASIC_ROUNDED_OPERATIONS the header maps it to the bare native instruction), and __fdiv_rn, the full div_scale / div_fmas / div_fixup sequence.  Every AdamW kernel goes through this one function, so that all forms round alike.
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamwCoef& c) {
    const float gh = g * c.gscale;
    p = p * c.dk;
    m = c.w1 < 0.5f ? fmaf(c.w1, gh - m, m) : fmaf(-c.b1, gh - m, gh);
    v = fmaf(c.b2, v, (c.w2 * gh) * gh);
    p = fmaf(-c.ss, __fdiv_rn(m, fmaf(sqrtf(v), c.isq, c.eps)), p);
}

// ---------------------------------------------------------------- calibration record and confidence (calibration.hip)
// Confidence of a pixel: the probability of the class the kernel reports (first maximum), fp32, from values the producer already has:
//     one softmax (dsrl_calibration_from_logits, the single-view tail):  1 / s, s = sum_c exp_nonpos(v_c - m) with c ascending, m the fmaxf chain from v_0
//                                                                        (the max term is exp(0) = 1, so s >= 1 and the confidence <= 1)
//     two views (the flip tail):          half the winning entry of e_a / s_a + e_b / s_b, as the kernel formed it for the arg-max
//     V views (the multi-scale finish):   min(1, winning sum / V)
// A NaN stays a NaN in all three (the comparison in confidence_views fails for it).  Bin of a confidence among B equal-width bins: one fp32 multiply
// (the library is built with -ffp-contract=off), conf = 1 goes to the last bin.  The record is int64 [3 B] = [n_b | hit_b | q_b]: counted pixels,
// those with pred == target, and the sum of rintf(conf 2^24) as an integer - no float is ever added, so a record does not depend on the order of the
// additions.  A NaN confidence is counted nowhere.  Per block the three rows are LDS integers (CalBins; q is 64-bit there already: 256 pixels of
// confidence 1 are 2^32), flushed as one 64-bit atomic per non-zero entry.  Every producer goes through these functions, so that they bin alike.
constexpr int kCalMaxBins = 64;
constexpr float kCalQScale = 16777216.f;        // 2^24
template <int CT>
__device__ __forceinline__ float softmax_denominator(const float* v, int C) {
    const int n = CT > 0 ? CT : C;
    float m = v[0];
#pragma unroll
    for (int c = 1; c < n; ++c) m = fmaxf(m, v[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < n; ++c) s += exp_nonpos(v[c] - m);
    return s;
}
__device__ __forceinline__ float confidence_pixel(float s) { return 1.f / s; }
__device__ __forceinline__ float confidence_flip(float best_sum) { return 0.5f * best_sum; }
__device__ __forceinline__ float confidence_views(float best_sum, float views) {
    const float q = best_sum / views;
    return q > 1.f ? 1.f : q;
}
__device__ __forceinline__ int calibration_bin(float conf, int B) { return min(B - 1, (int)(conf * (float)B)); }
struct CalBins {
    unsigned n[kCalMaxBins], hit[kCalMaxBins];
    unsigned long long q[kCalMaxBins];
    // every thread of the block; the caller synchronises before the first count
    __device__ __forceinline__ void clear(int B) {
        for (int b = threadIdx.x; b < B; b += blockDim.x) { n[b] = 0u; hit[b] = 0u; q[b] = 0ull; }
    }
    __device__ __forceinline__ void count(float conf, bool is_hit, int B) {
        if (!(conf >= 0.f && conf <= 1.f)) return;      // a NaN fails the comparison (every producer's confidence is in [0, 1] otherwise)
        const int b = calibration_bin(conf, B);
        atomicAdd(&n[b], 1u);
        if (is_hit) atomicAdd(&hit[b], 1u);
        atomicAdd(&q[b], (unsigned long long)rintf(conf * kCalQScale));
    }
    // every thread of the block, behind a __syncthreads() that follows the last count
    __device__ __forceinline__ void flush(unsigned long long* __restrict__ rec, int B) {
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
            if (n[b]) atomicAdd(&rec[b], (unsigned long long)n[b]);
            if (hit[b]) atomicAdd(&rec[B + b], (unsigned long long)hit[b]);
            if (q[b]) atomicAdd(&rec[2 * B + b], q[b]);
        }
    }
};

// ---------------------------------------------------------------- temperature scaling (temperature.hip)
// The NLL of softmax(beta v) at the label t of one live pixel, with its first and second derivative in beta = 1 / T, fp32, c ascending.  The caller
// passes d_c = v_c - m (m the fmaxf chain from v_0, so d_c <= 0) and dt = d_t:
//     e_c = exp_nonpos(beta d_c), s = sum e_c, a = sum e_c d_c, q = sum (e_c d_c) d_c
//     L = log_ge1(s) - beta dt,  mu = a / s,  G = mu - dt = dL/dbeta,  H = q / s - mu mu = d2L/dbeta2 (the variance of d under softmax(beta v), >= 0)
// Every producer of a temperature record goes through this function, so that they round alike (no contraction: -ffp-contract=off).
// The logarithm is log_ge1, not logf: the device's logf (v_log_f32 underneath) came out 3.1e-8 relative LOW on average when measured alone (sum of
// logf(m), m = 1..19, over 30720 pixels against float64; numpy's float32 log: +8e-9), and a sum over 10^5 - 10^6 pixels keeps such a bias where it
// averages rounding out: the L entries were 1.9e-9 - 2.3e-8 off against 2e-10 - 1.6e-9 for a float32 restatement.  log_ge1 is the float32 polynomial
// of the Cephes logf (s = m 2^e with m in [sqrt(1/2), sqrt(2)), degree 9 in m - 1, ln 2 in two parts): about 25 instructions, within 8.1e-8 relative
// for s >= 1.1 and 4.1e-9 absolute below, mean error 8e-10 (2.4 M samples of [1, 19] against float64).  s >= 1 here: the maximum's term is exp(0).
__device__ __forceinline__ float log_ge1(float s) {
    int ei;
    float m = frexpf(s, &ei);                   // s = m 2^ei, m in [0.5, 1)
    float e = (float)ei;
    const bool lo = m < 0.707106769084930419921875f;
    e = lo ? e - 1.f : e;
    const float x = lo ? (m + m) - 1.f : m - 1.f;
    const float z = x * x;
    float y = 7.0376836292e-2f;
    y = y * x + -1.1514610310e-1f;
    y = y * x + 1.1676998740e-1f;
    y = y * x + -1.2420140846e-1f;
    y = y * x + 1.4249322787e-1f;
    y = y * x + -1.6668057665e-1f;
    y = y * x + 2.0000714765e-1f;
    y = y * x + -2.4999993993e-1f;
    y = y * x + 3.3333331174e-1f;
    y = y * x * z;
    y = y + -2.12194440e-4f * e;
    y = y + -0.5f * z;
    return (x + y) + 0.693359375f * e;
}
__device__ __forceinline__ void temperature_terms(const float* d, int C, float dt, float beta, float& L, float& G, float& H) {
    float s = 0.f, a = 0.f, q = 0.f;
    for (int c = 0; c < C; ++c) {
        const float dc = d[c];
        const float e = exp_nonpos(beta * dc);
        const float ed = e * dc;
        s += e;
        a += ed;
        q += ed * dc;
    }
    const float mu = a / s;
    L = log_ge1(s) - beta * dt;
    G = mu - dt;
    H = q / s - mu * mu;
}
// Applying a temperature in a producer: behind its arg-max every logit becomes v_c * beta (one fp32 multiply), then the softmax arithmetic that is
// already there runs on the result.  A positive beta is monotone under rounding, so the first maximum - the class map - does not move.
__device__ __forceinline__ float temperature_scale(float v, float beta) { return v * beta; }
// beta as every entry point that applies one wants it: a finite number > 0 (a NaN fails the comparison)
#define DSRL_TEMPERATURE_BETA(beta, what) \
    DSRL_REQUIRE((beta) > 0.f && (beta) <= 3.402823466e+38f, DSRL_E_BADARG, what ": beta = %g is not a finite number > 0", (double)(beta))

// ---------------------------------------------------------------- wave / block reductions
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------- operand magnitudes (f16x3 conv arithmetic, dsrl_amax)
// A kernel that writes a tensor a conv will read can leave max |x| of what it wrote (as a bit pattern; NaN patterns sort above every number)
// in a device record: per thread a running maximum over its stores, then amax_publish - one fire-and-forget atomic per block.
// A record ("amax record", kAmaxWords uint32) holds kAmaxShards partial maxima, one per 64-byte line: the ~1000 blocks of a streaming
// kernel finish together, and their atomics on ONE word would be served one after the other (~12 ns each: measured +9 us on a 7 us
// BatchNorm launch); spread over 16 lines they cost nothing visible.  The reader takes the maximum of the shards (amax_read).
// Every thread of the block must reach amax_publish (it synchronises); `out` may be null.
constexpr int kAmaxShards = 16, kAmaxShardStride = 16, kAmaxWords = kAmaxShards * kAmaxShardStride;     // 1 KiB per record
__device__ inline unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ inline unsigned* amax_shard(unsigned* rec) { return rec + (((blockIdx.x + 5u * blockIdx.y) & (kAmaxShards - 1)) * kAmaxShardStride); }
// maximum over the shards of a record, wave-uniform (every lane of the wave must be active).  Two halves so that a kernel can request the
// shards at its very start (amax_fetch: one load per lane, no wait) and consume them where the value is first needed (amax_reduce): the conv
// kernels used to sit through two dependent load latencies - one per operand record - before they computed a single address.
__device__ inline unsigned amax_fetch(const unsigned* rec) {
    const int lane = threadIdx.x & 63;
    return lane < kAmaxShards ? rec[lane * kAmaxShardStride] : 0u;
}
__device__ inline unsigned amax_reduce(unsigned m) {
#pragma unroll
    for (int o = kAmaxShards / 2; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    return __builtin_amdgcn_readfirstlane(m);
}
__device__ inline unsigned amax_read(const unsigned* rec) { return amax_reduce(amax_fetch(rec)); }
__device__ inline unsigned abs_bits4(unsigned m, float a, float b, float c, float d) {
    return max(max(m, abs_bits(a)), max(max(abs_bits(b), abs_bits(c)), abs_bits(d)));
}
__device__ inline void amax_publish(unsigned m, unsigned* out) {
    if (out == nullptr) return;
    __shared__ unsigned sm_amax;
    if (threadIdx.x == 0) sm_amax = 0u;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&sm_amax, m);
    __syncthreads();
    if (threadIdx.x == 0 && sm_amax) __hip_atomic_fetch_max(amax_shard(out), sm_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the same measurement as a launch of its own (conv_igemm.hip)
int launch_amax(const float* x, int ld, long long P, int C, unsigned* out, hipStream_t st);
// Zero-fill as a KERNEL launch (conv_igemm.hip), not hipMemsetAsync.  Round 3: with the 2 KiB amax scratch of the stem's weight gradient zeroed by a
// captured memset node, ~40 % of the replays of the two-graph step produced a NaN there, and replacing that one call by a kernel made it disappear.
// Round 4 dumped the captured graphs of a build with the memsets restored (profiles/round4_graph_memset_edges.txt): both graphs are pure chains and every memset node has its edge to the kernel that consumes the zeroed
// words - the capture did NOT drop a dependency.  Why the replay misbehaved is therefore not established (a runtime fault in how memset nodes execute,
// or a cause the substitution only perturbed); the kernel fill is kept because it leaves kernel nodes as the only node type of the step's graphs.
int launch_zero_fill(void* p, size_t bytes, hipStream_t st);

// Per-channel thread mapping for pixel-major [P][ld] tensors with C channels (channel group of <= 256):
// G = 256 / cg pixels are processed side by side, thread t < G*cg owns channel (t % cg) of pixel slot (t / cg).
struct ChanMap {
    int cg0;     // first channel of this block's group
    int cg;      // channels in the group (<= 256)
    int G;       // pixel slots
    int c;       // my channel (absolute), -1 if idle
    int slot;    // my pixel slot
};
__device__ inline ChanMap chan_map(int C, int group_idx) {
    ChanMap m;
    m.cg0 = group_idx * 256;
    m.cg = min(256, C - m.cg0);
    m.G = 256 / m.cg;
    const int t = threadIdx.x;
    if (t < m.G * m.cg) { m.c = m.cg0 + t % m.cg; m.slot = t / m.cg; }
    else { m.c = -1; m.slot = 0; }
    return m;
}

}  // namespace dsrl
