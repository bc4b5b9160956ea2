// Device helpers and argument blocks shared by the implicit-GEMM conv kernels (conv_igemm.hip: register-staged operands,
// conv_planes.hip: operands as fp16 planes staged by LDS-DMA).
#pragma once
#include "common.h"

namespace dsrl {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;

// Split-precision arithmetic ("bf16x3": NPL = 2 planes, "bf16x6": NPL = 3): an fp32 value is carried as NPL bf16 terms
// x = t0 + t1 (+ t2), t0 = bf16(x), t1 = bf16(x - t0), t2 = bf16(x - t0 - t1), i.e. 16 (24) mantissa bits, and a product is the sum
// of the bf16 MFMAs a_i * b_j with i + j < NPL (3 or 6 of them), small terms first, all accumulated in fp32
// (conv_igemm_split_kernel, conv_wgrad_split_kernel).
//
// "f16x3" (F16 = true, NPL = 2, round 3): the two terms are fp16 instead of bf16, t0 = f16(x * 2^e), t1 = f16(x * 2^e - t0), i.e. 22 mantissa
// bits in 3 MFMAs (v_mfma_f32_32x32x16_f16: a0*b1 + a1*b0 + a0*b0) - the accuracy of bf16x6 / fp32 MFMA at half the matrix work and
// two thirds of the LDS bytes.  fp16 has 5 exponent bits, so every operand tensor carries a power-of-two scale: 2^e maps the tensor's
// largest magnitude into [2^14, 2^15) (e from a device word holding max |x| as its bit pattern, written by the tensor's producer or by
// amax_kernel), and the accumulators are multiplied by 2^-(ea + eb) in the epilogue - exact.  Elements more than 2^18 below the
// tensor's maximum lose low-order bits gracefully (absolute error <= 2^-40 of the maximum: invisible in any sum an fp32 kernel forms).
template <bool F16> struct Plane;
template <> struct Plane<false> {
    using v4 = bf16x4; using v8 = bf16x8;
    static __device__ __forceinline__ v4 cvt(const float* r) { return v4{(__bf16)r[0], (__bf16)r[1], (__bf16)r[2], (__bf16)r[3]}; }
    static __device__ __forceinline__ void residual(float* r, v4 t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] -= (float)t[e];
    }
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
// fp16 split of one staged float4 in 8 vector instructions behind the scaling: two v_cvt_pk_f16_f32 per term and the residual r - t as ONE
// v_fma_mix_f32 per element (t * -1.0 + r, t read as the low / high fp16 half of its packed word: exact, like the subtraction it replaces;
// hipcc unpacks t with four v_cvt_f32_f16 and re-converts r twice when the same is written with casts).
__device__ __forceinline__ float f16_resid_lo(unsigned t, float r) { float d; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(t), "v"(r)); return d; }
__device__ __forceinline__ float f16_resid_hi(unsigned t, float r) { float d; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(t), "v"(r)); return d; }
template <> struct Plane<true> {
    using v4 = f16x4; using v8 = f16x8;
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    static __device__ __forceinline__ v4 cvt(const float* r) { return __builtin_convertvector((f32x4{r[0], r[1], r[2], r[3]}), v4); }
    static __device__ __forceinline__ void residual(float* r, v4 t) {
        const u32x2 u = __builtin_bit_cast(u32x2, t);
        r[0] = f16_resid_lo(u.x, r[0]); r[1] = f16_resid_hi(u.x, r[1]); r[2] = f16_resid_lo(u.y, r[2]); r[3] = f16_resid_hi(u.y, r[3]);
    }
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
// e with max|x| * 2^e in [2^14, 2^15) from the bit pattern of max|x| (zero / subnormal maxima count as 2^-126; Inf / NaN maxima give a
// finite e: such tensors turn into NaN in the split by themselves)
__device__ __forceinline__ int amax_shift_of(unsigned fetched) {      // fetched: this lane's amax_fetch() of the record
    const unsigned u = amax_reduce(fetched);
    int ex = (int)((u >> 23) & 0xffu);
    if (ex == 0) ex = 1;
    return 14 - (ex - 127);
}
__device__ __forceinline__ int amax_shift(const unsigned* p) { return amax_shift_of(amax_fetch(p)); }

// q = n / d for 0 <= n < 2^31: m = ceil(2^(31+l) / d) with l = ceil(log2 d) >= 1, q = mulhi(n, m) >> (l - 1), exact; d = 1 is
// flagged by shift 255 (host side: make_magic)
__device__ __forceinline__ int fast_div(int n, unsigned m, unsigned s) {       // a select, not a branch: it sits inside the K loops (scalar and vector)
    const int q = (int)(__umulhi((unsigned)n, m) >> (s & 31u));
    return s == 255u ? n : q;
}

struct ConvArgs {
    const float* x; const float* w; const float* bias; float* y;
    int ldx, ldy;
    int N, H, W, C;          // input tensor of this pass (for dgrad: dy's N,Ho,Wo,K)
    int K;                   // output channels of this pass
    int R, S, Ho, Wo;        // Ho,Wo: output spatial size of this pass
    int stride, pad, dil;
    int M;                   // N*Ho*Wo
    int cchunks;             // ceil(C/32)
    int splits;
    long long slab;          // floats per split slab (M*K) when splits > 1
    unsigned x_bytes, w_bytes, y_bytes;   // extents of the three buffers (< 2^31): buffer loads/stores bounds-check against them
    int mtiles, ntiles, xcd_remap;        // 1-D launch of mtiles*ntiles blocks (x splits in z); XCD-aware tile order when xcd_remap
    int kg;                               // split kernels: K groups per block (1, 2 or 4)
    int accumulate;                       // epilogue: y += result (only without slabs: a split-K launch accumulates in its reduce)
    float* stats;                         // split kernels, forward: per (row block, channel) BatchNorm partials (n, mean, M2) of the output, or null
    // split kernels, dgrad: the output is the gradient w.r.t. the output y = relu(bn(x)) of a BatchNorm; the epilogue leaves the
    // partial sums of g = dy * [y > 0] and g * xhat per (row block, channel) in bstats [2][parts][K] (null: off)
    const float* bn_x; const float* bn_y; const float* bn_mean; const float* bn_invstd; float* bstats;
    int bn_ldx, bn_ldy, bn_relu;          // bn_relu == 2: bn_y addresses the sign mask uint32 [K / 32][bn_ldy] of that output (bn.hip: bn_stats_apply_kernel), not y itself
    float bn_gscale;                      // factor on the masked gradient: 1 / (1 - p) when a Dropout sits behind the BatchNorm's ReLU (round 5), else 1
    int bn_fast;                          // KG == 1 builds: the BatchNorm-backward sums through LDS with 16-byte loads of x / y (host: alignment, K % 4 == 0, no parity order)
    // KG == 1 data-gradient builds: the whole epilogue by float4 rows of the LDS-parked tile (RowEpilogue below; host: row_epilogue_ok).  bn_x_bytes / bn_y_bytes:
    // extents of bn_x and of bn_y (the output or its sign mask) for that epilogue's bounds-checked loads
    int row_epi;
    unsigned bn_x_bytes, bn_y_bytes;
    // split kernels, dgrad of a strided conv (par = stride > 1, else 0): the GEMM rows are ordered by parity class - M-tile t (pbm rows) holds
    // rows (t / par^2) * pbm ... of class (ph, pw) = t % par^2, a class row j being pixel (n, hh*par + ph, wh*par + pw), (n, hh, wh) = j over the
    // Hh x Wh grid of the class - so that all rows of a tile share the taps that divide evenly (a row-major tile multiplies zeros for the
    // other par^2 - 1 of par^2 taps per row), and consecutive tiles cycle through the classes (their tap counts differ: 4, 2, 2, 1 of 9).
    // Host side: Ho % par == Wo % par == 0, pixels per class % pbm == 0 (a tile never straddles classes), Wh % 32 == 0 (32 consecutive rows
    // are 32 consecutive pixels of one image row of the class: the epilogue derives their offsets from the first one).
    int par, Hh, Wh, pbm;
    const unsigned* amax_a; const unsigned* amax_b;     // f16x3: amax records of the input tensor x and of the filter w
    int w_split;                                        // f16x3: `w` is the pre-split filter (kernel ARITH = 2)
    unsigned mHW, sHW, mW, sW, mNT, sNT;                // split kernels: magic numbers of the divisions by Ho*Wo, Wo and ntiles (fast_div; host: make_magic)
    // conv_planes_kernel: x / w point at the FIRST fp16 plane of the operand ([P][ldx] resp. [K][R][S][C] fp16, ldx in fp16 elements, x_bytes / w_bytes =
    // extent of one plane); the second plane lies a_lo / b_lo bytes behind it (unused with one plane)
    unsigned a_lo, b_lo;
    int planes;                                         // host side: route the launch to conv_planes_kernel
    // split-K ACROSS workgroups with the reduction inside the launch (conv_sk.hip, template COOP): the `splits` blocks of a tile (blockIdx.z) publish
    // their partial tiles in coop_slab [z][tile][...], take a ticket, and the block whose ticket is the last one adds them in the order z = 0 .. splits-1
    // and runs the whole epilogue (bias, accumulate, BatchNorm partials) on y.  tickets: one zeroed word per tile, left zero by the last arriver.
    float* coop_slab; unsigned* tickets;
};
// Arrival tickets of the cooperative split-K launches live in the words of the ACTIVATION operand's amax record that carry no shard: a record is
// kAmaxWords words of which every kAmaxShardStride-th holds a partial maximum; the other 240 are zero whenever the record is (arena fill, scratch
// fill) and nothing else touches them.  Ticket t < kCoopMaxTiles sits at word 16 * (t / 15) + 1 + t % 15.  The launches of a stream run one after the
// other and each leaves its tickets zero, so the convs that share an input tensor share its tickets.
constexpr int kCoopMaxTiles = (kAmaxShardStride - 1) * kAmaxShards;
__host__ __device__ inline int coop_ticket_word(int t) { return kAmaxShardStride * (t / (kAmaxShardStride - 1)) + 1 + t % (kAmaxShardStride - 1); }
__device__ __forceinline__ int dgrad_pix(const ConvArgs& a, int m) {        // row of the parity-ordered GEMM -> pixel index (n*Ho + h)*Wo + w
    const int t = m / a.pbm, p2 = a.par * a.par, c = t % p2, j = (t / p2) * a.pbm + (m - t * a.pbm);
    const int hw = a.Hh * a.Wh, n = j / hw, r = j - n * hw, hh = r / a.Wh, wh = r - hh * a.Wh;
    const int ph = c / a.par, pw = c - ph * a.par;
    return (n * a.Ho + hh * a.par + ph) * a.Wo + wh * a.par + pw;
}

// bn_relu == 2: the word of the sign mask that holds channel k of pixel px (bit k % 32 = y > 0), and a nibble of it as the "y" of four channels (1 or 0)
__device__ __forceinline__ unsigned bn_mask_word(const ConvArgs& a, int k, long long px) {
    return reinterpret_cast<const unsigned*>(a.bn_y)[(long long)(k >> 5) * a.bn_ldy + px];
}
__device__ __forceinline__ float4 bn_mask4(unsigned w) { return make_float4((w & 1u) ? 1.f : 0.f, (w & 2u) ? 1.f : 0.f, (w & 4u) ? 1.f : 0.f, (w & 8u) ? 1.f : 0.f); }

// Blocks are dealt round-robin over the 8 XCDs (private L2 each). Remap the linear block id so that every XCD works on a contiguous
// range of tile ids (bijective for any count): tiles that share input rows then hit the same L2. Speed only, never correctness.
__device__ inline int xcd_contiguous(int bid, int n) {
    const int q = n / kNumXCD, r = n % kNumXCD, xcd = bid % kNumXCD, local = bid / kNumXCD;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
constexpr unsigned kOOB = 0x80000000u;      // any offset >= 2^31 is outside every descriptor: loads return 0, stores are dropped
__device__ inline float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// ------------------------------------------------------------------------------------------------ row epilogue (one-group data-gradient builds)
// The accumulator layout (lane = column, register = row) makes every epilogue access 4 bytes wide, and the scalar epilogue of an accumulating launch
// pays one full memory round trip per 32x32 piece of the wave tile (load the old values, wait, add, store, next piece), then bn_fast's round trip for
// x / y of the BatchNorm - all of it on cold lines behind the last MFMA.  None of these operands depends on the accumulators.  Here a wave
//   fetch():  requests EVERYTHING the epilogue reads - the old y rows, the first NB rows of the BatchNorm's x and y (or sign-mask words), mean / invstd -
//             as float4 rows with unconditional buffer loads (dead rows: out-of-range offsets), before its tile is parked;
//   park():   writes its finished 32 MR x 32 NR tile to its private region of the idle LDS stages (where bn_fast parks it);
//   pass():   one pass over the float4 rows: y = (acc + old) + bias with one 16-byte store, and the BatchNorm-backward sums of the same values in
//             bn_fast's row and shuffle order.
// Every floating-point operation and its order are those of the scalar epilogue followed by bn_fast: the results are bit-identical.
// Shared by conv_igemm_split_kernel and conv_planes_kernel.  Row it of lane l: tile row l / CQ + RSTEP * it, channels 4 * (l % CQ) .. + 3.
template <int MR, int NR>
struct RowEpilogue {
    static constexpr int TR = 32 * MR, TC = 32 * NR, CQ = TC / 4, RSTEP = 64 / CQ, NIT = TR / RSTEP, NB = NIT < 8 ? NIT : 8;
    int c4, r0, kk, mrow0;
    bool kok4;
    u32x4 old[NIT];
    u32x4 xv[NB], yv[NB];
    unsigned mw[NB];
    float4 mu4, is4;

    // BatchNorm operands of rows b0 .. b0 + NB - 1: x, y (bn_relu == 1) and the sign-mask word (bn_relu == 2); what the launch does not read is out of range
    __device__ __forceinline__ void fetch_bn(const ConvArgs& a, __amdgpu_buffer_rsrc_t bx, __amdgpu_buffer_rsrc_t by, int b0) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int m = mrow0 + r0 + RSTEP * (b0 + u);
            const bool ok = kok4 && m < a.M && a.bstats != nullptr;
            xv[u] = __builtin_amdgcn_raw_buffer_load_b128(bx, (int)(ok ? ((unsigned)m * (unsigned)a.bn_ldx + (unsigned)kk) * 4u : kOOB), 0, 0);
            yv[u] = __builtin_amdgcn_raw_buffer_load_b128(by, (int)((ok && a.bn_relu == 1) ? ((unsigned)m * (unsigned)a.bn_ldy + (unsigned)kk) * 4u : kOOB), 0, 0);
            mw[u] = __builtin_amdgcn_raw_buffer_load_b32(by, (int)((ok && a.bn_relu == 2) ? ((unsigned)(kk >> 5) * (unsigned)a.bn_ldy + (unsigned)m) * 4u : kOOB), 0, 0);
        }
    }
    // mrow0_: first GEMM row of the wave tile, kcol0: its first output channel
    __device__ __forceinline__ void fetch(const ConvArgs& a, __amdgpu_buffer_rsrc_t yr, __amdgpu_buffer_rsrc_t bx, __amdgpu_buffer_rsrc_t by, int lane, int mrow0_, int kcol0) {
        c4 = lane % CQ; r0 = lane / CQ; mrow0 = mrow0_;
        kk = kcol0 + 4 * c4;
        kok4 = kk < a.K;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {          // all old rows of the tile are requested before the first store
            const int m = mrow0 + r0 + RSTEP * it;
            old[it] = __builtin_amdgcn_raw_buffer_load_b128(yr, (int)((kok4 && m < a.M && a.accumulate) ? ((unsigned)m * (unsigned)a.ldy + (unsigned)kk) * 4u : kOOB), 0, 0);
        }
        fetch_bn(a, bx, by, 0);
        const bool st = kok4 && a.bstats != nullptr;
        mu4 = st ? *reinterpret_cast<const float4*>(a.bn_mean + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        is4 = st ? *reinterpret_cast<const float4*>(a.bn_invstd + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ void park(float* wt, const f32x16 (&acc)[MR][NR], int lane) const {
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    wt[(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) * TC + j * 32 + (lane & 31)] = acc[i][j][e];
    }
    // part / nparts: the wave row's block of BatchNorm partials [2][nparts][K]
    __device__ __forceinline__ void pass(const ConvArgs& a, __amdgpu_buffer_rsrc_t yr, __amdgpu_buffer_rsrc_t bx, __amdgpu_buffer_rsrc_t by, const float* wt, int lane,
                                         int part, int nparts) {
        float bv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = (a.bias != nullptr && kok4) ? a.bias[kk + e] : 0.f;
        const bool sums = a.bstats != nullptr;
        float sg[4] = {0.f, 0.f, 0.f, 0.f}, sgx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b0 = 0; b0 < NIT; b0 += NB) {
            if (b0 > 0) fetch_bn(a, bx, by, b0);
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int row = r0 + RSTEP * (b0 + u), m = mrow0 + row;
                const bool ok = kok4 && m < a.M;
                float4 gv = *reinterpret_cast<const float4*>(wt + row * TC + 4 * c4);
                if (a.accumulate) {
                    const u32x4 o = old[b0 + u];
                    gv.x += __uint_as_float(o.x); gv.y += __uint_as_float(o.y); gv.z += __uint_as_float(o.z); gv.w += __uint_as_float(o.w);
                }
                const u32x4 q = {__float_as_uint(gv.x + bv[0]), __float_as_uint(gv.y + bv[1]), __float_as_uint(gv.z + bv[2]), __float_as_uint(gv.w + bv[3])};
                __builtin_amdgcn_raw_buffer_store_b128(q, yr, (int)(ok ? ((unsigned)m * (unsigned)a.ldy + (unsigned)kk) * 4u : kOOB), 0, 0);
                if (sums && ok) {
                    float4 y4 = make_float4(1.f, 1.f, 1.f, 1.f);
                    if (a.bn_relu == 2) y4 = bn_mask4(mw[u] >> (kk & 31));          // the lane's four channels: one nibble of the sign mask
                    else if (a.bn_relu) y4 = make_float4(__uint_as_float(yv[u].x), __uint_as_float(yv[u].y), __uint_as_float(yv[u].z), __uint_as_float(yv[u].w));
                    const float4 x4 = make_float4(__uint_as_float(xv[u].x), __uint_as_float(xv[u].y), __uint_as_float(xv[u].z), __uint_as_float(xv[u].w));
                    const float gs = a.bn_gscale;            // 1 / (1 - p) of a Dropout behind the ReLU (its mask is y > 0 as well), else 1: exact
                    const float g0 = (a.bn_relu && !(y4.x > 0.f)) ? 0.f : gv.x * gs, g1 = (a.bn_relu && !(y4.y > 0.f)) ? 0.f : gv.y * gs;
                    const float g2 = (a.bn_relu && !(y4.z > 0.f)) ? 0.f : gv.z * gs, g3 = (a.bn_relu && !(y4.w > 0.f)) ? 0.f : gv.w * gs;
                    sg[0] += g0; sgx[0] += g0 * ((x4.x - mu4.x) * is4.x);
                    sg[1] += g1; sgx[1] += g1 * ((x4.y - mu4.y) * is4.y);
                    sg[2] += g2; sgx[2] += g2 * ((x4.z - mu4.z) * is4.z);
                    sg[3] += g3; sgx[3] += g3 * ((x4.w - mu4.w) * is4.w);
                }
            }
        }
        if (!sums) return;
#pragma unroll
        for (int sft = CQ; sft < 64; sft <<= 1)
#pragma unroll
            for (int q = 0; q < 4; ++q) { sg[q] += __shfl_xor(sg[q], sft); sgx[q] += __shfl_xor(sgx[q], sft); }
        if (lane < CQ && kok4) {
            float* o = a.bstats + (long long)part * a.K + kk;
            *reinterpret_cast<float4*>(o) = make_float4(sg[0], sg[1], sg[2], sg[3]);
            *reinterpret_cast<float4*>(o + (long long)nparts * a.K) = make_float4(sgx[0], sgx[1], sgx[2], sgx[3]);
        }
    }
};

// Row epilogue for this pass / tile / arguments?  The ONE answer behind ConvArgs::row_epi and the dynamic-LDS size of every launcher (launch_igemm,
// launch_sk_igemm, the planes launch), so the flag and the LDS cannot disagree.  a: the launch's arguments with bn_fast already decided for the tile.
//   * stride-1 data gradient of an fp16 arithmetic on a one-group build, writing finished values (no slabs: splits == 1, or the cooperative launch);
//   * output channels and ldy multiples of 4, y 16-byte aligned, no parity order; the block tile fits 128 KiB of LDS (bn_fast's rule: up to 256x128);
//   * BatchNorm sums asked for: bn_fast's own conditions hold, and x / y of the BatchNorm lie inside a buffer descriptor's 2 GiB;
//   * the launch has epilogue operands to fetch (it accumulates or takes the sums).  Plain data gradients and every forward launch keep the scalar
//     epilogue: a row store with no loads to hide has to earn its LDS round trip, and that was not measured (docs/next_round_notes.md §3, item 5).
// DSRL_ROW_EPILOGUE=0: never.  Changes no size query.
inline bool row_epilogue_ok(const ConvArgs& a, bool dgrad, bool f16, int bm, int bn) {
    if (!dgrad || !f16 || a.kg > 1 || a.stride != 1 || a.par != 0) return false;
    if (a.splits > 1 && a.tickets == nullptr) return false;
    if (a.K % 4 != 0 || a.ldy % 4 != 0 || ((uintptr_t)a.y % 16) != 0 || (size_t)bm * bn * 4 > 128 * 1024) return false;
    if (a.bstats != nullptr && !(a.bn_fast && a.bn_x_bytes != 0 && (a.bn_relu == 0 || a.bn_y_bytes != 0))) return false;
    if (!a.accumulate && a.bstats == nullptr) return false;
    if (a.accumulate && a.stats != nullptr) return false;       // forward statistics are taken from the registers, which the row pass leaves without the old values
    return knob("DSRL_ROW_EPILOGUE", 1) != 0;
}
// bytes of dynamic LDS the epilogue of this launch parks its tile in (0: the scalar epilogue, nothing parked)
inline size_t epilogue_tile_bytes(const ConvArgs& a, int bm, int bn) { return (a.kg <= 1 && (a.bn_fast || a.row_epi)) ? (size_t)bm * bn * 4 : (size_t)0; }

struct WgradArgs {
    const float* x; const float* dy; float* dw;     // dw or slabs
    int ldx, lddy;
    int N, H, W, C, K, R, S, Ho, Wo, stride, pad, dil;
    long long P;                // N*Ho*Wo
    unsigned x_bytes, dy_bytes; // buffer extents (< 2^31)
    int ctiles;                 // tiles along C
    int psplits;
    long long slab;             // floats per split slab (K*RS*C) when psplits > 1
    int taps[64]; int ntaps;    // active filter taps (whole-tensor)
    int xcd_remap;              // pixel-range-major block order per XCD (blocks of one pixel range share dy / x chunks)
    int kctiles;                // ktiles * ctiles
    unsigned mHW, sHW, mW, sW;  // magic multipliers / shifts: p / (Ho*Wo) and rem / Wo for p < 2^31 (fast_div)
    int kg;                     // split kernel: pixel groups per block (1, 2 or 4)
    // grouped launches (dsrl_conv2d_wgrad_group_*): blocks of this problem (the rest up to the next start are padding), where the
    // slab reduce writes, and that reduce's block count
    int nblocks;
    float* dw_final;
    int rblocks;
    const unsigned* amax_dy; const unsigned* amax_x;        // f16x3: max |.| (bit patterns) of dy and of x
    int no_ident;               // DSRL_WGRAD_IDENT=0: the general per-row addressing also for taps that read pixel p for pixel p (A/B knob)
};

// conv_wgrad3.hip: 3x3 / stride-1 weight gradients with all nine taps in one block (f16x3 / f16x1; tile 64 out channels x 64 in channels: wgrad3_tile()).
// WgradArgs as for conv_wgrad_split_kernel with ntaps = 9, kctiles = tiles of that size, nblocks = kctiles * psplits.
bool wgrad3_eligible(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil, int npl, bool f16);
void wgrad3_tile(int& bm, int& bn);
int launch_wgrad3(const WgradArgs& a, int npl, hipStream_t st);
int launch_wgrad3_group(const WgradArgs* table, const int* starts, int nprob, int grid, int npl, int dil, hipStream_t st);

// conv_planes.hip: the same implicit GEMM with both operands as fp16 planes staged by LDS-DMA (a.x / a.w / a.a_lo / a.b_lo as described in ConvArgs);
// cfg is conv_igemm.hip's TileCfg, the tile / K-group / split-K plan (and with it the summation order) is the caller's.
bool planes_cfg_supported(int cfg, int kg);
int launch_planes_igemm(const ConvArgs& a, int cfg, bool dgrad, hipStream_t st);
// conv_sk.hip: 128x128 tiles, two K groups (8 waves), f16x3 / f16x1 with pre-split filters; a.splits > 1 with a.tickets set = cooperative split-K
bool sk_supported(int cfg, int kg, int npl, bool f16, bool w_split);
size_t sk_lds_bytes();
int launch_sk_igemm(const ConvArgs& a, bool dgrad, bool str1, int npl, hipStream_t st);
__host__ __device__ inline long long planes_lo_offset(long long elems) { return (elems * 2 + 255) / 256 * 256; }      // bytes from the first to the second plane

}  // namespace dsrl
