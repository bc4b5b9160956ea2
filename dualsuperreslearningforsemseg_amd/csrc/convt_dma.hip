// ConvTranspose2d k2 s2 backward with LDS-DMA staging (round 5): the logits tail of the step (models/DSRL.py:53-69 of the reference builds the layer,
// loss.backward() of train_or_resume.py:435-444 runs this pass).
//
// convt2x2_bwd_mfma_kernel (spatial.hip) loads a 128-pixel segment into 52 registers per lane, re-lays it out with ds_write_b32 behind two
// barriers and needs all 256 VGPRs, so a CU holds two blocks whose staging phases leave the matrix pipe half idle (169 us for 478 MB on the step's
// last layer).  Here the segment goes global -> LDS with buffer_load_dwordx4 ... lds in the layout it has in memory:
//     stage = [dy row 2h, pixels 2*w0 .. 2*w0+255][dy row 2h+1, the same pixels][x row h, pixels w0 .. w0+127]      (19 + 19 + 10 KB for 19 channels)
// With an odd channel count the MFMA operand reads of that layout hit distinct banks: the gradient of input pixel p, column k = tap*CO + co of the
// [px x 4 CO] matrix sits at word p * 2 CO + k (k < 2 CO, output row 2h) or one row segment further (k >= 2 CO), and 2 CO * p mod 64 is a bijection
// of 32 pixels onto the even banks (the half-wave with k + 1 reads the odd ones).  No registers, no ds_write, ONE barrier per segment, a ring of three
// stages.
// A block = 8 waves: waves 0-3 form dx [32 px x CI] = G . W^T of their 32 pixels (38 x v_mfma_f32_32x32x2_f32, filter in registers) and store it;
// waves 4-7 issue the DMA pieces (they have no other vector memory traffic, so their s_waitcnt vmcnt sees exactly the pieces) and accumulate
// dw [(CI + 1) x 4 CO] = X^T . G over every segment of the block (row CI multiplies ones: db per tap).  The arithmetic, the accumulation order within
// a segment and the per-block partial layout are those of convt2x2_bwd_mfma_kernel; convt2x2_dw_finalize_kernel merges the partials.
//
// CE = true (dsrl_convt2x2_bwd_ce): the layer's output IS the logits of nn.CrossEntropyLoss and the incoming gradient is never materialised.  The
// DMA brings the LOGITS rows and the target bytes of the segment, and d(loss)/d(logits) is formed in place in LDS - max, exp, sum, scale in the order
// and with the roundings of ce_fused_kernel (losses.hip), plus the stride-s feature transformer's rank-one contribution g * w_c on the sampled pixels
// (pointwise_bwd_kernel's `dx += g * w`) - one segment ahead of the MFMAs that consume it.  TW = true (default): by four more waves (8-11, one per SIMD,
// two output pixels per lane) while waves 0-7 multiply the previous segment; TW = false (DSRL_CONVT_CE_WAVES=8): inside the eight MFMA waves, one
// pixel per lane, the dx waves before their MFMAs and the dw waves after theirs.  The 319 MB gradient write of the loss pass and its 319 MB read
// here disappear; results are bit-identical to ce_fused + pointwise_bwd + this kernel with CE = false.
// Measured (profiles/round5_convt_tail.txt): 135 us without CE, 176-183 us with (TW), 188-195 (TW = false).  The softmax does not hide behind the
// MFMAs: SQ counters read 43 % of the SIMD cycles in MFMAs + 28 % in the other vector instructions with no co-execution counted, i.e. the ~290
// vector instructions per pixel add to the matrix work whichever wave issues them.
#include "common.h"
#include "lds_dma.h"
#include <algorithm>
#include <type_traits>

namespace dsrl {

using f32x16_t = __attribute__((ext_vector_type(16))) float;

struct ConvtCeArgs {
    const unsigned char* target;    // (N, 2H, 2W) labels
    const float* count;             // number of pixels that are not ignore_index (ce_finalize_kernel's out[1])
    const float* ft_g;              // (N, Hf, Wf) incoming gradient of the stride-s 1x1 conv on the logits, or null
    const float* ft_w;              // its CO weights
    int ignore_index, ft_s, ft_shift, Hf, Wf;     // ft_shift = log2(ft_s) when ft_s is a power of two, else -1
    const float* wtab;              // CW: the 256-float class-weight table, and `count` points to D
    float gamma;                    // FL: the focal exponent (> 0)
    float eps;                      // SM: the label smoothing (0 < eps <= 1)
};
// the arguments of the DC build: a type of its own, so that the kernel arguments of every other instantiation keep their size and offsets
struct ConvtCeDiceArgs : ConvtCeArgs {
    const float* dice;              // the record of dsrl_dice_fwd {lambda L_dice, |K|, a[0..CO), b[0..CO)}
};
// and of the LV build, for the same reason
struct ConvtCeLovaszArgs : ConvtCeArgs {
    const float* lovasz;            // the record of dsrl_lovasz_fwd {lambda L, |Present|, 0, 0, gf[CO][bins], gb[CO][bins]}
    int bins;                       // K, a power of two in [16, 4096]
};
// and of the RX build
struct ConvtCeRelaxArgs : ConvtCeArgs {
    const unsigned* mask;           // (N, 2H, 2W) class-set words (dsrl_relax_mask, or any words: relax_set cleans them)
};
template <bool DC, bool LV, bool RX = false>
using ConvtCeArgsOf = std::conditional_t<DC, ConvtCeDiceArgs, std::conditional_t<LV, ConvtCeLovaszArgs, std::conditional_t<RX, ConvtCeRelaxArgs, ConvtCeArgs>>>;

// CW = true (dsrl_convt2x2_bwd_ce_w): nn.CrossEntropyLoss(weight=).  ce.count points to D = sum n_c w_c and the only change is in transform(): the
// per-pixel sc = wtab[target] * (1 / D) stands where `scale` stands, as in ce_fused_body<true> (losses.hip).  The 256-float table sits in LDS, already
// multiplied by 1 / D (indexed by the label byte: entries >= CO are zero).  A template parameter, so that the CW = false instantiations compile to the
// code they were.
// FL = true (dsrl_convt2x2_bwd_ce_f): focal cross entropy.  transform() also forms so = sum_{c != t} e_c beside s and reads v_t once more from the
// stage (the raw logits are still there), focal_pixel (common.h) gives mod from them, and sc = (w[t] * mod) * (1 / D) as in ce_fused_body<true, true>:
// the table in LDS holds the raw weights here, so that the product rounds as it does there.  Everything after sc is the weighted code.
// SM = true (dsrl_convt2x2_bwd_ce_s): label-smoothed cross entropy.  The table in LDS holds the raw weights (its first CO entries are the per-class w_c
// of the smoothing term), W = sum_c w_c is summed from it once per block, a second table holds smooth_sub of every class, and the row is smooth_pixel /
// smooth_grad (common.h) on the e_c in registers, as ce_fused_body<true, false, true> forms it from its tile.  A backward needs no value, hence no log.
// DC = true (dsrl_convt2x2_bwd_ce_d): the weighted cross entropy plus the soft Dice term.  The coefficient tables a and b of the
// record sit in LDS beside the weight table (in sub_s, which the label smoothing does not use here), the row is (weighted CE row) + (Dice row) with
// the Dice row from dice_pixel / dice_grad (common.h) on the e_c in registers, and the transformer's g * w is added after that: the order and the
// roundings of dsrl_ce_fused_w -> dsrl_dice_bwd(accumulate = 1) -> dsrl_pointwise_strided_bwd.
// LV = true (dsrl_convt2x2_bwd_ce_l): the weighted cross entropy plus the Lovasz-Softmax term.  The record's tables (155 KB at
// 19 classes and 1024 levels) do not fit LDS beside the ring: lovasz_pixel (common.h) gathers the 19 coefficients of a pixel from global memory /
// L2 with the e_c in registers and keeps them there, the row is (weighted CE row) + (Lovasz row) through lovasz_grad, and the transformer's g * w is
// added after that: the order and the roundings of dsrl_ce_fused_w -> dsrl_lovasz_bwd(accumulate = 1) -> dsrl_pointwise_strided_bwd.
// RX = true (dsrl_convt2x2_bwd_ce_r): boundary label relaxation.  The label bytes arrive through the ring as ever; the pixel's
// class-set word is fetched from global memory at the top of transform(), where the transformer's gradient is fetched, so that the softmax covers its
// latency.  The row is relax_pixel / relax_grad (common.h) on the e_c in registers and the raw logits still in the stage, as
// ce_fused_body<true, false, false, true> forms it from its tile: m_S, inv, invz and the set word beside the 19 terms, g_c recomputed per class.
template <int CI, int CO, bool CE, bool TW = false, bool CW = false, bool FL = false, bool SM = false, bool DC = false, bool LV = false, bool RX = false>
__global__ __launch_bounds__(TW ? 768 : 512, 1) void convt2x2_bwd_dma_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy,
                                                                 float* __restrict__ dx, float* __restrict__ part, int N, int H, int W,
                                                                 int nseg_per_row, int nseg, ConvtCeArgsOf<DC, LV, RX> ce) {
    static_assert(CE || !CW, "class weights belong to the CE build");
    static_assert(!FL || CW, "the focal loss runs on the weighted machinery");
    static_assert(!SM || (CW && !FL), "label smoothing runs on the weighted machinery and has no focal form");
    static_assert(!DC || (CW && !FL && !SM && !TW && CO <= 32), "the Dice term runs on the weighted machinery, in the 8-wave build");
    static_assert(!LV || (CW && !FL && !SM && !TW && !DC), "the Lovasz term runs on the weighted machinery, in the 8-wave build");
    static_assert(!RX || (CW && !FL && !SM && !TW && !DC && !LV && CO <= kRelaxMaxC), "label relaxation runs on the weighted machinery, in the 8-wave build");
    constexpr int TP = 128, COLS = 4 * CO, NK = COLS / 2, NJ = (COLS + 31) / 32, NOUT = CI * COLS;
    constexpr int XB = TP * CI * 4, XP = (XB + 1023) / 1024;               // bytes / 1 KB pieces of an x segment
    constexpr int GB = 2 * TP * CO * 4, GP = GB / 1024;                    // of one dy row segment
    constexpr int PIECES = XP + 2 * GP + (CE ? 2 : 0), STAGE = PIECES * 1024, S = 3;
    constexpr int MAXPW = (PIECES + 3) / 4;                                // pieces per DMA wave (wave q takes pieces q, q + 4, ...)
    constexpr int GW = GB / 4;                                             // words between the two gradient rows of a stage
    constexpr int TOFF = (XP + 2 * GP) * 1024;                             // target bytes of the two output rows: 1 KB slots, 2 TP bytes used
    static_assert(CI < 32 && CO % 2 == 1 && NJ <= 3 && GB % 1024 == 0 && MAXPW <= 30 && 2 * TP <= 1024, "tile does not fit this kernel");
    static_assert(S * STAGE <= 160 * 1024, "three stages in LDS");
    static_assert((3 * NJ * 16 * 64 + (CI + 1) * COLS) * 4 <= S * STAGE, "the final merge of the dw tiles reuses the ring");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned ring_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_dw = wave >= 4 && wave < 8, is_tw = wave >= 8;           // waves 0-3: dx, 4-7: DMA + dw, 8-11 (CE): logits -> gradient
    const int wq = wave & 3;                                               // quarter of the segment this wave works on / DMA lane of the dw waves
    const int l31 = lane & 31, lh = lane >> 5;
    const int px0 = 32 * wq;
    const int grid = (int)gridDim.x;

    // Three descriptors for the whole tensors, made once; a piece's position travels in the scalar offset (segment + piece: a few scalar adds per
    // segment instead of three 64-bit descriptors, which cost 40 spilled SGPRs and a scalar preamble in every wave of the CE build).  The scalar offset
    // is not bounds-checked, so only pieces that lie inside their tensor use it; the x piece that crosses the end of its segment and the 1 KB label
    // pieces (2 TP bytes of a row are used) carry their position in the checked vector offset: they fetch neighbouring bytes of the tensor into LDS
    // words nobody reads, and zeros past the end of the tensor.  The host checks that every tensor is below 4 GB.
    const unsigned l16 = (unsigned)lane * 16u;
    const dma_u32x4 rs_dy = make_rsrc(dy, (unsigned)((long long)N * 4 * H * W * CO * 4));
    const dma_u32x4 rs_x = make_rsrc(x, (unsigned)((long long)N * H * W * CI * 4));
    const dma_u32x4 rs_t = make_rsrc(CE ? (const void*)ce.target : (const void*)dy, (unsigned)((long long)N * 4 * H * W));
    auto issue = [&](int seg, int slot) {                                  // dw waves only: this wave's pieces of the segment
        const int row = seg / nseg_per_row;                                // n*H + h
        const int w0 = (seg - row * nseg_per_row) * TP;
        const int n = row / H, h = row - n * H;
        const unsigned opx = (unsigned)((n * 2 * H + 2 * h) * (2 * W) + 2 * w0);         // first output pixel of the segment (row 2h)
        const unsigned o0 = opx * (unsigned)(CO * 4), o1 = o0 + (unsigned)(2 * W * CO * 4);  // byte offsets of the two gradient rows
        const unsigned ox = (unsigned)(row * W + w0) * (unsigned)(CI * 4);
        const unsigned base = ring_lds + (unsigned)(slot * STAGE);
#pragma unroll
        for (int i = 0; i < MAXPW; ++i) {
            const int q = wq + 4 * i;                                       // wave-uniform
            const unsigned lds = base + (unsigned)q * 1024u;
            if (q < GP) lds_dma16(rs_dy, l16, o0 + (unsigned)(q * 1024), lds);
            else if (q < 2 * GP) lds_dma16(rs_dy, l16, o1 + (unsigned)((q - GP) * 1024), lds);
            else if (q < 2 * GP + XP - 1 || XB % 1024 == 0) lds_dma16(rs_x, l16, ox + (unsigned)((q - 2 * GP) * 1024), lds);
            else if (q < 2 * GP + XP) lds_dma16(rs_x, l16 + ox + (unsigned)((XP - 1) * 1024), 0u, lds);           // may cross the end of x: checked offset
            else if (CE && q < PIECES) lds_dma16(rs_t, l16 + opx + (unsigned)((q - (2 * GP + XP)) * 2 * W), 0u, lds);   // 1 KB from a 2 TP byte row: likewise
        }
    };

    // ---- CE: logits -> d(loss)/d(logits) of this wave's 64 output pixels of a landed stage, in place.  ce_fused_kernel's arithmetic, per pixel:
    //      m = max, e_c = exp_nonpos(v_c - m), s = sum e_c (c ascending), dl_c = e_c * (scale / s) - (c == target ? scale : 0); ignored pixel: zeros
    float scale = 0.f;
    __shared__ float ftw_s[32];                                            // the feature transformer's weights (read as a broadcast by the few lanes on its grid)
    if (CE) {
        scale = 1.f / ce.count[0];
        if (tid < 32) ftw_s[tid] = (ce.ft_g && tid < CO) ? ce.ft_w[tid] : 0.f;          // visible after the first barrier below
    }
    __shared__ float wt_s[CW ? 256 : 1];
    __shared__ float sub_s[SM ? 32 : DC ? 64 : 1];                         // SM: ((eps / C) w_c) scale of every class; DC: a_c at c, b_c at 32 + c; published with wt_s
    if (SM && tid < 32) sub_s[tid] = tid < CO ? smooth_sub(ce.eps, CO, ce.wtab[tid], scale) : 0.f;
    if constexpr (DC) {
        if (tid < 64) sub_s[tid] = (tid & 31) < CO ? ce.dice[2 + (tid >> 5) * CO + (tid & 31)] : 0.f;
    }
    if (CW) {
        if (tid < 256) wt_s[tid] = (FL || SM) ? ce.wtab[tid] : ce.wtab[tid] * scale;   // sc of a pixel with label tid (FL, SM: its weight; sc is formed per pixel)
        // block_barrier() is a bare s_barrier: it does not wait for this wave's ds_write, so drain the LDS counter before the barrier that publishes the table
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    float Wsum = 0.f;                                                      // SM: sum_c w_c
    auto transform = [&](int seg, int slot) {                              // TW: wave wq of the tw waves takes 128 output pixels, two per lane; else every wave 64
        const int r = TW ? wq >> 1 : (is_dw ? 1 : 0);                       // output row 2h + r of the segment
        // the transformer's gradient g of this lane's pixels, fetched FIRST: the softmax arithmetic covers its latency (fetched where it is used it
        // stalled the wave for a memory round trip in every fourth row: +19 us on the step's last layer).  Odd output rows are never on the grid.
        float gft[TW ? 2 : 1];
        bool gon[TW ? 2 : 1];
#pragma unroll
        for (int u = 0; u < (TW ? 2 : 1); ++u) { gft[u] = 0.f; gon[u] = false; }
        bool any_grid = false;
        unsigned mword = 0u;                                                // RX: the class-set word of this lane's pixel, requested before anything else
        if constexpr (RX) {
            const int row = seg / nseg_per_row;
            const int w0 = (seg - row * nseg_per_row) * TP;
            const int n = row / H, h = row - n * H;
            mword = ce.mask[(long long)(n * 2 * H + 2 * h + r) * (2 * W) + 2 * w0 + wq * 64 + lane];
        }
        if (ce.ft_g && r == 0) {
            const int row = seg / nseg_per_row;
            const int w0 = (seg - row * nseg_per_row) * TP;
            const int n = row / H, oh = 2 * (row - n * H);
            const bool row_on = ce.ft_shift >= 0 ? (oh & (ce.ft_s - 1)) == 0 : oh % ce.ft_s == 0;      // wave-uniform
            if (row_on) {
                any_grid = true;
                const int fh = ce.ft_shift >= 0 ? oh >> ce.ft_shift : oh / ce.ft_s;
#pragma unroll
                for (int u = 0; u < (TW ? 2 : 1); ++u) {
                    const int ow = 2 * w0 + (TW ? (wq & 1) * 128 + u * 64 + lane : wq * 64 + lane);
                    const bool on = ce.ft_shift >= 0 ? (ow & (ce.ft_s - 1)) == 0 : ow % ce.ft_s == 0;
                    const int fw = ce.ft_shift >= 0 ? ow >> ce.ft_shift : ow / ce.ft_s;
                    gon[u] = on;
                    if (on) gft[u] = ce.ft_g[((long long)n * ce.Hf + fh) * ce.Wf + fw];
                }
            }
        }
#pragma unroll 1
        for (int u = 0; u < (TW ? 2 : 1); ++u) {                            // (rolled: two pixels in flight would need 2 x 19 more registers)
            const float g_u = (TW && u) ? gft[TW ? 1 : 0] : gft[0];
            const bool on_u = (TW && u) ? gon[TW ? 1 : 0] : gon[0];
            const int j = TW ? (wq & 1) * 128 + u * 64 + lane : wq * 64 + lane;       // output pixel 2*w0 + j of that row
            float* v = reinterpret_cast<float*>(smem + slot * STAGE) + r * GW + j * CO;
            const int tg = reinterpret_cast<const unsigned char*>(smem + slot * STAGE + TOFF + r * 1024)[j];
            float e[CO];
#pragma unroll
            for (int c = 0; c < CO; ++c) e[c] = v[c];
            float m = e[0];
#pragma unroll
            for (int c = 1; c < CO; ++c) m = fmaxf(m, e[c]);
            float s = 0.f, so = 0.f;
#pragma unroll
            for (int c = 0; c < CO; ++c) { e[c] = exp_nonpos(e[c] - m); s += e[c]; if (FL) so += c == tg ? 0.f : e[c]; }
            // e_c * inv - (c == tg ? scale : 0), zeros for an ignored pixel; then the feature transformer's term: ((e * inv) - scale) + g * w, the
            // roundings of ce_fused_kernel and pointwise_bwd_kernel.  Everything stays in registers between the 19 reads and the 19 writes: a
            // read-modify-write of the target word in LDS instead of the 19 selects measured +11 us
            const bool live = tg != ce.ignore_index;
            if (SM) {
                double val; float sub_t, inv;
                smooth_pixel<false>(v, wt_s, CO, tg, m, s, ce.eps, Wsum, scale, val, sub_t, inv);
#pragma unroll
                for (int c = 0; c < CO; ++c) e[c] = live ? smooth_grad(e[c], inv, c == tg, sub_t, sub_s[c]) : 0.f;
            } else if (FL) {
                const float vt = v[min(live ? tg : 0, CO - 1)];              // as ce_fused_body reads it; e_t = exp_nonpos(vt - m) has the bits of e[t]
                float fl, mod;
                focal_pixel(m, vt, exp_nonpos(vt - m), s, so, ce.gamma, fl, mod);
                const float sc = (wt_s[tg] * mod) * scale;
                const float inv = sc / s;
#pragma unroll
                for (int c = 0; c < CO; ++c) e[c] = live ? e[c] * inv - (c == tg ? sc : 0.f) : 0.f;
            } else if (DC) {
                // (weighted CE row) + (Dice row); a pixel whose label is >= CO takes no part in Dice and has weight 0 in the table
                const bool dlive = live && tg < CO;
                float inv_s, a_t, dot;
                dice_pixel<CO>(e, CO, s, tg, dlive, sub_s, sub_s + 32, inv_s, a_t, dot);
                const float sc = wt_s[tg];
                const float inv = sc / s;
#pragma unroll
                for (int c = 0; c < CO; ++c)
                    e[c] = live ? (e[c] * inv - (c == tg ? sc : 0.f)) + dice_grad(e[c], inv_s, sub_s[32 + c], c == tg, a_t, dot, dlive) : 0.f;
            } else if (LV) {
                // (weighted CE row) + (Lovasz row); a pixel whose label is >= CO takes no part in the term and has weight 0 in the table
                if constexpr (LV) {
                    const bool llive = live && tg < CO;
                    float inv_s, dot, g[CO];
                    lovasz_pixel<CO>(e, CO, s, tg, llive, ce.lovasz + kLovaszHeadFloats, ce.lovasz + kLovaszHeadFloats + CO * ce.bins, ce.bins, inv_s, g, dot);
                    const float sc = wt_s[tg];
                    const float inv = sc / s;
#pragma unroll
                    for (int c = 0; c < CO; ++c) e[c] = live ? (e[c] * inv - (c == tg ? sc : 0.f)) + lovasz_grad(e[c], inv_s, g[c], dot, llive) : 0.f;
                }
            } else if (RX) {
                if constexpr (RX) {
                    const unsigned S = relax_set(mword, tg, CO);
                    float mS, inv, invz, term;
                    relax_pixel<CO, false>(v, CO, S, m, s, wt_s[tg], mS, inv, invz, term);
#pragma unroll
                    for (int c = 0; c < CO; ++c) e[c] = live ? relax_grad(e[c], inv, (S >> c) & 1u, v[c], mS, invz) : 0.f;
                }
            } else if (CW) {
                // sc = table[target] is per lane where `scale` is uniform: held across the 19 operations beside inv it is one VGPR more than the
                // 768-thread build has (168, 2 spilled).  So it is read twice: for inv, and again - through a copy of the index the compiler cannot
                // match - once inv is dead.  Same operations and roundings: (e * inv) - sc
                const float inv = wt_s[tg] / s;
#pragma unroll
                for (int c = 0; c < CO; ++c) e[c] *= inv;
                int tg2 = tg;
                asm volatile("" : "+v"(tg2));
                const float sc = wt_s[tg2];
#pragma unroll
                for (int c = 0; c < CO; ++c) e[c] = live ? e[c] - (c == tg ? sc : 0.f) : 0.f;
            } else {
                const float inv = scale / s;
#pragma unroll
                for (int c = 0; c < CO; ++c) e[c] = live ? e[c] * inv - (c == tg ? scale : 0.f) : 0.f;
            }
            if (any_grid) {                                                 // wave-uniform: every eighth lane of every fourth row at stride 8
#pragma unroll
                for (int c = 0; c < CO; ++c) e[c] = on_u ? e[c] + g_u * ftw_s[c] : e[c];
            }
#pragma unroll
            for (int c = 0; c < CO; ++c) v[c] = e[c];
        }
    };

    // One set of persistent registers per wave: the dw waves' three accumulator tiles; in the dx waves the same registers hold the transposed filter,
    // the B operand of the dx GEMM (k = tap * CO + co, two per MFMA, n = ci) - declared once so that the two roles do not add up in the allocation.
    f32x16_t accw[NJ];
    static_assert(NK <= NJ * 16, "the filter fits the accumulator registers");
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) accw[j][e] = 0.f;
    if (wave < 4) {
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
            const int k = 2 * kk + lh, tap = k / CO, co = k - tap * CO;
            accw[kk / 16][kk % 16] = l31 < CI ? w[(l31 * CO + co) * 4 + tap] : 0.f;
        }
    }
    // word of column col = 32 j + l31 of the gradient matrix inside a stage, relative to the pixel's first word
    int colw[NJ];
    bool colok[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { const int col = 32 * j + l31; colok[j] = col < COLS; colw[j] = !colok[j] ? 0 : col < 2 * CO ? col : GW + col - 2 * CO; }
    const int xl = l31 < CI ? l31 : 0;
    const float aconst = l31 == CI ? 1.f : 0.f;

    // Schedule: at the barrier of iteration t segment t is ready to multiply (CE: transformed during iteration t - 1), segment t + 1 has LANDED (it
    // was issued during iteration t - 1 and the DMA waves drained their counters before the barrier), and the slot of segment t - 1 is free for
    // segment t + 2, issued right after the barrier.
    int seg = (int)blockIdx.x, t = 0;
    if (is_dw && seg < nseg) issue(seg, 0);
    if (CE) {
        if (is_dw) s_waitcnt_vm<0>();
        block_barrier();
        if (SM) {                                                          // the table is published: W, once per block, c ascending
#pragma unroll
            for (int c = 0; c < CO; ++c) Wsum += wt_s[c];
        }
        if ((is_tw || !TW) && seg < nseg) transform(seg, 0);
    }
    if (is_dw && seg + grid < nseg) issue(seg + grid, 1);
    for (; seg < nseg; seg += grid, ++t) {
        const int slot = t % S;
        if (is_dw) s_waitcnt_vm<0>();
        block_barrier();
        if (is_dw && seg + 2 * grid < nseg) issue(seg + 2 * grid, (t + 2) % S);
        const float* G = reinterpret_cast<const float*>(smem + slot * STAGE);
        const float* X = G + 2 * GW;
        const bool next = seg + grid < nseg;
        if (is_tw) {
            if (CE && next) transform(seg + grid, (t + 1) % S);
        } else if (!is_dw) {
            if (CE && !TW && next) transform(seg + grid, (t + 1) % S);
            // ---- dx tile of the wave's 32 pixels: A = gradients (row = pixel, two k per MFMA), B = transposed filter
            const int row = seg / nseg_per_row;
            const int w0 = (seg - row * nseg_per_row) * TP;
            f32x16_t acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            const float* g = G + (px0 + l31) * (2 * CO) + lh;
            constexpr int BK = TW ? 10 : 19, NBK = (NK + BK - 1) / BK;     // operand reads in batches; batch b + 1 is read while batch b multiplies
            float ga[2][BK];
            auto fetch = [&](int b, float (&a)[BK]) {
#pragma unroll
                for (int u = 0; u < BK; ++u) { const int kk = b * BK + u; if (kk < NK) a[u] = g[(kk < CO ? 0 : GW - 2 * CO) + 2 * kk]; }
            };
            fetch(0, ga[0]);
#pragma unroll
            for (int b = 0; b < NBK; ++b) {
                if (b + 1 < NBK) fetch(b + 1, ga[(b + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise re-serialises read -> wait -> two MFMAs through one register pair)
#pragma unroll
                for (int u = 0; u < BK; ++u) {
                    const int kk = b * BK + u;
                    if (kk < NK) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[b & 1][u], accw[kk / 16][kk % 16], acc, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (l31 < CI) {
                float* o = dx + ((long long)row * W + w0) * CI + l31;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int px = px0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    o[(long long)px * CI] = acc[e];
                }
            }
        } else {
            // ---- dw (+ db through the ones row): A = inputs transposed (row = ci, k = pixel), B = gradients (k = pixel, column = (tap, co))
            // unconditional reads (lanes past CI / past the last column fetch a valid word and drop it): no branches between the reads, so they are
            // issued ahead of the MFMAs that use them
            constexpr int HB = TW ? 2 : 4, NB = 16 / HB;   // pixel pairs per batch of operand reads; batch b + 1 is read while batch b multiplies
            float av[2][HB], bv[2][HB][NJ];
            auto fetch = [&](int b, float (&a)[HB], float (&v)[HB][NJ]) {
#pragma unroll
                for (int u = 0; u < HB; ++u) {
                    const int px = px0 + 2 * (b * HB + u) + lh;
                    a[u] = X[px * CI + xl];
#pragma unroll
                    for (int j = 0; j < NJ; ++j) v[u][j] = G[px * (2 * CO) + colw[j]];
                }
            };
            fetch(0, av[0], bv[0]);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (b + 1 < NB) fetch(b + 1, av[(b + 1) & 1], bv[(b + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < HB; ++u) {
                    const float a = l31 < CI ? av[b & 1][u] : aconst;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) accw[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, colok[j] ? bv[b & 1][u][j] : 0.f, accw[j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (CE && !TW && next) transform(seg + grid, (t + 1) % S);
        }
    }
    // ---- merge the four dw waves' tiles (fixed order) and leave the block's partials in the layout convt2x2_dw_finalize_kernel merges
    float* buf = reinterpret_cast<float*>(smem);
    float* xa = buf + 3 * NJ * 16 * 64;
    __syncthreads();
    if (is_dw && wq > 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) buf[(((wq - 1) * NJ + j) * 16 + e) * 64 + lane] = accw[j][e];
    }
    __syncthreads();
    if (is_dw && wq == 0) {
#pragma unroll 1
        for (int u = 0; u < 3; ++u)              // (one wave's tiles at a time: unrolled, the 144 reads in flight set the kernel's register count)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) accw[j][e] += buf[((u * NJ + j) * 16 + e) * 64 + lane];
#pragma unroll
        for (int j = 0; j < NJ; ++j)              // D[row = ci][col = (tap, co)] -> LDS as a dense [CI + 1][COLS] matrix
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ci = (e & 3) + 8 * (e >> 2) + 4 * lh, col = 32 * j + l31;
                if (ci <= CI && col < COLS) xa[ci * COLS + col] = accw[j][e];
            }
    }
    __syncthreads();
    float* po = part + (long long)blockIdx.x * (NOUT + CO);
    for (int o = tid; o < NOUT + CO; o += (int)blockDim.x) {
        float sum;
        if (o < NOUT) sum = xa[o];
        else {
            sum = 0.f;
#pragma unroll
            for (int ij = 0; ij < 4; ++ij) sum += xa[CI * COLS + ij * CO + (o - NOUT)];
        }
        po[o] = sum;
    }
}

// host side: supported = 19 -> 19 channels, W a multiple of the 128-pixel segment, 16-byte aligned tensors
bool convt_bwd_dma_supported(const void* x, const void* dy, int W, int Cin, int Cout) {
    if (!knob("DSRL_CONVT_DMA", 1)) return false;
    return Cin == 19 && Cout == 19 && W % 128 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0;
}
int convt_bwd_dma_blocks(long long nseg, int cap) { return (int)std::min<long long>(std::min(cap, kNumCU), nseg); }

template <bool CE, bool TW, bool CW = false, bool FL = false, bool SM = false, bool DC = false, bool LV = false, bool RX = false>
static int launch_dma(const float* x, const float* w, const float* dy, float* dx, float* part, int N, int H, int W, int nblocks, const ConvtCeArgs& ce, hipStream_t st,
                      const float* dice = nullptr, int bins = 0, const unsigned* mask = nullptr) {
    constexpr int CI = 19, CO = 19;
    constexpr int kLds = 3 * ((128 * CI * 4 + 1023) / 1024 + 2 * (2 * 128 * CO * 4 / 1024) + (CE ? 2 : 0)) * 1024;
    static_assert(kLds + (CW ? 1024 : 0) + (SM ? 128 : 0) + (DC ? 256 : 0) + 128 <= 160 * 1024,
                  "the ring, the transformer's weights, the class-weight tables and the Dice tables in LDS");
    static const hipError_t attr = hipFuncSetAttribute((const void*)convt2x2_bwd_dma_kernel<CI, CO, CE, TW, CW, FL, SM, DC, LV, RX>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    if (attr != hipSuccess) { set_error("convt2x2_bwd_dma_kernel: %d bytes of LDS refused (%s)", kLds, hipGetErrorString(attr)); return DSRL_E_LAUNCH; }
    const int nseg_per_row = W / 128;
    const long long nseg = (long long)N * H * nseg_per_row;
    if ((long long)N * 4 * H * W * CO * 4 >= (1ll << 32)) { set_error("convt2x2_bwd_dma_kernel: output gradient of 4 GB or more"); return DSRL_E_UNSUPPORTED; }
    if (nseg >= (1ll << 31) || nblocks < 1 || nblocks > nseg) { set_error("convt2x2_bwd_dma_kernel: %lld segments, %d blocks", nseg, nblocks); return DSRL_E_BADARG; }
    ConvtCeArgsOf<DC, LV, RX> args{};
    static_cast<ConvtCeArgs&>(args) = ce;
    if constexpr (DC) args.dice = dice;
    if constexpr (LV) { args.lovasz = dice; args.bins = bins; }
    if constexpr (RX) args.mask = mask;
    hipLaunchKernelGGL((convt2x2_bwd_dma_kernel<CI, CO, CE, TW, CW, FL, SM, DC, LV, RX>), dim3(nblocks), dim3(TW ? 768 : 512), kLds, st, x, w, dy, dx, part, N, H, W, nseg_per_row, (int)nseg, args);
    return launch_status("convt2x2_bwd_dma_kernel");
}
int launch_convt_bwd_dma(const float* x, const float* w, const float* dy, float* dx, float* part, int N, int H, int W, int nblocks, hipStream_t st) {
    return launch_dma<false, false>(x, w, dy, dx, part, N, H, W, nblocks, ConvtCeArgs{}, st);
}
int launch_convt_bwd_dma_ce(const float* x, const float* w, const float* logits, float* dx, float* part, int N, int H, int W, int nblocks,
                            const unsigned char* target, int ignore_index, const float* count, const float* ft_g, const float* ft_w, int ft_s,
                            const CeVariant& v, hipStream_t st) {
    ConvtCeArgs ce{};
    ce.target = target; ce.count = count; ce.ft_g = ft_g; ce.ft_w = ft_w; ce.ignore_index = ignore_index; ce.ft_s = ft_s > 0 ? ft_s : 1;
    ce.ft_shift = -1; ce.wtab = v.weights; ce.gamma = v.gamma; ce.eps = v.eps;
    for (int b = 0; b < 31; ++b) if (ce.ft_s == (1 << b)) ce.ft_shift = b;
    ce.Hf = (2 * H - 1) / ce.ft_s + 1; ce.Wf = (2 * W - 1) / ce.ft_s + 1;
    const bool w8 = knob("DSRL_CONVT_CE_WAVES", 12) == 8;                  // the transform inside the MFMA waves
    // focal: the 8-wave build whatever DSRL_CONVT_CE_WAVES says.  focal_pixel's log and two divisions beside the 19 terms need 172 VGPRs in the
    // 12-wave build, which has 168 (4 spilled, 20 B of scratch); the 8-wave build has 256 and takes 212
    if (v.kind == CeVariant::kFocal) return launch_dma<true, false, true, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st);
    // label smoothing: one wave build, the 8-wave one, as focal has
    if (v.kind == CeVariant::kSmoothed) return launch_dma<true, false, true, false, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st);
    // Dice: one wave build, the 8-wave one, as focal and label smoothing have.  The 12-wave build has 168 VGPRs and spills with focal already; the
    // Dice row keeps 1 / s, a_t and the class sum beside the 19 terms and the weighted row's inv and sc
    if (v.kind == CeVariant::kDice) return launch_dma<true, false, true, false, false, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st, v.dice);
    // Lovasz: the 8-wave build as well: 19 gathered coefficients beside the 19 terms
    if (v.kind == CeVariant::kLovasz)
        return launch_dma<true, false, true, false, false, false, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st, v.lovasz, v.bins);
    // label relaxation: the 8-wave build as well: m_S, inv, invz and the set word beside the 19 terms, and a second exponential per set class
    if (v.kind == CeVariant::kRelaxed)
        return launch_dma<true, false, true, false, false, false, false, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st, nullptr, 0, v.mask);
    if (v.kind == CeVariant::kWeighted) return w8 ? launch_dma<true, false, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st)
                        : launch_dma<true, true, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st);
    if (w8) return launch_dma<true, false>(x, w, logits, dx, part, N, H, W, nblocks, ce, st);
    return launch_dma<true, true>(x, w, logits, dx, part, N, H, W, nblocks, ce, st);
}

}  // namespace dsrl
