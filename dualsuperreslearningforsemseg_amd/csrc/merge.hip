// Multi-scale (and flip) inference ensemble: what happens to the views' logits after the eval-mode forward path has written them (include/dsrl_hip.h,
// "multi-scale ensemble").  A view is the (N,Hs,Ws,C) pixel-major logits of one scale, possibly in the horizontally mirrored frame.  Per output pixel
// of the (Ho,Wo) grid a view contributes softmax_c of its align-corners bilinear resample; the contributions are summed over the views in an
// accumulator the kernels own, and the launch of the LAST view ends in the class map, the validation counters, the loss and the confusion matrix.
//
//   dsrl_prob_merge         one view that is not the last: acc <- p (first) or acc <- acc + p
//   dsrl_prob_merge_finish  the last view: tot = acc + p in registers (acc is not written), pred = first maximum of tot, ce = -log(tot[t] / V)
//
// Source coordinate of output index o on an axis of S source and O output samples, exact in 32-bit integers: n = o (S - 1), i0 = n / (O - 1),
// frac = float(n mod (O - 1)) / float(O - 1), i1 = min(i0 + 1, S - 1); O = 1: i0 = 0, frac = 0.  Both integers are exact, so the weight carries ONE
// rounding at every size (dsrl_bilinear_ac_fwd evaluates scale * dst in fp32, whose error grows with the coordinate).  A mirrored view is mirrored back
// first: its source columns are Ws - 1 - i0 and Ws - 1 - i1 under the same weights.
//
// Mapping: a wave owns 64 consecutive pixels of ONE output row (spans; N * Ho * ceil(Wo / 64) of them, four consecutive ones per block and round), a
// lane one pixel with all C probabilities in registers.  The row coordinate and the decomposition of the span index are wave-uniform; a lane divides
// once, for its column.  The two source rows of a span are blended FIRST, (1 - fy) r0 + fy r1, over the contiguous run of source columns the span
// reads, by fully coalesced loads (lane i takes floats i, i + 64, ..: the logits are pixel-major, a lane's own 4 x C floats would be C-strided
// gathers), into the wave's 9 KB of LDS; a lane then blends its two columns, (1 - fx) s0 + fx s1, from there (a pixel stride of 19 floats is
// conflict-free).  Spans whose run does not fit (a view more than ~1.9 x the output width) read the four pixels from memory, same arithmetic.
// The accumulator is class-planar (N,C,Ho,Wo): for each class the 64 lanes read and write 256 consecutive bytes.  A pixel of the accumulator belongs
// to one thread and is updated by a plain load and store; counters and confusion bins are 32-bit LDS tallies per block, then one 64-bit integer atomic
// per block and non-zero bin; the loss goes through per-block double partials in the workspace, reduced in block order: every output is bit-identical
// run to run.  No float atomics.  pred and target are accessed one byte per lane: any base address and any Wo work.
//
// fp32 limit of ce: it is the logarithm of the ACCUMULATED probability.  Where the probability of the target underflows fp32 in every view (a logit gap
// above about 87) the pixel's term, and with it ce, is +inf - the value fp32 gives - while a gap of 60 (p = 9e-27) is exact to an ulp of the logarithm.
#include "merge_common.h"
#include <limits.h>
#include <math.h>

namespace dsrl {

namespace {

// i0, i1, frac of output index o (see the header comment)
__device__ __forceinline__ void merge_coord(int o, int S, int O, int& i0, int& i1, float& frac) {
    if (O > 1) {
        const int n = o * (S - 1);
        i0 = n / (O - 1);
        frac = (float)(n - i0 * (O - 1)) / (float)(O - 1);
    } else {
        i0 = 0;
        frac = 0.f;
    }
    i1 = min(i0 + 1, S - 1);
}

// this wave's span in round `it`: image, row, the lane's column (clamped into the row) and the span's first and last column
struct MergeSpan {
    int n, oy, ox, ox_first, ox_last;
    bool live;      // the wave has a span (wave-uniform)
    bool ok;        // the lane has a pixel
};
__device__ __forceinline__ MergeSpan merge_span(int it, int wv, int nspans, int XC, int Ho, int Wo) {
    MergeSpan s;
    const int span = (it * (int)gridDim.x + (int)blockIdx.x) * 4 + wv;
    s.live = span < nspans;
    const int sp = s.live ? span : 0;
    const int row = sp / XC;                                 // wave-uniform
    s.n = row / Ho;
    s.oy = row - s.n * Ho;
    s.ox_first = (sp - row * XC) * 64;
    s.ox_last = min(s.ox_first + 63, Wo - 1);
    const int ox = s.ox_first + (int)(threadIdx.x & 63);
    s.ok = s.live && ox < Wo;
    s.ox = min(ox, s.ox_last);
    return s;
}

// The resample and the softmax of one span of one view -> the lane's p[c] for c < C (the rest 0).  The one function both entry points go through: a
// view contributes the same bits whether it is merged first, in the middle or last.  EVERY thread of the block calls it in every round (it
// synchronises the block around the staged rows); a wave without a span passes live = false and gets zeros.  Blend: (1 - fy) r0 + fy r1 per source
// pixel, then (1 - fx) s0 + fx s1 (the library is built with -ffp-contract=off); an identity view (frac = 0) returns its logits exactly.  A NaN among
// the four sampled pixels makes every p[c] NaN (0 * NaN included): the accumulator carries it to the last view's launch, which raises the flag.
template <int CT>
__device__ __forceinline__ void merge_pixel(const float* __restrict__ logits, int ld, int Hs, int Ws, int C, int mirror, const MergeSpan& s, int Ho, int Wo,
                                            float* __restrict__ stage, float (&p)[CT]) {
    int y0, y1, x0, x1, a0, a1, b0, b1;
    float fy, fx, unused;
    merge_coord(s.oy, Hs, Ho, y0, y1, fy);
    merge_coord(s.ox, Ws, Wo, x0, x1, fx);
    merge_coord(s.ox_first, Ws, Wo, a0, a1, unused);
    merge_coord(s.ox_last, Ws, Wo, b0, b1, unused);
    // the span reads columns a0 .. b1 of the un-mirrored frame: in memory a run of ncol pixels from column lo on, the lane's two at offsets c0 and c1
    const int ncol = b1 - a0 + 1;
    const int lo = mirror ? Ws - 1 - b1 : a0;
    const int c0 = mirror ? b1 - x0 : x0 - a0, c1 = mirror ? b1 - x1 : x1 - a0;
    const float* r0 = logits + ((s.n * Hs + y0) * Ws + lo) * ld;
    const float* r1 = logits + ((s.n * Hs + y1) * Ws + lo) * ld;
    const float gx = 1.f - fx, gy = 1.f - fy;
    const int nfl = (ncol - 1) * ld + C;                     // floats of the run; the last pixel's padding is not the tensor's to read
    const bool staged = nfl <= kMergeStageFloats;            // wave-uniform
    if (s.live && staged)
        for (int i = (int)(threadIdx.x & 63); i < nfl; i += 64) stage[i] = gy * r0[i] + fy * r1[i];
    __syncthreads();
    float m = -INFINITY;
    if (s.live) {
        if (staged) {
            const float* s0 = stage + c0 * ld;
            const float* s1 = stage + c1 * ld;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (CT == kMergeMaxC && c >= C) { p[c] = -INFINITY; continue; }
                p[c] = gx * s0[c] + fx * s1[c];
                m = fmaxf(m, p[c]);
            }
        } else {
            const float *q00 = r0 + c0 * ld, *q01 = r0 + c1 * ld, *q10 = r1 + c0 * ld, *q11 = r1 + c1 * ld;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (CT == kMergeMaxC && c >= C) { p[c] = -INFINITY; continue; }
                const float v0 = gy * q00[c] + fy * q10[c];
                const float v1 = gy * q01[c] + fy * q11[c];
                p[c] = gx * v0 + fx * v1;
                m = fmaxf(m, p[c]);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) p[c] = 0.f;
        m = 0.f;
    }
    __syncthreads();            // the next round overwrites the staged rows
    merge_softmax<CT>(p, C, m);         // merge_common.h: the sliding-window ensemble takes the same softmax
}

template <int CT>
__global__ __launch_bounds__(256) void prob_merge_kernel(const float* __restrict__ logits, int ld, int Hs, int Ws, int C, int mirror,
                                                         float* __restrict__ acc, int Ho, int Wo, int first, int nspans, int XC, int rounds) {
    __shared__ float stage[4][kMergeStageFloats];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int plane = Ho * Wo;
    for (int it = 0; it < rounds; ++it) {
        const MergeSpan s = merge_span(it, wv, nspans, XC, Ho, Wo);
        float p[CT];
        merge_pixel<CT>(logits, ld, Hs, Ws, C, mirror, s, Ho, Wo, stage[wv], p);
        if (!s.ok) continue;
        float* a = acc + (s.n * C * Ho + s.oy) * Wo + s.ox;
        if (first) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (CT != kMergeMaxC || c < C) a[c * plane] = p[c];
        } else {
            float old[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) old[c] = (CT != kMergeMaxC || c < C) ? a[c * plane] : 0.f;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (CT != kMergeMaxC || c < C) a[c * plane] = old[c] + p[c];
        }
    }
}

// The last view.  target, counts, part (the loss), nan_flag and cm are nullable (counts, part and cm need a target); lnV = ln(views).
// CAL: the calibration record (common.h: CalBins, in LDS beside cmh; needs a target); CONF: the confidence map beside pred, one float per lane.  The
// confidence is min(1, winning sum / views) (confidence_views); a NaN pixel is in no bin and NaN in the map.
template <int CT, bool CAL = false, bool CONF = false>
__global__ __launch_bounds__(256) void prob_merge_finish_kernel(const float* __restrict__ logits, int ld, int Hs, int Ws, int C, int mirror,
                                                                const float* __restrict__ acc, int Ho, int Wo, float lnV,
                                                                unsigned char* __restrict__ pred, const unsigned char* __restrict__ target,
                                                                int ignore_index, unsigned long long* __restrict__ counts, double* __restrict__ part,
                                                                int* __restrict__ nan_flag, unsigned long long* __restrict__ cm, int nspans, int XC,
                                                                int rounds, float fV, unsigned long long* __restrict__ cal, int B,
                                                                float* __restrict__ conf) {
    __shared__ float stage[4][kMergeStageFloats];
    __shared__ unsigned hist[3 * kMergeMaxC + 2];
    __shared__ unsigned cmh[kMergeMaxC * kMergeMaxC];          // cmh[t * C + p]
    __shared__ double shd[4];
    __shared__ unsigned long long calraw[CAL ? sizeof(CalBins) / 8 : 1];
    CalBins& calb = *reinterpret_cast<CalBins*>(calraw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (CAL) calb.clear(B);         // CAL comes with a target: the barrier below covers it
    if (target != nullptr) {
        for (int t = tid; t < 3 * C + 2; t += 256) hist[t] = 0u;
        if (cm != nullptr)
            for (int t = tid; t < C * C; t += 256) cmh[t] = 0u;
        __syncthreads();
    }
    const int plane = Ho * Wo;
    double ce_loss = 0.0, ce_cnt = 0.0;
    bool bad = false, bad_label = false;
    for (int it = 0; it < rounds; ++it) {
        const MergeSpan s = merge_span(it, wv, nspans, XC, Ho, Wo);
        float p[CT];
        merge_pixel<CT>(logits, ld, Hs, Ws, C, mirror, s, Ho, Wo, stage[wv], p);
        if (!s.ok) continue;
        if (acc != nullptr) {
            const float* a = acc + (s.n * C * Ho + s.oy) * Wo + s.ox;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (CT != kMergeMaxC || c < C) p[c] = a[c * plane] + p[c];
        }
        const int pix = (s.n * Ho + s.oy) * Wo + s.ox;
        int best = 0;
        float bestv = p[0], total = p[0];
#pragma unroll
        for (int c = 1; c < CT; ++c) {
            if (CT == kMergeMaxC && c >= C) continue;
            if (p[c] > bestv) { bestv = p[c]; best = c; }           // first maximum, as seg_metrics_kernel and torch.argmax
            total += p[c];
        }
        bad |= !(total == total);               // a NaN logit of any view made every class of the pixel NaN
        pred[pix] = (unsigned char)best;
        float cf = 0.f;
        if (CAL || CONF) cf = confidence_views(bestv, fV);
        if (CONF) conf[pix] = cf;
        if (target != nullptr) {
            const int tg = (int)target[pix];
            const bool counted = tg != ignore_index && tg < C;
            if (CAL && counted) calb.count(cf, best == tg, B);
            bad_label |= tg != ignore_index && tg >= C;
            if (counts != nullptr && counted) {
                atomicAdd(&hist[best], 1u);
                atomicAdd(&hist[2 * C + tg], 1u);
                atomicAdd(&hist[3 * C + 1], 1u);
                if (best == tg) { atomicAdd(&hist[C + tg], 1u); atomicAdd(&hist[3 * C], 1u); }
            }
            if (cm != nullptr && counted) atomicAdd(&cmh[tg * C + best], 1u);
            if (part != nullptr && tg != ignore_index) {
                const int ts = min(tg, C - 1);
                float pt = p[0];
#pragma unroll
                for (int c = 1; c < CT; ++c) pt = (c == ts) ? p[c] : pt;
                ce_loss += (double)(lnV - logf(pt));            // -log(pt / V)
                ce_cnt += 1.0;
            }
        }
    }
    if (nan_flag != nullptr && __any(bad) && lane == 0) atomicOr(nan_flag, 1);
    if (target != nullptr && nan_flag != nullptr && __any(bad_label) && lane == 0) atomicOr(nan_flag, 2);
    if (target != nullptr) {
        __syncthreads();
        if (counts != nullptr)
            for (int t = tid; t < 3 * C + 2; t += 256)
                if (hist[t]) atomicAdd(&counts[t], (unsigned long long)hist[t]);
        if (cm != nullptr)
            for (int t = tid; t < C * C; t += 256)
                if (cmh[t]) atomicAdd(&cm[t], (unsigned long long)cmh[t]);
        if (CAL) calb.flush(cal, B);
    }
    if (part != nullptr) {
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
__global__ __launch_bounds__(256) void prob_merge_ce_finalize_kernel(const double* __restrict__ part, int nb, float* __restrict__ out) {
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

// every 32-bit index of a launch with pixel stride ld (the span index runs to the end of the last round: < nspans + 4 * kMergeMaxBlocks)
bool merge_indices_fit(int N, int Hs, int Ws, int ld, int Ho, int Wo, int C) {
    const long long lim = INT_MAX;
    return (long long)N * Ho * Wo * C <= lim && (long long)N * Hs * Ws * ld <= lim && (long long)(Ho - 1) * (Hs - 1) <= lim &&
           (long long)(Wo - 1) * (Ws - 1) <= lim && (long long)N * Ho * merge_spans_per_row(Wo) + 4LL * kMergeMaxBlocks <= lim;
}

int merge_check(const char* what, const float* logits, int ld, int N, int Hs, int Ws, int C, int Ho, int Wo) {
    DSRL_REQUIRE(logits && N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, DSRL_E_BADARG, "%s: null pointer or empty shape", what);
    DSRL_REQUIRE(dsrl_prob_merge_supported(N, Hs, Ws, Ho, Wo, C), DSRL_E_UNSUPPORTED,
                 "%s: needs 1 <= C <= %d and 32-bit indices (got C = %d, %d x %d x %d -> %d x %d)", what, kMergeMaxC, C, N, Hs, Ws, Ho, Wo);
    DSRL_REQUIRE(ld >= C && ((uintptr_t)logits % 4) == 0, DSRL_E_BADARG, "%s: ld < C, or logits not 4-byte aligned", what);
    DSRL_REQUIRE(merge_indices_fit(N, Hs, Ws, ld, Ho, Wo, C), DSRL_E_UNSUPPORTED, "%s: N*Hs*Ws*ld = %lld does not fit 32 bits", what,
                 (long long)N * Hs * Ws * ld);
    return DSRL_OK;
}

}  // namespace

int launch_merge_ce_finalize(const double* part, int nb, float* out, hipStream_t st) {
    hipLaunchKernelGGL(prob_merge_ce_finalize_kernel, dim3(1), dim3(256), 0, st, part, nb, out);
    return launch_status("prob_merge_ce_finalize_kernel");
}

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_prob_merge_supported(int N, int Hs, int Ws, int Ho, int Wo, int C) {
    if (N < 1 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || C < 1 || C > kMergeMaxC || C > dsrl_confusion_matrix_max_classes()) return 0;
    return merge_indices_fit(N, Hs, Ws, C, Ho, Wo, C) ? 1 : 0;
}

extern "C" size_t dsrl_prob_merge_acc_bytes(int N, int Ho, int Wo, int C) {
    if (N < 1 || Ho < 1 || Wo < 1 || C < 1) return 0;
    return (size_t)N * C * Ho * Wo * sizeof(float);
}

extern "C" size_t dsrl_prob_merge_workspace_bytes(int N, int Ho, int Wo) {
    if (N < 1 || Ho < 1 || Wo < 1) return 0;
    return (size_t)2 * merge_blocks(N, Ho, Wo) * sizeof(double);
}

extern "C" int dsrl_prob_merge(const float* logits, int ld, int N, int Hs, int Ws, int C, int mirror, float* acc, int Ho, int Wo, int first,
                               dsrl_stream_t stream) {
    if (int e = merge_check("prob_merge", logits, ld, N, Hs, Ws, C, Ho, Wo)) return e;
    DSRL_REQUIRE(acc && ((uintptr_t)acc % 4) == 0, DSRL_E_BADARG, "prob_merge: acc null or not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int XC = merge_spans_per_row(Wo), nspans = N * Ho * XC, nb = merge_blocks(N, Ho, Wo), rounds = (int)ceil_div(nspans, 4LL * nb);
    if (C == 19)
        hipLaunchKernelGGL(prob_merge_kernel<19>, dim3(nb), dim3(256), 0, st, logits, ld, Hs, Ws, C, mirror, acc, Ho, Wo, first, nspans, XC, rounds);
    else
        hipLaunchKernelGGL(prob_merge_kernel<kMergeMaxC>, dim3(nb), dim3(256), 0, st, logits, ld, Hs, Ws, C, mirror, acc, Ho, Wo, first, nspans, XC,
                           rounds);
    return launch_status("prob_merge_kernel");
}

namespace {

int merge_finish_launch(const float* logits, int ld, int N, int Hs, int Ws, int C, int mirror, const float* acc, int Ho, int Wo, int views, uint8_t* pred,
                        const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws, size_t ws_bytes,
                        unsigned long long* cm, unsigned long long* cal, int bins, float* conf, dsrl_stream_t stream) {
    if (int e = merge_check("prob_merge_finish", logits, ld, N, Hs, Ws, C, Ho, Wo)) return e;
    DSRL_REQUIRE(pred && views >= 1 && ((uintptr_t)acc % 4) == 0, DSRL_E_BADARG, "prob_merge_finish: null pred, views < 1, or acc not 4-byte aligned");
    DSRL_REQUIRE((acc != nullptr) == (views > 1), DSRL_E_BADARG, "prob_merge_finish: acc must be given exactly when there are earlier views (views = %d)",
                 views);
    DSRL_REQUIRE(target || (!counts && !ce_out && !cm && !cal), DSRL_E_BADARG, "prob_merge_finish: counts / ce_out / cm / cal need a target");
    DSRL_REQUIRE(!cal || (bins >= 1 && bins <= kCalMaxBins && ((uintptr_t)cal % 8) == 0), DSRL_E_BADARG,
                 "prob_merge_finish: %d calibration bins (1 to %d are possible), or cal not 8-byte aligned", bins, kCalMaxBins);
    DSRL_REQUIRE(((uintptr_t)conf % 4) == 0, DSRL_E_BADARG, "prob_merge_finish: conf not 4-byte aligned");
    const int nb = merge_blocks(N, Ho, Wo);
    DSRL_REQUIRE(!ce_out || (ws && ws_bytes >= dsrl_prob_merge_workspace_bytes(N, Ho, Wo) && ((uintptr_t)ws % 8) == 0), DSRL_E_WORKSPACE,
                 "prob_merge_finish: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int XC = merge_spans_per_row(Wo), nspans = N * Ho * XC, rounds = (int)ceil_div(nspans, 4LL * nb);
    double* part = ce_out ? (double*)ws : nullptr;
    const float lnV = (float)log((double)views), fV = (float)views;
#define DSRL_MERGE_FINISH(CT, CAL, CONF)                                                                                                                  \
    hipLaunchKernelGGL((prob_merge_finish_kernel<CT, CAL, CONF>), dim3(nb), dim3(256), 0, st, logits, ld, Hs, Ws, C, mirror, acc, Ho, Wo, lnV, pred, target, \
                       ignore_index, counts, part, nan_flag, cm, nspans, XC, rounds, fV, cal, bins, conf)
#define DSRL_MERGE_FINISH_CT(CT)                                        \
    do {                                                                \
        if (cal && conf) DSRL_MERGE_FINISH(CT, true, true);             \
        else if (cal) DSRL_MERGE_FINISH(CT, true, false);               \
        else if (conf) DSRL_MERGE_FINISH(CT, false, true);              \
        else DSRL_MERGE_FINISH(CT, false, false);                       \
    } while (0)
    if (C == 19) DSRL_MERGE_FINISH_CT(19);
    else DSRL_MERGE_FINISH_CT(kMergeMaxC);
#undef DSRL_MERGE_FINISH_CT
#undef DSRL_MERGE_FINISH
    if (int e = launch_status("prob_merge_finish_kernel")) return e;
    if (ce_out) return launch_merge_ce_finalize(part, nb, ce_out, st);
    return DSRL_OK;
}

}  // namespace

extern "C" int dsrl_prob_merge_finish(const float* logits, int ld, int N, int Hs, int Ws, int C, int mirror, const float* acc, int Ho, int Wo, int views,
                                      uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag,
                                      void* ws, size_t ws_bytes, unsigned long long* cm, dsrl_stream_t stream) {
    return merge_finish_launch(logits, ld, N, Hs, Ws, C, mirror, acc, Ho, Wo, views, pred, target, ignore_index, counts, ce_out, nan_flag, ws, ws_bytes, cm,
                               nullptr, 0, nullptr, stream);
}

// the same launch with every optional output: cal (the calibration record, int64 [3 * bins], ADDED; needs a target) and conf (the confidence map
// (N,Ho,Wo) fp32) are nullable; with both null this is dsrl_prob_merge_finish
extern "C" int dsrl_prob_merge_finish_ex(const float* logits, int ld, int N, int Hs, int Ws, int C, int mirror, const float* acc, int Ho, int Wo, int views,
                                         uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag,
                                         void* ws, size_t ws_bytes, unsigned long long* cm, unsigned long long* cal, int bins, float* conf,
                                         dsrl_stream_t stream) {
    return merge_finish_launch(logits, ld, N, Hs, Ws, C, mirror, acc, Ho, Wo, views, pred, target, ignore_index, counts, ce_out, nan_flag, ws, ws_bytes, cm,
                               cal, bins, conf, stream);
}
