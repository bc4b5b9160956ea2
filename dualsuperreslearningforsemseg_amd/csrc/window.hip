// Sliding-window inference ensemble (include/dsrl_hip.h, "sliding-window ensemble"): what happens to a window's logits after the eval-mode forward
// path has written them.  A view is the (N,hw,ww,C) pixel-major logits of ONE window position, possibly in the horizontally mirrored frame; it sits at
// (oy, ox) on the (Ho,Wo) output grid and contributes softmax_c of its logits to the pixels it covers - no resampling.
//
//   dsrl_window_merge          one view of one position: acc <- p where the pixel is covered for the first time, acc <- acc + p elsewhere
//   dsrl_window_merge_finish   one pass over acc: tot = acc, cnt = cover count of the pixel, pred = first maximum of tot, ce = -log(tot[t] / cnt)
//
// Which pixels a launch stores and which it adds: window pixel (wy, wx) is STORED without reading acc iff wy >= fresh_y && wx >= fresh_x.  With the
// positions of a separable plan visited row-major, a pixel of window (i, j) was covered before iff it lies above row ys[i-1] + hw of the grid or left
// of column xs[j-1] + ww: the caller passes fresh_y = ys[i-1] + hw - ys[i] (0 for i = 0), likewise for x, and fresh_y = hw for a view that is never
// the first one of its pixels (the mirrored view of a position).  No zero fill of acc, whatever it held.
//
// Mapping (merge.hip's): a wave owns 64 consecutive pixels of ONE window row (spans; four consecutive ones per block and round), a lane one pixel with
// all C probabilities in registers.  The decomposition of the span index is wave-uniform; a lane divides nothing.  The span's logits are one
// contiguous run of memory (a mirrored span the run read backwards): lane i takes floats i, i + 64, .. into the wave's 9 KB of LDS, fully coalesced,
// and picks its own pixel from there (a pixel stride of 19 floats is conflict-free).  A pixel stride so wide that 64 pixels do not fit the stage
// (ld > 36) reads the lane's pixel from memory.  The accumulator is class-planar (N,C,Ho,Wo): per class the 64 lanes touch 256 consecutive bytes.  A
// pixel of acc belongs to one thread of a launch and is updated by a plain load and store; in the finish counters and confusion bins are 32-bit LDS
// tallies per block, then one 64-bit integer atomic per block and non-zero bin; the loss goes through per-block double partials in the workspace,
// reduced in block order: every output is bit-identical run to run.  No float atomics.  pred and target are accessed one byte per lane.
//
// The positions of the finish are HOST arrays copied into the kernel's argument struct (at most 32 per axis): no device table, no copy, capturable.
// The row's cover count is a wave-uniform loop, the column's a per-lane loop over uniform values.
#include "merge_common.h"
#include <limits.h>
#include <math.h>

namespace dsrl {

namespace {

constexpr int kWindowMaxPositions = 32;

struct WindowPlan {
    int ys[kWindowMaxPositions], xs[kWindowMaxPositions];
    int ny, nx, hw, ww;
};

// this wave's span of a (N, H, W) pixel grid in round `it`: image, row, the lane's column (clamped into the row), the span's first and last column
struct WindowSpan {
    int n, y, x, x_first, x_last;
    bool live;      // the wave has a span (wave-uniform)
    bool ok;        // the lane has a pixel
};
__device__ __forceinline__ WindowSpan window_span(int it, int wv, int nspans, int XC, int H, int W) {
    WindowSpan s;
    const int span = (it * (int)gridDim.x + (int)blockIdx.x) * 4 + wv;
    s.live = span < nspans;
    const int sp = s.live ? span : 0;
    const int row = sp / XC;                                 // wave-uniform
    s.n = row / H;
    s.y = row - s.n * H;
    s.x_first = (sp - row * XC) * 64;
    s.x_last = min(s.x_first + 63, W - 1);
    const int x = s.x_first + (int)(threadIdx.x & 63);
    s.ok = s.live && x < W;
    s.x = min(x, s.x_last);
    return s;
}

template <int CT>
__global__ __launch_bounds__(256) void window_merge_kernel(const float* __restrict__ logits, int ld, int hw, int ww, int C, int mirror,
                                                           float* __restrict__ acc, int Ho, int Wo, int oy, int ox, int fresh_y, int fresh_x, int nspans,
                                                           int XC, int rounds) {
    __shared__ float stage[4][kMergeStageFloats];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int plane = Ho * Wo;
    for (int it = 0; it < rounds; ++it) {
        const WindowSpan s = window_span(it, wv, nspans, XC, hw, ww);
        // the span covers window columns x_first .. x_last: in memory a run of ncol pixels from column lo on, the lane's own at offset c0
        const int ncol = s.x_last - s.x_first + 1;
        const int lo = mirror ? ww - 1 - s.x_last : s.x_first;
        const int c0 = mirror ? s.x_last - s.x : s.x - s.x_first;
        const float* run = logits + ((s.n * hw + s.y) * ww + lo) * ld;
        const int nfl = (ncol - 1) * ld + C;                     // floats of the run; the last pixel's padding is not the tensor's to read
        const bool staged = nfl <= kMergeStageFloats;            // wave-uniform
        if (s.live && staged)
            for (int i = (int)(threadIdx.x & 63); i < nfl; i += 64) stage[wv][i] = run[i];
        __syncthreads();
        float p[CT];
        float m = -INFINITY;
        if (s.live) {
            const float* q = (staged ? stage[wv] : run) + c0 * ld;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (CT == kMergeMaxC && c >= C) { p[c] = -INFINITY; continue; }
                p[c] = q[c];
                m = fmaxf(m, p[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < CT; ++c) p[c] = 0.f;
            m = 0.f;
        }
        __syncthreads();            // the next round overwrites the staged run
        merge_softmax<CT>(p, C, m);
        if (!s.ok) continue;
        float* a = acc + (s.n * C * Ho + oy + s.y) * Wo + ox + s.x;
        if (s.y >= fresh_y && s.x >= fresh_x) {                 // the first view to cover this pixel: what acc holds is not read
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

// One pass over acc.  target, counts, part (the loss), nan_flag and cm are nullable (counts, part and cm need a target).  CAL: the calibration record
// (common.h: CalBins, in LDS beside cmh; needs a target); CONF: the confidence map beside pred.  cnt = (positions covering the row) x (positions
// covering the column) x vpp; the confidence is min(1, winning sum / cnt) (confidence_views); a NaN pixel is in no bin and NaN in the map.
template <int CT, bool CAL, bool CONF>
__global__ __launch_bounds__(256) void window_finish_kernel(const float* __restrict__ acc, int C, int Ho, int Wo, WindowPlan plan, int vpp,
                                                            unsigned char* __restrict__ pred, const unsigned char* __restrict__ target, int ignore_index,
                                                            unsigned long long* __restrict__ counts, double* __restrict__ part,
                                                            int* __restrict__ nan_flag, unsigned long long* __restrict__ cm, int nspans, int XC, int rounds,
                                                            unsigned long long* __restrict__ cal, int B, float* __restrict__ conf) {
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
        const WindowSpan s = window_span(it, wv, nspans, XC, Ho, Wo);
        if (!s.ok) continue;
        int cy = 0, cx = 0;
        for (int i = 0; i < plan.ny; ++i) cy += (s.y >= plan.ys[i] && s.y < plan.ys[i] + plan.hw) ? 1 : 0;       // wave-uniform
        for (int j = 0; j < plan.nx; ++j) cx += (s.x >= plan.xs[j] && s.x < plan.xs[j] + plan.ww) ? 1 : 0;
        const float fcnt = (float)(cy * cx * vpp);
        const float* a = acc + (s.n * C * Ho + s.y) * Wo + s.x;
        float p[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) p[c] = (CT != kMergeMaxC || c < C) ? a[c * plane] : 0.f;
        const int pix = (s.n * Ho + s.y) * Wo + s.x;
        int best = 0;
        float bestv = p[0], total = p[0];
#pragma unroll
        for (int c = 1; c < CT; ++c) {
            if (CT == kMergeMaxC && c >= C) continue;
            if (p[c] > bestv) { bestv = p[c]; best = c; }           // first maximum, as prob_merge_finish_kernel and torch.argmax
            total += p[c];
        }
        bad |= !(total == total);               // a NaN logit of any covering view made every class of the pixel NaN
        pred[pix] = (unsigned char)best;
        float cf = 0.f;
        if (CAL || CONF) cf = confidence_views(bestv, fcnt);
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
                ce_loss += (double)(0.f - logf(pt / fcnt));     // -log P[t]; cnt = 1 gives the bits of a single view of prob_merge_finish_kernel
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
        if (bad_label) ce_loss = __builtin_nan("");     // as prob_merge_finish_kernel
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

// every 32-bit index of the launches (the span index runs to the end of the last round: < nspans + 4 * kMergeMaxBlocks)
bool window_indices_fit(int N, int hw, int ww, int ld, int Ho, int Wo, int C) {
    const long long lim = INT_MAX;
    return (long long)N * Ho * Wo * C <= lim && (long long)N * hw * ww * ld <= lim &&
           (long long)N * Ho * merge_spans_per_row(Wo) + 4LL * kMergeMaxBlocks <= lim;
}

// positions along one axis of S grid pixels, window side w: 1 .. 32 of them, strictly increasing from 0, no gap, the last one ending at S
bool axis_covers(const int* a, int n, int w, int S) {
    if (a == nullptr || n < 1 || n > kWindowMaxPositions || w < 1 || a[0] != 0) return false;
    for (int i = 1; i < n; ++i)
        if (a[i] <= a[i - 1] || a[i] > a[i - 1] + w) return false;
    return (long long)a[n - 1] + w == S;
}

int window_finish_launch(const float* acc, int N, int C, int Ho, int Wo, const int* ys, int ny, const int* xs, int nx, int hw, int ww, int vpp,
                         uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts, float* ce_out, int* nan_flag, void* ws,
                         size_t ws_bytes, unsigned long long* cm, unsigned long long* cal, int bins, float* conf, dsrl_stream_t stream) {
    DSRL_REQUIRE(acc && pred && N > 0 && Ho > 0 && Wo > 0 && hw > 0 && ww > 0 && vpp >= 1, DSRL_E_BADARG,
                 "window_merge_finish: null acc or pred, an empty shape, or views_per_position < 1");
    DSRL_REQUIRE(axis_covers(ys, ny, hw, Ho) && axis_covers(xs, nx, ww, Wo), DSRL_E_BADARG,
                 "window_merge_finish: the positions (%d x %d of a %d x %d window) must be 1 to %d per axis, increasing from 0, and cover the %d x %d grid "
                 "without a gap", ny, nx, hw, ww, kWindowMaxPositions, Ho, Wo);
    DSRL_REQUIRE(dsrl_window_merge_supported(N, hw, ww, Ho, Wo, C), DSRL_E_UNSUPPORTED,
                 "window_merge_finish: needs 1 <= C <= %d and 32-bit indices (got C = %d, %d x %d x %d)", kMergeMaxC, C, N, Ho, Wo);
    DSRL_REQUIRE((long long)ny * nx * vpp < (1 << 24), DSRL_E_BADARG, "window_merge_finish: %d x %d positions of %d views", ny, nx, vpp);
    DSRL_REQUIRE(((uintptr_t)acc % 4) == 0 && ((uintptr_t)conf % 4) == 0, DSRL_E_BADARG, "window_merge_finish: acc or conf not 4-byte aligned");
    DSRL_REQUIRE(target || (!counts && !ce_out && !cm && !cal), DSRL_E_BADARG, "window_merge_finish: counts / ce_out / cm / cal need a target");
    DSRL_REQUIRE(!cal || (bins >= 1 && bins <= kCalMaxBins && ((uintptr_t)cal % 8) == 0), DSRL_E_BADARG,
                 "window_merge_finish: %d calibration bins (1 to %d are possible), or cal not 8-byte aligned", bins, kCalMaxBins);
    DSRL_REQUIRE(!ce_out || (ws && ws_bytes >= dsrl_window_merge_workspace_bytes(N, Ho, Wo) && ((uintptr_t)ws % 8) == 0), DSRL_E_WORKSPACE,
                 "window_merge_finish: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    WindowPlan plan;
    for (int i = 0; i < kWindowMaxPositions; ++i) { plan.ys[i] = i < ny ? ys[i] : 0; plan.xs[i] = i < nx ? xs[i] : 0; }
    plan.ny = ny; plan.nx = nx; plan.hw = hw; plan.ww = ww;
    const int nb = merge_blocks(N, Ho, Wo), XC = merge_spans_per_row(Wo), nspans = N * Ho * XC, rounds = (int)ceil_div(nspans, 4LL * nb);
    double* part = ce_out ? (double*)ws : nullptr;
#define DSRL_WINDOW_FINISH(CT, CAL, CONF)                                                                                                              \
    hipLaunchKernelGGL((window_finish_kernel<CT, CAL, CONF>), dim3(nb), dim3(256), 0, st, acc, C, Ho, Wo, plan, vpp, pred, target, ignore_index, counts, \
                       part, nan_flag, cm, nspans, XC, rounds, cal, bins, conf)
#define DSRL_WINDOW_FINISH_CT(CT)                                       \
    do {                                                                \
        if (cal && conf) DSRL_WINDOW_FINISH(CT, true, true);            \
        else if (cal) DSRL_WINDOW_FINISH(CT, true, false);              \
        else if (conf) DSRL_WINDOW_FINISH(CT, false, true);             \
        else DSRL_WINDOW_FINISH(CT, false, false);                      \
    } while (0)
    if (C == 19) DSRL_WINDOW_FINISH_CT(19);
    else DSRL_WINDOW_FINISH_CT(kMergeMaxC);
#undef DSRL_WINDOW_FINISH_CT
#undef DSRL_WINDOW_FINISH
    if (int e = launch_status("window_finish_kernel")) return e;
    if (ce_out) return launch_merge_ce_finalize(part, nb, ce_out, st);
    return DSRL_OK;
}

}  // namespace

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_window_merge_supported(int N, int hw, int ww, int Ho, int Wo, int C) {
    if (N < 1 || hw < 1 || ww < 1 || Ho < hw || Wo < ww || C < 1 || C > kMergeMaxC || C > dsrl_confusion_matrix_max_classes()) return 0;
    return window_indices_fit(N, hw, ww, C, Ho, Wo, C) ? 1 : 0;
}

extern "C" size_t dsrl_window_merge_workspace_bytes(int N, int Ho, int Wo) {
    if (N < 1 || Ho < 1 || Wo < 1) return 0;
    return (size_t)2 * merge_blocks(N, Ho, Wo) * sizeof(double);
}

extern "C" int dsrl_window_merge(const float* logits, int ld, int N, int hw, int ww, int C, int mirror, float* acc, int Ho, int Wo, int oy, int ox,
                                 int fresh_y, int fresh_x, dsrl_stream_t stream) {
    DSRL_REQUIRE(logits && acc && N > 0 && hw > 0 && ww > 0 && Ho > 0 && Wo > 0, DSRL_E_BADARG, "window_merge: null pointer or empty shape");
    DSRL_REQUIRE(oy >= 0 && ox >= 0 && (long long)oy + hw <= Ho && (long long)ox + ww <= Wo, DSRL_E_BADARG,
                 "window_merge: a %d x %d window at (%d, %d) leaves the %d x %d grid", hw, ww, oy, ox, Ho, Wo);
    DSRL_REQUIRE(fresh_y >= 0 && fresh_y <= hw && fresh_x >= 0 && fresh_x <= ww, DSRL_E_BADARG,
                 "window_merge: fresh_y = %d, fresh_x = %d are not inside the %d x %d window", fresh_y, fresh_x, hw, ww);
    DSRL_REQUIRE(dsrl_window_merge_supported(N, hw, ww, Ho, Wo, C), DSRL_E_UNSUPPORTED,
                 "window_merge: needs 1 <= C <= %d and 32-bit indices (got C = %d, %d x %d x %d on %d x %d)", kMergeMaxC, C, N, hw, ww, Ho, Wo);
    DSRL_REQUIRE(ld >= C && ((uintptr_t)logits % 4) == 0 && ((uintptr_t)acc % 4) == 0, DSRL_E_BADARG,
                 "window_merge: ld < C, or logits / acc not 4-byte aligned");
    DSRL_REQUIRE(window_indices_fit(N, hw, ww, ld, Ho, Wo, C), DSRL_E_UNSUPPORTED, "window_merge: N*hw*ww*ld = %lld does not fit 32 bits",
                 (long long)N * hw * ww * ld);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int XC = merge_spans_per_row(ww), nspans = N * hw * XC, nb = merge_blocks(N, hw, ww), rounds = (int)ceil_div(nspans, 4LL * nb);
    if (C == 19)
        hipLaunchKernelGGL(window_merge_kernel<19>, dim3(nb), dim3(256), 0, st, logits, ld, hw, ww, C, mirror, acc, Ho, Wo, oy, ox, fresh_y, fresh_x,
                           nspans, XC, rounds);
    else
        hipLaunchKernelGGL(window_merge_kernel<kMergeMaxC>, dim3(nb), dim3(256), 0, st, logits, ld, hw, ww, C, mirror, acc, Ho, Wo, oy, ox, fresh_y,
                           fresh_x, nspans, XC, rounds);
    return launch_status("window_merge_kernel");
}

extern "C" int dsrl_window_merge_finish(const float* acc, int N, int C, int Ho, int Wo, const int* ys, int ny, const int* xs, int nx, int hw, int ww,
                                        int views_per_position, uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts,
                                        float* ce_out, int* nan_flag, void* ws, size_t ws_bytes, unsigned long long* cm, dsrl_stream_t stream) {
    return window_finish_launch(acc, N, C, Ho, Wo, ys, ny, xs, nx, hw, ww, views_per_position, pred, target, ignore_index, counts, ce_out, nan_flag, ws,
                                ws_bytes, cm, nullptr, 0, nullptr, stream);
}

// the same launch with every optional output: cal (the calibration record, int64 [3 * bins], ADDED; needs a target) and conf (the confidence map
// (N,Ho,Wo) fp32) are nullable; with both null this is dsrl_window_merge_finish
extern "C" int dsrl_window_merge_finish_ex(const float* acc, int N, int C, int Ho, int Wo, const int* ys, int ny, const int* xs, int nx, int hw, int ww,
                                           int views_per_position, uint8_t* pred, const uint8_t* target, int ignore_index, unsigned long long* counts,
                                           float* ce_out, int* nan_flag, void* ws, size_t ws_bytes, unsigned long long* cm, unsigned long long* cal,
                                           int bins, float* conf, dsrl_stream_t stream) {
    return window_finish_launch(acc, N, C, Ho, Wo, ys, ny, xs, nx, hw, ww, views_per_position, pred, target, ignore_index, counts, ce_out, nan_flag, ws,
                                ws_bytes, cm, cal, bins, conf, stream);
}
