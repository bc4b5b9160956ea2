// Lovasz-Softmax loss term beside the cross entropy (Berman et al., CVPR 2018), in its QUANTISED form: the errors
// err_ic = |[t_i == c] - p_ic| of the live pixels (label neither ignore_index nor >= C) are put into K levels (lovasz_bin of common.h) and the Lovasz
// extension of the Jaccard loss is evaluated at the level centres (b + 1/2) / K.  The extension does not care about the order among tied errors, so
// that value - and a valid subgradient - follow exactly from two integer histograms per class, with no sort:
//     dsrl_lovasz_fwd   zero fill of the workspace; one streaming pass over the logits -> nf[C][K], nb[C][K] (uint32: foreground / background pixels per
//                       level) through per-block LDS histograms and 32-bit integer global atomics; a scan per class from the top level down and a
//                       one-block finish write the record {lambda L, |Present|, 0, 0, gf[C][K], gb[C][K]}
//     dsrl_lovasz_bwd   dlogits (+)= the row of every pixel from the logits and the record (lovasz_pixel / lovasz_grad of common.h, which the
//                       ConvTranspose backward of convt_dma.hip uses too)
// Integers only up to the tables, which are formed in double from them and rounded once: the record has the same bits on every call.
#include "common.h"
#include <algorithm>

namespace dsrl {

constexpr int kLvPre = 8;                       // 16-byte loads a thread keeps in flight for the next tile: tile floats / 4 / threads <= 8 in every plan
constexpr size_t kLvLds = 160 * 1024 - 2048;    // dynamic LDS of the histogram pass: the tile and the histograms of a class group
constexpr int kLvMaxBlocks = 256;               // one block per CU: every block flushes its non-zero bins, so fewer and longer blocks mean fewer global atomics
constexpr int kLvFlushPixels = 32768;           // a block flushes its LDS histogram after at most this many pixels: the two 16-bit halves of a word cannot carry
constexpr int kLvStride = 64;                   // classes per row of the tail (C <= kLovaszMaxC)
// the workspace: nf[C][K], nb[C][K] (uint32), then the tail {double L_c[64], uint32 G_c[64], uint32 nan, 3 words of padding}
constexpr size_t kLvTailBytes = (size_t)kLvStride * (sizeof(double) + sizeof(unsigned)) + 16;

// How the histogram pass runs a shape: threads per block, pixels per tile, classes per group, tiles, tiles per flush, dynamic LDS.  A function of C and
// K (and P for the tile count) alone.  16 waves and 1024-pixel tiles when the packed histogram of EVERY class fits beside such a tile (19 x 1024 does:
// 76 KB + 76 KB): one pass over the logits with four waves per SIMD to hide the LDS and memory latencies; otherwise 8 waves, 512-pixel tiles (256
// beyond 32 classes) and as many classes per pass as fit (19 x 4096: 7, three passes); never fewer than 5.
struct LvPlan { int nt, Tp, Gc, ntiles, batch; size_t lds; };
static LvPlan lv_plan(long long P, int C, int K) {
    LvPlan p;
    if (C <= 32 && ((size_t)1024 * C + (size_t)C * K) * sizeof(float) <= kLvLds) { p.nt = 1024; p.Tp = 1024; }
    else { p.nt = 512; p.Tp = C <= 32 ? 512 : 256; }
    p.Gc = (int)std::min<size_t>((size_t)C, (kLvLds - (size_t)p.Tp * C * sizeof(float)) / ((size_t)K * sizeof(unsigned)));
    p.ntiles = (int)ceil_div(P, p.Tp);
    p.batch = kLvFlushPixels / p.Tp;
    p.lds = ((size_t)p.Tp * C + (size_t)p.Gc * K) * sizeof(float);
    return p;
}
static bool lv_bins_ok(int K) { return K >= kLovaszMinBins && K <= kLovaszMaxBins && (K & (K - 1)) == 0; }

// ---------------------------------------------------------------------------------------------- histograms
// Block `blk` takes the tiles [blk * tpc, (blk + 1) * tpc) of Tp pixels.  A tile goes through LDS as in ce_fused_kernel (dense rows: 16-byte loads,
// requested one tile ahead into registers so that they fly under the arithmetic of the tile before); one thread per pixel forms the softmax terms
// e_c of its row and counts, for every class of the group [c0, c1), the level of p_c = e_c (1 / s) in the block's LDS histogram.  CT = 19: the row
// lives in registers (19 LDS reads in flight at once, unrolled arithmetic); CT = 0: `C` at run time, the terms kept in the tile.  Same operations,
// same bits.  A word of the histogram holds both counts of a (class, level): background pixels in the low half, foreground pixels in the high
// half - 19 x 1024 words are 76 KB where two arrays would not fit beside the tile - and a flush after at most kLvFlushPixels pixels keeps both
// below 2^16.  The flush adds the non-zero halves to nf / nb with 32-bit integer atomics.  A class count or a K too large for one group takes the
// tiles once per group.
// AGG: on a trained model almost every error is in level 0 and the 64 lanes of a wave hit one LDS word; the hits of a wave on level 0 and on level
// K - 1 are counted with a ballot and added by one lane (measured: DESIGN.md §6.1.14).  Integer sums: the result is the same.
template <bool AGG, int CT>
__global__ __launch_bounds__(1024) void lovasz_hist_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, int P, int C,
                                                           int ignore_index, int K, int Tp, int Gc, int batch, int tpc, int ntiles, unsigned* __restrict__ nf,
                                                           unsigned* __restrict__ nb, unsigned* __restrict__ nan_word, int* __restrict__ nan_flag, int vec_in) {
    extern __shared__ __attribute__((aligned(16))) float lv_smem[];
    float* tile = lv_smem;                                                  // [Tp][C]
    unsigned* h = reinterpret_cast<unsigned*>(lv_smem + Tp * C);            // [Gc][K]
    const int tid = threadIdx.x, lane = tid & 63, nt = (int)blockDim.x;
    const int t0 = (int)blockIdx.x * tpc, t1 = min(t0 + tpc, ntiles);
    bool bad = false;
    float4 pre0, pre1, pre2, pre3, pre4, pre5, pre6, pre7;                  // (named, not an array: an array under the guarded loads went to scratch)
    static_assert(kLvPre == 8, "eight registers of four floats");
    pre0 = pre1 = pre2 = pre3 = pre4 = pre5 = pre6 = pre7 = make_float4(0.f, 0.f, 0.f, 0.f);
#define LV_EACH(X) X(0, pre0) X(1, pre1) X(2, pre2) X(3, pre3) X(4, pre4) X(5, pre5) X(6, pre6) X(7, pre7)
#define LV_LOAD(u, r) { const int i = tid + u * nt; if (i < nv) r = src[i]; }
#define LV_STORE(u, r) { const int i = tid + u * nt; if (i < nv) reinterpret_cast<float4*>(tile)[i] = r; }
    auto fetch = [&](int tl) {                                              // dense rows: a tile is one contiguous run that starts on a 16-byte boundary
        const int p0 = tl * Tp;
        const int nv = (min(Tp, P - p0) * C) >> 2;
        const float4* src = reinterpret_cast<const float4*>(logits + (size_t)p0 * C);
        LV_EACH(LV_LOAD)
    };
    for (int c0 = 0; c0 < C; c0 += Gc) {
        const int c1 = min(C, c0 + Gc);
        const int nh = (c1 - c0) * K;
        // one element: class c (wave-uniform) of this lane's pixel.  Every lane of the wave comes here: the ballots see whole waves
        auto count = [&](int c, float p, bool live, int tg) {
            const bool hit = c == tg;
            const int b = live ? lovasz_bin(lovasz_err(p, hit), K) : 0;     // in [0, K) for any bits
            unsigned* hc = h + (c - c0) * K;
            if (AGG) {
                const unsigned long long mh = __ballot(live && hit);
                const unsigned long long m0 = __ballot(live && b == 0), mk = __ballot(live && b == K - 1);
                if (m0 && lane == __ffsll((long long)m0) - 1) atomicAdd(hc, (unsigned)__popcll(m0 & ~mh) + ((unsigned)__popcll(m0 & mh) << 16));
                if (mk && lane == __ffsll((long long)mk) - 1) atomicAdd(hc + (K - 1), (unsigned)__popcll(mk & ~mh) + ((unsigned)__popcll(mk & mh) << 16));
                if (live && b != 0 && b != K - 1) atomicAdd(hc + b, hit ? 0x10000u : 1u);
            } else {
                if (live) atomicAdd(hc + b, hit ? 0x10000u : 1u);
            }
        };
        if (vec_in && t0 < t1) fetch(t0);
        for (int tb = t0; tb < t1; tb += batch) {
            const int te = min(t1, tb + batch);
            for (int i = tid; i < nh; i += nt) h[i] = 0u;
            for (int tl = tb; tl < te; ++tl) {
                const int p0 = tl * Tp;
                const int np = min(Tp, P - p0);
                const int nfl = np * C;
                __syncthreads();                                            // the tile before is counted; the histogram is cleared
                if (vec_in) {
                    const int nv = nfl >> 2;
                    LV_EACH(LV_STORE)
                    for (int t = (nfl & ~3) + tid; t < nfl; t += nt) tile[t] = logits[(size_t)p0 * C + t];
                    if (tl + 1 < t1) fetch(tl + 1);
                } else {
                    for (int t = tid; t < nfl; t += nt) { const int r = t / C, c = t - r * C; tile[t] = logits[(size_t)(p0 + r) * ld + c]; }
                }
                __syncthreads();
                const bool in = tid < np;
                const int tg = in ? (int)target[p0 + tid] : ignore_index;
                const bool live = in && tg != ignore_index && tg < C;
                float* v = tile + tid * C;                                  // (read by the lanes with a pixel only)
                float inv_s = 0.f;
                if constexpr (CT > 0) {
                    float e[CT];
#pragma unroll
                    for (int c = 0; c < CT; ++c) e[c] = in ? v[c] : 0.f;
                    float m = e[0];
#pragma unroll
                    for (int c = 1; c < CT; ++c) m = fmaxf(m, e[c]);
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < CT; ++c) { e[c] = exp_nonpos(e[c] - m); s += e[c]; }
                    bad |= live && !(s == s);                               // any NaN logit poisons the sum (fmaxf alone would skip it)
                    inv_s = 1.f / s;
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (c >= c0 && c < c1) count(c, e[c] * inv_s, live, tg);
                } else {
                    if (in) {
                        float m = v[0];
                        for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
                        float s = 0.f;
                        for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; v[c] = e; }
                        bad |= live && !(s == s);
                        inv_s = 1.f / s;
                    }
                    for (int c = c0; c < c1; ++c) count(c, live ? v[c] * inv_s : 0.f, live, tg);
                }
            }
            __syncthreads();
            for (int i = tid; i < nh; i += nt) {                            // (a thread clears the words it flushed: no barrier before the next batch's clear)
                const unsigned w = h[i];
                if (w) {
                    const size_t o = (size_t)c0 * K + i;
                    if (w & 0xffffu) atomicAdd(nb + o, w & 0xffffu);
                    if (w >> 16) atomicAdd(nf + o, w >> 16);
                }
            }
        }
        __syncthreads();                                                    // the next group's first fetch and clear follow the last read of this one
    }
    if (__any(bad) && lane == 0) {
        atomicOr(nan_word, 1u);
        if (nan_flag) atomicOr(nan_flag, 1);
    }
}

// ---------------------------------------------------------------------------------------------- scan per class
// Block c.  G_j = sum_b nf_j[b] of every class (integers: order-free) gives |Present|; thread t owns the levels [t L, (t + 1) L), L = max(1, K / 256),
// takes the counts above its range from the per-thread sums and walks its levels from the top down:
//     NFincl = sum_{b' >= b} nf,  NBincl = sum_{b' >= b} nb,  NBabove = NBincl - nb[b]
//     wf = 1 / (G + NBabove)        wb = (G - NFincl) / ((G + NBabove) (G + NBincl))        (double; the denominators are >= G > 0)
//     gf = -(lambda / |Present|) wf,  gb = +(lambda / |Present|) wb, rounded once;  zeros for a class with G = 0
//     L_c = sum_b ((b + 1/2) / K) (nf[b] wf[b] + nb[b] wb[b]): per thread in descending b, then over the threads in ascending t by thread 0
// A fixed function of the histograms: the same bits on every call.
__global__ __launch_bounds__(256) void lovasz_scan_kernel(const unsigned* __restrict__ nf, const unsigned* __restrict__ nb, int C, int K, float lambda,
                                                          float* __restrict__ record, double* __restrict__ Lc, unsigned* __restrict__ Gc) {
    __shared__ unsigned g_all[kLvStride];
    __shared__ unsigned sf[256], sb[256];
    __shared__ double red[256];
    const int tid = threadIdx.x, c = (int)blockIdx.x;
    if (tid < kLvStride) g_all[tid] = 0u;
    __syncthreads();
    for (int j = 0; j < C; ++j) {
        unsigned a = 0u;
        for (int i = tid; i < K; i += 256) a += nf[(size_t)j * K + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += (unsigned)__shfl_xor((int)a, o, 64);
        if ((tid & 63) == 0 && a) atomicAdd(&g_all[j], a);
    }
    const int L = max(1, K / 256), nact = K / L;
    const int lo = tid * L;
    unsigned mf = 0u, mb = 0u;
    if (tid < nact)
        for (int b = lo; b < lo + L; ++b) { mf += nf[(size_t)c * K + b]; mb += nb[(size_t)c * K + b]; }
    sf[tid] = mf; sb[tid] = mb;
    __syncthreads();
    int npres = 0;
    for (int j = 0; j < C; ++j) npres += g_all[j] > 0u ? 1 : 0;
    const unsigned G = g_all[c];
    unsigned long long af = 0ull, ab = 0ull;                               // counts in the levels above this thread's range
    for (int t = tid + 1; t < nact; ++t) { af += sf[t]; ab += sb[t]; }
    const double lk = npres ? (double)lambda / (double)npres : 0.0;
    double acc = 0.0;
    if (tid < nact) {
        float* gf = record + kLovaszHeadFloats + (size_t)c * K;
        float* gb = gf + (size_t)C * K;
        for (int b = lo + L - 1; b >= lo; --b) {
            const unsigned f = nf[(size_t)c * K + b], n = nb[(size_t)c * K + b];
            const unsigned long long nb_incl = ab + n, nf_incl = af + f;
            float of = 0.f, ob = 0.f;
            if (G > 0u) {
                const double d1 = (double)G + (double)ab, d2 = (double)G + (double)nb_incl;
                const double wf = 1.0 / d1;
                const double wb = ((double)G - (double)nf_incl) / (d1 * d2);
                acc += (((double)b + 0.5) / (double)K) * ((double)f * wf + (double)n * wb);
                of = (float)(-lk * wf);
                ob = (float)(lk * wb);
            }
            gf[b] = of;
            gb[b] = ob;
            ab = nb_incl; af = nf_incl;
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int t = 0; t < nact; ++t) sum += red[t];
        Lc[c] = sum;
        Gc[c] = G;
    }
}
// record[0..4) = {lambda (sum_c L_c, c ascending) / |Present| - NaN when a live pixel had a NaN logit -, |Present|, 0, 0}; 0 when no class is present
__global__ __launch_bounds__(64) void lovasz_finish_kernel(const double* __restrict__ Lc, const unsigned* __restrict__ Gc, const unsigned* __restrict__ nan_word, int C,
                                                           float lambda, float* __restrict__ record) {
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    int npres = 0;
    for (int c = 0; c < C; ++c) { sum += Lc[c]; npres += Gc[c] > 0u ? 1 : 0; }
    const float val = npres ? (float)((double)lambda * (sum / (double)npres)) : 0.f;
    record[0] = nan_word[0] ? __uint_as_float(0x7fc00000u) : val;
    record[1] = (float)npres;
    record[2] = 0.f;
    record[3] = 0.f;
}

// ---------------------------------------------------------------------------------------------- gradient
// ce_fused_kernel's staging and softmax terms, then the row through lovasz_pixel / lovasz_grad; the coefficients are gathered from the record in
// global memory (155 KB at C = 19, K = 1024: L2), twice per element here - once for the sum over the classes, once for the row - where the fused
// kernel keeps them in registers.  accumulate: dl = dl + row (a pixel that is not live adds +0).
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, int P, int C,
                                                         int ignore_index, const float* __restrict__ record, int K, int accumulate, float* __restrict__ dl,
                                                         int lddl, int ntiles, int vec_in, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) float lv_smem[];      // [256][C]
    float* tile = lv_smem;
    const float* gf = record + kLovaszHeadFloats;
    const float* gb = gf + (size_t)C * K;
    const int tid = threadIdx.x;
    for (int tl = (int)blockIdx.x; tl < ntiles; tl += (int)gridDim.x) {
        const int p0 = tl * 256;
        const int np = min(256, P - p0);
        const int nfl = np * C;
        __syncthreads();
        if (vec_in) {
            const float4* src = reinterpret_cast<const float4*>(logits + (size_t)p0 * C);
            for (int t = tid; t < (nfl >> 2); t += 256) reinterpret_cast<float4*>(tile)[t] = src[t];
            for (int t = (nfl & ~3) + tid; t < nfl; t += 256) tile[t] = logits[(size_t)p0 * C + t];
        } else {
            for (int t = tid; t < nfl; t += 256) { const int r = t / C, c = t - r * C; tile[t] = logits[(size_t)(p0 + r) * ld + c]; }
        }
        __syncthreads();
        if (tid < np) {
            const int tg = target[p0 + tid];
            const bool live = tg != ignore_index && tg < C;
            float* v = tile + tid * C;
            float m = v[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) { const float e = exp_nonpos(v[c] - m); s += e; v[c] = e; }
            float inv_s, dot;
            lovasz_pixel<0>(v, C, s, tg, live, gf, gb, K, inv_s, nullptr, dot);
            for (int c = 0; c < C; ++c) {
                const float gc = live ? lovasz_coef(v[c] * inv_s, c == tg, c, gf, gb, K) : 0.f;
                v[c] = lovasz_grad(v[c], inv_s, gc, dot, live);
            }
        }
        __syncthreads();
        if (vec_out) {
            float4* dst = reinterpret_cast<float4*>(dl + (size_t)p0 * C);
            for (int t = tid; t < (nfl >> 2); t += 256) {
                float4 r = reinterpret_cast<const float4*>(tile)[t];
                if (accumulate) { const float4 o = dst[t]; r.x = o.x + r.x; r.y = o.y + r.y; r.z = o.z + r.z; r.w = o.w + r.w; }
                dst[t] = r;
            }
            for (int t = (nfl & ~3) + tid; t < nfl; t += 256) { float* o = dl + (size_t)p0 * C + t; *o = accumulate ? *o + tile[t] : tile[t]; }
        } else {
            for (int t = tid; t < nfl; t += 256) {
                const int r = t / C, c = t - r * C;
                float* o = dl + (size_t)(p0 + r) * lddl + c;
                *o = accumulate ? *o + tile[t] : tile[t];
            }
        }
    }
}

}  // namespace dsrl
using namespace dsrl;

#define DSRL_LOVASZ_SHAPE(P, C, K, what)                                                                                                            \
    DSRL_REQUIRE((P) > 0 && (P) <= 0x7fffffffll - 256 && (C) >= 1 && (C) <= kLovaszMaxC && lv_bins_ok(K), DSRL_E_BADARG,                             \
                 what ": P = %lld must be in [1, 2^31 - 256), C = %d in [1, 60] and bins = %d a power of two in [16, 4096]", (long long)(P), (int)(C), (int)(K))

extern "C" size_t dsrl_lovasz_record_floats(int C, int bins) {
    if (C < 1 || C > kLovaszMaxC || !lv_bins_ok(bins)) { set_error("lovasz_record_floats: bad arguments (C=%d, bins=%d)", C, bins); return 0; }
    return (size_t)kLovaszHeadFloats + 2 * (size_t)C * bins;
}
extern "C" size_t dsrl_lovasz_workspace_bytes(int64_t P, int C, int bins) {
    if (P <= 0 || P > 0x7fffffffll - 256 || C < 1 || C > kLovaszMaxC || !lv_bins_ok(bins)) {
        set_error("lovasz_workspace_bytes: bad arguments (P=%lld, C=%d, bins=%d)", (long long)P, C, bins);
        return 0;
    }
    return 2 * (size_t)C * bins * sizeof(unsigned) + kLvTailBytes;
}
extern "C" int dsrl_lovasz_fwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float lambda, int bins, float* record,
                               int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(lambda > 0.f && lambda <= 3.402823466e+38f, DSRL_E_BADARG, "lovasz_fwd: lambda = %g must be a finite number > 0", (double)lambda);
    DSRL_LOVASZ_SHAPE(P, C, bins, "lovasz_fwd");
    DSRL_REQUIRE(logits && target && record && ws && ld >= C && ((uintptr_t)record % 4) == 0, DSRL_E_BADARG, "lovasz_fwd: bad arguments (C=%d, ld=%d)", C, ld);
    DSRL_REQUIRE(ws_bytes >= dsrl_lovasz_workspace_bytes(P, C, bins) && ((uintptr_t)ws % 16) == 0, DSRL_E_WORKSPACE, "lovasz_fwd: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int K = bins;
    unsigned* nf = (unsigned*)ws;
    unsigned* nb = nf + (size_t)C * K;
    double* Lc = (double*)(nb + (size_t)C * K);
    unsigned* Gc = (unsigned*)(Lc + kLvStride);
    unsigned* nan_word = Gc + kLvStride;
    if (int e = launch_zero_fill(ws, dsrl_lovasz_workspace_bytes(P, C, K), st)) return e;       // the call clears its own histograms, on the stream
    const LvPlan pl = lv_plan(P, C, K);
    const int nblocks = std::min(kLvMaxBlocks, pl.ntiles);
    const int tpc = (int)ceil_div(pl.ntiles, nblocks);
    const int vec_in = (ld == C && ((uintptr_t)logits % 16) == 0) ? 1 : 0;          // Tp * C floats per tile: every tile starts 16-byte aligned
    const bool agg = knob("DSRL_LOVASZ_AGG", 1) != 0;
    void (*kern)(const float*, int, const unsigned char*, int, int, int, int, int, int, int, int, int, unsigned*, unsigned*, unsigned*, int*, int) =
        C == 19 ? (agg ? lovasz_hist_kernel<true, 19> : lovasz_hist_kernel<false, 19>) : (agg ? lovasz_hist_kernel<true, 0> : lovasz_hist_kernel<false, 0>);
    static const hipError_t attr[4] = {hipFuncSetAttribute((const void*)lovasz_hist_kernel<true, 19>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLvLds),
                                       hipFuncSetAttribute((const void*)lovasz_hist_kernel<false, 19>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLvLds),
                                       hipFuncSetAttribute((const void*)lovasz_hist_kernel<true, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLvLds),
                                       hipFuncSetAttribute((const void*)lovasz_hist_kernel<false, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLvLds)};
    for (hipError_t a : attr)
        if (a != hipSuccess) { set_error("lovasz_hist_kernel: %zu bytes of LDS refused", kLvLds); return DSRL_E_LAUNCH; }
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(pl.nt), pl.lds, st, logits, ld, target, (int)P, C, ignore_index, K, pl.Tp, pl.Gc, pl.batch, tpc, pl.ntiles, nf, nb,
                       nan_word, nan_flag, vec_in);
    if (int e = launch_status("lovasz_hist_kernel")) return e;
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(C), dim3(256), 0, st, (const unsigned*)nf, (const unsigned*)nb, C, K, lambda, record, Lc, Gc);
    if (int e = launch_status("lovasz_scan_kernel")) return e;
    hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)Lc, (const unsigned*)Gc, (const unsigned*)nan_word, C, lambda, record);
    return launch_status("lovasz_finish_kernel");
}
extern "C" int dsrl_lovasz_bwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* record, int bins, int accumulate,
                               float* dlogits, int lddl, dsrl_stream_t stream) {
    DSRL_LOVASZ_SHAPE(P, C, bins, "lovasz_bwd");
    DSRL_REQUIRE(logits && target && record && dlogits && ld >= C && lddl >= C && (accumulate == 0 || accumulate == 1) && ((uintptr_t)record % 4) == 0, DSRL_E_BADARG,
                 "lovasz_bwd: bad arguments (C=%d, ld=%d, lddl=%d, accumulate=%d)", C, ld, lddl, accumulate);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int vec_in = (ld == C && ((uintptr_t)logits % 16) == 0) ? 1 : 0;
    const int vec_out = (lddl == C && ((uintptr_t)dlogits % 16) == 0) ? 1 : 0;
    const int ntiles = (int)ceil_div(P, 256);
    hipLaunchKernelGGL(lovasz_bwd_kernel, dim3(std::min(1024, ntiles)), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, (int)P, C, ignore_index,
                       record, bins, accumulate, dlogits, lddl, ntiles, vec_in, vec_out);
    return launch_status("lovasz_bwd_kernel");
}
