// Quality of the super-resolved image: per image the squared error and the SSIM sum of pred against ref in one pass over both.
//     dsrl_sr_quality_workspace_bytes   16 bytes per (image, tile): the block partials
//     dsrl_sr_quality                   two launches: sr_quality_kernel (a block per 32 x 64 tile of the SSIM map) and sr_quality_finish_kernel
// A block stages its (32 + 10) x (64 + 10) input window of both images, de-normalised and clamped, as channel planes in LDS (float4 loads of the
// interleaved rows, de-interleaved on the way in), takes the squared error of the pixels it owns from the planes, and then wave c filters channel c:
// a thread owns one column of the tile and walks down the 42 rows.  Per row it forms the five row-filtered moments (x, y, xx, xy, yy: 22 LDS reads,
// taps ascending) and adds them with the column weights into the 11 output rows that are open - eleven accumulators of five moments in registers,
// indexed statically because the row loop is fully unrolled.  Nothing but the two planes goes through LDS and no moment goes through memory.
// LDS: 2 * C * 42 * 74 * 4 bytes = 74.6 KB at C = 3: two blocks per CU.  Input bytes re-read: 42 * 74 / (32 * 64) = 1.52 x, the halo from L2.
// Determinism: a tile's partials depend on its image alone (the grid's z is the image), every block writes its own slot, the finish launch adds an
// image's slots in a fixed order - no atomics, so a record is the same bits run to run and alone or inside a batch.
#include "common.h"
#include <math.h>
#include <utility>

namespace dsrl {

constexpr int kSrqTH = 32, kSrqTW = 64, kSrqWin = 11, kSrqHalo = kSrqWin - 1;
constexpr int kSrqIH = kSrqTH + kSrqHalo, kSrqIW = kSrqTW + kSrqHalo;

struct SrqArgs {
    float g[kSrqWin];       // the window, normalised in double and rounded once
};
struct SrqNorm {            // mean and std as vector values: picked by channel with selects, never through memory
    float4 mean, std;
};

// v = x * std + mean (two roundings: the library is built -ffp-contract=off), clamped to [0, 1] by comparisons, which a NaN fails both of
template <int C>
__device__ __forceinline__ float srq_value(float x, int c, const SrqNorm nm) {
    float s = nm.std.x, m = nm.mean.x;
    if (C > 1 && c == 1) { s = nm.std.y; m = nm.mean.y; }
    if (C > 2 && c == 2) { s = nm.std.z; m = nm.mean.z; }
    if (C > 3 && c == 3) { s = nm.std.w; m = nm.mean.w; }
    float v = x * s;
    v = v + m;
    v = v < 0.f ? 0.f : v;
    v = v > 1.f ? 1.f : v;
    return v;
}

// Rows [0, ih) x pixels [0, iw) of the window that starts at `src` (pixel stride ld, row stride `rowstride` floats) -> dst[c][row][pixel].
// A lane owns a 16-byte piece of the row segment (its pixel and channel are found once, by the one 32-bit division), a wave every fourth row.
// vec: src is 16-byte aligned and rowstride % 4 == 0; then no piece crosses the end of its row (the segment ends at the row's end or 4 | its length
// rounded up fits, both rows' lengths being multiples of 4 floats).
template <int C>
__device__ __forceinline__ void srq_stage(const float* __restrict__ src, int ld, int rowstride, int ih, int iw, bool vec, float (*dst)[kSrqIH][kSrqIW],
                                          const SrqNorm nm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nfl = iw * ld;
    if (vec) {
        const int nch = (nfl + 3) >> 2;
        for (int ch = lane; ch < nch; ch += 64) {
            const int f0 = ch * 4;
            const int p0 = f0 / ld, c0 = f0 - p0 * ld;
            for (int r0 = w; r0 < ih; r0 += 16) {
                float4 v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = r0 + 4 * i;
                    v[i] = r < ih ? *reinterpret_cast<const float4*>(src + r * rowstride + f0) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = r0 + 4 * i;
                    if (r < ih) {
                        int p = p0, c = c0;
                        auto put = [&](float e) {
                            if (c < C && p < iw) dst[c][r][p] = srq_value<C>(e, c, nm);
                            if (++c == ld) { c = 0; ++p; }
                        };
                        put(v[i].x); put(v[i].y); put(v[i].z); put(v[i].w);
                    }
                }
            }
        }
    } else {
        for (int f = lane; f < nfl; f += 64) {
            const int p = f / ld, c = f - p * ld;
            if (c >= C) continue;
            for (int r = w; r < ih; r += 4) dst[c][r][p] = srq_value<C>(src[r * rowstride + f], c, nm);
        }
    }
}

struct SrqTile { int n, c, col, oy0, ox0, vh, vw, ih, Ho, Wo; };

// Input row R of a thread's column: the five row-filtered moments, added into the open output rows (row R is tap R - o of output row o), and
// output row R - 10, which this row completes.  R is a template argument so that `acc` is indexed by constants and lives in registers.
template <int C, int R>
__device__ __forceinline__ void srq_row(const float (*sx)[kSrqIW], const float (*sy)[kSrqIW], const SrqArgs& a, const SrqTile& tl, float (&acc)[kSrqWin][5],
                                        double& ssum, float* __restrict__ map) {
    if (R >= tl.ih) return;         // block-uniform: a short last tile stops early
    float h[5];
#pragma unroll
    for (int k = 0; k < kSrqWin; ++k) {
        const float x = sx[R][tl.col + k], y = sy[R][tl.col + k];
        const float xx = x * x, xy = x * y, yy = y * y;
        if (k == 0) {
            h[0] = a.g[0] * x; h[1] = a.g[0] * y; h[2] = a.g[0] * xx; h[3] = a.g[0] * xy; h[4] = a.g[0] * yy;
        } else {
            h[0] = fmaf(a.g[k], x, h[0]); h[1] = fmaf(a.g[k], y, h[1]); h[2] = fmaf(a.g[k], xx, h[2]);
            h[3] = fmaf(a.g[k], xy, h[3]); h[4] = fmaf(a.g[k], yy, h[4]);
        }
    }
#pragma unroll
    for (int k = 0; k < kSrqWin; ++k) {
        const int o = R - k;
        if (o >= 0 && o < kSrqTH) {
            const int s = o % kSrqWin;
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[s][m] = k == 0 ? a.g[0] * h[m] : fmaf(a.g[k], h[m], acc[s][m]);
        }
    }
    if (R >= kSrqHalo) {
        constexpr int o = R >= kSrqHalo ? R - kSrqHalo : 0, s = o % kSrqWin;
        const float mux = acc[s][0], muy = acc[s][1];
        const float mxx = mux * mux, myy = muy * muy, mxy = mux * muy;
        const float sxx = acc[s][2] - mxx, sxy = acc[s][3] - mxy, syy = acc[s][4] - myy;
        const float num = (2.f * mxy + 1e-4f) * (2.f * sxy + 9e-4f);
        const float den = ((mxx + myy) + 1e-4f) * ((sxx + syy) + 9e-4f);
        const float v = __fdiv_rn(num, den);
        if (o < tl.vh && tl.col < tl.vw) {
            ssum += (double)v;
            if (map != nullptr) map[((tl.n * C + tl.c) * tl.Ho + (tl.oy0 + o)) * tl.Wo + (tl.ox0 + tl.col)] = v;
        }
    }
}
template <int C, int... R>
__device__ __forceinline__ void srq_rows(const float (*sx)[kSrqIW], const float (*sy)[kSrqIW], const SrqArgs& a, const SrqTile& tl, float (&acc)[kSrqWin][5],
                                         double& ssum, float* __restrict__ map, std::integer_sequence<int, R...>) {
    (srq_row<C, R>(sx, sy, a, tl, acc, ssum, map), ...);
}

template <int C>
__global__ __launch_bounds__(256) void sr_quality_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ ref, int ldr, int H, int W,
                                                         SrqArgs a, SrqNorm nm, double* __restrict__ part, float* __restrict__ map, int vec) {
    __shared__ float sx[C][kSrqIH][kSrqIW];
    __shared__ float sy[C][kSrqIH][kSrqIW];
    __shared__ double red[2][4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = blockIdx.z, oy0 = blockIdx.y * kSrqTH, ox0 = blockIdx.x * kSrqTW;
    const int Ho = H - kSrqHalo, Wo = W - kSrqHalo;
    const int vh = min(kSrqTH, Ho - oy0), vw = min(kSrqTW, Wo - ox0);       // this tile's rows and columns of the map
    const int ih = vh + kSrqHalo, iw = vw + kSrqHalo;                        // and of the input
    const int pix0 = (n * H + oy0) * W + ox0;                                // 32-bit: the host refuses N * H * W * ld >= 2^31

    srq_stage<C>(pred + (size_t)pix0 * ldp, ldp, W * ldp, ih, iw, (vec & 1) != 0, sx, nm);
    srq_stage<C>(ref + (size_t)pix0 * ldr, ldr, W * ldr, ih, iw, (vec & 2) != 0, sy, nm);
    __syncthreads();

    // squared error of the input pixels this tile owns: its own 32 x 64, and the halo too where no tile follows
    double sse = 0.0;
    {
        const int own_h = blockIdx.y == gridDim.y - 1 ? ih : kSrqTH, own_w = blockIdx.x == gridDim.x - 1 ? iw : kSrqTW;
        for (int c = 0; c < C; ++c)
            for (int r = w; r < own_h; r += 4)
                for (int p = lane; p < own_w; p += 64) {
                    const float d = sx[c][r][p] - sy[c][r][p];
                    sse += (double)(d * d);
                }
    }

    double ssum = 0.0;
    if (w < C) {
        float acc[kSrqWin][5];
        const SrqTile tl{n, w, lane, oy0, ox0, vh, vw, ih, Ho, Wo};
        srq_rows<C>(sx[w], sy[w], a, tl, acc, ssum, map, std::make_integer_sequence<int, kSrqIH>());
    }

    sse = wave_sum_d(sse);
    ssum = wave_sum_d(ssum);
    if (lane == 0) { red[0][w] = sse; red[1][w] = ssum; }
    __syncthreads();
    if (t == 0) {
        double* out = part + 2 * (size_t)((n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        out[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        out[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// records[n] = {sum of image n's sse partials, sum of its ssim partials}: thread t adds slots t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void sr_quality_finish_kernel(const double* __restrict__ part, int tiles, double* __restrict__ records) {
    __shared__ double s[2][256];
    const int t = threadIdx.x;
    const double* p = part + 2 * (size_t)blockIdx.x * tiles;
    double a = 0.0, b = 0.0;
    for (int i = t; i < tiles; i += 256) { a += p[2 * i]; b += p[2 * i + 1]; }
    s[0][t] = a; s[1][t] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { s[0][t] += s[0][t + o]; s[1][t] += s[1][t + o]; }
        __syncthreads();
    }
    if (t == 0) { records[2 * blockIdx.x] = s[0][0]; records[2 * blockIdx.x + 1] = s[1][0]; }
}

static inline bool srq_shape_ok(int N, int C, int H, int W) { return N >= 1 && C >= 1 && C <= 4 && H >= kSrqWin && W >= kSrqWin; }
static inline int64_t srq_tiles_y(int H) { return ceil_div(H - kSrqHalo, kSrqTH); }
static inline int64_t srq_tiles_x(int W) { return ceil_div(W - kSrqHalo, kSrqTW); }

}  // namespace dsrl

using namespace dsrl;

extern "C" size_t dsrl_sr_quality_workspace_bytes(int N, int C, int H, int W) {
    if (!srq_shape_ok(N, C, H, W)) return 0;
    return (size_t)N * (size_t)(srq_tiles_y(H) * srq_tiles_x(W)) * 2 * sizeof(double);
}

extern "C" int dsrl_sr_quality(const float* pred, int ld_pred, const float* ref, int ld_ref, int N, int C, int H, int W, const float* mean,
                               const float* std, double* records, float* ssim_map, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(pred && ref && mean && std && records, DSRL_E_BADARG, "sr_quality: null pointer");
    DSRL_REQUIRE(srq_shape_ok(N, C, H, W), DSRL_E_BADARG, "sr_quality: N=%d C=%d H=%d W=%d (1 <= C <= 4, H and W >= 11: the window is 11x11)", N, C, H, W);
    DSRL_REQUIRE(ld_pred >= C && ld_ref >= C, DSRL_E_BADARG, "sr_quality: leading dimensions %d, %d below C=%d", ld_pred, ld_ref, C);
    DSRL_REQUIRE(((uintptr_t)pred % 4) == 0 && ((uintptr_t)ref % 4) == 0 && ((uintptr_t)records % 8) == 0 && ((uintptr_t)ssim_map % 4) == 0, DSRL_E_BADARG,
                 "sr_quality: misaligned pointer");
    SrqArgs a;
    float mn[4] = {0.f, 0.f, 0.f, 0.f}, sd[4] = {1.f, 1.f, 1.f, 1.f};
    for (int c = 0; c < C; ++c) {
        mn[c] = mean[c]; sd[c] = std[c];
        DSRL_REQUIRE(isfinite(mn[c]) && isfinite(sd[c]) && sd[c] != 0.f, DSRL_E_BADARG, "sr_quality: mean[%d]=%g std[%d]=%g (finite, std != 0)", c,
                     (double)mn[c], c, (double)sd[c]);
    }
    const SrqNorm nm{make_float4(mn[0], mn[1], mn[2], mn[3]), make_float4(sd[0], sd[1], sd[2], sd[3])};
    const int64_t elems = (int64_t)N * H * W * (ld_pred > ld_ref ? ld_pred : ld_ref);
    const int64_t ty = srq_tiles_y(H), tx = srq_tiles_x(W);
    DSRL_REQUIRE(elems < (1ll << 31) && N <= 65535 && ty <= 65535, DSRL_E_UNSUPPORTED, "sr_quality: N=%d H=%d W=%d ld=%d,%d does not fit 32-bit element indices",
                 N, H, W, ld_pred, ld_ref);
    const size_t need = dsrl_sr_quality_workspace_bytes(N, C, H, W);
    DSRL_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws % 8) == 0, DSRL_E_WORKSPACE, "sr_quality: workspace of %zu bytes (8-byte aligned) needed, got %zu", need,
                 ws_bytes);
    {
        double g[kSrqWin], sum = 0.0;
        for (int k = 0; k < kSrqWin; ++k) { g[k] = exp(-(double)((k - 5) * (k - 5)) / 4.5); sum += g[k]; }
        for (int k = 0; k < kSrqWin; ++k) a.g[k] = (float)(g[k] / sum);
    }
    const int vec = ((((uintptr_t)pred % 16) == 0 && ((int64_t)W * ld_pred) % 4 == 0) ? 1 : 0) | ((((uintptr_t)ref % 16) == 0 && ((int64_t)W * ld_ref) % 4 == 0) ? 2 : 0);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)N);
    double* part = (double*)ws;
    switch (C) {
        case 1: hipLaunchKernelGGL(sr_quality_kernel<1>, grid, dim3(256), 0, st, pred, ld_pred, ref, ld_ref, H, W, a, nm, part, ssim_map, vec); break;
        case 2: hipLaunchKernelGGL(sr_quality_kernel<2>, grid, dim3(256), 0, st, pred, ld_pred, ref, ld_ref, H, W, a, nm, part, ssim_map, vec); break;
        case 3: hipLaunchKernelGGL(sr_quality_kernel<3>, grid, dim3(256), 0, st, pred, ld_pred, ref, ld_ref, H, W, a, nm, part, ssim_map, vec); break;
        default: hipLaunchKernelGGL(sr_quality_kernel<4>, grid, dim3(256), 0, st, pred, ld_pred, ref, ld_ref, H, W, a, nm, part, ssim_map, vec); break;
    }
    if (int e = launch_status("sr_quality_kernel")) return e;
    hipLaunchKernelGGL(sr_quality_finish_kernel, dim3((unsigned)N), dim3(256), 0, st, (const double*)part, (int)(ty * tx), records);
    return launch_status("sr_quality_finish_kernel");
}
