// Gradient-norm clipping on the flat gradient arena: torch.nn.utils.clip_grad_norm_ without a host read, a host write or a launch
// per parameter, so that the step stays one captured graph.  The clip coefficient is folded into the optimiser's grad_scale: no SGD kernel changes.
//     dsrl_grad_sumsq          one streaming pass over a 1024-aligned range of the arena -> the sum of squares of every 1024-float tile, in double
//     dsrl_grad_clip_finish    the tiles in a fixed order -> S; norm = gs sqrt(S), coef = min(1, max_norm / (norm + 1e-6)); writes the optimiser's four
//                              hyper-parameters with gs coef in the place of gs, and the record (common.h: GradClipRecord)
// Tiles are anchored at arena offset 0 and each is summed by one wave in an order that depends on nothing but the position inside the tile; the finish
// adds the tiles in an order that depends on nothing but their count.  So S has the same bits however the arena is cut into calls (the ranges of
// ddp.FlatParams.reduce_chunked_and_step) and on every run.  No atomics, no zero fill: a tile slot is written by exactly one wave.
// A float square is exact in double (24 x 24 bits), so the double additions are the only rounding: 1023 of them per tile.
#include "common.h"
#include <algorithm>

namespace dsrl {

constexpr int kClipTile = 1024;                 // floats per tile: 64 lanes x 4 float4
constexpr int kClipSumBlocks = 1024;            // at most 4 blocks of 4 waves per CU, each wave with 4 + 4 16-byte loads in flight; beyond it the grid wraps
constexpr int kClipChunk = 1024;                // tiles per block of the finish's first level (58.5 k tiles of the real arena: 58 blocks)

__device__ __forceinline__ double sq4(double acc, const float4 v) {
    acc += (double)v.x * (double)v.x;
    acc += (double)v.y * (double)v.y;
    acc += (double)v.z * (double)v.z;
    acc += (double)v.w * (double)v.w;
    return acc;
}

// One wave per tile, 4 tiles per block, the block's tile groups grid-strided.  Lane l takes the float4s l, l + 64, l + 128, l + 192 of the tile in
// that order, x y z w inside each, into one double; then the xor butterfly over the 64 lanes (the same tree in every lane).  The next tile's four
// loads are issued before the current tile is reduced.  A last tile of fewer than 1024 floats reads what is there (float4 where all four are, single
// floats behind) and adds zeros for the rest: same order, same bits as a full tile padded with zeros.  Indices inside a tile are 32-bit; the only
// 64-bit arithmetic is one multiply per tile.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n, long long ntiles, double* __restrict__ tiles) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long stride = (long long)gridDim.x * 4;
    const long long nfull = n / kClipTile;                  // tiles with all 1024 floats (once per thread)
    long long t = (long long)blockIdx.x * 4 + wave;
    float4 cur[4], nxt[4];
    if (t < nfull) {
        const float4* src = reinterpret_cast<const float4*>(g + t * kClipTile);
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = src[lane + 64 * j];
    }
    for (; t < nfull; t += stride) {
        const long long tn = t + stride;
        if (tn < nfull) {
            const float4* src = reinterpret_cast<const float4*>(g + tn * kClipTile);
#pragma unroll
            for (int j = 0; j < 4; ++j) nxt[j] = src[lane + 64 * j];
        }
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = sq4(acc, cur[j]);
        acc = wave_sum_d(acc);
        if (lane == 0) tiles[t] = acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    // the short last tile, if any: exactly one wave of the grid arrives here with t == nfull
    if (t == nfull && nfull < ntiles) {
        const float* src = g + nfull * kClipTile;
        const int left = (int)(n - nfull * kClipTile);      // 1 .. 1023
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = (lane + 64 * j) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e + 3 < left) {
                v = *reinterpret_cast<const float4*>(src + e);
            } else {
                if (e < left) v.x = src[e];
                if (e + 1 < left) v.y = src[e + 1];
                if (e + 2 < left) v.z = src[e + 2];
            }
            acc = sq4(acc, v);
        }
        acc = wave_sum_d(acc);
        if (lane == 0) tiles[nfull] = acc;
    }
}

// First level of the finish: block b adds the tiles [1024 b, 1024 b + 1024) - thread i the tiles i, i + 256, i + 512, i + 768 of the chunk in that
// order (independent loads), the butterfly per wave, the four waves in ascending order - into parts[b].  A fixed function of ntiles.
__global__ __launch_bounds__(256) void grad_clip_parts_kernel(const double* __restrict__ tiles, int ntiles, double* __restrict__ parts) {
    __shared__ double ws[4];
    const int t0 = (int)blockIdx.x * kClipChunk;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kClipChunk / 256; ++j) {
        const int t = t0 + (int)threadIdx.x + 256 * j;
        acc += t < ntiles ? tiles[t] : 0.0;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// Second level, one wave: lane l adds parts l, l + 64, ... in ascending order, then the butterfly -> S.  Lane 0 forms the coefficient in double and
// writes the hyper-parameters and the record.  torch's formula, clamp(max = 1) included: a NaN norm fails the comparison and stays a NaN coefficient,
// an infinite norm gives max_norm / inf = 0 (NaN when max_norm is infinite as well, as in torch).  coef == 1 hands gs through untouched.
__global__ __launch_bounds__(64) void grad_clip_final_kernel(const double* __restrict__ parts, int nparts, const float* __restrict__ hyper_in, float lr, float mom,
                                                             float wd, float gs, GradClipRecord* __restrict__ rec, float* __restrict__ hyper_out) {
    const int lane = threadIdx.x;
    double S = 0.0;
    for (int b = lane; b < nparts; b += 64) S += parts[b];
    S = wave_sum_d(S);
    if (lane != 0) return;
    if (hyper_in) { lr = hyper_in[0]; mom = hyper_in[1]; wd = hyper_in[2]; gs = hyper_in[3]; }
    const double norm = (double)gs * sqrt(S);
    const double max_norm = (double)rec->max_norm;
    double coef = max_norm / (norm + 1e-6);
    coef = coef > 1.0 ? 1.0 : coef;
    hyper_out[0] = lr; hyper_out[1] = mom; hyper_out[2] = wd;
    hyper_out[3] = coef == 1.0 ? gs : (float)((double)gs * coef);
    rec->sumsq = S;
    rec->norm = (float)norm;
    rec->coef = (float)coef;
    rec->steps += 1u;
    if (norm - norm == 0.0) {               // finite (inf - inf and NaN - NaN are NaN)
        rec->norm_sum += norm;
        rec->norm_max = fmaxf(rec->norm_max, (float)norm);
        if (coef < 1.0) rec->clipped += 1u;
    } else {
        rec->nonfinite += 1u;
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
static inline int64_t clip_tiles(int64_t n) { return ceil_div(n, kClipTile); }
static inline int64_t clip_parts(int64_t ntiles) { return ceil_div(ntiles, kClipChunk); }

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_grad_sumsq(const float* g, int64_t first, int64_t n, double* tiles, dsrl_stream_t stream) {
    DSRL_REQUIRE(g && tiles && first >= 0 && n > 0, DSRL_E_BADARG, "grad_sumsq: bad arguments");
    DSRL_REQUIRE(first % kClipTile == 0, DSRL_E_BADARG, "grad_sumsq: first = %lld is not a multiple of %d", (long long)first, kClipTile);
    DSRL_REQUIRE(aligned16(g) && ((uintptr_t)tiles % 8) == 0, DSRL_E_BADARG, "grad_sumsq: the arena must be 16-byte aligned (the tile array 8-byte)");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int64_t nt = clip_tiles(n);
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(nt, 4), kClipSumBlocks);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(256), 0, st, g + first, (long long)n, (long long)nt, tiles + first / kClipTile);
    return launch_status("grad_sumsq_kernel");
}

// the tile array, then the finish's first-level sums behind it: a function of the tile count alone, whatever is launched on it
extern "C" size_t dsrl_grad_clip_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    const int64_t nt = clip_tiles(n);
    return (size_t)(nt + clip_parts(nt)) * sizeof(double);
}

extern "C" int dsrl_grad_clip_finish(const double* tiles, int64_t ntiles, const float* hyper_in, float lr, float momentum, float weight_decay, float grad_scale,
                                     void* record, float* hyper_out, dsrl_stream_t stream) {
    DSRL_REQUIRE(tiles && record && hyper_out && ntiles > 0 && ntiles < (1ll << 31), DSRL_E_BADARG, "grad_clip_finish: bad arguments");
    DSRL_REQUIRE(((uintptr_t)tiles % 8) == 0 && aligned16(record) && ((uintptr_t)hyper_out % 4) == 0 && ((uintptr_t)hyper_in % 4) == 0, DSRL_E_BADARG,
                 "grad_clip_finish: the record must be 16-byte aligned (the tile array 8-byte, the hyper-parameters 4-byte)");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int np = (int)clip_parts(ntiles);
    double* parts = const_cast<double*>(tiles) + ntiles;        // the workspace behind the tiles (dsrl_grad_clip_workspace_bytes)
    hipLaunchKernelGGL(grad_clip_parts_kernel, dim3((unsigned)np), dim3(256), 0, st, tiles, (int)ntiles, parts);
    if (int e = launch_status("grad_clip_parts_kernel")) return e;
    hipLaunchKernelGGL(grad_clip_final_kernel, dim3(1), dim3(64), 0, st, (const double*)parts, np, hyper_in, lr, momentum, weight_decay, grad_scale,
                       (GradClipRecord*)record, hyper_out);
    return launch_status("grad_clip_final_kernel");
}
