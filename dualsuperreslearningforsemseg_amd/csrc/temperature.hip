// Temperature scaling, the fit (include/dsrl_hip.h, "temperature"): one streaming pass over a batch's logits leaves the NLL of
// softmax(beta v) against the labels, with its first and second derivative in beta = 1 / T, at up to 16 values of beta.  A fit then needs two passes
// over a split (a coarse grid, a fine grid across the bracket it found) instead of one softmax pass per optimiser iteration.
//     dsrl_temperature_stats   temperature_stats_kernel<KT>: per-block partial sums in double -> temperature_finish_kernel: one block adds them in a
//                              fixed order and adds the totals to the caller's record {live pixels, (sum L, sum G, sum H) per beta}
// Addressing of calibration_from_logits_kernel and staging of dice_sums_kernel: a block stages 256 pixels x C logits into LDS by coalesced loads (16-byte
// loads when the rows are dense and the base aligned), then a thread owns one pixel; inside a tile every index is a 32-bit integer (the tile's base
// pointers are formed once per tile).  The per-pixel arithmetic is temperature_terms (common.h).  A thread keeps its 3 K running sums in double
// registers across the tiles of its block: the K loop is unrolled over the template values KT = 1, 2, 4, 8, 16 (the smallest >= K), so the sums never
// become an indexed private array (no scratch).  No float atomics and a pixel -> block mapping that depends on P alone: a record has the same bits
// on every call.
#include "common.h"
#include <algorithm>
#include <limits.h>

namespace dsrl {

namespace {

constexpr int kTempMaxK = 16;
constexpr int kTempMaxC = 60;               // 256 * C staged floats within the default 64 KB of LDS, as dsrl_calibration_from_logits
constexpr int kTempMaxBlocks = 1024;        // partial sums [block][1 + 3 K]; a block walks the 256-pixel tiles with the grid's stride
constexpr int kTempMaxEntries = 1 + 3 * kTempMaxK;
constexpr int kTempFinishGroups = kTempMaxBlocks / 64;

long long temp_tiles(long long P) { return ceil_div(P, 256); }
int temp_blocks(long long P) { return (int)std::min<long long>(kTempMaxBlocks, temp_tiles(P)); }

// Block b of the nb = min(1024, tiles) blocks takes the tiles b, b + nb, ... (nb is a function of P alone).  Thread i adds the terms of pixel i of each
// of them, in tile order; at the end the 256 threads are added by the xor tree of wave_sum_d and the four waves in ascending order: a fixed function of P.
template <int KT>
__global__ __launch_bounds__(256) void temperature_stats_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target,
                                                                 int ntiles, int last_np, int C, int ignore_index,
                                                                 const float* __restrict__ betas, int K, double* __restrict__ part,
                                                                 int* __restrict__ nan_flag, int vec_in) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // [256][C] logits, then d_c = v_c - m in place
    __shared__ float beta_s[kTempMaxK];
    __shared__ double red[4][kTempMaxEntries];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < kTempMaxK) beta_s[tid] = tid < K ? betas[tid] : 1.f;      // the betas of a call are uniform: read once per block
    double acc[3 * KT];
#pragma unroll
    for (int i = 0; i < 3 * KT; ++i) acc[i] = 0.0;
    unsigned cnt = 0u;
    bool bad = false, bad_label = false;
    for (int tl = (int)blockIdx.x; tl < ntiles; tl += (int)gridDim.x) {
        const int np = tl == ntiles - 1 ? last_np : 256;
        const long long p0 = (long long)tl * 256;
        const float* __restrict__ lg = logits + p0 * ld;                // the one 64-bit product of the tile
        const int nf = np * C;
        __syncthreads();
        if (vec_in) {           // dense rows: a tile is one contiguous run that starts on a 16-byte boundary
            const float4* src = reinterpret_cast<const float4*>(lg);
            for (int t = tid; t < (nf >> 2); t += 256) reinterpret_cast<float4*>(tile)[t] = src[t];
            for (int t = (nf & ~3) + tid; t < nf; t += 256) tile[t] = lg[t];
        } else {
            for (int t = tid; t < nf; t += 256) { const int r = t / C, c = t - r * C; tile[t] = lg[r * ld + c]; }
        }
        __syncthreads();
        if (tid < np) {
            const int tg = (int)(target + p0)[tid];
            bad_label |= tg != ignore_index && tg >= C;
            if (tg != ignore_index && tg < C) {
                float* v = tile + tid * C;
                float m = v[0];
                unsigned nb = abs_bits(v[0]);
                for (int c = 1; c < C; ++c) { m = fmaxf(m, v[c]); nb = max(nb, abs_bits(v[c])); }
                bad |= nb > 0x7f800000u;                                // fmaxf alone would skip a NaN; through d_c it reaches every sum
                for (int c = 0; c < C; ++c) v[c] = v[c] - m;
                const float dt = v[tg];
                cnt += 1u;
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) {
                        float L, G, H;
                        temperature_terms(v, C, dt, beta_s[k], L, G, H);
                        acc[3 * k] += (double)L;
                        acc[3 * k + 1] += (double)G;
                        acc[3 * k + 2] += (double)H;
                    }
            }
        }
    }
    if (nan_flag != nullptr && __any(bad) && lane == 0) atomicOr(nan_flag, 1);
    if (nan_flag != nullptr && __any(bad_label) && lane == 0) atomicOr(nan_flag, 2);
    const double n = wave_sum_d((double)cnt);
    if (lane == 0) red[wv][0] = n;
#pragma unroll
    for (int i = 0; i < 3 * KT; ++i) {
        const double s = wave_sum_d(acc[i]);
        if (lane == 0) red[wv][1 + i] = s;
    }
    __syncthreads();
    const int nent = 1 + 3 * K;
    if (tid < nent) part[(size_t)blockIdx.x * nent + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// One block of 16 x 64 threads, one thread per entry and group: thread (g, e) adds the partials of entry e over the blocks [64 g, 64 g + 64) in
// ascending order (the loads of a group do not depend on its sums; one thread walking 1024 blocks is a chain of 1024 memory latencies, see
// dice_finish_kernel); thread (0, e) then adds the 16 group sums in ascending g and adds the total to the caller's record - no atomics, the order a
// fixed function of the block index.  A beta that is not a finite number > 0 makes its own three entries NaN.
__global__ __launch_bounds__(kTempFinishGroups * 64) void temperature_finish_kernel(const double* __restrict__ part, int nblocks, const float* __restrict__ betas,
                                                                                    int K, double* __restrict__ record) {
    __shared__ double grp[kTempFinishGroups][64];
    const int e = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int nent = 1 + 3 * K;
    double s = 0.0;
    if (e < nent) {
        const int b1 = min(64 * g + 64, nblocks);
#pragma unroll 8
        for (int b = 64 * g; b < b1; ++b) s += part[(size_t)b * nent + e];
    }
    grp[g][e] = s;
    __syncthreads();
    if (g == 0 && e < nent) {
        s = 0.0;
        for (int j = 0; j < kTempFinishGroups; ++j) s += grp[j][e];
        if (e > 0) {
            const float b = betas[(e - 1) / 3];
            if (!(b > 0.f && b <= 3.402823466e+38f)) s = __builtin_nan("");
        }
        record[e] = record[e] + s;
    }
}

}  // namespace

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_temperature_max_points(void) { return kTempMaxK; }

extern "C" size_t dsrl_temperature_workspace_bytes(int64_t P, int K) {
    if (P <= 0 || K < 1 || K > kTempMaxK || temp_tiles(P) > INT_MAX) {
        set_error("temperature_workspace_bytes: bad arguments (P=%lld, K=%d)", (long long)P, K);
        return 0;
    }
    return (size_t)temp_blocks(P) * (1 + 3 * K) * sizeof(double);       // a function of (P, K) alone: holds for every launch of that pair
}

extern "C" int dsrl_temperature_stats(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* betas, int K,
                                      double* record, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(logits && target && betas && record && ws && P > 0 && C > 0 && ld >= C, DSRL_E_BADARG,
                 "temperature_stats: null pointer, empty shape or ld < C (C=%d, ld=%d)", C, ld);
    DSRL_REQUIRE(K >= 1 && K <= kTempMaxK, DSRL_E_BADARG, "temperature_stats: %d temperatures, 1 to %d are possible", K, kTempMaxK);
    DSRL_REQUIRE(C <= kTempMaxC, DSRL_E_UNSUPPORTED, "temperature_stats: %d classes, the staged logits fit the LDS up to %d", C, kTempMaxC);
    DSRL_REQUIRE(((uintptr_t)logits % 4) == 0 && ((uintptr_t)betas % 4) == 0 && ((uintptr_t)record % 8) == 0, DSRL_E_BADARG,
                 "temperature_stats: logits / betas not 4-byte aligned, or record not 8-byte aligned");
    DSRL_REQUIRE(temp_tiles(P) <= INT_MAX && (long long)256 * ld <= INT_MAX, DSRL_E_UNSUPPORTED,
                 "temperature_stats: P = %lld pixels or ld = %d beyond the 32-bit tile indices", (long long)P, ld);
    DSRL_REQUIRE(ws_bytes >= dsrl_temperature_workspace_bytes(P, K) && ((uintptr_t)ws % 8) == 0, DSRL_E_WORKSPACE,
                 "temperature_stats: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int ntiles = (int)temp_tiles(P), last_np = (int)(P - (int64_t)(ntiles - 1) * 256);
    const int nb = temp_blocks(P);
    const int vec_in = (ld == C && ((uintptr_t)logits % 16) == 0) ? 1 : 0;      // 256 * C floats per tile: every tile starts 16-byte aligned
    double* part = (double*)ws;
#define DSRL_TEMP_LAUNCH(KT)                                                                                                                       \
    hipLaunchKernelGGL(temperature_stats_kernel<KT>, dim3(nb), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, ntiles, last_np, \
                       C, ignore_index, betas, K, part, nan_flag, vec_in)
    if (K == 1) DSRL_TEMP_LAUNCH(1);
    else if (K == 2) DSRL_TEMP_LAUNCH(2);
    else if (K <= 4) DSRL_TEMP_LAUNCH(4);
    else if (K <= 8) DSRL_TEMP_LAUNCH(8);
    else DSRL_TEMP_LAUNCH(16);
#undef DSRL_TEMP_LAUNCH
    if (int e = launch_status("temperature_stats_kernel")) return e;
    hipLaunchKernelGGL(temperature_finish_kernel, dim3(1), dim3(kTempFinishGroups * 64), 0, st, (const double*)part, nb, betas, K, record);
    return launch_status("temperature_finish_kernel");
}
