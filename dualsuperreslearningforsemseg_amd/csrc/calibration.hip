// Calibration record and confidence map from logits in memory (include/dsrl_hip.h, "calibration"): the stand-alone producer beside the fused inference
// tails (predict.hip, merge.hip), for validation inside training and any caller who has logits.  One streaming pass, no host work, capturable.
//
// Addressing of seg_metrics_kernel (losses.hip): a block stages 256 pixels x C logits into LDS by coalesced loads (the logits are pixel-major, a
// thread's own C floats would be a C-strided gather), then a thread owns one pixel: first maximum, softmax denominator (softmax_denominator: the fmaxf
// chain and the ascending sum of exp_nonpos, the arithmetic of every CE kernel and of the single-view tail), confidence_pixel, calibration_bin.
// Inside the chunk loop every index is a 32-bit integer: the chunk's base pointers are formed once per chunk, and a chunk is at most 256 * ld floats.
// The record goes through per-block LDS integers (CalBins) and one 64-bit atomic per block and non-zero entry: bit-identical run to run.
#include "common.h"
#include <algorithm>
#include <limits.h>

namespace dsrl {

namespace {

constexpr int kCalMaxC = 60;            // 256 * C staged floats within the default 64 KB of LDS, as dsrl_seg_metrics
constexpr int kCalBlocks = 1024;

// TEMP (dsrl_calibration_from_logits_t): behind the first-maximum search the pixel's logits become v_c * beta in place (temperature_scale), and the
// confidence is that of softmax(beta v) through the same arithmetic - what the TEMP builds of the fused tail (predict.hip) report, bit for bit.
template <bool TEMP>
__global__ __launch_bounds__(256) void calibration_from_logits_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target,
                                                                      int nchunks, int last_np, int C, int ignore_index, int B,
                                                                      unsigned long long* __restrict__ record, float* __restrict__ conf_map,
                                                                      int* __restrict__ nan_flag, float beta) {
    extern __shared__ float tile[];                     // [256][C] logits
    __shared__ CalBins bins;
    const int tid = threadIdx.x;
    const bool rec = record != nullptr;
    if (rec) bins.clear(B);
    bool bad = false, bad_label = false;
    for (int ch = (int)blockIdx.x; ch < nchunks; ch += (int)gridDim.x) {
        const int np = ch == nchunks - 1 ? last_np : 256;
        const long long p0 = (long long)ch * 256;
        const float* __restrict__ lg = logits + p0 * ld;            // the one 64-bit product of the chunk
        __syncthreads();
        if (ld == C) {
            for (int t = tid; t < np * C; t += 256) tile[t] = lg[t];
        } else {
            for (int t = tid; t < np * C; t += 256) { const int r = t / C, c = t - r * C; tile[t] = lg[r * ld + c]; }
        }
        __syncthreads();
        if (tid < np) {
            float* v = tile + tid * C;
            int best = 0;
            float bv = v[0];
            for (int c = 1; c < C; ++c)
                if (v[c] > bv) { bv = v[c]; best = c; }             // first maximum, as seg_metrics_kernel and torch.argmax
            if (TEMP)
                for (int c = 0; c < C; ++c) v[c] = temperature_scale(v[c], beta);
            const float conf = confidence_pixel(softmax_denominator<0>(v, C));
            bad |= !(conf == conf);                                 // any NaN logit poisons the sum
            if (conf_map != nullptr) (conf_map + p0)[tid] = conf;
            if (rec) {
                const int tg = (int)(target + p0)[tid];
                bad_label |= tg != ignore_index && tg >= C;
                if (tg != ignore_index && tg < C) bins.count(conf, best == tg, B);
            }
        }
    }
    if (nan_flag != nullptr && __any(bad) && (tid & 63) == 0) atomicOr(nan_flag, 1);
    if (nan_flag != nullptr && __any(bad_label) && (tid & 63) == 0) atomicOr(nan_flag, 2);
    if (rec) {
        __syncthreads();
        bins.flush(record, B);
    }
}

}  // namespace

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_calibration_max_bins(void) { return kCalMaxBins; }

// both entry points: `temp` selects the build that scales the logits by beta
static int calibration_launch(bool temp, float beta, const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, int B,
                              unsigned long long* record, float* conf_map, int* nan_flag, dsrl_stream_t stream) {
    DSRL_REQUIRE(logits && P > 0 && C > 0 && ld >= C && (record || conf_map), DSRL_E_BADARG,
                 "calibration_from_logits: null logits, empty shape, ld < C, or neither a record nor a confidence map (C=%d)", C);
    DSRL_REQUIRE(!record || target, DSRL_E_BADARG, "calibration_from_logits: the record needs a target");
    DSRL_REQUIRE(C <= kCalMaxC, DSRL_E_UNSUPPORTED, "calibration_from_logits: %d classes, the staged logits fit the LDS up to %d", C, kCalMaxC);
    DSRL_REQUIRE(!record || (B >= 1 && B <= kCalMaxBins), DSRL_E_BADARG, "calibration_from_logits: %d bins, 1 to %d are possible", B, kCalMaxBins);
    DSRL_REQUIRE(((uintptr_t)logits % 4) == 0 && ((uintptr_t)conf_map % 4) == 0 && ((uintptr_t)record % 8) == 0, DSRL_E_BADARG,
                 "calibration_from_logits: logits / conf_map not 4-byte aligned, or record not 8-byte aligned");
    DSRL_REQUIRE(ceil_div(P, 256) <= INT_MAX && (long long)256 * ld <= INT_MAX, DSRL_E_UNSUPPORTED,
                 "calibration_from_logits: P = %lld pixels or ld = %d beyond the 32-bit chunk indices", (long long)P, ld);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int nchunks = (int)ceil_div(P, 256), last_np = (int)(P - (int64_t)(nchunks - 1) * 256);
    const int nb = std::min(kCalBlocks, nchunks);
    if (temp)
        hipLaunchKernelGGL(calibration_from_logits_kernel<true>, dim3(nb), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, nchunks,
                           last_np, C, ignore_index, record ? B : 1, record, conf_map, nan_flag, beta);
    else
        hipLaunchKernelGGL(calibration_from_logits_kernel<false>, dim3(nb), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, nchunks,
                           last_np, C, ignore_index, record ? B : 1, record, conf_map, nan_flag, 1.f);
    return launch_status("calibration_from_logits_kernel");
}

extern "C" int dsrl_calibration_from_logits(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, int B,
                                            unsigned long long* record, float* conf_map, int* nan_flag, dsrl_stream_t stream) {
    return calibration_launch(false, 1.f, logits, ld, target, P, C, ignore_index, B, record, conf_map, nan_flag, stream);
}

// the record and the map of softmax(beta v), beta = 1 / T a finite number > 0 (include/dsrl_hip.h, "temperature")
extern "C" int dsrl_calibration_from_logits_t(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, int B,
                                              unsigned long long* record, float* conf_map, int* nan_flag, float beta, dsrl_stream_t stream) {
    DSRL_TEMPERATURE_BETA(beta, "calibration_from_logits_t");
    return calibration_launch(true, beta, logits, ld, target, P, C, ignore_index, B, record, conf_map, nan_flag, stream);
}
