// Online hard example mining (OHEM) for the cross entropy, as a rewrite of the target: the rule of mmseg's OHEMPixelSampler and
// HRNet's OhemCrossEntropy.  Three streaming steps, no CE kernel involved:
//     dsrl_ohem_prob     one pass over the logits -> p[i] = softmax probability of the target class of pixel i (kOhemSentinel where the pixel is no candidate)
//     dsrl_ohem_select   exact radix select on the bit patterns of p -> thr = max(k-th smallest p, thresh), and the counts, all on the device
//     dsrl_ohem_apply    target_out[i] = (candidate and p[i] >= thr) ? ignore_index : target[i]
// The rewritten target then goes to the CE paths as they are.  Everything below the probabilities is integer work: the result is a pure function
// of the inputs, the same bytes on every call.
#include "common.h"
#include <algorithm>
#include <string.h>

namespace dsrl {

constexpr float kOhemSentinel = 2.0f;           // p of a pixel that takes no part; every probability is <= 1
constexpr int kOhemHistBlocks = 256;            // partial histograms [block][256], the layout of class_hist_kernel's `part`
// the select's part of a workspace: the partial histograms, one partial count of p < thresh per block, the state of the passes
constexpr int kOhemStateWords = 16;             // [0] prefix of the k-th key found so far, [1] rank left inside that prefix, [2] keys below the prefix, [3] n, [4] keys below thresh
constexpr size_t kOhemSelectBytes = ((size_t)kOhemHistBlocks * 256 + kOhemHistBlocks + kOhemStateWords) * sizeof(unsigned);

// The key a probability is selected and compared by: its bit pattern, which orders non-negative floats as unsigned integers.  A NaN and anything
// not above zero (-0 included) is 0.  The same function forms the key of `thresh`.
__device__ __host__ __forceinline__ unsigned ohem_key_bits(float p, unsigned bits) { return p > 0.f ? bits : 0u; }
__device__ __forceinline__ unsigned ohem_key(float p) { return ohem_key_bits(p, __float_as_uint(p)); }
__device__ __forceinline__ bool ohem_candidate(float p) { return !(p >= kOhemSentinel); }         // (a NaN is a candidate, of key 0)

// ---------------------------------------------------------------------------------------------- probabilities
// The staging of ce_fused_kernel: a block takes 256 pixels x C logits through LDS (16-byte loads when the rows are dense and the base aligned), one
// thread per pixel, 32-bit indices inside the tile; and its arithmetic: m = max_c v_c, e_c = exp_nonpos(v_c - m), s = sum e_c with c ascending,
// p = e_t / s.  A NaN p (a NaN or +inf logit) is written as 0 - the hardest there is, so the pixel is kept and the CE pass that follows meets
// it - and raises bit 0 of nan_flag, as a NaN sum does in any pixel.
__global__ __launch_bounds__(256) void ohem_prob_kernel(const float* __restrict__ logits, int ld, const unsigned char* __restrict__ target, long long P, int C,
                                                         int ignore_index, float* __restrict__ p_out, int* __restrict__ nan_flag, int vec_in) {
    extern __shared__ __attribute__((aligned(16))) float tile[];         // [256][C]
    bool bad = false;
    for (long long p0 = (long long)blockIdx.x * 256; p0 < P; p0 += (long long)gridDim.x * 256) {
        const int np = (int)min(256ll, P - p0);
        const int nf = np * C;
        __syncthreads();
        if (vec_in) {           // dense rows: 256 pixels are one contiguous run that starts on a 16-byte boundary
            const float4* src = reinterpret_cast<const float4*>(logits + p0 * C);
            for (int t = threadIdx.x; t < (nf >> 2); t += 256) reinterpret_cast<float4*>(tile)[t] = src[t];
            for (int t = (nf & ~3) + threadIdx.x; t < nf; t += 256) tile[t] = logits[p0 * C + t];
        } else {
            for (int t = threadIdx.x; t < nf; t += 256) { const int r = t / C, c = t - r * C; tile[t] = logits[(p0 + r) * ld + c]; }
        }
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int tg = target[p0 + threadIdx.x];
            const float* v = tile + threadIdx.x * C;
            float m = v[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += exp_nonpos(v[c] - m);
            bad |= !(s == s);                   // any NaN logit poisons the sum (fmaxf alone would skip it)
            const bool cand = tg != ignore_index && tg < C;
            const float p = exp_nonpos(v[cand ? tg : 0] - m) / s;
            p_out[p0 + threadIdx.x] = cand ? (p == p ? p : 0.f) : kOhemSentinel;
        }
    }
    if (nan_flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(nan_flag, 1);
}

// ---------------------------------------------------------------------------------------------- radix select
// Pass `pass` (0..3) looks at digit (key >> (24 - 8 pass)) & 255 of the candidates whose higher digits equal those of state[0] (pass 0: of all of
// them).  Per-wave LDS bins as class_hist_kernel; the block's 256 bins leave as its own row of `part`, nothing to zero, merged in integers by
// ohem_pick_kernel.  Pass 0 also counts the candidates below `thresh` (lt_part[block]).  16-byte loads over the aligned body of p, the head up to
// the first 16-byte boundary and the tail element by element by block 0.
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ p, long long P, int pass, unsigned thresh_bits,
                                                         const unsigned* __restrict__ state, unsigned* __restrict__ part, unsigned* __restrict__ lt_part) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned sh_lt[4];
    for (int t = threadIdx.x; t < 4 * 256; t += 256) (&hist[0][0])[t] = 0u;
    __syncthreads();
    unsigned* h = hist[threadIdx.x >> 6];
    const int shift = 24 - 8 * pass;
    const unsigned want = pass ? state[0] >> (shift + 8) : 0u;
    unsigned lt = 0;
    auto take = [&](float x) {
        if (!ohem_candidate(x)) return;
        const unsigned key = ohem_key(x);
        if (pass == 0) { lt += key < thresh_bits ? 1u : 0u; atomicAdd(&h[key >> 24], 1u); }
        else if ((key >> (shift + 8)) == want) atomicAdd(&h[(key >> shift) & 0xffu], 1u);
    };
    const long long head = min(P, (long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2));
    const long long nv = (P - head) >> 2;
    const float4* v = reinterpret_cast<const float4*>(p + head);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long long)gridDim.x * 256) {
        const float4 q = v[e];
        take(q.x); take(q.y); take(q.z); take(q.w);
    }
    if (blockIdx.x == 0) {
        for (long long e = threadIdx.x; e < head; e += 256) take(p[e]);
        for (long long e = head + (nv << 2) + threadIdx.x; e < P; e += 256) take(p[e]);
    }
    __syncthreads();
    part[(long long)blockIdx.x * 256 + threadIdx.x] = hist[0][threadIdx.x] + hist[1][threadIdx.x] + hist[2][threadIdx.x] + hist[3][threadIdx.x];
    if (pass == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lt += __shfl_xor(lt, o, 64);
        if ((threadIdx.x & 63) == 0) sh_lt[threadIdx.x >> 6] = lt;
        __syncthreads();
        if (threadIdx.x == 0) lt_part[blockIdx.x] = sh_lt[0] + sh_lt[1] + sh_lt[2] + sh_lt[3];
    }
}
// One block: thread d sums bin d over the nb partial histograms, a scan over the 256 bins finds the digit that holds the rank, and the state moves
// on: prefix |= digit << shift, rank -= keys below the digit, below += the same.  Pass 0 forms n (all bins), k = min(min_kept, n - 1) and the count
// below thresh; pass 3 has the whole key v of the k-th smallest p and writes stats = {bits of thr = max(v, thresh), n, kept, below thresh}, where
// kept = #(key < thr) is the keys below v when thr == v and the count below thresh otherwise.  n == 0: v = 0, thr = thresh, zeros.
__global__ __launch_bounds__(256) void ohem_pick_kernel(const unsigned* __restrict__ part, int nb, const unsigned* __restrict__ lt_part, int pass,
                                                         unsigned thresh_bits, long long min_kept, unsigned* __restrict__ state, unsigned* __restrict__ stats) {
    __shared__ unsigned scan[256];
    __shared__ unsigned sh_lt, sh_digit, sh_below;
    const int t = threadIdx.x;
    unsigned c = 0;
    for (int b = 0; b < nb; ++b) c += part[b * 256 + t];
    scan[t] = c;
    if (t == 0) { sh_lt = 0u; sh_digit = 0u; sh_below = 0u; }
    __syncthreads();
    if (pass == 0 && t < nb) atomicAdd(&sh_lt, lt_part[t]);          // (integers: any order gives the same sum)
    for (int o = 1; o < 256; o <<= 1) {                               // inclusive scan
        const unsigned a = t >= o ? scan[t - o] : 0u;
        __syncthreads();
        scan[t] += a;
        __syncthreads();
    }
    const unsigned total = scan[255];
    unsigned rank;
    if (pass == 0) rank = total ? (unsigned)min((long long)(total - 1), min_kept) : 0u;
    else rank = state[1];
    const unsigned incl = scan[t], excl = incl - c;
    if (excl <= rank && rank < incl) { sh_digit = (unsigned)t; sh_below = excl; }        // exactly one thread, or none when there is no candidate
    __syncthreads();
    if (t == 0) {
        const int shift = 24 - 8 * pass;
        const unsigned prefix = (pass ? state[0] : 0u) | (sh_digit << shift);
        const unsigned below = (pass ? state[2] : 0u) + sh_below;
        const unsigned n = pass ? state[3] : total, n_lt = pass ? state[4] : sh_lt;
        state[0] = prefix; state[1] = rank - sh_below; state[2] = below; state[3] = n; state[4] = n_lt;
        if (pass == 3) {
            const unsigned thr = max(prefix, thresh_bits);
            stats[0] = thr; stats[1] = n; stats[2] = thr == prefix ? below : n_lt; stats[3] = n_lt;
        }
    }
}

// ---------------------------------------------------------------------------------------------- the rewritten target
// kept iff key(p) < thr, strictly; a pixel that is no candidate keeps its label.  Four pixels per thread as one 16-byte and two 4-byte accesses
// when the three buffers allow it.  target_out may be target itself.
__device__ __forceinline__ unsigned char ohem_label(float p, unsigned char tg, unsigned thr, unsigned char ig) {
    return (!ohem_candidate(p) || ohem_key(p) < thr) ? tg : ig;
}
__global__ __launch_bounds__(256) void ohem_apply_kernel(const float* __restrict__ p, const unsigned char* target, long long P, int ignore_index,
                                                          const unsigned* __restrict__ stats, unsigned char* target_out, int vec) {
    const unsigned thr = stats[0];
    const unsigned char ig = (unsigned char)ignore_index;
    const long long nv = vec ? P >> 2 : 0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nv; e += (long long)gridDim.x * 256) {
        const float4 q = reinterpret_cast<const float4*>(p)[e];
        const uchar4 tg = reinterpret_cast<const uchar4*>(target)[e];
        reinterpret_cast<uchar4*>(target_out)[e] = make_uchar4(ohem_label(q.x, tg.x, thr, ig), ohem_label(q.y, tg.y, thr, ig), ohem_label(q.z, tg.z, thr, ig),
                                                                ohem_label(q.w, tg.w, thr, ig));
    }
    for (long long e = (nv << 2) + (long long)blockIdx.x * 256 + threadIdx.x; e < P; e += (long long)gridDim.x * 256)
        target_out[e] = ohem_label(p[e], target[e], thr, ig);
}

static int ohem_prob_blocks(long long P) { return (int)std::max<long long>(1, std::min<long long>(1024, ceil_div(P, 256))); }     // loss_blocks of losses.hip
static int ohem_hist_blocks(long long P) { return (int)std::max<long long>(1, std::min<long long>(kOhemHistBlocks, ceil_div(P, 4096))); }
static unsigned ohem_thresh_bits(float thresh) { unsigned b; memcpy(&b, &thresh, sizeof b); return ohem_key_bits(thresh, b); }

static int launch_ohem_prob(const float* logits, int ld, const uint8_t* target, long long P, int C, int ignore_index, float* p_out, int* nan_flag, hipStream_t st) {
    const int vec_in = (ld == C && ((uintptr_t)logits % 16) == 0) ? 1 : 0;          // 256 * C floats per tile: every tile starts 16-byte aligned
    hipLaunchKernelGGL(ohem_prob_kernel, dim3(ohem_prob_blocks(P)), dim3(256), (size_t)256 * C * sizeof(float), st, logits, ld, target, P, C, ignore_index,
                       p_out, nan_flag, vec_in);
    return launch_status("ohem_prob_kernel");
}
// eight launches, none of them conditional: the sequence can be captured
static int launch_ohem_select(const float* p, long long P, float thresh, long long min_kept, unsigned* stats, void* ws, hipStream_t st) {
    unsigned* part = (unsigned*)ws;
    unsigned* lt_part = part + (size_t)kOhemHistBlocks * 256;
    unsigned* state = lt_part + kOhemHistBlocks;
    const int nb = ohem_hist_blocks(P);
    const unsigned tb = ohem_thresh_bits(thresh);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(ohem_hist_kernel, dim3(nb), dim3(256), 0, st, p, P, pass, tb, (const unsigned*)state, part, lt_part);
        if (int e = launch_status("ohem_hist_kernel")) return e;
        hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)part, nb, (const unsigned*)lt_part, pass, tb, min_kept, state, stats);
        if (int e = launch_status("ohem_pick_kernel")) return e;
    }
    return DSRL_OK;
}
static int launch_ohem_apply(const float* p, const uint8_t* target, long long P, int ignore_index, const unsigned* stats, uint8_t* target_out, hipStream_t st) {
    const int vec = (((uintptr_t)p % 16) == 0 && ((uintptr_t)target % 4) == 0 && ((uintptr_t)target_out % 4) == 0) ? 1 : 0;
    const int nb = (int)std::max<long long>(1, std::min<long long>(2048, ceil_div(P, 1024)));
    hipLaunchKernelGGL(ohem_apply_kernel, dim3(nb), dim3(256), 0, st, p, target, P, ignore_index, stats, target_out, vec);
    return launch_status("ohem_apply_kernel");
}

}  // namespace dsrl
using namespace dsrl;

// the checks the entry points share, scalars first (as gamma and eps of the CE entry points), each in the caller's name
#define DSRL_OHEM_P(P, what) DSRL_REQUIRE((P) <= 0x7fffffffll, DSRL_E_BADARG, what ": P = %lld does not fit the 32-bit counts", (long long)(P))
#define DSRL_OHEM_THRESH(thresh, what) \
    DSRL_REQUIRE((thresh) >= 0.f && (thresh) <= 1.f, DSRL_E_BADARG, what ": thresh = %g is not a number in [0, 1]", (double)(thresh))
#define DSRL_OHEM_MIN_KEPT(min_kept, what) DSRL_REQUIRE((min_kept) >= 0, DSRL_E_BADARG, what ": min_kept = %lld is negative", (long long)(min_kept))
#define DSRL_OHEM_IGNORE(ignore_index, what) \
    DSRL_REQUIRE((ignore_index) >= 0 && (ignore_index) <= 255, DSRL_E_BADARG, what ": ignore_index = %d is not a byte value 0..255", (int)(ignore_index))

extern "C" size_t dsrl_ohem_workspace_bytes(int64_t P) {
    if (P <= 0 || P > 0x7fffffffll) { set_error("ohem_workspace_bytes: bad arguments (P=%lld)", (long long)P); return 0; }
    return kOhemSelectBytes + align_up((size_t)P * sizeof(float), 16);
}
extern "C" int dsrl_ohem_prob(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float* p_out, int* nan_flag,
                              dsrl_stream_t stream) {
    DSRL_OHEM_IGNORE(ignore_index, "ohem_prob");
    DSRL_REQUIRE(logits && target && p_out && P > 0 && C > 0 && C <= 60 && ld >= C && ((uintptr_t)p_out % 4) == 0, DSRL_E_BADARG,
                 "ohem_prob: bad arguments (C=%d)", C);
    DSRL_OHEM_P(P, "ohem_prob");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    return launch_ohem_prob(logits, ld, target, (long long)P, C, ignore_index, p_out, nan_flag, st);
}
extern "C" int dsrl_ohem_select(const float* p, int64_t P, float thresh, int64_t min_kept, uint32_t* stats, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_OHEM_THRESH(thresh, "ohem_select");
    DSRL_OHEM_MIN_KEPT(min_kept, "ohem_select");
    DSRL_REQUIRE(p && stats && ws && P > 0 && ((uintptr_t)p % 4) == 0 && ((uintptr_t)stats % 4) == 0, DSRL_E_BADARG, "ohem_select: bad arguments");
    DSRL_OHEM_P(P, "ohem_select");
    DSRL_REQUIRE(ws_bytes >= kOhemSelectBytes && ((uintptr_t)ws % 16) == 0, DSRL_E_WORKSPACE, "ohem_select: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    return launch_ohem_select(p, (long long)P, thresh, (long long)min_kept, stats, ws, st);
}
extern "C" int dsrl_ohem_apply(const float* p, const uint8_t* target, int64_t P, int ignore_index, const uint32_t* stats, uint8_t* target_out,
                               dsrl_stream_t stream) {
    DSRL_OHEM_IGNORE(ignore_index, "ohem_apply");
    DSRL_REQUIRE(p && target && stats && target_out && P > 0 && ((uintptr_t)p % 4) == 0 && ((uintptr_t)stats % 4) == 0, DSRL_E_BADARG,
                 "ohem_apply: bad arguments");
    DSRL_OHEM_P(P, "ohem_apply");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    return launch_ohem_apply(p, target, (long long)P, ignore_index, stats, target_out, st);
}
extern "C" int dsrl_ohem_target(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float thresh, int64_t min_kept,
                                uint8_t* target_out, uint32_t* stats, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_OHEM_THRESH(thresh, "ohem_target");
    DSRL_OHEM_MIN_KEPT(min_kept, "ohem_target");
    DSRL_OHEM_IGNORE(ignore_index, "ohem_target");
    DSRL_REQUIRE(logits && target && target_out && stats && ws && P > 0 && C > 0 && C <= 60 && ld >= C && ((uintptr_t)stats % 4) == 0, DSRL_E_BADARG,
                 "ohem_target: bad arguments (C=%d)", C);
    DSRL_OHEM_P(P, "ohem_target");
    DSRL_REQUIRE(ws_bytes >= dsrl_ohem_workspace_bytes(P) && ((uintptr_t)ws % 16) == 0, DSRL_E_WORKSPACE, "ohem_target: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    float* p = (float*)((char*)ws + kOhemSelectBytes);                  // (a multiple of 16 bytes: the body of p takes the 16-byte loads)
    if (int e = launch_ohem_prob(logits, ld, target, (long long)P, C, ignore_index, p, nan_flag, st)) return e;
    if (int e = launch_ohem_select(p, (long long)P, thresh, (long long)min_kept, stats, ws, st)) return e;
    return launch_ohem_apply(p, target, (long long)P, ignore_index, stats, target_out, st);
}
