// What the inference ensembles share (merge.hip: multi-scale; window.hip: sliding window): the limits of a launch, the span mapping's block count, the
// softmax of one pixel and the finalize of the loss.  Both ensembles go through merge_softmax, so a view contributes the same bits to either: a single
// whole-image window IS a single identity view of dsrl_prob_merge_finish.
#pragma once
#include "common.h"
#include <algorithm>

namespace dsrl {

constexpr int kMergeMaxC = 32;
constexpr int kMergeMaxBlocks = 2048;       // eight blocks of 4 waves per CU
constexpr int kMergeStageFloats = 2304;     // per wave: 121 source columns of 19 floats

// p[c] <- softmax_c of the lane's C logits in p (m: their maximum, the fmaxf chain from -inf in ascending c); entries c >= C of the 32-wide
// instantiation become 0.  exp_nonpos of the max-subtracted logit, the sum in ascending c, one reciprocal, one product per class (the library is
// built with -ffp-contract=off).  A NaN logit makes every p[c] NaN; a wave without a span passes zeros with m = 0 and gets 1 / CT, which it drops.
template <int CT>
__device__ __forceinline__ void merge_softmax(float (&p)[CT], int C, float m) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (CT == kMergeMaxC && c >= C) { p[c] = 0.f; continue; }
        p[c] = exp_nonpos(p[c] - m);
        sum += p[c];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < CT; ++c) p[c] *= inv;
}

// a wave owns 64 consecutive pixels of one row: spans per row of W pixels, and the blocks (4 waves each) of a launch over N x H rows
static inline int merge_spans_per_row(int W) { return (int)ceil_div(W, 64); }
static inline int merge_blocks(int N, int H, int W) {
    const long long spans = (long long)N * H * merge_spans_per_row(W);
    return (int)std::max<long long>(1, std::min<long long>(kMergeMaxBlocks, ceil_div(spans, 4)));
}

// merge.hip: out = [sum of the per-block loss partials / sum of their pixel counts, that count], the nb pairs of `part` added in block order
int launch_merge_ce_finalize(const double* part, int nb, float* out, hipStream_t st);

}  // namespace dsrl
