// Boundary label relaxation: the class-set word of every pixel, the input of the relaxed cross entropy (the dsrl_*_r entry
// points; relax_pixel / relax_grad in common.h).  mask[i] = OR of (1 << label) over the live labels < C in the (2r+1) x (2r+1) window around pixel i,
// clipped at the borders of the pixel's own image; 0 for a pixel that is ignored or whose label is >= C.  Integer work only.
//
// A block takes a 64 x 16 tile of one image.  Labels -> bits for the tile and its halo of r pixels into LDS (zeros outside the image, so a window
// neither crosses into the next image nor wraps a row), then a separable OR: a row pass over the (16 + 2r) rows, a column pass over the tile.  A
// thread's position is (tid & 63, tid >> 6): no division per element; the three divisions that place the block are per block and 32-bit.  The
// words leave as 4-byte stores, a wave writing 256 contiguous bytes of a row.
// stats (optional): {live pixels, pixels with more than one class in their set} ADDED to what is there: per wave a shuffle sum, per block two LDS
// integers, then one 64-bit atomic per counter and block - integers, so the record does not depend on the order of the blocks.
#include "common.h"

namespace dsrl {

constexpr int kRxTW = 64, kRxTH = 16;
constexpr int kRxLW = kRxTW + 2 * kRelaxMaxRadius, kRxLH = kRxTH + 2 * kRelaxMaxRadius;

__global__ __launch_bounds__(256) void relax_mask_kernel(const unsigned char* __restrict__ target, int H, int W, int C, int ignore_index, int r, int nbx, int nby,
                                                          unsigned* __restrict__ mask, unsigned long long* __restrict__ stats) {
    __shared__ unsigned bits[kRxLH][kRxLW];
    __shared__ unsigned rows[kRxLH][kRxTW];
    __shared__ unsigned cnt[2];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const unsigned b = blockIdx.x;
    const unsigned bx = b % (unsigned)nbx, q = b / (unsigned)nbx;
    const unsigned by = q % (unsigned)nby, n = q / (unsigned)nby;
    const int x0 = (int)bx * kRxTW, y0 = (int)by * kRxTH;
    const long long img0 = (long long)n * H * W;
    const unsigned char* __restrict__ img = target + img0;
    const int lw = kRxTW + 2 * r, lh = kRxTH + 2 * r;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
    for (int ly = ty; ly < lh; ly += 4) {
        const int gy = y0 + ly - r;
        for (int lx = tx; lx < lw; lx += 64) {
            const int gx = x0 + lx - r;
            unsigned w = 0u;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int lbl = img[(long long)gy * W + gx];
                if (lbl != ignore_index && lbl < C) w = 1u << lbl;
            }
            bits[ly][lx] = w;
        }
    }
    __syncthreads();
    for (int ly = ty; ly < lh; ly += 4) {
        unsigned o = 0u;
        for (int d = 0; d <= 2 * r; ++d) o |= bits[ly][tx + d];
        rows[ly][tx] = o;
    }
    __syncthreads();
    unsigned live_n = 0u, multi_n = 0u;
    const int gx = x0 + tx;
    for (int oy = ty; oy < kRxTH; oy += 4) {
        const int gy = y0 + oy;
        if (gy < H && gx < W) {
            unsigned o = 0u;
            for (int d = 0; d <= 2 * r; ++d) o |= rows[oy + d][tx];
            const long long i = (long long)gy * W + gx;
            const int lbl = img[i];
            const bool live = lbl != ignore_index;
            o = (live && lbl < C) ? o : 0u;         // (a live label < C has its own bit in the window: the set is o itself)
            mask[img0 + i] = o;
            live_n += live ? 1u : 0u;
            multi_n += __popc(o) > 1 ? 1u : 0u;
        }
    }
    if (stats) {                                    // uniform
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { live_n += __shfl_xor(live_n, o, 64); multi_n += __shfl_xor(multi_n, o, 64); }
        if (tx == 0) { if (live_n) atomicAdd(&cnt[0], live_n); if (multi_n) atomicAdd(&cnt[1], multi_n); }
        __syncthreads();
        if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    }
}

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_relax_mask(const uint8_t* target, int N, int H, int W, int C, int ignore_index, int radius, uint32_t* mask, unsigned long long* stats,
                               dsrl_stream_t stream) {
    DSRL_REQUIRE(radius >= 1 && radius <= kRelaxMaxRadius, DSRL_E_BADARG, "relax_mask: radius = %d is not in [1, %d]", radius, kRelaxMaxRadius);
    DSRL_REQUIRE(C >= 1 && C <= kRelaxMaxC, DSRL_E_BADARG, "relax_mask: C = %d is not in [1, %d]", C, kRelaxMaxC);
    DSRL_REQUIRE(target && mask && N > 0 && H > 0 && W > 0 && ((uintptr_t)mask % 4) == 0 && ((uintptr_t)stats % 8) == 0, DSRL_E_BADARG, "relax_mask: bad arguments");
    const int nbx = (int)ceil_div(W, kRxTW), nby = (int)ceil_div(H, kRxTH);
    const int64_t blocks = (int64_t)N * nbx * nby;
    DSRL_REQUIRE(blocks < (1ll << 31), DSRL_E_UNSUPPORTED, "relax_mask: N=%d H=%d W=%d needs too many blocks", N, H, W);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(relax_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, st, target, H, W, C, ignore_index, radius, nbx, nby, mask, stats);
    return launch_status("relax_mask_kernel");
}
