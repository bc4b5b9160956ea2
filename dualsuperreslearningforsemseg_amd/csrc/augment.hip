// Random joint augmentations of the reference's training transform (command_handlers/train_or_resume.py:128-137) on the device.
//
// dsrl_augment_geometry: JointRandomRotate (PIL rotate, bilinear image / nearest labels, expand=False) followed by JointRandomCrop's PIL branch
// (resize of a crop box back to the full size, bilinear image / nearest labels), Pillow-exact on uint8.  One fused pass: every output pixel
// evaluates the rotated pixels its crop-resize taps read, so no rotated image is ever written.
//   rotate, image:   Pillow's generic transform with the bilinear filter (Geometry.c): source point in double at the pixel centre, fill outside
//                    [0,W)x[0,H), otherwise the two-row bilinear blend in double, truncated to uint8;
//   rotate, labels:  Pillow's 16.16 fixed-point affine path (nearest), fill 255 outside;
//   crop, image:     Pillow's two-pass resample (Resample.c): horizontal first into a uint8 intermediate, then vertical; 22-bit integer taps
//                    from the bilinear filter, normalised in double per output index;
//   crop, labels:    Pillow's nearest scale path (ImagingScaleAffine): the source column of output column i is int(xo_i) with xo_0 = box0 +
//                    0.5 * box_len / out_len and xo_{i+1} = xo_i + box_len / out_len summed in double one step at a time - the closed form
//                    box0 + (i + 0.5) * box_len / out_len differs from it for some boxes, and a sequential sum does not parallelise, so the host
//                    computes these indices (label_src) with the same sums.
// dsrl_prepare_batch_augmented: dsrl_prepare_batch with JointHFlip, JointRandomGaussianBlur (torchvision GaussianBlur, 3x3, reflect padding) and
// JointRandomGrayscale folded in.  The blur is evaluated only at the full-resolution taps the align-corners resize reads, the flip is a mirrored
// column index, and the grayscale is applied after the (linear) resize; with every flag off the arithmetic is prepare_image_kernel's, bit for bit.
// dsrl_colour_jitter_means + dsrl_prepare_batch_jittered: JointColorJitter (models/transforms/JointColorJitter.py; commented out in the reference's
// compose, between JointImageAndLabelTensor and JointHFlip) as an opt-in stage of the same tail.  Brightness, contrast, saturation (torchvision 0.8.1
// functional_tensor) and the reference's hue rotation matrix, in the per-sample order of a 64-byte row (dsrl_colour_jitter_params), each followed
// by a clamp.  All four are pointwise but for contrast's mean of gray over the whole sample, so the jitter is applied to every uint8 pixel as a
// tap fetches it (4 bilinear taps per output pixel, x9 under blur: the blur reads jittered pixels) and no float copy of the full-size image is
// written; the mean comes from a two-kernel reduction (per-block double partials, then one wave per sample in a fixed order: the same bits on
// every call, no atomics).  The operations are homogeneous, so they run in the kernel's 0..255 scale with clamps at 255 and the mean x 255.
// prepare_image_aug_kernel<false> is what dsrl_prepare_batch_augmented launches: the arithmetic it always had.
// Index arithmetic is 32-bit within a sample (one sample: < 2^31 bytes); the sample offset is the only 64-bit product.
#include "common.h"

namespace dsrl {

static_assert(sizeof(dsrl_augment_params) == 128, "dsrl_augment_params is a 128-byte table row");
static_assert(sizeof(dsrl_colour_jitter_params) == 64, "dsrl_colour_jitter_params is a 64-byte table row");

// ---------------------------------------------------------------------------------------------- geometry
// Pillow's bilinear rotate of one output pixel (x, y) of the rotated image: 3 channels, fill 0 outside.
__device__ __forceinline__ void rotate_bilinear_rgb(const unsigned char* __restrict__ img, const double* __restrict__ m, int W, int H, int x, int y, int v[3]) {
    const double xin = (double)x + 0.5, yin = (double)y + 0.5;
    double xi = m[0] * xin + m[1] * yin + m[2];
    double yi = m[3] * xin + m[4] * yin + m[5];
    if (!(xi >= 0.0 && xi < (double)W && yi >= 0.0 && yi < (double)H)) {       // the negated form also sends a NaN to the fill
        v[0] = v[1] = v[2] = 0;
        return;
    }
    xi -= 0.5; yi -= 0.5;
    const double fx = floor(xi), fy = floor(yi);
    const int ix = (int)fx, iy = (int)fy;
    const double dx = xi - fx, dy = yi - fy;
    const int x0 = min(max(ix, 0), W - 1), x1 = min(max(ix + 1, 0), W - 1);
    const int y0 = min(max(iy, 0), H - 1);
    const int y1 = (iy + 1 >= 0 && iy + 1 < H) ? iy + 1 : y0;       // Pillow repeats the first row when the second falls outside
    const unsigned char* r0 = img + y0 * W * 3;
    const unsigned char* r1 = img + y1 * W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a0 = r0[x0 * 3 + c], b0 = r0[x1 * 3 + c];
        const double a1 = r1[x0 * 3 + c], b1 = r1[x1 * 3 + c];
        const double t0 = a0 + (b0 - a0) * dx;
        const double t1 = a1 + (b1 - a1) * dx;
        v[c] = (int)(t0 + (t1 - t0) * dy);                               // (UINT8)v: truncation
    }
}

// Pillow's bilinear resample taps of one output index: first source index, tap count (<= 3) and 22-bit integer weights.
__device__ __forceinline__ int crop_taps(int i, int box0, int boxlen, int n_in, int n_out, int k[3]) {
    const double scale = (double)boxlen / (double)n_out;                 // filterscale = 1 (an up-sampling crop), support = 1
    const double center = (double)box0 + ((double)i + 0.5) * scale;
    int xmin = (int)(center - 1.0 + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + 1.0 + 0.5);
    if (xmax > n_in) xmax = n_in;
    xmax -= xmin;
    xmax = min(max(xmax, 0), 3);
    double w[3] = {0.0, 0.0, 0.0};
    double ww = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < xmax) {
            double a = ((double)(j + xmin) - center) + 0.5;
            if (a < 0.0) a = -a;
            w[j] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double wn = ww != 0.0 ? w[j] / ww : w[j];
        k[j] = (int)(0.5 + wn * 4194304.0);                             // 1 << PRECISION_BITS (22); the weights are never negative here
    }
    return xmin;
}

__device__ __forceinline__ int clip8(int v) { return v >= (255 << 22) ? 255 : (v <= 0 ? 0 : (v >> 22)); }

// grid (ceil(Ws / 256), Hs, N): one thread per output pixel, a block per row segment (the row taps are uniform across the block)
__global__ __launch_bounds__(256) void augment_geometry_kernel(const unsigned char* __restrict__ rgb, const unsigned char* __restrict__ labels,
                                                                const dsrl_augment_params* __restrict__ params, const int* __restrict__ label_src,
                                                                unsigned char* __restrict__ rgb_out, unsigned char* __restrict__ labels_out, int Hs, int Ws) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= Ws) return;
    const dsrl_augment_params& p = params[n];
    const size_t plane = (size_t)Hs * (size_t)Ws;
    const unsigned char* img = rgb + (size_t)n * plane * 3;
    const int o = y * Ws + x;
    const int bx = p.box[0], by = p.box[1], bw = p.box[2], bh = p.box[3];

    int kx[3], ky[3];
    const int xmin = crop_taps(x, bx, bw, Ws, Ws, kx);
    const int ymin = crop_taps(y, by, bh, Hs, Hs, ky);
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (ky[i] == 0) continue;                                        // a zero tap adds nothing to the integer sum
        int hs[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (kx[j] == 0) continue;
            int v[3];
            rotate_bilinear_rgb(img, p.rot, Ws, Hs, xmin + j, ymin + i, v);
            hs[0] += v[0] * kx[j]; hs[1] += v[1] * kx[j]; hs[2] += v[2] * kx[j];
        }
        acc[0] += clip8(hs[0]) * ky[i]; acc[1] += clip8(hs[1]) * ky[i]; acc[2] += clip8(hs[2]) * ky[i];
    }
    unsigned char* out = rgb_out + (size_t)n * plane * 3 + o * 3;
    out[0] = (unsigned char)clip8(acc[0]); out[1] = (unsigned char)clip8(acc[1]); out[2] = (unsigned char)clip8(acc[2]);

    if (labels) {
        const unsigned char* lab = labels + (size_t)n * plane;
        const int* src = label_src + n * (Ws + Hs);
        const int sx = src[x], sy = src[Ws + y];
        unsigned char lv = 255;
        if (sx >= 0 && sx < Ws && sy >= 0 && sy < Hs) {
            // 16.16 fixed point, wrapping arithmetic (Pillow accumulates the same sums in int)
            const int* a = p.rot_fix;
            const int X = (int)((unsigned)a[2] + (unsigned)sy * (unsigned)a[1] + (unsigned)sx * (unsigned)a[0]) >> 16;
            const int Y = (int)((unsigned)a[5] + (unsigned)sy * (unsigned)a[4] + (unsigned)sx * (unsigned)a[3]) >> 16;
            if (X >= 0 && X < Ws && Y >= 0 && Y < Hs) lv = lab[Y * Ws + X];
        }
        labels_out[(size_t)n * plane + o] = lv;
    }
}

// ---------------------------------------------------------------------------------------------- colour jitter
// One sample's row in registers (block-uniform: scalar loads), with contrast's constant term (1 - c) * mean * 255 folded.
struct JitterRow {
    unsigned ops;                      // the four slots, a byte each in application order; 0xff: nothing to do
    float b, c, s, cm, h[9];
};

__device__ __forceinline__ bool jitter_has_contrast(const dsrl_colour_jitter_params& p) {
    return p.order[0] == DSRL_JITTER_CONTRAST || p.order[1] == DSRL_JITTER_CONTRAST || p.order[2] == DSRL_JITTER_CONTRAST || p.order[3] == DSRL_JITTER_CONTRAST;
}

// `means` is read only for a sample with an enabled contrast
__device__ __forceinline__ JitterRow jitter_row(const dsrl_colour_jitter_params& p, const float* __restrict__ means, int n) {
    JitterRow j;
    j.ops = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) j.ops |= ((unsigned)p.order[k] < 4u ? (unsigned)p.order[k] : 0xffu) << (8 * k);
    j.b = p.brightness; j.c = p.contrast; j.s = p.saturation;
#pragma unroll
    for (int k = 0; k < 9; ++k) j.h[k] = p.hue[k];
    j.cm = (means != nullptr && jitter_has_contrast(p)) ? (1.f - j.c) * (means[n] * 255.f) : 0.f;
    return j;
}

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// The row's operations on one pixel in the 0..255 scale.  PREFIX: only those in front of contrast (what contrast's mean is taken over).
// The slot loop branches on block-uniform values; it stays a loop (one copy of the four operations per tap, not four).
template <bool PREFIX>
__device__ __forceinline__ void jitter_px(float v[3], const JitterRow& j) {
    unsigned ops = j.ops;
#pragma unroll 1
    for (int k = 0; k < 4; ++k, ops >>= 8) {
        const int op = (int)(ops & 0xffu);
        if (op == DSRL_JITTER_BRIGHTNESS) {
            v[0] = clamp255(j.b * v[0]); v[1] = clamp255(j.b * v[1]); v[2] = clamp255(j.b * v[2]);
        } else if (op == DSRL_JITTER_CONTRAST) {
            if (PREFIX) return;
            v[0] = clamp255(j.c * v[0] + j.cm); v[1] = clamp255(j.c * v[1] + j.cm); v[2] = clamp255(j.c * v[2] + j.cm);
        } else if (op == DSRL_JITTER_SATURATION) {
            const float g = (1.f - j.s) * (0.2989f * v[0] + 0.587f * v[1] + 0.114f * v[2]);
            v[0] = clamp255(j.s * v[0] + g); v[1] = clamp255(j.s * v[1] + g); v[2] = clamp255(j.s * v[2] + g);
        } else if (op == DSRL_JITTER_HUE) {
            const float r = v[0], g = v[1], b = v[2];
            v[0] = clamp255(r * j.h[0] + g * j.h[3] + b * j.h[6]);
            v[1] = clamp255(r * j.h[1] + g * j.h[4] + b * j.h[7]);
            v[2] = clamp255(r * j.h[2] + g * j.h[5] + b * j.h[8]);
        }
    }
}

// gray (0..255 scale) of one pixel after the operations in front of contrast
__device__ __forceinline__ double jitter_prefix_gray(float r, float g, float b, const JitterRow& j) {
    float v[3] = {r, g, b};
    jitter_px<true>(v, j);
    return (double)(0.2989f * v[0] + 0.587f * v[1] + 0.114f * v[2]);
}

constexpr int kMeanGroup = 16;          // pixels per 48-byte group: three 16-byte loads
constexpr int kMeanMaxBlocks = 256;     // per sample

// Blocks per sample of the mean reduction: a function of the sample size alone (the workspace query and every launch use it).
static int jitter_mean_blocks(int Hs, int Ws) {
    const long long nb = ceil_div((long long)Hs * Ws, 256 * kMeanGroup);
    return nb < 1 ? 1 : (nb > kMeanMaxBlocks ? kMeanMaxBlocks : (int)nb);
}

// grid (jitter_mean_blocks, N): sum over the sample of gray(x) / 255 after the operations in front of contrast, one double partial per block.
// A sample's bytes start at any address, so its pixels are split into a head of k0 < 16 pixels up to the first 16-byte boundary that is also a
// pixel boundary (3 k0 = -address mod 16), whole 48-byte groups read as three uint4, and a tail of < 16 pixels; block 0 takes head and tail.
__global__ __launch_bounds__(256) void colour_jitter_partial_kernel(const unsigned char* __restrict__ rgb, const dsrl_colour_jitter_params* __restrict__ jitter,
                                                                     double* __restrict__ part, int P) {
    __shared__ double sh[4];
    const int n = blockIdx.y;
    const dsrl_colour_jitter_params& p = jitter[n];
    if (!jitter_has_contrast(p)) return;                                  // block-uniform: nothing reads this sample's mean
    const JitterRow j = jitter_row(p, nullptr, n);
    const unsigned char* img = rgb + (size_t)n * (size_t)P * 3;
    const int k0 = min((int)((((16u - (unsigned)((uintptr_t)img & 15u)) & 15u) * 11u) & 15u), P);
    const int ngroups = (P - k0) / kMeanGroup;
    const uint4* body = (const uint4*)(img + k0 * 3);
    double acc = 0.0;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
        const uint4 a = body[g * 3], b = body[g * 3 + 1], c = body[g * 3 + 2];
        const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int q = 0; q < kMeanGroup; ++q) {
            const int b0 = 3 * q, b1 = 3 * q + 1, b2 = 3 * q + 2;
            acc += jitter_prefix_gray((float)((w[b0 >> 2] >> (8 * (b0 & 3))) & 255u), (float)((w[b1 >> 2] >> (8 * (b1 & 3))) & 255u),
                                      (float)((w[b2 >> 2] >> (8 * (b2 & 3))) & 255u), j);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 2 * kMeanGroup) {
        const int t = threadIdx.x;
        const int px = t < kMeanGroup ? (t < k0 ? t : -1) : k0 + ngroups * kMeanGroup + (t - kMeanGroup);
        if (px >= 0 && px < P) acc += jitter_prefix_gray((float)img[px * 3], (float)img[px * 3 + 1], (float)img[px * 3 + 2], j);
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)n * gridDim.x + blockIdx.x] = (sh[0] + sh[1] + sh[2] + sh[3]) * (1.0 / 255.0);
}

// grid (N), one wave per sample: the sample's partials in a fixed order
__global__ __launch_bounds__(64) void colour_jitter_mean_kernel(const double* __restrict__ part, const dsrl_colour_jitter_params* __restrict__ jitter,
                                                                 float* __restrict__ means, int nb, int P) {
    const int n = blockIdx.x;
    if (!jitter_has_contrast(jitter[n])) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 64) s += part[(size_t)n * nb + i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) means[n] = (float)(s / (double)P);
}

// ---------------------------------------------------------------------------------------------- flip, blur, grayscale + dual-scale resize
__device__ inline void ac_src_aug(int dst, float scale, int n_in, int& i0, int& ip, float& l1) {
    const float r = scale * (float)dst;
    i0 = min((int)r, n_in - 1); ip = (i0 < n_in - 1) ? 1 : 0; l1 = r - (float)i0;
}
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// value (0..255 scale) of the possibly flipped, possibly blurred image at row h, column w of the flipped frame; JITTER: of the colour-jittered image
template <bool JITTER>
__device__ __forceinline__ void aug_tap(const unsigned char* __restrict__ img, int Hs, int Ws, int h, int w, bool flip, bool blur, const float* __restrict__ k,
                                        const JitterRow& jr, float v[3]) {
    if (!blur) {
        const unsigned char* q = img + (h * Ws + (flip ? Ws - 1 - w : w)) * 3;
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
        if constexpr (JITTER) jitter_px<false>(v, jr);
        return;
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int hh = reflect1(h + i - 1, Hs);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            int ww = reflect1(w + j - 1, Ws);
            if (flip) ww = Ws - 1 - ww;
            const unsigned char* q = img + (hh * Ws + ww) * 3;
            const float kk = k[i * 3 + j];
            if constexpr (JITTER) {
                float t[3] = {(float)q[0], (float)q[1], (float)q[2]};
                jitter_px<false>(t, jr);
                s0 += kk * t[0]; s1 += kk * t[1]; s2 += kk * t[2];
            } else {
                s0 += kk * (float)q[0]; s1 += kk * (float)q[1]; s2 += kk * (float)q[2];
            }
        }
    }
    v[0] = s0; v[1] = s1; v[2] = s2;
}

// grid (ceil(Ho * Wo / 256), N)
// The jitter rows and means of a launch: the last kernel argument, empty without jitter, so that prepare_image_aug_kernel<false> has the
// arguments (and the code) of the kernel before there was a jitter.
template <bool JITTER>
struct JitterArgs {
    const dsrl_colour_jitter_params* rows;
    const float* means;
};
template <>
struct JitterArgs<false> {};

template <bool JITTER>
__global__ __launch_bounds__(256) void prepare_image_aug_kernel(const unsigned char* __restrict__ rgb, const dsrl_augment_params* __restrict__ params,
                                                                 float* __restrict__ out, int Hs, int Ws, int Ho, int Wo, int Cout, float sh, float sw,
                                                                 float m0, float m1, float m2, float i0s, float i1s, float i2s, JitterArgs<JITTER> ja) {
    const int e = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (e >= Ho * Wo) return;
    const int ho = e / Wo, wo = e - ho * Wo;
    const dsrl_augment_params& p = params[n];
    const bool flip = p.flags & DSRL_AUG_HFLIP, blur = p.flags & DSRL_AUG_BLUR, gray = p.flags & DSRL_AUG_GRAY;
    const unsigned char* img = rgb + (size_t)n * Hs * Ws * 3;
    int h0, hp, w0, wp; float lh, lw;
    ac_src_aug(ho, sh, Hs, h0, hp, lh); ac_src_aug(wo, sw, Ws, w0, wp, lw);
    JitterRow jr;                                                        // n is block-uniform: the row and its mean are scalar loads
    if constexpr (JITTER) jr = jitter_row(ja.rows[n], ja.means, n);
    float x00[3], x01[3], x10[3], x11[3];
    aug_tap<JITTER>(img, Hs, Ws, h0, w0, flip, blur, p.blur, jr, x00);
    aug_tap<JITTER>(img, Hs, Ws, h0, w0 + wp, flip, blur, p.blur, jr, x01);
    aug_tap<JITTER>(img, Hs, Ws, h0 + hp, w0, flip, blur, p.blur, jr, x10);
    aug_tap<JITTER>(img, Hs, Ws, h0 + hp, w0 + wp, flip, blur, p.blur, jr, x11);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (1.f - lh) * ((1.f - lw) * x00[c] + lw * x01[c]) + lh * ((1.f - lw) * x10[c] + lw * x11[c]);
    if (gray) v[0] = v[1] = v[2] = 0.2989f * v[0] + 0.587f * v[1] + 0.114f * v[2];      // torchvision rgb_to_grayscale, 3 output channels
    float* o = out + ((size_t)n * Ho * Wo + e) * Cout;
    o[0] = (v[0] * (1.f / 255.f) - m0) * i0s; o[1] = (v[1] * (1.f / 255.f) - m1) * i1s; o[2] = (v[2] * (1.f / 255.f) - m2) * i2s;
    if (Cout == 4) o[3] = 0.f;
}

__global__ __launch_bounds__(256) void prepare_target_aug_kernel(const unsigned char* __restrict__ labels, const unsigned char* __restrict__ lut,
                                                                  const dsrl_augment_params* __restrict__ params, unsigned char* __restrict__ target,
                                                                  int Hs, int Ws, int Ho, int Wo) {
    const int e = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (e >= Ho * Wo) return;
    const int ho = e / Wo, wo = e - ho * Wo;
    const float sh = (float)Hs / (float)Ho, sw = (float)Ws / (float)Wo;             // torch 'nearest': src = floor(dst * in/out)
    const int hs = min((int)floorf((float)ho * sh), Hs - 1);
    int ws = min((int)floorf((float)wo * sw), Ws - 1);
    if (params[n].flags & DSRL_AUG_HFLIP) ws = Ws - 1 - ws;
    target[(size_t)n * Ho * Wo + e] = lut[labels[(size_t)n * Hs * Ws + hs * Ws + ws]];
}

}  // namespace dsrl
using namespace dsrl;

static bool fits_i32(long long v) { return v > 0 && v < (1ll << 31); }

extern "C" int dsrl_augment_geometry(const uint8_t* rgb, const uint8_t* labels, const dsrl_augment_params* params, const int32_t* label_src,
                                     uint8_t* rgb_out, uint8_t* labels_out, int N, int Hs, int Ws, dsrl_stream_t stream) {
    DSRL_REQUIRE(rgb && params && rgb_out && N > 0 && N <= 65535 && Hs > 0 && Hs <= 65535 && Ws > 0, DSRL_E_BADARG, "augment_geometry: bad arguments");
    DSRL_REQUIRE((labels == nullptr) == (labels_out == nullptr) && (labels == nullptr) == (label_src == nullptr), DSRL_E_BADARG,
                 "augment_geometry: labels, label_src and labels_out go together");
    DSRL_REQUIRE(((uintptr_t)params % 8) == 0 && ((uintptr_t)label_src % 4) == 0, DSRL_E_BADARG, "augment_geometry: misaligned parameter tables");
    DSRL_REQUIRE(fits_i32(3ll * Hs * Ws) && fits_i32((long long)N * (Hs + Ws)), DSRL_E_UNSUPPORTED, "augment_geometry: a %dx%d sample exceeds 32-bit indexing", Hs, Ws);
    DSRL_REQUIRE(rgb_out != rgb && (labels_out == nullptr || labels_out != labels), DSRL_E_BADARG, "augment_geometry: in-place is not supported");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(augment_geometry_kernel, dim3((unsigned)ceil_div(Ws, 256), (unsigned)Hs, (unsigned)N), dim3(256), 0, st,
                       rgb, labels, params, (const int*)label_src, rgb_out, labels_out, Hs, Ws);
    return launch_status("augment_geometry_kernel");
}

// dsrl_prepare_batch_augmented (jitter == nullptr) and dsrl_prepare_batch_jittered: one argument check, one launch sequence
static int prepare_batch_aug(const char* who, const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut, const float* mean, const float* std_, float* img_in,
                             float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W, const dsrl_augment_params* params,
                             const dsrl_colour_jitter_params* jitter, const float* means, dsrl_stream_t stream) {
    DSRL_REQUIRE(rgb && mean && std_ && params && N > 0 && N <= 65535 && Hs >= 2 && Ws >= 2 && H > 0 && W > 0, DSRL_E_BADARG,
                 "%s: bad arguments (the 3x3 blur needs a sample of at least 2x2)", who);
    DSRL_REQUIRE((labels == nullptr) == (target == nullptr) && (labels == nullptr || lut != nullptr), DSRL_E_BADARG, "%s: labels, lut and target go together", who);
    DSRL_REQUIRE(((uintptr_t)params % 8) == 0, DSRL_E_BADARG, "%s: the parameter table must be 8-byte aligned", who);
    DSRL_REQUIRE(fits_i32(3ll * Hs * Ws) && fits_i32(16ll * H * W), DSRL_E_UNSUPPORTED, "%s: sizes exceed 32-bit indexing", who);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    auto sc = [](int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; };
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2], i0 = 1.f / std_[0], i1 = 1.f / std_[1], i2 = 1.f / std_[2];
    auto image = [&](float* out, int Ho, int Wo, int Cout) {
        const dim3 grid((unsigned)ceil_div((long long)Ho * Wo, 256), (unsigned)N);
        if (jitter)
            hipLaunchKernelGGL(prepare_image_aug_kernel<true>, grid, dim3(256), 0, st, rgb, params, out, Hs, Ws, Ho, Wo, Cout, sc(Hs, Ho), sc(Ws, Wo),
                               m0, m1, m2, i0, i1, i2, JitterArgs<true>{jitter, means});
        else
            hipLaunchKernelGGL(prepare_image_aug_kernel<false>, grid, dim3(256), 0, st, rgb, params, out, Hs, Ws, Ho, Wo, Cout, sc(Hs, Ho), sc(Ws, Wo),
                               m0, m1, m2, i0, i1, i2, JitterArgs<false>{});
        return launch_status("prepare_image_aug_kernel");
    };
    if (img_in)
        if (int e = image(img_in, H, W, 4)) return e;
    if (img_org)
        if (int e = image(img_org, 2 * H, 2 * W, 3)) return e;
    if (target) {
        hipLaunchKernelGGL(prepare_target_aug_kernel, dim3((unsigned)ceil_div(4ll * H * W, 256), (unsigned)N), dim3(256), 0, st,
                           labels, lut, params, target, Hs, Ws, 2 * H, 2 * W);
        return launch_status("prepare_target_aug_kernel");
    }
    return DSRL_OK;
}

extern "C" int dsrl_prepare_batch_augmented(const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut, const float* mean, const float* std_,
                                            float* img_in, float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W,
                                            const dsrl_augment_params* params, dsrl_stream_t stream) {
    return prepare_batch_aug("prepare_batch_augmented", rgb, labels, lut, mean, std_, img_in, img_org, target, N, Hs, Ws, H, W, params, nullptr, nullptr, stream);
}

extern "C" int dsrl_prepare_batch_jittered(const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut, const float* mean, const float* std_,
                                           float* img_in, float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W,
                                           const dsrl_augment_params* params, const dsrl_colour_jitter_params* jitter, const float* means, dsrl_stream_t stream) {
    DSRL_REQUIRE(jitter != nullptr && ((uintptr_t)jitter % 4) == 0, DSRL_E_BADARG, "prepare_batch_jittered: the jitter table is null or not 4-byte aligned");
    DSRL_REQUIRE(means != nullptr && ((uintptr_t)means % 4) == 0, DSRL_E_BADARG, "prepare_batch_jittered: a jitter table needs the per-sample means (4-byte aligned)");
    return prepare_batch_aug("prepare_batch_jittered", rgb, labels, lut, mean, std_, img_in, img_org, target, N, Hs, Ws, H, W, params, jitter, means, stream);
}

extern "C" size_t dsrl_colour_jitter_workspace_bytes(int N, int Hs, int Ws) {
    if (N <= 0 || Hs <= 0 || Ws <= 0) return 0;
    return (size_t)N * (size_t)jitter_mean_blocks(Hs, Ws) * sizeof(double);
}

extern "C" int dsrl_colour_jitter_means(const uint8_t* rgb, const dsrl_colour_jitter_params* jitter, float* means, void* ws, size_t ws_bytes, int N, int Hs,
                                        int Ws, dsrl_stream_t stream) {
    DSRL_REQUIRE(rgb && jitter && means && ws && N > 0 && N <= 65535 && Hs > 0 && Ws > 0, DSRL_E_BADARG, "colour_jitter_means: bad arguments");
    DSRL_REQUIRE(((uintptr_t)jitter % 4) == 0 && ((uintptr_t)means % 4) == 0 && ((uintptr_t)ws % 8) == 0, DSRL_E_BADARG,
                 "colour_jitter_means: misaligned jitter table, means or workspace");
    DSRL_REQUIRE(fits_i32(3ll * Hs * Ws), DSRL_E_UNSUPPORTED, "colour_jitter_means: a %dx%d sample exceeds 32-bit indexing", Hs, Ws);
    DSRL_REQUIRE(ws_bytes >= dsrl_colour_jitter_workspace_bytes(N, Hs, Ws), DSRL_E_WORKSPACE, "colour_jitter_means: workspace of %zu bytes, %zu needed", ws_bytes,
                 dsrl_colour_jitter_workspace_bytes(N, Hs, Ws));
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int nb = jitter_mean_blocks(Hs, Ws), P = Hs * Ws;
    hipLaunchKernelGGL(colour_jitter_partial_kernel, dim3((unsigned)nb, (unsigned)N), dim3(256), 0, st, rgb, jitter, (double*)ws, P);
    if (int e = launch_status("colour_jitter_partial_kernel")) return e;
    hipLaunchKernelGGL(colour_jitter_mean_kernel, dim3((unsigned)N), dim3(64), 0, st, (const double*)ws, jitter, means, nb, P);
    return launch_status("colour_jitter_mean_kernel");
}
