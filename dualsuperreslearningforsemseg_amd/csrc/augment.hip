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
// Index arithmetic is 32-bit within a sample (one sample: < 2^31 bytes); the sample offset is the only 64-bit product.
#include "common.h"

namespace dsrl {

static_assert(sizeof(dsrl_augment_params) == 128, "dsrl_augment_params is a 128-byte table row");

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

// ---------------------------------------------------------------------------------------------- flip, blur, grayscale + dual-scale resize
__device__ inline void ac_src_aug(int dst, float scale, int n_in, int& i0, int& ip, float& l1) {
    const float r = scale * (float)dst;
    i0 = min((int)r, n_in - 1); ip = (i0 < n_in - 1) ? 1 : 0; l1 = r - (float)i0;
}
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// value (0..255 scale) of the possibly flipped, possibly blurred image at row h, column w of the flipped frame
__device__ __forceinline__ void aug_tap(const unsigned char* __restrict__ img, int Hs, int Ws, int h, int w, bool flip, bool blur, const float* __restrict__ k, float v[3]) {
    if (!blur) {
        const unsigned char* q = img + (h * Ws + (flip ? Ws - 1 - w : w)) * 3;
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
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
            s0 += kk * (float)q[0]; s1 += kk * (float)q[1]; s2 += kk * (float)q[2];
        }
    }
    v[0] = s0; v[1] = s1; v[2] = s2;
}

// grid (ceil(Ho * Wo / 256), N)
__global__ __launch_bounds__(256) void prepare_image_aug_kernel(const unsigned char* __restrict__ rgb, const dsrl_augment_params* __restrict__ params,
                                                                 float* __restrict__ out, int Hs, int Ws, int Ho, int Wo, int Cout, float sh, float sw,
                                                                 float m0, float m1, float m2, float i0s, float i1s, float i2s) {
    const int e = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (e >= Ho * Wo) return;
    const int ho = e / Wo, wo = e - ho * Wo;
    const dsrl_augment_params& p = params[n];
    const bool flip = p.flags & DSRL_AUG_HFLIP, blur = p.flags & DSRL_AUG_BLUR, gray = p.flags & DSRL_AUG_GRAY;
    const unsigned char* img = rgb + (size_t)n * Hs * Ws * 3;
    int h0, hp, w0, wp; float lh, lw;
    ac_src_aug(ho, sh, Hs, h0, hp, lh); ac_src_aug(wo, sw, Ws, w0, wp, lw);
    float x00[3], x01[3], x10[3], x11[3];
    aug_tap(img, Hs, Ws, h0, w0, flip, blur, p.blur, x00);
    aug_tap(img, Hs, Ws, h0, w0 + wp, flip, blur, p.blur, x01);
    aug_tap(img, Hs, Ws, h0 + hp, w0, flip, blur, p.blur, x10);
    aug_tap(img, Hs, Ws, h0 + hp, w0 + wp, flip, blur, p.blur, x11);
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

extern "C" int dsrl_prepare_batch_augmented(const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut, const float* mean, const float* std_,
                                            float* img_in, float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W,
                                            const dsrl_augment_params* params, dsrl_stream_t stream) {
    DSRL_REQUIRE(rgb && mean && std_ && params && N > 0 && N <= 65535 && Hs >= 2 && Ws >= 2 && H > 0 && W > 0, DSRL_E_BADARG,
                 "prepare_batch_augmented: bad arguments (the 3x3 blur needs a sample of at least 2x2)");
    DSRL_REQUIRE((labels == nullptr) == (target == nullptr) && (labels == nullptr || lut != nullptr), DSRL_E_BADARG,
                 "prepare_batch_augmented: labels, lut and target go together");
    DSRL_REQUIRE(((uintptr_t)params % 8) == 0, DSRL_E_BADARG, "prepare_batch_augmented: the parameter table must be 8-byte aligned");
    DSRL_REQUIRE(fits_i32(3ll * Hs * Ws) && fits_i32(16ll * H * W), DSRL_E_UNSUPPORTED, "prepare_batch_augmented: sizes exceed 32-bit indexing");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    auto sc = [](int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; };
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2], i0 = 1.f / std_[0], i1 = 1.f / std_[1], i2 = 1.f / std_[2];
    if (img_in) {
        hipLaunchKernelGGL(prepare_image_aug_kernel, dim3((unsigned)ceil_div((long long)H * W, 256), (unsigned)N), dim3(256), 0, st,
                           rgb, params, img_in, Hs, Ws, H, W, 4, sc(Hs, H), sc(Ws, W), m0, m1, m2, i0, i1, i2);
        if (int e = launch_status("prepare_image_aug_kernel")) return e;
    }
    if (img_org) {
        hipLaunchKernelGGL(prepare_image_aug_kernel, dim3((unsigned)ceil_div(4ll * H * W, 256), (unsigned)N), dim3(256), 0, st,
                           rgb, params, img_org, Hs, Ws, 2 * H, 2 * W, 3, sc(Hs, 2 * H), sc(Ws, 2 * W), m0, m1, m2, i0, i1, i2);
        if (int e = launch_status("prepare_image_aug_kernel")) return e;
    }
    if (target) {
        hipLaunchKernelGGL(prepare_target_aug_kernel, dim3((unsigned)ceil_div(4ll * H * W, 256), (unsigned)N), dim3(256), 0, st,
                           labels, lut, params, target, Hs, Ws, 2 * H, 2 * W);
        return launch_status("prepare_target_aug_kernel");
    }
    return DSRL_OK;
}
