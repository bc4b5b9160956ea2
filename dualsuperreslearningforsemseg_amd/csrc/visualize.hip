// The panel the test command saves per image (utils.make_input_output_visualization), built on the device: input | class colours | overlay.
//
// A streaming kernel over uint8: per pixel 3 bytes of the shown image and one class byte come in, 9 bytes go out (the output row of image row
// (n, h) is [3W input bytes][3W colour bytes][3W overlay bytes]).  When W is a multiple of 4 (16) and the pointers are 4 (16) byte aligned, every
// image row, class row and each of the three segments of an output row starts on such a boundary, and a thread owns 4 (16) consecutive pixels of one
// row: 3 + 1 (+ 1 mask) loads and 9 stores of one (four) 32-bit words each.  Anything else takes one thread per pixel with byte accesses.
// The palette sits in LDS as one 32-bit word per label (r | g << 8 | b << 16): one ds_read per pixel.
// The overlay is uint8(min((1 - b) * in + b * colour, 255)) in double with the two products and the sum rounded separately (the library is built with
// -ffp-contract=off), which is how numpy evaluates the host function's expression; the conversion truncates, as astype(uint8) does.
#include "common.h"
#include <limits.h>

namespace dsrl {

namespace {

__device__ __forceinline__ unsigned blend_byte(unsigned in, unsigned col, double omb, double b) {
    const double p = omb * (double)in;
    const double q = b * (double)col;
    const double v = p + q;
    return (unsigned)(v < 255.0 ? v : 255.0);
}

__device__ __forceinline__ void load_palette(unsigned* pal, const unsigned char* __restrict__ palette) {
    for (int t = threadIdx.x; t < 256; t += blockDim.x)
        pal[t] = (unsigned)palette[3 * t] | ((unsigned)palette[3 * t + 1] << 8) | ((unsigned)palette[3 * t + 2] << 16);
    __syncthreads();
}

// V consecutive 32-bit words as one access (V = 4: a 16-byte aligned dwordx4)
template <int V>
__device__ __forceinline__ void load_words(const unsigned* __restrict__ p, unsigned* d) {
    if constexpr (V == 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
        d[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_words(unsigned* __restrict__ p, const unsigned* s) {
    if constexpr (V == 4) *reinterpret_cast<uint4*>(p) = make_uint4(s[0], s[1], s[2], s[3]);
    else *p = s[0];
}

// V 32-bit words of class bytes per thread: 4 V pixels, 3 V words of image bytes in, 3 x 3 V words out
template <int V>
__global__ __launch_bounds__(256) void class_map_visualize_vec_kernel(const unsigned* __restrict__ rgb, const unsigned* __restrict__ classes,
                                                                       const unsigned* __restrict__ mask, const unsigned char* __restrict__ palette,
                                                                       unsigned* __restrict__ out, unsigned W, unsigned ngroups, unsigned ignore_index,
                                                                       double omb, double b) {
    __shared__ unsigned pal[256];
    load_palette(pal, palette);
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= ngroups) return;
    const unsigned p = g * (4u * V);                // first pixel of the group; W % (4 V) == 0: the group lies inside one row
    const unsigned row = p / W, x = p - row * W;
    unsigned cw[V], mw[V], rw[3 * V], cow[3 * V], ovw[3 * V];
    load_words<V>(classes + g * V, cw);
#pragma unroll
    for (int i = 0; i < V; ++i) mw[i] = 0u;
    if (mask != nullptr) load_words<V>(mask + g * V, mw);
#pragma unroll
    for (int i = 0; i < 3; ++i) load_words<V>(rgb + g * (3u * V) + i * V, rw + i * V);
#pragma unroll
    for (int i = 0; i < 3 * V; ++i) cow[i] = ovw[i] = 0u;
#pragma unroll
    for (int i = 0; i < 4 * V; ++i) {
        unsigned cls = (cw[i >> 2] >> (8 * (i & 3))) & 0xffu;
        if (mask != nullptr && ((mw[i >> 2] >> (8 * (i & 3))) & 0xffu) == ignore_index) cls = ignore_index;
        const unsigned colour = pal[cls];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int j = 3 * i + c;
            const unsigned in = (rw[j >> 2] >> (8 * (j & 3))) & 0xffu;
            const unsigned col = (colour >> (8 * c)) & 0xffu;
            cow[j >> 2] |= col << (8 * (j & 3));
            ovw[j >> 2] |= blend_byte(in, col, omb, b) << (8 * (j & 3));
        }
    }
    // 32-bit words: the output row starts at word row * 9 W / 4, its segments 3 W / 4 words apart
    const unsigned w34 = (3u * W) >> 2;
    unsigned* o = out + row * (3u * w34) + ((3u * x) >> 2);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        store_words<V>(o + i * V, rw + i * V);
        store_words<V>(o + w34 + i * V, cow + i * V);
        store_words<V>(o + 2u * w34 + i * V, ovw + i * V);
    }
}

__global__ __launch_bounds__(256) void class_map_visualize_byte_kernel(const unsigned char* __restrict__ rgb, const unsigned char* __restrict__ classes,
                                                                        const unsigned char* __restrict__ mask, const unsigned char* __restrict__ palette,
                                                                        unsigned char* __restrict__ out, unsigned W, unsigned npix, unsigned ignore_index,
                                                                        double omb, double b) {
    __shared__ unsigned pal[256];
    load_palette(pal, palette);
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    const unsigned row = p / W, x = p - row * W;
    unsigned cls = classes[p];
    if (mask != nullptr && mask[p] == ignore_index) cls = ignore_index;
    const unsigned colour = pal[cls];
    unsigned char* o = out + row * (9u * W) + 3u * x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned in = rgb[3u * p + c], col = (colour >> (8 * c)) & 0xffu;
        o[c] = (unsigned char)in;
        o[3u * W + c] = (unsigned char)col;
        o[6u * W + c] = (unsigned char)blend_byte(in, col, omb, b);
    }
}

}  // namespace

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_class_map_visualize(const uint8_t* rgb, const uint8_t* classes, const uint8_t* mask, const uint8_t* palette, uint8_t* out, int N, int H, int W,
                                        int ignore_index, double blend_factor, dsrl_stream_t stream) {
    DSRL_REQUIRE(rgb && classes && palette && out && N > 0 && H > 0 && W > 0, DSRL_E_BADARG, "class_map_visualize: null pointer or empty shape");
    DSRL_REQUIRE(blend_factor > 0.0 && blend_factor < 1.0 && ignore_index >= 0 && ignore_index <= 255, DSRL_E_BADARG,
                 "class_map_visualize: blend_factor must lie in (0, 1) and ignore_index in [0, 255]");
    const long long P = (long long)N * H * W;
    DSRL_REQUIRE(9 * P <= (long long)INT_MAX, DSRL_E_UNSUPPORTED, "class_map_visualize: the panel is indexed in 32 bits (N*H*W*9 < 2^31, got %lld pixels)", P);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const double omb = 1.0 - blend_factor;
    const uintptr_t bits = (uintptr_t)rgb | (uintptr_t)classes | (uintptr_t)mask | (uintptr_t)out;
    const unsigned uW = (unsigned)W, ign = (unsigned)ignore_index;
    if (W % 16 == 0 && bits % 16 == 0) {
        const unsigned ng = (unsigned)(P / 16);
        hipLaunchKernelGGL((class_map_visualize_vec_kernel<4>), dim3((unsigned)ceil_div(ng, 256)), dim3(256), 0, st, (const unsigned*)rgb, (const unsigned*)classes,
                           (const unsigned*)mask, palette, (unsigned*)out, uW, ng, ign, omb, blend_factor);
    } else if (W % 4 == 0 && bits % 4 == 0) {
        const unsigned ng = (unsigned)(P / 4);
        hipLaunchKernelGGL((class_map_visualize_vec_kernel<1>), dim3((unsigned)ceil_div(ng, 256)), dim3(256), 0, st, (const unsigned*)rgb, (const unsigned*)classes,
                           (const unsigned*)mask, palette, (unsigned*)out, uW, ng, ign, omb, blend_factor);
    } else {
        hipLaunchKernelGGL(class_map_visualize_byte_kernel, dim3((unsigned)ceil_div(P, 256)), dim3(256), 0, st, rgb, classes, mask, palette, out, uW, (unsigned)P, ign,
                           omb, blend_factor);
    }
    return launch_status("class_map_visualize_kernel");
}
