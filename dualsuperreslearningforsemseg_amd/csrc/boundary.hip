// Boundary IoU: per class the pixels of the target's and of the prediction's boundary band and of their intersection, from two
// uint8 class maps.  A pixel is in the band of a map iff the (2d+1) x (2d+1) window centred on it leaves the image or holds a byte other than its own.
//     dsrl_boundary_counts_workspace_bytes   2 bytes per pixel: the row pass' result for both maps
//     dsrl_boundary_counts                   two launches: boundary_rows_kernel, boundary_cols_kernel
// The window test is separable and costs O(1) per pixel and pass, whatever d: a window is uniform iff the run of equal bytes that ends at its last
// element is at least 2d+1 long.
//   rows: a wave walks a piece of one image row left to right, 64 positions per step.  A lane normalises its pixel of both maps (void 255, bad 254),
//         compares it with its left neighbour's (a shuffle; lane 0 takes the previous step's lane 63) and finds the start of its run from the ballot
//         of those comparisons: the highest set bit at or below the lane, else the start carried from the steps before.  The lane at position i then
//         decides pixel i - d: its row window [i - 2d, i] is uniform iff i - start >= 2d, and it writes the label if so, the sentinel 253 if not
//         (also for the last d pixels of a row, whose window leaves the image; the first d fail the test by themselves: column 0 starts a run).
//         Both maps' bytes of a pixel go out as one 16-bit store.  Nothing goes through LDS and the walk's only carried state is wave-uniform;
//         a step's bytes are loaded one step ahead.
//   cols: a thread owns one column of a strip and walks down, keeping per map the length of the run of equal non-sentinel row results that ends
//         at row y + d: pixel (y, x) is interior iff that run is >= 2d+1 (rows at or below H count as sentinels, rows above 0 are simply missing from
//         the run).  It re-reads the pixel's two bytes, normalises them, writes the band byte and counts.  A wave's first d output rows need 2d rows
//         of warm-up reads: kBdRows output rows per wave keep that at (64 + 2d) / 64 reads of the 2-byte result per pixel, which the L2 serves.
//         The walk is a chain of dependent steps, so the loads of kBdBatch rows are issued together before the first is used.
//         Counters: a thread's consecutive pixels mostly repeat their (class, band) key, so a run of equal keys leaves as ONE LDS atomic (the CmRun
//         idea of the confusion matrix); the block's 3C 32-bit bins go out as 64-bit global atomics: exact, order independent, identical run to run.
//         A block counts at most 256 x 64 pixels: no bin can wrap.
// Integer arithmetic only, 32-bit indices (the host refuses N*H*W >= 2^31 - 2^16), one 32-bit division per block and none per element.  Loads and stores
// are per byte (16-bit for the row result): either map may start at any byte and W may be anything.
#include "common.h"

namespace dsrl {

constexpr int kBdMaxC = 253;            // labels 0..252; 253, 254 and 255 are taken:
constexpr unsigned kBdSent = 253u;      //   a row window that is not uniform, or leaves the image
constexpr unsigned kBdBad = 254u;       //   a predicted class >= C on a counted pixel
constexpr unsigned kBdVoid = 255u;      //   a pixel that is not counted
constexpr int kBdMaxD = 128;
constexpr int kBdSegW = 1024;           // output pixels of one wave of the row pass
constexpr int kBdRows = 64;             // output rows of one wave of the column pass
constexpr int kBdBatch = 8;             // rows of the column pass whose loads are in flight together
constexpr long long kBdMaxPixels = (1ll << 31) - (1ll << 16);       // a pixel index plus a kernel's stride (a step of 64, a piece of 1024, d) stays an int

// step 1 of the definition: g' from the target byte, p' from the prediction's under it
__device__ __forceinline__ void bd_normalise(unsigned t, unsigned p, int C, int ignore_index, unsigned& g, unsigned& q) {
    const bool live = (int)t < C && (int)t != ignore_index;
    g = live ? t : kBdVoid;
    q = !live ? kBdVoid : ((int)p < C ? p : kBdBad);
}

__global__ __launch_bounds__(256) void boundary_rows_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ target, int rows, int W,
                                                             int C, int ignore_index, int d, int nseg, unsigned short* __restrict__ res) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rg = (int)(blockIdx.x / (unsigned)nseg), seg = (int)blockIdx.x - rg * nseg;
    const int row = rg * 4 + w;
    if (row >= rows) return;                                    // wave-uniform; the kernel has no barrier
    const int s = seg * kBdSegW, e = min(W, s + kBdSegW);       // this wave's output pixels [s, e) of the row
    const int i0 = max(0, s - d), i1 = min(W - 1, e - 1 + d);   // the positions it walks: a run that reaches back to s - d is long enough for every output
    const int off = row * W;
    const unsigned char* tp = target + off;
    const unsigned char* pp = pred + off;
    unsigned short* out = res + off;
    const unsigned long long le = (2ull << lane) - 1ull;        // lanes at or below mine
    int sg = i0, sp = i0;                                       // start of the run the previous step ended in
    unsigned cg = 256u, cp = 256u;                              // its byte: no byte at first, so that position i0 starts a run
    unsigned nt = tp[min(i0 + lane, i1)], np_ = pp[min(i0 + lane, i1)];      // the step's bytes are loaded one step ahead (positions past i1 clamped)
    for (int base = i0; base <= i1; base += 64) {
        const int i = base + lane;
        const bool act = i <= i1;
        const unsigned ct = nt, cp_ = np_;
        if (base + 64 <= i1) { nt = tp[min(i + 64, i1)]; np_ = pp[min(i + 64, i1)]; }
        unsigned g = 256u, q = 256u;
        if (act) bd_normalise(ct, cp_, C, ignore_index, g, q);
        unsigned lg = (unsigned)__shfl_up((int)g, 1, 64), lq = (unsigned)__shfl_up((int)q, 1, 64);
        if (lane == 0) { lg = cg; lq = cp; }
        const unsigned long long bg = __ballot(g != lg), bq = __ballot(q != lq);
        const unsigned long long mg = bg & le, mq = bq & le;
        const int rs_g = mg ? base + 63 - __clzll((long long)mg) : sg;
        const int rs_q = mq ? base + 63 - __clzll((long long)mq) : sp;
        const int x = i - d;
        if (act && x >= s) {
            const unsigned rg_ = i - rs_g >= 2 * d ? g : kBdSent, rq_ = i - rs_q >= 2 * d ? q : kBdSent;
            out[x] = (unsigned short)(rg_ | (rq_ << 8));
        }
        if (bg) sg = base + 63 - __clzll((long long)bg);        // (lanes past i1 flag too: only in the last step, after which nothing reads it)
        if (bq) sp = base + 63 - __clzll((long long)bq);
        cg = (unsigned)__shfl((int)g, 63, 64);
        cp = (unsigned)__shfl((int)q, 63, 64);
    }
    for (int x = max(s, W - d) + lane; x < e; x += 64) out[x] = (unsigned short)(kBdSent | (kBdSent << 8));
}

// a run of equal keys leaves as one LDS atomic; key < 0: not counted
struct BdRun {
    int key = -1;
    unsigned n = 0u;
    __device__ __forceinline__ void flush(unsigned* h) { if (n) atomicAdd(&h[key], n); n = 0u; }
    __device__ __forceinline__ void add(unsigned* h, int k) {
        if (k != key) { flush(h); key = k; }
        n += k >= 0 ? 1u : 0u;
    }
};
__device__ __forceinline__ void bd_run(unsigned r, unsigned& prev, int& run) {
    run = r == kBdSent ? 0 : (r == prev ? run + 1 : 1);
    prev = r;
}

__global__ __launch_bounds__(256) void boundary_cols_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ target, int H, int W, int C,
                                                             int ignore_index, int d, int nbx, int nby, const unsigned short* __restrict__ res,
                                                             unsigned long long* __restrict__ counts, unsigned char* __restrict__ band, int* __restrict__ nan_flag) {
    __shared__ unsigned hist[3 * kBdMaxC];                      // I | G | P
    for (int t = threadIdx.x; t < 3 * C; t += 256) hist[t] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int per = nbx * nby;
    const int n = (int)(blockIdx.x / (unsigned)per), rem = (int)blockIdx.x - n * per;
    const int by = rem / nbx, bx = rem - by * nbx;
    const int x = bx * 64 + lane;
    const int y0 = (by * 4 + w) * kBdRows, y1 = min(H, y0 + kBdRows);
    bool bad = false;
    if (x < W && y0 < H) {
        const int need = 2 * d + 1;
        const int img = n * H;                                  // the image's first row
        const int w0 = max(0, y0 - d), w1 = min(H, y0 + d);     // warm-up: the rows above y0 + d
        int rung = 0, runq = 0;
        unsigned pg = kBdSent, pq = kBdSent;
        // Rows go by in batches of kBdBatch: every load of a batch is issued (rows past the end clamped to the last one, so that no load is
        // conditional) before the first is used - the walk is a chain of dependent steps, and one load latency per row was most of its time.
        for (int yy = w0; yy < w1; yy += kBdBatch) {
            unsigned r[kBdBatch];
#pragma unroll
            for (int u = 0; u < kBdBatch; ++u) r[u] = res[(img + min(yy + u, w1 - 1)) * W + x];
#pragma unroll
            for (int u = 0; u < kBdBatch; ++u)
                if (yy + u < w1) {
                    bd_run(r[u] & 0xffu, pg, rung);
                    bd_run(r[u] >> 8, pq, runq);
                }
        }
        BdRun ri, rgn, rpn;
        for (int y = y0; y < y1; y += kBdBatch) {
            unsigned r[kBdBatch], t[kBdBatch], p[kBdBatch];
#pragma unroll
            for (int u = 0; u < kBdBatch; ++u) {
                const int ip = (img + min(y + u, y1 - 1)) * W + x;
                r[u] = res[(img + min(y + u + d, H - 1)) * W + x];
                t[u] = target[ip];
                p[u] = pred[ip];
            }
#pragma unroll
            for (int u = 0; u < kBdBatch; ++u)
                if (y + u < y1) {
                    const unsigned rr = y + u + d < H ? r[u] : (kBdSent | (kBdSent << 8));      // rows below the image: sentinels
                    bd_run(rr & 0xffu, pg, rung);
                    bd_run(rr >> 8, pq, runq);
                    unsigned g, q;
                    bd_normalise(t[u], p[u], C, ignore_index, g, q);
                    const bool live = g != kBdVoid, gb = rung < need, qb = runq < need;
                    bad |= q == kBdBad;
                    const int kg = live && gb ? (int)g : -1;
                    const int kq = live && qb && q < kBdBad ? (int)q : -1;
                    ri.add(hist, kg >= 0 && kg == kq ? kg : -1);
                    rgn.add(hist + C, kg);
                    rpn.add(hist + 2 * C, kq);
                    if (band != nullptr) band[(img + y + u) * W + x] = live ? (unsigned char)((gb ? 1 : 0) | (qb ? 2 : 0)) : (unsigned char)0;
                }
        }
        ri.flush(hist);
        rgn.flush(hist + C);
        rpn.flush(hist + 2 * C);
    }
    if (nan_flag != nullptr && __any(bad) && lane == 0) atomicOr(nan_flag, 2);
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * C; t += 256) {
        const unsigned v = hist[t];
        if (v) atomicAdd(&counts[t], (unsigned long long)v);
    }
}

static inline bool bd_shape_ok(int N, int H, int W, int d) {
    return N >= 1 && H >= 1 && W >= 1 && d >= 1 && d <= kBdMaxD && (int64_t)N * H * W < kBdMaxPixels;
}

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_boundary_counts_max_classes(void) { return kBdMaxC; }
extern "C" int dsrl_boundary_counts_max_distance(void) { return kBdMaxD; }
extern "C" size_t dsrl_boundary_counts_workspace_bytes(int N, int H, int W, int d) {
    if (!bd_shape_ok(N, H, W, d)) return 0;
    return (size_t)N * (size_t)H * (size_t)W * sizeof(unsigned short);
}

extern "C" int dsrl_boundary_counts(const uint8_t* pred, const uint8_t* target, int N, int H, int W, int C, int ignore_index, int d, unsigned long long* counts,
                                    uint8_t* band, int* nan_flag, void* ws, size_t ws_bytes, dsrl_stream_t stream) {
    DSRL_REQUIRE(pred && target && counts, DSRL_E_BADARG, "boundary_counts: null pointer");
    DSRL_REQUIRE(N >= 1 && H >= 1 && W >= 1, DSRL_E_BADARG, "boundary_counts: N=%d H=%d W=%d", N, H, W);
    DSRL_REQUIRE(C >= 1 && d >= 1, DSRL_E_BADARG, "boundary_counts: C=%d d=%d (both >= 1)", C, d);
    DSRL_REQUIRE(C <= kBdMaxC, DSRL_E_UNSUPPORTED, "boundary_counts: %d classes, the labels above %d are the kernels' own", C, kBdMaxC - 1);
    DSRL_REQUIRE(d <= kBdMaxD, DSRL_E_UNSUPPORTED, "boundary_counts: distance %d above the maximum %d", d, kBdMaxD);
    DSRL_REQUIRE((int64_t)N * H * W < kBdMaxPixels, DSRL_E_UNSUPPORTED, "boundary_counts: N=%d H=%d W=%d does not fit 32-bit pixel indices", N, H, W);
    DSRL_REQUIRE(((uintptr_t)counts % 8) == 0 && ((uintptr_t)nan_flag % 4) == 0, DSRL_E_BADARG, "boundary_counts: misaligned counts or nan_flag");
    const size_t need = dsrl_boundary_counts_workspace_bytes(N, H, W, d);
    DSRL_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws % 2) == 0, DSRL_E_WORKSPACE, "boundary_counts: workspace of %zu bytes (2-byte aligned) needed, got %zu", need,
                 ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    const int rows = N * H;
    const int nseg = (int)ceil_div(W, kBdSegW);
    const int64_t row_blocks = ceil_div(rows, 4) * nseg;
    const int nbx = (int)ceil_div(W, 64), nby = (int)ceil_div(H, 4 * kBdRows);
    const int64_t col_blocks = (int64_t)N * nbx * nby;
    DSRL_REQUIRE(row_blocks < (1ll << 31) && col_blocks < (1ll << 31), DSRL_E_UNSUPPORTED, "boundary_counts: N=%d H=%d W=%d needs too many blocks", N, H, W);
    unsigned short* res = (unsigned short*)ws;
    hipLaunchKernelGGL(boundary_rows_kernel, dim3((unsigned)row_blocks), dim3(256), 0, st, pred, target, rows, W, C, ignore_index, d, nseg, res);
    if (int e = launch_status("boundary_rows_kernel")) return e;
    hipLaunchKernelGGL(boundary_cols_kernel, dim3((unsigned)col_blocks), dim3(256), 0, st, pred, target, H, W, C, ignore_index, d, nbx, nby,
                       (const unsigned short*)res, counts, band, nan_flag);
    return launch_status("boundary_cols_kernel");
}
