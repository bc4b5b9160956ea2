// Exponential moving average of the weights: e <- e + (1 - d_t) (p_new - e), fused into the SGD launches of losses.hip so that the
// average costs 8 bytes per parameter on top of the optimiser's 20 instead of a pass of its own (12 bytes and a launch), and the step stays one
// captured graph.  All HBM-bound streaming kernels: float4 main loop, scalar tail, 32-bit indices inside a segment.
//     dsrl_sgd_step_ema / _dev_ema / _dev_segments_ema   the three SGD launches with the average updated from the p they have just computed
//     dsrl_ema_update                                    the unfused update (the BatchNorm buffer arena; the comparison leg of tools/ema_bench.py)
//     dsrl_ema_advance                                   once per step, after the last of the above: updates += 1, the next step's 1 - d_t
//     dsrl_arena_swap                                    exchanges two arenas in place (validation on the averaged weights), bit patterns only
// The EMA record (common.h: EmaRecord) lives in device memory; every kernel but the advance only reads its `omd`, so a replayed graph follows the
// warm-up schedule without a host write.  The SGD arithmetic is that of sgd_kernel / sgd_dev_kernel / sgd_dev_segments_kernel, expression for
// expression (the library is built with -ffp-contract=off): p and buf come out bit-identical to the launches without the average.
#include "common.h"
#include <algorithm>

namespace dsrl {

// one element of torch.optim.SGD(momentum, weight_decay) as losses.hip writes it: buf = mom * buf + (wd * p + g * gscale); p -= lr * buf
__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, float lr, float mom, float wd, float gscale) {
    b = mom * b + fmaf(wd, p, g * gscale);
    p -= lr * b;
}
__device__ __forceinline__ void sgd_ema4(float4& pv, const float4 gv, float4& bv, float4& ev, float lr, float mom, float wd, float gscale, float omd) {
    sgd_elem(pv.x, gv.x, bv.x, lr, mom, wd, gscale); ev.x = ema_elem(ev.x, pv.x, omd);
    sgd_elem(pv.y, gv.y, bv.y, lr, mom, wd, gscale); ev.y = ema_elem(ev.y, pv.y, omd);
    sgd_elem(pv.z, gv.z, bv.z, lr, mom, wd, gscale); ev.z = ema_elem(ev.z, pv.z, omd);
    sgd_elem(pv.w, gv.w, bv.w, lr, mom, wd, gscale); ev.w = ema_elem(ev.w, pv.w, omd);
}
// the grid-stride body of sgd_kernel / sgd_dev_kernel with the average
__device__ __forceinline__ void sgd_ema_range(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float* __restrict__ ema, long long n,
                                              float lr, float mom, float wd, float gscale, float omd) {
    const long long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* b4 = reinterpret_cast<float4*>(buf); float4* e4 = reinterpret_cast<float4*>(ema);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        float4 pv = p4[e]; const float4 gv = g4[e]; float4 bv = b4[e]; float4 ev = e4[e];
        sgd_ema4(pv, gv, bv, ev, lr, mom, wd, gscale, omd);
        p4[e] = pv; b4[e] = bv; e4[e] = ev;
    }
    for (long long e = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        float pv = p[e], bv = buf[e];
        sgd_elem(pv, g[e], bv, lr, mom, wd, gscale);
        buf[e] = bv; p[e] = pv; ema[e] = ema_elem(ema[e], pv, omd);
    }
}
__global__ __launch_bounds__(256) void sgd_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float* __restrict__ ema,
                                                       long long n, float lr, float mom, float wd, float gscale, const EmaRecord* __restrict__ rec) {
    sgd_ema_range(p, g, buf, ema, n, lr, mom, wd, gscale, rec->omd);
}
__global__ __launch_bounds__(256) void sgd_dev_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float* __restrict__ ema,
                                                           long long n, const float* __restrict__ hyper, const EmaRecord* __restrict__ rec) {
    sgd_ema_range(p, g, buf, ema, n, hyper[0], hyper[1], hyper[2], hyper[3], rec->omd);
}
// sgd_dev_segments_kernel with the average: one block per table row {first float, floats, amax record or 0}; the record receives max |p_new| as before
__global__ __launch_bounds__(256) void sgd_dev_segments_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float* __restrict__ ema,
                                                                    const long long* __restrict__ table, const float* __restrict__ hyper,
                                                                    const EmaRecord* __restrict__ erec) {
    const float lr = hyper[0], mom = hyper[1], wd = hyper[2], gscale = hyper[3], omd = erec->omd;
    const long long* row = table + 3ll * blockIdx.x;
    const long long off = row[0];
    const int n4 = (int)(row[1] >> 2);
    unsigned* rec = reinterpret_cast<unsigned*>(row[2]);
    float4* p4 = reinterpret_cast<float4*>(p + off); const float4* g4 = reinterpret_cast<const float4*>(g + off);
    float4* b4 = reinterpret_cast<float4*>(buf + off); float4* e4 = reinterpret_cast<float4*>(ema + off);
    unsigned m = 0u;
    for (int e = threadIdx.x; e < n4; e += 256) {
        float4 pv = p4[e]; const float4 gv = g4[e]; float4 bv = b4[e]; float4 ev = e4[e];
        sgd_ema4(pv, gv, bv, ev, lr, mom, wd, gscale, omd);
        p4[e] = pv; b4[e] = bv; e4[e] = ev;
        m = abs_bits4(m, pv.x, pv.y, pv.z, pv.w);
    }
    amax_publish(m, rec);           // every thread of the block reaches it; a null record publishes nothing
}
// e <- e + omd (p - e) on its own
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long long n, const EmaRecord* __restrict__ rec) {
    const float omd = rec->omd;
    const long long n4 = n >> 2;
    float4* e4 = reinterpret_cast<float4*>(ema); const float4* p4 = reinterpret_cast<const float4*>(p);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        float4 ev = e4[e]; const float4 pv = p4[e];
        ev.x = ema_elem(ev.x, pv.x, omd); ev.y = ema_elem(ev.y, pv.y, omd); ev.z = ema_elem(ev.z, pv.z, omd); ev.w = ema_elem(ev.w, pv.w, omd);
        e4[e] = ev;
    }
    for (long long e = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        ema[e] = ema_elem(ema[e], p[e], omd);
}
// The schedule, one thread: t = updates + 1 averages have been formed; the next one decays by d = min(decay_max, (1 + t) / (10 + t)) under warm-up
// (the rule of tf.train.ExponentialMovingAverage(num_updates=) and timm's warm-up), else by decay_max.  The division is correctly rounded, so a host
// that evaluates the same formula in fp32 gets the same bits.
__global__ void ema_advance_kernel(EmaRecord* __restrict__ rec) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned t = rec->updates + 1u;
    float d = rec->decay_max;
    if (rec->warmup) d = fminf(d, __fdiv_rn(1.f + (float)t, 10.f + (float)t));
    rec->updates = t;
    rec->omd = 1.f - d;
}
// a <-> b, 16 bytes per lane and array; integer registers, so that no bit pattern (NaN payloads, -0, denormals) is touched
__global__ __launch_bounds__(256) void arena_swap_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, long long n) {
    const long long n4 = n >> 2;
    uint4* a4 = reinterpret_cast<uint4*>(a); uint4* b4 = reinterpret_cast<uint4*>(b);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        const uint4 av = a4[e], bv = b4[e];
        a4[e] = bv; b4[e] = av;
    }
    for (long long e = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const unsigned av = a[e], bv = b[e];
        a[e] = bv; b[e] = av;
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
static inline unsigned stream_grid(long long n) { return (unsigned)std::min<long long>(ceil_div(n, 1024), 4096); }

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_sgd_step_ema(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                                 float* ema, const void* ema_record, dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && buf && ema && ema_record && n > 0, DSRL_E_BADARG, "sgd_step_ema: bad arguments");
    DSRL_REQUIRE(aligned16(p) && aligned16(g) && aligned16(buf) && aligned16(ema) && aligned16(ema_record), DSRL_E_BADARG,
                 "sgd_step_ema: arenas and the EMA record must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(sgd_ema_kernel, dim3(stream_grid(n)), dim3(256), 0, st, p, g, buf, ema, (long long)n, lr, momentum, weight_decay, grad_scale,
                       (const EmaRecord*)ema_record);
    return launch_status("sgd_ema_kernel");
}
extern "C" int dsrl_sgd_step_dev_ema(float* p, const float* g, float* buf, int64_t n, const float* hyper, float* ema, const void* ema_record,
                                     dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && buf && hyper && ema && ema_record && n > 0, DSRL_E_BADARG, "sgd_step_dev_ema: bad arguments");
    DSRL_REQUIRE(aligned16(p) && aligned16(g) && aligned16(buf) && aligned16(ema) && aligned16(ema_record), DSRL_E_BADARG,
                 "sgd_step_dev_ema: arenas and the EMA record must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(sgd_dev_ema_kernel, dim3(stream_grid(n)), dim3(256), 0, st, p, g, buf, ema, (long long)n, hyper, (const EmaRecord*)ema_record);
    return launch_status("sgd_dev_ema_kernel");
}
extern "C" int dsrl_sgd_step_dev_segments_ema(float* p, const float* g, float* buf, const int64_t* table, int64_t nseg, const float* hyper, float* ema,
                                              const void* ema_record, dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && buf && table && hyper && ema && ema_record && nseg > 0 && nseg < (1ll << 31), DSRL_E_BADARG, "sgd_step_dev_segments_ema: bad arguments");
    DSRL_REQUIRE(aligned16(p) && aligned16(g) && aligned16(buf) && aligned16(ema) && aligned16(ema_record), DSRL_E_BADARG,
                 "sgd_step_dev_segments_ema: arenas and the EMA record must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(sgd_dev_segments_ema_kernel, dim3((unsigned)nseg), dim3(256), 0, st, p, g, buf, ema, (const long long*)table, hyper,
                       (const EmaRecord*)ema_record);
    return launch_status("sgd_dev_segments_ema_kernel");
}
extern "C" int dsrl_ema_update(float* ema, const float* p, int64_t n, const void* ema_record, dsrl_stream_t stream) {
    DSRL_REQUIRE(ema && p && ema_record && n > 0, DSRL_E_BADARG, "ema_update: bad arguments");
    DSRL_REQUIRE(aligned16(ema) && aligned16(p) && aligned16(ema_record), DSRL_E_BADARG, "ema_update: arenas and the EMA record must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(ema_update_kernel, dim3(stream_grid(n)), dim3(256), 0, st, ema, p, (long long)n, (const EmaRecord*)ema_record);
    return launch_status("ema_update_kernel");
}
extern "C" int dsrl_ema_advance(void* ema_record, dsrl_stream_t stream) {
    DSRL_REQUIRE(ema_record && aligned16(ema_record), DSRL_E_BADARG, "ema_advance: the EMA record must be a 16-byte aligned device address");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, st, (EmaRecord*)ema_record);
    return launch_status("ema_advance_kernel");
}
extern "C" int dsrl_arena_swap(float* a, float* b, int64_t n, dsrl_stream_t stream) {
    DSRL_REQUIRE(a && b && n > 0, DSRL_E_BADARG, "arena_swap: bad arguments");
    DSRL_REQUIRE(aligned16(a) && aligned16(b), DSRL_E_BADARG, "arena_swap: arenas must be 16-byte aligned");
    DSRL_REQUIRE(a + n <= b || b + n <= a, DSRL_E_BADARG, "arena_swap: the arenas overlap");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(arena_swap_kernel, dim3(stream_grid(n)), dim3(256), 0, st, reinterpret_cast<unsigned*>(a), reinterpret_cast<unsigned*>(b), (long long)n);
    return launch_status("arena_swap_kernel");
}
