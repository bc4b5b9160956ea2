// AdamW on the flat arenas: torch.optim.AdamW(lr, betas, eps, weight_decay) - one group, decoupled decay, no amsgrad, no maximize -
// as the launches of the SGD family, one for one, so that ddp.FlatParams swaps the optimiser without touching the captured step around it.
//     dsrl_adamw_step / _dev / _dev_segments             host hyper-parameters; the 4-float device record SGD reads ({lr, unused, weight_decay, grad_scale});
//                                                        the segment table that also leaves max |p_new| in every filter's amax record
//     dsrl_adamw_step_ema / _dev_ema / _dev_segments_ema the same with the weight average updated from the p still in registers (ema_elem)
//     dsrl_adamw_advance / dsrl_adamw_set_step           one thread: t and the bias-correction factors of step t, in double, into the AdamW record
// All HBM-bound streaming kernels over seven arenas (p, g, m, v read; p, m, v written; +2 with the average): float4 main loop, scalar tail, the SGD
// kernels' grid rule, no LDS and no atomics beside the amax publish.  The arithmetic is adamw_elem (common.h) everywhere: every form gives the same bits.
#include "common.h"
#include <algorithm>

namespace dsrl {

template <bool EMA>
__device__ __forceinline__ void adamw4(float4& pv, const float4 gv, float4& mv, float4& vv, float4& ev, const AdamwCoef& c, float omd) {
    adamw_elem(pv.x, gv.x, mv.x, vv.x, c); adamw_elem(pv.y, gv.y, mv.y, vv.y, c); adamw_elem(pv.z, gv.z, mv.z, vv.z, c); adamw_elem(pv.w, gv.w, mv.w, vv.w, c);
    if constexpr (EMA) {
        ev.x = ema_elem(ev.x, pv.x, omd); ev.y = ema_elem(ev.y, pv.y, omd); ev.z = ema_elem(ev.z, pv.z, omd); ev.w = ema_elem(ev.w, pv.w, omd);
    }
}
// DEV: {lr, -, wd, grad_scale} from the device floats `hyper` instead of the launch arguments.  Without EMA `ema` and `erec` are null and never touched.
template <bool DEV, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                     float* __restrict__ ema, long long n, float lr, float wd, float gscale, const float* __restrict__ hyper,
                                                     const AdamwRecord* __restrict__ rec, const EmaRecord* __restrict__ erec) {
    if constexpr (DEV) { lr = hyper[0]; wd = hyper[2]; gscale = hyper[3]; }
    const AdamwCoef c = adamw_coef(lr, wd, gscale, rec);
    float omd = 0.f;
    if constexpr (EMA) omd = erec->omd;
    const long long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m); float4* v4 = reinterpret_cast<float4*>(v); float4* e4 = reinterpret_cast<float4*>(ema);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x) {
        float4 pv = p4[e]; const float4 gv = g4[e]; float4 mv = m4[e]; float4 vv = v4[e]; float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (EMA) ev = e4[e];
        adamw4<EMA>(pv, gv, mv, vv, ev, c, omd);
        p4[e] = pv; m4[e] = mv; v4[e] = vv;
        if constexpr (EMA) e4[e] = ev;
    }
    for (long long e = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        float pv = p[e], mv = m[e], vv = v[e];
        adamw_elem(pv, g[e], mv, vv, c);
        p[e] = pv; m[e] = mv; v[e] = vv;
        if constexpr (EMA) ema[e] = ema_elem(ema[e], pv, omd);
    }
}
// one block per table row {first float, floats, amax record or 0}, as sgd_dev_segments_kernel: the record receives max |p_new| of what the block wrote
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_dev_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                                  float* __restrict__ ema, const long long* __restrict__ table, const float* __restrict__ hyper,
                                                                  const AdamwRecord* __restrict__ arec, const EmaRecord* __restrict__ erec) {
    const AdamwCoef c = adamw_coef(hyper[0], hyper[2], hyper[3], arec);
    float omd = 0.f;
    if constexpr (EMA) omd = erec->omd;
    const long long* row = table + 3ll * blockIdx.x;
    const long long off = row[0];
    const int n4 = (int)(row[1] >> 2);
    unsigned* rec = reinterpret_cast<unsigned*>(row[2]);
    float4* p4 = reinterpret_cast<float4*>(p + off); const float4* g4 = reinterpret_cast<const float4*>(g + off);
    float4* m4 = reinterpret_cast<float4*>(m + off); float4* v4 = reinterpret_cast<float4*>(v + off);
    float4* e4 = EMA ? reinterpret_cast<float4*>(ema + off) : nullptr;
    unsigned mx = 0u;
    // not unrolled: left alone the compiler unrolls this 32-bit loop around the division and square-root expansions into 343 VGPRs and spills -
    // one wave per SIMD -, while the grid-stride kernel above, which it leaves rolled, needs 47 and hides the loads by occupancy
#pragma unroll 1
    for (int e = threadIdx.x; e < n4; e += 256) {
        float4 pv = p4[e]; const float4 gv = g4[e]; float4 mv = m4[e]; float4 vv = v4[e]; float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (EMA) ev = e4[e];
        adamw4<EMA>(pv, gv, mv, vv, ev, c, omd);
        p4[e] = pv; m4[e] = mv; v4[e] = vv;
        if constexpr (EMA) e4[e] = ev;
        mx = abs_bits4(mx, pv.x, pv.y, pv.z, pv.w);
    }
    amax_publish(mx, rec);          // every thread of the block reaches it; a null record publishes nothing
}
// t and the factors of step t, one thread.  In double from t itself - not a running product - so that set_step(t) and t advances give the same bits;
// beta^t underflows to 0 for large t and both factors settle at 1.
__device__ __forceinline__ void adamw_factors(AdamwRecord* __restrict__ rec, long long t) {
    const double c1 = 1.0 - pow(rec->beta1_d, (double)t), c2 = 1.0 - pow(rec->beta2_d, (double)t);
    rec->t = t;
    rec->ss_factor = (float)(1.0 / c1);
    rec->isq = (float)(1.0 / sqrt(c2));
}
__global__ void adamw_advance_kernel(AdamwRecord* __restrict__ rec) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    adamw_factors(rec, rec->t + 1);
}
__global__ void adamw_set_step_kernel(AdamwRecord* __restrict__ rec, long long t) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    adamw_factors(rec, t);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
static inline unsigned stream_grid(long long n) { return (unsigned)std::min<long long>(ceil_div(n, 1024), 4096); }

template <bool DEV, bool EMA>
static int launch_adamw(const char* what, float* p, const float* g, float* m, float* v, int64_t n, float lr, float wd, float gscale, const float* hyper,
                        const void* record, float* ema, const void* ema_record, dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && m && v && record && n > 0 && (!DEV || hyper) && (!EMA || (ema && ema_record)), DSRL_E_BADARG, "%s: bad arguments", what);
    DSRL_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(record) && aligned16(ema) && aligned16(ema_record), DSRL_E_BADARG,
                 "%s: arenas and records must be 16-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL((adamw_kernel<DEV, EMA>), dim3(stream_grid(n)), dim3(256), 0, st, p, g, m, v, ema, (long long)n, lr, wd, gscale, hyper,
                       (const AdamwRecord*)record, (const EmaRecord*)ema_record);
    return launch_status(what);
}
template <bool EMA>
static int launch_adamw_segments(const char* what, float* p, const float* g, float* m, float* v, const int64_t* table, int64_t nseg, const float* hyper,
                                 const void* record, float* ema, const void* ema_record, dsrl_stream_t stream) {
    DSRL_REQUIRE(p && g && m && v && table && hyper && record && nseg > 0 && nseg < (1ll << 31) && (!EMA || (ema && ema_record)), DSRL_E_BADARG,
                 "%s: bad arguments", what);
    DSRL_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(record) && aligned16(ema) && aligned16(ema_record), DSRL_E_BADARG,
                 "%s: arenas and records must be 16-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL((adamw_dev_segments_kernel<EMA>), dim3((unsigned)nseg), dim3(256), 0, st, p, g, m, v, ema, (const long long*)table, hyper,
                       (const AdamwRecord*)record, (const EmaRecord*)ema_record);
    return launch_status(what);
}

}  // namespace dsrl

using namespace dsrl;

extern "C" int dsrl_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float weight_decay, float grad_scale, const void* record,
                               dsrl_stream_t stream) {
    return launch_adamw<false, false>("adamw_step", p, g, m, v, n, lr, weight_decay, grad_scale, nullptr, record, nullptr, nullptr, stream);
}
extern "C" int dsrl_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, const void* record, dsrl_stream_t stream) {
    return launch_adamw<true, false>("adamw_step_dev", p, g, m, v, n, 0.f, 0.f, 0.f, hyper, record, nullptr, nullptr, stream);
}
extern "C" int dsrl_adamw_step_dev_segments(float* p, const float* g, float* m, float* v, const int64_t* table, int64_t nseg, const float* hyper,
                                            const void* record, dsrl_stream_t stream) {
    return launch_adamw_segments<false>("adamw_step_dev_segments", p, g, m, v, table, nseg, hyper, record, nullptr, nullptr, stream);
}
extern "C" int dsrl_adamw_step_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, float weight_decay, float grad_scale, const void* record,
                                   float* ema, const void* ema_record, dsrl_stream_t stream) {
    return launch_adamw<false, true>("adamw_step_ema", p, g, m, v, n, lr, weight_decay, grad_scale, nullptr, record, ema, ema_record, stream);
}
extern "C" int dsrl_adamw_step_dev_ema(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, const void* record, float* ema,
                                       const void* ema_record, dsrl_stream_t stream) {
    return launch_adamw<true, true>("adamw_step_dev_ema", p, g, m, v, n, 0.f, 0.f, 0.f, hyper, record, ema, ema_record, stream);
}
extern "C" int dsrl_adamw_step_dev_segments_ema(float* p, const float* g, float* m, float* v, const int64_t* table, int64_t nseg, const float* hyper,
                                                const void* record, float* ema, const void* ema_record, dsrl_stream_t stream) {
    return launch_adamw_segments<true>("adamw_step_dev_segments_ema", p, g, m, v, table, nseg, hyper, record, ema, ema_record, stream);
}
extern "C" int dsrl_adamw_advance(void* record, dsrl_stream_t stream) {
    DSRL_REQUIRE(record && aligned16(record), DSRL_E_BADARG, "adamw_advance: the AdamW record must be a 16-byte aligned device address");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(64), 0, st, (AdamwRecord*)record);
    return launch_status("adamw_advance_kernel");
}
extern "C" int dsrl_adamw_set_step(void* record, int64_t t, dsrl_stream_t stream) {
    DSRL_REQUIRE(record && aligned16(record) && t >= 0, DSRL_E_BADARG, "adamw_set_step: a 16-byte aligned device record and t >= 0 expected");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bind_stream_device(st)) return e;
    hipLaunchKernelGGL(adamw_set_step_kernel, dim3(1), dim3(64), 0, st, (AdamwRecord*)record, (long long)t);
    return launch_status("adamw_set_step_kernel");
}
