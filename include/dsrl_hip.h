/*
 * dsrl_hip.h - C ABI of libdsrl_hip.so: the MI355X (gfx950) arithmetic of the DSRL stage-3 training hot path.
 *
 * The reference (sanje2v/DualSuperResLearningForSemSeg) has no FFI of its own: every operation below
 * replaces the torch.nn call the reference makes at the cited file:line (paths under /root/reference).
 * The host side (dualsuperreslearningforsemseg_amd/functional.py) binds these with ctypes and keeps the
 * reference's nn.Module surface above them; INTEGRATION.md shows the binding a reference maintainer adds.
 *
 * Conventions
 *   - fp32 only. Activations are "pixel-major": element (n,h,w,c) of a logical NCHW tensor lives at
 *     ((n*H + h)*W + w)*ld + c   (= torch.channels_last); `ld` >= C is the pixel stride in floats, so a
 *     channel slice of a concatenation buffer is addressed by (ptr + first_channel, ld = total channels).
 *   - Conv weights are [K][R][S][C] (= torch (K,C,R,S) in channels_last), ConvTranspose weights are the
 *     plain torch layout (Cin,Cout,2,2).
 *   - Every function enqueues on `stream` (a hipStream_t) and returns immediately; no allocation, no host
 *     synchronisation (the two read-out functions dsrl_prof_read and dsrl_bn_fused_barrier_timeouts excepted); re-entrant from
 *     the autograd worker thread. Process-wide state is limited to four settings (dsrl_conv_precision, dsrl_bn_fused_max_blocks,
 *     dsrl_prof_enable, dsrl_rng_bind_device_key) and the self-resetting arrival counter of the fused BatchNorm kernels'
 *     device-wide barrier. The fused BatchNorm launches of one device share that counter, so they must not overlap each other: the
 *     first one pins its stream, launches on any other stream (outside graph capture) take the three-kernel path.
 *   - The caller owns all buffers including `ws` (workspace, >= the matching *_workspace_bytes()).
 *   - Return 0 on success, a negative DSRL_E_* otherwise; dsrl_last_error() has the message (thread-local).
 */
#ifndef DSRL_HIP_H
#define DSRL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSRL_ABI_VERSION 1

#define DSRL_OK 0
#define DSRL_E_BADARG (-1)      /* inconsistent shape / null pointer / alignment                      */
#define DSRL_E_UNSUPPORTED (-2) /* shape outside what the kernels implement                            */
#define DSRL_E_WORKSPACE (-3)   /* workspace too small                                                 */
#define DSRL_E_LAUNCH (-4)      /* hipGetLastError() after launch                                      */

typedef void* dsrl_stream_t; /* hipStream_t */

int dsrl_version(void);
const char* dsrl_last_error(void);
/* fills cu_count; returns 0 only on a gfx950 device */
int dsrl_device_check(int* cu_count);

/* ------------------------------------------------------------------------------------------------
 * conv2d: implicit GEMM on the matrix cores; fp32 in / out / accumulate, products formed as dsrl_conv_precision selects
 * (default: "f16x3" split-precision fp16 MFMAs = fp32-equivalent in every pass; mode 0: v_mfma_f32_32x32x2_f32).
 * replaces nn.Conv2d forward/backward at ASPP.py:10-15,19; DSRL.py:19-23,34-38,42-46,50,78-83 and the
 * ResNet101.py convolutions; x (N,H,W,C) -> y (N,Ho,Wo,K).
 * ---------------------------------------------------------------------------------------------- */
size_t dsrl_conv2d_fwd_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil);
int dsrl_conv2d_fwd(const float* x, int ldx, const float* w, const float* bias /*nullable*/, float* y, int ldy,
                    int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                    void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* The same conv that additionally leaves BatchNorm partials of its output in `stats`: [3][parts][K] floats = (count, mean, centred
 * second moment) per (block of output rows, output channel), parts = dsrl_conv2d_fwd_stats_parts(shape) for the current arithmetic mode
 * (0: this launch cannot provide them - exact-fp32 kernels, some split-K plans, more than 4096 row blocks). The BatchNorm that follows
 * (ASPP.py:19-20, DSRL.py:22-24,36-40,44-48, every ResNet block) then skips its own statistics pass: dsrl_bn_train_fwd_from_stats. */
int dsrl_conv2d_fwd_stats_parts(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil);
int dsrl_conv2d_fwd_stats(const float* x, int ldx, const float* w, const float* bias /*nullable*/, float* y, int ldy,
                          int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                          void* ws, size_t ws_bytes, float* stats, int stats_parts, dsrl_stream_t stream);
/* dx (N,H,W,C) from dy (N,Ho,Wo,K). The kernel reads the filter as wt[c][tap][k] (k padded to a multiple of 4): pass `wt` from
 * dsrl_conv2d_transpose_filter (e.g. built during the forward pass on another stream) or NULL to have it built here in `ws`. */
size_t dsrl_conv2d_transposed_filter_floats(int C, int K, int R, int S);
int dsrl_conv2d_transpose_filter(const float* w, float* wt, int C, int K, int R, int S, dsrl_stream_t stream);
/* The same for n filters in one launch (once per training step instead of once per layer): table is a DEVICE array of n rows of ten
 * int64 {w pointer, wt pointer, K, Kp = K rounded up to 4, R*S, C, index of the row's first 32x32 tile, ceil(C/32), amax pointer, 0}, rows
 * ordered by first tile; total_tiles = sum over rows of R*S * ceil(C/32) * ceil(Kp/32). A non-zero amax pointer names an amax record
 * (DSRL_AMAX_WORDS uint32, zeroed by the caller before the launch) into which the launch maxes the bit pattern of max |w| of that filter:
 * the filter's operand magnitude for the "f16x3" arithmetic (dsrl_amax, dsrl_conv2d_*_amax below). */
int dsrl_conv2d_transpose_filters_batched(const int64_t* table, int n, int64_t total_tiles, dsrl_stream_t stream);
/* The amax records of all filters in one streaming launch (what the transpose above leaves as a by-product, without the transposes: the per-step filter
 * pass of the "f16x3" arithmetic needs only the records and the split forms below).  table: nseg rows of 3 int64 {pointer into a filter's contiguous
 * [K][R][S][C] storage, number of floats of this segment (<= dsrl_conv2d_filters_amax_segment_floats()), amax record of that filter}; the caller
 * zeroes the records; a filter is cut into as many segments as it needs. */
int dsrl_conv2d_filters_amax_segment_floats(void);
int dsrl_conv2d_filters_amax_batched(const int64_t* table, int64_t nseg, dsrl_stream_t stream);

/* Filters pre-split for the "f16x3" arithmetic, all filters in one launch behind the transpose above (which leaves the amax records this
 * launch scales by): table rows {w, wt_split, K, Kp, R*S, C, first tile, ceil(C/32), amax record, w_split}; w_split [K][R][S][C] and
 * wt_split [C][R][S][Kp] (either may be 0) hold, per 4 consecutive elements of the last dimension, the 4 fp16 first terms of v * 2^e
 * followed by the 4 second terms: 16 bytes for 16 bytes of fp32, indexed like w / wt. dsrl_conv2d_fwd_amax / _dgrad_amax take them as
 * w_split / wt_split together with the SAME amax record and then stage the filter operand without splitting it in every row tile. */
int dsrl_conv2d_split_filters_batched(const int64_t* table, int n, int64_t total_tiles, dsrl_stream_t stream);
size_t dsrl_conv2d_dgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil);
int dsrl_conv2d_dgrad(const float* dy, int lddy, const float* w, const float* wt /*nullable*/, float* dx, int lddx,
                      int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                      void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* dgrad of a conv whose input was y = relu(bn(x)) (or bn(x)): besides dx = the gradient w.r.t. y, the launch leaves the BatchNorm-backward
 * partial sums of g = dx * [y > 0] and g * xhat per (block of rows, channel) in bstats [2][parts][C], parts =
 * dsrl_conv2d_dgrad_stats_parts(shape) (0: this launch cannot - exact-fp32 kernels, split-K slabs, more than 4096 row blocks). The
 * BatchNorm backward then needs no reduction of its own: dsrl_bn_bwd_from_stats. bn_y may be null when bn_relu = 0. */
int dsrl_conv2d_dgrad_stats_parts(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil);
int dsrl_conv2d_dgrad_bnstats(const float* dy, int lddy, const float* w, const float* wt /*nullable*/, float* dx, int lddx,
                              int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                              void* ws, size_t ws_bytes, const float* bn_x, int bn_ldx, const float* bn_y /*nullable*/, int bn_ldy,
                              const float* bn_mean, const float* bn_invstd, int bn_relu, float* bstats, int stats_parts,
                              int accumulate /* dx += ..., the sums are taken of the accumulated values */, dsrl_stream_t stream);
/* Does a conv launch with these properties run the row epilogue (float4 rows of the LDS-parked tile, csrc/conv_common.h: RowEpilogue) in the
 * current arithmetic mode?  The host rule every launcher uses, for tests and tools; it changes no size query.  dgrad: 1 data gradient, 0 forward;
 * bm x bn: block tile; kg: K groups; parity: 1 = rows in parity order (strided data gradients); splits / coop: split-K plan and whether it reduces
 * inside the launch; channels, ldy, y_addr: output channels, row stride (floats) and address of the tensor written; accumulate: y += ...;
 * bn_sums: BatchNorm-backward sums asked for, bn_fast: the 16-byte conditions of those sums hold (multiples of 4, 16-byte aligned operands, extents
 * below 2 GiB); fwd_stats: forward BatchNorm partials asked for.  DSRL_ROW_EPILOGUE=0: always 0. */
int dsrl_conv2d_row_epilogue_supported(int dgrad, int bm, int bn, int kg, int stride, int parity, int splits, int coop, int channels, int ldy,
                                       size_t y_addr, int accumulate, int bn_sums, int bn_fast, int fwd_stats);
/* dx += dgrad(dy, w): the same computation accumulated onto the existing contents of dx (a tensor that feeds two branches receives
 * both gradient contributions in one buffer, e.g. the input of a ResNet bottleneck: ResNet101.py residual add + conv1). */
int dsrl_conv2d_dgrad_accumulate(const float* dy, int lddy, const float* w, const float* wt /*nullable*/, float* dx, int lddx,
                                 int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                                 void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* dw [K][R][S][C] from x and dy */
size_t dsrl_conv2d_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil);
int dsrl_conv2d_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw,
                      int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                      void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* Grouped weight gradients: every dsrl_conv2d_wgrad of a backward pass as a few grids (one per tile configuration, blocks ordered
 * longest first) plus one slab reduce, instead of one launch + reduce per layer. The weight gradients of a pass depend on nothing
 * but (x, dy) of their layer and are read by the optimiser only, so the caller may collect the problems while backward runs and
 * launch them once at its end (ddp.FlatParams does). Split-precision arithmetics only (dsrl_conv_precision 1..4).
 *   1. ws  = dsrl_conv2d_wgrad_group_workspace_bytes(problems, n); table = dsrl_conv2d_wgrad_group_table_bytes(n)
 *   2. dsrl_conv2d_wgrad_group_plan(problems, n, host_table, table, dev_table, ws_ptr, ws)  - fills host_table (host memory) with
 *      device-side descriptors that hold absolute device pointers (x, dy, dw, slabs inside ws_ptr) and offsets valid for dev_table
 *   3. the caller copies host_table -> dev_table (table bytes, stream-ordered before step 4; from pinned memory if asynchronous)
 *   4. dsrl_conv2d_wgrad_group_launch(host_table, dev_table, stream)
 * Same results as n calls of dsrl_conv2d_wgrad up to the summation order over pixel ranges. */
typedef struct dsrl_wgrad_problem {
    const float* x; const float* dy; float* dw;
    int32_t ldx, lddy, N, H, W, C, K, R, S, stride, pad, dil;
    const uint32_t* x_amax; const uint32_t* dy_amax;      /* "f16x3" arithmetic: operand magnitudes of x and dy (required there, else unused) */
} dsrl_wgrad_problem;
size_t dsrl_conv2d_wgrad_group_table_bytes(int n);
size_t dsrl_conv2d_wgrad_group_workspace_bytes(const dsrl_wgrad_problem* problems, int n);
int dsrl_conv2d_wgrad_group_plan(const dsrl_wgrad_problem* problems, int n, void* host_table, size_t table_bytes, const void* dev_table,
                                 void* ws, size_t ws_bytes);
int dsrl_conv2d_wgrad_group_launch(const void* host_table, const void* dev_table, dsrl_stream_t stream);
/* Operand magnitudes for the "f16x3" arithmetic (dsrl_conv_precision 4). That arithmetic carries every operand as two fp16 terms of
 * x * 2^e, with e chosen per TENSOR so that the tensor's largest magnitude lands in [2^14, 2^15); it therefore needs max |x| of both
 * operands of a launch, as an "amax record": DSRL_AMAX_WORDS uint32 device words (1 KiB, 64-byte aligned) of which every 16th holds the
 * bit pattern of a partial maximum of |x| (the writers' atomics are spread over 16 cache lines; the maximum of the record is max |x|).
 * Producers can leave the record while they write the tensor (the y_amax / dx_amax arguments of the BatchNorm kernels, the batched filter
 * transpose above); dsrl_amax measures any pixel-major tensor: it maxes into the record atomically, the caller zeroes the record first
 * (several calls may share a record).
 * The *_amax entry points below are dsrl_conv2d_fwd(_stats) / _dgrad(_bnstats, _accumulate) / _wgrad with the two records passed in; a
 * null record - and every call through the plain entry points - is measured by the call itself (one extra pass over that operand, in
 * the last 2 KiB of the workspace, which the *_workspace_bytes queries include). The other arithmetics ignore the records.
 * dsrl_conv2d_fwd_amax: stats may be null (no BatchNorm partials); dsrl_conv2d_dgrad_amax: bstats may be null (no BatchNorm sums; the
 * bn_* arguments are then unused), accumulate as in dsrl_conv2d_dgrad_accumulate. */
#define DSRL_AMAX_WORDS 256
int dsrl_amax(const float* x, int ld, int64_t P, int C, uint32_t* amax, dsrl_stream_t stream);
int dsrl_conv2d_fwd_amax(const float* x, int ldx, const uint32_t* x_amax, const float* w, const uint32_t* w_amax, const void* w_split /*nullable*/,
                         const float* bias /*nullable*/, float* y, int ldy, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                         void* ws, size_t ws_bytes, float* stats /*nullable*/, int stats_parts, dsrl_stream_t stream);
int dsrl_conv2d_dgrad_amax(const float* dy, int lddy, const uint32_t* dy_amax, const float* w, const float* wt /*nullable*/, const uint32_t* w_amax,
                           const void* wt_split /*nullable*/, float* dx, int lddx, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                           void* ws, size_t ws_bytes, const float* bn_x, int bn_ldx, const float* bn_y, int bn_ldy,
                           const float* bn_mean, const float* bn_invstd, int bn_relu, float* bstats /*nullable*/, int stats_parts, int accumulate,
                           dsrl_stream_t stream);
/* fp16 PLANES (round 4): an operand tensor of the "f16x3" arithmetic stored as its two terms, hi = f16(v * 2^e) and lo = f16(v * 2^e - hi) with e from
 * the tensor's amax record, each plane with the tensor's own indexing ([P][ld] fp16 for a pixel-major activation, [K][R][S][C] / [C][R][S][K] for a filter
 * and its transpose); the second plane starts dsrl_planes_lo_offset(elements of one plane) bytes behind the first. The conv kernels then stage operands by
 * LDS-DMA (buffer_load ... lds) without conversion. dsrl_planes_bytes: size of a plane buffer (nplanes 1 or 2).
 * dsrl_split_planes: planes of a pixel-major fp32 tensor (C and ld multiples of 8, 16-byte aligned), scaled by `amax` (a measured record, see dsrl_amax).
 * dsrl_conv2d_filter_planes_batched: all filters of a model in one launch; table rows of 10 int64 {w, wt_planes, K, unused, R*S, C, first tile,
 * ceil(C/32), amax record, w_planes} with tiles counted as R*S * ceil(C/32) * ceil(K/32) per filter; K and C multiples of 8; either pointer may be 0.
 * dsrl_conv2d_fwd_planes / _dgrad_planes: dsrl_conv2d_fwd_amax / _dgrad_amax with the plane forms passed as well (nullable); a launch that cannot
 * use them runs exactly as the _amax call; with the same tile plan the results are bit-identical to it. */
size_t dsrl_planes_lo_offset(int64_t elems);
size_t dsrl_planes_bytes(int64_t elems, int nplanes);
int dsrl_split_planes(const float* x, int ld, int64_t P, int C, const uint32_t* amax, void* planes, int nplanes, dsrl_stream_t stream);
int dsrl_conv2d_filter_planes_batched(const int64_t* table, int n, int64_t total_tiles, dsrl_stream_t stream);
int dsrl_conv2d_fwd_planes(const float* x, int ldx, const uint32_t* x_amax, const void* x_planes /*nullable*/, const float* w, const uint32_t* w_amax,
                           const void* w_split /*nullable*/, const void* w_planes /*nullable*/, const float* bias /*nullable*/, float* y, int ldy,
                           int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                           void* ws, size_t ws_bytes, float* stats /*nullable*/, int stats_parts, dsrl_stream_t stream);
int dsrl_conv2d_dgrad_planes(const float* dy, int lddy, const uint32_t* dy_amax, const void* dy_planes /*nullable*/, const float* w, const float* wt /*nullable*/,
                             const uint32_t* w_amax, const void* wt_split /*nullable*/, const void* wt_planes /*nullable*/, float* dx, int lddx,
                             int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                             void* ws, size_t ws_bytes, const float* bn_x, int bn_ldx, const float* bn_y, int bn_ldy,
                             const float* bn_mean, const float* bn_invstd, int bn_relu, float* bstats /*nullable*/, int stats_parts, int accumulate,
                             dsrl_stream_t stream);
/* the same with a Dropout(p) between the BatchNorm's ReLU and this conv (DSRL.py:38-41,46-49: cat_conv): bn_y is the tensor BEHIND the dropout, whose zeros are the
 * combined mask, and the sums are taken of g = dy / (1 - p) where bn_y > 0 (round 5) */
int dsrl_conv2d_dgrad_planes_drop(const float* dy, int lddy, const uint32_t* dy_amax, const void* dy_planes /*nullable*/, const float* w, const float* wt /*nullable*/,
                             const uint32_t* w_amax, const void* wt_split /*nullable*/, const void* wt_planes /*nullable*/, float* dx, int lddx,
                             int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                             void* ws, size_t ws_bytes, const float* bn_x, int bn_ldx, const float* bn_y, int bn_ldy,
                             const float* bn_mean, const float* bn_invstd, int bn_relu, float bn_drop_p, float* bstats /*nullable*/, int stats_parts, int accumulate,
                             dsrl_stream_t stream);
int dsrl_conv2d_wgrad_amax(const float* x, int ldx, const uint32_t* x_amax, const float* dy, int lddy, const uint32_t* dy_amax, float* dw,
                           int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil,
                           void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* Arithmetic of the implicit-GEMM conv kernels (forward, dgrad, wgrad, row-folded stem), process-wide. fp32 in, fp32 out and fp32
 * accumulation in every mode; the modes differ in how the products are formed on the matrix cores:
 *   0  v_mfma_f32_32x32x2_f32 (exact fp32 products)
 *   1  "bf16x3": operand = 2 bf16 terms (16 mantissa bits), 3 bf16 MFMAs per product; ~5e-6 relative error per conv
 *   2  "bf16x6": operand = 3 bf16 terms (24 mantissa bits), 6 bf16 MFMAs per product; error vs fp64 equal to mode 0
 *   3  "mixed": forward bf16x6, dgrad / wgrad bf16x3 (reduced-precision gradients, ~5e-6)
 *   4  "f16x3": operand = 2 fp16 terms of the per-tensor scaled value (22 mantissa bits), 3 fp16 MFMAs per product; error vs fp64 equal
 *      to modes 0 and 2 at half the matrix work of mode 2 (operand magnitudes: see dsrl_amax above); the default
 *   5  "f16x1": operand = ONE fp16 term of the per-tensor scaled value (11 significand bits), one fp16 MFMA per product, fp32 accumulation:
 *      the arithmetic of the reference's apex O1 / O2 runs (train_or_resume.py:68-72) - reduced precision (~5e-4 of the output range per conv);
 *      the operand scales of mode 4 stand in for loss scaling
 *  -1  follow the environment variable DSRL_CONV_PRECISION (unset = 4)
 * Any other value changes nothing (query). Returns the previous setting. */
int dsrl_conv_precision(int mode);
/* in-bounds multiply-accumulates of one forward conv (zero-padding taps excluded): the roofline numerator */
int64_t dsrl_conv2d_inbounds_macs(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dil);

/* Row-folded conv for few-channel inputs (the 7x7 stride-2 RGB stem, ResNet101.py:28): the caller pre-pads the image
 * physically (dsrl_pad_image_nhwc) and folds the S horizontal taps into the channel axis, so that one filter row is ONE
 * contiguous run of Cfold = S*ldx floats per output pixel: y[n,ho,wo,k] = sum_{r<R} sum_{c<Cfold} x[n, ho*stride + r, wo*stride, c] * w[k][r][c]
 * (c runs over neighbouring pixels). Requires (Ho-1)*stride + R <= H and (Wo-1)*stride*ldx + Cfold <= W*ldx.
 * algorithmic_macs is only bookkeeping for the launch timer (the true conv's in-bounds MACs). */
size_t dsrl_conv2d_rowfold_fwd_workspace_bytes(int N, int H, int W, int Cfold, int K, int R, int stride, int Ho, int Wo);
int dsrl_conv2d_rowfold_fwd(const float* x, int ldx, const float* w, const float* bias /*nullable*/, float* y, int ldy,
                            int N, int H, int W, int Cfold, int K, int R, int stride, int Ho, int Wo, int64_t algorithmic_macs,
                            void* ws, size_t ws_bytes, dsrl_stream_t stream);
size_t dsrl_conv2d_rowfold_wgrad_workspace_bytes(int N, int H, int W, int Cfold, int K, int R, int stride, int Ho, int Wo);
/* dw [K][R][Cfold] */
int dsrl_conv2d_rowfold_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw,
                              int N, int H, int W, int Cfold, int K, int R, int stride, int Ho, int Wo, int64_t algorithmic_macs,
                              void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* y (N,Hp,Wp,Cp) pixel-major, zero except y[n, top+h, left+w, c] = x[n*sn + c*sc + h*sh + w*sw] for c < C */
int dsrl_pad_image_nhwc(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float* y,
                        int N, int C, int H, int W, int Cp, int top, int left, int Hp, int Wp, dsrl_stream_t stream);

/* column sums: out[c] = sum_p x[p*ld + c]  (conv / convT bias gradients, DSRL.py:50,64-69,78-83) */
size_t dsrl_colsum_workspace_bytes(int64_t P, int C);
int dsrl_colsum(const float* x, int ld, int64_t P, int C, float* out, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (+ optional residual add, ReLU, Dropout) - nn.BatchNorm2d/ReLU/Dropout at ASPP.py:20-21,
 * DSRL.py:24-25,39-41,47-49,61-63,94-95 and the ResNet bottlenecks.
 * ---------------------------------------------------------------------------------------------- */
size_t dsrl_bn_workspace_bytes(int64_t P, int C);
/* training statistics: mean[c], invstd[c] = 1/sqrt(biased var + eps); running stats updated in place
 * (unbiased var, momentum) when non-null */
int dsrl_bn_stats(const float* x, int ldx, int64_t P, int C, float eps, float momentum,
                  float* mean, float* invstd, float* running_mean /*nullable*/, float* running_var /*nullable*/,
                  void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* invstd[c] = 1/sqrt(running_var[c] + eps) (eval mode / frozen BN, train_or_resume.py:379-382) */
int dsrl_bn_invstd_from_var(const float* running_var, int C, float eps, float* invstd, dsrl_stream_t stream);
/* y = dropout(relu((x-mean)*invstd*gamma + beta + residual)); flags: bit0 relu; dropout when p > 0.
 * y_amax / dx_amax (here and in the four functions below; nullable): an amax record (dsrl_amax), zeroed by the caller, into which the
 * launch maxes the bit pattern of max |.| of the tensor it writes - the operand magnitude of the "f16x3" conv arithmetic, taken while
 * the tensor is written instead of by a pass of its own. */
int dsrl_bn_apply(const float* x, int ldx, float* y, int ldy, int64_t P, int C,
                  const float* mean, const float* invstd, const float* gamma, const float* beta,
                  const float* residual /*nullable*/, int ldr, int relu, float drop_p, uint64_t seed, uint32_t rng_stream,
                  uint32_t* y_amax /*nullable*/, dsrl_stream_t stream);
/* dsrl_bn_train_fwd with the batch statistics taken from the partials a preceding dsrl_conv2d_fwd_stats left behind (C a multiple of 32):
 * one streaming kernel, no statistics pass over x, no device-wide barrier. Same outputs as dsrl_bn_train_fwd. More than 256 row blocks of
 * partials (up to 4096: the 65536-pixel layers) are first reduced to 32 by a small launch, into the room behind the partials: a partials
 * buffer holds dsrl_bn_stats_floats(rows = 3 here / 2 for dsrl_bn_bwd_from_stats, parts, C) floats. */
size_t dsrl_bn_stats_floats(int rows, int parts, int C);
int dsrl_bn_train_fwd_from_stats(const float* x, int ldx, float* y, int ldy, int64_t P, int C, float eps, float momentum, float* mean, float* invstd,
                                 float* running_mean /*nullable*/, float* running_var /*nullable*/, const float* gamma, const float* beta,
                                 const float* residual /*nullable*/, int ldr, int relu, float drop_p, uint64_t seed, uint32_t rng_stream,
                                 float* stats, int stats_parts, uint32_t* y_amax /*nullable*/, dsrl_stream_t stream);
/* ... that also leaves the sign mask of the stored y (behind residual add, ReLU and Dropout): mask [C / 32][P] 32-bit words, dsrl_bn_mask_words(P, C)
 * of them (0 when C is no multiple of 32), bit j of word (g, p) set iff y[p][32 g + j] > 0.  y, mean, invstd, the running statistics and y_amax are
 * those of dsrl_bn_train_fwd_from_stats; mask == NULL is that call.  Readers take the mask in place of y: relu (bn_relu) == 2 in
 * dsrl_bn_bwd_from_stats / _drop / _res and in dsrl_conv2d_dgrad_bnstats / _amax / _planes / _planes_drop means that the y (bn_y) pointer addresses
 * the mask and ldy (bn_ldy) is its row length P - one bit instead of four bytes per element, the same gradients bit for bit.  In those calls relu
 * (bn_relu) must be 0, 1 (y is the output) or 2 (y is the mask); any other value is DSRL_E_BADARG. */
size_t dsrl_bn_mask_words(int64_t P, int C);
int dsrl_bn_train_fwd_from_stats_mask(const float* x, int ldx, float* y, int ldy, int64_t P, int C, float eps, float momentum, float* mean, float* invstd,
                                      float* running_mean /*nullable*/, float* running_var /*nullable*/, const float* gamma, const float* beta,
                                      const float* residual /*nullable*/, int ldr, int relu, float drop_p, uint64_t seed, uint32_t rng_stream,
                                      float* stats, int stats_parts, uint32_t* y_amax /*nullable*/, uint32_t* mask /*nullable*/, dsrl_stream_t stream);
/* The fused small-tensor BN kernels (dsrl_bn_train_fwd / dsrl_bn_bwd) cross a device-wide barrier: all blocks of a launch (128, or
 * 256 for tensors of 4.2-8.4 M elements; one 512-thread block per CU) must become resident together, so they assume that the process
 * has the GPU to itself apart from its own streams. dsrl_bn_fused_max_blocks: 0 = never use them, 128 = the 128-block variant only (what
 * ddp.FlatParams selects when RCCL kernels share the device), 256 = both, -1 = follow DSRL_BN_FUSED / DSRL_BN_FUSED_BIG; other values
 * change nothing; returns the previous setting. A block that waits for seconds gives up, poisons its outputs with NaN and counts in
 * dsrl_bn_fused_barrier_timeouts (synchronous read). */
int dsrl_bn_fused_max_blocks(int max_blocks);
int dsrl_bn_fused_barrier_timeouts(int64_t* count);
/* Training-mode BatchNorm2d forward in one call: batch statistics (as dsrl_bn_stats: mean / invstd out, running stats updated in place)
 * and y = act(gamma * xhat + beta (+ residual)) (as dsrl_bn_apply). Small tensors (C a power-of-two multiple of 32, P*C <= 4.2 M) take a
 * single fused kernel that reads x once; everything else runs the statistics and apply kernels. nn.BatchNorm2d (+ReLU, +Dropout) of
 * ASPP.py:20-21, DSRL.py:24-25,39-41,47-49 and of every backbone block (ResNet101.py). Workspace: dsrl_bn_workspace_bytes(P, C). */
int dsrl_bn_train_fwd(const float* x, int ldx, float* y, int ldy, int64_t P, int C, float eps, float momentum, float* mean, float* invstd,
                      float* running_mean /*nullable*/, float* running_var /*nullable*/, const float* gamma, const float* beta,
                      const float* residual /*nullable*/, int ldr, int relu, float drop_p, uint64_t seed, uint32_t rng_stream,
                      void* ws, size_t ws_bytes, uint32_t* y_amax /*nullable*/, dsrl_stream_t stream);
/* backward of dsrl_bn_apply. y is the forward output (mask = y > 0 covers relu and dropout).
 * training != 0: batch-statistics gradient; == 0: statistics are constants. dresidual nullable. */
int dsrl_bn_bwd(const float* x, int ldx, const float* y, int ldy, const float* dy, int lddy,
                float* dx, int lddx, float* dresidual /*nullable*/, int lddr, int64_t P, int C,
                const float* mean, const float* invstd, const float* gamma,
                float* dgamma, float* dbeta, int relu, float drop_p, int training,
                void* ws, size_t ws_bytes, uint32_t* dx_amax /*nullable*/, dsrl_stream_t stream);
/* dsrl_bn_bwd (without dropout) with the two per-channel sums taken from the partials of dsrl_conv2d_dgrad_bnstats: one streaming kernel,
 * no reduction pass, no device-wide barrier (C a multiple of 32). */
int dsrl_bn_bwd_from_stats(const float* x, int ldx, const float* y /*nullable*/, int ldy, const float* dy, int lddy, float* dx, int lddx,
                           float* dresidual /*nullable*/, int lddr, int64_t P, int C, const float* mean, const float* invstd, const float* gamma,
                           float* dgamma /*nullable*/, float* dbeta /*nullable*/, int relu, int training, float* stats, int stats_parts,
                           uint32_t* dx_amax /*nullable*/, dsrl_stream_t stream);
/* ... with a Dropout(p) behind the ReLU: y is the tensor behind the dropout (mask y > 0, factor 1 / (1 - p)) */
int dsrl_bn_bwd_from_stats_drop(const float* x, int ldx, const float* y /*nullable*/, int ldy, const float* dy, int lddy, float* dx, int lddx,
                           float* dresidual /*nullable*/, int lddr, int64_t P, int C, const float* mean, const float* invstd, const float* gamma,
                           float* dgamma /*nullable*/, float* dbeta /*nullable*/, int relu, float drop_p, int training, float* stats, int stats_parts,
                           uint32_t* dx_amax /*nullable*/, dsrl_stream_t stream);
/* ... when the residual added before the ReLU is itself the output of a BatchNorm without ReLU - the downsample branch of a layer's first bottleneck,
 * out = relu(bn3(.) + bn_ds(conv_ds(x))), models/modules/backbone/ResNet101.py:67-89 (torchvision Bottleneck.forward) - its output gradient is the masked
 * gradient this launch writes to dresidual (required).  Given that BatchNorm's input res_x (pixel stride res_ldx) and batch statistics, the launch also
 * leaves ITS two backward sums per (row block, channel) in res_stats [2][res_parts][C] (room per dsrl_bn_stats_floats(2, res_parts, C)), res_parts =
 * dsrl_bn_bwd_from_stats_res_parts(P, C, stats_parts): the downsample BatchNorm's backward then is dsrl_bn_bwd_from_stats on dresidual - one streaming
 * launch instead of a reduction pass + apply pass (or the device-wide-barrier kernel) over the same tensors. */
int dsrl_bn_bwd_from_stats_res_parts(int64_t P, int C, int stats_parts);
int dsrl_bn_bwd_from_stats_res(const float* x, int ldx, const float* y /*nullable*/, int ldy, const float* dy, int lddy, float* dx, int lddx,
                           float* dresidual, int lddr, int64_t P, int C, const float* mean, const float* invstd, const float* gamma,
                           float* dgamma /*nullable*/, float* dbeta /*nullable*/, int relu, float drop_p, int training, float* stats, int stats_parts,
                           uint32_t* dx_amax /*nullable*/, const float* res_x, int res_ldx, const float* res_mean, const float* res_invstd,
                           float* res_stats, int res_parts, dsrl_stream_t stream);

/* Device-resident dropout key. By default every dropout-bearing launch (dsrl_bn_apply, dsrl_bn_train_fwd*, dsrl_dropout_*) bakes its
 * `seed` argument into the launch. After dsrl_rng_bind_device_key(ptr) the kernels of the CURRENT device ignore that argument and read
 * the 64-bit key at `ptr` when they run, so launches captured in a hipGraph draw fresh masks on every replay; NULL restores the
 * default. dsrl_rng_advance_key(state) enqueues the per-step key derivation on three device words {key, step, base}:
 * step += 1; key = base * 1000003 + step (mod 2^64) - the derivation functional.begin_forward() performs on the host. */
int dsrl_rng_bind_device_key(const uint64_t* dev_key /*nullable*/);
int dsrl_rng_advance_key(uint64_t* state /*device: key, step, base*/, dsrl_stream_t stream);

/* standalone Dropout (DSRL.py:54): Philox4x32-10 keyed by (seed, rng_stream), element index = p*C + c */
int dsrl_dropout_fwd(const float* x, int ldx, float* y, int ldy, int64_t P, int C, float p, uint64_t seed, uint32_t rng_stream, dsrl_stream_t stream);
int dsrl_dropout_bwd(const float* dy, int lddy, float* dx, int lddx, int64_t P, int C, float p, uint64_t seed, uint32_t rng_stream, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * bilinear resize, align_corners=True (ASPP.py:41, DSRL.py:53, DSRL.py:163) and pools
 * ---------------------------------------------------------------------------------------------- */
int dsrl_bilinear_ac_fwd(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int Ho, int Wo, dsrl_stream_t stream);
size_t dsrl_bilinear_ac_bwd_workspace_bytes(int N, int H, int W, int C, int Ho, int Wo);
int dsrl_bilinear_ac_bwd(const float* dy, int lddy, float* dx, int lddx, int N, int H, int W, int C, int Ho, int Wo,
                         void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* nn.AdaptiveAvgPool2d((1,1)) (ASPP.py:22,38) */
int dsrl_global_avgpool_fwd(const float* x, int ldx, float* y, int N, int HW, int C, dsrl_stream_t stream);
int dsrl_global_avgpool_bwd(const float* dy, float* dx, int lddx, int N, int HW, int C, dsrl_stream_t stream);
/* nn.MaxPool2d(3, stride 2, pad 1) (ResNet101.py:32) */
/* argmax (nullable in fwd): per output element the winning tap r*3+s (first maximum in scan order), consumed by the backward.
 * torch's scan: it starts at the first in-bounds tap and a tap replaces the best on `v > best || isnan(v)`, so the tap is always an
 * in-bounds one (an all -inf window: its first in-bounds element) and the last of several NaNs wins. */
int dsrl_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* argmax, int N, int H, int W, int C, dsrl_stream_t stream);
int dsrl_maxpool3x3s2_bwd(const uint8_t* argmax, const float* dy, float* dx, int N, int H, int W, int C, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ConvTranspose2d(kernel 2, stride 2, pad 0) (DSRL.py:55-60, 64-69); w is (Cin,Cout,2,2) contiguous
 * ---------------------------------------------------------------------------------------------- */
int dsrl_convt2x2_fwd(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H, int W, int Cin, int Cout, dsrl_stream_t stream);
size_t dsrl_convt2x2_bwd_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int dsrl_convt2x2_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* dbias /*nullable*/,
                      int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* dsrl_convt2x2_fwd that also evaluates nn.CrossEntropyLoss(ignore_index), mean reduction, of its output against `target` (N,2H,2W bytes) while the
 * output tile is in LDS (DSRL.py:69 -> train_or_resume.py:435): loss_out[0] = the loss, loss_out[1] = the number of pixels that count, as
 * dsrl_ce_fused writes them; nan_flag (nullable) bit 0 = NaN logit, bit 1 = label outside [0, Cout).  19 -> 19 channels, W % 4 == 0. */
int dsrl_convt2x2_fwd_ce_supported(const float* x, const float* y, int N, int H, int W, int Cin, int Cout);
size_t dsrl_convt2x2_fwd_ce_workspace_bytes(int N, int H, int W);
int dsrl_convt2x2_fwd_ce(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H, int W, int Cin, int Cout,
                         const uint8_t* target, int ignore_index, float* loss_out, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* The same backward when y IS the logits of nn.CrossEntropyLoss(ignore_index) with mean reduction (DSRL.py:69 feeds train_or_resume.py:435) and the
 * loss is the root of the backward pass with unit gradient: dy = d(CE)/d(logits) is formed inside the kernel from `logits` (the forward output y),
 * `target` (N,2H,2W bytes) and `ce_count` (the number of pixels that are not ignore_index, dsrl_ce_fused's loss_out[1]), in the arithmetic of
 * dsrl_ce_fused, and never written to memory.  ft_g (nullable): the incoming gradient (N, ceil(2H/s), ceil(2W/s)) of the stride-s single-channel 1x1
 * conv that also reads the logits (feature transformer, DSRL.py:88-93) and ft_w its Cout weights: g * w_c is added on the stride grid, as
 * dsrl_pointwise_strided_bwd(accumulate = 1) would.  Results are bit-identical to dsrl_ce_fused -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd.
 * _supported: 1 when the shape can take this path (19 -> 19 channels, W % 128 == 0, 16-byte aligned tensors); otherwise use the three calls. */
int dsrl_convt2x2_bwd_ce_supported(const float* x, const float* logits, const uint8_t* target, int N, int H, int W, int Cin, int Cout);
int dsrl_convt2x2_bwd_ce(const float* x, const float* w, const float* logits, const uint8_t* target, int ignore_index, const float* ce_count,
                         const float* ft_g /*nullable*/, const float* ft_w /*nullable*/, int ft_stride, float* dx, float* dw, float* dbias /*nullable*/,
                         int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* nn.PixelShuffle(r) (DSRL.py:84): x (N,H,W,c*r*r) -> y (N,H*r,W*r,c) */
int dsrl_pixel_shuffle_fwd(const float* x, float* y, int N, int H, int W, int c, int r, dsrl_stream_t stream);
int dsrl_pixel_shuffle_bwd(const float* dy, float* dx, int N, int H, int W, int c, int r, dsrl_stream_t stream);

/* 1x1 stride-s conv with a single output channel, no bias (feature transformers, DSRL.py:88-93) */
int dsrl_pointwise_strided_fwd(const float* x, const float* w, float* y, int N, int H, int W, int C, int stride, dsrl_stream_t stream);
size_t dsrl_pointwise_strided_bwd_workspace_bytes(int N, int H, int W, int C, int stride);
/* dx is fully written (zeros off the stride grid) when accumulate == 0, dx += on the stride grid only when 1; 2: dw only (dx may be null) */
int dsrl_pointwise_strided_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, int accumulate,
                               int N, int H, int W, int C, int stride, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* channel concatenation (ASPP.py:44, DSRL.py:165): dst[p*ld_dst + c] = src[p*ld_src + c], c < C (strided 2-D copy) */
int dsrl_copy2d(const float* src, int ld_src, float* dst, int ld_dst, int64_t P, int C, dsrl_stream_t stream);
/* the whole concatenation as one launch (round 5): sources srcs[i] (HOST array of n <= 8 device pointers; pixel strides lds[i], widths cs[i], all multiples of
 * 4, 16-byte aligned) written side by side into dst (pixel stride ld_dst), and max |value| of everything written left in the amax record `amax`
 * (nullable) - the consumers of a concatenated buffer (ASPP.py:44 -> the 1280 -> 256 projection; DSRL.py:165 -> cat_conv.0 and the SISR conv) need that
 * magnitude for their operand scale and used to measure it with a pass of its own.  dsrl_cat_channels_supported: 1 when the arguments qualify (the
 * kernel indexes float4 with 32 bits: P * stride / 4 < 2^31 for every tensor). */
int dsrl_cat_channels_supported(const float* const* srcs, const int* lds, const int* cs, int n, const float* dst, int ld_dst, int64_t P);
int dsrl_cat_channels(const float* const* srcs, const int* lds, const int* cs, int n, float* dst, int ld_dst, int64_t P, uint32_t* amax, dsrl_stream_t stream);

/* layout converters at the boundary (NCHW image in, ResNet101.py:92): y has Cpad >= C channels, extra = 0 */
int dsrl_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, int Cpad, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * losses (train_or_resume.py:116-119, 435-438)
 * ---------------------------------------------------------------------------------------------- */
size_t dsrl_ce_workspace_bytes(int64_t P);
/* nn.CrossEntropyLoss(ignore_index): logits [P][C] pixel-major, target uint8 [P]; loss_out[0] = mean NLL over
 * valid pixels, loss_out[1] = number of valid pixels */
int dsrl_ce_fwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index,
                float* loss_out, void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* dlogits = (softmax - onehot) * grad_out[0] / n_valid ; loss_out is the pair written by dsrl_ce_fwd */
int dsrl_ce_bwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index,
                const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream);
size_t dsrl_mse_workspace_bytes(int64_t n);
int dsrl_mse_fwd(const float* a, const float* b, int64_t n, float* loss_out, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_mse_bwd(const float* a, const float* b, int64_t n, const float* grad_out, float* da, dsrl_stream_t stream);
/* Fused loss pass (train_or_resume.py:116-117, 426-438): ONE pass over the logits computes CrossEntropyLoss(ignore_index,
 * mean) into loss_out[0] (loss_out[1] = pixels counted) AND writes d(loss)/d(logits) for an upstream gradient of 1 into dlogits
 * (nullable: forward only), and ORs 1 into nan_flag (nullable) if a logit is NaN. dsrl_mse_fused does the same for MSELoss:
 * da = grad_scale * d(mse)/da. dsrl_loss_mix writes {CE, w1*MSE, w2*FA, sum, (float)*nan_flag} to vals[5] (mse / fa nullable: stages 1, 2). */
size_t dsrl_ce_fused_workspace_bytes(int64_t P);
int dsrl_ce_fused(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float* dlogits /*nullable*/, int lddl,
                  float* loss_out /*[2]*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_mse_fused(const float* a, const float* b, int64_t n, float grad_scale, float* da /*nullable*/, float* loss_out, int* nan_flag /*nullable*/,
                   void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_loss_mix(const float* ce, const float* mse /*nullable*/, const float* fa /*nullable*/, float w1, float w2, const int* nan_flag /*nullable*/,
                  float* vals /*[5]*/, dsrl_stream_t stream);

/* Class-weighted cross entropy: nn.CrossEntropyLoss(weight, ignore_index, reduction='mean').  `weights` is a device table of 256 floats indexed
 * directly by the label byte: entries [0, C) hold the class weights (finite, >= 0), entries >= C are zero, so a label outside the classes never
 * reads out of bounds (it still makes the loss NaN and raises flag bit 1).  With nll_i = m_i + log s_i - v_i[t_i]:
 *     n_c  = pixels with t_i == c and t_i != ignore_index                         (exact integers: per-block histograms merged in integers)
 *     D    = fp32(sum over c ascending of (double)n_c * (double)w_c)             (rounded once; identical in every entry point)
 *     loss = (sum_i (double)w[t_i] * (double)nll_i) / D                           (0/0 = NaN when every live pixel has weight 0, as torch)
 *     dl_ic = sc_i * e_ic / s_i - (c == t_i ? sc_i : 0),  sc_i = w[t_i] * (1 / D);  ignored pixel: zeros
 * D takes the place of the pixel count: loss_out[1] = D, and dsrl_convt2x2_bwd_ce_w reads it there.  Everything runs on the stream (no host read),
 * so the calls can be captured.  All-ones weights give the bits of the unweighted entry points while the pixel count is below 2^24.
 * dsrl_ce_weight_sum is the pre-pass alone (d_out[0] = D, summed over the classes [0, C) only); each *_w entry point below runs it first.  The _w forms otherwise keep the contracts
 * of dsrl_ce_fwd / dsrl_ce_bwd / dsrl_ce_fused / dsrl_convt2x2_fwd_ce / dsrl_convt2x2_bwd_ce; the weighted dsrl_convt2x2_bwd_ce_w is bit-identical to
 * dsrl_ce_fused_w -> dsrl_pointwise_strided_bwd(accumulate = 1) -> dsrl_convt2x2_bwd. */
size_t dsrl_ce_weight_sum_workspace_bytes(void);
int dsrl_ce_weight_sum(const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/, float* d_out,
                       void* ws, size_t ws_bytes, dsrl_stream_t stream);
size_t dsrl_ce_w_workspace_bytes(int64_t P);
int dsrl_ce_fwd_w(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/,
                  float* loss_out /*[2]*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_ce_bwd_w(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/,
                  const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream);
size_t dsrl_ce_fused_w_workspace_bytes(int64_t P);
int dsrl_ce_fused_w(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/,
                    float* dlogits /*nullable*/, int lddl, float* loss_out /*[2]*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                    dsrl_stream_t stream);
size_t dsrl_convt2x2_fwd_ce_w_workspace_bytes(int N, int H, int W);
int dsrl_convt2x2_fwd_ce_w(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H, int W, int Cin, int Cout,
                           const uint8_t* target, int ignore_index, const float* weights /*[256]*/, float* loss_out, int* nan_flag /*nullable*/,
                           void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_convt2x2_bwd_ce_w(const float* x, const float* w, const float* logits, const uint8_t* target, int ignore_index, const float* weights /*[256]*/,
                           const float* ce_wsum /*D: loss_out + 1*/, const float* ft_g /*nullable*/, const float* ft_w /*nullable*/, int ft_stride,
                           float* dx, float* dw, float* dbias /*nullable*/, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes,
                           dsrl_stream_t stream);
/* counts[lut ? lut[label] : label] += 1 for each of the P label bytes (counts: 256 accumulated 64-bit counters; 64-bit integer atomics, exact and
 * order independent, like dsrl_seg_metrics).  The label buffer may start at any byte. */
int dsrl_class_histogram(const uint8_t* labels, int64_t P, const uint8_t* lut /*nullable, [256]*/, unsigned long long* counts /*[256]*/,
                         dsrl_stream_t stream);

/* Focal cross entropy (Lin et al.): the weighted loss above with one more per-pixel factor.  For a live pixel with p = softmax(v)[t], q = 1 - p,
 * nll = -log p:
 *     term_i = w[t_i] * q^gamma * nll,   loss = (sum_i term_i) / D,   D as above (the same pre-pass, the same bits)
 *     dl_ic  = sc_i * e_ic / s_i - (c == t_i ? sc_i : 0),  sc_i = (w[t_i] * mod_i) * (1 / D),  mod = q^(gamma-1) * (q + gamma * p * nll)
 * with q = (sum_{c != t} e_c) / s (never 1 - p), nll = (m - v_t) + log s, and the limits q == 0 -> term = 0, mod = 0; p == 0 -> p * nll = 0.
 * `gamma` must be finite and >= 0, else DSRL_E_BADARG and nothing is launched; gamma == 0 runs the _w entry point itself.  Each _f entry point is
 * its _w sibling with `float gamma` after `weights` (all-ones weights for an unweighted focal loss): same contracts, flags and workspaces (the
 * _f size queries are those of the _w siblings), and dsrl_convt2x2_bwd_ce_f is bit-identical to
 * dsrl_ce_fused_f -> dsrl_pointwise_strided_bwd(accumulate = 1) -> dsrl_convt2x2_bwd. */
size_t dsrl_ce_f_workspace_bytes(int64_t P);
int dsrl_ce_fwd_f(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/, float gamma,
                  float* loss_out /*[2]*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_ce_bwd_f(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/, float gamma,
                  const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream);
size_t dsrl_ce_fused_f_workspace_bytes(int64_t P);
int dsrl_ce_fused_f(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/, float gamma,
                    float* dlogits /*nullable*/, int lddl, float* loss_out /*[2]*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                    dsrl_stream_t stream);
size_t dsrl_convt2x2_fwd_ce_f_workspace_bytes(int N, int H, int W);
int dsrl_convt2x2_fwd_ce_f(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H, int W, int Cin, int Cout,
                           const uint8_t* target, int ignore_index, const float* weights /*[256]*/, float gamma, float* loss_out,
                           int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_convt2x2_bwd_ce_f(const float* x, const float* w, const float* logits, const uint8_t* target, int ignore_index, const float* weights /*[256]*/,
                           float gamma, const float* ce_wsum /*D: loss_out + 1*/, const float* ft_g /*nullable*/, const float* ft_w /*nullable*/,
                           int ft_stride, float* dx, float* dw, float* dbias /*nullable*/, int N, int H, int W, int Cin, int Cout, void* ws,
                           size_t ws_bytes, dsrl_stream_t stream);

/* Label-smoothed cross entropy: nn.CrossEntropyLoss(weight=, ignore_index=, label_smoothing=eps).  With C classes, nl_ic = (m_i - v_ic) + log s_i,
 * W = sum_{c < C} w_c and D as above (the same pre-pass, the same bits), over the pixels i whose label is not ignore_index:
 *     loss  = ((1 - eps) sum_i w[t_i] nl_i,t_i + (eps / C) sum_i sum_{c < C, w_c > 0} w_c nl_ic) / D
 *     dl_ic = ((1 - eps) w[t_i] (p_ic - [c == t_i]) + (eps / C) (p_ic W - w_c)) / D,   zeros for an ignored pixel
 * One deviation from torch: a class of weight 0 adds nothing to the smoothing sum even where nl_ic is +inf (torch forms 0 * inf = NaN).  A live pixel
 * whose target has weight 0 still contributes its smoothing term; D == 0 gives what IEEE division gives.  `eps` must satisfy 0 <= eps <= 1 (a NaN
 * does not), else DSRL_E_BADARG and nothing is launched or written; eps == 0 runs the _w entry point itself.  Each _s entry point is its _w sibling
 * with `float eps` after `weights` (all-ones weights for an unweighted smoothed loss): same contracts, flags and workspaces (the _s size queries
 * are those of the _w siblings), and dsrl_convt2x2_bwd_ce_s is bit-identical to
 * dsrl_ce_fused_s -> dsrl_pointwise_strided_bwd(accumulate = 1) -> dsrl_convt2x2_bwd.  There is no smoothed focal loss. */
size_t dsrl_ce_s_workspace_bytes(int64_t P);
int dsrl_ce_fwd_s(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/, float eps,
                  float* loss_out /*[2]*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_ce_bwd_s(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/, float eps,
                  const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream);
size_t dsrl_ce_fused_s_workspace_bytes(int64_t P);
int dsrl_ce_fused_s(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/, float eps,
                    float* dlogits /*nullable*/, int lddl, float* loss_out /*[2]*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                    dsrl_stream_t stream);
size_t dsrl_convt2x2_fwd_ce_s_workspace_bytes(int N, int H, int W);
int dsrl_convt2x2_fwd_ce_s(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H, int W, int Cin, int Cout,
                           const uint8_t* target, int ignore_index, const float* weights /*[256]*/, float eps, float* loss_out,
                           int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_convt2x2_bwd_ce_s(const float* x, const float* w, const float* logits, const uint8_t* target, int ignore_index, const float* weights /*[256]*/,
                           float eps, const float* ce_wsum /*D: loss_out + 1*/, const float* ft_g /*nullable*/, const float* ft_w /*nullable*/,
                           int ft_stride, float* dx, float* dw, float* dbias /*nullable*/, int N, int H, int W, int Cin, int Cout, void* ws,
                           size_t ws_bytes, dsrl_stream_t stream);

/* Boundary label relaxation (Zhu et al., CVPR 2019).  dsrl_relax_mask writes one class-set word per pixel of a (N, H, W) label map:
 *     mask[i] = OR of (1 << t_j) over the pixels j of the (2 radius + 1)^2 window around i, clipped at the borders of i's own image, whose label is
 *               neither ignore_index nor >= C;   0 when t_i itself is ignore_index or >= C
 * radius in [1, 4] and C in [1, 32], checked first: anything else is DSRL_E_BADARG and nothing is launched or written.  Integer work, one launch, no
 * workspace, no host read (graph-capturable).  `stats` (nullable, 8-byte aligned) receives ADDED counts {pixels with t != ignore_index, pixels whose
 * set holds more than one class}: integer atomics, identical run to run.
 * The relaxed cross entropy asks for the probability of the set S_i = (mask_i & ((1 << C) - 1)) | bit(t_i) instead of the label (a caller's word can
 * neither drop the own label nor name a class that does not exist; a word of zeros IS the weighted form, bit for bit).  With m, e_c, s, w and D as
 * for the _w entry points, m_S = max_{c in S} v_c, g_c = [c in S] exp(v_c - m_S), z = sum_{c in S} g_c (c ascending):
 *     loss  = sum_live w[t_i] ((m + log s) - (m_S + log z)) / D          dl_ic = live_i (w[t_i] / D) (e_c / s - g_c / z)
 * Each _r entry point is its _w sibling with `const uint32_t* mask` (P words, or N * 2H * 2W) after `weights` (all-ones weights for an unweighted
 * relaxed loss) and C <= 32: same contracts, flags and workspaces (the _r size queries are those of the _w siblings); dsrl_ce_fused_r and
 * dsrl_ce_fwd_r / dsrl_ce_bwd_r(grad_out = 1) give the same bits, and dsrl_convt2x2_bwd_ce_r is bit-identical to
 * dsrl_ce_fused_r -> dsrl_pointwise_strided_bwd(accumulate = 1) -> dsrl_convt2x2_bwd. */
int dsrl_relax_mask(const uint8_t* target, int N, int H, int W, int C, int ignore_index, int radius, uint32_t* mask,
                    unsigned long long* stats /*[2], nullable*/, dsrl_stream_t stream);
size_t dsrl_ce_r_workspace_bytes(int64_t P);
int dsrl_ce_fwd_r(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/,
                  const uint32_t* mask, float* loss_out /*[2]*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_ce_bwd_r(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/,
                  const uint32_t* mask, const float* loss_out, const float* grad_out, float* dlogits, int lddl, dsrl_stream_t stream);
size_t dsrl_ce_fused_r_workspace_bytes(int64_t P);
int dsrl_ce_fused_r(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* weights /*[256]*/,
                    const uint32_t* mask, float* dlogits /*nullable*/, int lddl, float* loss_out /*[2]*/, int* nan_flag /*nullable*/, void* ws,
                    size_t ws_bytes, dsrl_stream_t stream);
size_t dsrl_convt2x2_fwd_ce_r_workspace_bytes(int N, int H, int W);
int dsrl_convt2x2_fwd_ce_r(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H, int W, int Cin, int Cout,
                           const uint8_t* target, int ignore_index, const float* weights /*[256]*/, const uint32_t* mask, float* loss_out,
                           int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_convt2x2_bwd_ce_r(const float* x, const float* w, const float* logits, const uint8_t* target, int ignore_index, const float* weights /*[256]*/,
                           const uint32_t* mask, const float* ce_wsum /*D: loss_out + 1*/, const float* ft_g /*nullable*/, const float* ft_w /*nullable*/,
                           int ft_stride, float* dx, float* dw, float* dbias /*nullable*/, int N, int H, int W, int Cin, int Cout, void* ws,
                           size_t ws_bytes, dsrl_stream_t stream);

/* Online hard example mining (OHEM) for the cross entropy, as a rewrite of the target: the rule of mmseg's OHEMPixelSampler and HRNet's
 * OhemCrossEntropy.  For one call of P pixels, `thresh` in [0, 1] and min_kept >= 0:
 *     a pixel is a candidate iff target != ignore_index && target < C; every other pixel takes no part and keeps its label
 *     p_i = e_t / s of candidate i in fp32, in the arithmetic of the CE kernels (m = max_c v_c, e_c = exp(v_c - m), s = sum e_c, c ascending);
 *           a NaN p counts as 0 (the pixel is kept) and raises bit 0 of nan_flag, as a NaN sum does in any pixel
 *     n candidates (n == 0: nothing changes), k = min(min_kept, n - 1), v = the k-th smallest p counting from 0, thr = max(v, thresh)
 *     a candidate is kept iff p < thr, strictly; every other candidate gets the label ignore_index
 * The selection is a value threshold found by an exact radix select on the bit patterns of p (non-negative floats order as unsigned integers; four
 * passes of 8-bit digits, per-block integer partial histograms, no float atomics): no tie-breaking by index, the same bytes on every call.
 * n, k and thr are formed on the device and every launch is unconditional: the calls can be captured into a graph.
 *   dsrl_ohem_prob    p_out[i] = p_i, or 2.0f for a pixel that is not a candidate; reads the logits once (ld >= C; 16-byte loads when ld == C and the
 *                     base is 16-byte aligned).
 *   dsrl_ohem_select  stats[4] = {bits of thr, n, number kept, number with p < thresh} from p[P] (any 4-byte aligned buffer: a value >= 2.0f is no
 *                     candidate, a NaN or a value <= 0 counts as 0).  ws: >= dsrl_ohem_workspace_bytes(P), 16-byte aligned.
 *   dsrl_ohem_apply   target_out[i] = (p[i] >= 2.0f || p[i] < thr) ? target[i] : ignore_index, thr read from stats[0]; target_out may be target.
 *   dsrl_ohem_target  the three in order, p kept in ws.  dsrl_ohem_workspace_bytes(P) sizes the p buffer, the partial histograms and the state; it
 *                     depends on P alone (0, with a message, for P <= 0 or P >= 2^31).
 * Argument errors (DSRL_E_BADARG before any HIP call, nothing written): null pointers, P <= 0 or >= 2^31, C outside 1..60, ld < C, thresh outside
 * [0, 1] or NaN, min_kept < 0, ignore_index outside 0..255 (it is written into the target); a workspace too small or misaligned is DSRL_E_WORKSPACE. */
size_t dsrl_ohem_workspace_bytes(int64_t P);
int dsrl_ohem_prob(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float* p_out, int* nan_flag /*nullable*/,
                   dsrl_stream_t stream);
int dsrl_ohem_select(const float* p, int64_t P, float thresh, int64_t min_kept, uint32_t* stats /*[4]*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_ohem_apply(const float* p, const uint8_t* target, int64_t P, int ignore_index, const uint32_t* stats /*[4]*/, uint8_t* target_out,
                    dsrl_stream_t stream);
int dsrl_ohem_target(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float thresh, int64_t min_kept,
                     uint8_t* target_out, uint32_t* stats /*[4]*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* Soft Dice loss term beside the cross entropy: loss = CE + lambda L_dice.  A pixel is live when its label is neither ignore_index
 * nor >= C; p_ic = e_ic (1 / s_i) is its softmax with the terms of the CE kernels (m = max, e_c = exp(v_c - m), s = sum e_c with c ascending).  Over
 * the live pixels of the call:
 *     I_c = sum_i p_ic [t_i == c]     P_c = sum_i p_ic     G_c = sum_i [t_i == c]  (integer)     den_c = P_c + G_c + smooth
 *     K = {c : G_c > 0}     L_dice = 1 - (1 / |K|) sum_{c in K} (2 I_c + smooth) / den_c          (K empty: L_dice = 0 and every coefficient 0)
 *     a_c = -(lambda / |K|) 2 / den_c     b_c = (lambda / |K|) (2 I_c + smooth) / den_c^2          (c not in K: 0)
 *     d(lambda L_dice) / d v_ik = live_i p_ik (g_ik - sum_j p_ij g_ij),   g_ij = b_j + a_j [j == t_i]       (sum over j ascending)
 * The mean is over the classes PRESENT in the call; an absent class adds nothing.
 *   dsrl_dice_fwd  one pass over the logits (ld >= C; 16-byte loads when ld == C and the base is 16-byte aligned) leaves partial sums per chunk of
 *                  pixels (I_c, P_c in double, G_c in integers; the pixel -> chunk mapping depends on P alone), a one-block finish adds them in
 *                  a fixed ascending order (the chunks of each group of 64, then the groups) and writes record[128] = {lambda L_dice, |K|, a[0..C), b[0..C), zeros}, the coefficients formed in double
 *                  and rounded once.  No float atomics: the same bits on every call.  A NaN logit in a live pixel ORs 1 into nan_flag and makes the
 *                  value NaN.  After the call ws begins with the totals {double I[64], double P[64], uint32 G[64]}.
 *                  ws: >= dsrl_dice_workspace_bytes(P) (depends on P alone; 0, with a message, for P <= 0 or P >= 2^31 - 256), 8-byte aligned.
 *   dsrl_dice_bwd  dlogits[i][k] = the row above from the logits and the record (accumulate = 0), or dlogits + row (accumulate = 1, one fp32
 *                  addition per element; a pixel that is not live adds +0).
 *   dsrl_convt2x2_bwd_ce_d  dsrl_convt2x2_bwd_ce_w with the Dice row added to the weighted CE row inside the kernel (all-ones weights for an
 *                  unweighted CE): bit-identical to dsrl_ce_fused_w -> dsrl_dice_bwd(accumulate = 1) -> dsrl_pointwise_strided_bwd(accumulate = 1)
 *                  -> dsrl_convt2x2_bwd.  Same contract and workspace as the _w entry point.
 * Everything runs on the stream with no host read: the calls can be captured.  Argument errors (DSRL_E_BADARG before any HIP call, nothing written):
 * null pointers, P <= 0 or >= 2^31 - 256, C outside 1..60, ld or lddl < C, lambda not a finite number > 0, smooth not a finite number >= 0,
 * accumulate not 0 or 1; a workspace too small or misaligned is DSRL_E_WORKSPACE. */
size_t dsrl_dice_workspace_bytes(int64_t P);
int dsrl_dice_fwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float lambda, float smooth,
                  float* record /*[128]*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_dice_bwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* record /*[128]*/, int accumulate,
                  float* dlogits, int lddl, dsrl_stream_t stream);
int dsrl_convt2x2_bwd_ce_d(const float* x, const float* w, const float* logits, const uint8_t* target, int ignore_index, const float* weights /*[256]*/,
                           const float* dice_record /*[128]*/, const float* ce_wsum /*D: loss_out + 1*/, const float* ft_g /*nullable*/,
                           const float* ft_w /*nullable*/, int ft_stride, float* dx, float* dw, float* dbias /*nullable*/, int N, int H, int W, int Cin,
                           int Cout, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* Lovasz-Softmax loss term beside the cross entropy (Berman et al., CVPR 2018), in its QUANTISED form: loss = CE + lambda L.  A pixel
 * is live when its label is neither ignore_index nor >= C; p_ic = e_ic (1 / s_i) is its softmax with the terms of the CE kernels (m = max,
 * e_c = exp(v_c - m), s = sum e_c with c ascending).  K = bins levels:
 *     err_ic = |[t_i == c] - p_ic|     b_ic = min(K - 1, max(0, floor(err_ic K)))     e^_b = (b + 1/2) / K
 * Per class c over the live pixels of the call: nf_c[b] / nb_c[b] = the foreground (t_i == c) / background pixels in level b, G_c = sum_b nf_c[b], and
 * from the top level down NFincl_c[b] = sum_{b' >= b} nf_c[b'], NBincl_c[b] = sum_{b' >= b} nb_c[b'], NBabove_c[b] = NBincl_c[b] - nb_c[b]:
 *     wf_c[b] = 1 / (G_c + NBabove_c[b])          wb_c[b] = (G_c - NFincl_c[b]) / ((G_c + NBabove_c[b]) (G_c + NBincl_c[b]))
 *     L_c = sum_b e^_b (nf_c[b] wf_c[b] + nb_c[b] wb_c[b])
 *     Present = {c : G_c > 0}     L = (1 / |Present|) sum_{c in Present} L_c          (Present empty: L = 0 and every table entry 0)
 * This is the exact Lovasz extension of the Jaccard loss at the quantised errors (ties: foreground first; the value does not depend on the order
 * among ties), within 1 / (2 K) of the unquantised loss; classes = 'present', over the batch (per_image = False).  The gradient treats the ranking
 * as constant, as autograd does in the sorted implementation (straight-through over the quantisation):
 *     g_ic = (c == t_i ? gf_c : gb_c)[b_ic],   gf = -(lambda / |Present|) wf,   gb = +(lambda / |Present|) wb          (c not in Present: 0)
 *     d(lambda L) / d v_ik = live_i p_ik (g_ik - sum_j p_ij g_ij)          (sum over j ascending)
 *   dsrl_lovasz_record_floats(C, bins) = 4 + 2 C bins: record = {lambda L, |Present|, 0, 0, gf[C][bins], gb[C][bins]}, the tables formed in double and
 *                  rounded once.  dsrl_lovasz_workspace_bytes(P, C, bins) = 2 C bins uint32 + 784.  Both depend on their arguments alone (0, with a
 *                  message, for arguments out of range).
 *   dsrl_lovasz_fwd  clears its workspace on the stream, makes one pass over the logits (ld >= C; 16-byte loads when ld == C and the base is 16-byte
 *                  aligned; one pass per group of classes when C x bins packed words do not fit LDS beside the tile: 19 x 1024 do, 19 x 4096 take
 *                  three) into per-block LDS histograms flushed with 32-bit integer atomics, scans every class from the top level down and writes
 *                  the record.  Integers only up to the tables, no float atomics: the same bits on every call.  After the call ws begins with
 *                  uint32 nf[C][bins], nb[C][bins].  A NaN logit in a live pixel ORs 1 into nan_flag and makes record[0] NaN (its levels are still in
 *                  range).  ws: 16-byte aligned.
 *   dsrl_lovasz_bwd  dlogits[i][k] = the row above from the logits and the record (accumulate = 0), or dlogits + row (accumulate = 1, one fp32
 *                  addition per element; a pixel that is not live adds +0).
 *   dsrl_convt2x2_bwd_ce_l  dsrl_convt2x2_bwd_ce_w with the Lovasz row added to the weighted CE row inside the kernel (all-ones weights for an
 *                  unweighted CE), the tables gathered from global memory: bit-identical to dsrl_ce_fused_w -> dsrl_lovasz_bwd(accumulate = 1) ->
 *                  dsrl_pointwise_strided_bwd(accumulate = 1) -> dsrl_convt2x2_bwd.  Same contract and workspace as the _w entry point.
 * Everything runs on the stream with no host read: the calls can be captured.  Argument errors (DSRL_E_BADARG before any HIP call, nothing written):
 * null pointers, P <= 0 or >= 2^31 - 256, C outside 1..60, ld or lddl < C, lambda not a finite number > 0, bins not a power of two in [16, 4096],
 * accumulate not 0 or 1; a workspace too small or misaligned is DSRL_E_WORKSPACE. */
size_t dsrl_lovasz_workspace_bytes(int64_t P, int C, int bins);
size_t dsrl_lovasz_record_floats(int C, int bins);
int dsrl_lovasz_fwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, float lambda, int bins, float* record,
                    int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_lovasz_bwd(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* record, int bins, int accumulate,
                    float* dlogits, int lddl, dsrl_stream_t stream);
int dsrl_convt2x2_bwd_ce_l(const float* x, const float* w, const float* logits, const uint8_t* target, int ignore_index, const float* weights /*[256]*/,
                           const float* lovasz_record, int bins, const float* ce_wsum /*D: loss_out + 1*/, const float* ft_g /*nullable*/,
                           const float* ft_w /*nullable*/, int ft_stride, float* dx, float* dw, float* dbias /*nullable*/, int N, int H, int W, int Cin,
                           int Cout, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* FALoss (models/losses/FALoss.py:8-34). fm1/fm2 are (B,C,H,W) with element strides (sb,sc,sh,sw).
 * reduction: 0 mean, 1 sum, 2 none (out has B*C*n*n floats, n = (W/k)^2).
 * `saved` (>= dsrl_fa_saved_floats) carries S1,S2,sigma,u1,v1 to the backward. */
size_t dsrl_fa_saved_floats(int B, int C, int H, int W, int k);
size_t dsrl_fa_workspace_bytes(int B, int C, int H, int W, int k);
int dsrl_fa_fwd(const float* fm1, const float* fm2, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                int k, int reduction, float* out, float* saved, void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* mean/sum: grad_out is 1 float; d1/d2 are (B,C,H,W) contiguous */
int dsrl_fa_bwd(const float* fm1, const float* fm2, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                int k, int reduction, const float* grad_out, const float* saved, float* d1, float* d2,
                void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * callers / data formats either side of the path
 * ---------------------------------------------------------------------------------------------- */
/* Validation metrics (metrices/mIoU.py:15-41, metrices/Accuracy.py:13-30) straight from the logits: pred = argmax_c logits,
 * counts[0..C) += area_pred, [C..2C) += area_inter, [2C..3C) += area_target, counts[3C] += correct, counts[3C+1] += valid
 * (pixels whose target is the ignore label are excluded everywhere). 64-bit integer atomics: exact and order independent. */
int dsrl_seg_metrics(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index,
                     unsigned long long* counts, dsrl_stream_t stream);
/* Confusion matrix, one convention for every producer: cm is C*C accumulated 64-bit counters, cm[t*C + p] += pixels with target t and predicted
 * class p, counted under the rule of the table above (target != ignore_index && target < C).  Producers ADD and never clear, so one buffer collects a
 * whole split; 64-bit integer atomics, exact and order independent.  On zeroed buffers: row sums = area_target, column sums = area_pred, diagonal =
 * area_inter, total = valid, trace = correct.
 * dsrl_seg_metrics_cm: dsrl_seg_metrics' single pass over the logits (staged, first maximum) with the matrix beside the table; counts is nullable.
 *   C <= dsrl_seg_metrics_cm_max_classes() = 48 (256*C staged floats and C*C bins share the default 64 KB of LDS; dsrl_seg_metrics itself goes to 60):
 *   DSRL_E_UNSUPPORTED above, nothing is launched.
 * dsrl_confusion_matrix: from two class maps of P bytes each; either may start at any byte (aligned 16-byte loads, scalar head and tail; the loads
 *   stay inside the 16-byte granules the maps occupy).  A predicted class >= C on a counted pixel is not counted and raises bit 1 (|= 2) of nan_flag (nullable).
 *   C <= dsrl_confusion_matrix_max_classes() = 64, DSRL_E_UNSUPPORTED above; any P > 0 (launched in spans that keep every 32-bit LDS bin from wrapping). */
int dsrl_seg_metrics_cm_max_classes(void);
int dsrl_seg_metrics_cm(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index,
                        unsigned long long* counts /*nullable*/, unsigned long long* cm /*[C*C]*/, dsrl_stream_t stream);
int dsrl_confusion_matrix_max_classes(void);
int dsrl_confusion_matrix(const uint8_t* pred, const uint8_t* target, int64_t P, int C, int ignore_index, unsigned long long* cm /*[C*C]*/,
                          int* nan_flag /*nullable*/, dsrl_stream_t stream);
/* Deterministic tail of the training input pipeline (JointImageAndLabelTensor.py:9-16 label remap, JointNormalize.py:11,
 * JointScaledImage.py:27-32): from a decoded RGB uint8 crop (N,Hs,Ws,3) and its label-id map (N,Hs,Ws):
 *   img_in  (N,H,W,4)   = align-corners bilinear resize of ((u8/255 - mean)/std) to the model input size, 4th channel 0
 *                         (pixel-major, padded to the 4 channels the stem kernel wants), img_org (N,2H,2W,3) the same at the output size,
 *   target  (N,2H,2W)   = nearest resize of lut[label]                                                                        */
int dsrl_prepare_batch(const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut /*256*/, const float* mean /*3*/, const float* std /*3*/,
                       float* img_in, float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W, dsrl_stream_t stream);

/* Random joint augmentations of the training transform (train_or_resume.py:128-137), one 128-byte row per sample in device memory, drawn and
 * filled on the host (models/transforms DeviceJointAugmentation).  Samples of one launch may differ in every field. */
#define DSRL_AUG_HFLIP 1 /* JointHFlip                                   */
#define DSRL_AUG_BLUR 2  /* JointRandomGaussianBlur(3): blur[] applies    */
#define DSRL_AUG_GRAY 4  /* JointRandomGrayscale                          */
typedef struct dsrl_augment_params {
    double rot[6];      /* PIL Image.rotate's inverse matrix: source = (rot0 x + rot1 y + rot2, rot3 x + rot4 y + rot5) at output pixel centres   */
    int32_t rot_fix[6]; /* the same in 16.16 fixed point for the nearest path: a0, a1, a2 + half-pixel terms, a3, a4, a5 + half-pixel terms       */
    int32_t box[4];     /* crop x, y, width, height in the rotated image, resized back to the full size (0, 0, Ws, Hs: no crop)                  */
    int32_t flags;      /* DSRL_AUG_*                                                                                                              */
    float blur[9];      /* 3x3 Gaussian weights, row-major (torchvision GaussianBlur: outer product of the normalised 1-D kernel)                 */
} dsrl_augment_params;
/* JointRandomRotate (bilinear image, fill 0; nearest labels, fill 255) then JointRandomCrop's resize of the box back to (Ws, Hs) (bilinear image,
 * nearest labels), Pillow-exact on uint8: rgb (N,Hs,Ws,3) -> rgb_out, labels (N,Hs,Ws) raw ids -> labels_out.  label_src (N x (Ws + Hs) int32,
 * device) holds per sample the crop-box source column of every output column, then the source row of every output row, of the nearest label
 * resize: Pillow accumulates them by sequential double additions, which the host repeats.  labels, label_src and labels_out are nullable together.
 * One pass; the outputs must not alias the inputs. */
int dsrl_augment_geometry(const uint8_t* rgb, const uint8_t* labels, const dsrl_augment_params* params /*device, N rows*/, const int32_t* label_src,
                          uint8_t* rgb_out, uint8_t* labels_out, int N, int Hs, int Ws, dsrl_stream_t stream);
/* dsrl_prepare_batch after JointHFlip, JointRandomGaussianBlur (3x3, reflect padding, evaluated at the taps the resize reads) and
 * JointRandomGrayscale as each row's flags select; with every flag clear the output is bit-identical to dsrl_prepare_batch.  Hs, Ws >= 2. */
int dsrl_prepare_batch_augmented(const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut /*256*/, const float* mean /*3*/, const float* std /*3*/,
                                 float* img_in, float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W,
                                 const dsrl_augment_params* params /*device, N rows*/, dsrl_stream_t stream);

/* JointColorJitter (models/transforms/JointColorJitter.py), opt-in: one 64-byte row per sample in device memory beside the dsrl_augment_params rows.
 * On the float image x in [0, 1] (the geometry output / 255, before flip, blur and grayscale) the enabled operations run in the order of
 * order[], each followed by a clamp to [0, 1]; gray(x) = 0.2989 R + 0.587 G + 0.114 B (torchvision 0.8.1 functional_tensor):
 *   brightness  x <- b x;   contrast  x <- c x + (1 - c) m, m = mean of gray(x) over the sample as x is at that point;
 *   saturation  x <- s x + (1 - s) gray(x);   hue  out[j] = sum_i x[i] hue[3 i + j] (the reference's rotation matrix for hue_factor * 2 pi). */
#define DSRL_JITTER_BRIGHTNESS 0
#define DSRL_JITTER_CONTRAST 1
#define DSRL_JITTER_SATURATION 2
#define DSRL_JITTER_HUE 3
typedef struct dsrl_colour_jitter_params {
    int32_t order[4];                      /* DSRL_JITTER_* in application order; -1: a disabled slot; any other value is skipped */
    float brightness, contrast, saturation; /* factors b, c, s                                                                     */
    float hue[9];                          /* row-major 3x3 M, computed on the host in double                                     */
} dsrl_colour_jitter_params;
/* Bytes of workspace dsrl_colour_jitter_means needs for N samples of Hs x Ws: a function of these three alone. */
size_t dsrl_colour_jitter_workspace_bytes(int N, int Hs, int Ws);
/* means[n] = contrast's m (0..1 scale) of sample n of rgb (N,Hs,Ws,3) uint8: the mean over the sample of gray after the operations in front of
 * contrast in that sample's order.  Double partial sums per block, then one wave per sample in a fixed order: no atomics, the same bits on every
 * call with the same buffers.  The entry of a sample without an enabled contrast is left untouched (nothing reads it).  jitter, means 4-byte and
 * ws 8-byte aligned; ws_bytes >= the query (DSRL_E_WORKSPACE otherwise). */
int dsrl_colour_jitter_means(const uint8_t* rgb, const dsrl_colour_jitter_params* jitter /*device, N rows*/, float* means /*device, N*/, void* ws,
                             size_t ws_bytes, int N, int Hs, int Ws, dsrl_stream_t stream);
/* dsrl_prepare_batch_augmented with the colour jitter applied to every uint8 pixel a tap reads (so the blur's nine taps read jittered pixels and no
 * float copy of the full-size image exists); means from dsrl_colour_jitter_means on the same rgb and rows.  jitter and means must not be null. */
int dsrl_prepare_batch_jittered(const uint8_t* rgb, const uint8_t* labels, const uint8_t* lut /*256*/, const float* mean /*3*/, const float* std /*3*/,
                                float* img_in, float* img_org, uint8_t* target, int N, int Hs, int Ws, int H, int W,
                                const dsrl_augment_params* params /*device, N rows*/, const dsrl_colour_jitter_params* jitter /*device, N rows*/,
                                const float* means /*device, N*/, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * optimiser + bookkeeping on the flat parameter arena (train_or_resume.py:63-66, 445, 426-433)
 * ---------------------------------------------------------------------------------------------- */
/* torch.optim.SGD(momentum, weight_decay): d = g*grad_scale + wd*p; buf = mom*buf + d; p -= lr*buf */
int dsrl_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay,
                  float grad_scale, dsrl_stream_t stream);
/* the same update with {lr, momentum, weight_decay, grad_scale} read from four floats in device memory when the kernel runs: a launch
 * captured in a hipGraph follows the per-epoch LR schedule (train_or_resume.py:109-113, 349) without being re-captured */
int dsrl_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, const float* hyper /*device, 4 floats*/, dsrl_stream_t stream);
/* the same update driven by a device table of nseg rows {first float, floats, address of an amax record or 0} (int64 each) that covers the arena with segments of
 * whole float4 (first float a multiple of 4, count a multiple of 4, each segment inside ONE parameter; one block per segment, <= 32768 floats recommended): for
 * rows with a record the launch also leaves max |p| of the UPDATED values there (same bit patterns as dsrl_conv2d_filters_amax_batched; the records must be zero
 * when the launch starts) - the conv filters' operand magnitudes for the next step come out of the optimiser pass instead of a sweep of their own */
int dsrl_sgd_step_dev_segments(float* p, const float* g, float* buf, const int64_t* table, int64_t nseg, const float* hyper /*device, 4 floats*/, dsrl_stream_t stream);
/* Exponential moving average of the weights, e <- e + (1 - d_t) (p_new - e) with p_new the parameter the SGD update has just computed.
 * ema_record: 16 bytes of device memory, 16-byte aligned: {float omd = 1 - d_t of the update about to run, float decay_max, uint32 updates,
 * uint32 warmup}.  The element kernels only read omd; dsrl_ema_advance, once per step behind the last of them, does updates += 1 and writes the next
 * omd: d_t = warmup ? min(decay_max, (1 + t) / (10 + t)) : decay_max with t = updates, in fp32 with a correctly rounded division.  No host write per
 * step: a captured step advances the schedule on every replay.
 * The three dsrl_sgd_step*_ema take the arguments of their twins plus the average's arena `ema` (laid out as p, 16-byte aligned) and the record;
 * p and buf come out bit-identical to the twin's, the amax records of the segment form are published from p_new as before, and ema is bit-identical
 * to the twin followed by dsrl_ema_update(ema, p, n, ...). */
int dsrl_sgd_step_ema(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay, float grad_scale,
                      float* ema, const void* ema_record, dsrl_stream_t stream);
int dsrl_sgd_step_dev_ema(float* p, const float* g, float* buf, int64_t n, const float* hyper /*device, 4 floats*/, float* ema, const void* ema_record,
                          dsrl_stream_t stream);
int dsrl_sgd_step_dev_segments_ema(float* p, const float* g, float* buf, const int64_t* table, int64_t nseg, const float* hyper /*device, 4 floats*/,
                                   float* ema, const void* ema_record, dsrl_stream_t stream);
/* the unfused update: ema[i] <- ema[i] + omd (p[i] - ema[i]) for i < n (the BatchNorm buffer arena after the step); both 16-byte aligned */
int dsrl_ema_update(float* ema, const float* p, int64_t n, const void* ema_record, dsrl_stream_t stream);
int dsrl_ema_advance(void* ema_record, dsrl_stream_t stream);
/* exchanges n floats of two disjoint 16-byte aligned arenas in place, as bit patterns (NaN payloads, infinities, -0 and denormals survive) */
int dsrl_arena_swap(float* a, float* b, int64_t n, dsrl_stream_t stream);
/* Gradient-norm clipping on the gradient arena: torch.nn.utils.clip_grad_norm_(parameters, max_norm) with the coefficient folded into the
 * optimiser's grad_scale, everything on the device.
 * dsrl_grad_sumsq: one pass over g[first, first + n) of the arena `g`.  The arena is cut into tiles of 1024 floats anchored at g[0];
 * tiles[first / 1024 + k] receives the sum of squares of tile k of the range, in double (a float square is exact there), in an order fixed inside
 * the tile.  first must be a multiple of 1024 and g 16-byte aligned (DSRL_E_BADARG otherwise, nothing is written); the last tile of a range may be
 * short.  No atomics and no zero fill: only the tiles of the range are written, each once, and they do not depend on how the arena is cut into calls.
 * dsrl_grad_clip_workspace_bytes(n): the bytes of the tile array of an n-float arena plus the scratch the finish keeps BEHIND it.
 * dsrl_grad_clip_finish: `tiles` is the start of such a workspace and ntiles = ceil(n / 1024).  S = the sum of the tiles in a fixed order (two
 * launches).  {lr, momentum, weight_decay, gs} come from the four device floats `hyper_in`, or from the host arguments when hyper_in is null.  In double:
 * norm = gs sqrt(S), coef = min(1, max_norm / (norm + 1e-6)) - torch's formula; a NaN norm gives a NaN coefficient, an infinite one 0.
 * hyper_out (device, 4 floats, may not alias hyper_in) = {lr, momentum, weight_decay, (float)(gs coef)}, bit-equal to gs when coef == 1: the
 * `hyper` of the dsrl_sgd_step_dev* launches that follow.
 * record: 64 bytes of device memory, 16-byte aligned: {double sumsq, double norm_sum, float norm, float coef, float max_norm, float norm_max,
 * uint32 steps, uint32 clipped, uint32 nonfinite, 20 bytes of padding}.  max_norm is READ when the finish runs (+inf: monitor only), so a captured
 * step follows a new threshold without being re-captured; sumsq, norm and coef are those of this call; steps += 1; a finite norm is added to
 * norm_sum, raises norm_max and counts in `clipped` when coef < 1; a NaN or infinite norm counts in `nonfinite` alone. */
int dsrl_grad_sumsq(const float* g, int64_t first, int64_t n, double* tiles, dsrl_stream_t stream);
size_t dsrl_grad_clip_workspace_bytes(int64_t n);
int dsrl_grad_clip_finish(const double* tiles, int64_t ntiles, const float* hyper_in /*device, 4 floats, or null*/, float lr, float momentum,
                          float weight_decay, float grad_scale, void* record, float* hyper_out /*device, 4 floats*/, dsrl_stream_t stream);
/* torch.optim.AdamW(lr, betas, eps, weight_decay) - one parameter group, decoupled decay, no amsgrad, no maximize - on the flat arenas p, g, m
 * (exp_avg), v (exp_avg_sq), all 16-byte aligned.  Per element, in fp32, with gh = g * grad_scale (scaled before the moments: eps makes the update
 * depend on the gradient's scale):
 *     p <- p (1 - lr wd);  m <- m + (1 - b1)(gh - m);  v <- b2 v + (1 - b2) gh gh;  p <- p - ss m / (sqrt(v) isq + eps)
 *     ss = lr / (1 - b1^t), isq = 1 / sqrt(1 - b2^t); square root and division correctly rounded.
 * record: 64 bytes of device memory, 16-byte aligned: {float beta1, float beta2, float eps, float ss_factor = 1 / (1 - b1^t), float isq,
 * float (1 - beta1), float (1 - beta2) (of the double betas), 4 bytes of padding, int64 t, double beta1, double beta2, 8 bytes of padding}.  The host
 * writes the betas and eps once; t and the two factors are written by dsrl_adamw_advance (t += 1; once per optimiser pass, BEFORE its launches: a
 * fresh record holds t = 0, the first pass runs with t = 1) and dsrl_adamw_set_step (a resume), both of which form the factors in double from t
 * itself - the same bits whichever way t was reached - and never by the host.  The element launches only read the record.
 * The entry points mirror dsrl_sgd_step*: host hyper-parameters; `hyper` = the 4 device floats {lr, unused, weight_decay, grad_scale} the SGD
 * launches read (slot 1, SGD's momentum, is ignored: dsrl_grad_clip_finish serves both optimisers); the segment table of
 * dsrl_sgd_step_dev_segments, with max |p_new| published to the rows' amax records in the same way.  The _ema forms add the average's arena and the
 * EMA record and update the average from the p they have just computed.  All six give the same bits in p, m and v. */
int dsrl_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float weight_decay, float grad_scale, const void* record,
                    dsrl_stream_t stream);
int dsrl_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper /*device, 4 floats*/, const void* record,
                        dsrl_stream_t stream);
int dsrl_adamw_step_dev_segments(float* p, const float* g, float* m, float* v, const int64_t* table, int64_t nseg, const float* hyper /*device, 4 floats*/,
                                 const void* record, dsrl_stream_t stream);
int dsrl_adamw_step_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, float weight_decay, float grad_scale, const void* record,
                        float* ema, const void* ema_record, dsrl_stream_t stream);
int dsrl_adamw_step_dev_ema(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper /*device, 4 floats*/, const void* record,
                            float* ema, const void* ema_record, dsrl_stream_t stream);
int dsrl_adamw_step_dev_segments_ema(float* p, const float* g, float* m, float* v, const int64_t* table, int64_t nseg,
                                     const float* hyper /*device, 4 floats*/, const void* record, float* ema, const void* ema_record, dsrl_stream_t stream);
int dsrl_adamw_advance(void* record, dsrl_stream_t stream);
int dsrl_adamw_set_step(void* record, int64_t t, dsrl_stream_t stream);
/* flag[0] |= 1 if any element is NaN (the reference's per-output NaN asserts folded into one readback) */
int dsrl_nan_check(const float* x, int64_t n, int* flag, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * in-library launch timing (bench.py roofline): dsrl_prof_enable(n) brackets every n-th MFMA conv launch (n = 1: all of them,
 * 0: off) with HIP events on its own stream - an event pair costs ~3 us of device time, so a timed region samples. dsrl_prof_read() synchronises those events and reports per kernel family the launch count,
 * summed milliseconds and summed in-bounds FLOPs. family = 3 * arithmetic + pass, arithmetic 0 fp32 / 1 bf16x3 / 2 bf16x6
 * (see dsrl_conv_precision), pass 0 forward / 1 wgrad / 2 dgrad; dsrl_prof_kernel_name() names the kernel of a family.
 * ---------------------------------------------------------------------------------------------- */
int dsrl_prof_enable(int on);
int dsrl_prof_read(int family, int64_t* launches, double* total_ms, double* total_flops);
/* summed ALGORITHMIC bytes of the recorded launches of a family: every operand (input, filter, output) of the conv once, fp32 */
int dsrl_prof_read_bytes(int family, double* total_bytes);
const char* dsrl_prof_kernel_name(int family);

/* ------------------------------------------------------------------------------------------------
 * inference: the eval-mode SSSR tail (DSRL.py:53-69 after the bilinear x2) as one launch that ends in class indices (csrc/predict.hip)
 *   x (N,H,W,Cin) pixel-major with pixel stride ldx -> ConvTranspose2d k2 s2 w1 (Cin,Cmid,2,2), no bias -> fmaf(v, gamma * invstd, beta - mean * gamma * invstd)
 *   (the arithmetic of bn_apply) -> ReLU -> ConvTranspose2d k2 s2 w2 (Cmid,Cout,2,2) + bias2 -> pred (N,4H,4W) = lowest index among the maximal logits.
 *   fp32 products and accumulation whatever the conv precision mode says; neither the mid activations nor the logits are written to memory.
 *   target (N,4H,4W) given: counts[3*Cout+2] (nullable) gets what a seg_metrics call on the same predictions would ADD (pixels whose target is
 *   ignore_index or >= Cout excluded; one 64-bit atomic per block and counter), ce_out[2] (nullable) = mean nn.CrossEntropyLoss(ignore_index)
 *   of the logits and the number of counted pixels, reduced through per-block partials in ws in a fixed order (bit-identical run to run).
 *   nan_flag (nullable): |= 1 for a NaN logit or a NaN in front of the ReLU (which maps it to 0, as bn_apply does), |= 2 for a label outside [0,Cout) that is not ignore_index (which also makes ce_out NaN).
 *   pred is written for every pixel.  pred, target and x must be 4-byte aligned; ws 8-byte aligned (only read when ce_out is given).
 * _supported: 1 for Cin = Cmid = Cout = 19 and any N, H, W >= 1 with N*H*W*16 <= 2^31 - 1 (output pixels are indexed in 32 bits per image batch),
 *   0 otherwise; pure host code.  _workspace_bytes depends on the shape only and holds for every launch of that shape.
 * ---------------------------------------------------------------------------------------------- */
int dsrl_sssr_tail_predict_supported(int N, int H, int W, int Cin, int Cmid, int Cout);
size_t dsrl_sssr_tail_predict_workspace_bytes(int N, int H, int W);
int dsrl_sssr_tail_predict(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                           const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                           uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                           float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* Horizontal-flip ensemble of the same tail in the same single launch.  x holds 2 N images: image n is the plain view, image N + n the tail input
 * computed from the MIRRORED image n, still in the mirrored frame (the kernel un-mirrors it).  With La the logits of the plain view and Lb those of
 * the mirrored view mirrored back along W: E = logaddexp(log_softmax(La), log_softmax(Lb)) - ln 2 over the classes; pred (N,4H,4W) = lowest index
 * among the maxima of softmax(La) + softmax(Lb); ce_out = mean of -E[target] over the counted pixels, evaluated in log space; counts, nan_flag
 * (bit 0: a NaN in either view), target, ws and the alignment rules as above.  N is the number of class maps: _supported(N, ...) and
 * _workspace_bytes(N, H, W) answer for this launch too. */
int dsrl_sssr_tail_predict_flip(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                                uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                                float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
/* The two launches above with the confusion matrix of the class map they write (the ensemble's with _flip) against target: cm[t*Cout + p] as
 * dsrl_seg_metrics_cm defines it, ADDED (an LDS matrix per block, one 64-bit atomic per block and non-zero bin).  cm needs a target and neither counts
 * nor ce_out; with cm null these are dsrl_sssr_tail_predict / _flip themselves.  pred, counts and ce_out are bit-identical to those of the plain entry points. */
int dsrl_sssr_tail_predict_cm(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                              const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                              uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                              float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                              unsigned long long* cm /*nullable, [Cout*Cout]*/, dsrl_stream_t stream);
int dsrl_sssr_tail_predict_flip_cm(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                   const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                                   uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                                   float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                                   unsigned long long* cm /*nullable, [Cout*Cout]*/, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * inference: the multi-scale ensemble (csrc/merge.hip) - what follows the eval-mode forward path once it has written a view's logits
 *   A view v is the logits (N,Hs,Ws,C) of one scale, pixel-major with pixel stride ld >= C, in the plain or (mirror != 0) the horizontally mirrored
 *   frame; views may differ in Hs, Ws, ld and mirror.  The output grid is (Ho,Wo), the grid of pred and target.
 *   Resampling: align-corners bilinear interpolation OF THE LOGITS, a mirrored view mirrored back along W first.  The source coordinate of output
 *   index o on an axis with S source and O output samples is exact: n = o (S - 1), i0 = n / (O - 1), frac = float(n mod (O - 1)) / float(O - 1),
 *   i1 = min(i0 + 1, S - 1); O = 1: i0 = 0, frac = 0 (32-bit integers, one division per axis: the weight carries one rounding at every size, where
 *   dsrl_bilinear_ac_fwd's fp32 scale * dst loses accuracy with the coordinate).
 *   Result over V views: P = (1 / V) sum_v softmax_c(resampled L_v); pred = lowest index among the maxima of sum_v softmax; ce_out[0] = mean of
 *   -log P[target] over the counted pixels (target != ignore_index), ce_out[1] their number; counts = the dsrl_seg_metrics table of pred, ADDED;
 *   cm[t*C + p] ADDED under the one convention above; nan_flag |= 1 for a NaN among the sampled logits of ANY view (it travels through the
 *   accumulator to the last launch), |= 2 for a label >= C that is not ignore_index (which also makes ce_out NaN).  Every pixel ignored: ce_out[0] NaN.
 *   fp32 limit of ce: it is taken from the accumulated probabilities.  Where the target's probability underflows fp32 in every view (a logit gap above
 *   about 87) the value is what fp32 gives, +inf; a gap of 60 is still right to an ulp of the logarithm.
 *   dsrl_prob_merge: one view that is not the last.  first != 0 stores softmax into acc without reading it, otherwise it adds.
 *   dsrl_prob_merge_finish: the last view: the same resample and softmax plus what acc holds, in registers - acc is never written by this launch and
 *   is null exactly when views == 1 - then arg-max, counters, loss, NaN flag and confusion matrix.  views = V.  counts, ce_out and cm need a target.
 *   A view contributes the same bits whichever launch merges it.  Every output is bit-identical run to run: accumulator pixels are owned by one
 *   thread, counters and bins are 64-bit integer atomics (one per block and non-zero bin), the loss goes through per-block partials in ws reduced in
 *   a fixed order.  acc is the kernels' own tensor (class-planar) of dsrl_prob_merge_acc_bytes(N, Ho, Wo, C) bytes: callers allocate it and never
 *   interpret it.  logits and acc 4-byte aligned, ws 8-byte aligned (only used with ce_out); pred and target may start at any byte, Wo may be odd.
 * _supported: 1 for 1 <= C <= 32 (and C <= dsrl_confusion_matrix_max_classes()), every dimension >= 1 and every 32-bit index in range
 *   (N*Ho*Wo*C, N*Hs*Ws*C, o*(S-1) <= 2^31 - 1; a launch checks N*Hs*Ws*ld itself), 0 otherwise; pure host code.  _workspace_bytes and _acc_bytes
 *   depend on the shape only and hold for every launch of that shape.
 * ---------------------------------------------------------------------------------------------- */
int dsrl_prob_merge_supported(int N, int Hs, int Ws, int Ho, int Wo, int C);
size_t dsrl_prob_merge_acc_bytes(int N, int Ho, int Wo, int C);
size_t dsrl_prob_merge_workspace_bytes(int N, int Ho, int Wo);
int dsrl_prob_merge(const float* logits, int ld, int N, int Hs, int Ws, int C, int mirror, float* acc, int Ho, int Wo, int first, dsrl_stream_t stream);
int dsrl_prob_merge_finish(const float* logits, int ld, int N, int Hs, int Ws, int C, int mirror, const float* acc /*nullable: the only view*/, int Ho,
                           int Wo, int views, uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index,
                           unsigned long long* counts /*nullable*/, float* ce_out /*nullable, [2]: mean, counted pixels*/, int* nan_flag /*nullable*/,
                           void* ws, size_t ws_bytes, unsigned long long* cm /*nullable, [C*C]*/, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * inference: the sliding-window ensemble (csrc/window.hip) - "slide" evaluation: the image in overlapping windows of the training size
 *   Plan (pure host code, functional.window_plan).  Along an axis of S input pixels with window side w and stride s (1 <= s <= w <= S) the positions
 *   are n = max(S - w + s - 1, 0) / s + 1 and a_i = max(min(i s + w, S) - w, 0): the last window is pulled back to end at S, positions are strictly
 *   increasing.  The 2-D plan is the product ys x xs, visited row-major.  On the model path H, W, h, w are multiples of 16, 16 <= h <= H,
 *   16 <= w <= W, and there are at most 32 positions per axis.
 *   Ensemble.  A window's crop goes through the eval forward path (with flip the crop and its mirror image in one batch); its SSSR logits
 *   (N,C,2h,2w) sit at (2 y0, 2 x0) on the (2H,2W) grid.  On the grid (Ho,Wo): tot = sum over the views covering a pixel of softmax_c(logits), a
 *   mirrored view mirrored back along W first; cnt = (y-positions covering the row) x (x-positions covering the column) x views_per_position;
 *   P = tot / cnt; pred = lowest index among the maxima of tot; ce_out[0] = mean of -log P[target] over the counted pixels (target !=
 *   ignore_index), ce_out[1] their number; confidence = min(1, tot[pred] / cnt); counts, cm, cal, conf and nan_flag exactly as
 *   dsrl_prob_merge_finish_ex defines them for its ensemble (bit 0: a NaN logit in ANY covering view, bit 1: a label >= C that is not ignore_index,
 *   which also makes ce_out NaN).  Class PROBABILITIES are averaged, as in the flip and multi-scale modes; mmseg's slide mode averages logits.
 *   The softmax is the function of the multi-scale ensemble (csrc/merge_common.h): one whole-image window gives the bits of one identity view of
 *   dsrl_prob_merge_finish.
 * dsrl_window_merge: one view of one position.  logits (N,hw,ww,C) pixel-major with pixel stride ld >= C, in the plain or (mirror != 0) the mirrored
 *   frame; the window's pixel (wy, wx) is pixel (oy + wy, ox + wx) of acc (class-planar, dsrl_prob_merge_acc_bytes(N, Ho, Wo, C) bytes, the
 *   kernels' own).  It is STORED without reading acc iff wy >= fresh_y && wx >= fresh_x, otherwise ADDED: acc needs no fill.  With the positions
 *   visited row-major a pixel of window (i, j) has been covered before iff it lies above grid row ys[i-1] + hw or left of grid column xs[j-1] + ww,
 *   so the first view of position (i, j) takes fresh_y = i ? ys[i-1] + hw - ys[i] : 0, fresh_x likewise, and a view that is never the first one of
 *   its pixels (the mirrored one) fresh_y = hw.  0 <= fresh_y <= hw, 0 <= fresh_x <= ww; the window must lie inside the grid (DSRL_E_BADARG).
 *   functional.WindowMerge owns the order and the offsets: callers hand it logits only.
 * dsrl_window_merge_finish(_ex): one pass over acc after the last view.  ys / xs: HOST arrays of ny / nx grid offsets (at most 32 each), copied into
 *   the launch's arguments - no device table, no copy, capturable.  DSRL_E_BADARG unless each axis starts at 0, increases strictly, leaves no gap
 *   (a_i <= a_{i-1} + side) and ends at the grid's end.  counts, ce_out, cm and cal need a target; _ex adds cal (the record, [3 * bins]) and conf
 *   (the confidence map (N,Ho,Wo)), both nullable.  Every output is bit-identical run to run: integer atomics for the counters, per-block loss
 *   partials in ws reduced in block order, no float atomics.  acc and conf 4-byte, ws and cal 8-byte aligned; pred and target any byte, any Wo.
 * _supported: 1 for 1 <= C <= 32 (and C <= dsrl_confusion_matrix_max_classes()), hw <= Ho, ww <= Wo and every 32-bit index in range
 *   (N*Ho*Wo*C, N*hw*ww*C <= 2^31 - 1; a launch checks N*hw*ww*ld itself), 0 otherwise; pure host code.  _workspace_bytes depends on the shape only.
 * ---------------------------------------------------------------------------------------------- */
int dsrl_window_merge_supported(int N, int hw, int ww, int Ho, int Wo, int C);
size_t dsrl_window_merge_workspace_bytes(int N, int Ho, int Wo);
int dsrl_window_merge(const float* logits, int ld, int N, int hw, int ww, int C, int mirror, float* acc, int Ho, int Wo, int oy, int ox, int fresh_y,
                      int fresh_x, dsrl_stream_t stream);
int dsrl_window_merge_finish(const float* acc, int N, int C, int Ho, int Wo, const int* ys /*host, ny*/, int ny, const int* xs /*host, nx*/, int nx, int hw,
                             int ww, int views_per_position, uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index,
                             unsigned long long* counts /*nullable*/, float* ce_out /*nullable, [2]: mean, counted pixels*/, int* nan_flag /*nullable*/,
                             void* ws, size_t ws_bytes, unsigned long long* cm /*nullable, [C*C]*/, dsrl_stream_t stream);
int dsrl_window_merge_finish_ex(const float* acc, int N, int C, int Ho, int Wo, const int* ys /*host, ny*/, int ny, const int* xs /*host, nx*/, int nx,
                                int hw, int ww, int views_per_position, uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index,
                                unsigned long long* counts /*nullable*/, float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                                unsigned long long* cm /*nullable, [C*C]*/, unsigned long long* cal /*nullable, [3*bins]*/, int bins,
                                float* conf /*nullable, (N,Ho,Wo)*/, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * calibration: the reliability record and the confidence map (csrc/calibration.hip; the arithmetic is written once in csrc/common.h)
 *   Confidence of a pixel: the probability of the class the producer reports (first maximum), fp32, from values it already has -
 *     from logits and the single-view tail: 1 / sum_c exp(v_c - max) (the sum the cross entropy forms, c ascending);
 *     the flip tail: the winning entry of (ea_c / sa + eb_c / sb) / 2;   the multi-scale finish: min(1, winning sum / views).
 *   Bin: B equal-width bins, 1 <= B <= dsrl_calibration_max_bins() = 64; b = min(B - 1, (int)(conf * (float)B)), one fp32 multiply.
 *   Record: int64 [3 B] = [n_b | hit_b | q_b], ADDED: counted pixels of bin b (target != ignore_index and target < C: the pixels of the confusion
 *   matrix), those with pred == target, and sum rintf(conf * 2^24) as an integer.  A pixel whose confidence is NaN is counted nowhere (it raises
 *   bit 0 of nan_flag).  Integers only: per-block LDS counters (q in 64 bits), one 64-bit atomic per block and non-zero entry - a record is
 *   bit-identical run to run and, up to the summation of records, for an image alone or in a batch.
 *   Figures (host, float64): acc_b = hit_b / n_b, conf_b = q_b / (2^24 n_b), ECE = sum_b (n_b / N) |acc_b - conf_b|, MCE = the maximum over
 *   the non-empty bins.
 * dsrl_calibration_from_logits: logits (P, C) pixel-major with pixel stride ld, C <= 60 (the addressing of dsrl_seg_metrics), one streaming
 *   launch.  record (nullable, needs target) and conf_map (nullable, P floats, written for every pixel) - at least one; nan_flag (nullable):
 *   |= 1 for a NaN logit, |= 2 for a label >= C that is not ignore_index (record only).  logits and conf_map 4-byte, record 8-byte aligned.
 * dsrl_sssr_tail_predict_ex / _flip_ex / dsrl_prob_merge_finish_ex: the launches of dsrl_sssr_tail_predict_cm / _flip_cm /
 *   dsrl_prob_merge_finish with every optional output: cm, cal (the record, [3 * bins]; needs a target) and conf (the confidence map, the shape
 *   of pred, fp32; needs no target; 16-byte aligned for the tails, 4-byte for the finish) are nullable.  With cal and conf null they ARE those
 *   launches; with them pred, counts, ce_out, cm and nan_flag are bit-identical to theirs.  In the tails a NaN in front of the ReLU (which hides
 *   it from the logits) makes the confidence of the input pixel's 4x4 patch NaN.
 * ---------------------------------------------------------------------------------------------- */
int dsrl_calibration_max_bins(void);
int dsrl_calibration_from_logits(const float* logits, int ld, const uint8_t* target /*nullable*/, int64_t P, int C, int ignore_index, int bins,
                                 unsigned long long* record /*nullable, [3*bins]*/, float* conf_map /*nullable, [P]*/, int* nan_flag /*nullable*/,
                                 dsrl_stream_t stream);
int dsrl_sssr_tail_predict_ex(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                              const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                              uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                              float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                              unsigned long long* cm /*nullable, [Cout*Cout]*/, unsigned long long* cal /*nullable, [3*bins]*/, int bins,
                              float* conf /*nullable, (N,4H,4W)*/, dsrl_stream_t stream);
int dsrl_sssr_tail_predict_flip_ex(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                   const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                                   uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                                   float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                                   unsigned long long* cm /*nullable, [Cout*Cout]*/, unsigned long long* cal /*nullable, [3*bins]*/, int bins,
                                   float* conf /*nullable, (N,4H,4W)*/, dsrl_stream_t stream);
int dsrl_prob_merge_finish_ex(const float* logits, int ld, int N, int Hs, int Ws, int C, int mirror, const float* acc /*nullable: the only view*/, int Ho,
                              int Wo, int views, uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index,
                              unsigned long long* counts /*nullable*/, float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                              unsigned long long* cm /*nullable, [C*C]*/, unsigned long long* cal /*nullable, [3*bins]*/, int bins,
                              float* conf /*nullable, (N,Ho,Wo)*/, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * temperature: post-hoc temperature scaling (Guo et al. 2017) - fit one scalar T on a held-out split, report softmax(v / T)
 * (csrc/temperature.hip; the arithmetic is written once in csrc/common.h: temperature_terms, temperature_scale).  beta = 1 / T.
 *   The fit.  A live pixel is one whose label t is neither ignore_index nor >= C.  For its logits v_0..v_{C-1}: m = the fmaxf chain from v_0,
 *   d_c = v_c - m <= 0, and for each beta_k of the call, in fp32 with c ascending:
 *     e_c = exp(beta_k d_c), s = sum e_c, a = sum e_c d_c, q = sum (e_c d_c) d_c,
 *     L = log(s) - beta_k d_t  (the NLL of softmax(beta_k v) at t; the log is a float32 polynomial without the device logf's half-ulp bias),  mu = a / s,  G = mu - d_t = dL/dbeta,  H = q / s - mu mu = d2L/dbeta2 >= 0.
 *   Record: float64 [1 + 3 K], ADDED by every call: [0] the number of live pixels, then for each k the sums of L, G and H over the live pixels.
 *   L is convex in beta, so the root of sum G is the fitted 1 / T; G and H at K points give it by Hermite interpolation (functional.temperature_solve).
 * dsrl_temperature_stats: logits (P, C) pixel-major with pixel stride ld >= C, C <= 60; betas: DEVICE array of K floats, 1 <= K <=
 *   dsrl_temperature_max_points() = 16.  One streaming launch (256 pixels x C floats per tile through LDS, one thread per pixel, per-block partial
 *   sums in double) and a one-block finish that adds the partials in a fixed order and then adds the totals to record: no float atomics, the
 *   pixel -> block mapping depends on P alone, so a record has the same bits on every call.  ws: >= dsrl_temperature_workspace_bytes(P, K) (a
 *   function of P and K alone; 0, with a message, for bad arguments), 8-byte aligned.  nan_flag (nullable): |= 1 for a NaN logit of a live pixel
 *   (its NaN reaches the sums), |= 2 for a label >= C that is not ignore_index (not counted).  A beta that is not a finite number > 0 makes its own
 *   three entries NaN and leaves the others right.  logits / betas 4-byte, record 8-byte aligned.  No host reads; capturable.
 *   Argument errors, before any launch and with nothing written: null pointers, P <= 0, K outside 1..16, ld < C, a misaligned pointer
 *   (DSRL_E_BADARG); C > 60, or P / ld beyond the 32-bit tile indices (DSRL_E_UNSUPPORTED); a workspace too small or misaligned (DSRL_E_WORKSPACE).
 *   Applying a temperature: every producer, behind its arg-max, replaces each logit by v_c * beta (one fp32 multiply) and runs the softmax
 *   arithmetic it has on the result.  A positive beta is monotone under rounding: the class map and the counters of a single view are
 *   bit-identical with and without a temperature, and dsrl_calibration_from_logits_t reproduces the fused tail's confidence exactly.
 * dsrl_sssr_tail_predict_t / _flip_t: dsrl_sssr_tail_predict_ex / _flip_ex plus beta (a finite number > 0, DSRL_E_BADARG otherwise): ce_out, cal and
 *   conf are those of the scaled model; in the flip form each view is scaled in front of its softmax.
 * dsrl_calibration_from_logits_t: dsrl_calibration_from_logits plus beta.
 * ---------------------------------------------------------------------------------------------- */
int dsrl_temperature_max_points(void);
size_t dsrl_temperature_workspace_bytes(int64_t P, int K);
int dsrl_temperature_stats(const float* logits, int ld, const uint8_t* target, int64_t P, int C, int ignore_index, const float* betas /*device, K floats*/,
                           int K, double* record /*[1 + 3K], accumulated*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);
int dsrl_sssr_tail_predict_t(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                             const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                             uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                             float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                             unsigned long long* cm /*nullable, [Cout*Cout]*/, unsigned long long* cal /*nullable, [3*bins]*/, int bins,
                             float* conf /*nullable, (N,4H,4W)*/, float beta, dsrl_stream_t stream);
int dsrl_sssr_tail_predict_flip_t(const float* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout, const float* w1, const float* bn_mean,
                                  const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* w2, const float* bias2 /*nullable*/,
                                  uint8_t* pred, const uint8_t* target /*nullable*/, int ignore_index, unsigned long long* counts /*nullable*/,
                                  float* ce_out /*nullable*/, int* nan_flag /*nullable*/, void* ws, size_t ws_bytes,
                                  unsigned long long* cm /*nullable, [Cout*Cout]*/, unsigned long long* cal /*nullable, [3*bins]*/, int bins,
                                  float* conf /*nullable, (N,4H,4W)*/, float beta, dsrl_stream_t stream);
int dsrl_calibration_from_logits_t(const float* logits, int ld, const uint8_t* target /*nullable*/, int64_t P, int C, int ignore_index, int bins,
                                   unsigned long long* record /*nullable, [3*bins]*/, float* conf_map /*nullable, [P]*/, int* nan_flag /*nullable*/,
                                   float beta, dsrl_stream_t stream);

/* Fingerprint of tensors that must not change while an inference.FrozenOperands holds operands derived from them (a write through `.data` or a
 * raw pointer moves neither a tensor's address nor its version counter).  table: DEVICE array of nseg rows of 2 int64 {pointer (4-byte aligned),
 * number of 32-bit words <= dsrl_fingerprint_segment_words()}, one block per row; a tensor is cut into as many rows as it needs.  Row r gets
 * h = sum_i (word_i + 1) * K * (2 i + 1) modulo 2^64: any change of a single word changes h, and the value does not depend on the order of the
 * additions (bit-identical run to run).  out (nullable, nseg words): receives h; expect (nullable, nseg words) with flag: *flag |= bit when a row's h
 * differs from expect[r].  One launch; nothing is read back here. */
int dsrl_fingerprint_segment_words(void);
int dsrl_fingerprint_segments(const int64_t* table, int64_t nseg, uint64_t* out /*nullable*/, const uint64_t* expect /*nullable*/, int* flag /*nullable*/,
                              int bit, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * inference: the panel of the test command (utils.make_input_output_visualization) on the device (csrc/visualize.hip)
 *   rgb (N,H,W,3) uint8 pixel-major = the shown input, classes (N,H,W) uint8 = a class map (DSRL.predict's pred), mask (N,H,W) uint8, nullable: where
 *   mask == ignore_index the class is replaced by ignore_index (test.py's dataset mode: pred_map[target == IGNORE] = IGNORE), palette uint8 [256][3]
 *   in device memory: label -> colour (labels the palette does not name: black) -> out (N,H,3W,3) uint8 = input | class colours | overlay,
 *   overlay = uint8(min((1 - blend_factor) * in + blend_factor * colour, 255)) evaluated in double with both products and the sum rounded separately
 *   and the conversion truncating: byte for byte what numpy gives for that expression in float64, for all 65536 (input byte, colour byte) pairs.
 *   One streaming launch: a thread owns 16 (W % 16 == 0, pointers 16-byte aligned) or 4 (W % 4 == 0, 4-byte aligned) pixels of one row and moves them
 *   as 128- or 32-bit words, else one pixel with byte accesses; 32-bit indices (N*H*W*9 < 2^31, DSRL_E_UNSUPPORTED beyond), one division per thread.
 *   0 < blend_factor < 1, 0 <= ignore_index <= 255.  out must not alias the inputs.
 * ---------------------------------------------------------------------------------------------- */
int dsrl_class_map_visualize(const uint8_t* rgb, const uint8_t* classes, const uint8_t* mask /*nullable*/, const uint8_t* palette /*device, 256 x 3*/,
                             uint8_t* out, int N, int H, int W, int ignore_index, double blend_factor, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * quality of the super-resolved image: squared error and SSIM of pred against ref, per image (csrc/sr_quality.hip)
 *   pred, ref: fp32 (N,H,W,C) pixel-major with pixel strides ld_pred, ld_ref >= C (4-byte aligned; 16-byte aligned rows are loaded as float4),
 *   1 <= C <= 4, H >= 11 and W >= 11 (DSRL_E_BADARG otherwise).  mean, std: C HOST floats (finite, std != 0), passed on as kernel arguments.
 *   Every value is de-normalised as v = x * std[c] + mean[c] (a product, then a sum: two roundings) and clamped to [0, 1] by comparisons that a NaN
 *   fails, so a NaN stays one; mean = 0, std = 1 is "already in [0, 1]".
 *   sse      = sum over the image's C*H*W values of (vp - vr)^2; difference and square fp32, the sum double.
 *   SSIM     = the single-scale index of Wang et al. at data range 1: window g[k] = exp(-(k-5)^2 / 4.5), k = 0..10, normalised in double and rounded
 *              to fp32; applied separably (rows, then columns, taps ascending, fp32 fused multiply-adds) to x, y, x*x, x*y, y*y (single fp32
 *              products) over the valid region (H-10) x (W-10) of each channel; per pixel ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)
 *              (sxx + syy + C2)) with sab = E[ab] - ma mb, C1 = 1e-4f, C2 = 9e-4f, a correctly rounded division: bit-equal pred and ref give exactly 1.
 *   ssim_sum = sum of that map over channels and valid pixels, in double.
 *   records (N x {sse, ssim_sum}, float64, 8-byte aligned) is WRITTEN.  ssim_map (nullable; fp32, planar (N, C, H-10, W-10)) receives the map.
 *   Two launches, no allocation, no host synchronisation, no atomics: every block writes its two double partials to its own slot of ws and the second
 *   launch adds an image's slots in a fixed order.  The tiling of an image does not depend on N or on the image's place in the batch: results are
 *   bit-identical run to run, and an image's record is the same alone or inside a batch.  ws 8-byte aligned, ws_bytes >= the query
 *   (DSRL_E_WORKSPACE otherwise); the query depends on the shape only and holds for every launch of that shape (0 for a shape the launch refuses).
 *   32-bit element indices: N * H * W * max(ld_pred, ld_ref) < 2^31 and N <= 65535, DSRL_E_UNSUPPORTED beyond.
 * ---------------------------------------------------------------------------------------------- */
size_t dsrl_sr_quality_workspace_bytes(int N, int C, int H, int W);
int dsrl_sr_quality(const float* pred, int ld_pred, const float* ref, int ld_ref, int N, int C, int H, int W, const float* mean /*host, C*/,
                    const float* std /*host, C*/, double* records /*N x 2*/, float* ssim_map /*nullable*/, void* ws, size_t ws_bytes, dsrl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Boundary IoU (Cheng et al., CVPR 2021) of two class maps: the counters of the IoU restricted to the pixels within distance d of a class outline
 * (csrc/boundary.hip).  pred, target: uint8 (N,H,W); either may start at any byte and W may be anything (byte loads).
 *   1. g' = target where target < C and target != ignore_index, else 255 (void).  p' = 255 where g' == 255, else pred where pred < C, else 254 (bad);
 *      a bad pixel raises bit 1 (|= 2) of nan_flag (nullable), as in dsrl_confusion_matrix.
 *   2. A pixel is in the band of a map iff the (2d+1) x (2d+1) window centred on it leaves the image or holds a byte other than its own; windows do
 *      not reach into the batch's next image.  gb: the band of g', pb: the band of p'.  For every class at once this is the paper's
 *      mask - erode(mask, 3x3, d iterations) on a mask padded by a ring of zeros.
 *   3. Over the pixels with g' != 255: G[c] += gb && g' == c;  P[c] += pb && p' == c (p' < C only);  I[c] += gb && pb && g' == c && p' == c.
 *   counts = [I | G | P], 3*C 64-bit counters, ADDED to (8-byte aligned); Boundary IoU of class c = I / (G + P - I).
 *   band (nullable, N*H*W bytes) is WRITTEN: bit 0 gb, bit 1 pb, 0 on void pixels.
 *   Two launches (a row pass that leaves one byte per pixel and map in ws - the label where the row window is uniform and inside the image, 253
 *   otherwise - and a column pass that tests those bytes and counts), O(1) work per pixel and pass whatever d; integer arithmetic, per-block LDS bins
 *   flushed as 64-bit atomics: exact, order independent, identical run to run, and an image counts the same alone or inside a batch.  No allocation
 *   and no host synchronisation.
 *   1 <= C <= dsrl_boundary_counts_max_classes() = 253 and 1 <= d <= dsrl_boundary_counts_max_distance() = 128 (DSRL_E_UNSUPPORTED above, DSRL_E_BADARG
 *   below, as for a dimension below 1 or a null pred, target or counts); N*H*W < 2^31 - 2^16 (DSRL_E_UNSUPPORTED); ws 2-byte aligned, ws_bytes >= the query
 *   (DSRL_E_WORKSPACE).  The query depends on its arguments only and holds for every launch of that shape (0 for arguments the launch refuses).
 * ---------------------------------------------------------------------------------------------- */
int dsrl_boundary_counts_max_classes(void);
int dsrl_boundary_counts_max_distance(void);
size_t dsrl_boundary_counts_workspace_bytes(int N, int H, int W, int d);
int dsrl_boundary_counts(const uint8_t* pred, const uint8_t* target, int N, int H, int W, int C, int ignore_index, int d,
                         unsigned long long* counts /*[3*C]: I | G | P, ADDED to*/, uint8_t* band /*nullable*/, int* nan_flag /*nullable*/, void* ws,
                         size_t ws_bytes, dsrl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DSRL_HIP_H */
