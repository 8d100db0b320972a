// resnet_bf16.hip -- the ResNet trunk's own pieces on the 16-bit chain (models/resnet.py -> chainer ResNetLayers, /root/reference/models/resnet.py:11-45):
// the bottleneck 1x1 convolution (stride 1 or 2, optional fused residual tail), the 7x7/2 stem's columns and the 3x3/2 max-pool, all on channel-blocked
// [C/16][H][W][16] 16-bit maps.  The 3x3 conv2 of every bottleneck runs on conv_bf16.hip's kernels unchanged.  Operands rounded to nearest even, fp32
// accumulation on v_mfma_f32_32x32x16_bf16 (fp16 twin: resnet_f16.hip, the same source under FRCNN_HALF_F16).
//
// The 1x1 convolution is a GEMM over the FLAT pixel axis: y[co][p] = act(sum_ci W[co][ci] x[ci][src(p)] + b[co] (+ r[co][p])), src(p) = p at stride 1,
// (2*(p / Wo), 2*(p % Wo)) at stride 2 (pad 0: Chainer's 1x1 / stride 2, i.e. frcnn_subsample2_f32 folded into the load).  Both operands are
// fragment-ready in memory: a 16-channel K-chunk of 32 pixels of x ([C/16][HW][16]) and of 32 weight rows (frcnn_bf16_pack_conv_w, ksize 1:
// [CinP/16][CoutP][16]) is 16 contiguous bytes per MFMA lane, so the waves read their fragments straight from global memory (L1 / L2) -- no LDS
// staging, no barrier in the K loop -- in batches of kC1Batch chunks with the next batch in flight while the current one feeds the MFMAs.
// A wave owns 64 couts x 32 pixels (two accumulators); a workgroup of 4 waves owns 128 couts x 64 px (WCO 2) or, for CoutP <= 64, 64 couts x 128 px
// (WCO 1).  Launches with fewer tiles than the chip has CUs split K across workgroups (at most 8 ways, at least 4 chunks per wave): partial tiles go
// to a caller-owned workspace and the last arriver adds them in split order (deterministic), the same contract as frcnn_conv_bf16_ws.
#include "frcnn_common.h"
#include <stdlib.h>
#include <frcnn_buffer.h>   // angle brackets: shadowed by the test emulator
#include <frcnn_intrin.h>
#include <frcnn_sync.h>

namespace {

constexpr int kC1Batch = 4;                          // K-chunks (16 channels) whose fragment loads a wave issues together
constexpr int kC1MaxSplit = 8;
constexpr size_t kC1CounterPageBytes = 64 * 1024;    // tile counters: zeroed once, left zeroed by every launch
constexpr size_t kC1SlotBytes = 256 * 2 * 16 * sizeof(float);   // one split's partial tile: 256 threads x 2 accumulators

__device__ __forceinline__ uint4 c1_as_u4(float4 v) { return make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)); }

// WCO = waves along cout (2: 128co x 64px tiles, 1: 64co x 128px tiles); STRIDE 1 or 2
template <int WCO, int STRIDE>
__global__ void __launch_bounds__(256)
conv1x1_bf16_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ wp, const float *__restrict__ bias, const uint16_t *__restrict__ res,
                    uint16_t *__restrict__ y, int CinP, int Cout, int CoutP, int H, int W, int Wo, int HWo, int act, int ptiles, int nsplit,
                    float *__restrict__ partial_ws, int *__restrict__ tile_counters) {
    constexpr int WPX = 4 / WCO;                                 // waves along the pixel axis
    constexpr int TPX = 32 * WPX, TCO = 64 * WCO;                // tile
    __shared__ int s_ticket;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int tile = blockIdx.x / nsplit, split = blockIdx.x - tile * nsplit;
    const int pt = tile % ptiles, ct = tile / ptiles;
    const int p0 = pt * TPX + (wave % WPX) * 32, co0 = ct * TCO + (wave / WPX) * 64;
    const int nchunks = CinP / 16;
    const int per = (nchunks + nsplit - 1) / nsplit;
    const int cbeg = split * per, cend = min(nchunks, cbeg + per);
    const int HW = H * W;
    const frcnn_buf_t xbuf = frcnn_make_buf(x, (uint32_t)((size_t)CinP * HW * 2));
    const frcnn_buf_t wbuf = frcnn_make_buf(wp, (uint32_t)((size_t)CinP * CoutP * 2));
    // per-lane byte offsets inside chunk 0 (pixels past the map, weight rows past CoutP: out of range -> zeros)
    const int p = p0 + l31;
    int src = p;
    if (STRIDE == 2) { const int oy = p / Wo; src = 2 * oy * W + 2 * (p - oy * Wo); }
    const uint32_t b_off = p < HWo ? (uint32_t)(src * 32 + khalf * 16) : kBufOob;
    uint32_t a_off[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) a_off[cb] = co0 + cb * 32 + l31 < CoutP ? (uint32_t)((co0 + cb * 32 + l31) * 32 + khalf * 16) : kBufOob;
    const uint32_t x_chunk = (uint32_t)HW * 32u, w_chunk = (uint32_t)CoutP * 32u;
    frcnn_f32x16 acc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
    float4 bq[kC1Batch], aq[kC1Batch][2];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int u = 0; u < kC1Batch; ++u) {
            const bool in = c0 + u < cend;                       // chunks past this split's range read zeros (and cost an MFMA on zeros)
            const uint32_t c = (uint32_t)(c0 + u);
            bq[u] = frcnn_buf_load_f32x4(xbuf, in && b_off != kBufOob ? b_off + c * x_chunk : kBufOob);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) aq[u][cb] = frcnn_buf_load_f32x4(wbuf, in && a_off[cb] != kBufOob ? a_off[cb] + c * w_chunk : kBufOob);
        }
    };
    if (cbeg < cend) fetch(cbeg);
    for (int c0 = cbeg; c0 < cend; c0 += kC1Batch) {
        uint4 bv[kC1Batch], av[kC1Batch][2];
#pragma unroll
        for (int u = 0; u < kC1Batch; ++u) {
            bv[u] = c1_as_u4(bq[u]);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) av[u][cb] = c1_as_u4(aq[u][cb]);
        }
        if (c0 + kC1Batch < cend) fetch(c0 + kC1Batch);          // the next batch in flight while this one feeds the MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kC1Batch; ++u)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[cb] = frcnn_mfma_32x32x16_bf16(av[u][cb], bv[u], acc[cb]);
    }
    if (nsplit > 1) {
        // publish this split's accumulators (write-through float4s), take a ticket; the last arriver sums the splits in split order
        float *slot = partial_ws + ((size_t)tile * nsplit + split) * (kC1SlotBytes / sizeof(float));
        const frcnn_buf_t pbuf = frcnn_make_buf(slot, (uint32_t)kC1SlotBytes);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                frcnn_buf_store_f32x4_wt(pbuf, (uint32_t)(((cb * 4 + r4) * 256 + tid) * 16),
                                         make_float4(acc[cb][4 * r4], acc[cb][4 * r4 + 1], acc[cb][4 * r4 + 2], acc[cb][4 * r4 + 3]));
        frcnn_drain_vmem();
        __syncthreads();
        if (tid == 0) s_ticket = frcnn_ticket(&tile_counters[tile]);
        __syncthreads();
        if (s_ticket != nsplit - 1) return;                      // workgroup-uniform
        if (tid == 0) {
            frcnn_acquire_agent();
            frcnn_counter_reset(&tile_counters[tile]);           // leave the counter page zeroed for the next launch
        }
        __syncthreads();
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
        for (int q = 0; q < nsplit; ++q) {
            const float4 *piece = reinterpret_cast<const float4 *>(partial_ws + ((size_t)tile * nsplit + q) * (kC1SlotBytes / sizeof(float)));
            float4 v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = piece[(size_t)e * 256 + tid];
#pragma unroll
            for (int e = 0; e < 8; ++e) frcnn_pin(v[e]);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const float4 t = v[cb * 4 + r4];
                    acc[cb][4 * r4] += t.x; acc[cb][4 * r4 + 1] += t.y; acc[cb][4 * r4 + 2] += t.z; acc[cb][4 * r4 + 3] += t.w;
                }
        }
    }
    // epilogue: register r of lane l = cout (r&3) + 8*(r>>2) + 4*khalf of pixel l31 -> four consecutive couts of one pixel = one 8-byte store
    if (p >= HWo) return;
    const frcnn_buf_t bbuf = frcnn_make_buf(bias, (uint32_t)Cout * 4u);
    const size_t HWs = (size_t)HWo;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = co0 + cb * 32 + 8 * g + 4 * khalf;
            if (co >= CoutP) continue;
            const size_t off = ((size_t)(co >> 4) * HWs + p) * 16 + (co & 15);
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = acc[cb][4 * g + t] + frcnn_buf_load_f32(bbuf, (uint32_t)(co + t) * 4u);
            if (act == 3) {
                const uint2 rq = *reinterpret_cast<const uint2 *>(res + off);
                v[0] += frcnn_h16_to_f32((uint16_t)(rq.x & 0xffffu)); v[1] += frcnn_h16_to_f32((uint16_t)(rq.x >> 16));
                v[2] += frcnn_h16_to_f32((uint16_t)(rq.y & 0xffffu)); v[3] += frcnn_h16_to_f32((uint16_t)(rq.y >> 16));
            }
            if (act != 0) {
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.0f);
            }
            *reinterpret_cast<uint2 *>(y + off) = make_uint2(frcnn_pack_bf16x2(v[0], v[1]), frcnn_pack_bf16x2(v[2], v[3]));
        }
}

// the stem's columns: cols[(ci*49 + ky*7 + kx)][oy][ox] = x[ci][2*oy - 3 + ky][2*ox - 3 + kx] (0 outside; rows Cin*49 .. Kp-1 zero), written
// channel-blocked [Kp/16][OH*OW][16]: one thread = one output pixel x 8 rows (one 16-byte store)
__global__ void __launch_bounds__(256)
im2col7x7s2_bf16_kernel(const float *__restrict__ x, int Cin, int H, int W, int OH, int OW, int Kp, uint16_t *__restrict__ cols) {
    const size_t OHW = (size_t)OH * OW, total = (size_t)(Kp / 8) * OHW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int half = (int)(i & 1);
        const size_t pq = (i >> 1) % OHW;
        const int kb = (int)((i >> 1) / OHW);
        const int oy = (int)(pq / OW), ox = (int)(pq - (size_t)oy * OW);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = kb * 16 + half * 8 + e;
            v[e] = 0.0f;
            if (k < Cin * 49) {
                const int ci = k / 49, t = k - ci * 49, ky = t / 7, kx = t - ky * 7;
                const int iy = 2 * oy - 3 + ky, ix = 2 * ox - 3 + kx;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) v[e] = x[((size_t)ci * H + iy) * W + ix];
            }
        }
        *reinterpret_cast<uint4 *>(cols + (((size_t)kb * OHW + pq) * 16 + half * 8)) =
            make_uint4(frcnn_pack_bf16x2(v[0], v[1]), frcnn_pack_bf16x2(v[2], v[3]), frcnn_pack_bf16x2(v[4], v[5]), frcnn_pack_bf16x2(v[6], v[7]));
    }
}

// F.max_pooling_2d(3, stride 2), cover_all (OH = ceil((H-3)/2)+1, windows clipped at the border), channel-blocked in and out: one thread = one
// output pixel x 8 channels.  A maximum of 16-bit values is a 16-bit value: exact, the same values as frcnn_maxpool3x3s2_f32 on the widened map.
__global__ void __launch_bounds__(256)
maxpool3x3s2_bf16_kernel(const uint16_t *__restrict__ x, uint16_t *__restrict__ y, int C, int H, int W, int OH, int OW) {
    const size_t total = (size_t)(C / 16) * OH * OW * 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int half = (int)(i & 1), ow = (int)((i >> 1) % OW), oh = (int)(((i >> 1) / OW) % OH), cb = (int)((i >> 1) / ((size_t)OW * OH));
        const uint16_t *base = x + ((size_t)cb * H * W) * 16 + half * 8;
        float m[8];
        {
            const uint4 q = *reinterpret_cast<const uint4 *>(base + ((size_t)(2 * oh) * W + 2 * ow) * 16);
            const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = frcnn_h16_to_f32((uint16_t)(w4[e >> 1] >> (16 * (e & 1))));
        }
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = 2 * oh + dy, ix = 2 * ow + dx;
                if (iy >= H || ix >= W) continue;
                const uint4 q = *reinterpret_cast<const uint4 *>(base + ((size_t)iy * W + ix) * 16);
                const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], frcnn_h16_to_f32((uint16_t)(w4[e >> 1] >> (16 * (e & 1)))));
            }
        *reinterpret_cast<uint4 *>(y + (((size_t)cb * OH + oh) * OW + ow) * 16 + half * 8) =
            make_uint4(frcnn_f32_to_h16_exact(m[0]) | (frcnn_f32_to_h16_exact(m[1]) << 16), frcnn_f32_to_h16_exact(m[2]) | (frcnn_f32_to_h16_exact(m[3]) << 16),
                       frcnn_f32_to_h16_exact(m[4]) | (frcnn_f32_to_h16_exact(m[5]) << 16), frcnn_f32_to_h16_exact(m[6]) | (frcnn_f32_to_h16_exact(m[7]) << 16));
    }
}

struct C1Plan { int wco, ptiles, tiles, nsplit; };

// The tile shape and K split of a 1x1 launch.  Default: WCO 2 unless CoutP <= 64; split K (powers of two, at most 8 ways, at least 4 chunks per wave)
// until the launch has a workgroup per CU.  FRCNN_C1_SPLIT=1/2/4/8 forces a split (tests, A/B), still capped by the chunk count.
static C1Plan conv1x1_bf16_plan(int CinP, int CoutP, int HWo) {
    C1Plan pl;
    pl.wco = CoutP <= 64 ? 1 : 2;
    pl.ptiles = frcnn_cdiv(HWo, 32 * (4 / pl.wco));
    pl.tiles = pl.ptiles * frcnn_cdiv(CoutP, 64 * pl.wco);
    const int nchunks = CinP / 16;
    const int forced = frcnn_tune_int("FRCNN_C1_SPLIT", 0);
    int s = 1;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) s = forced;
    else {
        const long cus = frcnn_cu_count() > 0 ? frcnn_cu_count() : 256;
        while (s < kC1MaxSplit && (long)pl.tiles * s < cus && nchunks / (2 * s) >= 4) s *= 2;
    }
    while (s > 1 && nchunks / s < 4) s >>= 1;
    if ((long)pl.tiles > (long)(kC1CounterPageBytes / sizeof(int))) s = 1;      // one counter per tile in the page
    pl.nsplit = s;
    return pl;
}

static int conv1x1_out_size(int n, int stride) { return stride == 2 ? (n + 1) / 2 : n; }

}  // namespace

extern "C" {

size_t frcnn_conv1x1_bf16_workspace_bytes(int Cin, int Cout, int H, int W, int stride) {
    if (Cin < 1 || Cout < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return 0;
    const C1Plan pl = conv1x1_bf16_plan(frcnn_bf16_padded_channels(Cin), frcnn_bf16_padded_channels(Cout),
                                        conv1x1_out_size(H, stride) * conv1x1_out_size(W, stride));
    return kC1CounterPageBytes + (pl.nsplit > 1 ? (size_t)pl.tiles * pl.nsplit * kC1SlotBytes : 0);
}

int frcnn_conv1x1_bf16_workspace_init(void *workspace, size_t workspace_bytes, void *stream) {
    if (!workspace || workspace_bytes < kC1CounterPageBytes) return FRCNN_ERR_INVALID;
    FRCNN_HIP_TRY(hipMemsetAsync(workspace, 0, kC1CounterPageBytes, (hipStream_t)stream));
    return FRCNN_OK;
}

int frcnn_conv1x1_bf16_splits(int Cin, int Cout, int H, int W, int stride) {
    if (Cin < 1 || Cout < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return FRCNN_ERR_INVALID;
    return conv1x1_bf16_plan(frcnn_bf16_padded_channels(Cin), frcnn_bf16_padded_channels(Cout),
                             conv1x1_out_size(H, stride) * conv1x1_out_size(W, stride)).nsplit;
}

int frcnn_conv1x1_bf16(const uint16_t *x, const uint16_t *w_packed, const float *bias, const uint16_t *residual, uint16_t *y, int Cin, int Cout,
                       int H, int W, int stride, int act, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !w_packed || !bias || !y || Cin < 1 || Cout < 1 || H < 1 || W < 1) return FRCNN_ERR_INVALID;
    if ((stride != 1 && stride != 2) || (act != 0 && act != 1 && act != 3) || (act == 3 && !residual)) return FRCNN_ERR_INVALID;
    const int CinP = frcnn_bf16_padded_channels(Cin), CoutP = frcnn_bf16_padded_channels(Cout);
    const int Ho = conv1x1_out_size(H, stride), Wo = conv1x1_out_size(W, stride), HWo = Ho * Wo;
    if ((size_t)H * W * CinP * 2 >= (1ull << 31) || (size_t)CoutP * CinP * 2 >= (1ull << 31)) return FRCNN_ERR_INVALID;   // 32-bit buffer ranges
    C1Plan pl = conv1x1_bf16_plan(CinP, CoutP, HWo);
    if (pl.nsplit > 1 && (!workspace || workspace_bytes < kC1CounterPageBytes + (size_t)pl.tiles * pl.nsplit * kC1SlotBytes)) pl.nsplit = 1;
    float *partials = pl.nsplit > 1 ? (float *)((char *)workspace + kC1CounterPageBytes) : nullptr;
    int *counters = pl.nsplit > 1 ? (int *)workspace : nullptr;
    const dim3 grid((unsigned)(pl.tiles * pl.nsplit));
    hipStream_t s = (hipStream_t)stream;
#define FRCNN_C1_GO(WCO, STRIDE)                                                                                                       \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(conv1x1_bf16_kernel<WCO, STRIDE>), grid, dim3(256), 0, s, x, w_packed, bias, residual, y, CinP, Cout, \
                       CoutP, H, W, Wo, HWo, act, pl.ptiles, pl.nsplit, partials, counters)
    if (pl.wco == 2) { if (stride == 2) FRCNN_C1_GO(2, 2); else FRCNN_C1_GO(2, 1); }
    else { if (stride == 2) FRCNN_C1_GO(1, 2); else FRCNN_C1_GO(1, 1); }
#undef FRCNN_C1_GO
    return frcnn_launch_status();
}

int frcnn_im2col7x7s2_bf16(const float *x, int Cin, int H, int W, int Kp, uint16_t *cols, void *stream) {
    if (!x || !cols || Cin < 1 || H < 1 || W < 1 || Kp < Cin * 49 || Kp % 16 != 0) return FRCNN_ERR_INVALID;
    const int OH = (H + 6 - 7) / 2 + 1, OW = (W + 6 - 7) / 2 + 1;
    const size_t total = (size_t)(Kp / 8) * OH * OW;
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(im2col7x7s2_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, Cin, H, W, OH, OW, Kp, cols);
    return frcnn_launch_status();
}

int frcnn_maxpool3x3s2_bf16(const uint16_t *x, uint16_t *y, int C, int H, int W, void *stream) {
    if (!x || !y || C < 1 || H < 3 || W < 3) return FRCNN_ERR_INVALID;
    const int CP = frcnn_bf16_padded_channels(C);
    const int OH = (H - 3 + 1) / 2 + 1, OW = (W - 3 + 1) / 2 + 1;
    const size_t total = (size_t)(CP / 8) * OH * OW;
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(maxpool3x3s2_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, CP, H, W, OH, OW);
    return frcnn_launch_status();
}

}  // extern "C"
