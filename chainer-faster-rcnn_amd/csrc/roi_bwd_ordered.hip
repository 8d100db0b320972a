// roi_bwd_ordered.hip -- RoI max-pooling backward with a FIXED order of additions (the backward of F.roi_pooling_2d, call site models/faster_rcnn.py:125-126):
// dx[c, argmax[r, c, b]] += dy[r, c, b], the RoIs r ascending and within a RoI the bins b ascending -- the order of the reference's CPU loop.
// The plane-resident kernel of roi_pool.hip adds into its LDS cells with float atomics in whatever order its waves arrive: two runs differ in the last bit of a
// few cells.  In the fp32 step that stays at rounding level; the mixed-precision step (RCNNTrainer(precision=...)) rounds this map to 16 bits for conv5_3's
// backward products, where a last-bit difference decides a rounding now and then, and the trunk's gradients then differ by 1e-4 ... 1e-3 between two runs.
// Here one WAVE owns one channel plane of dx in LDS and walks the RoIs in order; the <= 64 bins of a RoI sit one per lane.  Bins of one RoI that hit the same
// cell (small RoIs) are served in rounds: every pending lane puts its lane number into the cell's slot of a tag plane with an integer minimum (ds_min_u32:
// the result of a minimum does not depend on the order of its operands), the lane that reads its own number back is the LOWEST pending bin of that cell, adds
// its value to the cell and clears the tag; the others go round again.  A RoI whose bins hit distinct cells takes one round.  No floating-point atomics:
// identical bits from run to run, and the same order of additions as the reference's loop.  The (cell, value) pairs of eight RoIs are fetched as one batch of
// independent loads.
#include "frcnn_common.h"

namespace {

template <int NW, int PLANE>
__global__ void __launch_bounds__(64 * NW)
roi_pool_bwd_ordered_kernel(const float *__restrict__ dy, const int32_t *__restrict__ argmax, int R, int C, int HW, int bins, float *__restrict__ dx) {
    constexpr int U = 8;
    __shared__ float planes[NW * PLANE];
    __shared__ uint32_t tags[NW * PLANE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int c = (int)blockIdx.x * NW + wave;
    if (c >= C) return;                                                    // (wave-uniform; no workgroup barrier below)
    float *plane = planes + wave * PLANE;
    uint32_t *tag = tags + wave * PLANE;
    for (int i = lane; i < HW; i += 64) { plane[i] = 0.0f; tag[i] = 0xffffffffu; }
    __builtin_amdgcn_wave_barrier();                                       // wave-private LDS, in-order DS: a scheduling fence only
    const bool live = lane < bins;
    for (int r0 = 0; r0 < R; r0 += U) {
        int tg[U];
        float vl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = live && r0 + u < R;
            const size_t i = ((size_t)(ok ? r0 + u : 0) * C + c) * bins + (ok ? lane : 0);
            const int a = argmax[i];
            const float v = dy[i];
            tg[u] = (ok && a >= 0 && a < HW) ? a : -1;
            vl[u] = v;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = tg[u];
            const int cell = t >= 0 ? t : 0;
            int pend = t >= 0 ? 1 : 0;
            while (__any(pend)) {                                          // rounds: the lowest pending bin of every cell adds, the rest wait
                atomicMin(&tag[cell], pend ? (uint32_t)lane : 0xffffffffu);   // (a lane with nothing pending offers the neutral element)
                __builtin_amdgcn_wave_barrier();
                const int win = pend & (tag[cell] == (uint32_t)lane ? 1 : 0);
                __builtin_amdgcn_wave_barrier();                           // every lane has read its tag before a winner clears one
                if (win) {
                    plane[cell] += vl[u];
                    tag[cell] = 0xffffffffu;
                }
                pend &= ~win;
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    float *out = dx + (size_t)c * HW;
    for (int i = lane; i < HW; i += 64) out[i] = plane[i];
}

}  // namespace

extern "C" int frcnn_roi_pool_bwd_ordered(const float *dy, const int32_t *argmax, int R, int C, int H, int W, int outh, int outw, float *dx, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dy || !argmax || !dx || R < 0 || C < 1 || H < 1 || W < 1 || outh < 1 || outw < 1) return FRCNN_ERR_INVALID;
    const int bins = outh * outw, HW = H * W;
    if (bins > 64 || HW > 16384) return FRCNN_ERR_UNSUPPORTED;             // a RoI's bins sit one per lane; a channel plane and its tags sit in LDS
    if (HW <= 38 * 64) hipLaunchKernelGGL((roi_pool_bwd_ordered_kernel<4, 38 * 64>), dim3(frcnn_cdiv(C, 4)), dim3(256), 0, stream, dy, argmax, R, C, HW, bins, dx);
    else hipLaunchKernelGGL((roi_pool_bwd_ordered_kernel<1, 16384>), dim3(C), dim3(64), 0, stream, dy, argmax, R, C, HW, bins, dx);
    return frcnn_launch_status();
}
