// loss_scale.hip -- the dynamic loss scaler of the fp16 mixed-precision RPN step (RPNTrainer(conv_math="f16")), entirely on
// the device: the scale, the overflow flag, the skip decision and growth / back-off are words of one small device buffer that the
// kernels read and write; the host never reads them inside a step, so the step stays as asynchronous as the fp32 one.
//
// Serves the optimizer step of train_rpn.py:165-174 (MomentumSGD + WeightDecay through chainer's updater) for a step whose gradients were
// computed from S * dL/d(head outputs):
//   frcnn_scale_by_loss_scale_f32   x *= S                          (the heads' output gradient, right after frcnn_rpn_loss)
//   frcnn_grad_check_finite_f32     flag |= any(!isfinite(G))       (after the all-reduce: every rank decides on the same sums)
//   frcnn_sgd_momentum_wd_scaled    frcnn_sgd_momentum_wd on G * (1 / S), or nothing at all when the flag is set
//   frcnn_loss_scaler_update        back off / count / grow, clear the flag
// S is a power of two, so G * (1 / S) is the exact unscaled gradient (correctly rounded where it is subnormal, as G / S is) and the update
// is bit-identical to frcnn_sgd_momentum_wd on the unscaled gradient.  No FMA contraction (built with -ffp-contract=off).
#include "frcnn_common.h"
#include <string.h>

namespace {

// the state buffer: FRCNN_LOSS_SCALER_WORDS 32-bit words (include/frcnn_hip.h documents the order)
struct ScalerState {
    float scale;               // S
    float inv_scale;           // 1 / S (exact: S is a power of two)
    int good_steps;            // consecutive clean steps since the scale last changed
    int found_nonfinite;       // set by the finite check, cleared by the update
    int skipped_steps;         // updates skipped so far
    int overflow_steps;        // skipped steps that found the scale already at min_scale (backing off could not answer them)
    float step_scale;          // the scale the last finished step used (what its gradient buffer is multiplied by)
    int reserved;
};
static_assert(sizeof(ScalerState) == FRCNN_LOSS_SCALER_WORDS * 4, "state layout");

__global__ void __launch_bounds__(64)
loss_scaler_init_kernel(ScalerState *__restrict__ s, float init_scale) {
    if (threadIdx.x != 0) return;
    s->scale = init_scale;
    s->inv_scale = 1.0f / init_scale;
    s->good_steps = 0;
    s->found_nonfinite = 0;
    s->skipped_steps = 0;
    s->overflow_steps = 0;
    s->step_scale = init_scale;
    s->reserved = 0;
}

__global__ void __launch_bounds__(256)
scale_by_loss_scale_kernel(float *__restrict__ x, size_t n, const ScalerState *__restrict__ s) {
    const float sc = s->scale;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] *= sc;
}

__device__ __forceinline__ uint32_t nonfinite_bits(uint32_t u) { return (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// One read of the gradient buffer at the memory rate: 16-byte loads, four per thread in flight, an exponent-field test per word.  Nothing is
// written unless a non-finite value was seen; then ONE atomic OR per workgroup (a flag, not a sum: the result does not depend on order).
// `head` elements in front of the first 16-byte boundary and the tail behind the last whole vector are read one by one by workgroup 0.
__global__ void __launch_bounds__(256)
grad_check_finite_kernel(const float *__restrict__ g, size_t n, size_t head, ScalerState *__restrict__ s) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const uint4 *g4 = reinterpret_cast<const uint4 *>(g + head);
    const size_t n4 = (n - head) / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = g4[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) bad |= nonfinite_bits(v[u].x) | nonfinite_bits(v[u].y) | nonfinite_bits(v[u].z) | nonfinite_bits(v[u].w);
    }
    for (; i < n4; i += stride) {
        const uint4 v = g4[i];
        bad |= nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
    }
    if (blockIdx.x == 0) {
        const uint32_t *gu = reinterpret_cast<const uint32_t *>(g);
        for (size_t k = threadIdx.x; k < head; k += blockDim.x) bad |= nonfinite_bits(gu[k]);
        for (size_t k = head + n4 * 4 + threadIdx.x; k < n; k += blockDim.x) bad |= nonfinite_bits(gu[k]);
    }
    if (__any((int)bad) && (threadIdx.x & (FRCNN_WAVE - 1)) == 0) s_bad = 1;       // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0 && s_bad != 0) atomicOr(&s->found_nonfinite, 1);
}

// frcnn_sgd_momentum_wd's kernel (train.hip sgd_momentum_wd_kernel) on g * (1 / S); a step whose flag is set moves nothing
__global__ void __launch_bounds__(256)
sgd_momentum_wd_scaled_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ v, size_t n, float lr, float momentum, float wd,
                              const ScalerState *__restrict__ s) {
    if (s->found_nonfinite != 0) return;                           // grid-uniform: the check finished before this launch started
    const float inv = s->inv_scale;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float wi = w[i];
        const float gi = g[i] * inv + wd * wi;
        const float vi = momentum * v[i] - lr * gi;
        v[i] = vi;
        w[i] = wi + vi;
    }
}

__global__ void __launch_bounds__(64)
loss_scaler_update_kernel(ScalerState *__restrict__ s, float growth, float backoff, int growth_interval, float min_scale, float max_scale) {
    if (threadIdx.x != 0) return;
    float sc = s->scale;
    s->step_scale = sc;
    if (s->found_nonfinite != 0) {
        if (sc <= min_scale) s->overflow_steps += 1;
        sc *= backoff;
        if (sc < min_scale) sc = min_scale;
        s->good_steps = 0;
        s->skipped_steps += 1;
    } else {
        const int good = s->good_steps + 1;
        if (good >= growth_interval) {
            sc *= growth;
            if (sc > max_scale) sc = max_scale;
            s->good_steps = 0;
        } else {
            s->good_steps = good;
        }
    }
    s->scale = sc;
    s->inv_scale = 1.0f / sc;
    s->found_nonfinite = 0;
}

bool power_of_two(float v) {
    if (!(v > 0.0f) || v > 3.0e38f) return false;
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x007fffffu) == 0 && (u >> 23) != 0;              // a normal number with an empty mantissa field
}

}  // namespace

extern "C" {

int frcnn_loss_scaler_init(void *state, float init_scale, void *stream) {
    if (!state || !power_of_two(init_scale)) return FRCNN_ERR_INVALID;
    hipLaunchKernelGGL(loss_scaler_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (ScalerState *)state, init_scale);
    return frcnn_launch_status();
}

int frcnn_scale_by_loss_scale_f32(float *x, size_t n, const void *state, void *stream) {
    if (n == 0) return FRCNN_OK;
    if (!x || !state) return FRCNN_ERR_INVALID;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(scale_by_loss_scale_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, n, (const ScalerState *)state);
    return frcnn_launch_status();
}

int frcnn_grad_check_finite_f32(const float *g, size_t n, void *state, void *stream) {
    if (n == 0) return FRCNN_OK;
    if (!g || !state || (reinterpret_cast<uintptr_t>(g) & 3) != 0) return FRCNN_ERR_INVALID;
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) / 4;       // floats in front of the first 16-byte boundary
    if (head > n) head = n;
    // two workgroups per CU, each thread four 16-byte loads per trip: 17.1 M floats are 8 trips
    const size_t want = ((n - head) / 4 + 256 * 4 - 1) / (256 * 4);
    const size_t cap = 2 * (size_t)frcnn_cu_count();
    const int blocks = (int)(want < 1 ? 1 : (want < cap ? want : cap));
    hipLaunchKernelGGL(grad_check_finite_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n, head, (ScalerState *)state);
    return frcnn_launch_status();
}

int frcnn_sgd_momentum_wd_scaled(float *w, const float *grad, float *velocity, size_t n, float lr, float momentum, float weight_decay, const void *state,
                                 void *stream) {
    if (n == 0) return FRCNN_OK;
    if (!w || !grad || !velocity || !state) return FRCNN_ERR_INVALID;
    const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(sgd_momentum_wd_scaled_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, grad, velocity, n, lr, momentum, weight_decay,
                       (const ScalerState *)state);
    return frcnn_launch_status();
}

int frcnn_loss_scaler_update(void *state, float growth, float backoff, int growth_interval, float min_scale, float max_scale, void *stream) {
    if (!state || growth_interval < 1 || !power_of_two(growth) || !power_of_two(backoff) || !power_of_two(min_scale) || !power_of_two(max_scale) ||
        growth < 1.0f || backoff > 1.0f || min_scale > max_scale)
        return FRCNN_ERR_INVALID;
    hipLaunchKernelGGL(loss_scaler_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (ScalerState *)state, growth, backoff, growth_interval, min_scale,
                       max_scale);
    return frcnn_launch_status();
}

}  // extern "C"
