// optimizer.hip -- the update rules of utils/prepare_train.py:146-167 (get_optimizer: --opt Adam / AdaGrad / RMSprop; MomentumSGD is
// train.hip's frcnn_sgd_momentum_wd) as ONE kernel family over the trainers' flat fp32 arenas: w, grad and one or two state buffers.
//
// The arithmetic is Chainer v1's published update rules, every operation rounded separately in fp32 and parenthesised as written here
// (no FMA contraction: built with -ffp-contract=off; `/` and sqrtf are the correctly rounded forms, hipcc's default for HIP):
//   all rules  ge = g * inv_S + wd * w                          (inv_S = 1 without a loss scaler: the expression of sgd_momentum_wd_scaled_kernel)
//   Adam       m = m + omb1 * (ge - m);  v = v + omb2 * ((ge * ge) - v);  w = w - ((lr_t * m) / (sqrt(v) + eps))
//              omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2), lr_t = (float)(alpha * sqrt(1 - beta2^t) / (1 - beta1^t)) in double
//   AdaGrad    h = h + (ge * ge);                                         w = w - ((lr * ge) / (sqrt(h) + eps))
//   RMSprop    ms = (alpha * ms) + ((oma * ge) * ge);                     w = w - ((lr * ge) / (sqrt(ms) + eps)),   oma = (float)(1.0 - alpha)
//
// Adam's bias correction depends on t = the number of APPLIED steps, and in the fp16 step only the device knows whether a step is applied
// (csrc/loss_scale.hip: the overflow flag is never read by the host).  So t, the two powers and lr_t are words of a small device buffer
// (OptState; include/frcnn_hip.h documents the order): a one-lane prologue launch advances them -- or leaves them alone when the flag is
// set -- and the update launch that follows on the same stream reads lr_t.  beta1^t and beta2^t are RUNNING DOUBLE PRODUCTS, multiplied
// by the step's beta once per applied step (p = p * beta, starting from 1.0): no pow() on the device, and a beta schedule is followed.
//
// Memory path: the update is pure bandwidth (Adam: 4 words read, 3 written per parameter).  When every pointer is 16-byte aligned a thread
// moves 16-byte vectors, four per stream in flight before the first use; a workgroup walks contiguous tiles of 1024 vectors, grid-stride,
// at most 8 workgroups per CU; the < 4 elements behind the last whole vector are done one by one by workgroup 0.  Any other alignment
// takes the same kernel on single floats: the same arithmetic per element, hence the same bits.  No LDS, no scratch.
#include "frcnn_common.h"
#include <math.h>

namespace {

struct OptState {
    int t;                     // applied steps so far
    float lr_t;                // the step size of the last applied Adam step
    double beta1_pow_t;        // running product beta1^t
    double beta2_pow_t;        // running product beta2^t
    int reserved[2];
};
static_assert(sizeof(OptState) == FRCNN_OPT_STATE_WORDS * 4, "state layout");

// what this file reads of loss_scale.hip's state buffer (the word order is part of the ABI: include/frcnn_hip.h)
struct ScalerWords {
    float scale, inv_scale;
    int good_steps, found_nonfinite;
    int rest[4];
};
static_assert(sizeof(ScalerWords) == FRCNN_LOSS_SCALER_WORDS * 4, "scaler state layout");

struct OptConst {
    float lr;                  // AdaGrad, RMSprop: lr; Adam: replaced by the state's lr_t inside the kernel
    float c1, c2;              // Adam: omb1, omb2; RMSprop: alpha, oma
    float eps, wd;
};

__global__ void __launch_bounds__(64)
opt_state_init_kernel(OptState *__restrict__ s, int t, double p1, double p2) {
    if (threadIdx.x != 0) return;
    s->t = t;
    s->lr_t = 0.0f;
    s->beta1_pow_t = p1;
    s->beta2_pow_t = p2;
    s->reserved[0] = s->reserved[1] = 0;
}

// the prologue of an update launch: one lane counts the step and, for Adam, forms its step size; a skipped step leaves every word alone
__global__ void __launch_bounds__(64)
opt_state_advance_kernel(OptState *__restrict__ s, int adam, double alpha, double beta1, double beta2, const ScalerWords *__restrict__ sc) {
    if (threadIdx.x != 0) return;
    if (sc != nullptr && sc->found_nonfinite != 0) return;
    s->t += 1;
    if (!adam) return;
    const double p1 = s->beta1_pow_t * beta1;
    const double p2 = s->beta2_pow_t * beta2;
    s->beta1_pow_t = p1;
    s->beta2_pow_t = p2;
    const double fix1 = 1.0 - p1;
    const double fix2 = 1.0 - p2;
    s->lr_t = (float)((alpha * sqrt(fix2)) / fix1);
}

template <int RULE>
__device__ __forceinline__ void opt_element(float &w, float g, float &s1, float &s2, const OptConst &c, float inv) {
    const float ge = g * inv + c.wd * w;
    if (RULE == FRCNN_OPT_ADAM) {
        s1 = s1 + c.c1 * (ge - s1);
        s2 = s2 + c.c2 * ((ge * ge) - s2);
        w = w - ((c.lr * s1) / (sqrtf(s2) + c.eps));
    } else if (RULE == FRCNN_OPT_ADAGRAD) {
        s1 = s1 + (ge * ge);
        w = w - ((c.lr * ge) / (sqrtf(s1) + c.eps));
    } else {
        s1 = (c.c1 * s1) + ((c.c2 * ge) * ge);
        w = w - ((c.lr * ge) / (sqrtf(s1) + c.eps));
    }
}

typedef float opt_f4 __attribute__((ext_vector_type(4)));           // a 16-byte vector the compiler moves as ONE global_load / store_dwordx4

template <int RULE>
__device__ __forceinline__ void opt_apply(float &w, const float &g, float &s1, float &s2, const OptConst &c, float inv) {
    opt_element<RULE>(w, g, s1, s2, c, inv);
}
template <int RULE>
__device__ __forceinline__ void opt_apply(opt_f4 &w, const opt_f4 &g, opt_f4 &s1, opt_f4 &s2, const OptConst &c, float inv) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float wj = w[j], aj = s1[j], bj = s2[j];
        opt_element<RULE>(wj, g[j], aj, bj, c, inv);
        w[j] = wj;
        s1[j] = aj;
        s2[j] = bj;
    }
}

// every word is read once and written once per step and not touched again before the next step's forward pass: non-temporal both ways
template <typename V> __device__ __forceinline__ V opt_load(const V *p) { return __builtin_nontemporal_load(p); }
template <typename V> __device__ __forceinline__ void opt_store(V v, V *p) { __builtin_nontemporal_store(v, p); }

constexpr int kInFlight = 4;       // loads per stream a thread issues before it uses the first
constexpr int kThreads = 256;

// V = opt_f4 (all pointers 16-byte aligned) or float.  s2 is touched by Adam only.  A workgroup takes CONTIGUOUS tiles of kThreads * kInFlight
// units (a thread's kInFlight units lie kThreads units apart), tile t, t + gridDim.x, ...; the last tile may be partial.
template <int RULE, typename V>
__global__ void __launch_bounds__(kThreads)
opt_update_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ s1, float *__restrict__ s2, size_t n, OptConst c,
                  const OptState *__restrict__ os, const ScalerWords *__restrict__ sc) {
    if (sc != nullptr && sc->found_nonfinite != 0) return;         // grid-uniform: the check finished before this launch started
    const float inv = sc != nullptr ? sc->inv_scale : 1.0f;
    if (RULE == FRCNN_OPT_ADAM) c.lr = os->lr_t;                   // written by the prologue launch in front of this one
    constexpr bool TWO = RULE == FRCNN_OPT_ADAM;
    constexpr size_t L = sizeof(V) / sizeof(float);
    constexpr size_t TILE = (size_t)kThreads * kInFlight;
    const size_t nv = n / L;
    V *wv = reinterpret_cast<V *>(w);
    const V *gv = reinterpret_cast<const V *>(g);
    V *av = reinterpret_cast<V *>(s1);
    V *bv = reinterpret_cast<V *>(s2);
    const size_t tiles = (nv + TILE - 1) / TILE;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t base = t * TILE + threadIdx.x;
        if ((t + 1) * TILE > nv) {                                 // the last, partial tile: one unit at a time
            for (size_t i = base; i < nv; i += kThreads) {
                V rw = opt_load(wv + i), ra = opt_load(av + i), rb = ra;
                const V rg = opt_load(gv + i);
                if (TWO) rb = opt_load(bv + i);
                opt_apply<RULE>(rw, rg, ra, rb, c, inv);
                opt_store(rw, wv + i);
                opt_store(ra, av + i);
                if (TWO) opt_store(rb, bv + i);
            }
            continue;
        }
        V rw[kInFlight], rg[kInFlight], ra[kInFlight], rb[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const size_t i = base + (size_t)u * kThreads;
            rw[u] = opt_load(wv + i);
            rg[u] = opt_load(gv + i);
            ra[u] = opt_load(av + i);
            rb[u] = TWO ? opt_load(bv + i) : ra[u];
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) opt_apply<RULE>(rw[u], rg[u], ra[u], rb[u], c, inv);
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const size_t i = base + (size_t)u * kThreads;
            opt_store(rw[u], wv + i);
            opt_store(ra[u], av + i);
            if (TWO) opt_store(rb[u], bv + i);
        }
    }
    if (L > 1 && blockIdx.x == 0) {                                // the elements behind the last whole vector
        for (size_t k = nv * L + threadIdx.x; k < n; k += blockDim.x) {
            float rw = w[k], ra = s1[k], rb = ra;
            if (TWO) rb = s2[k];
            opt_element<RULE>(rw, g[k], ra, rb, c, inv);
            w[k] = rw;
            s1[k] = ra;
            if (TWO) s2[k] = rb;
        }
    }
}

template <int RULE>
void launch_update(float *w, const float *g, float *s1, float *s2, size_t n, const OptConst &c, const OptState *os, const ScalerWords *sc, hipStream_t stream) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(s1) |
                           (RULE == FRCNN_OPT_ADAM ? reinterpret_cast<uintptr_t>(s2) : 0);
    const bool vec = (bits & 15) == 0;
    // one workgroup per tile up to 8 workgroups per CU; beyond that a workgroup walks several tiles (the 17.1 M floats of the RPN arena: three trips)
    const size_t units = vec ? n / 4 : n;
    const size_t want = (units + kThreads * kInFlight - 1) / (kThreads * kInFlight);
    const size_t cap = 8 * (size_t)frcnn_cu_count();
    const int blocks = (int)(want < 1 ? 1 : (want < cap ? want : cap));
    if (vec) hipLaunchKernelGGL((opt_update_kernel<RULE, opt_f4>), dim3(blocks), dim3(kThreads), 0, stream, w, g, s1, s2, n, c, os, sc);
    else hipLaunchKernelGGL((opt_update_kernel<RULE, float>), dim3(blocks), dim3(kThreads), 0, stream, w, g, s1, s2, n, c, os, sc);
}

bool unit_interval(double v) { return v >= 0.0 && v < 1.0; }       // (false for NaN)

}  // namespace

extern "C" {

int frcnn_opt_state_init(void *opt_state, int t, double beta1_pow_t, double beta2_pow_t, void *stream) {
    if (!opt_state || (reinterpret_cast<uintptr_t>(opt_state) & 7) != 0 || t < 0 || !(beta1_pow_t >= 0.0 && beta1_pow_t <= 1.0) ||
        !(beta2_pow_t >= 0.0 && beta2_pow_t <= 1.0))
        return FRCNN_ERR_INVALID;
    hipLaunchKernelGGL(opt_state_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OptState *)opt_state, t, beta1_pow_t, beta2_pow_t);
    return frcnn_launch_status();
}

int frcnn_opt_step(int rule, float *w, const float *grad, float *state1, float *state2, size_t n, double lr, double beta1, double beta2, float eps,
                   float weight_decay, void *opt_state, const void *scaler_state, void *stream) {
    if (rule != FRCNN_OPT_ADAM && rule != FRCNN_OPT_ADAGRAD && rule != FRCNN_OPT_RMSPROP) return FRCNN_ERR_INVALID;
    if (!(eps > 0.0f)) return FRCNN_ERR_INVALID;
    if (rule == FRCNN_OPT_ADAM && (!unit_interval(beta1) || !unit_interval(beta2))) return FRCNN_ERR_INVALID;
    if (rule == FRCNN_OPT_RMSPROP && !unit_interval(beta1)) return FRCNN_ERR_INVALID;
    if (!w || !grad || !state1 || (rule == FRCNN_OPT_ADAM && (!state2 || !opt_state))) return FRCNN_ERR_INVALID;
    if (((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(state1) | reinterpret_cast<uintptr_t>(state2)) & 3) != 0 ||
        (reinterpret_cast<uintptr_t>(opt_state) & 7) != 0)
        return FRCNN_ERR_INVALID;
    if (n == 0) return FRCNN_OK;
    hipStream_t st = (hipStream_t)stream;
    const ScalerWords *sc = (const ScalerWords *)scaler_state;
    OptState *os = (OptState *)opt_state;
    if (os != nullptr)
        hipLaunchKernelGGL(opt_state_advance_kernel, dim3(1), dim3(64), 0, st, os, rule == FRCNN_OPT_ADAM ? 1 : 0, lr, beta1, beta2, sc);
    OptConst c;
    c.lr = (float)lr;
    c.c1 = c.c2 = 0.0f;
    c.eps = eps;
    c.wd = weight_decay;
    if (rule == FRCNN_OPT_ADAM) {
        c.c1 = (float)(1.0 - beta1);
        c.c2 = (float)(1.0 - beta2);
        launch_update<FRCNN_OPT_ADAM>(w, grad, state1, state2, n, c, os, sc, st);
    } else if (rule == FRCNN_OPT_ADAGRAD) {
        launch_update<FRCNN_OPT_ADAGRAD>(w, grad, state1, state1, n, c, os, sc, st);
    } else {
        c.c1 = (float)beta1;
        c.c2 = (float)(1.0 - beta1);
        launch_update<FRCNN_OPT_RMSPROP>(w, grad, state1, state1, n, c, os, sc, st);
    }
    return frcnn_launch_status();
}

}  // extern "C"
