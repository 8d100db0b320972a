// bn_train.hip -- BatchNormalization on batch statistics (forward and backward) and the backward of the two ResNet-only glue kernels
// (frcnn_maxpool3x3s2_f32, frcnn_subsample2_f32): what models/resnet.py needs to run the reference's models/resnet.py:41-45 with
// `test = not self.train` = False.  fp32 NCHW, batch 1: a map is (C, HW), a channel one contiguous row of m = HW values.
//
// Shape of both directions: two launches over a (channels, parts) grid, `parts` workgroups per channel each owning one contiguous slice of
// the row (bn_parts below: the rule of bias_grad_parts).
//   launch 1   every workgroup reduces its slice to two sums, accumulated in DOUBLE (forward: sum z, sum z^2; backward: sum g, sum g*xhat),
//              and writes them to the workspace at [c][part].
//   launch 2   every workgroup adds its channel's `parts` pairs IN PART ORDER (every thread the same few loads: a broadcast), derives the
//              channel's scalars and applies them to its slice.  The workgroup of part 0 also writes the per-channel outputs.  No third
//              "final" launch, no atomics: the same inputs give the same bits.
// Double accumulation is what keeps sum z^2 / m - mean^2 meaningful when |mean| >> std (a channel with mean 100 and std 0.01 loses every
// digit of its variance in a single fp32 pass); the kernels are memory-bound and an fp64 FMA per loaded value is hidden behind the loads.
// Loads and stores are 16-byte vectors over the aligned middle of a slice with scalar heads and tails (a row starts 16-byte aligned only
// when HW % 4 == 0); when the operands of one launch do not share their alignment modulo 16 the launch runs element by element.
#include "frcnn_common.h"
#include <frcnn_intrin.h>   // angle brackets: the test emulator shadows it
#include <initializer_list>

namespace {

constexpr int kBnMaxGridC = 32768;          // channels beyond this are strided over by the same workgroups

int bn_parts(int C, int HW) {
    int parts = frcnn_cdiv(1024, C);                      // about four workgroups per CU in total
    const int max_parts = frcnn_cdiv(HW, 2048);
    if (parts > max_parts) parts = max_parts;
    return parts < 1 ? 1 : parts;
}

// the slice [begin, end) of a row for workgroup `part`, and the number of leading scalars up to the first 16-byte boundary of `row`
struct BnSlice { int begin, end, head, n4; };
__device__ __forceinline__ BnSlice bn_slice(const float *row, int HW, int parts, int part, int vec) {
    BnSlice s;
    const int per = (HW + parts - 1) / parts;
    s.begin = min(HW, part * per);
    s.end = min(HW, s.begin + per);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(row + s.begin);
    s.head = vec ? (int)(((16 - (addr & 15)) & 15) >> 2) : s.end - s.begin;
    if (s.head > s.end - s.begin) s.head = s.end - s.begin;
    s.n4 = (s.end - s.begin - s.head) >> 2;
    return s;
}

// block-wide sum of two doubles, result valid in every thread
__device__ __forceinline__ void bn_block_sum2(double &a, double &b) {
    __shared__ double red[2][256];
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int q = 128; q > 0; q >>= 1) {
        if ((int)threadIdx.x < q) {
            red[0][threadIdx.x] += red[0][threadIdx.x + q];
            red[1][threadIdx.x] += red[1][threadIdx.x + q];
        }
        __syncthreads();
    }
    a = red[0][0];
    b = red[1][0];
    __syncthreads();                                                  // the next channel of a strided grid reuses the array
}

// the channel's two totals: its `parts` pairs added in part order
__device__ __forceinline__ void bn_sum_parts(const double *__restrict__ ws, int parts, double &a, double &b) {
    a = 0.0;
    b = 0.0;
    for (int p = 0; p < parts; ++p) {
        a += ws[2 * p];
        b += ws[2 * p + 1];
    }
}

__device__ __forceinline__ void bn_acc4(const float4 v, double &s, double &q) {
    const double x = v.x, y = v.y, z = v.z, w = v.w;
    s += (x + y) + (z + w);
    q += (x * x + y * y) + (z * z + w * w);
}

// ---- forward, launch 1: sum z and sum z^2 of a slice --------------------------------------------------
__global__ void __launch_bounds__(256)
bn_fwd_stats_kernel(const float *__restrict__ z, int C, int HW, int parts, int vec, double *__restrict__ ws) {
    const int part = blockIdx.y;
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        const float *p = z + (size_t)c * HW;
        const BnSlice sl = bn_slice(p, HW, parts, part, vec);
        double s = 0.0, q = 0.0;
        for (int j = sl.begin + threadIdx.x; j < sl.begin + sl.head; j += 256) {
            const double v = p[j];
            s += v;
            q += v * v;
        }
        const float4 *p4 = reinterpret_cast<const float4 *>(p + sl.begin + sl.head);
        // four independent 16-byte loads in flight per thread and trip, four running pairs added at the end in a fixed order
        double s1 = 0.0, q1 = 0.0, s2 = 0.0, q2 = 0.0, s3 = 0.0, q3 = 0.0;
        int i = threadIdx.x;
        for (; i + 768 < sl.n4; i += 1024) {
            float4 v0 = p4[i], v1 = p4[i + 256], v2 = p4[i + 512], v3 = p4[i + 768];
            frcnn_pin(v0); frcnn_pin(v1); frcnn_pin(v2); frcnn_pin(v3);
            bn_acc4(v0, s, q);
            bn_acc4(v1, s1, q1);
            bn_acc4(v2, s2, q2);
            bn_acc4(v3, s3, q3);
        }
        for (; i < sl.n4; i += 256) bn_acc4(p4[i], s, q);
        s = (s + s1) + (s2 + s3);
        q = (q + q1) + (q2 + q3);
        for (int j = sl.begin + sl.head + 4 * sl.n4 + threadIdx.x; j < sl.end; j += 256) {
            const double v = p[j];
            s += v;
            q += v * v;
        }
        bn_block_sum2(s, q);
        if (threadIdx.x == 0) {
            ws[2 * ((size_t)c * parts + part)] = s;
            ws[2 * ((size_t)c * parts + part) + 1] = q;
        }
    }
}

// ---- forward, launch 2: the channel's statistics from its partial sums, then y over the slice ---------
struct BnFwdScalars { double mean; float rstd, gamma, beta; };

template <bool RELU, bool RES>
__device__ __forceinline__ float bn_fwd_one(float z, float r, const BnFwdScalars &k) {
    // (z - mean) in double: the subtraction is where a channel with |mean| >> std would lose its digits to the rounding of mean
    float v = k.gamma * ((float)((double)z - k.mean) * k.rstd) + k.beta;
    if (RES) v += r;
    if (RELU) v = v > 0.0f ? v : 0.0f;
    return v;
}

template <bool RELU, bool RES>
__global__ void __launch_bounds__(256)
bn_fwd_apply_kernel(const float *__restrict__ z, const float *__restrict__ gamma, const float *__restrict__ beta,
                    const float *__restrict__ residual, const double *__restrict__ ws, int C, int HW, int parts, int vec, double eps,
                    double decay, float *__restrict__ y, float *__restrict__ save_mean, float *__restrict__ save_rstd,
                    float *__restrict__ running_mean, float *__restrict__ running_var) {
    const int part = blockIdx.y;
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        double S, Q;
        bn_sum_parts(ws + 2 * (size_t)c * parts, parts, S, Q);
        const double m = (double)HW, mean = S / m;
        double var = Q / m - mean * mean;                              // biased (Chainer's x.var(axis)); >= 0 up to rounding
        if (var < 0.0) var = 0.0;
        const double rstd = 1.0 / sqrt(var + eps);
        BnFwdScalars k;
        k.mean = mean;
        k.rstd = (float)rstd;
        k.gamma = gamma[c];
        k.beta = beta[c];
        if (part == 0 && threadIdx.x == 0) {
            save_mean[c] = (float)mean;
            save_rstd[c] = k.rstd;
            if (running_mean) running_mean[c] = (float)(decay * (double)running_mean[c] + (1.0 - decay) * mean);
            if (running_var) {
                const double adjust = m / (m - 1.0 > 1.0 ? m - 1.0 : 1.0);
                running_var[c] = (float)(decay * (double)running_var[c] + (1.0 - decay) * adjust * (var + eps));
            }
        }
        const size_t row = (size_t)c * HW;
        const float *p = z + row, *r = RES ? residual + row : nullptr;
        float *o = y + row;
        const BnSlice sl = bn_slice(p, HW, parts, part, vec);
        for (int i = sl.begin + threadIdx.x; i < sl.begin + sl.head; i += 256) o[i] = bn_fwd_one<RELU, RES>(p[i], RES ? r[i] : 0.0f, k);
        const int mid = sl.begin + sl.head;
        const float4 *p4 = reinterpret_cast<const float4 *>(p + mid), *r4 = reinterpret_cast<const float4 *>(RES ? r + mid : p + mid);
        float4 *o4 = reinterpret_cast<float4 *>(o + mid);
        int i = threadIdx.x;
        for (; i + 256 < sl.n4; i += 512) {                           // two vectors of every operand in flight per thread
            float4 a0 = p4[i], a1 = p4[i + 256], b0 = a0, b1 = a1;
            if (RES) { b0 = r4[i]; b1 = r4[i + 256]; frcnn_pin(b0); frcnn_pin(b1); }
            frcnn_pin(a0); frcnn_pin(a1);
            o4[i] = make_float4(bn_fwd_one<RELU, RES>(a0.x, b0.x, k), bn_fwd_one<RELU, RES>(a0.y, b0.y, k), bn_fwd_one<RELU, RES>(a0.z, b0.z, k),
                                bn_fwd_one<RELU, RES>(a0.w, b0.w, k));
            o4[i + 256] = make_float4(bn_fwd_one<RELU, RES>(a1.x, b1.x, k), bn_fwd_one<RELU, RES>(a1.y, b1.y, k),
                                      bn_fwd_one<RELU, RES>(a1.z, b1.z, k), bn_fwd_one<RELU, RES>(a1.w, b1.w, k));
        }
        for (; i < sl.n4; i += 256) {
            const float4 a0 = p4[i], b0 = RES ? r4[i] : a0;
            o4[i] = make_float4(bn_fwd_one<RELU, RES>(a0.x, b0.x, k), bn_fwd_one<RELU, RES>(a0.y, b0.y, k), bn_fwd_one<RELU, RES>(a0.z, b0.z, k),
                                bn_fwd_one<RELU, RES>(a0.w, b0.w, k));
        }
        for (int j = mid + 4 * sl.n4 + threadIdx.x; j < sl.end; j += 256) o[j] = bn_fwd_one<RELU, RES>(p[j], RES ? r[j] : 0.0f, k);
    }
}

// ---- backward, launch 1: sum g and sum g * xhat of a slice (g = dy where y > 0) --------------------------
template <bool MASK>
__device__ __forceinline__ void bn_bwd_acc(float dy, float y, float z, float mean, float rstd, double &s, double &q) {
    const float g = (!MASK || y > 0.0f) ? dy : 0.0f;
    const float xhat = (z - mean) * rstd;
    s += (double)g;
    q += (double)g * (double)xhat;
}

template <bool MASK>
__global__ void __launch_bounds__(256)
bn_bwd_stats_kernel(const float *__restrict__ dy, const float *__restrict__ y, const float *__restrict__ z, const float *__restrict__ save_mean,
                    const float *__restrict__ save_rstd, int C, int HW, int parts, int vec, double *__restrict__ ws) {
    const int part = blockIdx.y;
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        const size_t row = (size_t)c * HW;
        const float *pd = dy + row, *pz = z + row, *py = MASK ? y + row : pd;
        const float mean = save_mean[c], rstd = save_rstd[c];
        const BnSlice sl = bn_slice(pz, HW, parts, part, vec);
        double s = 0.0, q = 0.0, s1 = 0.0, q1 = 0.0;
        for (int i = sl.begin + threadIdx.x; i < sl.begin + sl.head; i += 256) bn_bwd_acc<MASK>(pd[i], py[i], pz[i], mean, rstd, s, q);
        const int mid = sl.begin + sl.head;
        const float4 *d4 = reinterpret_cast<const float4 *>(pd + mid), *z4 = reinterpret_cast<const float4 *>(pz + mid),
                     *y4 = reinterpret_cast<const float4 *>(py + mid);
        int i = threadIdx.x;
        for (; i + 256 < sl.n4; i += 512) {                           // two vectors of every operand in flight per thread
            float4 a0 = d4[i], a1 = d4[i + 256], b0 = z4[i], b1 = z4[i + 256], c0 = a0, c1 = a1;
            if (MASK) { c0 = y4[i]; c1 = y4[i + 256]; frcnn_pin(c0); frcnn_pin(c1); }
            frcnn_pin(a0); frcnn_pin(a1); frcnn_pin(b0); frcnn_pin(b1);
            bn_bwd_acc<MASK>(a0.x, c0.x, b0.x, mean, rstd, s, q);
            bn_bwd_acc<MASK>(a0.y, c0.y, b0.y, mean, rstd, s, q);
            bn_bwd_acc<MASK>(a0.z, c0.z, b0.z, mean, rstd, s, q);
            bn_bwd_acc<MASK>(a0.w, c0.w, b0.w, mean, rstd, s, q);
            bn_bwd_acc<MASK>(a1.x, c1.x, b1.x, mean, rstd, s1, q1);
            bn_bwd_acc<MASK>(a1.y, c1.y, b1.y, mean, rstd, s1, q1);
            bn_bwd_acc<MASK>(a1.z, c1.z, b1.z, mean, rstd, s1, q1);
            bn_bwd_acc<MASK>(a1.w, c1.w, b1.w, mean, rstd, s1, q1);
        }
        for (; i < sl.n4; i += 256) {
            const float4 a0 = d4[i], b0 = z4[i], c0 = MASK ? y4[i] : a0;
            bn_bwd_acc<MASK>(a0.x, c0.x, b0.x, mean, rstd, s, q);
            bn_bwd_acc<MASK>(a0.y, c0.y, b0.y, mean, rstd, s, q);
            bn_bwd_acc<MASK>(a0.z, c0.z, b0.z, mean, rstd, s, q);
            bn_bwd_acc<MASK>(a0.w, c0.w, b0.w, mean, rstd, s, q);
        }
        s += s1;
        q += q1;
        for (int j = mid + 4 * sl.n4 + threadIdx.x; j < sl.end; j += 256) bn_bwd_acc<MASK>(pd[j], py[j], pz[j], mean, rstd, s, q);
        bn_block_sum2(s, q);
        if (threadIdx.x == 0) {
            ws[2 * ((size_t)c * parts + part)] = s;
            ws[2 * ((size_t)c * parts + part) + 1] = q;
        }
    }
}

// ---- backward, launch 2: dbeta, dgamma from the partial sums, then dz (and dres = g) over the slice ------
struct BnBwdScalars { float mean, rstd, scale, a, b; };       // scale = gamma * rstd, a = dbeta / m, b = dgamma / m

template <bool MASK, bool DRES>
__device__ __forceinline__ float bn_bwd_one(float dy, float y, float z, const BnBwdScalars &k, float &g) {
    g = (!MASK || y > 0.0f) ? dy : 0.0f;
    const float xhat = (z - k.mean) * k.rstd;
    return k.scale * ((g - k.a) - xhat * k.b);
}

template <bool MASK, bool DRES>
__global__ void __launch_bounds__(256)
bn_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ y, const float *__restrict__ z, const float *__restrict__ gamma,
                    const float *__restrict__ save_mean, const float *__restrict__ save_rstd, const double *__restrict__ ws, int C, int HW,
                    int parts, int vec, float *__restrict__ dz, float *__restrict__ dgamma, float *__restrict__ dbeta, float *__restrict__ dres) {
    const int part = blockIdx.y;
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        double S, Q;
        bn_sum_parts(ws + 2 * (size_t)c * parts, parts, S, Q);
        BnBwdScalars k;
        k.mean = save_mean[c];
        k.rstd = save_rstd[c];
        k.scale = gamma[c] * k.rstd;
        k.a = (float)(S / (double)HW);
        k.b = (float)(Q / (double)HW);
        if (part == 0 && threadIdx.x == 0) {
            dbeta[c] = (float)S;
            dgamma[c] = (float)Q;
        }
        const size_t row = (size_t)c * HW;
        const float *pd = dy + row, *pz = z + row, *py = MASK ? y + row : pd;
        float *o = dz + row, *r = DRES ? dres + row : nullptr;
        const BnSlice sl = bn_slice(pz, HW, parts, part, vec);
        float g;
        for (int i = sl.begin + threadIdx.x; i < sl.begin + sl.head; i += 256) {
            o[i] = bn_bwd_one<MASK, DRES>(pd[i], py[i], pz[i], k, g);
            if (DRES) r[i] = g;
        }
        const int mid = sl.begin + sl.head;
        const float4 *d4 = reinterpret_cast<const float4 *>(pd + mid), *z4 = reinterpret_cast<const float4 *>(pz + mid),
                     *y4 = reinterpret_cast<const float4 *>(py + mid);
        float4 *o4 = reinterpret_cast<float4 *>(o + mid), *r4 = reinterpret_cast<float4 *>(DRES ? r + mid : o + mid);
        int i = threadIdx.x;
        for (; i + 256 < sl.n4; i += 512) {                           // two vectors of every operand in flight per thread
            float4 a0 = d4[i], a1 = d4[i + 256], b0 = z4[i], b1 = z4[i + 256], c0 = a0, c1 = a1, v, gg;
            if (MASK) { c0 = y4[i]; c1 = y4[i + 256]; frcnn_pin(c0); frcnn_pin(c1); }
            frcnn_pin(a0); frcnn_pin(a1); frcnn_pin(b0); frcnn_pin(b1);
            v.x = bn_bwd_one<MASK, DRES>(a0.x, c0.x, b0.x, k, gg.x);
            v.y = bn_bwd_one<MASK, DRES>(a0.y, c0.y, b0.y, k, gg.y);
            v.z = bn_bwd_one<MASK, DRES>(a0.z, c0.z, b0.z, k, gg.z);
            v.w = bn_bwd_one<MASK, DRES>(a0.w, c0.w, b0.w, k, gg.w);
            o4[i] = v;
            if (DRES) r4[i] = gg;
            v.x = bn_bwd_one<MASK, DRES>(a1.x, c1.x, b1.x, k, gg.x);
            v.y = bn_bwd_one<MASK, DRES>(a1.y, c1.y, b1.y, k, gg.y);
            v.z = bn_bwd_one<MASK, DRES>(a1.z, c1.z, b1.z, k, gg.z);
            v.w = bn_bwd_one<MASK, DRES>(a1.w, c1.w, b1.w, k, gg.w);
            o4[i + 256] = v;
            if (DRES) r4[i + 256] = gg;
        }
        for (; i < sl.n4; i += 256) {
            const float4 a0 = d4[i], b0 = z4[i], c0 = MASK ? y4[i] : a0;
            float4 v, gg;
            v.x = bn_bwd_one<MASK, DRES>(a0.x, c0.x, b0.x, k, gg.x);
            v.y = bn_bwd_one<MASK, DRES>(a0.y, c0.y, b0.y, k, gg.y);
            v.z = bn_bwd_one<MASK, DRES>(a0.z, c0.z, b0.z, k, gg.z);
            v.w = bn_bwd_one<MASK, DRES>(a0.w, c0.w, b0.w, k, gg.w);
            o4[i] = v;
            if (DRES) r4[i] = gg;
        }
        for (int j = mid + 4 * sl.n4 + threadIdx.x; j < sl.end; j += 256) {
            o[j] = bn_bwd_one<MASK, DRES>(pd[j], py[j], pz[j], k, g);
            if (DRES) r[j] = g;
        }
    }
}

// ---- adjoint of frcnn_maxpool3x3s2_f32, gather form: one thread per INPUT pixel -------------------------
// Window (oh, ow) covers rows 2*oh .. 2*oh+2 and columns 2*ow .. 2*ow+2, clipped at the bottom and right edges (cover_all).  A pixel lies
// in at most two windows per axis; it receives a window's dy when it is that window's FIRST maximum in row-major order (Chainer's and
// torch's rule).  Windows are visited in ascending (oh, ow): the order in which a scatter over the outputs would add.
__global__ void __launch_bounds__(256)
maxpool3x3s2_bwd_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ dx, int C, int H, int W, int OH, int OW) {
    const size_t total = (size_t)C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ix = (int)(i % W), iy = (int)((i / W) % H), c = (int)(i / ((size_t)W * H));
        const float *p = x + (size_t)c * H * W;
        const float *g = dy + (size_t)c * OH * OW;
        const float mine = p[(size_t)iy * W + ix];
        const int oh0 = iy >= 2 ? (iy - 1) / 2 : 0, oh1 = min(OH - 1, iy / 2);
        const int ow0 = ix >= 2 ? (ix - 1) / 2 : 0, ow1 = min(OW - 1, ix / 2);
        float acc = 0.0f;
        for (int oh = oh0; oh <= oh1; ++oh)
            for (int ow = ow0; ow <= ow1; ++ow) {
                // the pixel wins the window when nothing before it (row-major) is >= it and nothing after it is > it
                bool win = true;
                for (int dyy = 0; dyy < 3; ++dyy)
                    for (int dxx = 0; dxx < 3; ++dxx) {
                        const int yy = 2 * oh + dyy, xx = 2 * ow + dxx;
                        if (yy >= H || xx >= W) continue;
                        const float v = p[(size_t)yy * W + xx];
                        const bool before = yy < iy || (yy == iy && xx < ix);
                        if (before ? v >= mine : v > mine) win = false;
                    }
                if (win) acc += g[(size_t)oh * OW + ow];
            }
        dx[i] = acc;
    }
}

// ---- adjoint of frcnn_subsample2_f32: zero-stuffing, every element of dx written by this launch -------
__global__ void __launch_bounds__(256)
subsample2_bwd_kernel(const float *__restrict__ dy, float *__restrict__ dx, int C, int H, int W, int OH, int OW) {
    const size_t total = (size_t)C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ix = (int)(i % W), iy = (int)((i / W) % H), c = (int)(i / ((size_t)W * H));
        dx[i] = ((ix | iy) & 1) ? 0.0f : dy[((size_t)c * OH + (iy >> 1)) * OW + (ix >> 1)];
    }
}

// every operand of a launch walks the same element offsets: the vector path needs them to agree modulo 16 bytes (NULL operands do not count)
int bn_same_alignment(std::initializer_list<const void *> ptrs) {
    uintptr_t ref = 16;
    for (const void *p : ptrs) {
        if (!p) continue;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p) & 15;
        if (a & 3) return 0;
        if (ref == 16) ref = a;
        else if (a != ref) return 0;
    }
    return 1;
}

}  // namespace

size_t frcnn_bn_workspace_bytes(int C, int HW) {
    if (C < 1 || HW < 1) return 0;
    return frcnn_align256((size_t)C * bn_parts(C, HW) * 2 * sizeof(double));
}

int frcnn_bn_train_fwd_f32(const float *z, const float *gamma, const float *beta, const float *residual, int relu, int C, int HW, double eps,
                           double decay, float *y, float *save_mean, float *save_rstd, float *running_mean, float *running_var, void *workspace,
                           size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!z || !gamma || !beta || !y || !save_mean || !save_rstd || C < 1 || HW < 1 || !(eps >= 0.0) || !(decay >= 0.0) || !(decay <= 1.0))
        return FRCNN_ERR_INVALID;
    const int parts = bn_parts(C, HW);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < (size_t)C * parts * 2 * sizeof(double)) return FRCNN_ERR_INVALID;
    const int vec = bn_same_alignment({z, y, residual});
    const dim3 grid(C < kBnMaxGridC ? C : kBnMaxGridC, parts);
    double *ws = (double *)workspace;
    hipLaunchKernelGGL(bn_fwd_stats_kernel, grid, dim3(256), 0, stream, z, C, HW, parts, vec, ws);
#define BN_FWD(RELU, RES)                                                                                                                      \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(bn_fwd_apply_kernel<RELU, RES>), grid, dim3(256), 0, stream, z, gamma, beta, residual, (const double *)ws, C, HW, \
                       parts, vec, eps, decay, y, save_mean, save_rstd, running_mean, running_var)
    if (relu && residual) BN_FWD(true, true);
    else if (relu) BN_FWD(true, false);
    else if (residual) BN_FWD(false, true);
    else BN_FWD(false, false);
#undef BN_FWD
    return frcnn_launch_status();
}

int frcnn_bn_train_bwd_f32(const float *dy, const float *y, const float *z, const float *gamma, const float *save_mean, const float *save_rstd, int C,
                           int HW, float *dz, float *dgamma, float *dbeta, float *dres, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dy || !z || !gamma || !save_mean || !save_rstd || !dz || !dgamma || !dbeta || C < 1 || HW < 1) return FRCNN_ERR_INVALID;
    const int parts = bn_parts(C, HW);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < (size_t)C * parts * 2 * sizeof(double)) return FRCNN_ERR_INVALID;
    const int vec = bn_same_alignment({dy, y, z, dz, dres});
    const dim3 grid(C < kBnMaxGridC ? C : kBnMaxGridC, parts);
    double *ws = (double *)workspace;
    if (y) hipLaunchKernelGGL(HIP_KERNEL_NAME(bn_bwd_stats_kernel<true>), grid, dim3(256), 0, stream, dy, y, z, save_mean, save_rstd, C, HW, parts, vec, ws);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(bn_bwd_stats_kernel<false>), grid, dim3(256), 0, stream, dy, y, z, save_mean, save_rstd, C, HW, parts, vec, ws);
#define BN_BWD(MASK, DRES)                                                                                                                     \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(bn_bwd_apply_kernel<MASK, DRES>), grid, dim3(256), 0, stream, dy, y, z, gamma, save_mean, save_rstd,    \
                       (const double *)ws, C, HW, parts, vec, dz, dgamma, dbeta, dres)
    if (y && dres) BN_BWD(true, true);
    else if (y) BN_BWD(true, false);
    else if (dres) BN_BWD(false, true);
    else BN_BWD(false, false);
#undef BN_BWD
    return frcnn_launch_status();
}

int frcnn_maxpool3x3s2_bwd_f32(const float *x, const float *dy, float *dx, int C, int H, int W, void *stream) {
    if (!x || !dy || !dx || C < 1 || H < 1 || W < 1) return FRCNN_ERR_INVALID;
    const int OH = H >= 2 ? (H - 2) / 2 + 1 : 1, OW = W >= 2 ? (W - 2) / 2 + 1 : 1;
    const size_t total = (size_t)C * H * W;                       // one thread per input pixel
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, dy, dx, C, H, W, OH, OW);
    return frcnn_launch_status();
}

int frcnn_subsample2_bwd_f32(const float *dy, float *dx, int C, int H, int W, void *stream) {
    if (!dy || !dx || C < 1 || H < 1 || W < 1) return FRCNN_ERR_INVALID;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const size_t total = (size_t)C * H * W;
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(subsample2_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, dx, C, H, W, OH, OW);
    return frcnn_launch_status();
}
