// linear_train_bf16.hip -- the three matrix products of an L.Linear in the mixed-precision stage-2 step (RCNNTrainer(precision="bf16" / "f16")): forward,
// input gradient and weight gradient of fc6 / fc7 / cls_score / bbox_pred (models/faster_rcnn.py:33-36,127-134) on 16-bit operands with fp32 accumulation.
// Every operand is an fp32 array (activations, upstream gradients, the fp32 MASTER weights) and is rounded to nearest even WHILE IT IS STAGED: a 16-bit copy
// of fc6's 411 MB weight matrix is never written to memory (the step reads the fp32 weights twice and writes the fp32 gradient once).
//
// One kernel, three operand orientations.  D(rows, cols) = sum over `red` of A(row, red) * B(col, red); a workgroup (four waves) owns BM = 32 MT rows and 128
// columns and walks the reduction axis in chunks of 64.  A chunk sits in LDS as two tiles of 16-bit values, [tile row][64 red], pitch 128 bytes, the 16-byte
// group g of row r in slot g ^ ((r >> 1) & 7) ^ ((r >> 4) & 3), so that a wave's fragment reads (32 consecutive rows, one group) and both kinds of staging
// writes below spread over the banks.  Staging is through registers, double buffered: the global loads of chunk c + 1 are issued before the MFMAs of chunk c
// and converted / deposited after them, one barrier per chunk.
//   row-major operand  (source [tile row][red], red contiguous: x and W of the forward product, dy of the input gradient): a thread loads four consecutive
//                      red values of one row, packs them (frcnn_pack_bf16x2) and writes 8 bytes;
//   transposed operand (source [red][tile row], tile row contiguous: W AS STORED in the input gradient, dy and x in the weight gradient): a thread loads an
//                      8 (red) x 4 (rows) block as eight 16-byte loads and writes four 16-byte groups -- the transpose happens in registers, each weight
//                      byte is read once as part of a 512-byte run, and no transposed copy of anything exists.
// A wave owns 32 columns and all MT row tiles: MT accumulators of 16 registers.  The MFMA's operands are swapped (A = the column fragment), so the
// accumulator tile is transposed -- lane = output row, four consecutive registers = four consecutive columns -- and leaves as 16-byte stores.
//   forward / input gradient: split over the reduction axis into slabs [split][rows][ldp] in the caller's workspace (ldp = cols rounded up to 4), summed IN
//                             SPLIT ORDER by linear_train_reduce_kernel (bias, ReLU): no atomics, two runs give identical bits;
//   weight gradient:          the reduction axis is the M <= 320 rows of the mini-batch (at most five chunks): no split, the tile goes straight into dW.
// Budgets (hipcc -S, asserted in tests/test_rcnn16_train_emulated.py): no scratch; MT = 10 / 4 / 1 use 114688 / 65536 / 40960 bytes of LDS
// (2 stages x (32 MT + 128) rows x 128 B); the largest form (MT = 10: 160 accumulators + 28 staged float4) stays below 512 registers at one wave per SIMD.
#include "frcnn_common.h"
#include "frcnn_reduce.h"
#include <frcnn_buffer.h>
#include <frcnn_intrin.h>

namespace {

constexpr int kTK = 64;                  // reduction values per chunk
constexpr int kTBN = 128;                // output columns per workgroup
constexpr int kTPitch = 128;             // bytes per tile row: 64 16-bit values

typedef float lt_f4 __attribute__((ext_vector_type(4)));      // a staged quad (element access stays in registers)

__device__ __forceinline__ uint32_t lt_slot(int row, int g) { return (uint32_t)((g ^ ((row >> 1) & 7) ^ ((row >> 4) & 3)) << 4); }

// elements [line][pos .. pos + 3] of an (nlines, ld) fp32 matrix; zeros outside it.  AL: ld % 4 == 0 and pos % 4 == 0 -- one 16-byte load, wholly
// inside a line or wholly outside; otherwise four 4-byte loads with a range test each (cls_score / bbox_pred: rows of 21 and 84 floats).
template <bool AL>
__device__ __forceinline__ lt_f4 lt_load4(frcnn_buf_t buf, int line, int pos, int nlines, int ld) {
    const bool in = line >= 0 && line < nlines;
    if constexpr (AL) {
        const float4 f = frcnn_buf_load_f32x4(buf, (in && pos < ld) ? (uint32_t)(line * ld + pos) * 4u : kBufOob);
        return lt_f4{f.x, f.y, f.z, f.w};
    }
    const uint32_t base = (uint32_t)(line * ld + pos) * 4u;
    const float v0 = frcnn_buf_load_f32(buf, (in && pos < ld) ? base : kBufOob);
    const float v1 = frcnn_buf_load_f32(buf, (in && pos + 1 < ld) ? base + 4u : kBufOob);
    const float v2 = frcnn_buf_load_f32(buf, (in && pos + 2 < ld) ? base + 8u : kBufOob);
    const float v3 = frcnn_buf_load_f32(buf, (in && pos + 3 < ld) ? base + 12u : kBufOob);
    return lt_f4{v0, v1, v2, v3};
}

// float4 a thread stages per chunk for a tile of ROWS rows
template <int ROWS, bool T>
struct LtStage { static constexpr int NQ = T ? 8 * ((2 * ROWS + 255) / 256) : ROWS / 16; };

// fetch this thread's share of chunk [k0, k0 + 64) of the tile whose first row is r0.  Row-major: the matrix is (nrows, ld = reduction length);
// transposed: the matrix is (nred, ld = row count).
template <int ROWS, bool T, bool AL, int NQ>
__device__ __forceinline__ void lt_fetch(lt_f4 (&v)[NQ], frcnn_buf_t buf, int tid, int r0, int k0, int nlines, int ld) {
    if constexpr (!T) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = tid + 256 * q, row = idx >> 4, c4 = idx & 15;
            v[q] = lt_load4<AL>(buf, r0 + row, k0 + 4 * c4, nlines, ld);
        }
    } else {
        constexpr int CQ = ROWS / 4;                                       // 4-row quads of the tile; a block = 8 red x one quad
#pragma unroll
        for (int b = 0; b < NQ / 8; ++b) {
            const int blk = tid + 256 * b, cq = blk % CQ, rg = blk / CQ;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[b * 8 + i] = lt_load4<AL>(buf, rg < 8 ? k0 + 8 * rg + i : -1, r0 + 4 * cq, nlines, ld);
        }
    }
}

// column U of an 8 (red) x 4 (rows) block -> the 16 bytes of tile row U, as two 8-byte writes
template <int U>
__device__ __forceinline__ void lt_put8(unsigned char *dst, const lt_f4 &v0, const lt_f4 &v1, const lt_f4 &v2, const lt_f4 &v3, const lt_f4 &v4,
                                        const lt_f4 &v5, const lt_f4 &v6, const lt_f4 &v7) {
    *reinterpret_cast<uint2 *>(dst) = make_uint2(frcnn_pack_bf16x2(v0[U], v1[U]), frcnn_pack_bf16x2(v2[U], v3[U]));
    *reinterpret_cast<uint2 *>(dst + 8) = make_uint2(frcnn_pack_bf16x2(v4[U], v5[U]), frcnn_pack_bf16x2(v6[U], v7[U]));
}

// round to the translation unit's 16-bit format and write the tile image
template <int ROWS, bool T, int NQ>
__device__ __forceinline__ void lt_deposit(const lt_f4 (&v)[NQ], unsigned char *tile, int tid) {
    if constexpr (!T) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = tid + 256 * q, row = idx >> 4, c4 = idx & 15;
            const uint2 p = make_uint2(frcnn_pack_bf16x2(v[q][0], v[q][1]), frcnn_pack_bf16x2(v[q][2], v[q][3]));
            *reinterpret_cast<uint2 *>(tile + row * kTPitch + lt_slot(row, c4 >> 1) + (c4 & 1) * 8) = p;
        }
    } else {
        constexpr int CQ = ROWS / 4;
#pragma unroll
        for (int b = 0; b < NQ / 8; ++b) {
            const int blk = tid + 256 * b, cq = blk % CQ, rg = blk / CQ;
            if (rg < 8) {
                const int row = 4 * cq;
                lt_put8<0>(tile + (row + 0) * kTPitch + lt_slot(row + 0, rg), v[b * 8], v[b * 8 + 1], v[b * 8 + 2], v[b * 8 + 3], v[b * 8 + 4], v[b * 8 + 5], v[b * 8 + 6], v[b * 8 + 7]);
                lt_put8<1>(tile + (row + 1) * kTPitch + lt_slot(row + 1, rg), v[b * 8], v[b * 8 + 1], v[b * 8 + 2], v[b * 8 + 3], v[b * 8 + 4], v[b * 8 + 5], v[b * 8 + 6], v[b * 8 + 7]);
                lt_put8<2>(tile + (row + 2) * kTPitch + lt_slot(row + 2, rg), v[b * 8], v[b * 8 + 1], v[b * 8 + 2], v[b * 8 + 3], v[b * 8 + 4], v[b * 8 + 5], v[b * 8 + 6], v[b * 8 + 7]);
                lt_put8<3>(tile + (row + 3) * kTPitch + lt_slot(row + 3, rg), v[b * 8], v[b * 8 + 1], v[b * 8 + 2], v[b * 8 + 3], v[b * 8 + 4], v[b * 8 + 5], v[b * 8 + 6], v[b * 8 + 7]);
            }
        }
    }
}

// part[split][rows][ldp] (+)= A B^T over this split's chunks.  a_lines / b_lines: the number of lines of the source matrices (rows or red, by orientation).
// AAL: A's leading dimension is a multiple of 4 (16-byte loads); B's always is (the hosts require K % 4 == 0)
template <int MT, bool AT, bool BT, bool AAL>
__global__ void __launch_bounds__(256)
linear_train_kernel(const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ part, int rows, int cols, int red, int lda, int ldb,
                    int ldp, int splits, int cps) {
    constexpr int BM = 32 * MT;
    constexpr int ABYTES = BM * kTPitch, BBYTES = kTBN * kTPitch, STAGE = ABYTES + BBYTES;
    constexpr int AQ = LtStage<BM, AT>::NQ, BQ = LtStage<kTBN, BT>::NQ;
    static_assert(2 * STAGE <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int split = (int)blockIdx.x % splits, cb = (int)blockIdx.x / splits;
    const int r0 = (int)blockIdx.y * BM, c0 = cb * kTBN;
    const int nch_all = (red + kTK - 1) / kTK;
    const int c_begin = split * cps;
    const int nch = min(nch_all, c_begin + cps) - c_begin;                  // >= 1 (host)
    const int a_lines = AT ? red : rows, b_lines = BT ? red : cols;
    const frcnn_buf_t abuf = frcnn_make_buf(A, (uint32_t)((size_t)a_lines * lda * 4));
    const frcnn_buf_t bbuf = frcnn_make_buf(B, (uint32_t)((size_t)b_lines * ldb * 4));

    frcnn_f32x16 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    lt_f4 va[AQ], vb[BQ];
    lt_fetch<BM, AT, AAL, AQ>(va, abuf, tid, r0, c_begin * kTK, a_lines, lda);
    lt_fetch<kTBN, BT, true, BQ>(vb, bbuf, tid, c0, c_begin * kTK, b_lines, ldb);
    lt_deposit<BM, AT, AQ>(va, lds, tid);
    lt_deposit<kTBN, BT, BQ>(vb, lds + ABYTES, tid);
    __syncthreads();

    const int brow = wave * 32 + l31;
    for (int c = 0; c < nch; ++c) {
        const unsigned char *st = lds + (c & 1) * STAGE;
        unsigned char *nx = lds + ((c + 1) & 1) * STAGE;
        const bool more = c + 1 < nch;                                      // workgroup-uniform
        if (more) {
            lt_fetch<BM, AT, AAL, AQ>(va, abuf, tid, r0, (c_begin + c + 1) * kTK, a_lines, lda);
            lt_fetch<kTBN, BT, true, BQ>(vb, bbuf, tid, c0, (c_begin + c + 1) * kTK, b_lines, ldb);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int g = 2 * ks + khalf;
            const uint4 fb = *reinterpret_cast<const uint4 *>(st + ABYTES + brow * kTPitch + lt_slot(brow, g));
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int arow = i * 32 + l31;
                const uint4 fa = *reinterpret_cast<const uint4 *>(st + arow * kTPitch + lt_slot(arow, g));
                acc[i] = frcnn_mfma_32x32x16_bf16(fb, fa, acc[i]);         // operands swapped: lane = output row, registers = columns
            }
        }
        if (more) {
            lt_deposit<BM, AT, AQ>(va, nx, tid);
            lt_deposit<kTBN, BT, BQ>(vb, nx + ABYTES, tid);
        }
        __syncthreads();
    }

    // lane = output row r0 + 32 i + l31; registers 4 g .. 4 g + 3 = columns c0 + 32 wave + 8 g + 4 khalf .. + 3 (ldp % 4 == 0: a quad is inside the slab row or
    // outside); rows past `rows` and columns past ldp get an out-of-range offset and store nothing
    const frcnn_buf_t pbuf = frcnn_make_buf(part + (size_t)split * rows * ldp, (uint32_t)((size_t)rows * ldp * 4));
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = r0 + i * 32 + l31;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = c0 + wave * 32 + 8 * g + 4 * khalf;
            const uint32_t off = (m < rows && n < ldp) ? (uint32_t)(m * ldp + n) * 4u : kBufOob;
            frcnn_buf_store_f32x4_soff<0>(pbuf, off, 0u, make_float4(acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]));
        }
    }
}

// y(M, N) = act(sum over splits, in split order, of part[split][M][ldp] + bias)
__global__ void __launch_bounds__(256)
linear_train_reduce_kernel(const float *__restrict__ part, const float *__restrict__ bias, float *__restrict__ y, int M, int N, int ldp, int splits, int relu) {
    const size_t total = (size_t)M * N, slab = (size_t)M * ldp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t m = i / N, n = i % N;
        float v = frcnn_sum_splits(part, slab, m * ldp + n, splits);
        if (bias) v += bias[n];
        if (relu) v = fmaxf(v, 0.0f);
        y[i] = v;
    }
}

struct LtPlan { int mt, rowblocks, colblocks, splits, cps, ldp; };
static LtPlan lt_plan(int rows, int cols, int red, bool may_split) {
    LtPlan p;
    p.mt = rows > 128 ? 10 : (rows > 32 ? 4 : 1);
    p.rowblocks = frcnn_cdiv(rows, 32 * p.mt);
    p.colblocks = frcnn_cdiv(cols, kTBN);
    p.ldp = (cols + 3) & ~3;
    const int nch = frcnn_cdiv(red, kTK);
    int splits = 1;
    if (may_split) {
        splits = frcnn_cu_count() / (p.rowblocks * p.colblocks);
        if (splits > nch / 2) splits = nch / 2;                           // a split is at least two chunks long
        const int forced = frcnn_tune_int("FRCNN_LINEAR_TRAIN_SPLITS", 0);   // A/B and test hook: the number of slabs
        if (forced > 0) splits = forced;
        if (splits > 64) splits = 64;
        if (splits > nch) splits = nch;
        if (splits < 1) splits = 1;
    }
    p.cps = frcnn_cdiv(nch, splits);
    p.splits = frcnn_cdiv(nch, p.cps);
    return p;
}

static bool lt_fits(size_t a, size_t b, size_t c) { return a * 4 < (1ull << 31) && b * 4 < (1ull << 31) && c * 4 < (1ull << 31); }

template <bool AT, bool BT>
static void lt_launch(const LtPlan &p, const float *A, const float *B, float *part, int rows, int cols, int red, int lda, int ldb, int ldp, hipStream_t stream) {
    const dim3 grid(p.colblocks * p.splits, p.rowblocks);
#define LT_LAUNCH(MT_) do { \
        if ((lda & 3) == 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(linear_train_kernel<MT_, AT, BT, true>), grid, dim3(256), 0, stream, A, B, part, rows, cols, red, lda, ldb, ldp, p.splits, p.cps); \
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(linear_train_kernel<MT_, AT, BT, false>), grid, dim3(256), 0, stream, A, B, part, rows, cols, red, lda, ldb, ldp, p.splits, p.cps); } while (0)
    if constexpr (AT) {                                                    // (a transposed A tile is staged in whole 256-thread passes: 128 or 32 rows)
        if (p.mt == 1) LT_LAUNCH(1);
        else LT_LAUNCH(4);
    } else {
        if (p.mt == 10) LT_LAUNCH(10);
        else if (p.mt == 4) LT_LAUNCH(4);
        else LT_LAUNCH(1);
    }
#undef LT_LAUNCH
}

static void lt_reduce(const LtPlan &p, const float *part, const float *bias, float *y, int M, int N, int relu, hipStream_t stream) {
    const size_t total = (size_t)M * N;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(linear_train_reduce_kernel, dim3(blocks), dim3(256), 0, stream, part, bias, y, M, N, p.ldp, p.splits, relu);
}

}  // namespace

extern "C" {

size_t frcnn_linear_bf16_train_workspace_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    const LtPlan p = lt_plan(M, N, K, true);
    return frcnn_align256((size_t)p.splits * M * p.ldp * sizeof(float));
}

int frcnn_linear_bf16_train(const float *x, const float *w, const float *bias, float *y, int M, int N, int K, int relu, void *workspace,
                            size_t workspace_bytes, void *stream) {
    if (!x || !w || !y || M < 1 || N < 1 || K < 1) return FRCNN_ERR_INVALID;
    if ((K & 3) != 0) return FRCNN_ERR_UNSUPPORTED;                       // rows of x and W are read 16 bytes at a time
    const LtPlan p = lt_plan(M, N, K, true);
    if (!lt_fits((size_t)M * K, (size_t)N * K, (size_t)M * p.ldp)) return FRCNN_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < (size_t)p.splits * M * p.ldp * sizeof(float)) return FRCNN_ERR_INVALID;
    lt_launch<false, false>(p, x, w, (float *)workspace, M, N, K, K, K, p.ldp, (hipStream_t)stream);
    lt_reduce(p, (const float *)workspace, bias, y, M, N, relu, (hipStream_t)stream);
    return frcnn_launch_status();
}

size_t frcnn_linear_dgrad_bf16_workspace_bytes(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    const LtPlan p = lt_plan(M, K, N, true);
    return frcnn_align256((size_t)p.splits * M * p.ldp * sizeof(float));
}

int frcnn_linear_dgrad_bf16(const float *dy, const float *w, float *dx, int M, int N, int K, void *workspace, size_t workspace_bytes, void *stream) {
    if (!dy || !w || !dx || M < 1 || N < 1 || K < 1) return FRCNN_ERR_INVALID;
    if ((K & 3) != 0) return FRCNN_ERR_UNSUPPORTED;                       // W is read as stored, 16 bytes of a row at a time
    const LtPlan p = lt_plan(M, K, N, true);
    if (!lt_fits((size_t)M * N, (size_t)N * K, (size_t)M * p.ldp)) return FRCNN_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < (size_t)p.splits * M * p.ldp * sizeof(float)) return FRCNN_ERR_INVALID;
    lt_launch<false, true>(p, dy, w, (float *)workspace, M, K, N, N, K, p.ldp, (hipStream_t)stream);
    lt_reduce(p, (const float *)workspace, nullptr, dx, M, K, 0, (hipStream_t)stream);
    return frcnn_launch_status();
}

size_t frcnn_linear_wgrad_bf16_workspace_bytes(int M, int N, int K) {
    (void)M; (void)N; (void)K;
    return 0;                                                            // the weight gradient is written directly: no slabs
}

int frcnn_linear_wgrad_bf16(const float *dy, const float *x, float *dw, int M, int N, int K, void *workspace, size_t workspace_bytes, void *stream) {
    (void)workspace; (void)workspace_bytes;
    if (!dy || !x || !dw || M < 1 || N < 1 || K < 1) return FRCNN_ERR_INVALID;
    if ((K & 3) != 0) return FRCNN_ERR_UNSUPPORTED;                       // dW's rows are written 16 bytes at a time
    LtPlan p = lt_plan(N, K, M, false);
    if (p.mt == 10) { p.mt = 4; p.rowblocks = frcnn_cdiv(N, 128); }
    if (!lt_fits((size_t)M * N, (size_t)M * K, (size_t)N * K)) return FRCNN_ERR_UNSUPPORTED;
    lt_launch<true, true>(p, dy, x, dw, N, K, M, N, K, K, (hipStream_t)stream);
    return frcnn_launch_status();
}

}  // extern "C"
