// conv1x1_train_bf16.hip -- the 1x1 convolution of the ResNet trunk in training form on bf16 operands (ResNet(train_dtype="bf16"); the
// L.Convolution2D 1x1 forward / backward inside chainer's ResNetLayers, /root/reference/models/resnet.py:11-45): forward, input gradient and weight
// gradient as three GEMMs over the FLAT pixel axis of (C, HW) row-major fp32 maps, fp32 accumulation on v_mfma_f32_32x32x16_bf16.  Every operand is an
// fp32 array -- x, dz, the fp32 MASTER weights in pack_w's (Cin, Cout) layout -- and is rounded to nearest even WHILE IT IS STAGED (frcnn_pack_bf16x2),
// the form of linear_train_bf16.hip: no 16-bit copy of anything is written to memory, so a weight update needs no re-pack for these layers and the
// input gradient reads the very weights the forward pass read.
//
// One kernel, three operand orientations.  D(rows, cols) = sum over `red` of A(row, red) * B(col, red), cols contiguous in D:
//   forward          z [co][p]  : rows = Cout, cols = HW,   red = Cin;  A = W  as [red][row] (transposed source), B = x  as [red][col] (transposed source)
//   input gradient   dx[ci][p]  : rows = Cin,  cols = HW,   red = Cout; A = W  as [row][red] (row-major source),  B = dz as [red][col] (transposed source)
//   weight gradient  dW[ci][co] : rows = Cin,  cols = Cout, red = HW;   A = x  as [row][red] (row-major source),  B = dz as [col][red] (row-major source)
// A workgroup (four waves) owns 32 MT rows (MT = 2; 4 only for launches of more than eight 64-row tiles per CU) and 128 columns and walks the reduction axis in chunks of 64.  A chunk sits in
// LDS as two tiles of 16-bit values, [tile row][64 red], pitch 128 bytes, 16-byte group g of row r in slot g ^ ((r >> 1) & 7) ^ ((r >> 4) & 3)
// (linear_train_bf16.hip's image).  Staging goes through registers, double buffered, one barrier per chunk.  Every dimension is ragged and a row of a
// (C, HW) map is only 4-byte aligned (HW = 9375, 2394 ...), so EVERY global access is a 4-byte buffer access, arranged so that a wave-instruction
// covers whole lines:
//   transposed source: a thread owns one tile row and one group of 8 red values: eight loads, each of them 64 consecutive floats per wave (the tile-row
//                      axis is the contiguous one), one 16-byte LDS write -- the transpose happens in registers;
//   row-major source:  a thread owns four consecutive red values of one tile row: four loads (a wave covers 4 rows x 256 bytes, each line touched by
//                      the four of them), one 8-byte LDS write.
// Out-of-range rows, columns and reduction indices read zeros through the buffer descriptors' range check (an explicit kBufOob where the flat index
// would alias into the next line).  A wave owns 32 columns and all MT row tiles; register r of lane l of accumulator i is row 32 i + (r & 3) +
// 8 (r >> 2) + 4 (l >> 5), column l & 31: a store instruction writes two runs of 32 consecutive floats.
//
// K split.  Forward / input gradient (red <= 2048; few tiles on the small maps): in-launch, conv1x1_bf16_plan's contract -- a split publishes its
// accumulators as write-through 16-byte stores into its slot of the workspace, drains, takes a ticket on the tile's counter; the last arriver acquires
// once, resets the counter (the counter page is zeroed once by the caller and left zero by every launch) and adds ALL slots in split order, its own
// included, from memory: the bits do not depend on who arrives last.  Weight gradient (red = HW up to 150 000, 2 .. 256 tiles): split until the launch
// has two workgroups per CU; up to 16 pieces finish in the launch the same way, more of them (the layers with few tiles) each write a slab shaped
// like dW and a second launch adds the slabs in split order on the whole chip (a last arriver would read tens of slots of 32 KB alone).
// No atomics on data anywhere.  Tuning keys (tests, A/B): FRCNN_C1T_SPLIT forces the forward / input-gradient split count, FRCNN_C1T_WGRAD_SPLITS the
// weight gradient's; both are capped by the chunk count.  FRCNN_C1T_MT = 2 / 4 forces the tile's row count (64 / 128).
// Budgets (hipcc -Rpass-analysis=kernel-resource-usage): no private segment; 2 x (32 MT + 128) x 128 B of LDS = 65536 / 49152 bytes.
#include "frcnn_common.h"
#include <frcnn_buffer.h>   // angle brackets: shadowed by the test emulator
#include <frcnn_intrin.h>
#include <frcnn_sync.h>

namespace {

constexpr int kCK = 64;                              // reduction values per chunk
constexpr int kCBN = 128;                            // output columns per workgroup
constexpr int kCPitch = 128;                         // bytes per tile row: 64 16-bit values
constexpr int kCMaxSplit = 8;                        // K splits of the forward / input gradient (always finished in the launch)
constexpr int kCMaxTicket = 16;                      // pieces of a weight gradient that are still finished in the launch
constexpr int kCMaxSlabs = 256;                      // slabs of the weight gradient
constexpr size_t kCCounterPageBytes = 64 * 1024;     // tile counters: zeroed once by the caller, left zeroed by every launch

__device__ __forceinline__ uint32_t c1t_slot(int row, int g) { return (uint32_t)((g ^ ((row >> 1) & 7) ^ ((row >> 4) & 3)) << 4); }

// floats a thread stages per chunk for a tile of ROWS rows (either orientation: ROWS * 64 values over 256 threads)
template <int ROWS>
struct C1tStage { static constexpr int NV = ROWS / 4; };

// fetch this thread's share of chunk [k0, k0 + 64) of the tile whose first row is r0.  T: the source is [red][tile row] (nred lines of ld floats, ld = the
// tile-row count); otherwise [tile row][red] (nrows lines of ld = nred floats).
template <int ROWS, bool T>
__device__ __forceinline__ void c1t_fetch(float (&v)[C1tStage<ROWS>::NV], frcnn_buf_t buf, int tid, int r0, int k0, int nrows, int nred, int ld) {
    if constexpr (T) {
#pragma unroll
        for (int q = 0; q < ROWS / 32; ++q) {
            const int idx = tid + 256 * q, row = idx % ROWS, g = idx / ROWS;
            const bool in = r0 + row < nrows;
            const int red = k0 + 8 * g;
            const uint32_t base = (uint32_t)red * (uint32_t)ld + (uint32_t)(r0 + row);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[q * 8 + i] = frcnn_buf_load_f32(buf, (in && red + i < nred) ? (base + (uint32_t)i * (uint32_t)ld) * 4u : kBufOob);
        }
    } else {
#pragma unroll
        for (int q = 0; q < ROWS / 16; ++q) {
            const int idx = tid + 256 * q, row = idx >> 4, c4 = idx & 15;
            const bool in = r0 + row < nrows;
            const int red = k0 + 4 * c4;
            const uint32_t base = (uint32_t)(r0 + row) * (uint32_t)ld + (uint32_t)red;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[q * 4 + i] = frcnn_buf_load_f32(buf, (in && red + i < nred) ? (base + (uint32_t)i) * 4u : kBufOob);
        }
    }
}

// round to nearest even and write the tile image
template <int ROWS, bool T>
__device__ __forceinline__ void c1t_deposit(const float (&v)[C1tStage<ROWS>::NV], unsigned char *tile, int tid) {
    if constexpr (T) {
#pragma unroll
        for (int q = 0; q < ROWS / 32; ++q) {
            const int idx = tid + 256 * q, row = idx % ROWS, g = idx / ROWS;
            *reinterpret_cast<uint4 *>(tile + row * kCPitch + c1t_slot(row, g)) =
                make_uint4(frcnn_pack_bf16x2(v[q * 8], v[q * 8 + 1]), frcnn_pack_bf16x2(v[q * 8 + 2], v[q * 8 + 3]),
                           frcnn_pack_bf16x2(v[q * 8 + 4], v[q * 8 + 5]), frcnn_pack_bf16x2(v[q * 8 + 6], v[q * 8 + 7]));
        }
    } else {
#pragma unroll
        for (int q = 0; q < ROWS / 16; ++q) {
            const int idx = tid + 256 * q, row = idx >> 4, c4 = idx & 15;
            *reinterpret_cast<uint2 *>(tile + row * kCPitch + c1t_slot(row, c4 >> 1) + (c4 & 1) * 8) =
                make_uint2(frcnn_pack_bf16x2(v[q * 4], v[q * 4 + 1]), frcnn_pack_bf16x2(v[q * 4 + 2], v[q * 4 + 3]));
        }
    }
}

enum { kC1tDirect = 0, kC1tTicket = 1, kC1tSlab = 2 };       // what a workgroup does with its accumulators

// MODE direct: out = A B^T (+ bias per row).  ticket: `part` holds [tile][split] slots of 256 x MT x 16 floats behind the counters; the last arriver
// writes out.  slab: part[split] is shaped like out and receives this split's sum (summed by c1t_slab_sum_kernel).
template <int MT, bool AT, bool BT>
__global__ void __launch_bounds__(256)
c1t_kernel(const float *__restrict__ A, const float *__restrict__ B, const float *__restrict__ bias, float *__restrict__ out, float *__restrict__ part,
           int *__restrict__ counters, int rows, int cols, int red, int lda, int ldb, int colblocks, int splits, int cps, int mode) {
    constexpr int BM = 32 * MT;
    constexpr int ABYTES = BM * kCPitch, BBYTES = kCBN * kCPitch, STAGE = ABYTES + BBYTES;
    constexpr int AV = C1tStage<BM>::NV, BV = C1tStage<kCBN>::NV;
    constexpr int SLOT = 256 * MT * 16;                                     // floats of one split's accumulators
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];   // (the ticket is broadcast through its first word: ONE LDS object)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int tile = (int)blockIdx.x / splits, split = (int)blockIdx.x - tile * splits;
    const int rb = tile / colblocks, cb = tile - rb * colblocks;
    const int r0 = rb * BM, c0 = cb * kCBN;
    const int nch_all = (red + kCK - 1) / kCK;
    const int c_begin = split * cps;
    const int nch = min(nch_all, c_begin + cps) - c_begin;                  // >= 1 (host)
    const frcnn_buf_t abuf = frcnn_make_buf(A, (uint32_t)((size_t)rows * red * 4));
    const frcnn_buf_t bbuf = frcnn_make_buf(B, (uint32_t)((size_t)cols * red * 4));

    frcnn_f32x16 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    float va[AV], vb[BV];
    c1t_fetch<BM, AT>(va, abuf, tid, r0, c_begin * kCK, rows, red, lda);
    c1t_fetch<kCBN, BT>(vb, bbuf, tid, c0, c_begin * kCK, cols, red, ldb);
    c1t_deposit<BM, AT>(va, lds, tid);
    c1t_deposit<kCBN, BT>(vb, lds + ABYTES, tid);
    __syncthreads();

    const int brow = wave * 32 + l31;
    for (int c = 0; c < nch; ++c) {
        const unsigned char *st = lds + (c & 1) * STAGE;
        unsigned char *nx = lds + ((c + 1) & 1) * STAGE;
        const bool more = c + 1 < nch;                                      // workgroup-uniform
        if (more) {
            c1t_fetch<BM, AT>(va, abuf, tid, r0, (c_begin + c + 1) * kCK, rows, red, lda);
            c1t_fetch<kCBN, BT>(vb, bbuf, tid, c0, (c_begin + c + 1) * kCK, cols, red, ldb);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int g = 2 * ks + khalf;
            const uint4 fb = *reinterpret_cast<const uint4 *>(st + ABYTES + brow * kCPitch + c1t_slot(brow, g));
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int arow = i * 32 + l31;
                const uint4 fa = *reinterpret_cast<const uint4 *>(st + arow * kCPitch + c1t_slot(arow, g));
                acc[i] = frcnn_mfma_32x32x16_bf16(fa, fb, acc[i]);         // lane = output column, registers = rows
            }
        }
        if (more) {
            c1t_deposit<BM, AT>(va, nx, tid);
            c1t_deposit<kCBN, BT>(vb, nx + ABYTES, tid);
        }
        __syncthreads();
    }

    if (mode == kC1tTicket) {
        // publish this split's accumulators (write-through 16-byte stores: no release fence needed), take a ticket
        const frcnn_buf_t pbuf = frcnn_make_buf(part + ((size_t)tile * splits + split) * SLOT, (uint32_t)(SLOT * sizeof(float)));
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                frcnn_buf_store_f32x4_wt(pbuf, (uint32_t)(((i * 4 + r4) * 256 + tid) * 16),
                                         make_float4(acc[i][4 * r4], acc[i][4 * r4 + 1], acc[i][4 * r4 + 2], acc[i][4 * r4 + 3]));
        frcnn_drain_vmem();
        __syncthreads();
        int *s_ticket = reinterpret_cast<int *>(lds);                       // (every fragment read is behind the loop's last barrier)
        if (tid == 0) *s_ticket = frcnn_ticket(&counters[tile]);
        __syncthreads();
        if (*s_ticket != splits - 1) return;                                // workgroup-uniform
        if (tid == 0) {
            frcnn_acquire_agent();
            frcnn_counter_reset(&counters[tile]);                           // leave the counter page zeroed for the next launch
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        for (int q = 0; q < splits; ++q) {                                  // ALL slots, in split order, from memory
            const float4 *piece = reinterpret_cast<const float4 *>(part + ((size_t)tile * splits + q) * SLOT);
            float4 v[MT * 4];
#pragma unroll
            for (int e = 0; e < MT * 4; ++e) v[e] = piece[(size_t)e * 256 + tid];
#pragma unroll
            for (int e = 0; e < MT * 4; ++e) frcnn_pin(v[e]);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const float4 t = v[i * 4 + r4];
                    acc[i][4 * r4] += t.x; acc[i][4 * r4 + 1] += t.y; acc[i][4 * r4 + 2] += t.z; acc[i][4 * r4 + 3] += t.w;
                }
        }
    }

    // register r of accumulator i: row r0 + 32 i + (r & 3) + 8 (r >> 2) + 4 khalf, column c0 + 32 wave + l31; rows and columns past the matrix get an
    // out-of-range offset and store nothing
    float *dst = mode == kC1tSlab ? part + (size_t)split * rows * cols : out;
    const frcnn_buf_t obuf = frcnn_make_buf(dst, (uint32_t)((size_t)rows * cols * 4));
    const frcnn_buf_t bibuf = frcnn_make_buf(bias, (uint32_t)rows * 4u);
    const bool has_bias = bias != nullptr;                                  // workgroup-uniform
    const int n = c0 + wave * 32 + l31;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = r0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
            const bool in = m < rows && n < cols;
            float b = 0.0f;          // every register of a lane is another row: one bias load per register (two addresses per wave-instruction), none without a bias (all layers but the stem)
            if (has_bias) b = frcnn_buf_load_f32(bibuf, m < rows ? (uint32_t)m * 4u : kBufOob);
            frcnn_buf_store_f32(obuf, in ? ((uint32_t)m * (uint32_t)cols + (uint32_t)n) * 4u : kBufOob, acc[i][r] + b);
        }
}

// out[i] = sum over the slabs, in slab order, of part[s][i]
__global__ void __launch_bounds__(256)
c1t_slab_sum_kernel(const float *__restrict__ part, float *__restrict__ out, int total, int splits) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
        float v = 0.0f;
        int s = 0;
        for (; s + 4 <= splits; s += 4) {
            float t0 = part[(size_t)s * total + i], t1 = part[(size_t)(s + 1) * total + i], t2 = part[(size_t)(s + 2) * total + i],
                  t3 = part[(size_t)(s + 3) * total + i];
            frcnn_pin(t0); frcnn_pin(t1); frcnn_pin(t2); frcnn_pin(t3);
            v += t0; v += t1; v += t2; v += t3;
        }
        for (; s < splits; ++s) v += part[(size_t)s * total + i];
        out[i] = v;
    }
}

struct C1tPlan { int mt, rowblocks, colblocks, tiles, splits, cps; bool ticket; };

// The tile shape and K split of a launch.  These products are bound by memory, not by the MFMAs, so the tile is the small one (64 rows: 141-180
// registers, two workgroups per CU -- three in the weight-gradient form -- where 128 rows need 202-257 and were slower in the forward and input-gradient forms at every measured shape) unless the launch would have more than eight of them per CU; K is split (each piece at least two chunks long) until
// the launch has `fill` workgroups per CU; `forced` > 0 sets the count (still capped by the chunk count and `cap`).  Up to kCMaxSplit pieces are
// finished in the launch (a counter per tile in the page) and up to kCMaxTicket of a weight gradient; more of them (layers with few tiles) go through slabs.
static C1tPlan c1t_plan(int rows, int cols, int red, int cap, int fill, int forced) {
    C1tPlan p;
    const long cus = frcnn_cu_count();
    p.colblocks = frcnn_cdiv(cols, kCBN);
    p.mt = (rows > 64 && (long)frcnn_cdiv(rows, 64) * p.colblocks > 8 * cus) ? 4 : 2;
    const int mt_forced = frcnn_tune_int("FRCNN_C1T_MT", 0);                // A/B and test hook: the tile's rows / 32
    if (mt_forced == 2 || mt_forced == 4) p.mt = mt_forced;
    p.rowblocks = frcnn_cdiv(rows, 32 * p.mt);
    const long tiles = (long)p.rowblocks * p.colblocks;
    p.tiles = (int)tiles;
    const int nch = frcnn_cdiv(red, kCK);
    long s = fill * cus / tiles;
    if (s > nch / 2) s = nch / 2;
    if (forced > 0) s = forced;
    if (s > cap) s = cap;
    if (s > nch) s = nch;
    if (s < 1) s = 1;
    const bool counters_fit = tiles <= (long)(kCCounterPageBytes / sizeof(int));
    if (cap <= kCMaxSplit && !counters_fit) s = 1;
    p.cps = frcnn_cdiv(nch, (int)s);
    p.splits = frcnn_cdiv(nch, p.cps);
    p.ticket = p.splits <= kCMaxTicket && counters_fit;
    return p;
}

static size_t c1t_ws_bytes(const C1tPlan &p, int rows, int cols) {
    if (p.splits <= 1) return kCCounterPageBytes;
    return kCCounterPageBytes + (p.ticket ? (size_t)p.tiles * p.splits * 256 * p.mt * 16 : (size_t)p.splits * rows * cols) * sizeof(float);
}

static bool c1t_fits(size_t a, size_t b, size_t c) { return a * 4 < (1ull << 31) && b * 4 < (1ull << 31) && c * 4 < (1ull << 31); }

template <bool AT, bool BT>
static int c1t_launch(const C1tPlan &p, const float *A, const float *B, const float *bias, float *out, void *workspace, int rows, int cols, int red,
                      int lda, int ldb, hipStream_t stream) {
    const int mode = p.splits <= 1 ? kC1tDirect : (p.ticket ? kC1tTicket : kC1tSlab);
    int *counters = (int *)workspace;
    float *part = (float *)((char *)workspace + kCCounterPageBytes);
    const dim3 grid((unsigned)((long)p.tiles * p.splits));
    if (p.mt == 2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(c1t_kernel<2, AT, BT>), grid, dim3(256), 0, stream, A, B, bias, out, part, counters, rows, cols, red, lda, ldb,
                           p.colblocks, p.splits, p.cps, mode);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(c1t_kernel<4, AT, BT>), grid, dim3(256), 0, stream, A, B, bias, out, part, counters, rows, cols, red, lda, ldb,
                           p.colblocks, p.splits, p.cps, mode);
    if (mode == kC1tSlab) {
        const int total = rows * cols;
        const int blocks = (total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048;
        hipLaunchKernelGGL(c1t_slab_sum_kernel, dim3(blocks), dim3(256), 0, stream, (const float *)part, out, total, p.splits);
    }
    return frcnn_launch_status();
}

static C1tPlan c1t_plan_fwd(int Cin, int Cout, int HW) { return c1t_plan(Cout, HW, Cin, kCMaxSplit, 1, frcnn_tune_int("FRCNN_C1T_SPLIT", 0)); }
static C1tPlan c1t_plan_dgrad(int Cin, int Cout, int HW) { return c1t_plan(Cin, HW, Cout, kCMaxSplit, 1, frcnn_tune_int("FRCNN_C1T_SPLIT", 0)); }
static C1tPlan c1t_plan_wgrad(int Cin, int Cout, int HW) { return c1t_plan(Cin, Cout, HW, kCMaxSlabs, 2, frcnn_tune_int("FRCNN_C1T_WGRAD_SPLITS", 0)); }
static bool c1t_dims_ok(int Cin, int Cout, int HW) {
    return Cin >= 1 && Cout >= 1 && HW >= 1 && c1t_fits((size_t)Cin * HW, (size_t)Cout * HW, (size_t)Cin * Cout);
}

}  // namespace

extern "C" {

size_t frcnn_conv1x1_fwd_bf16_train_workspace_bytes(int Cin, int Cout, int HW) {
    if (!c1t_dims_ok(Cin, Cout, HW)) return 0;
    return c1t_ws_bytes(c1t_plan_fwd(Cin, Cout, HW), Cout, HW);
}

int frcnn_conv1x1_fwd_bf16_train(const float *x, const float *w_packed, const float *bias, float *z, int Cin, int Cout, int HW, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    if (!x || !w_packed || !z || !workspace || !c1t_dims_ok(Cin, Cout, HW)) return FRCNN_ERR_INVALID;
    const C1tPlan p = c1t_plan_fwd(Cin, Cout, HW);
    if (workspace_bytes < c1t_ws_bytes(p, Cout, HW)) return FRCNN_ERR_INVALID;
    return c1t_launch<true, true>(p, w_packed, x, bias, z, workspace, Cout, HW, Cin, Cout, HW, (hipStream_t)stream);
}

size_t frcnn_conv1x1_dgrad_bf16_workspace_bytes(int Cin, int Cout, int HW) {
    if (!c1t_dims_ok(Cin, Cout, HW)) return 0;
    return c1t_ws_bytes(c1t_plan_dgrad(Cin, Cout, HW), Cin, HW);
}

int frcnn_conv1x1_dgrad_bf16(const float *dz, const float *w_packed, float *dx, int Cin, int Cout, int HW, void *workspace, size_t workspace_bytes,
                             void *stream) {
    if (!dz || !w_packed || !dx || !workspace || !c1t_dims_ok(Cin, Cout, HW)) return FRCNN_ERR_INVALID;
    const C1tPlan p = c1t_plan_dgrad(Cin, Cout, HW);
    if (workspace_bytes < c1t_ws_bytes(p, Cin, HW)) return FRCNN_ERR_INVALID;
    return c1t_launch<false, true>(p, w_packed, dz, nullptr, dx, workspace, Cin, HW, Cout, Cout, HW, (hipStream_t)stream);
}

size_t frcnn_conv1x1_wgrad_bf16_workspace_bytes(int Cin, int Cout, int HW) {
    if (!c1t_dims_ok(Cin, Cout, HW)) return 0;
    return c1t_ws_bytes(c1t_plan_wgrad(Cin, Cout, HW), Cin, Cout);
}

int frcnn_conv1x1_wgrad_bf16(const float *x, const float *dz, float *dw_packed, int Cin, int Cout, int HW, void *workspace, size_t workspace_bytes,
                             void *stream) {
    if (!x || !dz || !dw_packed || !workspace || !c1t_dims_ok(Cin, Cout, HW)) return FRCNN_ERR_INVALID;
    const C1tPlan p = c1t_plan_wgrad(Cin, Cout, HW);
    if (workspace_bytes < c1t_ws_bytes(p, Cin, Cout)) return FRCNN_ERR_INVALID;
    return c1t_launch<false, false>(p, x, dz, nullptr, dw_packed, workspace, Cin, Cout, HW, HW, HW, (hipStream_t)stream);
}

}  // extern "C"
