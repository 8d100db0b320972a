// conv_wino.hip -- the fp32 3x3 / pad 1 convolutions of the VGG-16 inference forward as Winograd F(2x2, 3x3) on the matrix cores.
//
// A 2x2 output block of one (cin, cout) pair costs 16 multiplies instead of the direct form's 36:
//   Y = A^T [ U (.) V ] A,   U = G g G^T (the weights, once per load),   V = B^T d B (the 4x4 input patch d),
//   B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],  G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1],  A^T = [1 1 1 0; 0 1 -1 -1].
// Each of the 16 components (r, k) is its own GEMM  M[r][k][co][tile] = sum_ci U[ci][r][co][k] * V[ci][r][k][tile]  on
// v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation), so the matrix work is 16/36 of the direct kernel's (conv.hip).
//   * A workgroup (4 waves) owns BCO = 32 x CB couts x 4 TB output rows x 32 output columns = 32 TB Winograd tiles (one MFMA N = 32
//     per 4-row band).  Per K-chunk of CK channels it stages the (4 TB + 2) x 34 input halo of each channel (LDS-DMA, 16-byte pieces at
//     pitch 40 -- the staging of conv.hip's HB form) and the CK x 16 x BCO slab of U, double-buffered.
//   * Wave w owns component row w of B^T: it reads the two patch rows that row combines (B operand lane l = (channel l>>5, tile l&31)),
//     forms (B^T d)[w][0..3] and then (B^T d B)[w][0..3] in 8 VALU operations, and feeds the four results straight into the MFMAs of
//     components (w, 0..3) x CB cout blocks: 4 CB (x TB) MFMAs per 8 VALU, the transform never touches LDS.
//   * U is stored [Cin][4 rows][Cout][4 columns], so a lane's A operands of the four components of its row are ONE ds_read_b128.
//   * Epilogue: Z = M A (two columns) in registers, Z exchanged through LDS, Y = A^T Z, + bias, ReLU, optionally the 2x2/2 max-pool
//     (the aligned 2x2 output block of a tile is exactly a pool window).  Output fp32 NCHW.
//   * Small maps split K over `pieces` workgroups per tile; every piece writes its Y (after A^T M A, 4x fewer bytes than M) into a
//     workspace slab and a second launch adds the slabs IN PIECE ORDER, then bias / ReLU / pool: bit-identical over repeats.
// Weight memory: U holds 16 floats per (cout, cin) pair where the packed direct weights hold 9.
#include "frcnn_common.h"
#include <frcnn_buffer.h>
#include <frcnn_intrin.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kWinoPitch = 40;      // floats per halo row in LDS: ten 16-byte groups x0-4 .. x0+35
constexpr int kWinoLead = 3;        // halo column 0 (input column x0-1) sits at float 3 of its row

// mode bit 0: ReLU, bit 1: fused 2x2/2 max-pool (ceil mode; ReLU implied), bit 2: K piece -> raw Y (no bias) into y + piece * Cout*H*W
template <int CB, int TB, int CK, int BPC, bool SOFF>
__global__ void __launch_bounds__(256, BPC)
conv_wino_f32_kernel(const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ bias, float *__restrict__ y,
                     int Cin, int Cout, int H, int W, int mode, int xtiles, int ytiles, int nchunks, int piece_chunks) {
    constexpr int NT = 256;
    constexpr int BCO = 32 * CB;
    constexpr int HR = 4 * TB + 2;                    // halo rows per channel
    constexpr int WV = CK * 4 * BCO;                  // float4s of U per chunk: rows (ci, r) x BCO couts (4 k-components each)
    constexpr int WIT = WV / NT;
    constexpr int HG = CK * HR * 10;                  // 16-byte halo groups per chunk
    constexpr int HIT4 = (HG + NT - 1) / NT;
    constexpr int HVP = (HG + 63) / 64 * 256;         // a buffer holds whole DMA pieces (the tail lanes deposit zeros)
    constexpr int WBUF = WV * 4;
    constexpr int ZF = 4 * 2 * TB * CB * 16 * 64;     // epilogue exchange: Z[wave][column][tb][cb][16 regs][64 lanes]
    constexpr int MAINF = 2 * WBUF + 2 * HVP;
    constexpr int SMEM = MAINF > ZF ? MAINF : ZF;
    static_assert(WV % NT == 0, "U slab must split into whole per-thread float4s");
    static_assert(CK % 2 == 0 && CK * HR * 3 <= NT, "chunk shape");
    static_assert(SMEM * 4 <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) float smem[SMEM];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int HW = H * W;
    const int npx = xtiles * ytiles, ntiles = npx * (Cout / BCO);
    // XCD-aware placement (as conv.hip): XCD x gets the x-th contiguous eighth of [piece][cout block][pixel tile]
    int g = blockIdx.x;
    {
        const int G = gridDim.x, xcd = g & 7, q = G >> 3, r = G & 7;
        g = xcd * q + (xcd < r ? xcd : r) + (g >> 3);
    }
    const int piece = g / ntiles, tile = g % ntiles;
    const int pxt = tile % npx, cot = tile / npx;
    const int tx = pxt % xtiles, ty = pxt / xtiles;
    const int x0 = tx * 32, y0 = ty * 4 * TB, co0 = cot * BCO;
    const int c_begin = piece * piece_chunks;
    const int c_end = nchunks < c_begin + piece_chunks ? nchunks : c_begin + piece_chunks;
    const int K4 = Cin * 4;

    const frcnn_buf_t xbuf = frcnn_make_buf(x, (uint32_t)((size_t)Cin * HW * sizeof(float)));
    const frcnn_buf_t ubuf = frcnn_make_buf(u, (uint32_t)((size_t)K4 * Cout * 4 * sizeof(float)));
    const uint32_t u_chunk_bytes = (uint32_t)(CK * 4 * Cout * 4) * 4u, x_chunk_bytes = (uint32_t)(CK * HW) * 4u;

    uint32_t woff[WIT], hoff[HIT4];
#pragma unroll
    for (int q = 0; q < WIT; ++q) {
        const int v = tid + q * NT;
        const int row = v / BCO, c4 = v % BCO;
        woff[q] = (uint32_t)(row * Cout * 4 + (co0 + c4) * 4) * 4u;
    }
#pragma unroll
    for (int q = 0; q < HIT4; ++q) {                         // group e4 = (channel, halo row, group of four columns)
        const int e4 = tid + q * NT;
        const int c = e4 / (HR * 10), rem = e4 % (HR * 10);
        const int hr = rem / 10, g4 = rem % 10;
        const int gy = y0 - 1 + hr, gx = x0 - 4 + 4 * g4;
        const bool inside = e4 < HG && gy >= 0 && gy < H && gx >= 0 && gx < W;
        hoff[q] = inside ? (uint32_t)(c * HW + gy * W + gx) * 4u : kBufOob;
    }
    auto w_lds = [&](int buf) { return smem + buf * WBUF; };
    auto in_lds = [&](int buf) { return smem + 2 * WBUF + buf * HVP; };
    // a 16-byte group that straddles the right image border (W % 4 != 0) brings up to three floats of the next row along: zero them
    const int fix_lo = W - x0 + 4, fix_hi = (fix_lo + 3) & ~3;
    const bool edge_fix = (W & 3) != 0 && fix_lo > 0 && fix_lo < kWinoPitch;
    auto edge_zero = [&](int buf) {
        const int row = tid / 3, i = fix_lo + tid % 3;
        if (row < CK * HR && i < fix_hi) in_lds(buf)[row * kWinoPitch + i] = 0.0f;
        frcnn_barrier_nofence();
    };
    auto issue = [&](int chunk, int buf) {
        if constexpr (SOFF) {               // Cin is a whole number of chunks: the chunk offset rides in the scalar offset
            const uint32_t wb = (uint32_t)chunk * u_chunk_bytes, xb = (uint32_t)chunk * x_chunk_bytes;
#pragma unroll
            for (int q = 0; q < WIT; ++q) frcnn_buf_load_lds_b128(ubuf, w_lds(buf) + (q * NT + wave * 64) * 4, woff[q], wb);
#pragma unroll
            for (int q = 0; q < HIT4; ++q)
                if ((q + 1) * NT * 4 <= HVP || (wave * 64 + q * NT) * 4 < HVP)
                    frcnn_buf_load_lds_b128(xbuf, in_lds(buf) + (q * NT + wave * 64) * 4, hoff[q], xb);
        } else {                            // ragged last chunk: per-chunk descriptors whose range ends at the tensor's end
            const long long wrem = (long long)(K4 - chunk * CK * 4) * Cout * 4, xrem = (long long)(Cin - chunk * CK) * HW;
            const frcnn_buf_t ub_c = frcnn_make_buf(u + (size_t)chunk * CK * 4 * Cout * 4, (uint32_t)((wrem > 0 ? wrem : 0) * sizeof(float)));
            const frcnn_buf_t xb_c = frcnn_make_buf(x + (size_t)chunk * CK * HW, (uint32_t)((xrem > 0 ? xrem : 0) * sizeof(float)));
#pragma unroll
            for (int q = 0; q < WIT; ++q) frcnn_buf_load_lds_b128(ub_c, w_lds(buf) + (q * NT + wave * 64) * 4, woff[q], 0);
#pragma unroll
            for (int q = 0; q < HIT4; ++q)
                if ((q + 1) * NT * 4 <= HVP || (wave * 64 + q * NT) * 4 < HVP)
                    frcnn_buf_load_lds_b128(xb_c, in_lds(buf) + (q * NT + wave * 64) * 4, hoff[q], 0);
        }
    };

    f32x16 acc[TB][4][CB];
#pragma unroll
    for (int t = 0; t < TB; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < CB; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][k][c][r] = 0.0f;

    // row w of B^T d = d[ra] + sb * d[rb]:  w0 d0 - d2,  w1 d1 + d2,  w2 d2 - d1,  w3 d1 - d3  (fmaf with sb = +-1 is the exact add / subtract)
    const int ra = wave == 0 ? 0 : (wave == 2 ? 2 : 1);
    const int rb = wave == 0 ? 2 : (wave == 1 ? 2 : (wave == 2 ? 1 : 3));
    const float sb = wave == 1 ? 1.0f : -1.0f;
    const int tr = l31 >> 4, tc = l31 & 15;              // tile of this lane: tile row (within a 4-row band), tile column

    issue(c_begin, 0);
    frcnn_wait_vmcnt<0>();
    frcnn_barrier_nofence();
    if (edge_fix) edge_zero(0);
    int cur = 0;
    for (int chunk = c_begin; chunk < c_end; ++chunk) {
        const bool more = chunk + 1 < c_end;
        if (more) issue(chunk + 1, cur ^ 1);
        constexpr int NSTEP = CK / 2;
        const float *b_base = in_lds(cur) + (khalf * HR + 2 * tr) * kWinoPitch + kWinoLead + 2 * tc;
        const float *ba = b_base + ra * kWinoPitch, *bb = b_base + rb * kWinoPitch;
        const float4 *a_base = reinterpret_cast<const float4 *>(w_lds(cur)) + (khalf * 4 + wave) * BCO + l31;
        auto frag = [&](int s, float4 *a, float (*da)[4], float (*db)[4]) {
#pragma unroll
            for (int c = 0; c < CB; ++c) a[c] = a_base[2 * s * 4 * BCO + 32 * c];
#pragma unroll
            for (int t = 0; t < TB; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    da[t][j] = ba[(2 * s * HR + 4 * t) * kWinoPitch + j];
                    db[t][j] = bb[(2 * s * HR + 4 * t) * kWinoPitch + j];
                }
        };
        float4 a[2][CB];
        float da[2][TB][4], db[2][TB][4];
        frag(0, a[0], da[0], db[0]);
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            if (s + 1 < NSTEP) frag(s + 1, a[(s + 1) & 1], da[(s + 1) & 1], db[(s + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);       // keep the prefetch ahead of this step's MFMAs
#pragma unroll
            for (int t = 0; t < TB; ++t) {
                float tt[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) tt[j] = fmaf(sb, db[s & 1][t][j], da[s & 1][t][j]);
                const float v[4] = {tt[0] - tt[2], tt[1] + tt[2], tt[2] - tt[1], tt[1] - tt[3]};
#pragma unroll
                for (int c = 0; c < CB; ++c) {
                    const float4 av = a[s & 1][c];
                    acc[t][0][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, v[0], acc[t][0][c], 0, 0, 0);
                    acc[t][1][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, v[1], acc[t][1][c], 0, 0, 0);
                    acc[t][2][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, v[2], acc[t][2][c], 0, 0, 0);
                    acc[t][3][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, v[3], acc[t][3][c], 0, 0, 0);
                }
            }
        }
        frcnn_wait_vmcnt<0>();           // chunk + 1 has landed (nothing else is in flight)
        frcnn_barrier_nofence();         // ... for everybody, and everybody is done reading buffer `cur`
        if (edge_fix && more) edge_zero(cur ^ 1);
        cur ^= 1;
    }

    // ---- epilogue.  Z[w][0] = M[w][0] + M[w][1] + M[w][2],  Z[w][1] = M[w][1] - M[w][2] - M[w][3]  (M A, this wave's row)
    float4 *z4 = reinterpret_cast<float4 *>(smem);          // the loop's last barrier: nobody reads the staging buffers any more
#pragma unroll
    for (int t = 0; t < TB; ++t)
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                float z0[4], z1[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * r4 + e;
                    z0[e] = (acc[t][0][c][r] + acc[t][1][c][r]) + acc[t][2][c][r];
                    z1[e] = (acc[t][1][c][r] - acc[t][2][c][r]) - acc[t][3][c][r];
                }
                z4[(((wave * 2 + 0) * TB * CB + t * CB + c) * 4 + r4) * 64 + lane] = make_float4(z0[0], z0[1], z0[2], z0[3]);
                z4[(((wave * 2 + 1) * TB * CB + t * CB + c) * 4 + r4) * 64 + lane] = make_float4(z1[0], z1[1], z1[2], z1[3]);
            }
    __syncthreads();
    // wave w finishes D registers 4w .. 4w+3 of every accumulator: couts co0 + 32 c + 8 w + 4 khalf + e, all four outputs of the block
    const bool relu = (mode & 1) != 0, pool = (mode & 2) != 0, partial = (mode & 4) != 0;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
#pragma unroll
    for (int t = 0; t < TB; ++t) {
        const int oy = y0 + 4 * t + 2 * tr, ox = x0 + 2 * tc;
        const bool in0 = oy < H && ox < W, has_r = ox + 1 < W, has_d = oy + 1 < H;
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            float4 zz[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 2; ++q) zz[r][q] = z4[(((r * 2 + q) * TB * CB + t * CB + c) * 4 + wave) * 64 + lane];
            const int cob = co0 + 32 * c + 8 * wave + 4 * khalf;
            const float4 bq = partial ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4 *>(&bias[cob]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                auto comp = [&](const float4 &v) { return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w)); };
                float yv[2][2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    yv[0][q] = (comp(zz[0][q]) + comp(zz[1][q])) + comp(zz[2][q]);
                    yv[1][q] = (comp(zz[1][q]) - comp(zz[2][q])) - comp(zz[3][q]);
                }
                const float b = comp(bq);
                const int co = cob + e;
                if (!in0) continue;
                if (pool) {
                    float m = yv[0][0];
                    if (has_r) m = fmaxf(m, yv[0][1]);
                    if (has_d) m = fmaxf(m, yv[1][0]);
                    if (has_r && has_d) m = fmaxf(m, yv[1][1]);
                    y[(size_t)co * OH * OW + (size_t)(oy >> 1) * OW + (ox >> 1)] = fmaxf(m + b, 0.0f);       // max, +bias, ReLU commute
                } else {
                    float *yo = y + (partial ? (size_t)piece * Cout * HW : 0) + (size_t)co * HW + (size_t)oy * W + ox;
#pragma unroll
                    for (int p = 0; p < 2; ++p)
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            if ((p && !has_d) || (q && !has_r)) continue;
                            float v = yv[p][q] + b;
                            if (relu) v = fmaxf(v, 0.0f);
                            yo[p * W + q] = v;
                        }
                }
            }
        }
    }
}

// the K pieces of a split launch: slabs added in piece order, then bias, ReLU and (mode bit 1) the 2x2/2 ceil-mode max-pool
__global__ void __launch_bounds__(256)
wino_combine_kernel(const float *__restrict__ ws, const float *__restrict__ bias, float *__restrict__ y, int P, int C, int H, int W, int mode) {
    const size_t HW = (size_t)H * W, slab = (size_t)C * HW;
    const bool relu = (mode & 1) != 0, pool = (mode & 2) != 0;
    const int OH = pool ? (H + 1) / 2 : H, OW = pool ? (W + 1) / 2 : W;
    const size_t total = (size_t)C * OH * OW;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ow = (int)(i % OW), oh = (int)((i / OW) % OH), c = (int)(i / ((size_t)OW * OH));
        auto sum = [&](int yy, int xx) {
            const float *p = ws + (size_t)c * HW + (size_t)yy * W + xx;
            float s = p[0];
            for (int k = 1; k < P; ++k) s += p[(size_t)k * slab];
            return s;
        };
        if (pool) {
            const int yy = 2 * oh, xx = 2 * ow;
            float m = sum(yy, xx);
            if (xx + 1 < W) m = fmaxf(m, sum(yy, xx + 1));
            if (yy + 1 < H) m = fmaxf(m, sum(yy + 1, xx));
            if (xx + 1 < W && yy + 1 < H) m = fmaxf(m, sum(yy + 1, xx + 1));
            y[i] = fmaxf(m + bias[c], 0.0f);
        } else {
            float v = sum(oh, ow) + bias[c];
            y[i] = relu ? fmaxf(v, 0.0f) : v;
        }
    }
}

// U[ci][r][co][k] = (G g G^T)[r][k], evaluated in double and rounded once.  packed: w is frcnn_pack_conv3x3_w's [(ci*9+tap)][Cout] (a
// trainer's live weights), else (Cout, Cin, 3, 3)
__global__ void __launch_bounds__(256)
wino_pack_w_kernel(const float *__restrict__ w, int Cout, int Cin, int packed, float *__restrict__ u) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Cout * Cin) return;
    const int co = i % Cout, ci = i / Cout;
    auto tap = [&](int t) { return (double)(packed ? w[((size_t)ci * 9 + t) * Cout + co] : w[((size_t)co * Cin + ci) * 9 + t]); };
    double gg[3][4];                      // (g G^T)[row][k]
    for (int a = 0; a < 3; ++a) {
        const double g0 = tap(a * 3), g1 = tap(a * 3 + 1), g2 = tap(a * 3 + 2);
        gg[a][0] = g0;
        gg[a][1] = 0.5 * (g0 + g1 + g2);
        gg[a][2] = 0.5 * (g0 - g1 + g2);
        gg[a][3] = g2;
    }
    for (int k = 0; k < 4; ++k) {
        const double v[4] = {gg[0][k], 0.5 * (gg[0][k] + gg[1][k] + gg[2][k]), 0.5 * (gg[0][k] - gg[1][k] + gg[2][k]), gg[2][k]};
        for (int r = 0; r < 4; ++r) u[(((size_t)ci * 4 + r) * Cout + co) * 4 + k] = (float)v[r];
    }
}

struct WinoPlan { int xtiles, ytiles, ntiles, nchunks, piece_chunks, pieces; };

template <int CB, int TB, int CK>
static WinoPlan plan_wino(int Cin, int Cout, int H, int W, int pieces) {
    WinoPlan p;
    p.xtiles = frcnn_cdiv(W, 32); p.ytiles = frcnn_cdiv(H, 4 * TB);
    p.ntiles = p.xtiles * p.ytiles * (Cout / (32 * CB));
    p.nchunks = frcnn_cdiv(Cin, CK);
    if (pieces < 1) pieces = 1;
    if (pieces > p.nchunks) pieces = p.nchunks;
    p.piece_chunks = frcnn_cdiv(p.nchunks, pieces);
    p.pieces = frcnn_cdiv(p.nchunks, p.piece_chunks);
    return p;
}

template <int CB, int TB, int CK, int BPC>
static int launch_wino(const float *x, const float *u, const float *bias, float *y, int Cin, int Cout, int H, int W, int mode, int pieces,
                       void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (Cout % (32 * CB) != 0) return FRCNN_ERR_INVALID;
    const WinoPlan p = plan_wino<CB, TB, CK>(Cin, Cout, H, W, pieces);
    const bool split = p.pieces > 1;
    if (split && (!workspace || workspace_bytes < (size_t)p.pieces * Cout * H * W * sizeof(float))) return FRCNN_ERR_INVALID;
    const int kmode = split ? 4 : mode;
    float *out = split ? (float *)workspace : y;
    const int G = p.ntiles * p.pieces;
    if (Cin % CK == 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_wino_f32_kernel<CB, TB, CK, BPC, true>), dim3(G), dim3(256), 0, stream, x, u, bias, out, Cin, Cout, H, W,
                           kmode, p.xtiles, p.ytiles, p.nchunks, p.piece_chunks);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_wino_f32_kernel<CB, TB, CK, BPC, false>), dim3(G), dim3(256), 0, stream, x, u, bias, out, Cin, Cout, H, W,
                           kmode, p.xtiles, p.ytiles, p.nchunks, p.piece_chunks);
    if (split) {
        const size_t total = (size_t)Cout * ((mode & 2) ? (size_t)((H + 1) / 2) * ((W + 1) / 2) : (size_t)H * W);
        const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
        hipLaunchKernelGGL(wino_combine_kernel, dim3(blocks), dim3(256), 0, stream, (const float *)workspace, bias, y, p.pieces, Cout, H, W, mode);
    }
    return frcnn_launch_status();
}

// Decomposition ids (FRCNN_CONV_WINO_CFG overrides the pick):
//   1: 64 couts x 4 rows, 8-channel chunks, two workgroups per CU     2: the same with 4-channel chunks
// (128 couts per wave, or 8-row tiles, need 256 accumulator registers per wave and spill at one wave per SIMD: not built)
static int pick_wino_config(int Cin, int Cout, int H, int W) {
    const int forced = frcnn_tune_int("FRCNN_CONV_WINO_CFG", 0);
    if (forced >= 1 && forced <= 2) return forced;
    (void)Cin; (void)Cout; (void)H; (void)W;
    return 1;
}

// K pieces per tile: enough workgroups for about two per CU slot, a piece never shorter than four chunks.  FRCNN_CONV_WINO_SPLIT forces.
static int pick_wino_pieces(int cfg, int Cin, int Cout, int H, int W) {
    const int forced = frcnn_tune_int("FRCNN_CONV_WINO_SPLIT", 0);
    if (forced > 0) return forced;
    const int CK = cfg == 1 ? 8 : 4, BPC = 2;
    const long ntiles = (long)frcnn_cdiv(W, 32) * frcnn_cdiv(H, 4) * (Cout / 64);
    const long slots = (long)frcnn_cu_count() * BPC;
    const int nchunks = frcnn_cdiv(Cin, CK);
    if (ntiles >= 2 * slots) return 1;
    int pieces = (int)((2 * slots + ntiles - 1) / ntiles);
    const int maxp = nchunks / 4 > 1 ? nchunks / 4 : 1;
    return pieces < maxp ? pieces : maxp;
}

}  // namespace

extern "C" {

int frcnn_wino_pack_w(const float *w, int Cout, int Cin, int packed, float *u, void *stream) {
    if (!w || !u || Cout < 1 || Cin < 1 || (packed != 0 && packed != 1)) return FRCNN_ERR_INVALID;
    hipLaunchKernelGGL(wino_pack_w_kernel, dim3(frcnn_cdiv(Cout * Cin, 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, packed, u);
    return frcnn_launch_status();
}

size_t frcnn_conv_wino_workspace_bytes(int Cin, int Cout, int H, int W) {
    if (Cin < 1 || Cout < 1 || H < 1 || W < 1) return 0;
    size_t best = 256;
    for (int cfg = 1; cfg <= 2; ++cfg) {
        const int CK = cfg == 1 ? 8 : 4;
        int pieces = pick_wino_pieces(cfg, Cin, Cout, H, W);
        const int nchunks = frcnn_cdiv(Cin, CK);
        if (pieces > nchunks) pieces = nchunks;
        const int pc = frcnn_cdiv(nchunks, pieces > 0 ? pieces : 1);
        pieces = frcnn_cdiv(nchunks, pc);
        const size_t b = pieces > 1 ? frcnn_align256((size_t)pieces * Cout * H * W * sizeof(float)) : 256;
        if (b > best) best = b;
    }
    return best;
}

// act: 1 = bias + ReLU, 4 = bias + ReLU + 2x2/2 ceil-mode max-pool (y is Cout x ceil(H/2) x ceil(W/2)), 0 = bias only
int frcnn_conv3x3_wino_f32(const float *x, const float *u, const float *bias, float *y, int Cin, int Cout, int H, int W, int act,
                           void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !u || !bias || !y || Cin < 1 || Cout < 1 || H < 1 || W < 1 || (Cout % 64) != 0) return FRCNN_ERR_INVALID;
    if (act != 0 && act != 1 && act != 4) return FRCNN_ERR_INVALID;
    if ((size_t)Cin * H * W * 4 >= (1ull << 31) || (size_t)Cin * 16 * Cout * 4 >= (1ull << 31)) return FRCNN_ERR_INVALID;   // 32-bit buffer offsets
    const int mode = act == 4 ? 3 : act;
    const int cfg = pick_wino_config(Cin, Cout, H, W);
    const int pieces = pick_wino_pieces(cfg, Cin, Cout, H, W);
    switch (cfg) {
        case 2: return launch_wino<2, 1, 4, 2>(x, u, bias, y, Cin, Cout, H, W, mode, pieces, workspace, workspace_bytes, stream);
        default: return launch_wino<2, 1, 8, 2>(x, u, bias, y, Cin, Cout, H, W, mode, pieces, workspace, workspace_bytes, stream);
    }
}

}  // extern "C"
