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
#include <frcnn_sync.h>   // angle brackets: the test emulator shadows these headers via its include path
#include <frcnn_buffer.h>
#include <frcnn_intrin.h>
#include <frcnn_wino_loop.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kWinoPitch = 40;      // floats per halo row in LDS: ten 16-byte groups x0-4 .. x0+35
constexpr int kWinoLead = 3;        // halo column 0 (input column x0-1) sits at float 3 of its row

// LDS geometry of one workgroup (4 waves): two U slabs and two halo buffers of a CK-channel chunk; the epilogue's Z exchange reuses them
template <int CB, int TB, int CK>
struct WinoGeom {
    static constexpr int NT = 256;
    static constexpr int BCO = 32 * CB;
    static constexpr int HR = 4 * TB + 2;                    // halo rows per channel
    static constexpr int WV = CK * 4 * BCO;                  // float4s of U per chunk: rows (ci, r) x BCO couts (4 k-components each)
    static constexpr int WIT = WV / NT;
    static constexpr int HG = CK * HR * 10;                  // 16-byte halo groups per chunk
    static constexpr int HIT4 = (HG + NT - 1) / NT;
    static constexpr int HVP = (HG + 63) / 64 * 256;         // a buffer holds whole DMA pieces (the tail lanes deposit zeros)
    static constexpr int WBUF = WV * 4;
    static constexpr int ZF = 4 * 2 * TB * CB * 16 * 64;     // epilogue exchange: Z[wave][column][tb][cb][16 regs][64 lanes]
    static constexpr int MAINF = 2 * WBUF + 2 * HVP;
    static constexpr int SMEM = MAINF > ZF ? MAINF : ZF;
    static_assert(WV % NT == 0, "U slab must split into whole per-thread float4s");
    static_assert(CK % 2 == 0 && CK * HR * 3 <= NT, "chunk shape");
    static_assert(SMEM * 4 <= 160 * 1024, "LDS");
};

#ifdef FRCNN_TUNING_FORMS
// The loop as first built (research builds only: FRCNN_CONV_WINO_LOOP=0) -- the bit reference of the shipped loop and the A/B arm of
// profiles/wino_loop_gate.txt.  One loop body with a run-time buffer index: 16 address VALU per 8-channel chunk, step 0 of every chunk waits
// for its own LDS reads, four instructions per DMA piece.
// ABL (timing ablations, WRONG results, only in -DFRCNN_TIMING_ABLATIONS builds: FRCNN_CONV_WINO_ABL): 1 MFMAs only, 2 + the fragment reads and
// the transform, 3 + the DMA issue (no per-chunk wait and barrier); 0 is the whole loop.
template <int CB, int TB, int CK, bool SOFF, int ABL>
__device__ __forceinline__ void wino_tile_loop_v0(float *smem, const float *__restrict__ x, const float *__restrict__ u, int Cin, int Cout, int H, int W,
                                               int x0, int y0, int co0, int c_begin, int c_end, f32x16 (&acc)[TB][4][CB]) {
    using Geo = WinoGeom<CB, TB, CK>;
    constexpr int NT = Geo::NT, BCO = Geo::BCO, HR = Geo::HR, WIT = Geo::WIT, HG = Geo::HG, HIT4 = Geo::HIT4, HVP = Geo::HVP, WBUF = Geo::WBUF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int HW = H * W;
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
    if constexpr (ABL != 0) issue(c_begin, 1);     // both buffers hold real data: the ablated loops never wait for a later chunk
    frcnn_wait_vmcnt<0>();
    frcnn_barrier_nofence();
    if (edge_fix) edge_zero(0);
    int cur = 0;
    [[maybe_unused]] float4 a_fix[CB];
    [[maybe_unused]] float v_fix[TB][4];
    if constexpr (ABL == 1) {                      // MFMAs only: operands read once, outside the loop
        const float4 *a_base = reinterpret_cast<const float4 *>(w_lds(0)) + (khalf * 4 + wave) * BCO + l31;
#pragma unroll
        for (int c = 0; c < CB; ++c) a_fix[c] = a_base[32 * c];
#pragma unroll
        for (int t = 0; t < TB; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) v_fix[t][j] = in_lds(0)[(khalf * HR + 2 * tr + 4 * t) * kWinoPitch + kWinoLead + 2 * tc + j];
    }
    for (int chunk = c_begin; chunk < c_end; ++chunk) {
        const bool more = chunk + 1 < c_end;
        if constexpr (ABL == 1) {
#pragma unroll
            for (int s = 0; s < CK / 2; ++s)
#pragma unroll
                for (int t = 0; t < TB; ++t)
#pragma unroll
                    for (int c = 0; c < CB; ++c) {
                        acc[t][0][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_fix[c].x, v_fix[t][0], acc[t][0][c], 0, 0, 0);
                        acc[t][1][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_fix[c].y, v_fix[t][1], acc[t][1][c], 0, 0, 0);
                        acc[t][2][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_fix[c].z, v_fix[t][2], acc[t][2][c], 0, 0, 0);
                        acc[t][3][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_fix[c].w, v_fix[t][3], acc[t][3][c], 0, 0, 0);
                    }
            cur ^= 1;
            continue;
        }
        if (more && (ABL == 0 || ABL == 3)) issue(chunk + 1, cur ^ 1);
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
                float tt[4], v[4];
                if constexpr (ABL == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) tt[j] = fmaf(sb, db[s & 1][t][j], da[s & 1][t][j]);
                    v[0] = tt[0] - tt[2]; v[1] = tt[1] + tt[2]; v[2] = tt[2] - tt[1]; v[3] = tt[1] - tt[3];
                } else {            // the same eight VALU as a block: without the chunk's barrier the compiler packs and shuffles the C++ form (70 VALU per chunk, not 48)
                    frcnn_wino_bt_row(sb, da[s & 1][t], db[s & 1][t], v);
                }
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
        if constexpr (ABL == 0) {
            frcnn_wait_vmcnt<0>();           // chunk + 1 has landed (nothing else is in flight)
            frcnn_barrier_nofence();         // ... for everybody, and everybody is done reading buffer `cur`
            if (edge_fix && more) edge_zero(cur ^ 1);
        } else {
            asm volatile("" ::: "memory");   // no instruction: the compiler keeps the chunk's shape (no LDS read carried into the next iteration)
        }
        cur ^= 1;
    }
    if constexpr (ABL != 0) {                // the epilogue reuses the staging buffers
        frcnn_wait_vmcnt<0>();
        frcnn_barrier_nofence();
    }
}
#endif  // FRCNN_TUNING_FORMS


// ---- loop forms.  kWinoLoop is the one every shipped kernel takes; research builds (-DFRCNN_TUNING_FORMS) carry the others under
// FRCNN_CONV_WINO_LOOP as the bit reference and the A/B arms of profiles/wino_loop_gate.txt.  0: wino_tile_loop_v0.  Bit 0: the chunk loop
// unrolled by two, so the buffer index -- every LDS base, every M0 value -- is a compile-time constant in each half, the row bases of every
// (buffer, step) stay in registers and no address VALU is left between the MFMAs; the transform is frcnn_wino_bt_row's eight scalar VALU.
// Bit 2: lean DMA issue (a wave's U pieces are contiguous: four per M0 write and wait state).  Bit 1: the chunk's wait and barrier stand in
// front of the LAST step's MFMAs, the next chunk's step-0 fragments are read under them, and the right-border zeros are written before that
// barrier by the lanes whose own pieces brought the floats along (no second barrier).  The gate's arms are 1, 5 and 7.  All forms run the
// same operations on the same values in the same order: the results are the same bits.
constexpr int kWinoLoop = 7;
template <int V> struct WinoInt { static constexpr int value = V; };

// The main loop of one output tile (BCO couts at co0, 4 TB rows at y0, 32 columns at x0) over the K chunks [c_begin, c_end): staging ring,
// input transform, MFMAs.  acc is zeroed here; the loop's last barrier leaves the staging buffers free for the epilogue.  The ring starts in
// buffer 0 at c_begin whatever c_begin is; the odd last chunk of a range runs after the loop.
template <int CB, int TB, int CK, bool SOFF, int LF>
__device__ __forceinline__ void wino_tile_loop(float *smem, const float *__restrict__ x, const float *__restrict__ u, int Cin, int Cout, int H, int W,
                                               int x0, int y0, int co0, int c_begin, int c_end, f32x16 (&acc)[TB][4][CB]) {
    using Geo = WinoGeom<CB, TB, CK>;
    constexpr int NT = Geo::NT, BCO = Geo::BCO, HR = Geo::HR, WIT = Geo::WIT, HG = Geo::HG, HIT4 = Geo::HIT4, HVP = Geo::HVP, WBUF = Geo::WBUF;
    constexpr int NSTEP = CK / 2;
    constexpr bool PREFETCH = (LF & 2) != 0, LEAN = (LF & 4) != 0;
    static_assert((LF & 1) != 0 && LF <= 7, "loop form");
    static_assert(!PREFETCH || NSTEP % 2 == 0, "the prefetched step 0 lands in fragment slot 0 while slot 1 is in use");
    static_assert(!LEAN || WIT % 4 == 0, "U pieces go in groups of four");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int HW = H * W;
    const int K4 = Cin * 4;

    const frcnn_buf_t xbuf = frcnn_make_buf(x, (uint32_t)((size_t)Cin * HW * sizeof(float)));
    const frcnn_buf_t ubuf = frcnn_make_buf(u, (uint32_t)((size_t)K4 * Cout * 4 * sizeof(float)));
    const uint32_t u_chunk_bytes = (uint32_t)(CK * 4 * Cout * 4) * 4u, x_chunk_bytes = (uint32_t)(CK * HW) * 4u;

    uint32_t woff[WIT], hoff[HIT4];
#pragma unroll
    for (int q = 0; q < WIT; ++q) {                          // LEAN: wave w stages float4s [w * WIT * 64, (w + 1) * WIT * 64) of the slab, piece q & 3 of a group
        const int v = LEAN ? (wave * WIT + q) * 64 + lane : tid + q * NT;      // through the immediate offset 1024 (q & 3): 16 v >= 1024 q keeps it non-negative
        const int row = v / BCO, c4 = v % BCO;
        woff[q] = (uint32_t)(row * Cout * 4 + (co0 + c4) * 4) * 4u - (LEAN ? (uint32_t)(q & 3) * 1024u : 0u);
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
    auto in_lds = [&](int buf) { return smem + 2 * WBUF + buf * HVP; };
    // a 16-byte group that straddles the right image border (W % 4 != 0) brings up to three floats of the next row along: zero them
    const int fix_lo = W - x0 + 4, fix_hi = (fix_lo + 3) & ~3;
    const bool edge_fix = (W & 3) != 0 && fix_lo > 0 && fix_lo < kWinoPitch;
    auto edge_zero = [&](int buf) {
        const int row = tid / 3, i = fix_lo + tid % 3;
        if (row < CK * HR && i < fix_hi) in_lds(buf)[row * kWinoPitch + i] = 0.0f;
        frcnn_barrier_nofence();
    };
    // the same zeros before the chunk's barrier instead of behind a second one: the lane whose own piece brought the straddling group along
    // overwrites them once its pieces have landed (after its vmcnt(0) wait), and the barrier that publishes the chunk publishes them too
    int zfix[HIT4];                                      // float index of this lane's straddling group in a halo buffer, or -1
#pragma unroll
    for (int q = 0; q < HIT4; ++q) {
        const int e4 = tid + q * NT;
        zfix[q] = (edge_fix && e4 < HG && e4 % 10 == (fix_lo >> 2)) ? e4 * 4 : -1;
    }
    auto edge_zero_own = [&](int buf) {
        const int k0 = fix_lo & 3;                       // 1 .. 3: floats k0 .. 3 of the group lie past the border
#pragma unroll
        for (int q = 0; q < HIT4; ++q)
            if (zfix[q] >= 0) {
                float *g = in_lds(buf) + zfix[q];
                if (k0 <= 1) g[1] = 0.0f;
                if (k0 <= 2) g[2] = 0.0f;
                g[3] = 0.0f;
            }
    };
    auto issue = [&](int chunk, auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        float *wl = smem + buf * WBUF, *il = smem + 2 * WBUF + buf * HVP;
        auto pieces = [&](frcnn_buf_t ub, frcnn_buf_t xb_, uint32_t wb, uint32_t xb) {
            if constexpr (LEAN) {
#pragma unroll
                for (int q = 0; q < WIT; q += 4)
                    frcnn_buf_load_lds_b128_x4(ub, wl + (wave * WIT + q) * 64 * 4, woff[q], woff[q + 1], woff[q + 2], woff[q + 3], wb);
            } else {
#pragma unroll
                for (int q = 0; q < WIT; ++q) frcnn_buf_load_lds_b128(ub, wl + (q * NT + wave * 64) * 4, woff[q], wb);
            }
#pragma unroll
            for (int q = 0; q < HIT4; ++q)
                if ((q + 1) * NT * 4 <= HVP || (wave * 64 + q * NT) * 4 < HVP)
                    frcnn_buf_load_lds_b128(xb_, il + (q * NT + wave * 64) * 4, hoff[q], xb);
        };
        if constexpr (SOFF) {               // Cin is a whole number of chunks: the chunk offset rides in the scalar offset
            pieces(ubuf, xbuf, (uint32_t)chunk * u_chunk_bytes, (uint32_t)chunk * x_chunk_bytes);
        } else {                            // ragged last chunk: per-chunk descriptors whose range ends at the tensor's end
            const long long wrem = (long long)(K4 - chunk * CK * 4) * Cout * 4, xrem = (long long)(Cin - chunk * CK) * HW;
            pieces(frcnn_make_buf(u + (size_t)chunk * CK * 4 * Cout * 4, (uint32_t)((wrem > 0 ? wrem : 0) * sizeof(float))),
                   frcnn_make_buf(x + (size_t)chunk * CK * HW, (uint32_t)((xrem > 0 ? xrem : 0) * sizeof(float))), 0, 0);
        }
    };

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
    const int d_off = (khalf * HR + 2 * tr) * kWinoPitch + kWinoLead + 2 * tc, a_off = (khalf * 4 + wave) * BCO + l31;

    // the row bases of every (buffer, step), pinned in registers: a step's ds_read2_b32 pairs reach 255 dwords, the next channel pair lies 480 away
    const float *bap[2][NSTEP], *bbp[2][NSTEP];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            bap[b][s] = frcnn_pin_lds(smem + 2 * WBUF + b * HVP + d_off + ra * kWinoPitch + 2 * s * HR * kWinoPitch);
            bbp[b][s] = frcnn_pin_lds(smem + 2 * WBUF + b * HVP + d_off + rb * kWinoPitch + 2 * s * HR * kWinoPitch);
        }
    float4 a[2][CB];
    float da[2][TB][4], db[2][TB][4];
    auto frag = [&](auto bufc, int s, int slot) {        // step s of the chunk in buffer `buf` -> fragment slot
        constexpr int buf = decltype(bufc)::value;
        const float *ba = bap[buf][s], *bb = bbp[buf][s];
        const float4 *a_base = reinterpret_cast<const float4 *>(smem + buf * WBUF) + a_off;
#pragma unroll
        for (int c = 0; c < CB; ++c) a[slot][c] = a_base[2 * s * 4 * BCO + 32 * c];
#pragma unroll
        for (int t = 0; t < TB; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                da[slot][t][j] = ba[4 * t * kWinoPitch + j];
                db[slot][t][j] = bb[4 * t * kWinoPitch + j];
            }
    };
    auto step = [&](int slot) {                          // the transform of one channel pair and its 4 CB TB MFMAs
#pragma unroll
        for (int t = 0; t < TB; ++t) {
            float v[4];                                   // tt = fmaf(sb, db, da);  v = {tt0 - tt2, tt1 + tt2, tt2 - tt1, tt1 - tt3}
            frcnn_wino_bt_row(sb, da[slot][t], db[slot][t], v);
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                const float4 av = a[slot][c];
                acc[t][0][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, v[0], acc[t][0][c], 0, 0, 0);
                acc[t][1][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, v[1], acc[t][1][c], 0, 0, 0);
                acc[t][2][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, v[2], acc[t][2][c], 0, 0, 0);
                acc[t][3][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, v[3], acc[t][3][c], 0, 0, 0);
            }
        }
    };
    // one chunk, in buffer `buf`; LAST: known at compile time to be the range's last chunk (more is false)
    auto half = [&](auto bufc, auto lastc, int chunk, const bool more) {
        constexpr int buf = decltype(bufc)::value;
        constexpr bool LAST = decltype(lastc)::value != 0;
        if (more) issue(chunk + 1, WinoInt<buf ^ 1>{});
        if constexpr (!PREFETCH) frag(bufc, 0, 0);
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            if (s + 1 < NSTEP) {
                frag(bufc, s + 1, (s + 1) & 1);
            } else if constexpr (PREFETCH) {
                frcnn_wait_vmcnt<0>();           // chunk + 1 has landed (nothing else is in flight)
                if (edge_fix && more) edge_zero_own(buf ^ 1);
                frcnn_barrier_nofence();         // ... for everybody, and everybody has read the last of buffer `buf` (the barrier drains the LDS reads)
                // the next chunk's step 0, under this chunk's last MFMAs (unconditional: behind a range's last chunk it reads stale floats nobody uses)
                if constexpr (!LAST) frag(WinoInt<buf ^ 1>{}, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);       // keep the prefetch ahead of this step's MFMAs
            step(s & 1);
        }
        if constexpr (!PREFETCH) {
            frcnn_wait_vmcnt<0>();
            frcnn_barrier_nofence();
            if (edge_fix && more) edge_zero(buf ^ 1);
        }
    };

    issue(c_begin, WinoInt<0>{});
    frcnn_wait_vmcnt<0>();
    if constexpr (PREFETCH) {
        if (edge_fix) edge_zero_own(0);
        frcnn_barrier_nofence();
    } else {
        frcnn_barrier_nofence();
        if (edge_fix) edge_zero(0);
    }
    if (c_begin >= c_end) return;
    if constexpr (PREFETCH) frag(WinoInt<0>{}, 0, 0);
    int chunk = c_begin;
    for (; chunk + 1 < c_end; chunk += 2) {              // one way out of the loop: the accumulators stay where they are
        half(WinoInt<0>{}, WinoInt<0>{}, chunk, true);
        half(WinoInt<1>{}, WinoInt<0>{}, chunk + 1, chunk + 2 < c_end);
    }
    if (chunk < c_end) half(WinoInt<0>{}, WinoInt<1>{}, chunk, false);  // the odd last chunk
}

// the loop form LF (0: wino_tile_loop_v0 with its timing ablation ABL, research builds only)
template <int CB, int TB, int CK, bool SOFF, int LF, int ABL>
__device__ __forceinline__ void wino_loop(float *smem, const float *__restrict__ x, const float *__restrict__ u, int Cin, int Cout, int H, int W, int x0,
                                          int y0, int co0, int c_begin, int c_end, f32x16 (&acc)[TB][4][CB]) {
    if constexpr (LF == 0) {
#ifdef FRCNN_TUNING_FORMS
        wino_tile_loop_v0<CB, TB, CK, SOFF, ABL>(smem, x, u, Cin, Cout, H, W, x0, y0, co0, c_begin, c_end, acc);
#else
        static_assert(LF != 0, "the first loop is a research form");
#endif
    } else {
        static_assert(ABL == 0, "the ablations are cut into the first loop");
        wino_tile_loop<CB, TB, CK, SOFF, LF>(smem, x, u, Cin, Cout, H, W, x0, y0, co0, c_begin, c_end, acc);
    }
}

// ---- epilogue, first half.  Z[w][0] = M[w][0] + M[w][1] + M[w][2],  Z[w][1] = M[w][1] - M[w][2] - M[w][3]  (M A, this wave's row), exchanged
// through LDS (the main loop's last barrier: nobody reads the staging buffers any more)
template <int CB, int TB>
__device__ __forceinline__ void wino_z_exchange(float *smem, const f32x16 (&acc)[TB][4][CB]) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float4 *z4 = reinterpret_cast<float4 *>(smem);
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
}

// ---- second half: Y = A^T Z.  Wave w finishes D registers 4w .. 4w+3 of every accumulator: couts co0 + 32 c + 8 w + 4 khalf + e, all four
// outputs of the lane's 2x2 block, for accumulator (t, c)
template <int CB, int TB>
__device__ __forceinline__ void wino_y_of_z(const float *smem, int t, int c, float (&yv)[4][2][2]) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float4 *z4 = reinterpret_cast<const float4 *>(smem);
    float4 zz[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) zz[r][q] = z4[(((r * 2 + q) * TB * CB + t * CB + c) * 4 + wave) * 64 + lane];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        auto comp = [&](const float4 &v) { return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w)); };
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            yv[e][0][q] = (comp(zz[0][q]) + comp(zz[1][q])) + comp(zz[2][q]);
            yv[e][1][q] = (comp(zz[1][q]) - comp(zz[2][q])) - comp(zz[3][q]);
        }
    }
}

// one 2x2 output block of cout `co` at (oy, ox), inside the map: + bias, ReLU / the fused pool (the block is exactly a pool window), store
__device__ __forceinline__ void wino_emit(float *__restrict__ y, const float (&yv)[2][2], float b, int co, int oy, int ox, int H, int W, bool relu,
                                          bool pool, bool has_r, bool has_d, size_t base) {
    if (pool) {
        const int OH = (H + 1) / 2, OW = (W + 1) / 2;
        float m = yv[0][0];
        if (has_r) m = fmaxf(m, yv[0][1]);
        if (has_d) m = fmaxf(m, yv[1][0]);
        if (has_r && has_d) m = fmaxf(m, yv[1][1]);
        y[(size_t)co * OH * OW + (size_t)(oy >> 1) * OW + (ox >> 1)] = fmaxf(m + b, 0.0f);       // max, +bias, ReLU commute
    } else {
        float *yo = y + base + (size_t)co * H * W + (size_t)oy * W + ox;
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

// mode bit 0: ReLU, bit 1: fused 2x2/2 max-pool (ceil mode; ReLU implied), bit 2: K piece -> raw Y (no bias) into y + piece * Cout*H*W
template <int CB, int TB, int CK, bool SOFF, int LF, int ABL>
__device__ __forceinline__ void wino_classic_body(float *smem, const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ bias,
                                                  float *__restrict__ y, int Cin, int Cout, int H, int W, int mode, int xtiles, int ytiles, int nchunks,
                                                  int piece_chunks) {
    using Geo = WinoGeom<CB, TB, CK>;
    constexpr int BCO = Geo::BCO;

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

    f32x16 acc[TB][4][CB];
    wino_loop<CB, TB, CK, SOFF, LF, ABL>(smem, x, u, Cin, Cout, H, W, x0, y0, co0, c_begin, c_end, acc);
    wino_z_exchange<CB, TB>(smem, acc);
    const bool relu = (mode & 1) != 0, pool = (mode & 2) != 0, partial = (mode & 4) != 0;
    const int tr = l31 >> 4, tc = l31 & 15;
#pragma unroll
    for (int t = 0; t < TB; ++t) {
        const int oy = y0 + 4 * t + 2 * tr, ox = x0 + 2 * tc;
        const bool in0 = oy < H && ox < W, has_r = ox + 1 < W, has_d = oy + 1 < H;
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            float yv[4][2][2];
            wino_y_of_z<CB, TB>(smem, t, c, yv);
            const int cob = co0 + 32 * c + 8 * wave + 4 * khalf;
            const float4 bq = partial ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4 *>(&bias[cob]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float b = e == 0 ? bq.x : (e == 1 ? bq.y : (e == 2 ? bq.z : bq.w));
                if (!in0) continue;
                wino_emit(y, yv[e], b, cob + e, oy, ox, H, W, relu, pool, has_r, has_d, partial ? (size_t)piece * Cout * HW : 0);
            }
        }
    }
}

template <int CB, int TB, int CK, int BPC, bool SOFF>
__global__ void __launch_bounds__(256, BPC)
conv_wino_f32_kernel(const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ bias, float *__restrict__ y,
                     int Cin, int Cout, int H, int W, int mode, int xtiles, int ytiles, int nchunks, int piece_chunks) {
    __shared__ __attribute__((aligned(16))) float smem[WinoGeom<CB, TB, CK>::SMEM];
    wino_classic_body<CB, TB, CK, SOFF, kWinoLoop, 0>(smem, x, u, bias, y, Cin, Cout, H, W, mode, xtiles, ytiles, nchunks, piece_chunks);
}
#ifdef FRCNN_TUNING_FORMS
// the same kernel around another loop form / timing ablation (research builds: FRCNN_CONV_WINO_LOOP, FRCNN_CONV_WINO_ABL)
template <int CB, int TB, int CK, int BPC, bool SOFF, int LF, int ABL>
__global__ void __launch_bounds__(256, BPC)
wino_lab_f32_kernel(const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ bias, float *__restrict__ y,
                    int Cin, int Cout, int H, int W, int mode, int xtiles, int ytiles, int nchunks, int piece_chunks) {
    __shared__ __attribute__((aligned(16))) float smem[WinoGeom<CB, TB, CK>::SMEM];
    wino_classic_body<CB, TB, CK, SOFF, LF, ABL>(smem, x, u, bias, y, Cin, Cout, H, W, mode, xtiles, ytiles, nchunks, piece_chunks);
}
#endif

// ---- the form that finishes its K split itself (frcnn_conv3x3_wino_sk_f32).  Work distribution as conv.hip's stream-K: the unit is one
// 8-channel chunk of one output tile, total = ntiles * nchunks units, workgroup g of G takes the contiguous range [g*total/G, (g+1)*total/G)
// -- or, with pieces > 0 (FRCNN_CONV_WINO_SK_PIECES), the classic launch's partition: tile g / pieces, its chunks
// [p * piece_chunks, (p+1) * piece_chunks) for p = g % pieces.  A workgroup may end one tile, own whole tiles and begin another; the staging
// ring restarts at every tile boundary.  A tile that one workgroup owns whole takes the normal epilogue and touches no workspace.  A piece
// of a shared tile runs the output transform and stores its raw Y lane-linear (8 float4 per thread: 64 couts x 4 x 32 floats = 32 KB) in
// one of its workgroup's two slots (0: the piece it starts with, 1: the piece it ends with) as write-through 16-byte stores, drains,
// barriers and takes a ticket on the tile's counter; the holder of ticket P-1 acquires, puts the counter back to zero and adds the P
// pieces in ascending piece order (s = y_0; s += y_k, wino_combine_kernel's order), then bias / ReLU / pool through the same code as the
// main epilogue.  Nobody waits for anybody: correctness does not depend on residency or arrival order.
template <bool SOFF, int LF, int ABL>
__device__ __forceinline__ void wino_sk_body(float *smem, const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ bias,
                                             float *__restrict__ y, int Cin, int Cout, int H, int W, int mode, int xtiles, int ytiles, int nchunks,
                                             long long total, int pieces, int piece_chunks, float *__restrict__ slots, int *__restrict__ tile_counters) {
    constexpr int CB = 2, TB = 1, CK = 8;
    using Geo = WinoGeom<CB, TB, CK>;
    constexpr int BCO = Geo::BCO, NT = Geo::NT;
    constexpr int SLOT_V = TB * CB * 4;                      // float4s per thread and slot
    constexpr size_t kSlotFloats = (size_t)NT * SLOT_V * 4;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, khalf = lane >> 5;
    const int tr = l31 >> 4, tc = l31 & 15;
    const int npx = xtiles * ytiles;
    // XCD-aware placement: XCD x gets the x-th contiguous eighth of the ranges, so the ranges of one cout block meet its slice of U in one L2
    const long long G = gridDim.x;
    long long g = blockIdx.x;
    {
        const long long xcd = g & 7, q = G >> 3, r = G & 7;
        g = xcd * q + (xcd < r ? xcd : r) + (g >> 3);
    }
    auto start_of = [&](long long b) -> long long {          // first unit of workgroup b's range (b == G: total)
        if (pieces > 0) {
            const long long c = (b % pieces) * (long long)piece_chunks;
            return (b / pieces) * nchunks + (c < nchunks ? c : nchunks);
        }
        return b * total / G;
    };
    auto owner_of = [&](long long i) -> long long {          // the workgroup whose range contains unit i
        if (pieces > 0) return (i / nchunks) * pieces + (i % nchunks) / piece_chunks;
        long long b = i * G / total;
        while (start_of(b + 1) <= i) ++b;
        while (start_of(b) > i) --b;
        return b;
    };
    const long long it_begin = start_of(g), it_end = start_of(g + 1);
    const bool relu = (mode & 1) != 0, pool = (mode & 2) != 0;

    for (long long it = it_begin; it < it_end;) {
        const int tile = (int)(it / nchunks);
        const int c_begin = (int)(it - (long long)tile * nchunks);
        const int c_end = (int)((long long)nchunks < c_begin + (it_end - it) ? (long long)nchunks : c_begin + (it_end - it));
        const int pxt = tile % npx, cot = tile / npx;
        const int x0 = (pxt % xtiles) * 32, y0 = (pxt / xtiles) * 4 * TB, co0 = cot * BCO;
        if (it != it_begin) __syncthreads();                 // the previous tile's epilogue is done with the LDS the ring restarts in

        f32x16 acc[TB][4][CB];
        wino_loop<CB, TB, CK, SOFF, LF, ABL>(smem, x, u, Cin, Cout, H, W, x0, y0, co0, c_begin, c_end, acc);
        wino_z_exchange<CB, TB>(smem, acc);

        const bool whole = c_begin == 0 && c_end == nchunks;
        float4 sum[SLOT_V];                                  // raw Y of this thread's 2x2 blocks: [t][c][e] x (y00, y01, y10, y11)
#pragma unroll
        for (int t = 0; t < TB; ++t)
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                float yv[4][2][2];
                wino_y_of_z<CB, TB>(smem, t, c, yv);
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[(t * CB + c) * 4 + e] = make_float4(yv[e][0][0], yv[e][0][1], yv[e][1][0], yv[e][1][1]);
            }
        bool finish = true;
        if (!whole) {
            const long long t_first = (long long)tile * nchunks;
            const long long g_first = owner_of(t_first), g_last = owner_of(t_first + nchunks - 1);
            const int P = (int)(g_last - g_first + 1);
            const int my_slot = (it == it_begin) ? 0 : 1;
            const frcnn_buf_t pbuf = frcnn_make_buf(slots + ((size_t)g * 2 + my_slot) * kSlotFloats, (uint32_t)(kSlotFloats * sizeof(float)));
#pragma unroll
            for (int v = 0; v < SLOT_V; ++v)                 // + 0.0f: the classic pieces store Y + a zero bias (a -0 becomes +0 there too)
                frcnn_buf_store_f32x4_wt(pbuf, (uint32_t)((v * NT + tid) * 16),
                                         make_float4(sum[v].x + 0.0f, sum[v].y + 0.0f, sum[v].z + 0.0f, sum[v].w + 0.0f));
            // write-through stores need no release fence: every wave drains, barrier, one ticket (cdna_hip_programming.md G16 R1)
            frcnn_drain_vmem();
            __syncthreads();                                 // ... and everybody has read its Z: the ticket travels through smem[0]
            int *s_ticket = reinterpret_cast<int *>(smem);
            if (tid == 0) *s_ticket = frcnn_ticket(&tile_counters[tile]);
            __syncthreads();
            finish = (*s_ticket == P - 1);                   // workgroup-uniform
            if (finish) {
                if (tid == 0) {
                    frcnn_acquire_agent();
                    frcnn_counter_reset(&tile_counters[tile]);      // all P tickets are drawn: the page is zero again for the next launch
                }
                __syncthreads();
                // ALL P pieces in piece order, this workgroup's own one read back from its slot: the sum does not depend on who arrived last
                for (int q = 0; q < P; ++q) {
                    const long long b = g_first + q;
                    const int slot = (q == 0 && start_of(b) != t_first) ? 1 : 0;
                    const float4 *piece = reinterpret_cast<const float4 *>(slots + ((size_t)b * 2 + slot) * kSlotFloats);
                    float4 v[SLOT_V];
#pragma unroll
                    for (int e = 0; e < SLOT_V; ++e) v[e] = piece[(size_t)e * NT + tid];       // all loads of a piece in flight
#pragma unroll
                    for (int e = 0; e < SLOT_V; ++e) frcnn_pin(v[e]);
#pragma unroll
                    for (int e = 0; e < SLOT_V; ++e) {
                        if (q == 0) sum[e] = v[e];
                        else { sum[e].x += v[e].x; sum[e].y += v[e].y; sum[e].z += v[e].z; sum[e].w += v[e].w; }
                    }
                }
            }
        }
        if (finish) {
#pragma unroll
            for (int t = 0; t < TB; ++t) {
                const int oy = y0 + 4 * t + 2 * tr, ox = x0 + 2 * tc;
                const bool in0 = oy < H && ox < W, has_r = ox + 1 < W, has_d = oy + 1 < H;
#pragma unroll
                for (int c = 0; c < CB; ++c) {
                    const int cob = co0 + 32 * c + 8 * wave + 4 * khalf;
                    const float4 bq = *reinterpret_cast<const float4 *>(&bias[cob]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float b = e == 0 ? bq.x : (e == 1 ? bq.y : (e == 2 ? bq.z : bq.w));
                        const float4 sv = sum[(t * CB + c) * 4 + e];
                        const float yv[2][2] = {{sv.x, sv.y}, {sv.z, sv.w}};
                        if (!in0) continue;
                        wino_emit(y, yv, b, cob + e, oy, ox, H, W, relu, pool, has_r, has_d, 0);
                    }
                }
            }
        }
        it += c_end - c_begin;
    }
}

template <bool SOFF>
__global__ void __launch_bounds__(256, 2)
wino_sk_f32_kernel(const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ bias, float *__restrict__ y,
                   int Cin, int Cout, int H, int W, int mode, int xtiles, int ytiles, int nchunks, long long total, int pieces, int piece_chunks,
                   float *__restrict__ slots, int *__restrict__ tile_counters) {
    __shared__ __attribute__((aligned(16))) float smem[WinoGeom<2, 1, 8>::SMEM];
    wino_sk_body<SOFF, kWinoLoop, 0>(smem, x, u, bias, y, Cin, Cout, H, W, mode, xtiles, ytiles, nchunks, total, pieces, piece_chunks, slots, tile_counters);
}
#ifdef FRCNN_TUNING_FORMS
template <bool SOFF, int LF, int ABL>
__global__ void __launch_bounds__(256, 2)
wino_lab_sk_f32_kernel(const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ bias, float *__restrict__ y,
                       int Cin, int Cout, int H, int W, int mode, int xtiles, int ytiles, int nchunks, long long total, int pieces, int piece_chunks,
                       float *__restrict__ slots, int *__restrict__ tile_counters) {
    __shared__ __attribute__((aligned(16))) float smem[WinoGeom<2, 1, 8>::SMEM];
    wino_sk_body<SOFF, LF, ABL>(smem, x, u, bias, y, Cin, Cout, H, W, mode, xtiles, ytiles, nchunks, total, pieces, piece_chunks, slots, tile_counters);
}
#endif

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

// FRCNN_CONV_WINO_LOOP: the loop form of every launch (-1: not in this build).  The product library carries kWinoLoop alone and refuses every
// other value; research builds (-DFRCNN_TUNING_FORMS) also carry 0 (the first loop: every shape) and the gate's arms 1, 5, 7 (whole 8-channel chunks)
static int wino_loop_form() {
    const char *v = frcnn_tune("FRCNN_CONV_WINO_LOOP");
    if (!v) return kWinoLoop;
    const int f = atoi(v);
#ifdef FRCNN_TUNING_FORMS
    return (f == 0 || f == 1 || f == 5 || f == 7) ? f : -1;
#else
    return f == kWinoLoop ? f : -1;
#endif
}
// FRCNN_CONV_WINO_ABL: a timing ablation of the first loop (WRONG results; -DFRCNN_TUNING_FORMS -DFRCNN_TIMING_ABLATIONS builds with FRCNN_CONV_WINO_LOOP=0)
static int wino_loop_ablation() {
    const int a = frcnn_tune_int("FRCNN_CONV_WINO_ABL", 0);
#if defined(FRCNN_TUNING_FORMS) && defined(FRCNN_TIMING_ABLATIONS)
    return (a >= 0 && a <= 3) ? a : -1;
#else
    return a == 0 ? 0 : -1;
#endif
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
    const int lf = wino_loop_form(), abl = wino_loop_ablation();
    if (lf < 0 || abl < 0) return FRCNN_ERR_INVALID;
    const bool soff = Cin % CK == 0;
#define FRCNN_WINO_LAUNCH(...) hipLaunchKernelGGL(HIP_KERNEL_NAME(__VA_ARGS__), dim3(G), dim3(256), 0, stream, x, u, bias, out, Cin, Cout, H, W, kmode, \
                                                  p.xtiles, p.ytiles, p.nchunks, p.piece_chunks)
    if (lf == kWinoLoop && abl == 0) {
        if (soff) FRCNN_WINO_LAUNCH(conv_wino_f32_kernel<CB, TB, CK, BPC, true>);
        else FRCNN_WINO_LAUNCH(conv_wino_f32_kernel<CB, TB, CK, BPC, false>);
    }
#ifdef FRCNN_TUNING_FORMS
    else if (lf == 0 && abl == 0) {
        if (soff) FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, CK, BPC, true, 0, 0>);
        else FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, CK, BPC, false, 0, 0>);
    } else if (CK == 8 && soff && abl == 0) {          // the gate's arms: whole 8-channel chunks only
        if (lf == 1) FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, 8, BPC, true, 1, 0>);
        else if (lf == 5) FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, 8, BPC, true, 5, 0>);
        else FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, 8, BPC, true, 7, 0>);
    }
#ifdef FRCNN_TIMING_ABLATIONS
    else if (CK == 8 && soff && lf == 0) {
        if (abl == 1) FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, 8, BPC, true, 0, 1>);
        else if (abl == 2) FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, 8, BPC, true, 0, 2>);
        else FRCNN_WINO_LAUNCH(wino_lab_f32_kernel<CB, TB, 8, BPC, true, 0, 3>);
    }
#endif
#endif
    else return FRCNN_ERR_INVALID;                      // a form this build does not carry: refused, never substituted
#undef FRCNN_WINO_LAUNCH
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


// ---- the in-kernel form: plan, pick, launch
constexpr size_t kWinoSkCounterPage = 64 * 1024;               // one int per tile; zeroed once, every launch leaves it zero
constexpr size_t kWinoSkSlotBytes = 64 * 4 * 32 * sizeof(float);

struct WinoSkPlan { WinoPlan t; long long total; int G, pieces; bool classic, shared, self_cleaning; size_t counters_bytes, ws_bytes; };

// Which shapes take the in-kernel form (profiles/wino_sk_gate.txt): those the classic launch splits (fewer tiles than two rounds of the
// chip's 2 x CU workgroup slots, K long enough to split) -- with the classic launch's pieces by default, with one contiguous range per
// slot (G = min(total, 2 x CU count)) under FRCNN_CONV_WINO_SK_BALANCE=1.  Everything else keeps the classic whole-tile launch.  FRCNN_CONV_WINO_SK_G / FRCNN_CONV_WINO_SK_PIECES force the form and its partition on any shape
// (FRCNN_CONV_WINO_SK_PIECES=-1: on the shapes the classic launch splits, with its piece count).
static WinoSkPlan plan_wino_sk(int Cin, int Cout, int H, int W) {
    WinoSkPlan p;
    const int forced_g = frcnn_tune_int("FRCNN_CONV_WINO_SK_G", 0);
    int forced_p = frcnn_tune_int("FRCNN_CONV_WINO_SK_PIECES", 0);
    const int classic_pieces = pick_wino_pieces(1, Cin, Cout, H, W);
    if (forced_p < 0) forced_p = classic_pieces > 1 ? classic_pieces : 0;      // -1: the classic rule's own count per shape (an unsplit shape stays classic)
    // The adopted partition is the classic launch's own (bit-identical outputs: the proposals' coordinates feel every regrouping of the K sum
    // in their last bits); FRCNN_CONV_WINO_SK_BALANCE=1 takes one balanced range per workgroup slot instead (faster: profiles/wino_sk_gate.txt)
    const bool balance = frcnn_tune_int("FRCNN_CONV_WINO_SK_BALANCE", 0) == 1;
    if (forced_p == 0 && forced_g <= 0 && !balance && classic_pieces > 1) forced_p = classic_pieces;
    p.t = plan_wino<2, 1, 8>(Cin, Cout, H, W, forced_p > 0 ? forced_p : 1);
    p.total = (long long)p.t.ntiles * p.t.nchunks;
    p.classic = false;
    p.pieces = 0;
    if (forced_p > 0) {
        p.pieces = p.t.pieces;
        p.G = p.t.ntiles * p.t.pieces;
        p.shared = p.t.pieces > 1;
    } else {
        const long long slots = 2LL * frcnn_cu_count();
        if (forced_g > 0) p.G = (int)(forced_g < p.total ? forced_g : p.total);
        else if (classic_pieces > 1) p.G = (int)(slots < p.total ? slots : p.total);
        else { p.G = p.t.ntiles; p.classic = true; }
        p.shared = p.G != p.t.ntiles;
    }
    const size_t need = frcnn_align256((size_t)p.t.ntiles * sizeof(int));
    p.counters_bytes = need > kWinoSkCounterPage ? need : kWinoSkCounterPage;
    p.self_cleaning = need <= kWinoSkCounterPage;               // more than 16384 tiles: the counters are zeroed per launch instead
    p.ws_bytes = p.shared ? p.counters_bytes + (size_t)p.G * 2 * kWinoSkSlotBytes : 0;
    return p;
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

size_t frcnn_conv_wino_sk_workspace_bytes(int Cin, int Cout, int H, int W) {
    if (Cin < 1 || Cout < 1 || H < 1 || W < 1 || (Cout % 64) != 0) return 0;
    const WinoSkPlan p = plan_wino_sk(Cin, Cout, H, W);
    return p.ws_bytes > kWinoSkCounterPage ? p.ws_bytes : kWinoSkCounterPage;
}

int frcnn_conv_wino_sk_workspace_init(void *workspace, size_t workspace_bytes, void *stream) {
    if (!workspace || workspace_bytes < kWinoSkCounterPage) return FRCNN_ERR_INVALID;
    FRCNN_HIP_TRY(hipMemsetAsync(workspace, 0, kWinoSkCounterPage, (hipStream_t)stream));
    return FRCNN_OK;
}

// the arguments of frcnn_conv3x3_wino_f32; shapes that share no tile (plan_wino_sk) need no workspace and take the classic launch
int frcnn_conv3x3_wino_sk_f32(const float *x, const float *u, const float *bias, float *y, int Cin, int Cout, int H, int W, int act,
                              void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !u || !bias || !y || Cin < 1 || Cout < 1 || H < 1 || W < 1 || (Cout % 64) != 0) return FRCNN_ERR_INVALID;
    if (act != 0 && act != 1 && act != 4) return FRCNN_ERR_INVALID;
    if ((size_t)Cin * H * W * 4 >= (1ull << 31) || (size_t)Cin * 16 * Cout * 4 >= (1ull << 31)) return FRCNN_ERR_INVALID;   // 32-bit buffer offsets
    const int mode = act == 4 ? 3 : act;
    const WinoSkPlan p = plan_wino_sk(Cin, Cout, H, W);
    const int lf = wino_loop_form(), abl = wino_loop_ablation();
    if (lf < 0 || abl < 0) return FRCNN_ERR_INVALID;
    if (p.classic) return launch_wino<2, 1, 8, 2>(x, u, bias, y, Cin, Cout, H, W, mode, 1, nullptr, 0, stream);
    if (p.shared && (!workspace || workspace_bytes < p.ws_bytes)) return FRCNN_ERR_INVALID;
    int *counters = p.shared ? (int *)workspace : nullptr;
    float *slots = p.shared ? (float *)((char *)workspace + p.counters_bytes) : nullptr;
    if (p.shared && !p.self_cleaning) FRCNN_HIP_TRY(hipMemsetAsync(counters, 0, p.counters_bytes, stream));
    const bool soff = Cin % 8 == 0;
#define FRCNN_WINO_LAUNCH(...) hipLaunchKernelGGL(HIP_KERNEL_NAME(__VA_ARGS__), dim3(p.G), dim3(256), 0, stream, x, u, bias, y, Cin, Cout, H, W, mode, p.t.xtiles, \
                                                  p.t.ytiles, p.t.nchunks, p.total, p.pieces, p.t.piece_chunks, slots, counters)
    if (lf == kWinoLoop && abl == 0) {
        if (soff) FRCNN_WINO_LAUNCH(wino_sk_f32_kernel<true>);
        else FRCNN_WINO_LAUNCH(wino_sk_f32_kernel<false>);
    }
#ifdef FRCNN_TUNING_FORMS
    else if (lf == 0 && abl == 0) {
        if (soff) FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<true, 0, 0>);
        else FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<false, 0, 0>);
    } else if (soff && abl == 0) {
        if (lf == 1) FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<true, 1, 0>);
        else if (lf == 5) FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<true, 5, 0>);
        else FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<true, 7, 0>);
    }
#ifdef FRCNN_TIMING_ABLATIONS
    else if (soff && lf == 0) {
        if (abl == 1) FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<true, 0, 1>);
        else if (abl == 2) FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<true, 0, 2>);
        else FRCNN_WINO_LAUNCH(wino_lab_sk_f32_kernel<true, 0, 3>);
    }
#endif
#endif
    else return FRCNN_ERR_INVALID;
#undef FRCNN_WINO_LAUNCH
    return frcnn_launch_status();
}

}  // extern "C"
