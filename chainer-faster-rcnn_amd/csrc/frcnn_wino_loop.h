// frcnn_wino_loop.h -- what the Winograd chunk loop (csrc/conv_wino.hip, wino_tile_loop) needs beside frcnn_buffer.h and frcnn_intrin.h: the
// four-piece LDS-DMA issue (a sibling of frcnn_buf_load_lds_b128, whose contract stays as it is), the row transform as a block of scalar VALU,
// and the pin that keeps an LDS address in its register.  (the test emulator shadows this header with a host version)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <frcnn_buffer.h>

// Four pieces whose LDS destinations lie 1 KB apart (lds_wave_base + 1024 i + 16 * lane) behind ONE M0 write and one wait state: piece i rides
// on the instruction's immediate offset 1024 i, which the hardware adds to the LDS address AND to the buffer offset (before the range check).  So
// the caller passes byte_off_i = (source offset of piece i) - 1024 i, which must not be negative for a lane that is in range; a lane with
// nothing to fetch passes kBufOob itself (bit 31 stays set under the immediate).  6 instructions per 4 KB where four single pieces take 12.
__device__ __forceinline__ void frcnn_buf_load_lds_b128_x4(frcnn_buf_t b, void *lds_wave_base, uint32_t byte_off0, uint32_t byte_off1, uint32_t byte_off2,
                                                           uint32_t byte_off3, uint32_t soff) {
    const uint32_t la = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)lds_wave_base;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %1, %5, %6 offen lds\n\t"
                 "buffer_load_dwordx4 %2, %5, %6 offen offset:1024 lds\n\t"
                 "buffer_load_dwordx4 %3, %5, %6 offen offset:2048 lds\n\t"
                 "buffer_load_dwordx4 %4, %5, %6 offen offset:3072 lds"
                 :
                 : "s"(la), "v"(byte_off0), "v"(byte_off1), "v"(byte_off2), "v"(byte_off3), "s"(b), "s"(soff)
                 : "memory", "m0");
}

// One row of the Winograd F(2x2,3x3) input transform (csrc/conv_wino.hip): tt_j = fmaf(sb, db_j, da_j), v = {tt0 - tt2, tt1 + tt2, tt2 - tt1, tt1 - tt3},
// as exactly eight scalar VALU instructions.  Written as one asm block because the compiler otherwise pairs the fmas into v_pk_fma_f32 (+ the
// v_mov that gather its operands) wherever its SLP pass finds two of them in one block, and a packed fp32 VALU instruction beside MFMAs costs
// more than the two scalar ones (MI355X_MICROARCH.md, "price of one filler beside MFMAs").  v feeds MFMAs, and the compiler's hazard recognizer
// does not see a VALU write inside an asm string: the two wait states a VALU result needs before an MFMA reads it are the block's last line.
__device__ __forceinline__ void frcnn_wino_bt_row(float sb, const float (&da)[4], const float (&db)[4], float (&v)[4]) {
    float t1;
    asm("v_fma_f32 %0, %5, %10, %6\n\t"
        "v_fma_f32 %4, %5, %11, %7\n\t"
        "v_fma_f32 %2, %5, %12, %8\n\t"
        "v_fma_f32 %3, %5, %13, %9\n\t"
        "v_sub_f32 %0, %0, %2\n\t"
        "v_add_f32 %1, %4, %2\n\t"
        "v_sub_f32 %2, %2, %4\n\t"
        "v_sub_f32 %3, %4, %3\n\t"
        "s_nop 1"
        : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(t1)
        : "v"(sb), "v"(da[0]), "v"(da[1]), "v"(da[2]), "v"(da[3]), "v"(db[0]), "v"(db[1]), "v"(db[2]), "v"(db[3]));
}
// Pins an LDS address in a register: the compiler holds THIS value across a loop instead of re-deriving it from a neighbour with a v_add at every use
// (it folds base + constant into the instruction where the offset field reaches, and sinks the add next to the use where it does not)
__device__ __forceinline__ const float *frcnn_pin_lds(const float *p) {
    uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const float *)p;
    asm volatile("" : "+v"(a));
    return (const float *)(__attribute__((address_space(3))) const float *)(uintptr_t)a;
}
