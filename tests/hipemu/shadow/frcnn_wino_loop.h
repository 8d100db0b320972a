// Emulator stand-in for csrc/frcnn_wino_loop.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <frcnn_buffer.h>
static inline void frcnn_buf_load_lds_b128_x4(frcnn_buf_t b, void *lds_wave_base, uint32_t off0, uint32_t off1, uint32_t off2, uint32_t off3, uint32_t soff) {
    // piece i: the immediate 1024 i joins the per-lane offset BEFORE the range check (a sum past 32 bits is out of range) and moves the LDS destination along
    const uint32_t off[4] = {off0, off1, off2, off3};
    for (int i = 0; i < 4; ++i) {
        const uint64_t o = (uint64_t)off[i] + 1024u * i;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 4; ++k)
            if (o + 4 * k + 4 <= b.bytes) memcpy(&v[k], b.base + o + soff + 4 * k, 4);
        hipemu::dma_deposit((char *)lds_wave_base + 1024 * i + 16 * (threadIdx.x & 63), v, 16);
    }
}
static inline void frcnn_wino_bt_row(float sb, const float (&da)[4], const float (&db)[4], float (&v)[4]) {
    float tt[4];
    for (int j = 0; j < 4; ++j) tt[j] = fmaf(sb, db[j], da[j]);
    v[0] = tt[0] - tt[2]; v[1] = tt[1] + tt[2]; v[2] = tt[2] - tt[1]; v[3] = tt[1] - tt[3];
}
static inline const float *frcnn_pin_lds(const float *p) { return p; }
