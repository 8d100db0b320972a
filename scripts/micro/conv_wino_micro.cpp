// conv_wino_micro.cpp -- the Winograd F(2x2,3x3) fp32 convolution (frcnn_conv3x3_wino_f32) against the direct one (frcnn_conv_f32_ex) on the
// VGG-16 layer shapes at 600 x 1000, without torch.  Per layer and arm: a captured graph of 5 back-to-back launches (outputs rotating over 3
// buffers), bursts of graph launches between two events; the two arms alternate, `CONV_MICRO_REPS` rounds (default 3), median per arm.
// Also the largest |wino - direct| / max|direct| per layer (a sanity check; tests/ hold the accuracy bars).
// --sk: the gate of the in-kernel K split (profiles/wino_sk_gate.txt) instead: the classic entry (kernel + wino_combine_kernel) against
// frcnn_conv3x3_wino_sk_f32 with G = CU count, G = 2 x CU count and the classic partition (FRCNN_CONV_WINO_SK_PIECES), all arms interleaved;
// per arm the median and the spread (min .. max) of the repeats.
// --loop: the gate of the chunk-loop forms (profiles/wino_loop_gate.txt; research build of the library, -DFRCNN_TUNING_FORMS): the library's own entry
// (frcnn_conv3x3_wino_sk_f32) under FRCNN_CONV_WINO_LOOP = 0 (the first loop), 1, 5, 7, all arms interleaved, and every arm's output against arm 0's
// bit for bit.  --abl: the timing ablations of the first loop (-DFRCNN_TIMING_ABLATIONS too; WRONG results by design): FRCNN_CONV_WINO_ABL = 1 (MFMAs
// only), 2 (+ fragment reads and transform), 3 (+ DMA issue), 0 (the whole loop), interleaved.  Each reading: the median of three batches of bursts.
// Usage: conv_wino_micro [--sk | --loop | --abl] [layer ...]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <string>
#include <vector>
#include "frcnn_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

struct Layer { const char *name; int ci, co, h, w, pool, times; };
static const Layer kLayers[] = {
    {"conv1_2", 64, 64, 600, 1000, 1, 1}, {"conv2_1", 64, 128, 300, 500, 0, 1}, {"conv2_2", 128, 128, 300, 500, 1, 1}, {"conv3_1", 128, 256, 150, 250, 0, 1},
    {"conv3_2", 256, 256, 150, 250, 0, 1}, {"conv3_3", 256, 256, 150, 250, 1, 1}, {"conv4_1", 256, 512, 75, 125, 0, 1}, {"conv4_2", 512, 512, 75, 125, 0, 1},
    {"conv4_3", 512, 512, 75, 125, 1, 1}, {"conv5_1", 512, 512, 38, 63, 0, 4}};

static int sk_gate(const std::vector<std::string> &want) {
    hipStream_t s; CK(hipStreamCreate(&s));
    const int burst = getenv("CONV_MICRO_BURST") ? atoi(getenv("CONV_MICRO_BURST")) : 8;
    const int reps = getenv("CONV_MICRO_REPS") ? atoi(getenv("CONV_MICRO_REPS")) : 3;
    int cus = 0; CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    std::mt19937 g(1); std::uniform_real_distribution<float> u(-1.f, 1.f);
    constexpr int NA = 4;
    printf("# us per launch, median [min .. max] of %d interleaved bursts of %d x 5 launches; %d CUs\n", reps * 3, burst, cus);
    printf("# %-8s %-22s %-26s %-26s %-26s %-26s\n", "layer", "shape", "classic (kernel+combine)", "sk G=CUs", "sk G=2xCUs", "sk classic partition");
    for (const Layer &L : kLayers) {
        if (!want.empty() && std::find(want.begin(), want.end(), std::string(L.name)) == want.end()) continue;
        const int OH = L.pool ? (L.h + 1) / 2 : L.h, OW = L.pool ? (L.w + 1) / 2 : L.w;
        const size_t nx = (size_t)L.ci * L.h * L.w, nw = (size_t)9 * L.co * L.ci, ny = (size_t)L.co * OH * OW;
        std::vector<float> hx(nx), hw(nw), hb(L.co);
        for (auto &e : hx) e = u(g);
        for (auto &e : hw) e = 0.05f * u(g);
        for (auto &e : hb) e = 0.1f * u(g);
        float *dx, *dw, *du, *db, *dy[3]; void *ws[NA]; size_t wsb[NA];
        CK(hipMalloc(&dx, nx * 4)); CK(hipMalloc(&dw, nw * 4)); CK(hipMalloc(&du, nw / 9 * 16 * 4)); CK(hipMalloc(&db, L.co * 4));
        for (auto &p : dy) CK(hipMalloc(&p, ny * 4));
        CK(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(db, hb.data(), L.co * 4, hipMemcpyHostToDevice));
        if (frcnn_wino_pack_w(dw, L.co, L.ci, 0, du, s) != 0) { printf("pack failed\n"); return 1; }
        const size_t classic_ws = frcnn_conv_wino_workspace_bytes(L.ci, L.co, L.h, L.w);
        const int pieces = classic_ws > 256 ? (int)(classic_ws / ((size_t)L.co * L.h * L.w * 4)) : 1;      // exactly the slabs
        char v1[16], v2[16], v3[16];
        snprintf(v1, sizeof v1, "%d", cus); snprintf(v2, sizeof v2, "%d", 2 * cus); snprintf(v3, sizeof v3, "%d", pieces);
        const char *key[NA] = {nullptr, "FRCNN_CONV_WINO_SK_G", "FRCNN_CONV_WINO_SK_G", "FRCNN_CONV_WINO_SK_PIECES"};
        const char *val[NA] = {nullptr, v1, v2, v3};
        hipGraphExec_t ge[NA];
        std::vector<float> y0(ny), y1(ny);
        double md[NA] = {0, 0, 0, 0};
        for (int arm = 0; arm < NA; ++arm) {
            if (key[arm] && frcnn_set_tuning(key[arm], val[arm]) != 0) { printf("set_tuning failed\n"); return 1; }
            wsb[arm] = arm == 0 ? classic_ws : frcnn_conv_wino_sk_workspace_bytes(L.ci, L.co, L.h, L.w);
            CK(hipMalloc(&ws[arm], wsb[arm]));
            if (arm > 0 && frcnn_conv_wino_sk_workspace_init(ws[arm], wsb[arm], s) != 0) { printf("workspace init failed\n"); return 1; }
            CK(hipStreamSynchronize(s));
            hipGraph_t gr;
            CK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
            bool ok = true;
            for (int i = 0; i < 5; ++i)
                ok = ok && (arm == 0 ? frcnn_conv3x3_wino_f32(dx, du, db, dy[i % 3], L.ci, L.co, L.h, L.w, L.pool ? 4 : 1, ws[arm], wsb[arm], s)
                                     : frcnn_conv3x3_wino_sk_f32(dx, du, db, dy[i % 3], L.ci, L.co, L.h, L.w, L.pool ? 4 : 1, ws[arm], wsb[arm], s)) == 0;
            CK(hipStreamEndCapture(s, &gr));
            if (key[arm]) frcnn_set_tuning(key[arm], nullptr);
            if (!ok) { printf("%s: launch refused (arm %d)\n", L.name, arm); return 1; }
            CK(hipGraphInstantiate(&ge[arm], gr, nullptr, nullptr, 0));
            CK(hipGraphDestroy(gr));
            for (int i = 0; i < 2; ++i) CK(hipGraphLaunch(ge[arm], s));
            CK(hipStreamSynchronize(s));
            CK(hipMemcpy(arm == 0 ? y0.data() : y1.data(), dy[1], ny * 4, hipMemcpyDeviceToHost));
            if (arm > 0) for (size_t i = 0; i < ny; ++i) md[arm] = std::max(md[arm], (double)fabsf(y0[i] - y1[i]));
        }
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<float> us[NA];
        for (int r = -1; r < reps * 3; ++r)                  // round -1 is untimed: the first burst after the host-side setup runs at ramping clocks
            for (int arm = 0; arm < NA; ++arm) {
                CK(hipEventRecord(e0, s));
                for (int b = 0; b < burst; ++b) CK(hipGraphLaunch(ge[arm], s));
                CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
                float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) us[arm].push_back(ms * 200.f / burst);
            }
        printf("%-8s %3d->%3d %4dx%-4d p%d ", L.name, L.ci, L.co, L.h, L.w, pieces);
        for (int arm = 0; arm < NA; ++arm) {
            std::sort(us[arm].begin(), us[arm].end());
            printf(" %7.1f [%6.1f ..%6.1f]", us[arm][us[arm].size() / 2], us[arm].front(), us[arm].back());
        }
        printf("  max|sk-classic| %.1e %.1e %.1e\n", md[1], md[2], md[3]);
        fflush(stdout);
        for (auto &x : ge) CK(hipGraphExecDestroy(x));
        CK(hipFree(dx)); CK(hipFree(dw)); CK(hipFree(du)); CK(hipFree(db));
        for (auto &p : ws) CK(hipFree(p));
        for (auto &p : dy) CK(hipFree(p));
    }
    return 0;
}

// the arms of --loop / --abl: one knob value per arm, everything else the library's own pick
static int loop_arms(const std::vector<std::string> &want, bool abl) {
    hipStream_t s; CK(hipStreamCreate(&s));
    const int burst = getenv("CONV_MICRO_BURST") ? atoi(getenv("CONV_MICRO_BURST")) : 8;
    const int reps = getenv("CONV_MICRO_REPS") ? atoi(getenv("CONV_MICRO_REPS")) : 3;
    std::mt19937 g(1); std::uniform_real_distribution<float> u(-1.f, 1.f);
    constexpr int NA = 4;
    const char *key = abl ? "FRCNN_CONV_WINO_ABL" : "FRCNN_CONV_WINO_LOOP";
    const char *val[NA] = {abl ? "1" : "0", abl ? "2" : "1", abl ? "3" : "5", abl ? "0" : "7"};
    if (abl && frcnn_set_tuning("FRCNN_CONV_WINO_LOOP", "0") != 0) { printf("set_tuning failed\n"); return 1; }
    printf("# us per launch: median of %d batches (each the median of 3 interleaved bursts of %d x 5 launches) [min .. max of all bursts]\n", reps, burst);
    if (abl) printf("# %-8s %-22s %-24s %-24s %-24s %-24s\n", "layer", "shape", "MFMAs only", "+ reads, transform", "+ DMA issue", "+ wait, barrier (whole)");
    else printf("# %-8s %-22s %-24s %-24s %-24s %-24s %s\n", "layer", "shape", "loop 0 (first)", "loop 1 (item 2)", "loop 5 (+ item 4)", "loop 7 (+ item 3)", "bits vs loop 0");
    for (const Layer &L : kLayers) {
        if (!want.empty() && std::find(want.begin(), want.end(), std::string(L.name)) == want.end()) continue;
        const int OH = L.pool ? (L.h + 1) / 2 : L.h, OW = L.pool ? (L.w + 1) / 2 : L.w;
        const size_t nx = (size_t)L.ci * L.h * L.w, nw = (size_t)9 * L.co * L.ci, ny = (size_t)L.co * OH * OW;
        std::vector<float> hx(nx), hw(nw), hb(L.co);
        for (auto &e : hx) e = u(g);
        for (auto &e : hw) e = 0.05f * u(g);
        for (auto &e : hb) e = 0.1f * u(g);
        float *dx, *dw, *du, *db, *dy[3]; void *ws;
        CK(hipMalloc(&dx, nx * 4)); CK(hipMalloc(&dw, nw * 4)); CK(hipMalloc(&du, nw / 9 * 16 * 4)); CK(hipMalloc(&db, L.co * 4));
        for (auto &p : dy) CK(hipMalloc(&p, ny * 4));
        CK(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(db, hb.data(), L.co * 4, hipMemcpyHostToDevice));
        if (frcnn_wino_pack_w(dw, L.co, L.ci, 0, du, s) != 0) { printf("pack failed\n"); return 1; }
        const size_t wsb = frcnn_conv_wino_sk_workspace_bytes(L.ci, L.co, L.h, L.w);
        CK(hipMalloc(&ws, wsb));
        if (frcnn_conv_wino_sk_workspace_init(ws, wsb, s) != 0) { printf("workspace init failed\n"); return 1; }
        hipGraphExec_t ge[NA];
        std::vector<float> y0(ny), y1(ny);
        size_t differ[NA] = {0, 0, 0, 0};
        for (int arm = 0; arm < NA; ++arm) {
            if (frcnn_set_tuning(key, val[arm]) != 0) { printf("set_tuning failed\n"); return 1; }
            CK(hipStreamSynchronize(s));
            hipGraph_t gr;
            CK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
            bool ok = true;
            for (int i = 0; i < 5; ++i) ok = ok && frcnn_conv3x3_wino_sk_f32(dx, du, db, dy[i % 3], L.ci, L.co, L.h, L.w, L.pool ? 4 : 1, ws, wsb, s) == 0;
            CK(hipStreamEndCapture(s, &gr));
            frcnn_set_tuning(key, nullptr);
            if (!ok) { printf("%s: launch refused (arm %d: this build does not carry the form)\n", L.name, arm); return 1; }
            CK(hipGraphInstantiate(&ge[arm], gr, nullptr, nullptr, 0));
            CK(hipGraphDestroy(gr));
            for (int i = 0; i < 2; ++i) CK(hipGraphLaunch(ge[arm], s));
            CK(hipStreamSynchronize(s));
            CK(hipMemcpy(arm == 0 ? y0.data() : y1.data(), dy[1], ny * 4, hipMemcpyDeviceToHost));
            if (arm > 0) for (size_t i = 0; i < ny; ++i) differ[arm] += memcmp(&y0[i], &y1[i], 4) != 0;
        }
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<float> us[NA], med[NA];
        for (int r = -1; r < reps; ++r)                      // batch -1 is untimed: the first bursts after the host-side setup run at ramping clocks
            for (int k = 0; k < 3; ++k)
                for (int arm = 0; arm < NA; ++arm) {
                    CK(hipEventRecord(e0, s));
                    for (int b = 0; b < burst; ++b) CK(hipGraphLaunch(ge[arm], s));
                    CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
                    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
                    if (r >= 0) us[arm].push_back(ms * 200.f / burst);
                }
        printf("%-8s %3d->%3d %4dx%-4d ", L.name, L.ci, L.co, L.h, L.w);
        for (int arm = 0; arm < NA; ++arm) {
            for (int r = 0; r < reps; ++r) {                 // the median of each batch of three, then the median of the batches
                std::vector<float> b3(us[arm].begin() + 3 * r, us[arm].begin() + 3 * r + 3);
                std::sort(b3.begin(), b3.end());
                med[arm].push_back(b3[1]);
            }
            std::sort(med[arm].begin(), med[arm].end());
            std::sort(us[arm].begin(), us[arm].end());
            printf(" %7.1f [%6.1f ..%6.1f]", med[arm][med[arm].size() / 2], us[arm].front(), us[arm].back());
        }
        if (!abl) printf("  differing floats %zu %zu %zu of %zu", differ[1], differ[2], differ[3], ny);
        printf("\n");
        fflush(stdout);
        for (auto &x : ge) CK(hipGraphExecDestroy(x));
        CK(hipFree(dx)); CK(hipFree(dw)); CK(hipFree(du)); CK(hipFree(db)); CK(hipFree(ws));
        for (auto &p : dy) CK(hipFree(p));
    }
    return 0;
}

int main(int argc, char **argv) {
    std::vector<std::string> want;
    bool sk = false, loop = false, abl = false;
    for (int i = 1; i < argc; ++i) {
        if (std::string(argv[i]) == "--sk") sk = true;
        else if (std::string(argv[i]) == "--loop") loop = true;
        else if (std::string(argv[i]) == "--abl") abl = true;
        else want.push_back(argv[i]);
    }
    if (loop || abl) return loop_arms(want, abl);
    if (sk) return sk_gate(want);
#ifdef WINO_MICRO_LAB_ONLY                                   // linked against the research build of conv_wino.hip alone: no direct kernels to compare with
    printf("this build runs --loop, --abl and --sk only\n");
    return 1;
#else
    hipStream_t s; CK(hipStreamCreate(&s));
    const int burst = getenv("CONV_MICRO_BURST") ? atoi(getenv("CONV_MICRO_BURST")) : 8;
    const int reps = getenv("CONV_MICRO_REPS") ? atoi(getenv("CONV_MICRO_REPS")) : 3;
    std::mt19937 g(1); std::uniform_real_distribution<float> u(-1.f, 1.f);
    double tot[2] = {0, 0};
    for (const Layer &L : kLayers) {
        if (!want.empty() && std::find(want.begin(), want.end(), std::string(L.name)) == want.end()) continue;
        const int OH = L.pool ? (L.h + 1) / 2 : L.h, OW = L.pool ? (L.w + 1) / 2 : L.w;
        const size_t nx = (size_t)L.ci * L.h * L.w, nw = (size_t)9 * L.co * L.ci, ny = (size_t)L.co * OH * OW;
        std::vector<float> hx(nx), hw(nw), hb(L.co);
        for (auto &e : hx) e = u(g);
        for (auto &e : hw) e = 0.05f * u(g);
        for (auto &e : hb) e = 0.1f * u(g);
        float *dx, *dw, *dwp, *du, *db, *dy[2][3]; void *ws[2];
        CK(hipMalloc(&dx, nx * 4)); CK(hipMalloc(&dw, nw * 4)); CK(hipMalloc(&dwp, nw * 4)); CK(hipMalloc(&du, nw / 9 * 16 * 4)); CK(hipMalloc(&db, L.co * 4));
        for (auto &a : dy) for (auto &p : a) CK(hipMalloc(&p, ny * 4));
        const size_t wsb[2] = {frcnn_conv3x3_workspace_bytes(L.ci, L.co, L.h, L.w), frcnn_conv_wino_workspace_bytes(L.ci, L.co, L.h, L.w)};
        CK(hipMalloc(&ws[0], wsb[0])); CK(hipMalloc(&ws[1], wsb[1]));
        if (frcnn_conv3x3_workspace_init(ws[0], wsb[0], s) != 0) { printf("workspace init failed\n"); return 1; }
        CK(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(db, hb.data(), L.co * 4, hipMemcpyHostToDevice));
        if (frcnn_pack_conv3x3_w(dw, L.co, L.ci, dwp, s) != 0 || frcnn_wino_pack_w(dw, L.co, L.ci, 0, du, s) != 0) { printf("pack failed\n"); return 1; }
        const double gflop = 2.0 * L.h * L.w * L.co * L.ci * 9 / 1e9;
        hipGraphExec_t ge[2];
        for (int arm = 0; arm < 2; ++arm) {
            hipGraph_t gr;
            CK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
            bool ok = true;
            for (int i = 0; i < 5; ++i)
                ok = ok && (arm == 0 ? frcnn_conv_f32_ex(dx, dwp, db, nullptr, dy[0][i % 3], L.ci, L.co, L.h, L.w, 3, L.pool ? 4 : 1, ws[0], wsb[0], s)
                                     : frcnn_conv3x3_wino_f32(dx, du, db, dy[1][i % 3], L.ci, L.co, L.h, L.w, L.pool ? 4 : 1, ws[1], wsb[1], s)) == 0;
            CK(hipStreamEndCapture(s, &gr));
            if (!ok) { printf("%s: launch refused (arm %d)\n", L.name, arm); return 1; }
            CK(hipGraphInstantiate(&ge[arm], gr, nullptr, nullptr, 0));
            CK(hipGraphDestroy(gr));
            for (int i = 0; i < 2; ++i) CK(hipGraphLaunch(ge[arm], s));
        }
        CK(hipStreamSynchronize(s));
        // sanity: the two arms' outputs
        std::vector<float> y0(ny), y1(ny);
        CK(hipMemcpy(y0.data(), dy[0][1], ny * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(y1.data(), dy[1][1], ny * 4, hipMemcpyDeviceToHost));
        double md = 0, mx = 0;
        for (size_t i = 0; i < ny; ++i) { md = std::max(md, (double)fabsf(y0[i] - y1[i])); mx = std::max(mx, (double)fabsf(y0[i])); }
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<float> us[2];
        for (int r = 0; r < reps * 3; ++r)
            for (int arm = 0; arm < 2; ++arm) {
                CK(hipEventRecord(e0, s));
                for (int b = 0; b < burst; ++b) CK(hipGraphLaunch(ge[arm], s));
                CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
                float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1)); us[arm].push_back(ms * 200.f / burst);
            }
        double med[2];
        for (int arm = 0; arm < 2; ++arm) { std::sort(us[arm].begin(), us[arm].end()); med[arm] = us[arm][us[arm].size() / 2]; tot[arm] += med[arm] * L.times; }
        printf("%-8s %3d->%3d %4dx%-4d %s direct %7.1f us  wino %7.1f us  (x%.2f; direct %6.1f TFLOP/s)  max|wino-direct|/max|direct| %.2e\n", L.name, L.ci, L.co,
               L.h, L.w, L.pool ? "relu+pool" : "relu     ", med[0], med[1], med[0] / med[1], gflop / med[0] * 1e3, md / (mx > 0 ? mx : 1));
        fflush(stdout);
        for (auto &x : ge) CK(hipGraphExecDestroy(x));
        CK(hipFree(dx)); CK(hipFree(dw)); CK(hipFree(dwp)); CK(hipFree(du)); CK(hipFree(db)); CK(hipFree(ws[0])); CK(hipFree(ws[1]));
        for (auto &a : dy) for (auto &p : a) CK(hipFree(p));
    }
    printf("chain (conv5_1 x 4; conv1_1 not included): direct %.1f us, wino %.1f us\n", tot[0], tot[1]);
    return 0;
#endif
}
