// A plain C-ABI client of xrfthip_exec_ex (include/xrft_hip.h, "a kept pass 1"): no Python, no torch.
// Two 512 x 256 float32 fields, batch 3, Hann windows, linear detrend.  A CROSS plan writes both fields' pass-1 blocks (PRODUCE) into memory of the client's;
// a POWER plan per field then reads its block (CONSUME) and must give, bit for bit, what it gives with everything private (xrfthip_exec) -- and so must the
// CROSS plan itself.  The argument checks of xrfthip_exec_ex are driven on the way.
// Builds against the real library (hipcc --offload-arch=gfx950 pass1_example.cpp -I../../include -L../../xrft_amd -lxrft_hip) and, with -DXRFT_EMULATE
// -I../emu, against the emulated one together with the library's sources -- the form tests/test_column_reuse_emulated.py runs under AddressSanitizer and UBSan.
#ifdef XRFT_EMULATE
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xrft_hip.h"

#define CK(x) do { int rc_ = (x); if (rc_) { std::fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, xrfthip_strerror(rc_)); return 1; } } while (0)
#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s -> hipError_t %d\n", #x, (int)e_); return 1; } } while (0)
#define WANT(x, rc) do { int rc_ = (x); if (rc_ != (rc)) { std::fprintf(stderr, "%s -> %d, expected %d\n", #x, rc_, (int)(rc)); return 1; } } while (0)

static int make_plan(xrfthip_plan** plan, int out_mode, int64_t nb, int64_t ny, int64_t nx) {
    xrfthip_desc d = {};
    d.struct_size = sizeof d; d.ndim = 2; d.batch = nb; d.ny = ny; d.nx = nx;
    d.dtype = XRFTHIP_F32; d.out_mode = out_mode; d.detrend = XRFTHIP_DETREND_LINEAR; d.flags = XRFTHIP_SHIFT_Y | XRFTHIP_SHIFT_X; d.scale = 1.0;
    int rc = xrfthip_plan_create(plan, &d);
    const double pi = 3.14159265358979323846;
    std::vector<double> wy((size_t)ny), wx((size_t)nx);
    for (int64_t i = 0; i < ny; ++i) wy[(size_t)i] = 0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)ny);
    for (int64_t i = 0; i < nx; ++i) wx[(size_t)i] = 0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)nx);
    if (!rc) rc = xrfthip_plan_set_window(*plan, 0, wy.data(), ny);
    if (!rc) rc = xrfthip_plan_set_window(*plan, 1, wx.data(), nx);
    return rc;
}

int main() {
    const int64_t nb = 3, ny = 512, nx = 256;
    const size_t n = (size_t)nb * ny * nx;
    std::vector<float> h0(n), h1(n);
    unsigned s = 2463534242u;
    for (size_t e = 0; e < n; ++e) {
        s = s * 1664525u + 1013904223u;
        const float u = (float)((s >> 8) & 0xffff) / 65536.0f - 0.5f;
        s = s * 1664525u + 1013904223u;
        const float v = (float)((s >> 8) & 0xffff) / 65536.0f - 0.5f;
        const size_t i = (e / (size_t)nx) % (size_t)ny, j = e % (size_t)nx;
        h0[e] = u + 0.01f * (float)i - 0.02f * (float)j + 3.0f;
        h1[e] = 0.5f * h0[e] + v;
    }
    xrfthip_plan *cross = nullptr, *pow0 = nullptr;
    CK(make_plan(&cross, XRFTHIP_OUT_CROSS, nb, ny, nx));
    CK(make_plan(&pow0, XRFTHIP_OUT_POWER, nb, ny, nx));
    const size_t pb = xrfthip_plan_pass1_bytes(cross);
    if (!pb || pb % 256 || xrfthip_plan_pass1_bytes(pow0) != pb) { std::fprintf(stderr, "pass1_bytes: %zu / %zu\n", pb, xrfthip_plan_pass1_bytes(pow0)); return 1; }
    uint64_t sc0 = 0, sc1 = 0, sp = 0;
    CK(xrfthip_plan_pass1_signature(cross, 0, &sc0));
    CK(xrfthip_plan_pass1_signature(cross, 1, &sc1));
    CK(xrfthip_plan_pass1_signature(pow0, 0, &sp));
    WANT(xrfthip_plan_pass1_signature(pow0, 1, &sp), XRFTHIP_BAD_ARG);
    if (sc0 != sp || sc1 != sp) { std::fprintf(stderr, "signatures differ\n"); return 1; }

    const size_t ws_c = xrfthip_workspace_bytes(cross), ws_p = xrfthip_workspace_bytes(pow0);
    const size_t ws_c_small = ws_c - 2 * pb, ws_p_small = ws_p - pb, ws_max = ws_c > ws_p ? ws_c : ws_p;
    float *d_in0 = nullptr, *d_in1 = nullptr;
    void *d_cs = nullptr, *d_cs2 = nullptr, *d_ps = nullptr, *d_ps2 = nullptr, *d_ws = nullptr, *d_blocks = nullptr;
    HK(hipMalloc((void**)&d_in0, n * sizeof(float)));
    HK(hipMalloc((void**)&d_in1, n * sizeof(float)));
    HK(hipMalloc(&d_cs, n * 8)); HK(hipMalloc(&d_cs2, n * 8));
    HK(hipMalloc(&d_ps, n * 4)); HK(hipMalloc(&d_ps2, n * 4));
    HK(hipMalloc(&d_ws, ws_max));
    HK(hipMalloc(&d_blocks, 2 * pb));
    HK(hipMemcpy(d_in0, h0.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HK(hipMemcpy(d_in1, h1.data(), n * sizeof(float), hipMemcpyHostToDevice));
    char* blk = (char*)d_blocks;

    // everything private: the results to meet
    CK(xrfthip_exec(cross, d_in0, d_in1, d_cs, nullptr, d_ws, ws_c, nullptr));
    HK(hipDeviceSynchronize());
    std::vector<char> ref_cs(n * 8), ref_ps0(n * 4), ref_ps1(n * 4), got(n * 8);
    HK(hipMemcpy(ref_cs.data(), d_cs, n * 8, hipMemcpyDeviceToHost));
    CK(xrfthip_exec(pow0, d_in0, nullptr, d_ps, nullptr, d_ws, ws_p, nullptr));
    HK(hipDeviceSynchronize());
    HK(hipMemcpy(ref_ps0.data(), d_ps, n * 4, hipMemcpyDeviceToHost));
    CK(xrfthip_exec(pow0, d_in1, nullptr, d_ps, nullptr, d_ws, ws_p, nullptr));
    HK(hipDeviceSynchronize());
    HK(hipMemcpy(ref_ps1.data(), d_ps, n * 4, hipMemcpyDeviceToHost));

    // the argument checks
    xrfthip_exec_args a = {};
    a.struct_size = sizeof a;
    a.d_in0 = d_in0; a.d_in1 = d_in1; a.d_out = d_cs2; a.d_workspace = d_ws; a.ws_bytes = ws_c; a.stream = nullptr;
    xrfthip_exec_args bad = a;
    bad.field[0].pass1_mode = 3; bad.field[0].pass1_block = blk;
    WANT(xrfthip_exec_ex(cross, &bad), XRFTHIP_BAD_ARG);  // no such mode
    bad = a; bad.field[0].pass1_mode = XRFTHIP_PASS1_PRODUCE;
    WANT(xrfthip_exec_ex(cross, &bad), XRFTHIP_BAD_ARG);  // no block
    bad.field[0].pass1_block = blk + 64;
    WANT(xrfthip_exec_ex(cross, &bad), XRFTHIP_BAD_ARG);  // not aligned
    bad.field[0].pass1_block = (char*)d_ws + 256;
    WANT(xrfthip_exec_ex(cross, &bad), XRFTHIP_BAD_ARG);  // inside the workspace
    bad = a; bad.field[0].pass1_mode = bad.field[1].pass1_mode = XRFTHIP_PASS1_PRODUCE; bad.field[0].pass1_block = blk; bad.field[1].pass1_block = blk + 256;
    WANT(xrfthip_exec_ex(cross, &bad), XRFTHIP_BAD_ARG);  // the two blocks overlap
    bad.field[1].pass1_block = blk + pb; bad.ws_bytes = ws_c_small - 256;
    WANT(xrfthip_exec_ex(cross, &bad), XRFTHIP_WORKSPACE_TOO_SMALL);
    bad = a; bad.struct_size = 8;
    WANT(xrfthip_exec_ex(cross, &bad), XRFTHIP_BAD_ARG);

    // produce: the CROSS plan writes both blocks, with the small workspace
    a.field[0].pass1_mode = a.field[1].pass1_mode = XRFTHIP_PASS1_PRODUCE;
    a.field[0].pass1_block = blk; a.field[1].pass1_block = blk + pb; a.ws_bytes = ws_c_small;
    CK(xrfthip_exec_ex(cross, &a));
    HK(hipDeviceSynchronize());
    HK(hipMemcpy(got.data(), d_cs2, n * 8, hipMemcpyDeviceToHost));
    int bad_bits = std::memcmp(got.data(), ref_cs.data(), n * 8) != 0;
    std::printf("cross, blocks produced: %s\n", bad_bits ? "DIFFERS" : "identical");
    // consume: a POWER plan per field reads its block -- the input pointers are passed but pass 1 does not run
    for (int f = 0; f < 2; ++f) {
        xrfthip_exec_args c = {};
        c.struct_size = sizeof c;
        c.d_in0 = f ? d_in1 : d_in0; c.d_out = d_ps2; c.d_workspace = d_ws; c.ws_bytes = ws_p_small;
        c.field[0].pass1_mode = XRFTHIP_PASS1_CONSUME; c.field[0].pass1_block = blk + (size_t)f * pb;
        CK(xrfthip_exec_ex(pow0, &c));
        HK(hipDeviceSynchronize());
        HK(hipMemcpy(got.data(), d_ps2, n * 4, hipMemcpyDeviceToHost));
        const int diff = std::memcmp(got.data(), (f ? ref_ps1 : ref_ps0).data(), n * 4) != 0;
        std::printf("power of field %d, block consumed: %s\n", f, diff ? "DIFFERS" : "identical");
        bad_bits |= diff;
    }
    // ... and the CROSS plan reading field 0's block while it computes field 1 inside its (full) workspace
    a.field[0].pass1_mode = XRFTHIP_PASS1_CONSUME; a.field[1].pass1_mode = XRFTHIP_PASS1_PRIVATE; a.field[1].pass1_block = nullptr; a.ws_bytes = ws_c;
    CK(xrfthip_exec_ex(cross, &a));
    HK(hipDeviceSynchronize());
    HK(hipMemcpy(got.data(), d_cs2, n * 8, hipMemcpyDeviceToHost));
    const int diff = std::memcmp(got.data(), ref_cs.data(), n * 8) != 0;
    std::printf("cross, field 0 consumed, field 1 private: %s\n", diff ? "DIFFERS" : "identical");
    bad_bits |= diff;

    CK(xrfthip_plan_destroy(cross));
    CK(xrfthip_plan_destroy(pow0));
    hipFree(d_in0); hipFree(d_in1); hipFree(d_cs); hipFree(d_cs2); hipFree(d_ps); hipFree(d_ps2); hipFree(d_ws); hipFree(d_blocks);
    std::puts(bad_bits ? "FAIL" : "OK");
    return bad_bits;
}
