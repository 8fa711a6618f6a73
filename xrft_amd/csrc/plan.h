#pragma once
// plan.h -- what the host side of libxrft_hip.so shares between its translation units (not part of the C ABI: include/xrft_hip.h is):
// the plan (struct xrfthip_plan), device tables, the small host helpers, the table of per-family host operations (struct FamilyOps: one row
// per Family, defined in the unit that owns the family) and the few host functions more than one unit calls.
//
//   xrft_hip.cpp     the plan builder (xrfthip_plan_create: descriptor checks, then the families' try_* in order of precedence), the generic
//                    tile passes (tile_fft.h) and their workspace layout, the table of rows (family_ops), profiling, the C ABI of the plan:
//                    finalize / set_binmap / kernel_info / describe / exec go through the plan's row
//                    (Generic)
//   host_fasty.cpp   the y-first float32 two-pass pipeline (fasty.h, fasty_mean.h) and its complex form (fasty_c2c.h): try_*, tables, launchers
//                    (FastY, FastY1D, FastYC, FastYCFourStep)
//   host_fastm.cpp   the mixed-radix pipeline on the lat/lon lengths (fastm.h), its run-time-radix form (fastn.h), the one-axis table kernels
//                    (FastM, FastN, FastMY, FastMX)
//   host_fastg.cpp   the one-pass lengths-as-data kernels (fastg.h): small slabs, one axis of any smooth length, Rader / Bluestein tables;
//                    the last pass of a three-axis spectrum (fasth.h)
//                    (FastG, FastGY, FastH)
//   host_rows.cpp    the register-resident one-pass kernels: small float32 slabs (fasts.h), long rows and complex rows (fastr.h)
//                    (FastS, FastR, FastRComplex, FastRRows)
//   host_welch.inc   ... and, included at its end (one translation unit), the segments of a series in an LDS tile: Welch spectra, averaged in one pass
//                    (fastw.h), or every segment's spectrum kept (fastk.h); the descriptor checks of xrfthip_desc.seg_*
//                    (FastW, FastK)
//   host_inner.cpp   two transform axes that are not the trailing pair (xrfthip_desc.inner / .mid): the fused passes and the composite plan
//                    (FusedInner, Composite)
//   ops.cpp          the stand-alone operations of the ABI (detrend, spectrum tail, gather, convert, reduce, isotropize, ...)
//   inst_g1..7.cpp   the explicit instantiations of the fasty / fastm / fastn kernel templates (instances.h)
//
// A plan is a short list of kernel launches per group of slabs, chosen when the plan is created (xrfthip_plan_describe says which):
//   * generic passes (tile_fft.h), any shape:   [slab_moments -> finalize_coef]  ->  x pass(es)  ->  y pass(es)  [-> radial sums]
//     The x pass reads the user's array (detrend / window / flip / ifftshift fused into its loads) and the last pass writes the
//     user's output (fftshift / phase / scaling / |F|^2 / cross / mirror fused into its stores); the only intermediate is the
//     half spectrum of ONE group of slabs, re-used for every group.
//   * the specialised families above: enum class Family, one value per plan; each family's launcher, describe text, workspace layout and
//     reactions to the plan's tables are its row of FamilyOps.
// Nothing allocates or synchronises in exec.
#include <algorithm>
#include <functional>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/xrft_hip.h"
#ifndef XRFT_EMULATE
#include <hip/hip_ext.h>
#endif
#include "aux_kernels.h"
#include "fastp2.h"
#include "fasty.h"
#include "fasty_c2c.h"
#include "selftest.h"
#include "fastm.h"
#include "fastn.h"
#include "fastr.h"
#include "fasts.h"
#include "fasty_mean.h"
#include "tile_fft.h"
#include "fastg.h"
#include "fasth.h"
#include "fastw.h"
#include "fastk.h"
#include "fasto.h"
#include "fastf.h"
#include "fastt.h"
#ifdef XRFT_SPLIT_TUS  /* the library built from several translation units: the fasty / fastm kernels are instantiated in inst_g*.cpp */
namespace xrft {
#define XRFT_KW extern template __global__
#include "instances.h"
#undef XRFT_KW
}
#endif

using namespace xrft;

namespace xrfth {

extern thread_local int g_last_hip_error;

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) {                         \
            g_last_hip_error = (int)e_;                 \
            return XRFTHIP_HIP_ERROR;                   \
        }                                               \
    } while (0)

constexpr size_t kLdsMax = 160 * 1024;  // gfx950: 160 KiB per CU, one workgroup may use all of it
constexpr int kCUs = 256;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int upload(const void* host, size_t n) {
        if (p) { (void)hipFree(p); p = nullptr; }
        bytes = n;
        if (hipMalloc(&p, n ? n : 16) != hipSuccess) { p = nullptr; return XRFTHIP_ALLOC_FAILED; }
        HIP_TRY(hipMemcpy(p, host, n, hipMemcpyHostToDevice));
        return XRFTHIP_OK;
    }
    void clear() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
};

struct FftTables {  // per FFT length, in the plan's precision
    int n = 0;
    std::vector<int> radix;
    bool generic = false;
    DevBuf tw, rev;
    // Bluestein (a prime factor above XRFTHIP_MAX_RADIX): the LDS transform has blue_m = 2^a 3^b 5^c >= 2n-1 points;
    // blue_c[k] = exp(+i pi k^2 / n), blue_b = FFT_m(chirp kernel) / m in the order the DIF passes leave it
    int blue_m = 0;
    DevBuf blue_c, blue_b;
};

enum BufKind { B_NONE = 0, B_IN, B_W, B_W2, B_F0, B_OUT };

struct Pass {
    TileGeom g{};
    Prologue pr{};
    Epilogue ep{};
    bool first = false, final_ = false, generic = false;
    int path = 0;  // tile_fft_kernel PATH: 0 = general instantiation, 1..4 = lean single-purpose ones
    int threads = 256;
    size_t lds = 0;
    int in_kind = B_NONE, out_kind = B_NONE;
    long long outer_per_slab = 1;  // n_outer = outer_per_slab * slabs in the group
    std::string label;
};

inline long long env_ll(const char* name, long long dflt) {
    const char* e = getenv(name);
    return e && *e ? atoll(e) : dflt;
}

inline int factorize(long long n, std::vector<int>& out, bool& generic) {
    // prime factors first: anything above XRFTHIP_MAX_RADIX is refused here (Bluestein takes over, see lds_fft_len)
    std::vector<int> big;  // primes other than 2, 3, 5: O(r^2) butterflies of their own
    long long m = n;
    int c2 = 0, c3 = 0, c5 = 0;
    while (m % 2 == 0) { ++c2; m /= 2; }
    while (m % 3 == 0) { ++c3; m /= 3; }
    while (m % 5 == 0) { ++c5; m /= 5; }
    for (long long p = 7; m > 1; p += 2) {
        if (p * p > m) p = m;
        while (m % p == 0) {
            if (p > XRFTHIP_MAX_RADIX) return XRFTHIP_UNSUPPORTED_LENGTH;
            big.push_back((int)p);
            m /= p;
        }
    }
    generic = !big.empty();
    std::sort(big.begin(), big.end(), [](int a, int b) { return a > b; });
    // 2^a 3^b 5^c into as few passes as possible with the in-register butterflies 16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2
    // (every pass is one trip of every point through LDS): exhaustive search, the exponents are small
    static const int R[] = {16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2};
    static const int E2[] = {4, 0, 2, 1, 0, 3, 1, 0, 2, 0, 1}, E3[] = {0, 1, 1, 0, 2, 0, 1, 0, 0, 1, 0}, E5[] = {0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const bool comp = env_ll("XRFTHIP_COMPOSITE", 1) != 0, r16 = env_ll("XRFTHIP_RADIX16", 1) != 0;
    std::vector<int> best, cur;
    std::function<void(int, int, int, int)> dfs = [&](int a2, int a3, int a5, int from) {
        if (a2 == 0 && a3 == 0 && a5 == 0) {
            if (best.empty() || cur.size() < best.size()) best = cur;
            return;
        }
        if (!best.empty() && cur.size() + 1 >= best.size()) return;
        for (int i = from; i < 11; ++i) {  // non-increasing radices: each multiset once, big radices tried first
            if (E2[i] > a2 || E3[i] > a3 || E5[i] > a5) continue;
            if (!comp && (R[i] == 15 || R[i] == 12 || R[i] == 10 || R[i] == 9 || R[i] == 6)) continue;
            if (!r16 && R[i] == 16) continue;
            cur.push_back(R[i]);
            dfs(a2 - E2[i], a3 - E3[i], a5 - E5[i], i);
            cur.pop_back();
        }
    };
    if (c2 || c3 || c5) dfs(c2, c3, c5, 0);
    // DIF order: odd and composite radices first (their passes then run on lane-contiguous LDS), powers of two last
    std::vector<int> odd, two;
    for (int r : best) ((r & (r - 1)) == 0 ? two : odd).push_back(r);
    out = big;
    out.insert(out.end(), odd.begin(), odd.end());
    out.insert(out.end(), two.begin(), two.end());
    if ((int)out.size() > XRFT_MAX_PASSES) return XRFTHIP_UNSUPPORTED_LENGTH;
    return XRFTHIP_OK;
}

// host-side forward FFT (float64) of any length whose prime factors are small: recursive decimation in time over the
// smallest factor (used once per plan for the Bluestein kernel's spectrum)
inline void host_fft_rec(const double* xr, const double* xi, size_t n, size_t stride, double* yr, double* yi) {
    if (n == 1) { yr[0] = xr[0]; yi[0] = xi[0]; return; }
    size_t p = 2;
    while (n % p) ++p;
    const size_t m = n / p;
    std::vector<double> tr(n), ti(n);
    for (size_t r = 0; r < p; ++r) host_fft_rec(xr + r * stride, xi + r * stride, m, stride * p, tr.data() + r * m, ti.data() + r * m);
    const long double w0 = -2.0L * 3.14159265358979323846264338327950288L / (long double)n;
    for (size_t k = 0; k < n; ++k) {
        long double ar = 0.0L, ai = 0.0L;
        const size_t km = k % m;
        for (size_t r = 0; r < p; ++r) {
            const long double a = w0 * (long double)((r * k) % n);
            const long double c = cosl(a), s = sinl(a);
            ar += c * tr[r * m + km] - s * ti[r * m + km];
            ai += c * ti[r * m + km] + s * tr[r * m + km];
        }
        yr[k] = (double)ar; yi[k] = (double)ai;
    }
}
inline void host_fft_smooth(std::vector<double>& re, std::vector<double>& im) {
    std::vector<double> yr(re.size()), yi(re.size());
    host_fft_rec(re.data(), im.data(), re.size(), 1, yr.data(), yi.data());
    re.swap(yr); im.swap(yi);
}

// length of the transform actually run in LDS for an n-point sequence: n, or the Bluestein length m = 2^a 3^b 5^c >= 2n - 1 (a
// power of two can be almost twice as long and then misses the LDS) when n has a prime factor the radix passes do not take
// -- or take badly: a prime above kGenericMax = 6 runs through the O(r^2) butterfly with its operands in scratch memory
// ((64, 721, 1440) float32, 721 = 7 x 103: 22.3 ms in the column pass, 2.9 GFFT/s -> 54.7 through Bluestein; 1001 = 7 x 11 x 13: 13 ->
// 26; a lone factor 7 breaks even), so it goes to Bluestein as long as four sequences of m points fit the LDS
// (scripts/prof_primes.py, prof_primes2.py).
inline long long lds_fft_len(long long n, size_t csize) {
    std::vector<int> r;
    bool g;
    if (n < 2) return n;
    const bool ok = factorize(n, r, g) == XRFTHIP_OK;
    static const long long kGenericMax = env_ll("XRFTHIP_GENERIC_MAX", 6);
    if (ok && (!g || r[0] <= kGenericMax)) return n;  // (g: a prime factor other than 2, 3, 5; those come first in r, largest first)
    long long m = 2 * n - 1;
    for (;; ++m) {
        long long q = m;
        while (q % 2 == 0) q /= 2;
        while (q % 3 == 0) q /= 3;
        while (q % 5 == 0) q /= 5;
        if (q == 1) break;
    }
    if (!ok) return m;
    const size_t per = (size_t)(m + m / 16 + 2) * csize;
    // (a factor above 13 through the O(r^2) butterfly is hopeless -- 1460 = 2 x 2 x 5 x 73 daily samples of four years, float64: 1.0 GFFT/s along the time axis --:
    // Bluestein even when only one or two sequences of m points fit the tile)
    const size_t seqs = r[0] > 13 ? 1 : 4;
    return seqs * per + 4096 <= kLdsMax ? m : n;
}

// host-side radix-2 FFT (float64) for the two 4096-point window spectra the fused detrend needs
inline void host_fft_pow2(std::vector<double>& re, std::vector<double>& im) {
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * 3.14159265358979323846264338327950288 / (double)len;
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const double wr = cos(ang * (double)k), wi = sin(ang * (double)k);
                const size_t a = i + k, b = i + k + len / 2;
                const double xr = re[b] * wr - im[b] * wi, xi = re[b] * wi + im[b] * wr;
                re[b] = re[a] - xr; im[b] = im[a] - xi;
                re[a] += xr; im[a] += xi;
            }
    }
}

template <typename T>
int build_tables(FftTables& t, int n_logical) {
    t.n = n_logical;
    const int n = (int)lds_fft_len(n_logical, 2 * sizeof(T));
    t.blue_m = n != n_logical ? n : 0;
    int rc = factorize(n, t.radix, t.generic);
    if (rc) return rc;
    std::vector<C2<T>> tw((size_t)std::max(n, 1));
    for (int k = 0; k < n; ++k) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
        tw[k].re = (T)cosl(a);
        tw[k].im = (T)sinl(a);
    }
    std::vector<unsigned> rev((size_t)std::max(n, 1));
    for (int pos = 0; pos < n; ++pos) {  // frequency held at LDS position `pos` after the DIF passes
        long long L = n, rem = pos, k = 0, mult = 1;
        for (int r : t.radix) {
            const long long m = L / r;
            k += (rem / m) * mult;
            rem %= m;
            mult *= r;
            L = m;
        }
        rev[(size_t)k] = (unsigned)pos;
    }
    rc = t.tw.upload(tw.data(), tw.size() * sizeof(C2<T>));
    if (rc) return rc;
    if (t.blue_m) {
        const long long N = n_logical;
        const long double pi = 3.14159265358979323846264338327950288L;
        std::vector<C2<T>> c((size_t)N);
        std::vector<double> br((size_t)n, 0.0), bi((size_t)n, 0.0);
        for (long long k = 0; k < N; ++k) {
            const long double a = pi * (long double)((k * k) % (2 * N)) / (long double)N;  // k^2 mod 2N keeps the angle small
            const long double cr = cosl(a), ci = sinl(a);
            c[(size_t)k].re = (T)cr; c[(size_t)k].im = (T)ci;
            br[(size_t)k] = (double)cr; bi[(size_t)k] = (double)ci;
            if (k) { br[(size_t)(n - k)] = (double)cr; bi[(size_t)(n - k)] = (double)ci; }
        }
        host_fft_smooth(br, bi);
        std::vector<C2<T>> bh((size_t)n);
        for (int k = 0; k < n; ++k) {
            bh[(size_t)rev[(size_t)k]].re = (T)(br[(size_t)k] / n);
            bh[(size_t)rev[(size_t)k]].im = (T)(bi[(size_t)k] / n);
        }
        rc = t.blue_c.upload(c.data(), c.size() * sizeof(C2<T>));
        if (!rc) rc = t.blue_b.upload(bh.data(), bh.size() * sizeof(C2<T>));
        if (rc) return rc;
    }
    return t.rev.upload(rev.data(), rev.size() * sizeof(unsigned));
}

template <typename T>
int build_twiddle(DevBuf& buf, long long N, long long count) {  // W_N^k, k < count
    std::vector<C2<T>> tw((size_t)count);
    for (long long k = 0; k < count; ++k) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)N;
        tw[(size_t)k].re = (T)cosl(a);
        tw[(size_t)k].im = (T)sinl(a);
    }
    return buf.upload(tw.data(), tw.size() * sizeof(C2<T>));
}

// The kernel family that serves a plan: one launcher (and one describe form) each.  xrfthip_plan_create picks it, the first of the
// families' try_* (in order of precedence) that takes the descriptor; settle_family can hand it on once the plan's tables arrive.
enum class Family {
    Generic,         // the tile passes (tile_fft.h)
    Composite,       // xrfthip_desc.inner / .mid: two one-axis plans (sub_x, sub_y)
    FusedInner,      // ... or the two fused passes where the axes lie (fastn.h)
    FastS,           // one pass over a small float32 slab in registers (fasts.h)
    FastG,           // one pass over a small slab, or groups of rows (g_one_d), lengths as data (fastg.h)
    FastGY,          // one pass along one axis that is not the contiguous one, or along rows with one Rader prime (gy_rows) (fastg.h)
    FastMX,          // short rows, table lengths (fastm.h, fastm_xonly_kernel)
    FastMY,          // one axis that is not the contiguous one, table lengths (fastm.h, fastm_yonly_kernel)
    FastR,           // one pass over a long real float32 row in registers (fastr.h)
    FastRComplex,    // ... complex rows of 2048 .. 16384 points (fastc_kernel)
    FastRRows,       // complex rows of 256 .. 4096 points: the row pass of fasty_c2c.h on the input's own rows
    FastW,           // xrfthip_desc.seg_hop, Welch spectra: the mean spectrum of the overlapping segments of a series, rows or column layout (fastw.h); with xrfthip_desc.seg_tapers the multitaper form, the sum over K tapers of ONE series' spectra (fastt.h)
    FastK,           // ... with xrfthip_desc.seg_keep, spectrograms: every segment's spectrum kept (fastk.h); with seg_synth the way back, the series rebuilt from them (fasto.h); with seg_filter both in one tile, a series filtered by overlap-save (fastf.h)
    FastYC,          // the two passes of fasty_c2c.h over complex float32 slabs
    FastYCFourStep,  // ... over ONE long complex sequence per batch entry, the four-step form of pass 2
    FastY,           // the two y-first passes over real float32 slabs of powers of two (fasty.h)
    FastY1D,         // ... as the two steps of a four-step transform of one long real sequence
    FastM,           // the two y-first passes, table lengths (fastm.h)
    FastN,           // ... with the lengths as data (fastn.h; either pass may still be a table kernel)
    FastH,           // xrfthip_desc.herm_ny / herm_nx, the last pass of a three-axis spectrum / transform: half spectrum in, full power / cross / field result out (fasth.h)
};
constexpr int kFamilyCount = (int)Family::FastH + 1;  // (FastH is the last value: a value added behind it moves this line, and the table of rows with it)
constexpr int kDeclined = 1;  // a try_* that does not take the descriptor (XRFTHIP_OK: taken, its tables built; < 0: an error)

}  // namespace xrfth
using namespace xrfth;

// FastW / FastK: the LDS tile of a workgroup (host_welch.inc).  Sequence t of the tile is (column t % C, pair of segments | segment t / C)
struct SegGeom {
    int C = 1, lgC = 0;      // the column layout (xrfthip_desc.seg_stride): adjacent columns per workgroup and their log2; 1: the rows layout
    long long ngroups = 1;   // ... groups of C columns per block
    int seqs = 1;            // sequences of the tile: FastW pairs of segments (of L points), FastK segments (of L / 2 points)
    int stride = 0;          // points between sequences: padded, odd
    size_t lds = 0;          // dynamic LDS of the launch
    long long rounds = 1;    // FastK only: rounds per series (group of columns), one workgroup each (FastW walks its runs inside the workgroup: 1)
};

struct xrfthip_plan {
    xrfthip_desc d{};
    bool dbl = false, cplx_in = false;
    int in16 = 0;  // the input holds 2-byte real samples: 1 float16 (XRFTHIP_F16), 2 bfloat16 (XRFTHIP_BF16).  The plan is the float32 plan (d.dtype = XRFTHIP_F32) in everything but
                   // the loads of the kernel that reads the caller's input (half_in.h); only the families half_family() names take it
    size_t rsize = 4, csize = 8;
    long long nxh = 0, width = 0, nx_out = 0, w_cols = 0;  // w_cols: columns of the row->column intermediate incl. tile padding
    bool mirror = false;
    int G = 1;
    int mom_chunks = 1;  // blocks per slab of the moments pass (partial sums added in order: deterministic)
    std::map<int, FftTables> tables;
    std::vector<DevBuf*> extra;  // r2c / four-step twiddles
    DevBuf win[2], phase[2], binmap;
    int nbins = 0;
    std::vector<Pass> passes;     // main pipeline (field 1 for CROSS)
    std::vector<Pass> passes_f0;  // CROSS: field 0 -> raw F0 buffer
    // workspace layout (byte offsets)
    size_t off_acc = 0, off_coef = 0, off_w = 0, off_w2 = 0, off_f0 = 0, off_pt = 0, off_rowfit = 0, off_corr = 0, off_isopart = 0, off_isotmp = 0, ws_bytes = 0;
    // the two y-first passes: what pass 1 leaves for ONE field inside the workspace -- its share of the intermediate (off_w), of the per-column sums and lines (off_rowfit) and
    // of the corrections (off_corr).  A pass-1 block handed in from outside (xrfthip_exec_ex) holds the three, in this order (layout_passes; fasty_pass1_bytes)
    size_t p1_w = 0, p1_fit = 0, p1_corr = 0;
    int iso_chunks = 1;  // workgroups per slab of the generic radial-sum pass (partial sums added in order)
    std::string desc_text;
    Family family = Family::Generic;  // what xrfthip_exec runs
    Family chosen = Family::Generic;  // what the plan's tables serve: `family`, unless settle_family parks a FastY plan on the generic passes
    // FastY: real float32 slabs whose two lengths are 256 .. 4096 powers of two (fasty.h), columns -> [fit] -> rows, no untile pass
    DevBuf tw_fx, tw_fy, ones4096, fph[2];
    std::vector<double> host_phase[2];  // complex, as handed to xrfthip_plan_set_phase (empty = none)
    // FastY1D: as the two steps of a four-step transform, one long real sequence per slab: N = yny * ynx samples viewed as
    // a [yny][ynx] slab (fasty.h, FS).  yny / ynx are d.ny / d.nx for the 2-D plans.
    // FastYC: the same two passes for COMPLEX float32 slabs (fasty_c2c.h): xrft.ifft over two axes, xrft.fft of complex data
    // FastM: the mixed-radix form (fastm.h): the lat/lon lengths
    // FastN: the same pipeline with the LENGTHS AS DATA (fastn.h): either pass (or both) may be the run-time-radix kernel -- every
    // length that is a product of the butterflies 2 ... 20 (7, 11, 13 included), and for the columns any other length through a chirp convolution
    struct NSide { bool rt = false; NGeo geo{}; size_t lds = 0; DevBuf twm, geo_dev; };
    NSide n_c, n_r;                 // pass 1 (columns, length ny) and pass 2 (rows, length nx)
    int n_cw = 0, n_rk = 1, n_rpu = 0, n_nxb = 0;  // the intermediate's layout: columns per block, rows per line; rows per pass-2 workgroup; column blocks per row
    long long y_pitch = 0;          // complex elements per row of the intermediate (ynx, or n_nxb * n_cw when the last column block is ragged)
    int n_blue_m = 0;               // pass 1 through a chirp convolution of this length
    DevBuf n_bluec, n_blueb;
    int n_rad_p = 0;                // ... or, ny = q p with ONE prime 17 ... 127 whose p - 1 the butterflies factor: the prime-factor form with Rader's algorithm along p
    std::vector<int> n_rq, n_rp;    // the radices of q and of p - 1
    DevBuf n_rgeo, n_radpin, n_radpout, n_radb;
    // FusedInner: xrfthip_desc.inner > 1 (two adjacent transform axes, the independent elements innermost) as the same two passes (fastn.h: fastn_cols_kernel on the
    // [ny][nx inner] view, fastn_fit_inner_kernel, fastn_irows_kernel).  n_c: the ny-point columns of the view; n_r: GE sequences of nx points per row workgroup
    int n_dbg = 0, fi_dbg = 0, fi_vec = 1;  // the measuring scripts' ablation switches (XRFTHIP_FASTN_DBG / _FI_DBG / _FI_VEC), read when the plan is made: xrfthip_exec reads no environment
    DevBuf winx_exp;                // the window along x expanded to the view's columns (never null: ones)
    // FastMY: pass 1 alone for ONE transform axis that is not the contiguous one (XRFTHIP_AXIS_Y, fastm_yonly_kernel)
    // FastMX: the same transform over short contiguous rows packed in pairs (ndim = 1, fastm_xonly_kernel)
    // FastG: ONE pass for a small real slab of any smooth shape, either precision, held in LDS with run-time radices (fastg.h)
    std::vector<int> g_rx, g_ry;
    DevBuf g_twx, g_twy, g_twr, g_revx, g_revy, g_isopos, g_isostart;
    std::vector<unsigned> g_hrevx, g_hrevy;  // (host copies: the radial-sum lists are built from them when the bin map arrives)
    bool g_one_d = false;  // ... the same kernel on groups of g_rows ROWS of a 1-D transform along x (no y passes, a mean / line per row)
    int g_rows = 0, g_lpr = 1, g_nred = 0;
    int g_rs = 0, g_n = 0;  // LDS row stride; length of the x transforms: nx / 2 (rows packed in pairs of samples) or nx (an odd nx)
    bool g_packed = true;
    // FastGY: ONE pass for one transform axis that is not the contiguous one (XRFTHIP_AXIS_Y), any smooth length, real input (fastg.h: fastgy_kernel)
    int gy_G = 0, gy_thr = 0, gy_blue_m = 0;  // gy_blue_m: Bluestein inside the tile on blue_m rows (a prime factor of ny with no butterfly)
    int gy_rad_p = 0;                         // ... or, ny = q p with ONE such prime p <= 127 and p - 1 smooth: the prime-factor form with Rader's algorithm along p
    bool gy_rows = false;                     // ... the same form along the CONTIGUOUS axis of a 1-D plan ([batch rows][nx samples]; fastgy_kernel FORM 3): gy_n = nx
    long long gy_n = 0;                       // the transform length of a fastgy plan
    std::vector<int> gy_rp;                   // the radices of p - 1
    DevBuf gy_twp, gy_radb, gy_permin;
    bool gy_tw_lds = true;
    size_t gy_lds = 0;
    DevBuf gy_bluec, gy_blueb;
    size_t g_lds = 0;
    // FastH: the last pass of a three-axis power / cross spectrum (fasth.h): h_G columns of the half spectrum per workgroup.  It shares FastG's fields for the
    // radices, twiddles and digit reversal of nt: g_ry, g_twy, g_revy, g_hrevy
    int h_G = 0, h_thr = 0;
    size_t h_lds = 0;
    std::vector<double> h_host_ph[3];  // XRFTHIP_HERM_FIELD: the output phase along t, herm_ny, herm_nx as handed to xrfthip_plan_set_phase (empty = none) ...
    DevBuf h_ph[3];                    // ... and in the plan's precision on the device: all three (ones for an axis without a table) or none
    // FastS: ONE pass for a small real float32 slab that fits the registers of a CU: 256 x 256 power spectra (fasts.h)
    DevBuf tw_sy, tw_sx, s_tfirst;
    long long tune_sstagger = 0;  // XRFTHIP_FASTS_STAGGER: classes << 8 | steps of 3.4 us between the classes of a resident set of slab workgroups
    long long tune_sgrid = -1;    // XRFTHIP_FASTS_GRID: workgroups of the launch (0 = one per slab, the default; else a resident set walking the slabs)
    // FastR: ONE pass for a long real float32 row that fits the registers of a CU: 65536 samples per workgroup (fastr.h); FastRComplex: its
    // complex-row form, rows of 2048 .. 16384 complex64 points, forward or inverse (fastc_kernel); FastRRows: complex rows of 256 .. 4096
    // points, pass 2 of the complex two-pass pipeline on the rows of the input itself (fastyc_rows_kernel, nrows > 0)
    // FastYCFourStep: ONE long complex sequence per batch entry (ndim = 1, 2^16 .. 2^20 points): the [n / 256][256] view, the four-step form of pass 2 (FastYC::fs)
    DevBuf fs_phx;                // ... the x factor of a separable input phase (PHASE_IN): 256 entries (fph[0]: the factor per row of the view)
    DevBuf tw_rm, tw_rs, tw_rn;   // W_M^p (p < 1024), W_1024^n (n < 32), W_N^p (p < 1024)
    long long tune_rstagger = 0;  // XRFTHIP_FASTR_STAGGER: classes << 8 | units of 3.4 us between the start of consecutive classes of workgroups (FastR::stagger)
    long long tune_rgrid = 0;     // XRFTHIP_FASTR_GRID: workgroups of the launch (0 = one per row; default: a resident set of one per CU walking the rows)
    bool fph_on = false;  // some entry of the combined phase tables (fph) differs from 1
    long long yny = 0, ynx = 0;
    DevBuf tw_big1d;
    int y_nrow_pad = 0;  // rows ky = 0..ny/2 of the intermediate, rounded up to what one row workgroup covers
    DevBuf ywhat0, ywhat1, ytcodes;
    DevBuf ytfirst, ytwin, ytunits;  // (ytwin: the bins each unit of rows reaches; ytunits: the units that reach each bin)
    bool ytfirst_on = false;       // ... and a radial map's: the radial sums are gathered per bin without atomics (fasty_build_tcodes)
    bool ytcodes_compact = false;  // the bin map has a radial map's structure: 4 bytes per 16 samples (fasty_build_tcodes)
    std::vector<double> host_win_y;
    std::vector<double> host_win_x;  // (four-step 1-D: the window of the whole sequence)
    DevBuf win2d;                    // ... as float32, laid out like the slab [yny][ynx]
    bool fast1d_win = false;         // the four-step plan carries a window: slab-shaped window table, per-column window spectra
    // tuning knobs from the environment, read once when the plan is created (never in xrfthip_exec)
    long long tune_group = 0, tune_fast_group = 0, tune_group_bytes = 512LL << 20, tune_cols_grid = 256, tune_max_grid = 8192;
    // optional per-pass event timing (bench only; a plan with profiling on is not re-entrant)
    bool prof = false;
    struct ProfRec { std::string label; hipEvent_t a, b; };
    std::vector<ProfRec> prof_recs;
    void prof_clear() { for (auto& r : prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); } prof_recs.clear(); }
    // xrfthip_desc.inner > 1: [batch][ny][nx][inner], two adjacent transform axes with the independent elements innermost.  A
    // composite of two in-place one-axis plans (XRFTHIP_AXIS_Y): sub_x transforms x of [batch ny][nx][inner], sub_y transforms y of
    // [batch][ny][nx inner]; a detrend runs first as a pass of its own (plane_inner_* kernels).  No transposed copy anywhere.
    long long inner = 1, mid = 1;
    bool sub_x_1d = false;  // the x stage is a 1-D plan (nothing behind x: inner = 1), its axis is 1
    xrfthip_plan* sub_x = nullptr;
    xrfthip_plan* sub_y = nullptr;
    size_t off_sub = 0, off_det = 0, off_mid = 0, off_dws = 0;
    // xrfthip_desc.mean_batch > 1 (fasty_mean.h, fasts_mean.h): mean_P runs per output (and group of slabs), each with a float64 partial of its own at off_mean --
    // [batch / M][mean_P][ny/2 + 1][nx] (x2 complex) -- summed in order by mean_finish_kernel
    int mean_P = 1;
    long long mean_run = 0;        // the longest run of slabs one workgroup walks (describe)
    long long tune_mean_runs = 0;  // XRFTHIP_MEAN_RUNS: runs per output, 0 = chosen by mean_layout
    size_t off_mean = 0;
    // XRFTHIP_OUT_COHERENCE: the descriptor says OUT_CROSS from xrfthip_plan_create on -- every check, table, family and the column pass are the CROSS mean plan's -- and
    // this remembers what the row pass sums (fasty_rows_mean_kernel<NX, 3>: re C, im C, A, B per sample) and what mean_finish writes (|C|^2 / (A B), real)
    bool coherence = false;
    // FastW / FastK (xrfthip_desc.seg_hop): samples between series (the descriptor's in_stride_batch, or the dense span; d.in_stride_batch is 0 from xrfthip_plan_create on),
    // the tile of a workgroup (the family's layout entry), and FastK's W_L^k of the unpacking
    long long w_pitch = 0;
    SegGeom w;
    DevBuf w_twr;
    DevBuf w_taps;                 // the multitaper form (xrfthip_desc.seg_tapers): the table [K][N] float32, xrfthip_plan_set_tapers
    ~xrfthip_plan() { for (auto* b : extra) delete b; prof_clear(); delete sub_x; delete sub_y; }
};


// geometry of the y-first float32 kernels as the host needs it (host_fasty.cpp; host_rows.cpp runs their row pass on the input's own rows)
struct YGeomRt { int thr, gxy, cw, rk, lbs; size_t lds; };

// What xrfthip_exec hands a family's launcher: the caller's buffers (out: null when the spectrum is not stored), the workspace, the stream.
// p1_block / p1_mode: per field, xrfthip_exec_args.field (0 = private: pass 1 of the field writes into the workspace; only FastY takes anything else).
struct ExecArgs { const void* in0; const void* in1; void* out; double* iso; char* ws; hipStream_t stream; char* p1_block[2] = {nullptr, nullptr}; uint32_t p1_mode[2] = {0, 0}; };

// One row per Family: the host side of a kernel family, defined in the unit that owns it (the file map above) and found through family_ops().
// A null entry: nothing to do / no / none.
struct FamilyOps {
    Family family;                                                         // the row's own place in the table (checked once, set_kernel_attrs_once)
    int (*run)(const xrfthip_plan*, const ExecArgs&);                      // the launcher: neither allocates, nor synchronises, nor reads the environment
    void (*describe)(const xrfthip_plan*, std::string&, const char* in_note);  // the family's lines of xrfthip_plan_describe (in_note: the strided-input note, "" on a dense plan)
    void (*kernel_info)(const xrfthip_plan*, int32_t* kind, int32_t* per_workgroup);
    int (*finalize)(xrfthip_plan*) = nullptr;                              // the tables that depend on windows / phases; may hand the plan on (settle_family)
    void (*layout)(xrfthip_plan*) = nullptr;                               // G and the workspace offsets (null: the family laid out its own when it was created)
    int (*binmap)(xrfthip_plan*, const int32_t*) = nullptr;                // the reaction to a bin map, looked up by `chosen`; may hand the plan on
    bool (*uses_bluestein)(const xrfthip_plan*) = nullptr;
    bool reads_strided = false;                                            // real input addressed as in + slab * in_stride_batch + y * in_stride_y + x ...
    bool (*strided_if)(const xrfthip_plan*) = nullptr;                     // ... where this holds, too
    bool dbl_tables = false;                                               // float64 phase / window-spectrum tables in a float64 plan
    bool two_pass_y = false;                                               // columns -> [fit] -> rows: the y-first intermediate, per-column sums and corrections
    bool fastm_pipeline = false;                                           // ... of fastm.h / fastn.h
    bool inner_layout = false;                                             // xrfthip_desc.inner / .mid: a header and a workspace of their own, no tile passes
    bool no_generic_passes = false;                                        // the family serves every plan it takes: no tile passes are built behind it
};
const FamilyOps& family_ops(Family f);
extern const FamilyOps kOpsComposite, kOpsFusedInner, kOpsFastS, kOpsFastG, kOpsFastGY, kOpsFastMX, kOpsFastMY, kOpsFastR, kOpsFastRComplex, kOpsFastRRows, kOpsFastW, kOpsFastK, kOpsFastYC,
    kOpsFastYCFourStep, kOpsFastY, kOpsFastY1D, kOpsFastM, kOpsFastN, kOpsFastH;

// ---- host functions more than one translation unit of the library calls (xrft_hip.cpp, host_*.cpp, ops.cpp)
// xrft_hip.cpp
void appendf(std::string& s, const char* fmt, ...);  // (describe)
int upload_real_table(xrfthip_plan* P, DevBuf& buf, const double* h, int64_t n, int cplx);
int plan_twiddle(xrfthip_plan* P, DevBuf& buf, long long N, long long count);
int plan_ones(xrfthip_plan* P, long long n);
void settle_family(xrfthip_plan* P, bool decline = false);
void layout_one_pass(xrfthip_plan* P);  // the layout entry of the rows: no workspace ...
void layout_passes(xrfthip_plan* P);    // ... or the generic passes' / the two y-first passes' workspace
int iso_chunk_count(long long total);
int run_radial_sums(int32_t dtype, const void* spec, const int32_t* d_binmap, long long bc, long long ny, long long nxo, int sy, int sx, int nbins, int chunks, double* part, double* iso, hipStream_t st);
xrfthip_plan::ProfRec* prof_begin(const xrfthip_plan* P, const std::string& label, hipStream_t st);
void prof_end(xrfthip_plan::ProfRec* r, hipStream_t st);
// host_fasty.cpp
bool cross_iso_phase(const xrfthip_plan* P);
int fast_phase_tables(xrfthip_plan* P);
int one_axis_tables(xrfthip_plan* P);  // ... and a window on the rotated input of an inverse one-axis plan handed to the generic passes
int two_pass_tables(xrfthip_plan* P);
YGeomRt ycols_geom(long long ny);
YGeomRt yrows_geom(long long nx, bool fs = false);
long long fasty_rows_gx(const xrfthip_plan* P);
int build_unit_windows(xrfthip_plan* P, const int32_t* bm, int rpu);
bool fasty_fits(const xrfthip_plan* P);
int fasty_tables(xrfthip_plan* P);
size_t fasty_pass1_bytes(const xrfthip_plan* P);
uint64_t fasty_pass1_signature(const xrfthip_plan* P, int field);
// host_fastm.cpp
bool fastm_iso_fused(const xrfthip_plan* P);
int fastm_rows_rpu(const xrfthip_plan* P);
bool fastn_factor(long long n, int maxr, std::vector<int>& out, int need_last = 0);
bool fastn_pick(long long n, int g, bool blue, bool dbl, bool cols, int maxr, int thr_force, NGeo& out);
size_t fastn_lds(const NGeo& g, size_t csize, bool cols);
void fastn_launch_cols(const xrfthip_plan* P, const FastM& m, hipStream_t st);
template <typename T> int fastn_upload_twm(const NGeo& g, DevBuf& buf, bool blue = false);  // (both precisions instantiated where it is defined)
// host_fastg.cpp
bool rader_split(long long n, bool allow17, int& p_out, std::vector<int>& rq, std::vector<int>& rp);
template <typename T> int fastn_rader_tables(xrfthip_plan* P);  // (both precisions instantiated where it is defined)
// host_inner.cpp, ops.cpp
int create_inner_plan(xrfthip_plan** plan, const xrfthip_desc& d);
size_t detrend_inner_ws(bool cplx, long long batch, long long inner);
int run_detrend_inner(int32_t dtype, int32_t ndim, long long batch, long long ny, long long nx, long long inner, int32_t kind, const void* in, void* out, char* ws, hipStream_t st, long long mid = 1);
// the kernels of each unit that take more than 64 KB of dynamic LDS (set_kernel_attrs_once)
void set_attrs_fasty();
void set_attrs_fastm();
void set_attrs_fastg();
void set_attrs_rows();
void set_attrs_welch();
// host_welch.inc: the checks of xrfthip_desc.seg_* (xrfthip_plan_create, on its copy of the descriptor); *pitch: samples between series
int seg_desc_check(xrfthip_desc& d, long long* pitch);

// the families' try_* (xrfthip_plan_create calls them in this order; the first that does not return kDeclined decides)
int try_fastw(xrfthip_plan* P);
int try_fasth(xrfthip_plan* P);
int try_fasts(xrfthip_plan* P);
int try_fastyc(xrfthip_plan* P);
int try_fastr(xrfthip_plan* P);
int try_fasty(xrfthip_plan* P);
int try_fast1d(xrfthip_plan* P);
int try_fastm(xrfthip_plan* P);
int try_fastmx(xrfthip_plan* P);
int try_fastmy(xrfthip_plan* P);
int try_fastgy(xrfthip_plan* P);
int try_fastg(xrfthip_plan* P);
int try_fastn(xrfthip_plan* P);

inline bool fasty_len(long long n) { return n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096; }  // the lengths of fasty.h / fasty_c2c.h
inline bool plan_two(const xrfthip_plan* P) { return P->d.out_mode == XRFTHIP_OUT_CROSS || P->d.out_mode == XRFTHIP_OUT_PHASE; }
inline int ilog2i(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// sets of families: each a lookup of the plan's row
inline bool fastm_pipeline(const xrfthip_plan* P) { return family_ops(P->family).fastm_pipeline; }
inline bool two_pass_y(const xrfthip_plan* P) { return family_ops(P->family).two_pass_y; }
inline bool inner_layout(const xrfthip_plan* P) { return family_ops(P->family).inner_layout; }
inline bool dbl_phase_tables(const xrfthip_plan* P) { return P->dbl && family_ops(P->family).dbl_tables; }
inline bool herm_field_plan(const xrfthip_plan* P) { return P && P->d.herm_ny > 0 && (P->d.flags & XRFTHIP_HERM_FIELD); }  // (... whose last pass writes the complex field)
// The mean over the batch inside the last pass (xrfthip_desc.mean_batch, normalised by xrfthip_plan_create: 0 = off, else M > 1): the families with a mean form are
// FastY's two-pass slabs and FastS below 256 points per axis with dense float32 input; every other family answers XRFTHIP_UNSUPPORTED_LENGTH (the caller composes).
inline bool mean_plan(const xrfthip_plan* P) { return P->d.mean_batch > 1 && !P->d.seg_keep && !P->d.seg_synth && !P->d.seg_filter; }  // (seg_keep, seg_synth, seg_filter: mean_batch counts the segments of a series, nothing is averaged)
inline bool mean_family(const xrfthip_plan* P) { return P->family == Family::FastY || (P->family == Family::FastS && !P->coherence) || P->family == Family::FastW; }  // (FastS has no two-field form)
size_t mean_layout(xrfthip_plan* P, size_t off, long long units, long long slabs);  // (xrft_hip.cpp: mean_P and the partials behind `off`; returns the new end)
int run_mean_finish(const xrfthip_plan* P, const double* part, void* out, hipStream_t st);  // (... and the finishing kernel, after the last group)
inline bool welch_cols(const xrfthip_plan* P) { return P->d.seg_hop > 0 && P->d.seg_stride > 0; }  // (... along a leading axis: d.inner adjacent series, samples d.seg_stride apart; S = 1 was normalised to 0, the rows layout -- but for the filter's column layout, filter_cols())
inline bool welch_plan(const xrfthip_plan* P) { return P->d.seg_hop > 0; }  // (the descriptor asks for the segments of a series: served by FastW / FastK or not at all)
inline bool keep_plan(const xrfthip_plan* P) { return P->d.seg_hop > 0 && P->d.seg_keep == 1; }  // (... every segment's spectrum kept, none averaged: Family::FastK, fastk.h)
inline bool synth_plan(const xrfthip_plan* P) { return P->d.seg_hop > 0 && P->d.seg_synth == 1; }  // (... the series rebuilt from its segments' half spectra: the synthesis form of Family::FastK, fasto.h)
inline bool filter_plan(const xrfthip_plan* P) { return P->d.seg_hop > 0 && P->d.seg_filter == 1; }  // (... a series filtered by overlap-save: the filter form of Family::FastK, fastf.h)
inline bool filter_cols(const xrfthip_plan* P) { return filter_plan(P) && P->d.seg_filter_cols == 1; }  // (... its column layout: welch_cols() holds too -- seg_stride >= 1 is kept as it came, S = 1 included)
inline bool taper_plan(const xrfthip_plan* P) { return P->d.seg_tapers > 0; }  // (... the sum over K tapers of one series' spectra: the multitaper form of Family::FastW, fastt.h; seg_hop = 0)
inline bool herm_plan(const xrfthip_plan* P) { return P->d.herm_ny > 0; }  // (the DESCRIPTOR asks for the last pass of a three-axis spectrum: argument checks; the family that serves it is Family::FastH)
// Input strides (xrfthip_desc.in_stride_y / in_stride_batch, normalised by xrfthip_plan_create: both 0 on a dense plan).  Only the kernels that read the caller's
// input take them: pass 1 of the two-pass families, the load of the one-pass families.  The intermediate and the output are dense.
inline bool in_strided(const xrfthip_plan* P) { return P->d.in_stride_y != 0 || P->d.in_stride_batch != 0; }
inline long long in_pitch(const xrfthip_plan* P) { return P->d.in_stride_y ? P->d.in_stride_y : P->d.nx; }               // elements between rows (real-input families: rows of nx)
inline long long in_slab(const xrfthip_plan* P) { return P->d.in_stride_batch ? P->d.in_stride_batch : P->d.ny * P->d.nx; }  // elements between slabs
// Half-precision input (xrfthip_plan::in16): read dense by the float32 families' own input pass -- the two y-first passes (and their four-step 1-D form), the register-
// resident slabs and rows, the one-pass slabs and row groups with real input.  Every other family: XRFTHIP_UNSUPPORTED_LENGTH from xrfthip_plan_create or from the
// xrfthip_plan_set_* call that moves the plan there (the caller widens with xrfthip_convert and takes the float32 plan).
inline bool in_half(const xrfthip_plan* P) { return P->in16 != 0; }
inline bool half_family(const xrfthip_plan* P) {
    const Family f = P->family;
    return !P->dbl && !P->cplx_in && (f == Family::FastY || f == Family::FastY1D || f == Family::FastS || f == Family::FastR || f == Family::FastG);
}
inline bool family_reads_strided(const xrfthip_plan* P) {  // (the complex-input forms are kernels of their own)
    const FamilyOps& o = family_ops(P->family);
    return o.reads_strided && !P->cplx_in && (!o.strided_if || o.strided_if(P));
}
