// fasts_mean.h -- the pieces of fasts_power_kernel<.., MEAN> (fasts.h includes this file behind its geometry): the mean over M consecutive slabs inside the one pass
// (xrfthip_desc.mean_batch, see fasty_mean.h).  A thread holds the same (row, kx) set on every trip of the slab loop, so the sums are 32 floats in the layout of b[]
// (+ 2 for the thread that holds the four real corner samples); after at most kMeanChain slabs they leave through the staged rows of the plain kernel into the
// workgroup's own float64 partial [output][P][NY/2 + 1][NX], which mean_finish_kernel (fasty_mean.h) turns into the output.
#pragma once
#include "fasty_mean.h"

namespace xrft {

// what fasts_power_kernel<.., MEAN> carries across the back edge of its slab loop; the other instantiations carry an empty object
template <bool MEAN> struct FastSMeanState {};
template <> struct FastSMeanState<true> {
    float acc[32], accx[2];  // the sums in the layout of b[]; the two extra real corner samples of the thread that holds them
    int chain;               // slabs added since the last flush
    bool first;              // nothing flushed yet: the partial is written, not added to
    long long lo, hi;        // the run of slabs: run wg % mean_p of output wg / mean_p
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int e = 0; e < 32; ++e) acc[e] = 0.f;
        accx[0] = accx[1] = 0.f;
        chain = 0;
    }
    template <typename Params> __device__ __forceinline__ void init(const Params& p, long long wg) {
        const long long o = wg / p.mean_p, q = wg % p.mean_p;
        lo = o * p.mean_m + q * p.mean_m / p.mean_p;
        hi = o * p.mean_m + (q + 1) * p.mean_m / p.mean_p;
        first = true;
        clear();
    }
};

// acc += |F|^2 scale of this slab, register by register, READ BACK from the rows the plain kernel's own staging code has just written (a thread reads only what it
// wrote itself: no barrier).  The values are therefore the plain kernel's to the bit -- squared by the same statements, not by a copy of them whose fused
// multiply-adds the compiler may form differently -- and a slab stored twice averages to the plain plan's result exactly.
template <int RY, int RX> __device__ __forceinline__ void fasts_mean_accumulate(const float* Lf, float* acc, float* accx, int row, int cx) {
    typedef SGeom<RY, RX> G;
    constexpr int NX = G::NX, NROW = G::NROW, KGX = G::KGX, PF = G::PF, HX = RX / 2;
    if (row != 0) {
#pragma unroll
        for (int g = 0; g < KGX; ++g)
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int k2 = 0; k2 < RX; ++k2) acc[(4 * g + w) * RX + k2] = mean_add(acc[(4 * g + w) * RX + k2], Lf[row * PF + fasts_k1(cx * KGX + g, w) + 32 * k2]);
        return;
    }
    // the packed row: the lower register stands for F[0][idx], its partner for F[NY/2][idx]; idx = 0 carries the four real corner samples
#pragma unroll
    for (int g = 0; g < KGX; ++g)
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int k2 = 0; k2 < HX; ++k2) {
                const int idx = fasts_k1(cx * KGX + g, w) + 32 * k2, ie = (4 * g + w) * RX + k2, io = (4 * g + (w ^ 1)) * RX + RX - 1 - k2;
                acc[ie] = mean_add(acc[ie], Lf[idx]);
                acc[io] = mean_add(acc[io], Lf[NROW * PF + idx]);
                if (idx == 0) {
                    accx[0] = mean_add(accx[0], Lf[NX / 2]);
                    accx[1] = mean_add(accx[1], Lf[NROW * PF + NX / 2]);
                }
            }
}

// the sums staged as float rows (row r, 0 <= r <= NY/2, at r PF + kx: the plain kernel's layout), between two barriers of the caller's
template <int RY, int RX> __device__ __forceinline__ void fasts_mean_stage(const float* acc, const float* accx, float* Lf, int row, int cx) {
    typedef SGeom<RY, RX> G;
    constexpr int NX = G::NX, NROW = G::NROW, KGX = G::KGX, PF = G::PF, HX = RX / 2;
    if (row != 0) {
#pragma unroll
        for (int g = 0; g < KGX; ++g)
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int k2 = 0; k2 < RX; ++k2) Lf[row * PF + fasts_k1(cx * KGX + g, w) + 32 * k2] = acc[(4 * g + w) * RX + k2];
        return;
    }
#pragma unroll
    for (int g = 0; g < KGX; ++g)
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int k2 = 0; k2 < HX; ++k2) {
                const int idx = fasts_k1(cx * KGX + g, w) + 32 * k2;
                const float pe = acc[(4 * g + w) * RX + k2], po = acc[(4 * g + (w ^ 1)) * RX + RX - 1 - k2];
                if (idx == 0) {
                    Lf[0] = pe; Lf[NX / 2] = accx[0];
                    Lf[NROW * PF] = po; Lf[NROW * PF + NX / 2] = accx[1];
                } else {
                    Lf[idx] = pe; Lf[NX - idx] = pe;
                    Lf[NROW * PF + idx] = po; Lf[NROW * PF + NX - idx] = po;
                }
            }
}

}  // namespace xrft
