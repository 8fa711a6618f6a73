// fastw.h -- Welch spectra (xrfthip_desc.seg_hop = H >= 1): the mean power / cross spectrum of the M overlapping L-sample segments of a long series, the segments
// read where they lie (segment s of series p starts at p * pitch + s * H) and their spectra never stored -- what the reference's users write as
// power_spectrum(da, dim="time", chunks_to_segments=True, window="hann", detrend="linear").mean("time_segment"), with the overlap of Welch's method.
//
//   fastw_kernel          one 256-thread workgroup walks one run of one series' segments, up to 2 G of them per round (G L = 4096 points at most): the samples are
//                         loaded with 4-byte loads (a segment start is on a 4-byte boundary only; consecutive lanes read consecutive samples, and the overlap of
//                         neighbouring segments is served by the cache), segments 2 t and 2 t + 1 PACKED as the real and imaginary part of sequence t of an LDS tile,
//                         detrended (mean or least-squares line per segment, sums in float64) and windowed in the tile, transformed by the in-place radix passes of
//                         tile_fft.h, and |Z|^2 scale (Z conj(Z') scale for two fields) is added into float32 registers, one per tile position the thread owns.
//                         The pair is never split: with Z = FFT(a + i b), |A_k|^2 + |B_k|^2 = (|Z_k|^2 + |Z_{L-k}|^2) / 2, and for two fields
//                         A_k conj(A'_k) + B_k conj(B'_k) = (D_k + conj(D_{L-k})) / 2 with D = Z conj(Z'): one symmetrisation, when the plan finishes.  An odd count
//                         pairs the last segment with zeros.  Both members of a pair belong to the same output: a non-finite sample reaches its own series only.
//                         After kMeanChain rounds (or the last) the registers are staged in the tile and added, float64, over the G sequences and into the
//                         workgroup's own partial [output][run][L] of the workspace, in natural frequency order (first chain: stored).  No atomics.
//                         The COLUMN layout (xrfthip_desc.seg_stride = S, fastw_kernel<TWO, true>): the series are `inner` adjacent columns of a block whose samples lie
//                         S elements apart -- a (time, y, x) cube read where it lies.  A workgroup takes one block, one group of C adjacent columns (C = 32 for
//                         L <= 128: 128 bytes of one time row per wave-load; 16 at L = 256 and 8 at L = 512, what the tile holds) and one run of segments;
//                         sequence t of the tile is (column t % C, pair t / C), both members of a pair from the SAME column; the load loop runs column fastest,
//                         then sample, then segment, the offset (s H + j) S + e in 64 bits; columns beyond `inner` in the last group load zeros and write
//                         nothing; at the end of a chain the float64 sum runs over the G / C pairs of one column, into that column's own partial.
//   fastw_finish_kernel   sums the runs of an output in order, symmetrises, x 1 / M, real-dim factor, true-phase factor (once, on the mean), fftshift or half output.
// The order of every addition is fixed by the plan (M, G, the runs): repeated calls return identical bits.  XRFTHIP_ISHIFT_X is a factor (-1)^k on each transform that
// cancels in |F|^2 and in F0 conj(F1): ignored.
#pragma once
#include "fasty_mean.h"
#include "seg_tile.h"

namespace xrft {

constexpr int kWAcc = kWPoints / kWThreads;  // tile positions (float32 sums) per thread and field: G = min(kWPoints / L, pairs of the longest run) sequences
constexpr const char* kWColsResources = "115 VGPRs, no scratch, 4 waves per SIMD (two fields: 164 VGPRs, 3 waves)";  // (scripts/kernel_resources.sh, gfx950: the rows kernels' figures)

struct FastW {
    SegTile t;                 // (tw: W_L^k, k < L)
    const float* in0;
    const float* in1;          // the second field (CROSS), same layout
    double* part;              // [output][P][L] float64 (x2 complex: CROSS)
    int P, G;                  // runs per series, sequences (pairs of segments) per round
};

// LDS: [tile 0][tile 1 (TWO)][red: 2 kWThreads doubles][coef: 4 G doubles]
// COLS: the column layout (xrfthip_desc.seg_stride) -- blockIdx = ((block, group of C columns), run); the float64 sum at the end of a chain runs over the G / C pairs
// of ONE column, into that column's own partial; columns beyond `inner` in the last group write nothing
template <bool TWO, bool COLS = false>
__global__ void __launch_bounds__(kWThreads) fastw_kernel(FastW a) {
    const SegTile& p = a.t;
    XRFT_DYN_SMEM(smem_raw);
    const int tid = threadIdx.x;
    const int tile_elems = (a.G * p.seq_stride + 1) & ~1;  // (16-byte multiples: the doubles behind the tiles stay aligned)
    cf* tile0 = reinterpret_cast<cf*>(smem_raw);
    cf* tile1 = tile0 + (TWO ? tile_elems : 0);
    double* red = reinterpret_cast<double*>(tile0 + (TWO ? 2 : 1) * tile_elems);
    double* coef = red + 2 * kWThreads;
    const int pp = (int)((long long)blockIdx.x % a.P);
    const long long s_lo = (long long)pp * p.M / a.P, s_hi = (long long)(pp + 1) * p.M / a.P;
    const SegUnit un = seg_unit<COLS>(p, (long long)blockIdx.x / a.P);
    const long long blk = un.blk, c0 = un.c0;
    PairLayout<COLS> ow;
    ow.lgC = COLS ? p.lgC : 0;
    ow.live = un.live;
    ow.s_hi = s_hi;
    const int lgC = ow.lgC, Gp = a.G >> lgC;  // pairs of segments of one column per round
    const float* __restrict__ src0 = a.in0 + (size_t)blk * (size_t)p.pitch + (size_t)c0;
    const float* __restrict__ src1 = TWO ? a.in1 + (size_t)blk * (size_t)p.pitch + (size_t)c0 : src0;
    constexpr int CW = TWO ? 2 : 1;
    // the partial of output o (COLS: o = block * inner + column), run pp: [o][P][L]
    double* __restrict__ dst = a.part + (((size_t)blk * (size_t)(COLS ? p.inner : 1) + (size_t)c0) * a.P + pp) * (size_t)p.L * CW;
    const size_t dst_col = (size_t)a.P * (size_t)p.L * CW;  // between the partials of neighbouring columns
    const int L = p.L, lgL = 31 - __builtin_clz((unsigned)L), live = a.G * L;  // tile positions in use
    float acc[kWAcc * CW];
#pragma unroll
    for (int e = 0; e < kWAcc * CW; ++e) acc[e] = 0.f;
    int chain = 0;
    bool first = true;
    for (long long s = s_lo; s < s_hi; s += 2 * Gp) {
        ow.s0 = s;
        seg_load<COLS>(p, ow, src0, 2 * a.G, tile0, red, coef, tid);
        if (TWO) seg_load<COLS>(p, ow, src1, 2 * a.G, tile1, red, coef, tid);
        seg_fft(p, L, a.G, tile0, tid);
        if (TWO) seg_fft(p, L, a.G, tile1, tid);
#pragma unroll
        for (int q = 0; q < kWAcc; ++q) {
            const int e = tid + q * kWThreads;
            if (e < live) {
                const int i = (e >> lgL) * p.seq_stride + phys(e & (L - 1), p.pad_shift);
                const cf z = tile0[i];
                if (TWO) {
                    const cf v = cscale(cmulc(z, tile1[i]), p.scale);
                    acc[CW * q] = mean_add(acc[CW * q], v.re);
                    acc[CW * q + (TWO ? 1 : 0)] = mean_add(acc[CW * q + (TWO ? 1 : 0)], v.im);
                } else {
                    acc[q] = mean_add(acc[q], (z.re * z.re + z.im * z.im) * p.scale);
                }
            }
        }
        if (++chain < kMeanChain && s + 2 * Gp < s_hi) { __syncthreads(); continue; }  // (the next round's loads overwrite the tile)
        // ---- the chain ends: every sum to its own tile position (nobody else reads or writes it), then per frequency the sequences of an output added in order, float64
#pragma unroll
        for (int q = 0; q < kWAcc; ++q) {
            const int e = tid + q * kWThreads;
            if (e < live) tile0[(e >> lgL) * p.seq_stride + phys(e & (L - 1), p.pad_shift)] = mk<float>(acc[CW * q], TWO ? acc[CW * q + (TWO ? 1 : 0)] : 0.f);
        }
        __syncthreads();
        for (int w = tid; w < (ow.live << lgL); w += kWThreads) {  // (rows layout: w = k)
            const int k = w & (L - 1), c = w >> lgL;
            const int pos = phys((int)p.rev[k], p.pad_shift);
            double sr = 0.0, si = 0.0;
            for (int t = 0; t < Gp; ++t) {
                const cf v = tile0[((t << lgC) + c) * p.seq_stride + pos];
                sr += (double)v.re;
                if (TWO) si += (double)v.im;
            }
            double* __restrict__ d = dst + (size_t)c * dst_col;
            if (TWO) {
                d[2 * k] = first ? sr : d[2 * k] + sr;
                d[2 * k + 1] = first ? si : d[2 * k + 1] + si;
            } else {
                d[k] = first ? sr : d[k] + sr;
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kWAcc * CW; ++e) acc[e] = 0.f;
        chain = 0;
        first = false;
    }
}

// out[o][c], c < nx_out: the P runs of frequency k and of L - k summed in order, the pair symmetrised ((S_k + S_{L-k}) / 2; CROSS: (D_k + conj(D_{L-k})) / 2), x 1 / M,
// x 2 for 0 < k < L / 2 of a real-dim output, x the true-phase factor of k (CROSS).  shift: c is the fftshifted place of k; nx_out = L / 2 + 1: the half output.
template <bool CPLX>
__global__ void __launch_bounds__(256) fastw_finish_kernel(const double* __restrict__ part, void* out, int L, int nx_out, int P, double half_inv_m, int shift, int realdim2,
                                                           const cf* __restrict__ ph, int ph_on) {
    const long long o = (long long)blockIdx.x;
    constexpr int CW = CPLX ? 2 : 1;
    const double* __restrict__ src = part + (size_t)o * P * (size_t)L * CW;
    for (int c = threadIdx.x; c < nx_out; c += 256) {
        const int k = (c - shift) & (L - 1), k2 = (L - k) & (L - 1);
        double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
        for (int q = 0; q < P; ++q) {
            const double* __restrict__ s = src + (size_t)q * L * CW;
            ar += s[(size_t)k * CW];
            br += s[(size_t)k2 * CW];
            if (CPLX) { ai += s[(size_t)k * CW + 1]; bi += s[(size_t)k2 * CW + 1]; }
        }
        const double f = half_inv_m * ((realdim2 && k > 0 && 2 * k < L) ? 2.0 : 1.0);
        const size_t oi = (size_t)o * nx_out + c;
        if (CPLX) {
            cf v = mk<float>((float)((ar + br) * f), (float)((ai - bi) * f));
            if (ph_on) v = cmul(v, ph[k]);
            reinterpret_cast<cf*>(out)[oi] = v;
        } else {
            reinterpret_cast<float*>(out)[oi] = (float)((ar + br) * f);
        }
    }
}

}  // namespace xrft
