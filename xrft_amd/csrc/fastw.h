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
#include "tile_fft.h"

namespace xrft {

constexpr int kWThreads = 256;   // threads of a fastw workgroup
constexpr int kWPoints = 4096;   // complex points of one field's tile: G = min(kWPoints / L, pairs of the longest run) sequences
constexpr int kWAcc = kWPoints / kWThreads;  // tile positions (float32 sums) per thread and field
constexpr int kWCols = 32;       // the column layout: adjacent columns per workgroup where the tile holds them (128 bytes of one time row per wave-load)
constexpr int kWColsMaxL = 512;  // ... and its longest segment: 8 columns of 512 points fill the tile (a 32-byte piece of a time row per row of the load)
constexpr const char* kWColsResources = "115 VGPRs, no scratch, 4 waves per SIMD (two fields: 164 VGPRs, 3 waves)";  // (scripts/kernel_resources.sh, gfx950: the rows kernels' figures)

struct FastW {
    const float* in0;
    const float* in1;          // the second field (CROSS), same layout
    double* part;              // [output][P][L] float64 (x2 complex: CROSS)
    const cf* tw;              // W_L^k, k < L
    const unsigned* rev;       // rev[k] = tile position of frequency k after the passes
    const float* win;          // L window values, or null
    long long pitch;           // samples between series (the column layout: between blocks)
    long long hop;             // samples between segment starts
    long long sstride;         // the column layout: elements between consecutive samples of a series (S)
    int L, M, P, G;            // segment length, segments per series, runs per series, sequences (pairs of segments) per round
    int seq_stride, pad_shift; // the tile: sequence t at t * seq_stride, point p at p + (p >> pad_shift)
    int nr, radix[XRFT_MAX_PASSES];
    int detrend;
    float scale;
    int inner, lgC, ngroups;   // the column layout: columns per block, log2 of the columns per workgroup (C), groups of C columns per block
};

// Who owns the sequences of a tile.  Rows layout (COLS = false): all G sequences are pairs of segments of ONE series.  Column layout: a workgroup has C adjacent
// columns of one block, sequence t = (column t % C, pair t / C): G / C pairs of every column per round.  Tile segment sg = 2 t + (member of the pair).
template <bool COLS>
struct WOwner {
    int lgC, live;  // log2 C; the columns of this group that exist (the last group of a block may hold fewer than C: the rest are zeros and write nothing)
    __device__ __forceinline__ int col(int sg) const { return COLS ? ((sg >> 1) & ((1 << lgC) - 1)) : 0; }
    __device__ __forceinline__ int seg(int sg) const { return COLS ? ((((sg >> 1) >> lgC) << 1) | (sg & 1)) : sg; }  // the segment of its column, from the round's first
    __device__ __forceinline__ bool has(int sg, long long s0, long long s_hi) const { return s0 + seg(sg) < s_hi && (!COLS || col(sg) < live); }
};

// one field's 2 G tile segments from segment `s0` on (those below s_hi; the rest zeros) into its tile, detrended and windowed.  red: 2 * kWThreads doubles, coef: 2 * 2 * G doubles
// src: the first sample of the series (COLS: of the group's first column).  COLS: the load loop runs column fastest, then sample, then segment -- consecutive lanes
// read consecutive addresses of one time row; the index (s H + j) S + e in 64 bits
template <bool COLS>
__device__ __forceinline__ void fastw_load(const FastW& p, const WOwner<COLS>& ow, const float* __restrict__ src, long long s0, long long s_hi, cf* tile, double* red, double* coef, int tid) {
    const int L = p.L, lgL = 31 - __builtin_clz((unsigned)L), nseg = 2 * p.G, total = nseg * L;
    const bool det = p.detrend != 0;
    for (int e = tid; e < total; e += kWThreads) {
        int sg, j;
        long long off;
        bool on;
        if (COLS) {
            const int c = e & ((1 << ow.lgC) - 1), r = e >> ow.lgC, sl = r >> lgL;  // column of the group, (segment of the round, sample)
            j = r & (L - 1);
            sg = ((((sl >> 1) << ow.lgC) | c) << 1) | (sl & 1);
            on = s0 + sl < s_hi && c < ow.live;
            off = ((s0 + sl) * p.hop + j) * p.sstride + c;
        } else {
            sg = e >> lgL; j = e & (L - 1);
            on = s0 + sg < s_hi;
            off = (s0 + sg) * p.hop + j;
        }
        float v = 0.f;
        if (on) {
            v = src[(size_t)off];
            if (!det && p.win) v *= p.win[j];
        }
        float* dst = reinterpret_cast<float*>(tile + (sg >> 1) * p.seq_stride + phys(j, p.pad_shift));
        dst[sg & 1] = v;
    }
    __syncthreads();
    if (!det) return;
    // per segment: sum x and sum (j - c) x, c = (L - 1) / 2, float64; tps threads per segment, then a tree over them (a fixed order)
    const int tps = kWThreads / nseg, seg = tid / tps, lane = tid % tps;  // (nseg <= 128: tps >= 2, a power of two)
    const double c = 0.5 * (double)(L - 1);
    {
        const float* col = reinterpret_cast<const float*>(tile + (seg >> 1) * p.seq_stride) + (seg & 1);
        double s0x = 0.0, s1x = 0.0;
        for (int j = lane; j < L; j += tps) {
            const double x = (double)col[2 * phys(j, p.pad_shift)];
            s0x += x;
            s1x += ((double)j - c) * x;
        }
        red[2 * tid] = s0x;
        red[2 * tid + 1] = s1x;
    }
    __syncthreads();
    for (int w = tps >> 1; w >= 1; w >>= 1) {
        if (lane < w) {
            red[2 * tid] += red[2 * (tid + w)];
            red[2 * tid + 1] += red[2 * (tid + w) + 1];
        }
        __syncthreads();
    }
    if (lane == 0) {
        const double Ld = (double)L;
        coef[2 * seg] = red[2 * tid] / Ld;  // the mean
        coef[2 * seg + 1] = p.detrend == 2 ? red[2 * tid + 1] / (Ld * (Ld * Ld - 1.0) / 12.0) : 0.0;  // the slope of the least-squares line about c
    }
    __syncthreads();
    for (int e = tid; e < total; e += kWThreads) {
        const int sg = e >> lgL, j = e & (L - 1);
        float* dst = reinterpret_cast<float*>(tile + (sg >> 1) * p.seq_stride + phys(j, p.pad_shift)) + (sg & 1);
        float v = 0.f;
        if (ow.has(sg, s0, s_hi)) {  // (a missing segment stays zero whatever the window)
            v = (float)((double)*dst - (coef[2 * sg] + coef[2 * sg + 1] * ((double)j - c)));
            if (p.win) v *= p.win[j];
        }
        *dst = v;
    }
    __syncthreads();
}

__device__ __forceinline__ void fastw_fft(const FastW& p, cf* tile, int tid) {
    TileGeom g{};
    g.n = p.L; g.T = p.G; g.seq_stride = p.seq_stride; g.pad_shift = p.pad_shift;
    int L = p.L;
    for (int ip = 0; ip < p.nr; ++ip) {
        const int R = p.radix[ip];
        switch (R) {
            case 2: run_pass<float, 2>(tile, g, L, tid, kWThreads, p.tw); break;
            case 4: run_pass<float, 4>(tile, g, L, tid, kWThreads, p.tw); break;
            case 8: run_pass<float, 8>(tile, g, L, tid, kWThreads, p.tw); break;
            default: run_pass<float, 16>(tile, g, L, tid, kWThreads, p.tw); break;
        }
        L /= R;
        __syncthreads();
    }
}

// LDS: [tile 0][tile 1 (TWO)][red: 2 kWThreads doubles][coef: 4 G doubles]
// COLS: the column layout (xrfthip_desc.seg_stride) -- blockIdx = ((block, group of C columns), run); the float64 sum at the end of a chain runs over the G / C pairs
// of ONE column, into that column's own partial; columns beyond `inner` in the last group write nothing
template <bool TWO, bool COLS = false>
__global__ void __launch_bounds__(kWThreads) fastw_kernel(FastW p) {
    XRFT_DYN_SMEM(smem_raw);
    const int tid = threadIdx.x;
    const int tile_elems = (p.G * p.seq_stride + 1) & ~1;  // (16-byte multiples: the doubles behind the tiles stay aligned)
    cf* tile0 = reinterpret_cast<cf*>(smem_raw);
    cf* tile1 = tile0 + (TWO ? tile_elems : 0);
    double* red = reinterpret_cast<double*>(tile0 + (TWO ? 2 : 1) * tile_elems);
    double* coef = red + 2 * kWThreads;
    const long long u = (long long)blockIdx.x / p.P;  // the series (COLS: the group of columns, over all blocks)
    const int pp = (int)((long long)blockIdx.x % p.P);
    const long long s_lo = (long long)pp * p.M / p.P, s_hi = (long long)(pp + 1) * p.M / p.P;
    const long long blk = COLS ? u / p.ngroups : u;
    const long long c0 = COLS ? (u % p.ngroups) << p.lgC : 0;  // the group's first column
    WOwner<COLS> ow;
    ow.lgC = COLS ? p.lgC : 0;
    ow.live = !COLS ? 1 : ((long long)p.inner - c0 < (1LL << p.lgC) ? (int)((long long)p.inner - c0) : (1 << p.lgC));
    const int lgC = ow.lgC, Gp = p.G >> lgC;  // pairs of segments of one column per round
    const float* __restrict__ src0 = p.in0 + (size_t)blk * (size_t)p.pitch + (size_t)c0;
    const float* __restrict__ src1 = TWO ? p.in1 + (size_t)blk * (size_t)p.pitch + (size_t)c0 : src0;
    constexpr int CW = TWO ? 2 : 1;
    // the partial of output o (COLS: o = block * inner + column), run pp: [o][P][L]
    double* __restrict__ dst = p.part + (((size_t)blk * (size_t)(COLS ? p.inner : 1) + (size_t)c0) * p.P + pp) * (size_t)p.L * CW;
    const size_t dst_col = (size_t)p.P * (size_t)p.L * CW;  // between the partials of neighbouring columns
    const int L = p.L, lgL = 31 - __builtin_clz((unsigned)L), live = p.G * L;  // tile positions in use
    float acc[kWAcc * CW];
#pragma unroll
    for (int e = 0; e < kWAcc * CW; ++e) acc[e] = 0.f;
    int chain = 0;
    bool first = true;
    for (long long s = s_lo; s < s_hi; s += 2 * Gp) {
        fastw_load<COLS>(p, ow, src0, s, s_hi, tile0, red, coef, tid);
        if (TWO) fastw_load<COLS>(p, ow, src1, s, s_hi, tile1, red, coef, tid);
        fastw_fft(p, tile0, tid);
        if (TWO) fastw_fft(p, tile1, tid);
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
