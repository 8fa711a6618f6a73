// seg_tile.h -- what the two segment kernels share (fastw.h: Welch spectra, pairs of segments per sequence; fastk.h: spectrograms, a segment packed with itself):
// the head of their arguments, who a workgroup is, the load of the tile with detrend and window per segment, and the radix passes.  A kernel differs in its LAYOUT,
// a small type that says where sample j of tile segment sg lives and which tile segments exist (PairLayout, SelfLayout); everything here is inlined into the kernel.
#pragma once
#include "tile_fft.h"

namespace xrft {

constexpr int kWThreads = 256;   // threads of a segment workgroup
constexpr int kWPoints = 4096;   // complex points of one field's tile
constexpr int kWCols = 32;       // the column layout: adjacent columns per workgroup where the tile holds them (128 bytes of one time row per wave-load)
constexpr int kWColsMaxL = 512;  // ... and its longest segment: 8 columns of 512 points fill the tile (a 32-byte piece of a time row per row of the load)

struct SegTile {
    const cf* tw;              // W_n^k, k < n, n the points of a sequence
    const unsigned* rev;       // rev[k] = tile position of frequency k after the passes
    const float* win;          // L window values, or null
    long long pitch;           // samples between series (the column layout: between blocks)
    long long hop;             // samples between segment starts
    long long sstride;         // the column layout: elements between consecutive samples of a series (S)
    int L, M;                  // segment length, segments per series
    int seq_stride, pad_shift; // the tile: sequence t at t * seq_stride, point p at p + (p >> pad_shift)
    int nr, radix[XRFT_MAX_PASSES];
    int detrend;
    float scale;
    int inner, lgC, ngroups;   // the column layout: columns per block, log2 of the columns per workgroup (C), groups of C columns per block
};

// Unit u of the launch: a series, or (COLS) a group of C adjacent columns of a block.  live: the columns of the group that exist (the last group of a block may hold
// fewer than C: the rest load zeros and write nothing)
struct SegUnit { long long blk, c0; int live; };
template <bool COLS>
__device__ __forceinline__ SegUnit seg_unit(const SegTile& p, long long u) {
    SegUnit b;
    b.blk = COLS ? u / p.ngroups : u;
    b.c0 = COLS ? (u % p.ngroups) << p.lgC : 0;  // the group's first column
    b.live = !COLS ? 1 : ((long long)p.inner - b.c0 < (1LL << p.lgC) ? (int)((long long)p.inner - b.c0) : (1 << p.lgC));
    return b;
}

// The layouts.  A round holds the segments s0 .. of every column of the group (those below s_hi exist); (sl, c) = (segment of the round, column of the group).
// Pairs: segments 2 q and 2 q + 1 of a column are the real and the imaginary part of ONE sequence, t = (column t % C, pair t / C); tile segment sg = 2 t + member
template <bool COLS>
struct PairLayout {
    int lgC, live;
    long long s0, s_hi;
    __device__ __forceinline__ int tile_seg(int sl, int c) const { return COLS ? (((((sl >> 1) << lgC) | c) << 1) | (sl & 1)) : sl; }
    __device__ __forceinline__ int col(int sg) const { return COLS ? ((sg >> 1) & ((1 << lgC) - 1)) : 0; }
    __device__ __forceinline__ int seg(int sg) const { return COLS ? ((((sg >> 1) >> lgC) << 1) | (sg & 1)) : sg; }
    __device__ __forceinline__ bool has(int sg) const { return s0 + seg(sg) < s_hi && (!COLS || col(sg) < live); }
    __device__ __forceinline__ float* at(cf* tile, const SegTile& p, int sg, int j) const { return reinterpret_cast<float*>(tile + (sg >> 1) * p.seq_stride + phys(j, p.pad_shift)) + (sg & 1); }
};
// Self: a segment is a sequence of its own, samples 2 j and 2 j + 1 the real and the imaginary part of point j; tile segment sg = sequence (column sg % C, segment sg / C)
template <bool COLS>
struct SelfLayout {
    int lgC, live;
    long long s0, s_hi;
    __device__ __forceinline__ int tile_seg(int sl, int c) const { return (sl << lgC) | c; }
    __device__ __forceinline__ bool has(int sg) const { return s0 + (sg >> lgC) < s_hi && (sg & ((1 << lgC) - 1)) < live; }
    __device__ __forceinline__ float* at(cf* tile, const SegTile& p, int sg, int j) const { return reinterpret_cast<float*>(tile + sg * p.seq_stride + phys(j >> 1, p.pad_shift)) + (j & 1); }
};

// One field's nseg tile segments into its tile, detrended and windowed; a tile segment that does not exist is zeros whatever the window.  red: 2 * kWThreads doubles,
// coef: 2 * nseg doubles.  src: the first sample of the series (COLS: of the group's first column).  The samples are loaded with 4-byte loads (a segment start is on a
// 4-byte boundary only); COLS: the load loop runs column fastest, then sample, then segment -- consecutive lanes read consecutive addresses of one time row; the index
// (s H + j) S + e in 64 bits
template <bool COLS, class LAY>
__device__ __forceinline__ void seg_load(const SegTile& p, const LAY& lay, const float* __restrict__ src, int nseg, cf* tile, double* red, double* coef, int tid) {
    const int L = p.L, lgL = 31 - __builtin_clz((unsigned)L), total = nseg * L;
    const bool det = p.detrend != 0;
    for (int e = tid; e < total; e += kWThreads) {
        int c, sl, j;
        if (COLS) { c = e & ((1 << lay.lgC) - 1); const int r = e >> lay.lgC; sl = r >> lgL; j = r & (L - 1); }
        else { c = 0; sl = e >> lgL; j = e & (L - 1); }
        float v = 0.f;
        if (lay.s0 + sl < lay.s_hi && c < lay.live) {
            const long long off = COLS ? ((lay.s0 + sl) * p.hop + j) * p.sstride + c : (lay.s0 + sl) * p.hop + j;
            v = src[(size_t)off];
            if (!det && p.win) v *= p.win[j];
        }
        *lay.at(tile, p, lay.tile_seg(sl, c), j) = v;
    }
    __syncthreads();
    if (!det) return;
    // per segment: sum x and sum (j - c) x, c = (L - 1) / 2, float64; tps threads per segment, then a tree over them (a fixed order)
    const int tps = kWThreads / nseg, seg = tid / tps, lane = tid % tps;  // (nseg <= 128: tps >= 2, a power of two)
    const double c = 0.5 * (double)(L - 1);
    {
        double s0x = 0.0, s1x = 0.0;
        for (int j = lane; j < L; j += tps) {
            const double x = (double)*lay.at(tile, p, seg, j);
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
        float* dst = lay.at(tile, p, sg, j);
        float v = 0.f;
        if (lay.has(sg)) {  // (a missing segment stays zero whatever the window)
            v = (float)((double)*dst - (coef[2 * sg] + coef[2 * sg + 1] * ((double)j - c)));
            if (p.win) v *= p.win[j];
        }
        *dst = v;
    }
    __syncthreads();
}

// T transforms of n points, in place: the radix passes of tile_fft.h (radices 2, 4, 8, 16: the host declines every other length)
__device__ __forceinline__ void seg_fft(const SegTile& p, int n, int T, cf* tile, int tid) {
    TileGeom g{};
    g.n = n; g.T = T; g.seq_stride = p.seq_stride; g.pad_shift = p.pad_shift;
    int len = n;
    for (int ip = 0; ip < p.nr; ++ip) {
        const int R = p.radix[ip];
        switch (R) {
            case 2: run_pass<float, 2>(tile, g, len, tid, kWThreads, p.tw); break;
            case 4: run_pass<float, 4>(tile, g, len, tid, kWThreads, p.tw); break;
            case 8: run_pass<float, 8>(tile, g, len, tid, kWThreads, p.tw); break;
            default: run_pass<float, 16>(tile, g, len, tid, kWThreads, p.tw); break;
        }
        len /= R;
        __syncthreads();
    }
}

}  // namespace xrft
