// fastk.h -- spectrograms (xrfthip_desc.seg_keep = 1 with seg_hop = H >= 1): the spectrum of EVERY one of the M overlapping L-sample segments of a series, the segments
// read where they lie (fastw.h: segment s of series p starts at p * pitch + s * H) and each spectrum written once -- scipy.signal.spectrogram / stft, the reference's
// power_spectrum(da, dim="time", chunks_to_segments=True, ...) without .mean("time_segment"), with an overlap.  The third form of the fastw family.
//
//   fastk_kernel   one 256-thread workgroup takes one ROUND of one series' segments: NS = 8192 / L of them at most (the tile's 4096 complex points).  Unlike the Welch
//                  kernel no two segments share a transform: segment s is packed WITH ITSELF, z_j = x_{2j} + i x_{2j+1}, an L/2-point sequence of the LDS tile -- a
//                  non-finite sample fills its own segment's spectrum only, and a quiet segment's rounding error does not know its neighbour's magnitude.  The samples are
//                  loaded with 4-byte loads (consecutive lanes read consecutive samples), detrended per segment (mean or least-squares line, sums in float64) and windowed
//                  in the tile, transformed by the in-place radix passes of tile_fft.h (tables of L/2), and unpacked as the generic tiles' r2c form does:
//                  X_k = E_k + W_L^k O_k, E = (Z_k + conj Z_{n-k}) / 2, O = -i (Z_k - conj Z_{n-k}) / 2, n = L / 2, k = 0 .. n; X_{L-k} = conj X_k fills the upper half of
//                  a full output.  Written: |X_k|^2 scale (POWER; x 2 for 0 < k < L/2 of a real-dim output) or X_k scale (COMPLEX) at [series][segment][c], c the
//                  fftshifted place of k or k itself (k <= L/2 only: the half output); consecutive lanes store consecutive elements -- the round's output is one run.
//                  The COLUMN layout (xrfthip_desc.seg_stride = S, fastk_kernel<.., true>): a workgroup takes C adjacent columns of one block (C = min(32, NS)) and NS / C
//                  segments of each; sequence t of the tile is (column t % C, segment t / C); the load runs column fastest (the offset (s H + j) S + e in 64 bits), the
//                  stores too: d_out is [block][segment][c][column], the place the time axis had.  Columns beyond `inner` in the last group and segments beyond M in the
//                  last round load zeros and write nothing.
// No workspace, no partial sums, no second kernel, no atomics: every output element is computed and stored by one thread, once.
#pragma once
#include "fastw.h"

namespace xrft {

constexpr const char* kKResources = "fastk_kernel: 91 VGPRs, no scratch, 5 waves per SIMD";  // (scripts/kernel_resources.sh, gfx950: all four instances)

struct FastK {
    SegTile t;                 // (tw: W_n^k, k < n = L / 2; rev: of the n-point transform)
    const float* in;
    void* out;
    const cf* twr;             // W_L^k, k <= n (the unpacking)
    int NS, rounds;            // segments (sequences) of the tile, rounds per series (group of columns)
    int nx_out, shift, realdim2;  // L or L / 2 + 1; L / 2 or 0; interior bins of the half output doubled (POWER)
};

// LDS: [tile: NS sequences][red: 2 kWThreads doubles][coef: 2 NS doubles]
template <bool POWER, bool COLS>
__global__ void __launch_bounds__(kWThreads) fastk_kernel(FastK a) {
    const SegTile& p = a.t;
    XRFT_DYN_SMEM(smem_raw);
    const int tid = threadIdx.x;
    const int tile_elems = (a.NS * p.seq_stride + 1) & ~1;  // (16-byte multiples: the doubles behind the tile stay aligned)
    cf* tile = reinterpret_cast<cf*>(smem_raw);
    double* red = reinterpret_cast<double*>(tile + tile_elems);
    double* coef = red + 2 * kWThreads;
    const int rd = (int)((long long)blockIdx.x % a.rounds);
    const SegUnit un = seg_unit<COLS>(p, (long long)blockIdx.x / a.rounds);
    const int lgC = COLS ? p.lgC : 0, cmask = (1 << lgC) - 1, spr = a.NS >> lgC;  // segments of one column per round
    const long long s0 = (long long)rd * spr;                                      // the round's first segment
    const long long blk = un.blk, c0 = un.c0;
    const int live = un.live;
    const int nseg = (long long)p.M - s0 < spr ? (int)((long long)p.M - s0) : spr;  // segments of this round that exist
    const int L = p.L, n = L >> 1, ss = p.seq_stride, psh = p.pad_shift;
    // ---- the samples, detrended and windowed: tile sequence sg = (segment sl of the round, column c), sample j at component j & 1 of point j >> 1
    SelfLayout<COLS> lay;
    lay.lgC = lgC; lay.live = live; lay.s0 = s0; lay.s_hi = p.M;
    seg_load<COLS>(p, lay, a.in + (size_t)blk * (size_t)p.pitch + (size_t)c0, a.NS, tile, red, coef, tid);
    seg_fft(p, n, a.NS, tile, tid);  // ---- NS transforms of n = L / 2 points
    // ---- every segment's spectrum, unpacked and stored: element e of the round's output = (segment sl, place c[, column])
    const int nxo = a.nx_out, total_out = (nseg * nxo) << lgC;
    const float inv_nxo = 1.0f / (float)nxo;
    const size_t obase = ((size_t)blk * (size_t)p.M + (size_t)s0) * (size_t)nxo;  // (in places: x inner for the column layout)
    for (int e = tid; e < total_out; e += kWThreads) {
        const int col = COLS ? (e & cmask) : 0, r = e >> lgC;
        const int sl = fdiv(r, inv_nxo), c = r - sl * nxo;
        if (COLS && col >= live) continue;
        const int k = (c - a.shift) & (L - 1);
        const bool up = k > n;             // X_k = conj X_{L-k}
        const int kk = up ? L - k : k;     // 0 .. n
        const int ka = kk == n ? 0 : kk, kb = kk == 0 ? 0 : n - kk;
        const cf* sq = tile + ((sl << lgC) | col) * ss;
        const cf zk = sq[phys((int)p.rev[ka], psh)];
        const cf zc = cconj(sq[phys((int)p.rev[kb], psh)]);
        const cf E = cscale(zk + zc, 0.5f);
        const cf O = cscale(mul_mi(zk - zc), 0.5f);
        cf X = E + cmul(a.twr[kk], O);
        const size_t oi = COLS ? (obase + (size_t)r) * (size_t)p.inner + (size_t)c0 + (size_t)col : obase + (size_t)r;
        if (POWER) {
            const float f = (a.realdim2 && k > 0 && k < n) ? 2.0f * p.scale : p.scale;
            reinterpret_cast<float*>(a.out)[oi] = (X.re * X.re + X.im * X.im) * f;
        } else {
            if (up) X = cconj(X);
            reinterpret_cast<cf*>(a.out)[oi] = cscale(X, p.scale);
        }
    }
}

}  // namespace xrft
