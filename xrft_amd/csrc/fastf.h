// fastf.h -- FIR filtering along a series by overlap-save (xrfthip_desc.seg_filter = 1 with seg_hop = V, L / 2 <= V <= L): scipy.signal.convolve(x, h, mode) for
// K = L - V + 1 real taps -- every L-sample segment transformed, multiplied by the response H = rfft(h, L), transformed back, and the V samples that do not wrap
// around kept.  The fifth form of the fastw family: the load of fastk.h, its unpacking, the packing of fasto.h and seg_fft twice, in one tile.
//
//   fastf_kernel   one 256-thread workgroup takes NS = 8192 / L consecutive segments s0 .. of one series into the LDS tile, each packed WITH ITSELF
//                  (z_j = x_{2j} + i x_{2j+1}, an n = L / 2-point sequence: a non-finite sample stays in the segments that hold it, fastk.h).  Sample j of segment s
//                  is x[s V + a - (K - 1) + j] where that index lies in [0, N), else 0.f: the guard is per sample, the index in 64 bits, nothing outside the series
//                  is read; consecutive lanes read consecutive samples.  Then
//                    seg_fft                        Z_k at the tile's point rev[k]
//                    per pair (k, n - k), k <= n/2  X_k = E_k + W_L^k O_k as fastk.h unpacks it, Y_k = H_k X_k, Z'_k = E'_k + i O'_k as fasto.h packs it (E' = Y_k +
//                                                   conj Y_{n-k}, O' = conj(W_L^k) (Y_k - conj Y_{n-k}): twice the spectrum of y_{2j} + i y_{2j+1}), conj Z' held in
//                                                   registers (at most 9 pairs per thread), barrier, stored at the NATURAL points k and n - k: the pass is also the
//                                                   permutation the second transform needs
//                    seg_fft                        conj of the unnormalised inverse: y_{2j} = Re t, y_{2j+1} = -Im t of point rev[j], times L (in the caller's scale)
//                  Store: out[(s0 + sl) V + i] = scale y_{K-1+i} of segment sl, i < V, below n_out: the workgroup's output is ONE contiguous run of NS V floats,
//                  consecutive lanes store consecutive samples.
//                  The COLUMN layout (xrfthip_desc.seg_filter_cols with seg_stride = S, fastf_kernel<.., true>): a workgroup takes C = min(32, NS) adjacent columns of
//                  one block and spr = NS / C consecutive segments of each (4, 2, 1, 1 at L = 64, 128, 256, 512); sequence t of the tile is (column t % C, segment
//                  t / C) (SelfLayout<true>).  The load runs column fastest, then sample, then segment: sample j of segment s of column c is at
//                  blk * pitch + (s V + a - (K - 1) + j) S + c0 + c, in 64 bits, 0.f where the time index is outside [0, N) or c >= live.  The two transforms and
//                  the pair pass run over the tile's sequences as they do for rows.  The store runs column fastest too: (row r of the run, column c) goes to
//                  out[(blk * n_out + o0 + r) * inner + c0 + c], r < count, c < live -- the array's own order; one thread, one store.
//                  LDS banks (derived from the bank rules): lanes of one time row differ by seq_stride points = 2 seq_stride dwords, seq_stride odd.  The load's
//                  4-byte writes (32 banks per 32-lane group) reach 16 banks with 32 columns: 2-way (C = 16: an even and an odd sample per group, no conflict); the
//                  store's 8-byte reads (64 banks) are conflict-free at C = 32 and at most 2-way at C = 16 (two time rows per group).  Measured
//                  (SQ_LDS_BANK_CONFLICT against the rows kernel, profiles/r30_fir_filter_cols.txt): at L = 128 exactly the load's 2 cycles per wave-instruction
//                  more and nothing else, at L = 512 no more than the rows kernel; the C = 16 store's share was not separated.
// No workspace, no second tile, no second kernel, no atomics: every output sample is written once by one thread, and its bits depend on its own segment's L inputs, on
// H and on scale only -- not on P, M or the workgroups.
#pragma once
#include "fasto.h"

namespace xrft {

constexpr const char* kFResources = "fastf_kernel: 91 VGPRs, no scratch, 5 waves per SIMD by registers (a full tile, 34.8 KB of LDS: 4 workgroups per CU, 4 waves per SIMD)";  // (scripts/kernel_resources.sh, gfx950: both instances)
constexpr const char* kFColsResources = "fastf_kernel<cols>: 91 VGPRs, no scratch, 5 waves per SIMD by registers (a full tile, 34.1 .. 35.0 KB of LDS: 4 workgroups per CU, 4 waves per SIMD)";  // (scripts/kernel_resources.sh, gfx950: both column instances)
constexpr int kFPairs = 9;  // pairs (k, n - k) a thread holds across the barrier: ceil(NS (n / 2 + 1) / 256) for every L in 64 .. 4096 (the column layout: the same NS sequences, L <= 512)

struct FastF {
    SegTile t;                 // (tw: W_n^k, k < n = L / 2; rev: of the n-point transform; pitch: samples between series; hop: V; M: segments per series)
    const float* in;
    float* out;
    const cf* twr;             // W_L^k, k <= n (the unpacking and the packing)
    const cf* resp;            // H_k, k <= n, or null
    int NS, wgs;               // segments (sequences) of a tile, workgroups per series (per group of columns)
    int K;                     // taps: L - V + 1
    long long N, n_out, lead;  // samples per series in and out, the first output sample within the full convolution (a)
};

// LDS: [tile: min(NS, M) sequences; COLS: C min(NS / C, M)].  RESP: a response was set (else ones: a delay).  COLS: the column layout -- the branches on it are
// compile-time, and with COLS = false every index below is the rows layout's own expression (lgC = 0, one column, the sequence is the segment)
template <bool RESP, bool COLS = false>
__global__ void __launch_bounds__(kWThreads) fastf_kernel(FastF a) {
    const SegTile& p = a.t;
    XRFT_DYN_SMEM(smem_raw);
    const int tid = threadIdx.x;
    cf* tile = reinterpret_cast<cf*>(smem_raw);
    const SegUnit un = seg_unit<COLS>(p, (long long)blockIdx.x / a.wgs);       // a series, or C adjacent columns of a block
    const int lgC = COLS ? p.lgC : 0, cmask = (1 << lgC) - 1, spr = a.NS >> lgC;  // segments of one series (column) per tile
    const long long s0 = ((long long)blockIdx.x % a.wgs) * spr;                // the tile's first segment
    const int L = p.L, n = L >> 1, ss = p.seq_stride, psh = p.pad_shift, V = (int)p.hop;
    const int lgL = 31 - __builtin_clz((unsigned)L);
    const int nseg = (long long)p.M - s0 < spr ? (int)((long long)p.M - s0) : spr;  // segments of the tile that exist
    const int nseq = nseg << lgC;                                               // its sequences: (segment sl, column c) at (sl << lgC) | c
    // ---- the samples: segment sl starts at (s0 + sl) V + a - (K - 1) of the series, zeros outside [0, N) (COLS: and in the columns of the group beyond `live`)
    const float* __restrict__ src = a.in + (size_t)un.blk * (size_t)p.pitch + (size_t)un.c0;
    const long long first = s0 * V + a.lead - (a.K - 1);
    const int total_in = nseq << lgL;
    SelfLayout<COLS> lay;
    lay.lgC = lgC; lay.live = un.live; lay.s0 = s0; lay.s_hi = p.M;
    for (int e = tid; e < total_in; e += kWThreads) {
        const int c = COLS ? (e & cmask) : 0, r = e >> lgC;  // (COLS: column fastest, then sample, then segment -- consecutive lanes, consecutive addresses of one time row)
        const int sl = r >> lgL, j = r & (L - 1);
        const long long idx = first + (long long)sl * V + j;
        float v = 0.f;
        if (idx >= 0 && idx < a.N && (!COLS || c < un.live)) v = src[COLS ? (size_t)(idx * p.sstride + c) : (size_t)idx];
        *lay.at(tile, p, lay.tile_seg(sl, c), j) = v;
    }
    __syncthreads();
    seg_fft(p, n, nseq, tile, tid);  // ---- nseq transforms of n points
    // ---- per pair (k, n - k), k = 0 .. n / 2: unpack, multiply, pack, conjugate; held in registers while every thread still reads the points rev[.]
    const int hp = (n >> 1) + 1, total_pairs = nseq * hp;
    const float inv_hp = 1.0f / (float)hp;
    cf za[kFPairs], zb[kFPairs];
#pragma unroll
    for (int i = 0; i < kFPairs; ++i) {
        const int e = tid + i * kWThreads;
        if (e < total_pairs) {
            const int sl = fdiv(e, inv_hp), k = e - sl * hp, kb = n - k;
            const cf* sq = tile + sl * ss;
            const cf zk = sq[phys((int)p.rev[k], psh)], zn = sq[phys((int)p.rev[kb & (n - 1)], psh)];  // (Z_n = Z_0)
            const cf wa = a.twr[k], wb = a.twr[kb];
            // X_k = E + W_L^k O, E = (Z_k + conj Z_{n-k}) / 2, O = -i (Z_k - conj Z_{n-k}) / 2; X_{n-k} from the same two points
            cf xa = cscale(zk + cconj(zn), 0.5f) + cmul(wa, cscale(mul_mi(zk - cconj(zn)), 0.5f));
            cf xb = cscale(zn + cconj(zk), 0.5f) + cmul(wb, cscale(mul_mi(zn - cconj(zk)), 0.5f));
            if (RESP) {
                cf ha = a.resp[k], hb = a.resp[kb];
                if (k == 0) ha.im = hb.im = 0.f;  // (entries 0 and L / 2: real)
                xa = cmul(xa, ha);
                xb = cmul(xb, hb);
            }
            if (k == 0) xa.im = xb.im = 0.f;      // (bins 0 and L / 2 of a real series, as fasto.h takes them)
            // Z'_k = Y_k + conj Y_{n-k} + i conj(W_L^k) (Y_k - conj Y_{n-k}), conjugated for the forward passes
            za[i] = cconj(xa + cconj(xb) + mul_pi(cmulc(xa - cconj(xb), wa)));
            zb[i] = cconj(xb + cconj(xa) + mul_pi(cmulc(xb - cconj(xa), wb)));
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kFPairs; ++i) {
        const int e = tid + i * kWThreads;
        if (e < total_pairs) {
            const int sl = fdiv(e, inv_hp), k = e - sl * hp;
            cf* sq = tile + sl * ss;
            sq[phys(k, psh)] = za[i];
            if (k > 0 && 2 * k < n) sq[phys(n - k, psh)] = zb[i];
        }
    }
    __syncthreads();
    seg_fft(p, n, nseq, tile, tid);  // ---- ... and back
    // ---- the kept samples: row r of the workgroup's run = (segment sl, sample K - 1 + i), i < V; COLS: element e = (row e >> lgC, column e & cmask), column fastest
    const long long o0 = s0 * V;
    const long long left = a.n_out - o0;
    const int count = left < (long long)nseg * V ? (int)left : nseg * V;
    float* __restrict__ dst = COLS ? a.out + ((size_t)un.blk * (size_t)a.n_out + (size_t)o0) * (size_t)p.inner + (size_t)un.c0
                                   : a.out + (size_t)un.blk * (size_t)a.n_out + (size_t)o0;
    const float inv_v = 1.0f / (float)V;
    for (int e = tid; e < (count << lgC); e += kWThreads) {
        const int c = COLS ? (e & cmask) : 0, r = e >> lgC;
        if (COLS && c >= un.live) continue;
        const int sl = fdiv(r, inv_v), j = r - sl * V + a.K - 1;
        const cf t = tile[((sl << lgC) | c) * ss + phys((int)p.rev[j >> 1], psh)];
        dst[COLS ? (size_t)r * (size_t)p.inner + (size_t)c : (size_t)r] = ((j & 1) ? -t.im : t.re) * p.scale;
    }
}

}  // namespace xrft
