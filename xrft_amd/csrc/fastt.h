// fastt.h -- multitaper spectra (xrfthip_desc.seg_tapers = K >= 1, seg_taper_len = N): the weighted sum over K orthogonal tapers d_j of the power / cross spectrum of ONE
// series of N samples, zero-extended to L points -- S[k] = scale sum_j |sum_n t_j[n] y[n] W_L^kn|^2 with t_j = sqrt(w_j) d_j the table xrfthip_plan_set_tapers carries
// (the kernel knows no weights) and y the series after the detrend over its N samples.  A form of the fastw family: the pairing of fastw.h, where the two members of
// a pair are the SAME samples under two different tapers, and no workspace -- one workgroup owns a whole output.
//
//   fastt_kernel   KP = ceil(K / 2) sequences of L points per series: tapers 2 t and 2 t + 1 the real and the imaginary part of sequence t (an odd K pairs the last
//                  taper with zeros).  With G = 4096 / L sequences in the tile a 256-thread workgroup takes NS = max(1, G / KP) consecutive series, sequence
//                  sl KP + t = (series sl, pair t); where KP > G it takes one series and walks its pairs in ceil(KP / G) rounds, sequence t of round r = pair r G + t
//                  (K <= 32: at most 16 rounds, ONE float32 chain of kMeanChain).  The last workgroup may hold fewer live series: the rest load zeros, write nothing.
//                  The detrend (mean, or least-squares line about (N - 1) / 2, over the N samples; sums in float64) is computed once per series: the samples staged
//                  in the tile (consecutive lanes on consecutive samples), `tps` threads per series and a tree over them -- tps depends on NS, that is on (L, K), never
//                  on P or on how many series are live.  Then per round: sample n < N read again (4-byte loads, the series offset p * pitch in 64 bits; a series is
//                  at most 16 KB and the cache serves it), minus the fit, times the two tapers, n >= N zero; seg_fft; |Z|^2 scale (two fields: Z conj(Z') scale)
//                  added into one float32 register per tile position.  After the last round the registers are staged in the tile and, per series and frequency,
//                  added in float64 over that series' sequences in ascending order, symmetrised ((S_k + S_{L-k}) / 2; CROSS: (D_k + conj D_{L-k}) / 2), x 2 for
//                  0 < k < L / 2 of a real-dim output, x the phase table (CROSS), fftshift or half output -- what fastw_finish_kernel does -- and stored once,
//                  consecutive lanes on consecutive outputs.
// No workspace, no second kernel, no atomics.  An output's bits depend on its own series, the table, L and scale only; a non-finite sample reaches its own series only.
// XRFTHIP_ISHIFT_X is a factor (-1)^k on each transform that cancels in |F|^2 and in F0 conj(F1): ignored.
#pragma once
#include "fastw.h"

namespace xrft {

constexpr const char* kTResources = "fastt_kernel: 109 VGPRs, no scratch, 4 waves per SIMD by registers (two fields: 161 VGPRs, 3 waves); by LDS a full tile (37 .. 41 KB) allows 3 workgroups per CU, 3 waves per SIMD (two fields, 72 .. 76 KB: 2)";  // (scripts/kernel_resources.sh, gfx950)

struct FastT {
    SegTile t;                 // (tw: W_L^k, k < L; pitch: samples between series; L; seq_stride / pad_shift; the radices; detrend; scale.  hop, M, win, the column words: unused)
    const float* in0;
    const float* in1;          // the second field (CROSS), same layout
    const float* tap;          // [K][N] float32: sqrt(w_j) d_j[n]
    void* out;                 // [P][nx_out] float32, or complex64 (CROSS)
    const cf* ph;              // the net true-phase factor per unshifted frequency (CROSS), or null
    long long P;               // series
    int K, KP, N;              // tapers, pairs of tapers, samples per series
    int NS, seqs, rounds;      // series per workgroup, sequences of the tile in use, rounds
    int tps;                   // threads per series of the detrend's sums (a power of two, NS tps <= 256)
    int nx_out, shift, realdim2, ph_on;
};

// one field's detrend coefficients: coef[2 sl] the mean, coef[2 sl + 1] the slope about (N - 1) / 2, of the `live` series from src on.  The samples are staged in the
// tile (series sl at the floats behind its first sequence: KP (or G) sequences of more than L cf each hold N <= L floats) so that the loads are coalesced
__device__ __forceinline__ void fastt_fit(const FastT& a, const float* __restrict__ src, int live, cf* tile, double* red, double* coef, int tid) {
    const SegTile& p = a.t;
    const int N = a.N, per = (a.rounds > 1 ? a.seqs : a.KP) * p.seq_stride;  // cf between the staged series
    const float inv_n = 1.0f / (float)N;
    for (int e = tid; e < live * N; e += kWThreads) {
        const int sl = fdiv(e, inv_n), n = e - sl * N;
        reinterpret_cast<float*>(tile + sl * per)[n] = src[(size_t)sl * (size_t)p.pitch + (size_t)n];
    }
    __syncthreads();
    const int tps = a.tps, sl = tid / tps, lane = tid % tps;
    const double c = 0.5 * (double)(N - 1);
    {
        double s0x = 0.0, s1x = 0.0;
        if (sl < live) {
            const float* st = reinterpret_cast<const float*>(tile + sl * per);
            for (int n = lane; n < N; n += tps) {
                const double x = (double)st[n];
                s0x += x;
                s1x += ((double)n - c) * x;
            }
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
    if (lane == 0 && sl < a.NS) {
        const double Nd = (double)N;
        coef[2 * sl] = red[2 * tid] / Nd;
        coef[2 * sl + 1] = (p.detrend == 2 && N > 1) ? red[2 * tid + 1] / (Nd * (Nd * Nd - 1.0) / 12.0) : 0.0;
    }
    __syncthreads();
}

// one field's sequences of round r: (x[n] - fit) t_2q[n] + i (x[n] - fit) t_2q+1[n], zeros for n >= N, for a pair q >= KP and for a series that is not live
__device__ __forceinline__ void fastt_load(const FastT& a, const float* __restrict__ src, int live, int r, cf* tile, const double* coef, int tid) {
    const SegTile& p = a.t;
    const int L = p.L, lgL = 31 - __builtin_clz((unsigned)L), N = a.N, total = a.seqs << lgL;
    const bool det = p.detrend != 0;
    const double c = 0.5 * (double)(N - 1);
    const float inv_kp = 1.0f / (float)a.KP;
    for (int e = tid; e < total; e += kWThreads) {
        const int t = e >> lgL, n = e & (L - 1);
        int sl, q;
        if (a.rounds > 1) { sl = 0; q = r * a.seqs + t; }
        else { sl = fdiv(t, inv_kp); q = t - sl * a.KP; }
        cf z = mk<float>(0.f, 0.f);
        if (n < N && sl < live && q < a.KP) {
            float v = src[(size_t)sl * (size_t)p.pitch + (size_t)n];
            if (det) v = (float)((double)v - (coef[2 * sl] + coef[2 * sl + 1] * ((double)n - c)));
            const float* __restrict__ t0 = a.tap + (size_t)(2 * q) * (size_t)N;
            z.re = v * t0[n];
            if (2 * q + 1 < a.K) z.im = v * t0[(size_t)N + (size_t)n];
        }
        tile[t * p.seq_stride + phys(n, p.pad_shift)] = z;
    }
    __syncthreads();
}

// LDS: [tile 0][tile 1 (TWO)][red: 2 kWThreads doubles][coef: 2 NS doubles per field]
template <bool TWO>
__global__ void __launch_bounds__(kWThreads) fastt_kernel(FastT a) {
    const SegTile& p = a.t;
    XRFT_DYN_SMEM(smem_raw);
    const int tid = threadIdx.x;
    const int tile_elems = (a.seqs * p.seq_stride + 1) & ~1;  // (16-byte multiples: the doubles behind the tiles stay aligned)
    cf* tile0 = reinterpret_cast<cf*>(smem_raw);
    cf* tile1 = tile0 + (TWO ? tile_elems : 0);
    double* red = reinterpret_cast<double*>(tile0 + (TWO ? 2 : 1) * tile_elems);
    double* coef0 = red + 2 * kWThreads;
    double* coef1 = coef0 + 2 * a.NS;
    const long long p0 = (long long)blockIdx.x * a.NS;  // the workgroup's first series
    const int live = a.P - p0 < (long long)a.NS ? (int)(a.P - p0) : a.NS;
    const float* __restrict__ src0 = a.in0 + (size_t)p0 * (size_t)p.pitch;
    const float* __restrict__ src1 = TWO ? a.in1 + (size_t)p0 * (size_t)p.pitch : src0;
    constexpr int CW = TWO ? 2 : 1;
    const int L = p.L, lgL = 31 - __builtin_clz((unsigned)L), used = a.seqs << lgL;  // tile positions in use
    if (p.detrend != 0) {
        fastt_fit(a, src0, live, tile0, red, coef0, tid);
        if (TWO) fastt_fit(a, src1, live, tile1, red, coef1, tid);
    }
    float acc[kWAcc * CW];
#pragma unroll
    for (int e = 0; e < kWAcc * CW; ++e) acc[e] = 0.f;
    for (int r = 0; r < a.rounds; ++r) {
        fastt_load(a, src0, live, r, tile0, coef0, tid);
        if (TWO) fastt_load(a, src1, live, r, tile1, coef1, tid);
        seg_fft(p, L, a.seqs, tile0, tid);
        if (TWO) seg_fft(p, L, a.seqs, tile1, tid);
#pragma unroll
        for (int q = 0; q < kWAcc; ++q) {
            const int e = tid + q * kWThreads;
            if (e < used) {
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
        __syncthreads();  // (the next round's loads, or the staging below, overwrite the tile)
    }
    // ---- every sum to its own tile position, then per series and frequency the sequences added in order, float64
#pragma unroll
    for (int q = 0; q < kWAcc; ++q) {
        const int e = tid + q * kWThreads;
        if (e < used) tile0[(e >> lgL) * p.seq_stride + phys(e & (L - 1), p.pad_shift)] = mk<float>(acc[CW * q], TWO ? acc[CW * q + (TWO ? 1 : 0)] : 0.f);
    }
    __syncthreads();
    const int nxo = a.nx_out, nseq = a.rounds > 1 ? a.seqs : a.KP;  // sequences of one series
    const float inv_nxo = 1.0f / (float)nxo;
    for (int w = tid; w < live * nxo; w += kWThreads) {
        const int sl = fdiv(w, inv_nxo), c = w - sl * nxo;
        const int k = (c - a.shift) & (L - 1), k2 = (L - k) & (L - 1);
        const int pa = phys((int)p.rev[k], p.pad_shift), pb = phys((int)p.rev[k2], p.pad_shift);
        const cf* sq = tile0 + sl * nseq * p.seq_stride;
        double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
        for (int t = 0; t < nseq; ++t) {
            const cf va = sq[t * p.seq_stride + pa], vb = sq[t * p.seq_stride + pb];
            ar += (double)va.re;
            br += (double)vb.re;
            if (TWO) { ai += (double)va.im; bi += (double)vb.im; }
        }
        const double f = (a.realdim2 && k > 0 && 2 * k < L) ? 1.0 : 0.5;
        const size_t oi = (size_t)p0 * (size_t)nxo + (size_t)w;
        if (TWO) {
            cf v = mk<float>((float)((ar + br) * f), (float)((ai - bi) * f));
            if (a.ph_on) v = cmul(v, a.ph[k]);
            reinterpret_cast<cf*>(a.out)[oi] = v;
        } else {
            reinterpret_cast<float*>(a.out)[oi] = (float)((ar + br) * f);
        }
    }
}

}  // namespace xrft
