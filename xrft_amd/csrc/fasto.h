// fasto.h -- synthesis (xrfthip_desc.seg_synth = 1 with seg_hop = H >= 1): a series rebuilt from the half spectra of its M overlapping L-sample segments, the inverse of
// what fastk.h writes -- scipy.signal.istft: every segment inverse-transformed, windowed, overlap-added at s H and divided by the sum of the squared windows.  The
// fourth form of the fastw family, and the GATHER form: every output sample is owned by one thread, which adds the (at most R = ceil(L / H)) segments that cover it.
//
//   fasto_kernel   one 256-thread workgroup takes NS = 8192 / L consecutive segments s0 .. s0 + NS - 1 of one series into the LDS tile, each as an n = L / 2-point
//                  sequence (the packing of fastk.h, backwards).  Consecutive workgroups of a series advance by F = NS - (R - 1) segments -- the last R - 1 segments
//                  of a tile are transformed again by the next -- and workgroup r owns the samples [(r F + R - 1) H, ((r + 1) F + R - 1) H), the first from 0, the
//                  last up to span = (M - 1) H + L: a segment that covers an owned sample n has s >= (n - L + 1) / H >= r F and s <= n / H <= r F + NS - 1, so it is
//                  in the tile (the host declines 2 (R - 1) > NS: at most half the transforms are repeated).
//                  Load: consecutive lanes read consecutive complex elements of the round's ONE contiguous run of half spectra; bin k of a segment to point k of its
//                  sequence, k = 0 .. n (point n lies in the padding behind the sequence's last point), the imaginary parts of bins 0 and n zeroed.  Then per pair
//                  (k, n - k), in place: E_k = X_k + conj X_{n-k}, O_k = conj(W_L^k) (X_k - conj X_{n-k}), Z_k = E_k + i O_k -- twice the spectrum of
//                  z_j = x_{2j} + i x_{2j+1}; n z = L z / 2, so the unnormalised inverse of Z is L x: the factor 1 / 2 is in the caller's 1 / L.  The inverse is
//                  conj -> the forward radix passes of tile_fft.h (seg_fft, the tables of n) -> conj: conj Z_k is stored, and x_{2j} = Re t, x_{2j+1} = -Im t of the
//                  tile's point rev[j].
//                  Output: the thread of sample n adds num = sum_s w[n - s H] x_s[n - s H] scale and den = sum_s w^2[n - s H] over the covering segments in
//                  ascending s, float32, and stores den > 1e-10 ? num / den : num; consecutive lanes store consecutive samples.
// No workspace, no partial sums, no second kernel, no atomics: a sample's bits depend on its own covering segments only, not on P, M or the workgroups.
#pragma once
#include "fastk.h"

namespace xrft {

constexpr const char* kOResources = "fasto_kernel: 91 VGPRs, no scratch, 5 waves per SIMD by registers (a full tile, 34.8 KB of LDS: 4 workgroups per CU, 4 waves per SIMD)";  // (scripts/kernel_resources.sh, gfx950: both instances)

struct FastO {
    SegTile t;                 // (tw: W_n^k, k < n = L / 2; rev: of the n-point transform; win: the synthesis window; pitch: complex elements between series)
    const cf* in;
    float* out;
    const cf* twr;             // W_L^k, k <= n (the packing)
    int NS, F, R, wgs;         // segments of a tile, segments a workgroup advances by, segments that meet in a sample, workgroups per series
    long long span;            // (M - 1) H + L samples per series
};

// LDS: [tile: min(NS, M) sequences].  WIN: a window was set (else ones: den counts the covering segments)
template <bool WIN>
__global__ void __launch_bounds__(kWThreads) fasto_kernel(FastO a) {
    const SegTile& p = a.t;
    XRFT_DYN_SMEM(smem_raw);
    const int tid = threadIdx.x;
    cf* tile = reinterpret_cast<cf*>(smem_raw);
    const long long series = (long long)blockIdx.x / a.wgs;
    const int r = (int)((long long)blockIdx.x % a.wgs);
    const int L = p.L, n = L >> 1, ss = p.seq_stride, psh = p.pad_shift, H = (int)p.hop;
    const int s0 = r * a.F;                                    // the tile's first segment
    const int nseg = p.M - s0 < a.NS ? p.M - s0 : a.NS;        // segments of the tile that exist
    // ---- the half spectra: one contiguous run of nseg (n + 1) complex elements
    const cf* __restrict__ src = a.in + (size_t)series * (size_t)p.pitch + (size_t)s0 * (size_t)(n + 1);
    const int total_in = nseg * (n + 1);
    const float inv_n1 = 1.0f / (float)(n + 1);
    for (int e = tid; e < total_in; e += kWThreads) {
        const int sl = fdiv(e, inv_n1), k = e - sl * (n + 1);
        cf v = src[e];
        if (k == 0 || k == n) v.im = 0.f;
        tile[sl * ss + phys(k, psh)] = v;
    }
    __syncthreads();
    // ---- per pair (k, n - k), k = 0 .. n / 2: the packed spectrum, conjugated for the forward passes; (0, n) and (n / 2, n / 2) write one point
    const int hp = (n >> 1) + 1, total_pairs = nseg * hp;
    const float inv_hp = 1.0f / (float)hp;
    for (int e = tid; e < total_pairs; e += kWThreads) {
        const int sl = fdiv(e, inv_hp), k = e - sl * hp;
        cf* sq = tile + sl * ss;
        const int ia = phys(k, psh), ib = phys(n - k, psh);
        const cf xa = sq[ia], xb = sq[ib];
        const cf da = xa - cconj(xb), db = xb - cconj(xa);
        const cf oa = cmulc(da, a.twr[k]), ob = cmulc(db, a.twr[n - k]);           // conj(W_L^k) (X_k - conj X_{n-k})
        sq[ia] = cconj(xa + cconj(xb) + mul_pi(oa));
        if (k > 0 && 2 * k < n) sq[ib] = cconj(xb + cconj(xa) + mul_pi(ob));
    }
    __syncthreads();
    seg_fft(p, n, nseg, tile, tid);  // ---- nseg transforms of n points
    // ---- the owned samples: m = n - s0 H, the place in the tile's own span; the covering segments sl_lo .. sl_hi of the tile, sample j = m - sl H of each
    const long long lo = r == 0 ? 0 : ((long long)s0 + a.R - 1) * H;
    const long long hi = r == a.wgs - 1 ? a.span : ((long long)s0 + a.F + a.R - 1) * H;
    const int m0 = (int)(lo - (long long)s0 * H), count = (int)(hi - lo);
    float* __restrict__ dst = a.out + (size_t)series * (size_t)a.span + (size_t)lo;
    const float inv_h = 1.0f / (float)H;
    for (int e = tid; e < count; e += kWThreads) {
        const int m = m0 + e;
        int sl = m < L ? 0 : fdiv(m - L, inv_h) + 1;
        int sl_hi = fdiv(m, inv_h);
        if (sl_hi > nseg - 1) sl_hi = nseg - 1;
        float num = 0.f, den = 0.f;
        for (int j = m - sl * H; sl <= sl_hi; ++sl, j -= H) {
            const cf t = tile[sl * ss + phys((int)p.rev[j >> 1], psh)];
            const float w = WIN ? p.win[j] : 1.0f;
            num += w * ((j & 1) ? -t.im : t.re) * p.scale;
            den += w * w;
        }
        dst[e] = den > 1e-10f ? num / den : num;
    }
}

}  // namespace xrft
