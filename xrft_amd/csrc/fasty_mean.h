// fasty_mean.h -- the mean over the batch inside the last pass (xrfthip_desc.mean_batch = M > 1): every M consecutive slabs give ONE power / cross spectrum, their
// mean -- what the reference's users do with a batch of spectra (power_spectrum(...).mean("time"), xrft's Parseval / chunk / MITgcm notebooks) without the M full
// spectra ever reaching memory.
//
//   fasty_rows_mean_kernel   pass 2 of the y-first pipeline (fasty.h) for one run of slabs: a workgroup owns its rows ky of ONE output and walks a contiguous run
//                            of that output's slabs inside the current group; |F|^2 scale (F0 conj(F1) scale) is added into float32 registers for at most
//                            kMeanChain slabs, then the registers are staged in natural order (the staging of fasty_rows_kernel) and added, float64, into the
//                            workgroup's own rows of a partial [output][P][ny/2 + 1][nx] in the workspace.  No atomics: a row of a partial belongs to one
//                            workgroup per launch, and the launches of one exec are ordered by the stream.
//   mean_finish_kernel       sums the P partials of an output in order, x 1/M, and writes every row twice: rotated (fftshift) and Hermitian-mirrored (conjugated,
//                            and x the true-phase factors, for a cross spectrum).  Shared with the one-pass small-slab kernel (fasts.h, MEAN).
// The order of every addition is fixed by the plan (M, P, the groups of slabs): repeated calls return identical bits.  No float32 chain is longer than kMeanChain
// terms; a non-finite slab reaches its own output only.
#pragma once
#include "fasty.h"

namespace xrft {

constexpr int kMeanChain = 16;  // float32 additions in a row before the sum moves to float64

struct YMean {
    double* part;   // [output][P][ny/2 + 1][nx] float64, or complex128 (cross spectra): zeroed by the exec before the first group
    long long g0;   // first slab of the group, counted in the whole batch (FastY::nslab slabs follow)
    int M;          // slabs per output
    int P;          // runs per output and group
};

// acc + v with v kept apart from the multiplication that made it: an fma here would round x + x differently from the stored sample x of the plain plan
__device__ __forceinline__ float mean_add(float acc, float v) {
    XRFT_OPAQUE(v);
    return acc + v;
}

// MODE 1 power, 2 cross (fasty_rows_kernel's).  The loads, the residual-trend terms and the transforms are fasty_rows_kernel's; nothing of its store loops is here.
// MODE 3 coherence (XRFTHIP_OUT_COHERENCE): the geometry, loads and transforms of MODE 2 and 64 sums per thread -- the 32 of the cross spectrum, by the same
// statements, and 16 + 16 of |F0|^2 |scale| and |F1|^2 |scale|, by the statements of MODE 1 -- for the partial [..][nx][re C, im C, A, B] that
// mean_finish_coherence_kernel turns into |C|^2 / (A B).  64 sums beside the two rows do not fit the 168 registers of three waves per SIMD: two waves, 256 registers.
template <int NX, int MODE>
__global__ void __launch_bounds__((YRows<NX>::THR), (MODE == 3 ? 2 : 3)) fasty_rows_mean_kernel(FastY p, YMean m) {
    static_assert(MODE == 1 || MODE == 2 || MODE == 3, "the mean of power and cross spectra, and the sums of a coherence");
    typedef P2<NX> G;
    typedef YRows<NX> R;
    constexpr bool TWO = MODE >= 2, COH = MODE == 3;
    constexpr int NACC = COH ? 64 : 32;
    constexpr int NT = G::NT, GX = R::GX, THR = R::THR, RPU = TWO ? GX : 2 * GX, GSTR = YLds<NX, GX>::GSTR;
    constexpr int RSP = R::RS, RSC = NX + NX / 16;
    XRFT_DYN_SMEM(smem_raw);
    cf* lds = reinterpret_cast<cf*>(smem_raw);
    float* stg = reinterpret_cast<float*>(smem_raw);
    cf* tw2 = lds + GX * GSTR;  // (behind the transforms' LDS and behind the staged rows: filled once)
    fill_tw2<NX>(tw2, p.tw_x, (int)threadIdx.x, THR);
    const int nyh = p.ny >> 1, upr = p.nrow_pad / RPU;
    const int unit = (int)blockIdx.x % upr, rest = (int)blockIdx.x / upr, pp = rest % m.P, ol = rest / m.P;
    const int ky0 = unit * RPU;
    // the slabs of output o inside this group, and run pp of them
    const long long o = m.g0 / m.M + ol;
    const long long lo = max(m.g0, o * (long long)m.M), hi = min(m.g0 + (long long)p.nslab, (o + 1) * (long long)m.M), len = hi - lo;
    const long long s_lo = lo + (long long)pp * len / m.P, s_hi = lo + (long long)(pp + 1) * len / m.P;
    float acc[NACC];
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.f;
    int chain = 0;
    for (long long s = s_lo; s < s_hi; ++s) {
        int tid = threadIdx.x;
        XRFT_OPAQUE(tid);  // (nothing derived from the thread index is hoisted out of the slab loop and spilled)
        const int g = tid % GX, u = tid / GX;
        cf* mine = lds + g * GSTR;
        const int slab = (int)(s - m.g0);  // inside the group: the intermediate and the corrections are the group's
        const int kyA = min(ky0 + g, nyh), kyB = TWO ? kyA : min(ky0 + GX + g, nyh);
        const char* __restrict__ w2s = reinterpret_cast<const char*>(p.w2 + (size_t)slab * p.nrow_pad * NX);
        const char* __restrict__ w2t = TWO ? reinterpret_cast<const char*>(p.w2b + (size_t)slab * p.nrow_pad * NX) : w2s;
        const char* __restrict__ crb = reinterpret_cast<const char*>(p.corr + (size_t)slab * NX * 2);
        const bool addback = p.detrend != 0;
        cf a[16], b[16];
        if (NT >= (1 << p.l_cw)) {  // x = u + NT q advances by whole column blocks: constant stride
            const unsigned offA = w2_offset(p, kyA, u) * 8u, offB = w2_offset(p, kyB, u) * 8u;
            const unsigned qstr = (unsigned)(((NT >> p.l_cw) * 2) << (p.l_rk + p.l_2gy)) * 8u;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                a[q] = *reinterpret_cast<const cf*>(w2s + (offA + qstr * (unsigned)q));
                b[q] = *reinterpret_cast<const cf*>(w2t + (offB + qstr * (unsigned)q));
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                a[q] = *reinterpret_cast<const cf*>(w2s + w2_offset(p, kyA, u + NT * q) * 8u);
                b[q] = *reinterpret_cast<const cf*>(w2t + w2_offset(p, kyB, u + NT * q) * 8u);
            }
        }
        if (addback) {  // add back wx[x] * (subtracted line - plane fit) in the spectral domain (fasty_rows_kernel: the same fmaf per sample)
            // (the residual-trend pairs in two batches of eight: with all sixteen beside the rows and the 32 sums the kernel does not fit three waves per SIMD)
            const cf a0 = p.what0[kyA], a1 = p.what1[kyA], b0 = p.what0[kyB], b1 = p.what1[kyB];
            const char* __restrict__ crc = TWO ? reinterpret_cast<const char*>(p.corr_b + (size_t)slab * NX * 2) : crb;  // (the second field has its own residual trend)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                cf cr[8], cs[TWO ? 8 : 1];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    cr[q] = *reinterpret_cast<const cf*>(crb + (unsigned)(u + NT * (8 * h + q)) * 8u);
                    if (TWO) cs[TWO ? q : 0] = *reinterpret_cast<const cf*>(crc + (unsigned)(u + NT * (8 * h + q)) * 8u);
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int i = 8 * h + q;
                    const float al = cr[q].re, ga = cr[q].im, bl = TWO ? cs[TWO ? q : 0].re : al, bg = TWO ? cs[TWO ? q : 0].im : ga;
                    a[i].re = fmaf(al, a0.re, fmaf(ga, a1.re, a[i].re));
                    a[i].im = fmaf(al, a0.im, fmaf(ga, a1.im, a[i].im));
                    b[i].re = fmaf(bl, b0.re, fmaf(bg, b1.re, b[i].re));
                    b[i].im = fmaf(bl, b0.im, fmaf(bg, b1.im, b[i].im));
                }
            }
        }
        fft_p2_pair<NX>(a, b, u, mine, p.tw_x, tw2);  // (ends with a barrier: the LDS is free)
        if (TWO) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {  // F0 conj(F1) * scale, the expression of fasty_rows_kernel
                const cf v = cscale(cmulc(a[e], b[e]), p.scale);
                acc[2 * e] = mean_add(acc[2 * e], v.re);
                acc[2 * e + 1] = mean_add(acc[2 * e + 1], v.im);
            }
            if (COH) {
                const float sc = fabsf(p.scale);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const cf va = a[e], vb = b[e];
                    acc[(COH ? 32 : 0) + e] = mean_add(acc[(COH ? 32 : 0) + e], (va.re * va.re + va.im * va.im) * sc);
                    acc[(COH ? 48 : 0) + e] = mean_add(acc[(COH ? 48 : 0) + e], (vb.re * vb.re + vb.im * vb.im) * sc);
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const cf va = a[e], vb = b[e];
                acc[e] = mean_add(acc[e], (va.re * va.re + va.im * va.im) * p.scale);
                acc[16 + e] = mean_add(acc[16 + e], (vb.re * vb.re + vb.im * vb.im) * p.scale);
            }
        }
        if (++chain < kMeanChain && s + 1 < s_hi) continue;
        // ---- the chain ends: the registers staged row-major in natural order (17/16 padding), then added to this workgroup's rows of the partial, float64, whole rows
        if (TWO) {
#pragma unroll
            for (int bb = 0; bb < G::NB; ++bb)
#pragma unroll
                for (int k3 = 0; k3 < G::R3; ++k3) {
                    const int e = bb * G::R3 + k3;
                    lds[g * RSC + nat16(held_k<NX>(u, bb, k3))] = mk<float>(acc[2 * e], acc[2 * e + 1]);
                }
        } else {
#pragma unroll
            for (int bb = 0; bb < G::NB; ++bb)
#pragma unroll
                for (int k3 = 0; k3 < G::R3; ++k3) {
                    const int sl = nat16(held_k<NX>(u, bb, k3)), e = bb * G::R3 + k3;
                    stg[g * RSP + sl] = acc[e];
                    stg[(GX + g) * RSP + sl] = acc[16 + e];
                }
        }
        __syncthreads();
        constexpr int CW = TWO ? 2 : 1;  // doubles per sample and staging round
        constexpr int PW = COH ? 4 : CW;  // doubles per sample of the partial
        double* __restrict__ dst = m.part + ((size_t)(o * m.P + pp) * (size_t)(nyh + 1) + (size_t)ky0) * (size_t)NX * PW;
        for (int e = tid; e < RPU * NX * CW; e += THR) {
            const int rl = e / (NX * CW), c = e % (NX * CW);
            if (ky0 + rl > nyh) continue;  // (padding rows of the last unit)
            const float v = TWO ? stg[rl * 2 * RSC + 2 * nat16(c >> 1) + (c & 1)] : stg[rl * RSP + nat16(c)];
            dst[(size_t)rl * NX * PW + (COH ? 4 * (c >> 1) + (c & 1) : c)] += (double)v;
        }
        __syncthreads();  // (the next slab's transforms overwrite the staged rows)
        if (COH) {  // the second round through the same region (two values per sample do not fit beside each other): (A, B) staged as the pair (re C, im C) was
#pragma unroll
            for (int bb = 0; bb < G::NB; ++bb)
#pragma unroll
                for (int k3 = 0; k3 < G::R3; ++k3) {
                    const int e = bb * G::R3 + k3;
                    lds[g * RSC + nat16(held_k<NX>(u, bb, k3))] = mk<float>(acc[(COH ? 32 : 0) + e], acc[(COH ? 48 : 0) + e]);
                }
            __syncthreads();
            for (int e = tid; e < RPU * NX * 2; e += THR) {
                const int rl = e / (NX * 2), c = e % (NX * 2);
                if (ky0 + rl > nyh) continue;
                dst[(size_t)rl * NX * 4 + 4 * (c >> 1) + 2 + (c & 1)] += (double)stg[rl * 2 * RSC + 2 * nat16(c >> 1) + (c & 1)];
            }
            __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < NACC; ++e) acc[e] = 0.f;
        chain = 0;
    }
}

// out[o][row][c] = (1/M) sum_pp part[o][pp][..]: one workgroup per output row.  part rows are ky = 0 .. ny/2 in natural kx order; the output row of frequency ky > ny/2
// is row ny - ky read backwards (F[-ky][-kx] = conj F[ky][kx]).  CPLX: complex128 partials, complex64 output, x the true-phase factors of the DESTINATION sample.
template <bool CPLX>
__global__ void __launch_bounds__(256) mean_finish_kernel(const double* __restrict__ part, void* out, int ny, int nx, int P, double inv_m, int shift_y, int shift_x,
                                                          const cf* __restrict__ ph_y, const cf* __restrict__ ph_x, int ph_on) {
    const long long o = (long long)blockIdx.x / ny;
    const int orow = (int)((long long)blockIdx.x % ny);
    const int fy = (orow - shift_y) & (ny - 1);  // unshifted frequency index of this output row
    const bool mir = fy > ny / 2;
    const int r = mir ? ny - fy : fy, nrow = ny / 2 + 1;
    constexpr int CW = CPLX ? 2 : 1;
    const size_t pstr = (size_t)nrow * nx * CW;
    const double* __restrict__ src = part + ((size_t)o * P * nrow + r) * (size_t)nx * CW;
    for (int c = threadIdx.x; c < nx; c += 256) {
        const int fx = (c - shift_x) & (nx - 1), kx = mir ? (nx - fx) & (nx - 1) : fx;
        double sr = 0.0, si = 0.0;
        for (int q = 0; q < P; ++q) {
            sr += src[q * pstr + (size_t)kx * CW];
            if (CPLX) si += src[q * pstr + (size_t)kx * CW + 1];
        }
        const size_t oi = ((size_t)o * ny + orow) * (size_t)nx + c;
        if (CPLX) {
            cf v = mk<float>((float)(sr * inv_m), (float)(si * inv_m));
            if (mir) v = cconj(v);
            if (ph_on) v = cmul(v, cmul(ph_y[fy], ph_x[fx]));
            reinterpret_cast<cf*>(out)[oi] = v;
        } else {
            reinterpret_cast<float*>(out)[oi] = (float)(sr * inv_m);
        }
    }
}

// The coherence of a mean plan (XRFTHIP_OUT_COHERENCE): part is [output][P][ny/2 + 1][nx][re C, im C, A, B] -- the sums over the M slabs of F0 conj(F1) scale,
// |F0|^2 |scale| and |F1|^2 |scale| -- and out[o][row][c] = |sum C|^2 / (sum A  sum B), the P partials of each of the four added in order, float64.  1 / M and the
// scale cancel; the mirrored row holds the same number (|conj C| = |C|, and the true-phase factors have modulus one): rows rotated and mirrored as a power spectrum's.
// No clamp: a value may exceed 1 by rounding, and a zero denominator gives what IEEE division gives.
static __global__ void __launch_bounds__(256) mean_finish_coherence_kernel(const double* __restrict__ part, float* __restrict__ out, int ny, int nx, int P, int shift_y, int shift_x) {
    const long long o = (long long)blockIdx.x / ny;
    const int orow = (int)((long long)blockIdx.x % ny);
    const int fy = (orow - shift_y) & (ny - 1);
    const bool mir = fy > ny / 2;
    const int r = mir ? ny - fy : fy, nrow = ny / 2 + 1;
    const size_t pstr = (size_t)nrow * nx * 4;
    const double* __restrict__ src = part + ((size_t)o * P * nrow + r) * (size_t)nx * 4;
    for (int c = threadIdx.x; c < nx; c += 256) {
        const int fx = (c - shift_x) & (nx - 1), kx = mir ? (nx - fx) & (nx - 1) : fx;
        double sr = 0.0, si = 0.0, sa = 0.0, sb = 0.0;
        for (int q = 0; q < P; ++q) {
            const double* __restrict__ s4 = src + q * pstr + (size_t)kx * 4;
            sr += s4[0];
            si += s4[1];
            sa += s4[2];
            sb += s4[3];
        }
        out[((size_t)o * ny + orow) * (size_t)nx + c] = (float)((sr * sr + si * si) / (sa * sb));
    }
}

}  // namespace xrft
