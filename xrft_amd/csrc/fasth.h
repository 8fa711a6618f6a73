// fasth.h -- the LAST pass of a power / cross spectrum over THREE axes (t, y, x) of a real field (xrft.power_spectrum(da, dim=["time", "y", "x"]),
// cross_spectrum of two such fields: reference xrft/xrft.py:685-835; numpy's fftn over three axes, xrft.py:439-447): the transform along t of the HALF
// spectrum the two-axis stage wrote (XRFTHIP_HALF_X), |F|^2 or F0 conj(F1), and the FULL shifted result -- the redundant half from the Hermitian twin.
//
// Before it the three-axis spectra were a composition: the two-axis plan wrote the full complex spectrum (8 B / point), a one-axis plan transformed it along t
// (8 + 8) and xrfthip_spectrum_tail read it once more (8 + 4).  Here the two-axis stage writes 4 B / point and this pass reads 4 and writes 4.
//
//   in     H[batch][nt][ny][nxh] complex T, nxh = nx / 2 + 1: unshifted, the windows along y and x applied (CROSS: a second array of the same shape)
//   tile   G consecutive columns c = ky nxh + kx of one batch entry, [nt][G] complex in LDS with the lanes along the columns (fastgy_kernel's complex-input
//          form: row stride ny nxh in memory); a block of columns may straddle rows ky.  CROSS: both fields' columns side by side, [nt][2 G]
//   load   the window along t by SOURCE row (the reference windows, then ifftshifts: xrft.py:425-441); ISHIFT_Y is the row rotation
//   t      fastg_cols_pass with the radices of the parameter block (decimation in frequency, digit-reversed rows)
//   out    V = |F|^2 scale (real T) or F0 conj(F1) scale (complex T) at out[b][s_t(kt)][s_y(ky)][s_x(kx)] of the dense [batch][nt][ny][nx] result, and for
//          every column whose twin is not a column of H (1 <= kx <= nx - nxh) V (conj V) at out[b][s_t(-kt)][s_y(-ky)][s_x(nx - kx)]; s = the fftshift
//          rotation or the identity.  Columns kx = 0 and (an even nx) kx = nx / 2 are their own twins' partners: those columns write themselves.  Every
//          element is written exactly once.  A thread owns 16 bytes of an output row: along kx the direct stores ascend and the twin stores descend, both are
//          runs, so eight lanes write a whole 128-byte piece of a row with one 16-byte non-temporal store each (the result is read much later, by the
//          caller); where a piece crosses a row end, the fftshift seam or the range of the twins, its samples are stored one by one.
// No sums, no atomics: repeated calls return identical bits.
//
// FIELD: the transform those spectra are made of (xrft.fft(da, dim=["time", "y", "x"])): V = F scale [phase_t[kt] phase_y[ky] phase_x[kx]] (complex T), the twin
// conj(F) scale times the phase factors of its DESTINATION indices (-kt, -ky, nx - kx) -- fftfreq gives the index n / 2 of an even n the frequency -1 / (2 dx) for
// itself and for its own twin, so the rows kt = nt / 2 and ky = ny / 2 of the twins do not carry the conjugate factor (the twin columns never include kx = 0 or
// nx / 2: along x phase[nx - kx] = conj(phase[kx]) holds for them).  Without phase tables the twin is the plain conjugate, bit for bit.
#pragma once
#include "fastg.h"

namespace xrft {

struct FastH {
    const void* in;    // H[batch][nt][ny][nxh] complex T
    const void* in_b;  // CROSS: the second field's half spectrum (same layout); the result is F(in) conj F(in_b) (xrft.py:825)
    void* out;         // [batch][nt][ny][nx] real T (POWER) or complex T (CROSS, FIELD)
    long long nunits;  // batch x column blocks
    int nt, ny, nx, nxh, ncol, nblk;  // ncol = ny nxh columns of a batch entry; nblk = ceil(ncol / G)
    int G, lg, lch;    // columns per workgroup (a power of two = 128 bytes of an output row), its log2; log2 of the 16-byte pieces of a block's row
    int nrt, rt[kFastGMaxPasses];
    const void* tw_t;  // W_nt^k (complex T)
    const unsigned* rev_t;
    const void* win_t; // T, or null
    int ishift_in;     // tile row i is source row i + ishift_in (mod nt)
    int shift_t, shift_y, shift_x;  // 0 or n / 2 (xrft.py:446-447)
    double scale;
    const void *ph_t, *ph_y, *ph_x;  // FIELD: the output phase factors by UNSHIFTED index, complex T [nt], [ny], [nx] (the full x axis: the twins lie above nx / 2); all three or none
};

enum { kFastHPower = 0, kFastHCross = 1, kFastHField = 2 };  // the output forms: |F|^2, F0 conj(F1), F

template <typename T, int MODE> struct FastHOut { typedef C2<T> type; };
template <typename T> struct FastHOut<T, kFastHPower> { typedef T type; };

// BYTES (4 | 8 | 16) at dst, aligned like T only: non-temporal.  (A 16-byte store at 4-byte alignment is one global_store_dwordx4: gfx950 takes unaligned vector
// accesses to global memory.)
template <typename T, int BYTES>
__device__ __forceinline__ void fasth_store_nt(void* dst, const void* src) {
#ifdef XRFT_EMULATE
    memcpy(dst, src, BYTES);
#else
    if constexpr (BYTES == 4) {
        unsigned t;
        __builtin_memcpy(&t, src, 4);
        __builtin_nontemporal_store(t, reinterpret_cast<unsigned*>(dst));
    } else {
        typedef unsigned vec_t __attribute__((ext_vector_type(BYTES / 4)));
        typedef vec_t uvec_t __attribute__((aligned(sizeof(T))));
        vec_t t;
        __builtin_memcpy(&t, src, BYTES);
        __builtin_nontemporal_store(t, reinterpret_cast<uvec_t*>(dst));
    }
#endif
}

template <typename T, int MODE>
__device__ __forceinline__ typename FastHOut<T, MODE>::type fasth_value(C2<T> a, C2<T> b, T sc) {
    if constexpr (MODE == kFastHCross) { const C2<T> v = cmulc(a, b); return mk<T>(v.re * sc, v.im * sc); }  // F0 conj(F1)
    else if constexpr (MODE == kFastHField) return mk<T>(a.re * sc, a.im * sc);                           // F
    else return (a.re * a.re + a.im * a.im) * sc;
}
template <typename T> __device__ __forceinline__ T fasth_twin(T v) { return v; }                   // |F|^2 of the twin
template <typename T> __device__ __forceinline__ C2<T> fasth_twin(C2<T> v) { return cconj(v); }  // F0 conj(F1) of the twin: the conjugate, like a spectrum's

template <typename T, int MODE>
__global__ void __launch_bounds__(256, (sizeof(T) == 4 ? 3 : 2)) fasth_kernel(FastH p) {
    typedef C2<T> CT;
    typedef typename FastHOut<T, MODE>::type OT;
    constexpr bool CROSS = MODE == kFastHCross, FIELD = MODE == kFastHField;
    constexpr int NF = CROSS ? 2 : 1, VW = 16 / (int)sizeof(OT);  // fields; samples of a 16-byte piece
    XRFT_DYN_SMEM(smem_raw);
    CT* tile = reinterpret_cast<CT*>(smem_raw);
    const int tid = threadIdx.x, nthr = blockDim.x, nt = p.nt, ny = p.ny, nx = p.nx, nxh = p.nxh, ncol = p.ncol, G = p.G, lg = p.lg;
    const int GS = NF * G;  // complex values of a tile row
    unsigned char* tb = smem_raw + (((size_t)nt * GS * sizeof(CT) + 15) & ~(size_t)15);
    CT* tws = reinterpret_cast<CT*>(tb); tb += (size_t)nt * sizeof(CT);
    T* wts = reinterpret_cast<T*>(tb); tb += (size_t)nt * sizeof(T);
    unsigned short* revt = reinterpret_cast<unsigned short*>(tb);
    for (int k = tid; k < nt; k += nthr) {
        tws[k] = reinterpret_cast<const CT*>(p.tw_t)[k];
        revt[k] = (unsigned short)p.rev_t[k];
        if (p.win_t) wts[k] = reinterpret_cast<const T*>(p.win_t)[k];
    }
    const int g = tid & (G - 1), rq = tid >> lg, RQ = nthr >> lg;  // lane along the columns, row group
    const int CH = 1 << p.lch;                                      // 16-byte pieces of a block's row
    const T sc = (T)p.scale;
    OT* __restrict__ outp = reinterpret_cast<OT*>(p.out);
    for (long long unit = blockIdx.x; unit < p.nunits; unit += gridDim.x) {
        const long long b = unit / p.nblk;
        const int c0 = (int)(unit - b * p.nblk) * G;
        const int ky0 = c0 / nxh, kx0 = c0 - ky0 * nxh;  // (once per unit: the pieces count on from here)
        const bool live = c0 + g < ncol;
        __syncthreads();  // (the previous unit's output loop is done with the tile; the tables are in place)
        // ---- load: rows rq, rq + RQ, ... of column g (both fields'), the window by source row
        {
            const CT* __restrict__ s0 = reinterpret_cast<const CT*>(p.in) + (size_t)b * nt * ncol + c0 + g;
            const CT* __restrict__ s1 = CROSS ? reinterpret_cast<const CT*>(p.in_b) + (size_t)b * nt * ncol + c0 + g : nullptr;
            for (int i = rq; i < nt; i += RQ) {
                int is = i + p.ishift_in; if (is >= nt) is -= nt;
                CT z0 = mk<T>((T)0, (T)0), z1 = z0;
                if (live) { z0 = s0[(size_t)is * ncol]; if (CROSS) z1 = s1[(size_t)is * ncol]; }
                if (p.win_t) { const T w = wts[is]; z0 = mk<T>(z0.re * w, z0.im * w); z1 = mk<T>(z1.re * w, z1.im * w); }
                tile[i * GS + g] = z0;
                if (CROSS) tile[i * GS + G + g] = z1;
            }
        }
        __syncthreads();
        // ---- t: the passes of length nt over the GS columns of the tile
        {
            int L = nt;
            for (int ps = 0; ps < p.nrt; ++ps) {
                fastg_cols_pass<T>(tile, GS, nt, GS, p.rt[ps], L, tid, nthr, tws);
                L /= p.rt[ps];
                __syncthreads();
            }
        }
        // ---- out: (frequency kt, piece) = VW consecutive columns of one tile row
        const int tot = nt << p.lch;
        for (int e = tid; e < tot; e += nthr) {
            const int kt = e >> p.lch, ch = e & (CH - 1);
            const int cb = c0 + ch * VW;  // the piece's first column
            if (cb >= ncol) continue;
            const int nv = ncol - cb < VW ? ncol - cb : VW;  // (the last block of a batch entry may end inside a piece)
            int ky = ky0, kx = kx0 + ch * VW;
            while (kx >= nxh) { kx -= nxh; ++ky; }
            const CT* src = tile + (int)revt[kt] * GS + ch * VW;
            OT v[VW];
#pragma unroll
            for (int j = 0; j < VW; ++j) v[j] = fasth_value<T, MODE>(src[j], src[(CROSS ? G : 0) + j], sc);
            [[maybe_unused]] OT w[VW];  // FIELD: the twins' values
            if constexpr (FIELD) {
                const CT* __restrict__ pht = reinterpret_cast<const CT*>(p.ph_t);
                const CT* __restrict__ phy = reinterpret_cast<const CT*>(p.ph_y);
                const CT* __restrict__ phx = reinterpret_cast<const CT*>(p.ph_x);
                int kyj = ky, kxj = kx;
#pragma unroll
                for (int j = 0; j < VW; ++j) {
                    w[j] = cconj(v[j]);
                    if (pht && j < nv) {  // (the tables: all three or none)
                        if (kxj >= nxh) { kxj -= nxh; ++kyj; }
                        if (kxj >= 1 && kxj <= nx - nxh)  // the twin carries the factors of where IT lies: (-kt, -ky, nx - kx)
                            w[j] = cmul(w[j], cmul(cmul(pht[kt ? nt - kt : 0], phy[kyj ? ny - kyj : 0]), phx[nx - kxj]));
                        v[j] = cmul(v[j], cmul(cmul(pht[kt], phy[kyj]), phx[kxj]));
                        ++kxj;
                    }
                }
            }
            int ot = kt + p.shift_t; if (ot >= nt) ot -= nt;
            int mt = (kt ? nt - kt : 0) + p.shift_t; if (mt >= nt) mt -= nt;  // the twin's row along t
            const size_t rowd = ((size_t)b * nt + ot) * ny, rowm = ((size_t)b * nt + mt) * ny;
            // the sample itself: kx ascending
            bool whole = false;
            if (VW > 1 && nv == VW && kx + VW <= nxh) {
                int ox = kx + p.shift_x; if (ox >= nx) ox -= nx;
                if (ox + VW <= nx) {  // (not across the fftshift seam)
                    int oy = ky + p.shift_y; if (oy >= ny) oy -= ny;
                    fasth_store_nt<T, 16>(outp + (rowd + oy) * nx + ox, v);
                    whole = true;
                }
            }
            if (!whole) {
                int kyj = ky, kxj = kx;
#pragma unroll
                for (int j = 0; j < VW; ++j) {  // (unrolled: v stays in registers)
                    if (j < nv) {
                        if (kxj >= nxh) { kxj -= nxh; ++kyj; }
                        int ox = kxj + p.shift_x; if (ox >= nx) ox -= nx;
                        int oy = kyj + p.shift_y; if (oy >= ny) oy -= ny;
                        fasth_store_nt<T, (int)sizeof(OT)>(outp + (rowd + oy) * nx + ox, &v[j]);
                        ++kxj;
                    }
                }
            }
            // its Hermitian twin, for the columns 1 <= kx <= nx - nxh: kx descending
            whole = false;
            if (VW > 1 && nv == VW && kx >= 1 && kx + VW - 1 <= nx - nxh) {  // (then the piece lies in one row ky, too: nx - nxh < nxh)
                int lo = nx - kx - (VW - 1) + p.shift_x; if (lo >= nx) lo -= nx;
                if (lo + VW <= nx) {
                    int my = (ky ? ny - ky : 0) + p.shift_y; if (my >= ny) my -= ny;
                    OT r[VW];
#pragma unroll
                    for (int j = 0; j < VW; ++j) { if constexpr (FIELD) r[j] = w[VW - 1 - j]; else r[j] = fasth_twin(v[VW - 1 - j]); }
                    fasth_store_nt<T, 16>(outp + (rowm + my) * nx + lo, r);
                    whole = true;
                }
            }
            if (!whole) {
                int kyj = ky, kxj = kx;
#pragma unroll
                for (int j = 0; j < VW; ++j) {
                    if (j < nv) {
                        if (kxj >= nxh) { kxj -= nxh; ++kyj; }
                        if (kxj >= 1 && kxj <= nx - nxh) {
                            int ox = nx - kxj + p.shift_x; if (ox >= nx) ox -= nx;
                            int my = (kyj ? ny - kyj : 0) + p.shift_y; if (my >= ny) my -= ny;
                            OT tw;
                            if constexpr (FIELD) tw = w[j]; else tw = fasth_twin(v[j]);
                            fasth_store_nt<T, (int)sizeof(OT)>(outp + (rowm + my) * nx + ox, &tw);
                        }
                        ++kxj;
                    }
                }
            }
        }
    }
}

}  // namespace xrft
