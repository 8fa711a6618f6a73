#include "plan.h"

// one pass over small float32 slabs (fasts.h): resident workgroups walk the slabs
struct SGeomRt { int thr; size_t lds; int per_cu; size_t lds_iso; };
template <int RY, int RX> static SGeomRt sgeom_t() {
    typedef SGeom<RY, RX> G;
    const int by_lds = (int)((160 * 1024) / G::LDS);
    return {G::T, G::LDS, std::max(1, std::min(by_lds, (int)G::PER_CU)), G::LDS_ISO};
}
static SGeomRt sgeom(long long ny, long long nx) {
#define SG_(A, B) if (ny == 32 * A && nx == 32 * B) return sgeom_t<A, B>();
    SG_(2, 2) SG_(2, 4) SG_(2, 8) SG_(4, 2) SG_(4, 4) SG_(4, 8) SG_(8, 2) SG_(8, 4) SG_(8, 8)
#undef SG_
    return {0, 0, 0, 0};
}
// fasts: is the bin map a radial one (see fasts_power_kernel, ISO)?  If so: first[ky][b] = the smallest |kx| <= nx/2 of row ky whose bin is
// >= b (nx/2 + 1 if none), ky <= ny/2, b = 0 .. nbins.  Otherwise the plan leaves the one-pass path: FastY's tables (and FastY's reaction to the map) or the generic passes.
static int fasts_build_tfirst(xrfthip_plan* P, const int32_t* bm) {
    const int ny = (int)P->d.ny, nx = (int)P->d.nx, nyh = ny / 2, H = nx / 2;
    bool radial = P->nbins <= sgeom(ny, nx).thr && P->nbins >= 1;
    for (int ky = 0; ky <= nyh && radial; ++ky) {
        const int32_t* r = bm + (size_t)ky * nx;
        const bool twin = ky != 0 && 2 * ky != ny;
        const int32_t* t = bm + (size_t)(twin ? ny - ky : ky) * nx;
        for (int m = 0; m <= H; ++m) {
            const int32_t c = r[m];
            if (c < 0 || c >= P->nbins || (m > 0 && c < r[m - 1]) || (m >= 1 && m < H && r[nx - m] != c)) { radial = false; break; }
            if (twin && (t[m] != c || t[(nx - m) % nx] != c)) { radial = false; break; }
        }
    }
    if (!radial) {
        settle_family(P, true);
        return P->chosen == Family::FastY ? family_ops(Family::FastY).binmap(P, bm) : XRFTHIP_OK;
    }
    std::vector<uint16_t> f((size_t)(nyh + 1) * (P->nbins + 1), (uint16_t)(H + 1));
    for (int ky = 0; ky <= nyh; ++ky) {
        const int32_t* r = bm + (size_t)ky * nx;
        uint16_t* dst = f.data() + (size_t)ky * (P->nbins + 1);
        int m = 0;
        for (int b = 0; b <= P->nbins; ++b) {
            while (m <= H && r[m] < b) ++m;
            dst[b] = (uint16_t)m;
        }
    }
    return P->s_tfirst.upload(f.data(), f.size() * sizeof(uint16_t));
}

// FastS: a small float32 slab (64 | 128 | 256 points per axis) fits the registers of one workgroup: full power spectra in ONE pass.  A 256 x 256
// plan also builds FastY's tables: an isotropic plan whose bin map turns out not to be a radial one falls back to them (fasts_build_tfirst)
int try_fasts(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    auto small_len = [](long long n) { return n == 64 || n == 128 || n == 256; };
    const uint32_t oks = XRFTHIP_SHIFT_Y | XRFTHIP_SHIFT_X | (d.out_mode == XRFTHIP_OUT_POWER ? (XRFTHIP_ISO | XRFTHIP_NO_SPECTRUM_OUT) : (XRFTHIP_ISHIFT_Y | XRFTHIP_ISHIFT_X));
    if (!(d.ndim == 2 && d.dtype == XRFTHIP_F32 && small_len(d.ny) && small_len(d.nx) && (d.out_mode == XRFTHIP_OUT_POWER || d.out_mode == XRFTHIP_OUT_COMPLEX) &&
          !(d.flags & ~oks) && env_ll("XRFTHIP_FASTS", 1) != 0)) return kDeclined;
    // a mean plan (xrfthip_desc.mean_batch, fasts_mean.h): power spectra of 64 | 128 points per axis, dense float32 input.  A 1024-thread workgroup has 128 registers per
    // thread, all in use: 256 x 256 goes to FastY's mean form, and so does nothing else of this family
    if (mean_plan(P) && (d.ny == 256 || d.nx == 256 || d.out_mode != XRFTHIP_OUT_POWER || in_strided(P) || in_half(P))) return kDeclined;
    // ... and by default only the classes that measured faster than the composition they replace (profiles/r15_batch_mean.txt): 128 rows -- (16384, 128, 128) 5.3 against
    // 7.1 ms, (32768, 128, 64) 9.5 against 14.1.  With 64 rows -- (65536, 64, 64) 36.2 against 27.5, (32768, 64, 128) 18.6 against 14.1 -- the mean form lost, measured at
    // the 16 workgroups per output that mean_layout's cap of ny / 4 runs leaves a one-output launch: a verdict on that launch shape (XRFTHIP_MEAN_RUNS), not on the
    // kernel.  XRFTHIP_MEAN_ALL=1: every class the mean kernel takes
    if (mean_plan(P) && d.ny != 128 && env_ll("XRFTHIP_MEAN_ALL", 0) == 0) return kDeclined;
    P->family = P->chosen = Family::FastS;
    P->tune_sgrid = env_ll("XRFTHIP_FASTS_GRID", -1);
    P->tune_sstagger = env_ll("XRFTHIP_FASTS_STAGGER", (3 << 8) | 2);  // (three classes 6.8 us apart: (4096, 256, 256) linear + Hann 310 -> 320 (the walk) -> 328 GFFT/s, profiles/r06_fasts_prefetch.txt)
    int rc = plan_twiddle(P, P->tw_sy, d.ny, d.ny);
    if (!rc) rc = plan_twiddle(P, P->tw_sx, d.nx, d.nx);
    if (!rc) rc = plan_ones(P, 256);
    if (!rc && fasty_fits(P)) rc = fasty_tables(P);
    return rc;
}

// FastS's workspace: none, but a mean plan's partial sums (one workgroup per run of an output: the whole batch is one launch)
static void layout_fasts(xrfthip_plan* P) {
    layout_one_pass(P);
    if (mean_plan(P)) P->ws_bytes = mean_layout(P, 0, 1, P->d.batch);
}

static int run_fasts(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d = P->d;
    hipStream_t st = a.stream;
    FastS p{};
    p.in = (const float*)a.in0; p.out = (float*)a.out;
    p.tw_y = (const cf*)P->tw_sy.p; p.tw_x = (const cf*)P->tw_sx.p;
    const bool win = P->win[0].p || P->win[1].p;
    p.win_y = win ? (const float*)(P->win[0].p ? P->win[0].p : P->ones4096.p) : nullptr;
    p.win_x = win ? (const float*)(P->win[1].p ? P->win[1].p : P->ones4096.p) : nullptr;
    p.nslabs = d.batch;
    p.in_slab = in_slab(P); p.in_pitch = (int)in_pitch(P);
    p.in_bf16 = P->in16 == 2 ? 1 : 0;
    p.detrend = d.detrend;
    p.shift_y = (d.flags & XRFTHIP_SHIFT_Y) ? (int)(d.ny / 2) : 0;
    p.shift_x = (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0;
    p.scale = (float)d.scale;
    const SGeomRt G = sgeom(d.ny, d.nx);
    if (mean_plan(P)) {  // fasts_power_kernel<.., MEAN>: workgroup o P + q walks run q of output o; then the finishing pass writes d_out
        p.mean_part = reinterpret_cast<double*>(a.ws + P->off_mean); p.mean_m = (int)d.mean_batch; p.mean_p = P->mean_P;
        const long long nwg = d.batch / d.mean_batch * P->mean_P;
        if (nwg > 0x7fffffffLL) return XRFTHIP_BAD_ARG;
        const dim3 mgrid((unsigned)nwg), mblk((unsigned)G.thr);
        xrfthip_plan::ProfRec* mrec = prof_begin(P, "fasts_slab_mean", st);
#define SM_(A, B) if (d.ny == 32 * A && d.nx == 32 * B) { auto k = &fasts_power_kernel<A, B, 0, 1, false, false, true>; XRFT_LAUNCH(k, mgrid, mblk, G.lds, st, p); }
        SM_(2, 2) SM_(2, 4) SM_(4, 2) SM_(4, 4)
#undef SM_
        prof_end(mrec, st);
        HIP_TRY(hipGetLastError());
        return run_mean_finish(P, p.mean_part, a.out, st);
    }
    // one workgroup per slab by default: measured against the resident set (kCUs x per_cu workgroups walking the slabs), (16384, 128, 128)
    // linear + Hann 531 vs 425 GFFT/s, (65536, 64, 64) 577 vs 497, 256 x 256 even (profiles/r04_fasts.txt)
    // ... except a 256 x 256 power spectrum (ONE 1024-thread workgroup per CU): a resident set that asks for its next slab while the staged rows of the
    // current one leave (fasts_power_kernel PRE), when every workgroup has several slabs to walk (profiles/r06_fasts_prefetch.txt)
    const bool walk = G.thr >= 1024 && d.out_mode == XRFTHIP_OUT_POWER && d.batch >= 4LL * kCUs * G.per_cu;
    const long long res = P->tune_sgrid < 0 ? (walk ? (long long)kCUs * G.per_cu : 0) : P->tune_sgrid;
    const long long g = res > 0 ? std::min<long long>(res, d.batch) : d.batch;
    p.stagger = (res > 0 && d.batch >= 2 * g) ? (int)P->tune_sstagger : 0;
    const dim3 grid((unsigned)std::min<long long>(g, 0x7fffffffLL)), blk((unsigned)G.thr);
    xrfthip_plan::ProfRec* rec = prof_begin(P, "fasts_slab", st);
    const int isom = (d.flags & XRFTHIP_ISO) ? ((d.flags & XRFTHIP_NO_SPECTRUM_OUT) ? 2 : 1) : 0;
    p.iso = a.iso; p.tfirst = (const unsigned short*)P->s_tfirst.p; p.nbins = P->nbins;
    const bool cplx = d.out_mode == XRFTHIP_OUT_COMPLEX;
    p.ph_y = (const cf*)P->fph[0].p; p.ph_x = (const cf*)P->fph[1].p; p.ph_on = (cplx && P->fph_on) ? 1 : 0;
#define SLS_(A, B, SS, HI) do { \
        if (cplx) { auto k = &fasts_power_kernel<A, B, 0, 0, SS, HI>; XRFT_LAUNCH(k, grid, blk, G.lds, st, p); } \
        else if (isom == 0) { auto k = &fasts_power_kernel<A, B, 0, 1, SS, HI>; XRFT_LAUNCH(k, grid, blk, G.lds, st, p); } \
        else if (isom == 1) { auto k = &fasts_power_kernel<A, B, 1, 1, SS, HI>; XRFT_LAUNCH(k, grid, blk, G.lds_iso, st, p); } \
        else { auto k = &fasts_power_kernel<A, B, 2, 1, SS, HI>; XRFT_LAUNCH(k, grid, blk, G.lds_iso, st, p); } } while (0)
    /* (strided: a box of a larger field, read where it lies; half: float16 / bfloat16 input, dense, half_in.h) */
#define SL_(A, B) if (d.ny == 32 * A && d.nx == 32 * B) { if (in_half(P)) SLS_(A, B, false, true); else if (in_strided(P)) SLS_(A, B, true, false); else SLS_(A, B, false, false); }
    SL_(2, 2) SL_(2, 4) SL_(2, 8) SL_(4, 2) SL_(4, 4) SL_(4, 8) SL_(8, 2) SL_(8, 4) SL_(8, 8)
#undef SL_
#undef SLS_
    prof_end(rec, st);
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

// FastR: one real float32 row of 4096 .. 65536 samples per workgroup, transformed in registers in ONE pass (fastr.h): 12 bytes per sample
// through memory where the four-step form (FastY1D) moves 28.  FastRRows: complex rows of 256 .. 4096 points, two rows per thread through one
// LDS buffer (the row pass of fasty_c2c.h on the input's own rows; XRFTHIP_CROWS=0: FastRComplex / FastMX); FastRComplex: complex rows of
// 2048 .. 16384 points (xrft.ifft / fft of complex data along the contiguous axis), the same transform without the packing and the split
int try_fastr(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    if (d.ndim != 1 || (d.out_mode != XRFTHIP_OUT_COMPLEX && d.out_mode != XRFTHIP_OUT_POWER)) return kDeclined;
    const bool cplx_out = d.out_mode == XRFTHIP_OUT_COMPLEX;
    const uint32_t okr = XRFTHIP_SHIFT_X | XRFTHIP_HALF_X | (!cplx_out ? XRFTHIP_REALDIM_X2 : 0u) | (cplx_out ? XRFTHIP_ISHIFT_X : 0u);
    const uint32_t okc = XRFTHIP_SHIFT_X | (cplx_out ? (XRFTHIP_ISHIFT_X | XRFTHIP_INVERSE | XRFTHIP_PHASE_IN) : 0u);
    const bool c2r = (d.flags & XRFTHIP_C2R_X) != 0;  // (irfft along the contiguous axis: rows of nx/2 + 1 complex values in, nx real samples out)
    int rc;
    if (d.dtype == XRFTHIP_C64 && !d.detrend) {
        if ((c2r ? (d.nx % 2 == 0 && fasty_len(d.nx / 2) && cplx_out) : fasty_len(d.nx)) && !(d.flags & ~(okc | (cplx_out ? XRFTHIP_C2R_X : 0u))) &&
            env_ll("XRFTHIP_CROWS", 1) != 0) {
            P->family = P->chosen = Family::FastRRows;
            rc = plan_twiddle(P, P->tw_fx, c2r ? d.nx / 2 : d.nx, c2r ? d.nx / 2 : d.nx);
            if (!rc && c2r) rc = plan_twiddle(P, P->tw_big1d, d.nx, d.nx / 32);
            if (!rc) rc = plan_ones(P, 4096);
        } else if ((d.nx == 16384 || d.nx == 8192 || d.nx == 4096 || d.nx == 2048) && !(d.flags & ~okc) && env_ll("XRFTHIP_FASTC", 1) != 0) {
            P->family = P->chosen = Family::FastRComplex;
            P->tune_rgrid = env_ll("XRFTHIP_FASTR_GRID", 0);
            P->tune_rstagger = env_ll("XRFTHIP_FASTR_STAGGER", 0);
            const long long thr = d.nx / 32;  // threads per row: 32 complex values each
            rc = plan_twiddle(P, P->tw_rm, d.nx, thr);
            if (!rc) rc = plan_twiddle(P, P->tw_rs, thr, 32);
        } else {
            return kDeclined;
        }
    } else if ((d.nx == 65536 || d.nx == 32768 || d.nx == 16384 || d.nx == 8192 || d.nx == 4096) && d.dtype == XRFTHIP_F32 && !(d.flags & ~okr) &&
               !((d.flags & XRFTHIP_HALF_X) && (d.flags & XRFTHIP_SHIFT_X)) && env_ll("XRFTHIP_FASTR", 1) != 0) {
        P->family = P->chosen = Family::FastR;
        // 65536 samples: one resident workgroup per CU walks the rows (measured: 359 vs 344 GFFT/s for a workgroup per row, profiles/r04_fastr.txt);
        // the shorter rows (several workgroups per CU): a workgroup per row
        // 32768 / 16384 samples (one / two workgroups per CU): a resident set, too -- with the start stagger run_fastr picks (profiles/r06_rows_stagger.txt)
        P->tune_rgrid = env_ll("XRFTHIP_FASTR_GRID", d.nx == 65536 ? kCUs : (d.nx == 32768 && d.batch >= 2 * kCUs) ? kCUs : (d.nx == 16384 && cplx_out && d.batch >= 4 * kCUs) ? 2 * kCUs : 0);
        // two classes of workgroups 10 us apart: dft (1024, 65536) 388 -> 441 GFFT/s, power_spectrum 517 -> 586 (profiles/r06_c2_stagger.txt); -1: run_fastr's rule
        P->tune_rstagger = env_ll("XRFTHIP_FASTR_STAGGER", d.nx == 65536 ? ((2 << 8) | 3) : -1);
        const long long thr = d.nx / 64;  // threads per row: 32 packed complex values each
        rc = plan_twiddle(P, P->tw_rm, d.nx / 2, thr);
        if (!rc) rc = plan_twiddle(P, P->tw_rs, thr, 32);
        if (!rc) rc = plan_twiddle(P, P->tw_rn, d.nx, thr);
    } else {
        return kDeclined;
    }
    return rc;
}

// one pass over 65536-sample float32 rows (fastr.h): a 1024-thread workgroup per row, or a resident set walking the rows
static int run_fastr(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d = P->d;
    const void* in = a.in0; void* out = a.out; hipStream_t st = a.stream;
    const bool cin = P->family == Family::FastRComplex;
    if (P->family == Family::FastRRows) {  // complex rows of 256 .. 4096 points: the row pass of the complex two-pass pipeline on the input's own rows
        const bool c2r = (d.flags & XRFTHIP_C2R_X) != 0;
        const long long nxt = c2r ? d.nx / 2 : d.nx;
        const YGeomRt R = yrows_geom(nxt);
        FastYC p{};
        p.c2r = c2r ? 1 : 0; p.in_pitch = (int)(c2r ? nxt + 1 : d.nx); p.w2_nxb = 1;
        p.tw_big = reinterpret_cast<const cf*>(P->tw_big1d.p);
        p.w2 = reinterpret_cast<cf*>(const_cast<void*>(in));
        p.out = out;
        p.tw_x = reinterpret_cast<const cf*>(P->tw_fx.p);
        p.win_y = p.win_x = reinterpret_cast<const float*>(P->win[1].p ? P->win[1].p : P->ones4096.p);
        p.win_on = P->win[1].p ? 1 : 0;
        p.ph_y = p.ph_x = reinterpret_cast<const cf*>(P->fph[1].p);
        const bool phase = d.out_mode == XRFTHIP_OUT_COMPLEX && P->fph_on;
        p.ph_in = (phase && (d.flags & XRFTHIP_PHASE_IN)) ? 1 : 0;
        p.ph_on = (phase && !(d.flags & XRFTHIP_PHASE_IN)) ? 1 : 0;
        p.inv = (d.flags & XRFTHIP_INVERSE) ? 1 : 0;
        p.ishift_x = ((d.flags & XRFTHIP_INVERSE) && (d.flags & XRFTHIP_ISHIFT_X)) ? 1 : 0;
        p.shift_x = (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0;
        p.ny = R.rk; p.nx = (int)d.nx; p.nslab = 1;  // (ny: one unit of rows -- the kernel addresses by row number)
        p.l_cw = ilog2i((int)nxt); p.l_rk = 0;
        p.power = d.out_mode == XRFTHIP_OUT_POWER ? 1 : 0;
        p.scale = (float)d.scale;
        p.nrows = d.batch;
        xrfthip_plan::ProfRec* rec = prof_begin(P, "fastyc_rows", st);
        const dim3 gridr((unsigned)((d.batch + R.rk - 1) / R.rk)), blkr((unsigned)R.thr);
#define YCR_(NN) do { auto k = &fastyc_rows_kernel<NN>; XRFT_LAUNCH(k, gridr, blkr, R.lds, st, p); } while (0)
#define YC2_(NN) do { auto k = &fastyc_rows_c2r_kernel<NN, true>; XRFT_LAUNCH(k, gridr, blkr, R.lds, st, p); } while (0)
        if (c2r) { if (nxt == 2048) YC2_(2048); else if (nxt == 1024) YC2_(1024); else if (nxt == 512) YC2_(512); else YC2_(256); }
        else if (d.nx == 4096) YCR_(4096); else if (d.nx == 2048) YCR_(2048); else if (d.nx == 1024) YCR_(1024); else if (d.nx == 512) YCR_(512); else YCR_(256);
#undef YCR_
#undef YC2_
        prof_end(rec, st);
        HIP_TRY(hipGetLastError());
        return XRFTHIP_OK;
    }
    FastR p{};
    p.in = (const float*)in; p.out = out;
    p.tw_m = (const cf*)P->tw_rm.p; p.tw_s = (const cf*)P->tw_rs.p; p.tw_n = (const cf*)P->tw_rn.p;
    p.win = (const float*)P->win[1].p;
    p.ph = (const cf*)P->fph[1].p; p.ph_on = (d.out_mode == XRFTHIP_OUT_COMPLEX && P->fph_on) ? 1 : 0;
    p.nrows = d.batch;
    p.in_row = in_slab(P);  // (ndim = 1: a slab is a row)
    p.in_bf16 = P->in16 == 2 ? 1 : 0;
    p.detrend = d.detrend;
    p.half = (d.flags & XRFTHIP_HALF_X) ? 1 : 0;
    p.realdim2 = (d.flags & XRFTHIP_REALDIM_X2) ? 1 : 0;
    p.shift = (d.flags & XRFTHIP_SHIFT_X) ? 1 : 0;
    p.scale = (float)d.scale;
    p.stagger = (int)P->tune_rstagger;
    if (cin) {  // (the flags as fastm_xonly_kernel reads them: the input rotated and conjugated for an inverse, the phase table on the input or on the output)
        p.inv = (d.flags & XRFTHIP_INVERSE) ? 1 : 0;
        p.ishift = ((d.flags & XRFTHIP_INVERSE) && (d.flags & XRFTHIP_ISHIFT_X)) ? 1 : 0;
        p.ph_in = ((d.flags & XRFTHIP_PHASE_IN) && P->fph_on) ? 1 : 0;
        p.ph_on = (d.out_mode == XRFTHIP_OUT_COMPLEX && P->fph_on && !(d.flags & XRFTHIP_PHASE_IN)) ? 1 : 0;
    }
    const long long g = P->tune_rgrid > 0 ? std::min<long long>(P->tune_rgrid, d.batch) : d.batch;
    if (P->tune_rstagger < 0) {
        // rows of 32768 / 16384 samples on a resident set: three classes of workgroups 3.4 us apart for a complex result (6.8 us when the true-phase table rides
        // along: fft (2048, 32768) 275 -> 346 GFFT/s, dft 415 -> 435, fft (4096, 16384) 333 -> 356); a power spectrum gains nothing from a stagger
        const bool cplx = d.out_mode == XRFTHIP_OUT_COMPLEX && !cin;
        p.stagger = d.batch < 2 * g ? 0 : (cplx && d.nx == 32768) ? ((3 << 8) | (p.ph_on ? 2 : 1)) : (cplx && d.nx == 16384) ? ((3 << 8) | 1) : 0;
    }
    const dim3 grid((unsigned)std::min<long long>(g, 0x7fffffffLL)), blk((unsigned)(cin ? d.nx / 32 : d.nx / 64));
    const bool pw = d.out_mode == XRFTHIP_OUT_POWER;
    // profiling (bench.py's roofline.kernel): the start / stop timestamps ride on the kernel's own dispatch packet (hipExtLaunchKernelGGL)
    // instead of two event records around it -- barrier packets either side of a 0.18-ms kernel cost the C2 bench line 50 us per step
    hipEvent_t ea = nullptr, eb = nullptr;
#ifndef XRFT_EMULATE
    if (P->prof && P->prof_recs.size() + 1 < P->prof_recs.capacity() && hipEventCreate(&ea) == hipSuccess) {
        if (hipEventCreate(&eb) != hipSuccess) { (void)hipEventDestroy(ea); ea = nullptr; }
    }
#define RK_(KK, LL) do { auto k = &KK; if (ea) hipExtLaunchKernelGGL(k, grid, blk, LL, st, ea, eb, 0, p); else XRFT_LAUNCH(k, grid, blk, LL, st, p); } while (0)
#else
#define RK_(KK, LL) do { auto k = &KK; XRFT_LAUNCH(k, grid, blk, LL, st, p); } while (0)
#endif
#define RLS_(MM, HH, SS, HI) do { \
        if (d.nx == 65536) RK_((fastr_kernel<MM, HH, SS, HI>), kFastRLds); \
        else if (d.nx == 32768) RK_((fastr2_kernel<32, 16, MM, HH, SS, HI>), (R2Geom<32, 16>::LDS)); \
        else if (d.nx == 16384) RK_((fastr2_kernel<16, 16, MM, HH, SS, HI>), (R2Geom<16, 16>::LDS)); \
        else if (d.nx == 8192) RK_((fastr2_kernel<16, 8, MM, HH, SS, HI>), (R2Geom<16, 8>::LDS)); \
        else RK_((fastr2_kernel<8, 8, MM, HH, SS, HI>), (R2Geom<8, 8>::LDS)); } while (0)
    /* (strided: rows of a larger array, read where they lie; half: float16 / bfloat16 rows, dense, half_in.h) */
#define RL_(MM, HH) do { if (in_half(P)) RLS_(MM, HH, false, true); else if (in_strided(P)) RLS_(MM, HH, true, false); else RLS_(MM, HH, false, false); } while (0)
#define RC_(MM) do { \
        if (d.nx == 16384) RK_((fastc_kernel<32, 16, MM>), (R2Geom<32, 16>::LDS)); \
        else if (d.nx == 8192) RK_((fastc_kernel<16, 16, MM>), (R2Geom<16, 16>::LDS)); \
        else if (d.nx == 4096) RK_((fastc_kernel<16, 8, MM>), (R2Geom<16, 8>::LDS)); \
        else RK_((fastc_kernel<8, 8, MM>), (R2Geom<8, 8>::LDS)); } while (0)
    if (cin) { if (pw) RC_(1); else RC_(0); }
    else if (pw) { if (p.half) RL_(1, true); else RL_(1, false); } else { if (p.half) RL_(0, true); else RL_(0, false); }
#undef RC_
#undef RL_
#undef RLS_
#undef RK_
    if (ea) {
        xrfthip_plan::ProfRec r;
        r.label = "fastr_row"; r.a = ea; r.b = eb;
        const_cast<xrfthip_plan*>(P)->prof_recs.push_back(r);
    }
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the rows of FastS, FastR, FastRComplex and FastRRows (plan.h, FamilyOps)
// ---------------------------------------------------------------------------------------------------------------
static void describe_fasts(const xrfthip_plan* plan, std::string& s, const char* in_note) {
    const SGeomRt G = sgeom(plan->d.ny, plan->d.nx);
    appendf(s, "  [fasts] one pass, one %d-thread workgroup per %lld x %lld slab (%d fit a CU): the packed columns' transform, their split and the rows' "
               "transform in registers (32 complex per thread, r32x%lld / r32x%lld, three LDS exchanges in halves), exact plane detrend in the workgroup, |F|^2 "
               "rows staged in LDS and written whole with the fftshift and the Hermitian mirror, lds=%zuB; 8 algorithmic bytes per sample through memory%s\n",
            G.thr, (long long)plan->d.ny, (long long)plan->d.nx, G.per_cu, (long long)plan->d.ny / 32, (long long)plan->d.nx / 32, G.lds, in_note);
}
static void describe_fastr(const xrfthip_plan* plan, std::string& s, const char* in_note) {
    const long long nxr = plan->d.nx;
    appendf(s, "  [fastr] one pass, one %lld-thread workgroup per %lld-sample row (grid %lld): the packed %lld-point complex transform in registers (32 per thread, "
               "r32x%dx%d, LDS exchanges%s), real split through the LDS, lds=%zuB; per-row detrend + window + full (or half) spectrum; "
               "12 algorithmic bytes per sample through memory%s\n",
            nxr / 64, nxr, plan->tune_rgrid > 0 ? std::min<long long>(plan->tune_rgrid, plan->d.batch) : (long long)plan->d.batch, nxr / 2,
            nxr >= 32768 ? 32 : nxr == 4096 ? 8 : 16, nxr == 65536 ? 32 : nxr <= 8192 ? 8 : 16, nxr == 65536 ? " in halves" : "",
            nxr == 65536 ? kFastRLds : nxr == 32768 ? R2Geom<32, 16>::LDS : nxr == 16384 ? R2Geom<16, 16>::LDS : nxr == 8192 ? R2Geom<16, 8>::LDS : R2Geom<8, 8>::LDS, in_note);
}
static void describe_fastr_complex(const xrfthip_plan* plan, std::string& s, const char*) {
    appendf(s, "  [fastr complex rows] one pass, one %lld-thread workgroup per %lld-point complex row: the %s transform in registers (32 per thread, two LDS "
               "exchanges), natural order through the LDS, lds=%zuB; 16 algorithmic bytes per point through memory\n",
            (long long)plan->d.nx / 32, (long long)plan->d.nx, (plan->d.flags & XRFTHIP_INVERSE) ? "inverse" : "forward",
            plan->d.nx == 16384 ? R2Geom<32, 16>::LDS : plan->d.nx == 8192 ? R2Geom<16, 16>::LDS : plan->d.nx == 4096 ? R2Geom<16, 8>::LDS : R2Geom<8, 8>::LDS);
}
static void describe_fastr_rows(const xrfthip_plan* plan, std::string& s, const char*) {
    const bool c2r = (plan->d.flags & XRFTHIP_C2R_X) != 0;
    const YGeomRt R = yrows_geom(c2r ? plan->d.nx / 2 : plan->d.nx);
    if (c2r) appendf(s, "  [fasty complex rows] one pass: %d thr, %d rows/unit of the row-major half spectrum back to %lld real samples each (FFT%lld on the packed row; two rows per "
                        "thread through one LDS buffer), whole rows out; 8 algorithmic bytes per sample through memory\n", R.thr, R.rk, (long long)plan->d.nx, (long long)plan->d.nx / 2);
    else
    appendf(s, "  [fasty complex rows] one pass: %d thr, %d rows/unit of the row-major input (FFT%lld, %s; two rows per thread through one LDS buffer), whole rows out; "
               "16 algorithmic bytes per point through memory\n", R.thr, R.rk, (long long)plan->d.nx, (plan->d.flags & XRFTHIP_INVERSE) ? "inverse" : "forward");
}
static void info_fasts(const xrfthip_plan*, int32_t* k, int32_t* n) { *k = XRFTHIP_K_FASTS; *n = 1; }
static void info_fastr(const xrfthip_plan*, int32_t* k, int32_t* n) { *k = XRFTHIP_K_FASTR; *n = 1; }
// (the entries in the order of struct FamilyOps: family, run, describe, kernel_info, finalize, layout, binmap, uses_bluestein, reads_strided)
#ifndef __HIP_DEVICE_COMPILE__  /* host data: the device pass would emit a const object, and the launchers it points to do not exist there */
const FamilyOps kOpsFastS = {Family::FastS, run_fasts, describe_fasts, info_fasts, fast_phase_tables, layout_fasts, fasts_build_tfirst, nullptr, true};
const FamilyOps kOpsFastR = {Family::FastR, run_fastr, describe_fastr, info_fastr, fast_phase_tables, layout_one_pass, nullptr, nullptr, true};
const FamilyOps kOpsFastRComplex = {Family::FastRComplex, run_fastr, describe_fastr_complex, info_fastr, one_axis_tables, layout_one_pass};
const FamilyOps kOpsFastRRows = {Family::FastRRows, run_fastr, describe_fastr_rows, info_fastr, one_axis_tables, layout_one_pass};
#endif


// kernels of this unit that take more than 64 KB of dynamic LDS (the register-resident one-pass kernels): called once through set_kernel_attrs_once()
void set_attrs_rows() {
    const int m = (int)kLdsMax;
#define SETF(K) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, m)
    SETF((fasts_power_kernel<8, 8, 0, 0>)); SETF((fasts_power_kernel<8, 4, 0, 0>)); SETF((fasts_power_kernel<4, 8, 0, 0>));
    SETF((fasts_power_kernel<8, 8, 0>)); SETF((fasts_power_kernel<8, 8, 1>)); SETF((fasts_power_kernel<8, 8, 2>));  // (above 64 KB of dynamic LDS)
    SETF((fasts_power_kernel<8, 4, 0>)); SETF((fasts_power_kernel<8, 4, 1>)); SETF((fasts_power_kernel<8, 4, 2>));
    SETF((fasts_power_kernel<4, 8, 0>)); SETF((fasts_power_kernel<4, 8, 1>)); SETF((fasts_power_kernel<4, 8, 2>));
    SETF((fasts_power_kernel<8, 8, 0, 0, true>)); SETF((fasts_power_kernel<8, 4, 0, 0, true>)); SETF((fasts_power_kernel<4, 8, 0, 0, true>));  // (strided input)
    SETF((fasts_power_kernel<8, 8, 0, 1, true>)); SETF((fasts_power_kernel<8, 8, 1, 1, true>)); SETF((fasts_power_kernel<8, 8, 2, 1, true>));
    SETF((fasts_power_kernel<8, 4, 0, 1, true>)); SETF((fasts_power_kernel<8, 4, 1, 1, true>)); SETF((fasts_power_kernel<8, 4, 2, 1, true>));
    SETF((fasts_power_kernel<4, 8, 0, 1, true>)); SETF((fasts_power_kernel<4, 8, 1, 1, true>)); SETF((fasts_power_kernel<4, 8, 2, 1, true>));
    SETF((fastr_kernel<0, false, true>)); SETF((fastr_kernel<0, true, true>)); SETF((fastr_kernel<1, false, true>)); SETF((fastr_kernel<1, true, true>));
    SETF((fastr2_kernel<32, 16, 0, false, true>)); SETF((fastr2_kernel<32, 16, 0, true, true>)); SETF((fastr2_kernel<32, 16, 1, false, true>)); SETF((fastr2_kernel<32, 16, 1, true, true>));
    SETF((fastr2_kernel<16, 16, 0, false, true>)); SETF((fastr2_kernel<16, 16, 0, true, true>)); SETF((fastr2_kernel<16, 16, 1, false, true>)); SETF((fastr2_kernel<16, 16, 1, true, true>));
    SETF((fastr_kernel<0, false>)); SETF((fastr_kernel<0, true>)); SETF((fastr_kernel<1, false>)); SETF((fastr_kernel<1, true>));
    // (float16 / bfloat16 input)
    SETF((fasts_power_kernel<8, 8, 0, 0, false, true>)); SETF((fasts_power_kernel<8, 4, 0, 0, false, true>)); SETF((fasts_power_kernel<4, 8, 0, 0, false, true>));
    SETF((fasts_power_kernel<8, 8, 0, 1, false, true>)); SETF((fasts_power_kernel<8, 8, 1, 1, false, true>)); SETF((fasts_power_kernel<8, 8, 2, 1, false, true>));
    SETF((fasts_power_kernel<8, 4, 0, 1, false, true>)); SETF((fasts_power_kernel<8, 4, 1, 1, false, true>)); SETF((fasts_power_kernel<8, 4, 2, 1, false, true>));
    SETF((fasts_power_kernel<4, 8, 0, 1, false, true>)); SETF((fasts_power_kernel<4, 8, 1, 1, false, true>)); SETF((fasts_power_kernel<4, 8, 2, 1, false, true>));
    SETF((fastr_kernel<0, false, false, true>)); SETF((fastr_kernel<0, true, false, true>)); SETF((fastr_kernel<1, false, false, true>)); SETF((fastr_kernel<1, true, false, true>));
    SETF((fastr2_kernel<32, 16, 0, false, false, true>)); SETF((fastr2_kernel<32, 16, 0, true, false, true>)); SETF((fastr2_kernel<32, 16, 1, false, false, true>)); SETF((fastr2_kernel<32, 16, 1, true, false, true>));
    SETF((fastr2_kernel<16, 16, 0, false, false, true>)); SETF((fastr2_kernel<16, 16, 0, true, false, true>)); SETF((fastr2_kernel<16, 16, 1, false, false, true>)); SETF((fastr2_kernel<16, 16, 1, true, false, true>));
    SETF((fastc_kernel<32, 16, 0>)); SETF((fastc_kernel<32, 16, 1>)); SETF((fastc_kernel<16, 16, 0>)); SETF((fastc_kernel<16, 16, 1>));
    SETF((fastc_kernel<16, 8, 0>)); SETF((fastc_kernel<16, 8, 1>)); SETF((fastc_kernel<8, 8, 0>)); SETF((fastc_kernel<8, 8, 1>));
    SETF((fastr2_kernel<32, 16, 0, false>)); SETF((fastr2_kernel<32, 16, 0, true>)); SETF((fastr2_kernel<32, 16, 1, false>)); SETF((fastr2_kernel<32, 16, 1, true>));
    SETF((fastr2_kernel<16, 16, 0, false>)); SETF((fastr2_kernel<16, 16, 0, true>)); SETF((fastr2_kernel<16, 16, 1, false>)); SETF((fastr2_kernel<16, 16, 1, true>));
#undef SETF
}
#include "host_welch.inc"  // Family::FastW, Family::FastK: Welch spectra and spectrograms
