#include "plan.h"

// combined per-axis factors of the complex modes: the true-phase table (or 1) times (-1)^k for an ifftshifted input
// (rolling the input by n/2 -- xrft.py:436-441 -- is that sign in the spectrum; in a cross spectrum the two signs cancel)
int fast_phase_tables(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    if (d.out_mode == XRFTHIP_OUT_POWER) return XRFTHIP_OK;  // (the complex modes only)
    P->fph_on = false;
    for (int ax = 0; ax < 2; ++ax) {
        const long long n = ax == 0 ? d.ny : d.nx;
        const bool sign = d.out_mode == XRFTHIP_OUT_COMPLEX && !(d.flags & XRFTHIP_INVERSE) && (d.flags & (ax == 0 ? XRFTHIP_ISHIFT_Y : XRFTHIP_ISHIFT_X));  // (an inverse plan rotates its input)
        std::vector<cf> t((size_t)n);
        const bool dtab = dbl_phase_tables(P);
        std::vector<C2<double>> td(dtab ? (size_t)n : 0);
        for (long long k = 0; k < n; ++k) {
            double re = 1.0, im = 0.0;
            if ((size_t)(2 * k + 1) < P->host_phase[ax].size()) { re = P->host_phase[ax][(size_t)(2 * k)]; im = P->host_phase[ax][(size_t)(2 * k + 1)]; }  // (a C2R_X plan: nx/2 + 1 entries on axis 1)
            if (sign && !(n & 1)) { if (k & 1) { re = -re; im = -im; } }
            else if (sign) {  // an odd length (fastg.h takes them): the ifftshift is a rotation by n // 2 samples, X'[k] = X[k] exp(+2 pi i (n // 2) k / n)
                const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)((k * (n / 2)) % n) / (long double)n;
                const double cr = (double)cosl(a), ci = (double)sinl(a), r2 = re * cr - im * ci, i2 = re * ci + im * cr;
                re = r2; im = i2;
            }
            t[(size_t)k].re = (float)re; t[(size_t)k].im = (float)im;
            if (dtab) { td[(size_t)k].re = re; td[(size_t)k].im = im; }
            if (dtab ? (re != 1.0 || im != 0.0) : (t[(size_t)k].re != 1.0f || t[(size_t)k].im != 0.0f)) P->fph_on = true;
        }
        int rc = dtab ? P->fph[ax].upload(td.data(), td.size() * sizeof(C2<double>)) : P->fph[ax].upload(t.data(), t.size() * sizeof(cf));
        if (rc) return rc;
    }
    return XRFTHIP_OK;
}

// The one-axis families (FastMX, FastMY, FastGY, FastRComplex, FastRRows) read the window by the transform's own sample index, and the ISHIFT of an inverse plan
// rotates the samples on load: the window would multiply the DESTINATION of a sample.  The header's order is window, then rotation, so such a plan goes to the
// generic passes, which index window and input phase by the source position (their kernels are the forward transforms' too: the source-index form moved registers
// and scratch of instantiations the forward plans run).  An AXIS_Y plan with PHASE_IN has no generic form: XRFTHIP_BAD_ARG, as the header says of it.
int one_axis_tables(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    const int rc = fast_phase_tables(P);
    if (rc || !(d.flags & XRFTHIP_INVERSE)) return rc;
    if (!((P->win[0].p && (d.flags & XRFTHIP_ISHIFT_Y)) || (P->win[1].p && (d.flags & XRFTHIP_ISHIFT_X)))) return rc;
    if ((d.flags & XRFTHIP_AXIS_Y) && (d.flags & XRFTHIP_PHASE_IN)) {  // (the refused window is dropped: the plan stays what it was before the call)
        P->host_win_y.clear();
        (void)upload_real_table(P, P->win[0], nullptr, 0, 0);
        return XRFTHIP_BAD_ARG;
    }
    settle_family(P, true);
    return XRFTHIP_OK;
}

// an isotropic cross spectrum with a true-phase factor that is not 1 (two fields with different lags): its radial sums would need
// the factor per sample, which neither FastG's pass nor FastY's column pass carries (settle_family)
bool cross_iso_phase(const xrfthip_plan* P) {
    if (P->d.out_mode != XRFTHIP_OUT_CROSS || !(P->d.flags & XRFTHIP_ISO)) return false;
    for (int ax = 0; ax < 2; ++ax)
        for (size_t k = 0; k + 1 < P->host_phase[ax].size(); k += 2)
            if (std::fabs(P->host_phase[ax][k] - 1.0) > 1e-12 || std::fabs(P->host_phase[ax][k + 1]) > 1e-12) return true;
    return false;
}

// ---------------------------------------------------------------------------------------------------------------
// two-pass "y first" pipeline (fasty.h): full float32 power spectra of power-of-two slabs
// ---------------------------------------------------------------------------------------------------------------
template <int NY> static YGeomRt ycols_geom_t() {
    typedef YCols<NY> Y;
    return {Y::THR, Y::GY, Y::CW, Y::RK, Y::LBS, (size_t)(Y::GY * YLds<NY, Y::GY>::GSTR + 16 * P2<NY>::R3) * sizeof(cf) + (size_t)(Y::THR / 64) * Y::GY * 8 * sizeof(double)};
}
template <int NX, bool FS = false> static YGeomRt yrows_geom_t() {
    typedef YRows<NX, FS> R;
    return {R::THR, R::GX, 0, R::RPU, 0, (size_t)(R::GX * YLds<NX, R::GX>::GSTR + 16 * P2<NX>::R3) * sizeof(cf)};
}
// n, one of the five lengths of fasty.h (anything else counts as 256), as a compile-time constant: f(std::integral_constant<int, N>())
template <class F> static auto with_ylen(long long n, F&& f) {
    switch (n) {
        case 4096: return f(std::integral_constant<int, 4096>());
        case 2048: return f(std::integral_constant<int, 2048>());
        case 1024: return f(std::integral_constant<int, 1024>());
        case 512: return f(std::integral_constant<int, 512>());
        default: return f(std::integral_constant<int, 256>());
    }
}
static int ycols_gstr(long long ny) {  // complex elements of LDS per packed column pair of pass 1 (YLds<NY, GY>::GSTR)
    return with_ylen(ny, [](auto n) { constexpr int N = decltype(n)::value; return (int)YLds<N, YCols<N>::GY>::GSTR; });
}
YGeomRt ycols_geom(long long ny) { return with_ylen(ny, [](auto n) { return ycols_geom_t<decltype(n)::value>(); }); }
YGeomRt yrows_geom(long long nx, bool fs) {  // .rk = rows per workgroup; fs: the four-step 1-D form (256-point rows)
    if (fs) return yrows_geom_t<256, true>();
    return with_ylen(nx, [](auto n) { return yrows_geom_t<decltype(n)::value>(); });
}
long long fasty_rows_gx(const xrfthip_plan* P) { return yrows_geom(P->ynx, P->family == Family::FastY1D).gxy; }

// Four-step 1-D with a window w[n], n = nx i1 + i2: the slab-shaped float32 window table pass 1 reads, and -- column i2 of the view has
// its own window w[nx i1 + i2] -- the per-column transforms FFT_i1(w) and FFT_i1(w (i1 - ibar)) as tables [i2][k1 < nrow_pad] that carry
// the residual line back in pass 2 (fasty_rows_kernel, W2D).  Host, once per plan: nx transforms of ny points each.
static int fasty_window_spectra_1d(xrfthip_plan* P) {
    const int ny = (int)P->yny, nx = (int)P->ynx, nyh = ny / 2, nent = P->y_nrow_pad;
    const std::vector<double>& w = P->host_win_x;
    if ((long long)w.size() != (long long)ny * nx) return XRFTHIP_BAD_ARG;
    std::vector<float> wf(w.size());
    for (size_t i = 0; i < w.size(); ++i) wf[i] = (float)w[i];
    int rc = P->win2d.upload(wf.data(), wf.size() * sizeof(float));
    if (rc) return rc;
    std::vector<cf> h0((size_t)nx * nent), h1((size_t)nx * nent);
    std::vector<double> r0((size_t)ny), i0((size_t)ny), r1((size_t)ny), i1((size_t)ny);
    for (int x = 0; x < nx; ++x) {
        for (int i = 0; i < ny; ++i) {
            const double wv = w[(size_t)i * nx + x];
            r0[(size_t)i] = wv; i0[(size_t)i] = 0.0;
            r1[(size_t)i] = wv * ((double)i - 0.5 * (ny - 1)); i1[(size_t)i] = 0.0;
        }
        host_fft_pow2(r0, i0);
        host_fft_pow2(r1, i1);
        for (int k = 0; k < nent; ++k) {
            cf a, b;
            a.re = k <= nyh ? (float)r0[(size_t)k] : 0.f; a.im = k <= nyh ? (float)i0[(size_t)k] : 0.f;
            b.re = k <= nyh ? (float)r1[(size_t)k] : 0.f; b.im = k <= nyh ? (float)i1[(size_t)k] : 0.f;
            h0[(size_t)x * nent + k] = a; h1[(size_t)x * nent + k] = b;
        }
    }
    rc = P->ywhat0.upload(h0.data(), h0.size() * sizeof(cf));
    if (!rc) rc = P->ywhat1.upload(h1.data(), h1.size() * sizeof(cf));
    return rc;
}

// FFT_y(wy) and FFT_y(wy (i - ibar)) for ky < nrow_pad (zero beyond ny/2): what pass 2 needs to add the residual trend back
static int fasty_window_spectra(xrfthip_plan* P) {
    const int ny = (int)P->yny, nyh = ny / 2;
    std::vector<double> r0((size_t)ny), i0((size_t)ny, 0.0), r1((size_t)ny), i1((size_t)ny, 0.0);
    for (int i = 0; i < ny; ++i) {
        const double w = P->host_win_y.empty() ? 1.0 : P->host_win_y[(size_t)i];
        r0[(size_t)i] = w;
        r1[(size_t)i] = w * ((double)i - 0.5 * (ny - 1));
    }
    if ((ny & (ny - 1)) == 0) { host_fft_pow2(r0, i0); host_fft_pow2(r1, i1); }
    else {  // a direct O(n^2) transform with exact twiddle indices (n <= 1440, once per plan)
        std::vector<long double> cw((size_t)ny), sw((size_t)ny);
        for (int k = 0; k < ny; ++k) { const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)ny; cw[(size_t)k] = cosl(a); sw[(size_t)k] = sinl(a); }
        std::vector<double> o0r((size_t)ny), o0i((size_t)ny), o1r((size_t)ny), o1i((size_t)ny);
        for (int k = 0; k <= nyh; ++k) {
            long double a0 = 0, b0 = 0, a1 = 0, b1 = 0;
            for (int i = 0; i < ny; ++i) {
                const size_t m = (size_t)(((long long)i * k) % ny);
                a0 += r0[(size_t)i] * cw[m]; b0 += r0[(size_t)i] * sw[m];
                a1 += r1[(size_t)i] * cw[m]; b1 += r1[(size_t)i] * sw[m];
            }
            o0r[(size_t)k] = (double)a0; o0i[(size_t)k] = (double)b0; o1r[(size_t)k] = (double)a1; o1i[(size_t)k] = (double)b1;
        }
        r0 = o0r; i0 = o0i; r1 = o1r; i1 = o1i;
    }
    const int nent = P->y_nrow_pad;
    if (dbl_phase_tables(P)) {
        std::vector<C2<double>> d0((size_t)nent), d1((size_t)nent);
        for (int k = 0; k < nent; ++k) {
            d0[(size_t)k].re = k <= nyh ? r0[(size_t)k] : 0.0; d0[(size_t)k].im = k <= nyh ? i0[(size_t)k] : 0.0;
            d1[(size_t)k].re = k <= nyh ? r1[(size_t)k] : 0.0; d1[(size_t)k].im = k <= nyh ? i1[(size_t)k] : 0.0;
        }
        int rcd = P->ywhat0.upload(d0.data(), d0.size() * sizeof(C2<double>));
        if (!rcd) rcd = P->ywhat1.upload(d1.data(), d1.size() * sizeof(C2<double>));
        return rcd;
    }
    std::vector<cf> h0((size_t)nent), h1((size_t)nent);
    for (int k = 0; k < nent; ++k) {
        h0[(size_t)k].re = k <= nyh ? (float)r0[(size_t)k] : 0.f; h0[(size_t)k].im = k <= nyh ? (float)i0[(size_t)k] : 0.f;
        h1[(size_t)k].re = k <= nyh ? (float)r1[(size_t)k] : 0.f; h1[(size_t)k].im = k <= nyh ? (float)i1[(size_t)k] : 0.f;
    }
    int rc = P->ywhat0.upload(h0.data(), h0.size() * sizeof(cf));
    if (!rc) rc = P->ywhat1.upload(h1.data(), h1.size() * sizeof(cf));

    return rc;
}

// The bins a unit of rows (one workgroup of pass 2) reaches, and the units that reach a bin, of a RADIAL bin map (along a half row the
// bin never decreases: row ky holds the bins r[0] .. r[nx/2]): the unit gathers, writes and has reduced the union over its rows only.
int build_unit_windows(xrfthip_plan* P, const int32_t* bm, int rpu) {
    const int nx = (int)P->ynx, nyh = (int)P->yny / 2, units = P->y_nrow_pad / rpu;
    int rcf = XRFTHIP_OK;
    std::vector<uint32_t> w((size_t)units);
    for (int un = 0; un < units; ++un) {
        int lo = P->nbins, hi = 0;
        for (int ky = un * rpu; ky < (un + 1) * rpu && ky <= nyh; ++ky) {
            lo = std::min<int>(lo, bm[(size_t)ky * nx]);
            hi = std::max<int>(hi, bm[(size_t)ky * nx + nx / 2] + 1);
        }
        if (lo > hi) lo = hi = 0;  // (a unit of padding rows only)
        w[(size_t)un] = (uint32_t)lo | (uint32_t)hi << 16;
    }
    // ... and the units that reach a bin: a contiguous range when the windows move monotonically with ky (a radial map's do;
    // otherwise every unit keeps all bins)
    bool mono = units < 65535;
    for (int un = 1; un < units && mono; ++un) {
        if ((w[(size_t)un] >> 16) == 0) continue;  // (padding rows only)
        mono = (w[(size_t)un] & 0xffffu) >= (w[(size_t)un - 1] & 0xffffu) && (w[(size_t)un] >> 16) >= (w[(size_t)un - 1] >> 16);
    }
    if (!mono) std::fill(w.begin(), w.end(), (uint32_t)P->nbins << 16);
    std::vector<uint32_t> tu((size_t)P->nbins, 0u);
    for (int b = 0; b < P->nbins; ++b) {
        int ulo = units, uhi = 0;
        for (int un = 0; un < units; ++un)
            if ((int)(w[(size_t)un] & 0xffffu) <= b && b < (int)(w[(size_t)un] >> 16)) { ulo = std::min(ulo, un); uhi = std::max(uhi, un + 1); }
        if (ulo > uhi) ulo = uhi = 0;
        tu[(size_t)b] = (uint32_t)ulo | (uint32_t)uhi << 16;
    }
    rcf = P->ytwin.upload(w.data(), w.size() * sizeof(uint32_t));
    if (!rcf) rcf = P->ytunits.upload(tu.data(), tu.size() * sizeof(uint32_t));
    return rcf;
}

// the bin map as pass 2 reads it (fasty_rows_kernel).  Full form: [ky < nrow_pad][kx] in natural order,
// value = (bin of (ky, kx) + 1) | (bin of the mirror (-ky, -kx) + 1) << 16; rows beyond ny/2 and unbinned samples are 0.
// Compact form, when the map has the structure of a radial one (every sample of rows 0 .. ny/2 binned; along a half row the bin
// never decreases / never increases and moves by at most one per sample; the mirror sample is in the same bin except on the
// self-mirrored rows 0 and ny/2): [ky][kx / 16] = (first sample's bin + 1) | step mask << 16 -- 1/16 of the bytes.
static int fasty_build_tcodes(xrfthip_plan* P, const int32_t* bm) {
    const int ny = (int)P->yny, nx = (int)P->ynx, nyh = ny / 2;
    bool compact = env_ll("XRFTHIP_ISO_COMPACT", 1) != 0 && nx % 32 == 0;
    for (int ky = 0; ky <= nyh && compact; ++ky)
        for (int kx = 0; kx < nx; ++kx) {
            const int32_t cd = bm[(size_t)ky * nx + kx];
            if (cd < 0 || cd > 65533) { compact = false; break; }
            if (ky != 0 && ky != nyh && bm[(size_t)(ny - ky) * nx + ((nx - kx) & (nx - 1))] != cd) { compact = false; break; }
            if (kx & 15) {  // inside a segment: a step of 0 or one bin in the half row's direction
                const int32_t step = cd - bm[(size_t)ky * nx + kx - 1];
                if (step != 0 && step != (kx < nx / 2 ? 1 : -1)) { compact = false; break; }
            }
        }
    P->ytcodes_compact = compact;
    // ... and the form the atomic-free gather needs (fasty_rows_kernel): along a row the bin depends on |kx| only and never
    // decreases with it (a radial map), every sample is binned, a sample's Hermitian twin shares its bin: first[ky][b] = the
    // smallest |kx| <= nx/2 whose bin is >= b (nx/2 + 1 if none), b = 0 .. nbins
    bool radial = env_ll("XRFTHIP_ISO_GATHER", 1) != 0 && nx % 32 == 0 && P->nbins < 65535 && nx / 2 + 1 < 65535;
    for (int ky = 0; ky <= nyh && radial; ++ky) {
        const int32_t* r = bm + (size_t)ky * nx;
        for (int m = 0; m <= nx / 2; ++m) {
            const int32_t c = r[m];
            if (c < 0 || c >= P->nbins || (m > 0 && c < r[m - 1]) || (m > 0 && m < nx / 2 && r[nx - m] != c)) { radial = false; break; }
            if (ky != 0 && ky != nyh && (bm[(size_t)(ny - ky) * nx + ((nx - m) & (nx - 1))] != c || bm[(size_t)(ny - ky) * nx + m] != c)) { radial = false; break; }
        }
    }
    P->ytfirst_on = radial;
    if (radial) {
        std::vector<uint16_t> f((size_t)P->y_nrow_pad * (P->nbins + 1), (uint16_t)(nx / 2 + 1));
        for (int ky = 0; ky <= nyh; ++ky) {
            const int32_t* r = bm + (size_t)ky * nx;
            uint16_t* dst = f.data() + (size_t)ky * (P->nbins + 1);
            int m = 0;
            for (int b = 0; b <= P->nbins; ++b) {
                while (m <= nx / 2 && r[m] < b) ++m;
                dst[b] = (uint16_t)m;
            }
        }
        int rcf = P->ytfirst.upload(f.data(), f.size() * sizeof(uint16_t));
        if (rcf) return rcf;
        const bool two = P->d.out_mode == XRFTHIP_OUT_CROSS;
        const YGeomRt R = yrows_geom(P->ynx, false);
        rcf = build_unit_windows(P, bm, two ? R.gxy : R.rk);  // (rows per unit as fasty_launch_rows)
        if (rcf) return rcf;
        // the step masks of the 16-sample segments (any step size: the gather needs the run ends only)
        std::vector<uint32_t> t((size_t)P->y_nrow_pad * (nx / 16), 0u);
        for (int ky = 0; ky <= nyh; ++ky)
            for (int s0 = 0; s0 < nx; s0 += 16) {
                uint32_t w = (uint32_t)(std::min<int32_t>(bm[(size_t)ky * nx + s0], 65533) + 1);
                for (int i = 1; i < 16; ++i)
                    if (bm[(size_t)ky * nx + s0 + i] != bm[(size_t)ky * nx + s0 + i - 1]) w |= 1u << (16 + i);
                t[(size_t)ky * (nx / 16) + s0 / 16] = w;
            }
        P->ytcodes_compact = true;  // (the table has the compact form; the gather reads its masks only)
        return P->ytcodes.upload(t.data(), t.size() * sizeof(uint32_t));
    }
    if (compact) {
        std::vector<uint32_t> t((size_t)P->y_nrow_pad * (nx / 16), 0u);
        for (int ky = 0; ky <= nyh; ++ky)
            for (int s0 = 0; s0 < nx; s0 += 16) {
                uint32_t w = (uint32_t)(bm[(size_t)ky * nx + s0] + 1);
                for (int i = 1; i < 16; ++i)
                    if (bm[(size_t)ky * nx + s0 + i] != bm[(size_t)ky * nx + s0 + i - 1]) w |= 1u << (16 + i);
                t[(size_t)ky * (nx / 16) + s0 / 16] = w;
            }
        return P->ytcodes.upload(t.data(), t.size() * sizeof(uint32_t));
    }
    std::vector<uint32_t> t((size_t)P->y_nrow_pad * nx, 0u);
    for (int ky = 0; ky <= nyh; ++ky)
        for (int kx = 0; kx < nx; ++kx) {
            uint32_t v = 0;
            const int32_t cd = bm[(size_t)ky * nx + kx];
            if (cd >= 0) v |= (uint32_t)(cd + 1);
            if (ky != 0 && ky != nyh) {
                const int32_t cm = bm[(size_t)(ny - ky) * nx + ((nx - kx) & (nx - 1))];
                if (cm >= 0) v |= (uint32_t)(cm + 1) << 16;
            }
            t[(size_t)ky * nx + kx] = v;
        }
    return P->ytcodes.upload(t.data(), t.size() * sizeof(uint32_t));
}
// the radial-sum tables of one round share the transforms' LDS with the staged half of the workgroup's rows: they must fit the other half
static bool fasty_radial_tables_fit(const xrfthip_plan* P, int nbins) {
    const YGeomRt R = yrows_geom(P->ynx);
    const size_t half = (size_t)R.gxy * (size_t)(P->ynx + P->ynx / 16) * 4;  // GX rows of floats = GX / 2 rows of complex
    const size_t hw = P->d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1;
    return nbins <= 65534 && (size_t)nbins * (8 * hw + 4) <= half;
}

static void fasty_launch_cols(const xrfthip_plan* P, const FastY& p, long long gc, hipStream_t st, bool prof) {
    const xrfthip_desc& d = P->d;
    const YGeomRt C = ycols_geom(P->yny);
    xrfthip_plan::ProfRec* rec = prof ? prof_begin(P, "fasty_cols", st) : nullptr;
    const dim3 grid((unsigned)(gc * (P->ynx / C.cw))), blk((unsigned)C.thr);
    auto launch = [&](auto kern) { XRFT_LAUNCH(kern, grid, blk, C.lds, st, p); };
    with_ylen(P->yny, [&](auto n) {
        constexpr int NN = decltype(n)::value;
        const bool det = d.detrend != 0;
        if (in_half(P)) {  // float16 / bfloat16 input, dense (half_in.h): the 2-byte loaders of the same two forms
            if (P->fast1d_win) { if (det) launch(&fasty_cols_kernel<NN, true, true, false, true>); else launch(&fasty_cols_kernel<NN, false, true, false, true>); }
            else if (det) launch(&fasty_cols_kernel<NN, true, false, false, true>); else launch(&fasty_cols_kernel<NN, false, false, false, true>);
        }
        else if (in_strided(P)) {  // a box of a larger field, read where it lies (FastY only: xrfthip_plan_create)
            if (det) launch(&fasty_cols_kernel<NN, true, false, true>); else launch(&fasty_cols_kernel<NN, false, false, true>);
        }
        else if (P->fast1d_win) {  // four-step 1-D with a window: the slab-shaped window table
            if (det) launch(&fasty_cols_kernel<NN, true, true>); else launch(&fasty_cols_kernel<NN, false, true>);
        }
        else if (det) launch(&fasty_cols_kernel<NN, true>); else launch(&fasty_cols_kernel<NN, false>);
    });
    prof_end(rec, st);
    if (d.detrend) {  // plane (2-D) or line through the whole sequence (four-step 1-D) from the per-column sums -> what pass 2 has to add back
        rec = prof ? prof_begin(P, "fasty_fit", st) : nullptr;
        if (P->family == Family::FastY1D) { auto kf = &fasty_fit1d_kernel; XRFT_LAUNCH(kf, dim3((unsigned)gc), dim3(256), 3 * 256 * sizeof(double), st, (const double*)p.colfit, const_cast<float*>(p.corr), (int)P->ynx, (int)P->yny, (int)d.detrend); }
        else { auto kf = &fasty_fit_kernel; XRFT_LAUNCH(kf, dim3((unsigned)gc), dim3(256), 3 * 256 * sizeof(double), st, (const double*)p.colfit, p.win_x, const_cast<float*>(p.corr), (int)P->ynx, (int)P->yny, (int)d.detrend); }
        prof_end(rec, st);
    }
}

static void fasty_launch_rows(const xrfthip_plan* P, const FastY& p, long long gc, hipStream_t st, bool prof) {
    const xrfthip_desc& d = P->d;
    const YGeomRt R = yrows_geom(P->ynx, P->family == Family::FastY1D);
    const bool iso_on = (d.flags & XRFTHIP_ISO) != 0;
    const bool two = d.out_mode == XRFTHIP_OUT_CROSS || d.out_mode == XRFTHIP_OUT_PHASE;
    xrfthip_plan::ProfRec* rec = prof ? prof_begin(P, "fasty_rows", st) : nullptr;
    const int rpu = two ? R.gxy : R.rk;  // a cross spectrum spends both transforms of a thread on one row (field 0, field 1)
    // (four-step: rows 0 .. ny/2 - 1 in whole units, the Nyquist rows of R.gxy consecutive slabs in one extra unit each)
    const dim3 grid((unsigned)(P->family == Family::FastY1D ? gc * ((P->yny / 2) / rpu) + (gc + R.gxy - 1) / R.gxy : gc * (P->y_nrow_pad / rpu))), blk((unsigned)R.thr);
    const int hw = d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1;
    const size_t lds = R.lds;  // (the radial-sum tables alias the transforms' LDS)
    auto launch = [&](auto kern) { XRFT_LAUNCH(kern, grid, blk, lds, st, p); };
    if (P->family == Family::FastY1D) {  // four-step 1-D: rows of 256 samples, transposed stores
        if (P->fast1d_win) { if (d.out_mode == XRFTHIP_OUT_POWER) launch(&fasty_rows_kernel<256, 1, false, true, true>); else launch(&fasty_rows_kernel<256, 0, false, true, true>); }
        else if (d.out_mode == XRFTHIP_OUT_POWER) launch(&fasty_rows_kernel<256, 1, false, true>); else launch(&fasty_rows_kernel<256, 0, false, true>);
    }
    else with_ylen(P->ynx, [&](auto n) {
        constexpr int NN = decltype(n)::value;
        if (d.out_mode == XRFTHIP_OUT_POWER) { if (iso_on) launch(&fasty_rows_kernel<NN, 1, true>); else launch(&fasty_rows_kernel<NN, 1, false>); }
        else if (d.out_mode == XRFTHIP_OUT_CROSS) { if (iso_on) launch(&fasty_rows_kernel<NN, 2, true>); else launch(&fasty_rows_kernel<NN, 2, false>); }
        else if (d.out_mode == XRFTHIP_OUT_PHASE) launch(&fasty_rows_kernel<NN, 3, false>);
        else launch(&fasty_rows_kernel<NN, 0, false>);
    });
    prof_end(rec, st);
    if (iso_on) {  // the row workgroups' partial sums, added in order
        rec = prof ? prof_begin(P, "fasty_iso_reduce", st) : nullptr;
        const int nb = P->nbins * hw, upr = P->y_nrow_pad / rpu;
        auto kr = &iso_reduce_kernel;
        XRFT_LAUNCH(kr, dim3((unsigned)((nb + 63) / 64), (unsigned)gc), dim3(256), 4 * 64 * sizeof(double), st, (const double*)p.iso_part, p.iso, upr, nb, P->ytfirst_on ? reinterpret_cast<const unsigned*>(P->ytunits.p) : nullptr, hw);
        prof_end(rec, st);
    }
}

// pass 2 of a mean plan (fasty_mean.h) for the group [g0, g0 + gc): (units per slab) x (runs per output) x (the outputs the group reaches) workgroups
static void fasty_launch_rows_mean(const xrfthip_plan* P, const FastY& p, long long g0, long long gc, double* part, hipStream_t st) {
    const xrfthip_desc& d = P->d;
    const YGeomRt R = yrows_geom(P->ynx);
    const bool two = d.out_mode == XRFTHIP_OUT_CROSS;
    const int rpu = two ? R.gxy : R.rk;
    const long long M = d.mean_batch, nout = (g0 + gc - 1) / M - g0 / M + 1;
    YMean m{part, g0, (int)M, P->mean_P};
    xrfthip_plan::ProfRec* rec = prof_begin(P, "fasty_rows_mean", st);
    const dim3 grid((unsigned)((long long)(P->y_nrow_pad / rpu) * P->mean_P * nout)), blk((unsigned)R.thr);
    auto launch = [&](auto kern) { XRFT_LAUNCH(kern, grid, blk, R.lds, st, p, m); };
    with_ylen(P->ynx, [&](auto n) {
        constexpr int NN = decltype(n)::value;
        if (P->coherence) launch(&fasty_rows_mean_kernel<NN, 3>); else if (two) launch(&fasty_rows_mean_kernel<NN, 2>); else launch(&fasty_rows_mean_kernel<NN, 1>);
    });
    prof_end(rec, st);
}

// parameter block of one group of slabs [g0, g0 + gc): the intermediate and the fit tables sit in ring slot `slot` (of slot_slabs slabs each)
static FastY fasty_params(const xrfthip_plan* P, const float* in, void* out, double* iso, char* ws, long long g0, long long gc, int slot, long long slot_slabs) {
    // (slot 0 = field 0 / the only field, slot 1 = field 1 of a cross spectrum: its own intermediate and fit tables)
    const xrfthip_desc& d = P->d;
    const size_t slab_pts = (size_t)P->yny * P->ynx;
    const bool want_out = !(d.flags & XRFTHIP_NO_SPECTRUM_OUT);
    const bool iso_on = (d.flags & XRFTHIP_ISO) != 0;
    const YGeomRt C = ycols_geom(P->yny);
    const size_t s0 = (size_t)slot * slot_slabs;  // first slab of the slot inside the workspace arrays
    FastY p{};
    p.in = reinterpret_cast<const float*>(reinterpret_cast<const char*>(in) + (in_strided(P) ? (size_t)g0 * (size_t)in_slab(P) : (size_t)g0 * slab_pts) * (in_half(P) ? 2 : 4));
    p.in_bf16 = P->in16 == 2 ? 1 : 0;
    p.in_slab = in_slab(P); p.in_pitch = (int)in_pitch(P);
    p.w2 = reinterpret_cast<cf*>(ws + P->off_w) + s0 * (size_t)P->y_nrow_pad * P->ynx;
    const size_t out_esz = (d.out_mode == XRFTHIP_OUT_POWER || d.out_mode == XRFTHIP_OUT_PHASE) ? sizeof(float) : sizeof(cf);
    const size_t out_pts = (size_t)P->yny * ((d.flags & XRFTHIP_HALF_X) ? P->ynx / 2 + 1 : P->ynx);
    p.out = want_out ? (char*)out + (size_t)g0 * out_pts * out_esz : nullptr;
    p.half = (d.flags & XRFTHIP_HALF_X) ? 1 : 0;
    p.realdim2 = (d.flags & XRFTHIP_REALDIM_X2) ? 1 : 0;
    p.ph_y = reinterpret_cast<const cf*>(P->fph[0].p);
    p.ph_x = reinterpret_cast<const cf*>(P->fph[1].p);
    p.tw_big = reinterpret_cast<const cf*>(P->tw_big1d.p);
    p.ph_on = P->fph_on ? 1 : 0;
    p.tw_x = reinterpret_cast<const cf*>(P->tw_fx.p);
    p.tw_y = reinterpret_cast<const cf*>(P->tw_fy.p);
    p.win_y = reinterpret_cast<const float*>(P->win[0].p ? P->win[0].p : P->ones4096.p);
    p.win_x = reinterpret_cast<const float*>(P->win[1].p ? P->win[1].p : P->ones4096.p);
    p.colfit = reinterpret_cast<double*>(ws + P->off_rowfit) + s0 * (size_t)P->ynx * 4;
    p.corr = reinterpret_cast<const float*>(ws + P->off_corr) + s0 * (size_t)P->ynx * 2;
    p.what0 = reinterpret_cast<const cf*>(P->ywhat0.p);
    p.what1 = reinterpret_cast<const cf*>(P->ywhat1.p);
    p.tcodes = reinterpret_cast<const unsigned*>(P->ytcodes.p);
    p.tcodes_compact = P->ytcodes_compact ? 1 : 0;
    p.tfirst = P->ytfirst_on ? reinterpret_cast<const unsigned short*>(P->ytfirst.p) : nullptr;
    p.twin = P->ytfirst_on ? reinterpret_cast<const unsigned*>(P->ytwin.p) : nullptr;
    p.iso = iso_on ? iso + (size_t)g0 * P->nbins * (d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1) : nullptr;
    p.nbins = P->nbins;
    p.iso_part = reinterpret_cast<double*>(ws + P->off_isopart);
    p.ny = (int)P->yny; p.nx = (int)P->ynx;
    p.nrow_pad = P->y_nrow_pad;
    p.l_cw = ilog2i(C.cw); p.l_rk = ilog2i(C.rk); p.l_2gy = ilog2i(2 * C.gxy);
    p.detrend = d.detrend;
    p.nslab = (int)gc;
    p.shift_y = (d.flags & XRFTHIP_SHIFT_Y) ? (int)(P->yny / 2) : 0;
    p.shift_x = (d.flags & XRFTHIP_SHIFT_X) ? (int)(P->ynx / 2) : 0;  // (four-step 1-D: the shift by N/2 samples is k2 + nx/2)
    if (P->family == Family::FastY1D) p.win_y = p.win_x = reinterpret_cast<const float*>(P->ones4096.p);  // (a window of the whole sequence: win2d)
    p.win2d = reinterpret_cast<const float*>(P->fast1d_win ? P->win2d.p : nullptr);
    p.scale = (float)d.scale;
    return p;
}

// FastY: real float32 slabs whose two lengths are 256 .. 4096 powers of two, every mode (fasty_fits: also the fallback FastS builds beside itself)
bool fasty_fits(const xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    const uint32_t shifts = XRFTHIP_SHIFT_Y | XRFTHIP_SHIFT_X, ish = XRFTHIP_ISHIFT_Y | XRFTHIP_ISHIFT_X, isof = XRFTHIP_ISO | XRFTHIP_NO_SPECTRUM_OUT;
    const uint32_t halff = XRFTHIP_HALF_X | XRFTHIP_REALDIM_X2;  // real_dim: half output, no mirror
    const uint32_t allowed = d.out_mode == XRFTHIP_OUT_POWER ? (shifts | isof | halff) : d.out_mode == XRFTHIP_OUT_COMPLEX ? (shifts | ish | XRFTHIP_HALF_X)
                             : d.out_mode == XRFTHIP_OUT_CROSS ? (shifts | ish | isof | halff) : d.out_mode == XRFTHIP_OUT_PHASE ? (shifts | ish | XRFTHIP_HALF_X) : 0u;
    return d.ndim == 2 && fasty_len(d.ny) && fasty_len(d.nx) && d.dtype == XRFTHIP_F32 &&
           !(d.flags & ~allowed) && !((d.flags & halff) && (d.flags & XRFTHIP_ISO)) && !((d.flags & XRFTHIP_HALF_X) && (d.flags & XRFTHIP_SHIFT_X));
}
int fasty_tables(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    P->yny = d.ny; P->ynx = d.nx;
    const int rpu = yrows_geom(d.nx).rk;
    P->y_nrow_pad = (int)((d.ny / 2 + 1 + rpu - 1) / rpu * rpu);
    int rc = plan_twiddle(P, P->tw_fx, d.nx, d.nx);
    if (!rc) rc = plan_twiddle(P, P->tw_fy, d.ny, d.ny);
    if (!rc) rc = plan_ones(P, std::max(d.ny, d.nx));
    return rc;
}
int try_fasty(xrfthip_plan* P) {
    if (!fasty_fits(P)) return kDeclined;
    // (a mean plan, xrfthip_desc.mean_batch: every class of fasty_mean.h measured faster than the composition it replaces, profiles/r15_batch_mean.txt)
    P->family = P->chosen = Family::FastY;
    return fasty_tables(P);
}

// FastY1D: one long real float32 sequence per slab, N = n1 * 256 samples (2^16 .. 2^20): the two passes of the y-first pipeline are
// the two steps of its four-step transform (fasty.h, FS)
int try_fast1d(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    const long long n1 = d.nx / 256;
    const bool pow2 = d.nx >= 65536 && d.nx <= (1LL << 20) && (d.nx & (d.nx - 1)) == 0;
    const uint32_t ok1 = XRFTHIP_SHIFT_X | (d.out_mode == XRFTHIP_OUT_COMPLEX ? XRFTHIP_ISHIFT_X : 0u);
    if (!(d.ndim == 1 && pow2 && d.dtype == XRFTHIP_F32 && (d.out_mode == XRFTHIP_OUT_COMPLEX || d.out_mode == XRFTHIP_OUT_POWER) &&
          !(d.flags & ~ok1) && env_ll("XRFTHIP_FAST1D", 1) != 0)) return kDeclined;
    P->family = P->chosen = Family::FastY1D;
    P->yny = n1; P->ynx = 256;
    const int rpu = yrows_geom(256, true).rk;
    P->y_nrow_pad = (int)((n1 / 2 + 1 + rpu - 1) / rpu * rpu);
    int rc = plan_twiddle(P, P->tw_fx, 256, 256);
    if (!rc) rc = plan_twiddle(P, P->tw_fy, n1, n1);
    if (!rc) rc = plan_twiddle(P, P->tw_big1d, d.nx, d.nx / 2 + 1);
    if (!rc) rc = plan_ones(P, std::max<long long>(n1, 256));
    return rc;
}

// FastYC: complex float32 slabs of the fasty lengths (fasty_c2c.h); FastYCFourStep: ONE long complex float32 sequence per batch entry,
// 2^16 .. 2^20 points (xrft.ifft of the spectrum of a long row, fft of complex rows: the inverse twin of BASELINE config 2): the same two
// passes on the [n / 256][256] view, pass 2 in its four-step form (before: the generic four-step passes, 49 GFFT/s)
int try_fastyc(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    if (d.dtype != XRFTHIP_C64 || d.detrend || (d.out_mode != XRFTHIP_OUT_COMPLEX && d.out_mode != XRFTHIP_OUT_POWER) || env_ll("XRFTHIP_FASTYC", 1) == 0) return kDeclined;
    const bool cplx_out = d.out_mode == XRFTHIP_OUT_COMPLEX;
    const uint32_t okc = XRFTHIP_SHIFT_Y | XRFTHIP_SHIFT_X | (cplx_out ? (XRFTHIP_ISHIFT_Y | XRFTHIP_ISHIFT_X | XRFTHIP_INVERSE | XRFTHIP_PHASE_IN | XRFTHIP_C2R_X) : 0u);
    const uint32_t okf = XRFTHIP_SHIFT_X | (cplx_out ? (XRFTHIP_ISHIFT_X | XRFTHIP_INVERSE | XRFTHIP_PHASE_IN) : 0u);
    const bool c2r = (d.flags & XRFTHIP_C2R_X) != 0;  // (irfftn: the half spectrum in, nx real samples per row out; the row transforms have nx/2 points)
    int rc;
    if (d.ndim == 2 && fasty_len(d.ny) && (c2r ? (d.nx % 2 == 0 && fasty_len(d.nx / 2)) : fasty_len(d.nx)) && !(d.flags & ~okc)) {
        P->family = P->chosen = Family::FastYC;
        const long long nxt = c2r ? d.nx / 2 : d.nx;
        rc = plan_twiddle(P, P->tw_fx, nxt, nxt);
        if (!rc && c2r) rc = plan_twiddle(P, P->tw_big1d, d.nx, d.nx / 32);  // W_nx^u, u < (nx/2) / 16
        if (!rc) rc = plan_twiddle(P, P->tw_fy, d.ny, d.ny);
        P->yny = d.ny; P->ynx = d.nx;
    } else if (d.ndim == 1 && d.nx >= 65536 && d.nx <= 1048576 && (d.nx & (d.nx - 1)) == 0 && !(d.flags & ~okf)) {
        P->family = P->chosen = Family::FastYCFourStep;
        rc = plan_twiddle(P, P->tw_fx, 256, 256);
        if (!rc) rc = plan_twiddle(P, P->tw_big1d, d.nx, d.nx / 16);  // W_N^j, j < N / 16: the four-step twiddles of a row (k1 u, k1 NT)
        if (!rc) rc = plan_twiddle(P, P->tw_fy, d.nx / 256, d.nx / 256);
        P->yny = d.nx / 256; P->ynx = 256;
    } else {
        return kDeclined;
    }
    return rc ? rc : plan_ones(P, 4096);
}

// ---- the pass-1 block (xrfthip_exec_ex): what the column pass and the fit kernel leave for ONE field -- intermediate, per-column sums and lines, corrections --
// as one piece of memory outside the workspace, so that a second plan over the same field can read it instead of running the two kernels again.
// Only where the whole batch is one group of slabs (the block is the field's, not a ring slot's).
size_t fasty_pass1_bytes(const xrfthip_plan* P) {
    if (P->family != Family::FastY || P->d.batch < 1 || P->G < P->d.batch) return 0;
    if (((P->p1_w | P->p1_fit | P->p1_corr) & 255) || !P->p1_w) return 0;  // (the lengths of fasty.h leave whole 256-byte units: the workspace holds exactly these bytes per field)
    return P->p1_w + P->p1_fit + P->p1_corr;
}

// Everything that decides the bytes of a field's block, hashed (FNV-1a, 64 bit): two plans with equal signatures leave identical blocks from the same input.
namespace {
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } }
    void num(long long v) { bytes(&v, sizeof v); }
    void table(const std::vector<double>& t) { num((long long)t.size()); if (!t.empty()) bytes(t.data(), t.size() * sizeof(double)); }
};
}
uint64_t fasty_pass1_signature(const xrfthip_plan* P, int field) {
    const xrfthip_desc& d = P->d;
    const YGeomRt C = ycols_geom(P->yny);
    Fnv f;
    f.num(XRFTHIP_VERSION); f.num((long long)sizeof(cf));
    // the kernel: fasty_cols_kernel<NY, DET, W2D = false, STR>, then fasty_fit_kernel with a detrend
    f.num(P->yny); f.num(d.detrend != 0); f.num(in_strided(P)); f.num(d.detrend);
    f.num(d.ny); f.num(d.nx); f.num(d.batch); f.num(P->G); f.num(P->y_nrow_pad); f.num(d.dtype); f.num(d.ndim);
    f.num(C.thr); f.num(C.gxy); f.num(C.cw); f.num(C.rk); f.num(C.lbs); f.num((long long)C.lds); f.num(ycols_gstr(P->yny));
    f.num((long long)P->p1_w); f.num((long long)P->p1_fit); f.num((long long)P->p1_corr);
    f.num(in_pitch(P)); f.num(in_slab(P));
    if (in_half(P)) f.num(P->in16);  // (fasty_cols_kernel<.., H16> and the format it reads; a float32 plan's signature is what it was)
    // the field's own flip flags (fasty.h takes none today: a plan with one never reaches here)
    const uint32_t fy = field == 0 && plan_two(P) ? XRFTHIP_FLIP0_Y : XRFTHIP_FLIP_Y, fx = field == 0 && plan_two(P) ? XRFTHIP_FLIP0_X : XRFTHIP_FLIP_X;
    f.num((d.flags & fy) != 0); f.num((d.flags & fx) != 0);
    // the tables pass 1 reads: the windows (the float32 tables are these values rounded; none = ones) -- win_x is the fit kernel's, too; W_ny^k follows from ny
    f.table(P->host_win_y); f.table(P->host_win_x);
    return f.h;
}

static int run_fasty(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d = P->d;
    const float *in = (const float*)a.in0, *in1 = (const float*)a.in1;
    void* out = a.out; double* iso = a.iso; char* ws = a.ws; hipStream_t st = a.stream;
    const bool two = d.out_mode == XRFTHIP_OUT_CROSS || d.out_mode == XRFTHIP_OUT_PHASE;
    // a field whose pass 1 lives in a block of the caller's (xrfthip_exec_ex: one group of slabs, g0 = 0): the three parts in the workspace's order
    auto in_block = [&](FastY& q, int f) {
        if (!a.p1_mode[f]) return;
        q.w2 = reinterpret_cast<cf*>(a.p1_block[f]);
        q.colfit = reinterpret_cast<double*>(a.p1_block[f] + P->p1_w);
        q.corr = reinterpret_cast<const float*>(a.p1_block[f] + P->p1_w + P->p1_fit);
    };
    // ... and with every field there, the workspace is the plan's without the fields' shares: what lies behind them moves up
    const bool compact = a.p1_mode[0] && (!two || a.p1_mode[1]);
    // a mean plan (xrfthip_desc.mean_batch): the row pass adds into the outputs' partial sums, zero before the first group; one finishing pass writes d_out
    double* mpart = nullptr;
    if (mean_plan(P)) {
        mpart = reinterpret_cast<double*>(ws + (P->off_mean - (compact ? (size_t)(two ? 2 : 1) * fasty_pass1_bytes(P) : 0)));
        HIP_TRY(hipMemsetAsync(mpart, 0, P->ws_bytes - P->off_mean, st));
    }
    for (long long g0 = 0; g0 < d.batch; g0 += P->G) {
        const long long gc = std::min<long long>(P->G, d.batch - g0);
        FastY p = fasty_params(P, in, out, iso, ws, g0, gc, 0, P->G);
        in_block(p, 0);
        if (compact) p.iso_part = reinterpret_cast<double*>(ws + (P->off_isopart - (size_t)(two ? 2 : 1) * fasty_pass1_bytes(P)));
        if (a.p1_mode[0] != XRFTHIP_PASS1_CONSUME) fasty_launch_cols(P, p, gc, st, true);
        if (two) {  // field 1 through the same column pass into its own intermediate; the row pass reads both
            FastY p1 = fasty_params(P, in1, out, iso, ws, g0, gc, 1, P->G);
            in_block(p1, 1);
            if (a.p1_mode[1] != XRFTHIP_PASS1_CONSUME) fasty_launch_cols(P, p1, gc, st, true);
            p.w2b = p1.w2;
            p.corr_b = p1.corr;
        }
        if (mpart) fasty_launch_rows_mean(P, p, g0, gc, mpart, st);
        else fasty_launch_rows(P, p, gc, st, true);
        HIP_TRY(hipGetLastError());
    }
    return mpart ? run_mean_finish(P, mpart, out, st) : XRFTHIP_OK;
}

// the two-pass pipeline on complex float32 slabs (fasty_c2c.h): columns -> rows, group by group
static int run_fastyc(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d0 = P->d;
    const void* in = a.in0; void* out = a.out; char* ws = a.ws; hipStream_t st = a.stream;
    // (the four-step form: every batch entry is ONE sequence of d.nx points, transformed as the [d.nx / 256][256] view)
    const bool fs = P->family == Family::FastYCFourStep;
    struct { long long batch, ny, nx; uint32_t flags; int out_mode; double scale; } d{d0.batch, fs ? d0.nx / 256 : d0.ny, fs ? 256 : d0.nx, d0.flags, d0.out_mode, d0.scale};
    const bool c2r = (d.flags & XRFTHIP_C2R_X) != 0;
    const long long nxt = c2r ? d.nx / 2 : d.nx;  // points of the row transforms
    const YGeomRt C = ycols_geom(d.ny), R = yrows_geom(nxt);
    const int cw = 2 * C.gxy, rk = std::max(1, 16 / cw);
    const int nxb_full = (int)(nxt / cw), w2_nxb = nxb_full + (c2r ? 1 : 0);
    const long long in_pitch = c2r ? d.nx / 2 + 1 : d.nx;
    const size_t lds_c = (size_t)(C.gxy * (ycols_gstr(d.ny)) + 16 * (d.ny / 256)) * sizeof(cf);
    const size_t out_esz = (d.out_mode == XRFTHIP_OUT_POWER || c2r) ? sizeof(float) : sizeof(cf);
    for (long long g0 = 0; g0 < d.batch; g0 += P->G) {
        const long long gc = std::min<long long>(P->G, d.batch - g0);
        FastYC p{};
        p.in = reinterpret_cast<const cf*>(in) + (size_t)g0 * d.ny * in_pitch;
        p.c2r = c2r ? 1 : 0; p.in_pitch = (int)in_pitch; p.w2_nxb = w2_nxb;
        p.tw_big = reinterpret_cast<const cf*>(P->tw_big1d.p);
        p.w2 = reinterpret_cast<cf*>(ws + P->off_w);
        p.out = (char*)out + (size_t)g0 * d.ny * d.nx * out_esz;
        p.tw_x = reinterpret_cast<const cf*>(P->tw_fx.p);
        p.tw_y = reinterpret_cast<const cf*>(P->tw_fy.p);
        p.win_y = reinterpret_cast<const float*>(P->win[0].p ? P->win[0].p : P->ones4096.p);
        p.win_x = reinterpret_cast<const float*>(P->win[1].p ? P->win[1].p : P->ones4096.p);
        p.win_on = (P->win[0].p || P->win[1].p) ? 1 : 0;
        p.ph_y = reinterpret_cast<const cf*>(P->fph[0].p);
        p.ph_x = reinterpret_cast<const cf*>(P->fph[1].p);
        const bool phase = d.out_mode == XRFTHIP_OUT_COMPLEX && P->fph_on;
        p.ph_in = (phase && (d.flags & XRFTHIP_PHASE_IN)) ? 1 : 0;
        p.ph_on = (phase && !(d.flags & XRFTHIP_PHASE_IN)) ? 1 : 0;
        p.inv = (d.flags & XRFTHIP_INVERSE) ? 1 : 0;
        p.ishift_y = ((d.flags & XRFTHIP_INVERSE) && (d.flags & XRFTHIP_ISHIFT_Y)) ? 1 : 0;  // (a forward plan's ifftshifted input is the sign (-1)^k in the phase tables)
        p.ishift_x = ((d.flags & XRFTHIP_INVERSE) && (d.flags & XRFTHIP_ISHIFT_X)) ? 1 : 0;
        p.shift_y = (d.flags & XRFTHIP_SHIFT_Y) ? (int)(d.ny / 2) : 0;
        p.shift_x = (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0;
        if (fs) {
            p.fs = 1;
            // the sequence rotated by N / 2 = the view's rows rotated by ny / 2; its fftshift = the row transforms' output rotated by 128; an input phase in its
            // separable form (finalize_plan), an output phase as the table over the whole sequence
            p.ishift_y = p.ishift_x; p.ishift_x = 0; p.shift_y = 0;
            if (p.ph_in) p.ph_x = reinterpret_cast<const cf*>(P->fs_phx.p);
        }
        p.ny = (int)d.ny; p.nx = (int)d.nx; p.nslab = (int)gc;
        p.l_cw = ilog2i(cw); p.l_rk = ilog2i(rk);
        p.power = d.out_mode == XRFTHIP_OUT_POWER ? 1 : 0;
        p.scale = (float)d.scale;
        xrfthip_plan::ProfRec* rec = prof_begin(P, "fastyc_cols", st);
        const dim3 gridc((unsigned)(gc * nxb_full + (c2r ? gc : 0))), blkc((unsigned)C.thr);
        with_ylen(d.ny, [&](auto n) { auto k = &fastyc_cols_kernel<decltype(n)::value>; XRFT_LAUNCH(k, gridc, blkc, lds_c, st, p); });
        prof_end(rec, st);
        rec = prof_begin(P, "fastyc_rows", st);
        const dim3 gridr((unsigned)(gc * (d.ny / R.rk))), blkr((unsigned)R.thr);
#define YC2_(NN) do { auto k = &fastyc_rows_c2r_kernel<NN, false>; XRFT_LAUNCH(k, gridr, blkr, R.lds, st, p); } while (0)
        if (c2r) { if (nxt == 2048) YC2_(2048); else if (nxt == 1024) YC2_(1024); else if (nxt == 512) YC2_(512); else YC2_(256); }  // (four lengths: nx / 2)
        else with_ylen(d.nx, [&](auto n) { auto k = &fastyc_rows_kernel<decltype(n)::value>; XRFT_LAUNCH(k, gridr, blkr, R.lds, st, p); });
#undef YC2_
        prof_end(rec, st);
        HIP_TRY(hipGetLastError());
    }
    return XRFTHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the rows of FastY, FastY1D, FastYC and FastYCFourStep (plan.h, FamilyOps)
// ---------------------------------------------------------------------------------------------------------------
// the tables of the two y-first passes that depend on a window / a phase (FastY, FastM, FastN; the fused inner passes)
int two_pass_tables(xrfthip_plan* P) {
    const int rc = fasty_window_spectra(P);
    return rc ? rc : fast_phase_tables(P);
}
static int finalize_fast1d(xrfthip_plan* P) {
    P->fast1d_win = !P->host_win_x.empty();  // (a window rides on a slab-shaped table)
    const int rc = P->fast1d_win ? fasty_window_spectra_1d(P) : fasty_window_spectra(P);
    return rc ? rc : fast_phase_tables(P);
}
static int finalize_fastyc_four_step(xrfthip_plan* P) {
    int rc = fast_phase_tables(P);
    if (rc) return rc;
    // a window has no separable form over the view; an input phase (PHASE_IN: the lag's factor on the source samples) must be one -- exp(i theta n) is:
    // row factor ph[256 i1], column factor ph[i2] / ph[0]; checked, else the generic passes take the plan
    bool ok = P->host_win_x.empty() && !P->win[1].p;
    if (ok && (P->d.flags & XRFTHIP_PHASE_IN) && P->fph_on) {
        const std::vector<double>& h = P->host_phase[1];
        const long long n = P->d.nx, vy = n / 256;
        ok = (long long)h.size() >= 2 * n;
        std::vector<cf> py((size_t)vy), px(256);
        if (ok) {
            const double r0 = h[0], i0 = h[1], m0 = r0 * r0 + i0 * i0;
            for (long long i1 = 0; i1 < vy; ++i1) { py[(size_t)i1].re = (float)h[(size_t)(512 * i1)]; py[(size_t)i1].im = (float)h[(size_t)(512 * i1 + 1)]; }
            for (int i2 = 0; i2 < 256; ++i2) {  // ph[i2] conj(ph[0]) / |ph[0]|^2
                const double re = h[(size_t)(2 * i2)], im = h[(size_t)(2 * i2 + 1)];
                px[(size_t)i2].re = (float)((re * r0 + im * i0) / m0); px[(size_t)i2].im = (float)((im * r0 - re * i0) / m0);
            }
            double worst = 0.0;
            for (long long nn = 0; nn < n; ++nn) {  // (every product: one O(n) host pass when the table is set; a sample let a single wrong entry through)
                const long long i1 = nn / 256; const int i2 = (int)(nn % 256);
                const double yr = h[(size_t)(512 * i1)], yi = h[(size_t)(512 * i1 + 1)], xr = (h[(size_t)(2 * i2)] * r0 + h[(size_t)(2 * i2 + 1)] * i0) / m0, xi = (h[(size_t)(2 * i2 + 1)] * r0 - h[(size_t)(2 * i2)] * i0) / m0;
                worst = std::max(worst, std::hypot(yr * xr - yi * xi - h[(size_t)(2 * nn)], yr * xi + yi * xr - h[(size_t)(2 * nn + 1)]));
            }
            ok = worst < 1e-9 && m0 > 0.0;
        }
        if (ok) {
            rc = P->fph[0].upload(py.data(), py.size() * sizeof(cf));
            if (!rc) rc = P->fs_phx.upload(px.data(), px.size() * sizeof(cf));
        }
    }
    if (!rc && !ok) settle_family(P, true);  // (the generic four-step passes)
    return rc;
}
// the tiled intermediate of one group of slabs
static void layout_fastyc(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    long long G = d.slabs_per_group > 0 ? d.slabs_per_group : (P->tune_fast_group > 0 ? P->tune_fast_group : std::max<long long>(1, (32LL * 4096 * 4096) / (d.ny * d.nx)));
    G = std::max<long long>(1, std::min<long long>(G, std::max<long long>(d.batch, 1)));
    P->G = (int)G;
    P->off_w = 0;
    size_t w2_cols = (size_t)d.nx;  // complex columns of the intermediate per row
    if (d.flags & XRFTHIP_C2R_X) { const size_t cw = 2 * (size_t)ycols_geom(d.ny).gxy; w2_cols = (size_t)d.nx / 2 + cw; }  // (+ the block of the Nyquist column)
    P->ws_bytes = (((size_t)G * (size_t)d.ny * w2_cols * sizeof(cf)) + 255) & ~(size_t)255;
}
static int fasty_binmap(xrfthip_plan* P, const int32_t* bm) {
    const int rc = fasty_build_tcodes(P, bm);
    if (!rc && !P->ytfirst_on && !fasty_radial_tables_fit(P, P->nbins)) settle_family(P, true);  // (any map: the atomic tables alias half of the transforms' LDS)
    return rc;
}
static void describe_fasty(const xrfthip_plan* plan, std::string& s, const char* in_note) {
    const bool fs = plan->family == Family::FastY1D;
    const YGeomRt C = ycols_geom(plan->yny), R = yrows_geom(plan->ynx, fs);
    if (fs) appendf(s, "  [fasty four-step] %lld samples = [%lld][%lld]: columns = step 1 (half spectrum k1 <= %lld), rows x W_N^(i2 k1) = step 2, transposed stores + Hermitian mirror\n",
                              (long long)plan->d.nx, (long long)plan->yny, (long long)plan->ynx, (long long)plan->yny / 2);
    appendf(s, "  [fasty] cols: %d thr, %d x 2 packed column pairs (FFT%lld r16x16x%lld, column-local detrend fused), %d columns/unit, lds=%zuB -> W2[slab][%d/%d][nx/%d][2][%d][%d] -> rows: %d thr, %d rows/unit (FFT%lld r16x16x%lld), lds=%zuB, |F|^2 + fftshift + mirror rows%s\n",
            C.thr, C.gxy, (long long)plan->d.ny, (long long)plan->d.ny / 256, C.cw, C.lds, plan->y_nrow_pad, C.rk, C.cw, C.rk, 2 * C.gxy,
            R.thr, R.rk, (long long)plan->d.nx, (long long)plan->d.nx / 256, R.lds, in_note);
    if (mean_plan(plan)) appendf(s, "  [fasty mean] the row pass is fasty_rows_mean_kernel: a workgroup walks a run of ONE output's slabs inside the group, |F|^2 (F0 conj F1) summed in 32 registers%s\n",
                                  plan->coherence ? "; coherence: |F0|^2 and |F1|^2 beside them, 64 registers, two waves per SIMD" : "");
    if ((plan->d.flags & XRFTHIP_ISO) && plan->ytcodes.p)
        appendf(s, "  [fasty radial sums] fused into the row pass (runs of equal bins from the staged rows, int64 fixed-point tables), bin codes: %s\n",
                plan->ytfirst_on ? "radial map: per-bin gather, no atomics" : plan->ytcodes_compact ? "compact (radial map: first bin + step mask per 16 samples)" : "full (4 bytes per sample)");
}
static void describe_fastyc(const xrfthip_plan* plan, std::string& s, const char*) {
    const YGeomRt C = ycols_geom(plan->d.ny), R = yrows_geom(plan->d.nx);
    if (plan->d.flags & XRFTHIP_C2R_X) {
        const YGeomRt R2 = yrows_geom(plan->d.nx / 2);
        appendf(s, "  [fasty complex] cols: %d thr, %d x 2 adjacent complex columns of the half spectrum (FFT%lld, inverse: conjugate in / out) + one block for the Nyquist column, "
                   "%d columns/unit -> W2 -> rows: %d thr, %d rows/unit: the half spectrum of a row back to %lld real samples (FFT%lld on the packed row), whole rows out; "
                   "16 B per point through memory\n", C.thr, C.gxy, (long long)plan->d.ny, 2 * C.gxy, R2.thr, R2.rk, (long long)plan->d.nx, (long long)plan->d.nx / 2);
    } else
    appendf(s, "  [fasty complex] cols: %d thr, %d x 2 adjacent complex columns (FFT%lld, %s), %d columns/unit -> W2[slab][%lld/%d][nx/%d][%d][%d] -> rows: %d thr, %d rows/unit "
               "(FFT%lld), whole rows out (scale, %sfftshift); 32 B per point through memory\n",
            C.thr, C.gxy, (long long)plan->d.ny, (plan->d.flags & XRFTHIP_INVERSE) ? "inverse: conjugate in / out" : "forward", 2 * C.gxy, (long long)plan->d.ny,
            std::max(1, 16 / (2 * C.gxy)), 2 * C.gxy, std::max(1, 16 / (2 * C.gxy)), 2 * C.gxy, R.thr, R.rk, (long long)plan->d.nx, plan->fph_on ? "phase, " : "");
}
static void describe_fastyc_four_step(const xrfthip_plan* plan, std::string& s, const char*) {
    const YGeomRt C = ycols_geom(plan->d.nx / 256), R = yrows_geom(256);
    appendf(s, "  [fasty complex rows, four-step] two passes over the [%lld][256] view of every %lld-point sequence: cols: %d thr, FFT%lld along the view's rows index (input rotation / lag phase / "
               "conjugation on load) -> W2 in whole lines -> rows: %d thr, %d rows/unit x W_N^(i2 k1), FFT256, stored transposed (X[k1 + %lld k2]: runs of %d samples)%s; 32 bytes per point through memory\n",
            (long long)plan->d.nx / 256, (long long)plan->d.nx, C.thr, (long long)plan->d.nx / 256, R.thr, R.rk, (long long)plan->d.nx / 256, R.rk / 2,
            (plan->d.flags & XRFTHIP_INVERSE) ? "; inverse: conjugate in / out" : "");
}
static void info_fasty(const xrfthip_plan*, int32_t* k, int32_t* n) { *k = XRFTHIP_K_FASTY; *n = 0; }
// (the entries in the order of struct FamilyOps: family, run, describe, kernel_info, finalize, layout, binmap, uses_bluestein, reads_strided, strided_if, dbl_tables, two_pass_y)
#ifndef __HIP_DEVICE_COMPILE__  /* host data: the device pass would emit a const object, and the launchers it points to do not exist there */
const FamilyOps kOpsFastY = {Family::FastY, run_fasty, describe_fasty, info_fasty, two_pass_tables, layout_passes, fasty_binmap, nullptr, true, nullptr, false, true};
const FamilyOps kOpsFastY1D = {Family::FastY1D, run_fasty, describe_fasty, info_fasty, finalize_fast1d, layout_passes, nullptr, nullptr, false, nullptr, false, true};
const FamilyOps kOpsFastYC = {Family::FastYC, run_fastyc, describe_fastyc, info_fasty, fast_phase_tables, layout_fastyc};
const FamilyOps kOpsFastYCFourStep = {Family::FastYCFourStep, run_fastyc, describe_fastyc_four_step, info_fasty, finalize_fastyc_four_step, layout_fastyc};
#endif


// kernels of this unit that take more than 64 KB of dynamic LDS (the y-first float32 kernels): called once through set_kernel_attrs_once()
void set_attrs_fasty() {
    const int m = (int)kLdsMax;
#define SETF(K) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, m)
#define SETY(NN) SETF((fasty_cols_kernel<NN, false>)); SETF((fasty_cols_kernel<NN, true>)); SETF((fasty_cols_kernel<NN, false, true>)); SETF((fasty_cols_kernel<NN, true, true>)); SETF((fasty_cols_kernel<NN, false, false, true>)); SETF((fasty_cols_kernel<NN, true, false, true>)); \
                 SETF((fasty_cols_kernel<NN, false, false, false, true>)); SETF((fasty_cols_kernel<NN, true, false, false, true>)); SETF((fasty_cols_kernel<NN, false, true, false, true>)); SETF((fasty_cols_kernel<NN, true, true, false, true>)); /* (float16 / bfloat16 input) */ \
                 SETF((fasty_rows_kernel<NN, 1, false>)); SETF((fasty_rows_kernel<NN, 1, true>)); \
                 SETF((fasty_rows_kernel<NN, 0, false>)); SETF((fasty_rows_kernel<NN, 2, false>)); SETF((fasty_rows_kernel<NN, 2, true>)); SETF((fasty_rows_kernel<NN, 3, false>))
    SETY(4096); SETY(2048); SETY(1024); SETY(512); SETY(256);
#undef SETY
#define SETC(NN) SETF((fastyc_cols_kernel<NN>)); SETF((fastyc_rows_kernel<NN>))
    SETC(4096); SETC(2048); SETC(1024); SETC(512); SETC(256);
    SETF((fastyc_rows_c2r_kernel<2048, false>)); SETF((fastyc_rows_c2r_kernel<1024, false>)); SETF((fastyc_rows_c2r_kernel<512, false>)); SETF((fastyc_rows_c2r_kernel<256, false>));
    SETF((fastyc_rows_c2r_kernel<2048, true>)); SETF((fastyc_rows_c2r_kernel<1024, true>)); SETF((fastyc_rows_c2r_kernel<512, true>)); SETF((fastyc_rows_c2r_kernel<256, true>));
#undef SETC
    SETF((fasty_rows_kernel<256, 0, false, true>)); SETF((fasty_rows_kernel<256, 1, false, true>));
    SETF((fasty_rows_kernel<256, 0, false, true, true>)); SETF((fasty_rows_kernel<256, 1, false, true, true>));
#undef SETF
}
