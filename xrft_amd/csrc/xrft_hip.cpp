// xrft_hip.cpp -- the plan builder, the generic tile passes, and the C ABI of the plan (see plan.h for the map of the host units).
#include "plan.h"

thread_local int xrfth::g_last_hip_error = 0;

namespace {

struct TileChoice { int T, threads, seq_stride, pad_shift; size_t lds; };

// pick sequences-per-tile for an n-point FFT; `col`: the tile axis is the contiguous one in memory, so T*csize
// bytes per row segment should reach a 128-byte line.  Returns T = 0 if one sequence does not fit in LDS.
TileChoice choose_tile(long long n_logical, size_t csize, bool col, long long avail, size_t hist_bytes) {
    const long long n = lds_fft_len(n_logical, csize);
    TileChoice c{};
    c.pad_shift = csize == 8 ? 4 : 3;
    long long ss = n + (n >> c.pad_shift) + 1;
    if ((ss & 1) == 0) ++ss;
    c.seq_stride = (int)ss;
    const size_t per = (size_t)ss * csize;
    const size_t hard = kLdsMax - hist_bytes - 64;
    // measured (scripts/prof_generic3.py): for long sequences larger tiles (wider chunks, more threads) beat two small
    // workgroups per CU; short ones already get 8+ sequences into 64 KiB
    const size_t soft = (size_t)env_ll("XRFTHIP_LDS_SOFT", (64 * 1024) / per < 8 ? 144 * 1024 : 64 * 1024);
    long long target = std::max<long long>(1, 8192 / std::max<long long>(n, 1));
    if (col) target = std::max<long long>(target, (long long)(128 / csize));
    long long T = std::min<long long>(target, (long long)(soft / per));
    const long long want = col ? std::min<long long>(4, target) : 1;
    if (T < want) T = std::min<long long>(target, (long long)(hard / per));
    if (T > avail) T = avail;
    if (T < 1) { c.T = 0; return c; }
    if (col) { long long p2 = 1; while (p2 * 2 <= T) p2 *= 2; T = p2; }
    c.T = (int)T;
    long long th = (T * n + 15) / 16;
    th = ((th + 63) / 64) * 64;
    c.threads = (int)std::min<long long>(csize == 16 ? 512 : 1024, std::max<long long>(64, th));  // float64: 256 VGPRs per lane
    c.lds = (((size_t)T * per + 15) & ~(size_t)15) + hist_bytes;
    return c;
}

// split n = n1 * n2 with both factors as close to sqrt(n) as the factorisation allows
bool split_two(long long n, long long& n1, long long& n2) {
    long long best = 0;
    for (long long a = 1; a * a <= n; ++a)
        if (n % a == 0) best = a;
    if (best <= 1) return false;
    n1 = n / best;  // n1 >= n2
    n2 = best;
    return true;
}

template <typename T>
struct Builder {
    xrfthip_plan& P;
    bool cur_raw = false;  // building the field-0 pipeline of a cross spectrum: its own flip flags (xrft.py:436-441 flips each field by its own coordinate)
    explicit Builder(xrfthip_plan& p) : P(p) {}
    bool flip_x() const { return (P.d.flags & (cur_raw ? XRFTHIP_FLIP0_X : XRFTHIP_FLIP_X)) != 0; }
    bool flip_y() const { return (P.d.flags & (cur_raw ? XRFTHIP_FLIP0_Y : XRFTHIP_FLIP_Y)) != 0; }

    int tables_for(int n, FftTables** out) {
        auto it = P.tables.find(n);
        if (it == P.tables.end()) {
            FftTables& t = P.tables[n];
            int rc = build_tables<T>(t, n);
            if (rc) { P.tables.erase(n); return rc; }
            *out = &t;
        } else *out = &it->second;
        return XRFTHIP_OK;
    }

    int set_fft(Pass& ps, int n) {
        FftTables* t;
        int rc = tables_for(n, &t);
        if (rc) return rc;
        ps.g.n = t->blue_m ? t->blue_m : n;
        ps.g.blue_n = t->blue_m ? n : 0;
        ps.g.blue_c = t->blue_c.p;
        ps.g.blue_b = t->blue_b.p;
        ps.g.nr = (int)t->radix.size();
        for (int i = 0; i < ps.g.nr; ++i) ps.g.radix[i] = t->radix[i];
        ps.g.tw = t->tw.p;
        ps.g.rev = (const unsigned*)t->rev.p;
        ps.generic = t->generic;
        return XRFTHIP_OK;
    }

    void apply_tile(Pass& ps, const TileChoice& c) {
        ps.g.T = c.T;
        ps.g.dbg = (int)env_ll("XRFTHIP_DBG", 0);
        ps.g.seq_stride = c.seq_stride;
        ps.g.pad_shift = c.pad_shift;
        ps.threads = c.threads;
        ps.lds = c.lds;
        // twiddle table of this pass' FFT length in LDS when it fits next to the tile
        const size_t twb = (size_t)ps.g.n * P.csize + 32;
        if (ps.g.n > 1 && twb <= 48 * 1024 && ps.lds + twb <= kLdsMax && env_ll("XRFTHIP_TW_LDS", 1)) {
            ps.g.tw_lds = 1;
            ps.lds += twb;
        }
        const size_t rvb = (size_t)ps.g.n * sizeof(unsigned) + 32;
        if (ps.g.n > 1 && !ps.g.blue_n && rvb <= 32 * 1024 && ps.lds + rvb <= kLdsMax && env_ll("XRFTHIP_REV_LDS", 1)) {
            ps.g.rev_lds = 1;
            ps.lds += rvb;
        }
    }

    void fill_prologue(Pass& ps, long long rows, long long jmp, long long jmq) {
        const xrfthip_desc& d = P.d;
        Prologue& pr = ps.pr;
        pr.in_complex = P.cplx_in;
        pr.detrend = d.detrend != XRFTHIP_DETREND_NONE;
        pr.rows = rows;
        pr.j_mul_p = jmp;
        pr.j_mul_q = jmq;
        pr.ny = (int)d.ny;
        pr.nx = (int)d.nx;
        pr.flip_y = flip_y();
        pr.ishift_y = !!(d.flags & XRFTHIP_ISHIFT_Y);
        pr.flip_x = flip_x();
        pr.ishift_x = !!(d.flags & XRFTHIP_ISHIFT_X);
        pr.slab_stride = d.ny * d.nx;
        pr.row_stride = d.nx;
        pr.conj_in = !!(d.flags & XRFTHIP_INVERSE);
        if (d.flags & XRFTHIP_C2R_X) {
            pr.herm_nxh = (int)(d.nx / 2 + 1);
            pr.row_stride = d.nx / 2 + 1;
            pr.slab_stride = d.ny * (d.nx / 2 + 1);
        }
        ps.first = true;
        ps.in_kind = B_IN;
    }

    // raw: final pass of the F0 pipeline of CROSS (plain complex spectrum, unshifted, into the F0 buffer)
    void fill_epilogue(Pass& ps, bool raw, int p_axis, long long odiv) {
        const xrfthip_desc& d = P.d;
        Epilogue& ep = ps.ep;
        ep.mode = raw ? 0 : d.out_mode;
        ep.p_axis = p_axis;
        ep.odiv = odiv;
        ep.r_mul = odiv > 1 ? 1 : 0;
        ep.q_mul = 0;
        ep.p_mul = odiv;
        ep.ny = (int)d.ny;
        ep.nx = (int)d.nx;
        ep.scale = raw ? 1.0 : d.scale;
        if (raw) {
            ep.nx_out = (int)P.width;
            ep.mirror = 0;
            ep.shift_y = ep.shift_x = 0;
            ep.realdim_x2 = 0;
            ep.slab_stride = d.ny * P.width;
            ep.row_stride = P.width;
            ps.out_kind = B_F0;
        } else {
            ep.nx_out = (int)P.nx_out;
            ep.mirror = P.mirror;
            ep.shift_y = !!(d.flags & XRFTHIP_SHIFT_Y);
            ep.shift_x = !!(d.flags & XRFTHIP_SHIFT_X);
            ep.realdim_x2 = !!(d.flags & XRFTHIP_REALDIM_X2);
            ep.conj_out = !!(d.flags & XRFTHIP_INVERSE);
            ep.real_out = !!(d.flags & XRFTHIP_C2R_X);
            ep.slab_stride = d.ny * P.nx_out;
            ep.row_stride = P.nx_out;
            ep.other_slab_stride = d.ny * P.width;
            ep.other_row_stride = P.width;
            ps.out_kind = B_OUT;
        }
        ps.final_ = true;
    }

    size_t hist_bytes(bool) const { return 0; }  // (radial sums are a pass of their own over the stored spectrum: run_radial_sums)

    // ---------------------------------------------------------------- x passes (along the contiguous axis)
    // rows_per_slab = ny (2-D) or 1 (1-D).  `last`: the x transform is the whole transform (1-D).
    int build_x(std::vector<Pass>& out, bool raw) {
        const xrfthip_desc& d = P.d;
        const bool last = d.ndim == 1;
        const long long rows = d.ny;
        const bool real_in = !P.cplx_in;
        const bool want_r2c = real_in && d.nx % 2 == 0 && d.nx >= 2 && P.width == d.nx / 2 + 1;
        const long long n = want_r2c ? d.nx / 2 : d.nx;
        TileChoice c = choose_tile(n, P.csize, false, std::max<long long>(1, rows * d.batch), last ? hist_bytes(raw) : 0);
        const bool four = P.width == d.nx && (c.T == 0 || n >= env_ll("XRFTHIP_X_FOURSTEP_MIN", 1LL << 40)) && n > 1;
        if (c.T == 0 && !four) return XRFTHIP_UNSUPPORTED_LENGTH;
        if (!four) {
            Pass ps;
            ps.label = want_r2c ? "x:r2c-row" : "x:row";
            int rc = set_fft(ps, (int)n);
            if (rc) return rc;
            apply_tile(ps, c);
            ps.g.r2c = want_r2c;
            ps.g.n_out = (int)P.width;
            if (want_r2c) {
                DevBuf* b = new DevBuf();
                P.extra.push_back(b);
                rc = build_twiddle<T>(*b, d.nx, n + 1);
                if (rc) return rc;
                ps.g.tw_r2c = b->p;
            }
            ps.g.tile_axis = 0;
            ps.g.in_fast = 0;
            ps.g.out_fast = 0;
            ps.g.inner = 1;
            ps.g.tiles_per_outer = 1;
            ps.outer_per_slab = rows;
            fill_prologue(ps, rows, 1, 0);
            if (real_in && !flip_x() && !(d.flags & (XRFTHIP_C2R_X | XRFTHIP_INVERSE)) && env_ll("XRFTHIP_LEAN_ROWS", 1) &&
                ps.lds + 48 * (size_t)c.T + 32 <= kLdsMax) {  // lean row loader: per-row constants behind everything else
                ps.g.rowc_off = (int)((ps.lds + 15) & ~(size_t)15);
                ps.lds = (size_t)ps.g.rowc_off + 48 * (size_t)c.T;
            }
            if (last) {
                fill_epilogue(ps, raw, 0, 1);
            } else {
                ps.g.out_so = P.width;
                ps.g.out_sq = 0;
                ps.g.out_sp = 1;
                ps.out_kind = B_W;
            }
            out.push_back(ps);
            return XRFTHIP_OK;
        }
        // ---- four-step along x: nx = n1 * n2, A: FFT over i1 (stride n2) + twiddle, B: FFT over i2, transposed store
        long long n1, n2;
        if (!split_two(d.nx, n1, n2)) return XRFTHIP_UNSUPPORTED_LENGTH;
        TileChoice ca = choose_tile(n1, P.csize, true, n2, 0);
        TileChoice cb = choose_tile(n2, P.csize, true, n1, last ? hist_bytes(raw) : 0);
        if (ca.T == 0 || cb.T == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
        DevBuf* big = new DevBuf();
        P.extra.push_back(big);
        int rc = build_twiddle<T>(*big, d.nx, d.nx);
        if (rc) return rc;
        {
            Pass a;
            a.label = "x:four-step-A";
            rc = set_fft(a, (int)n1);
            if (rc) return rc;
            apply_tile(a, ca);
            a.g.n_out = (int)n1;
            a.g.tile_axis = 1;
            a.g.in_fast = 1;
            a.g.out_fast = 1;
            a.g.inner = n2;
            a.g.tiles_per_outer = (n2 + ca.T - 1) / ca.T;
            a.outer_per_slab = rows;
            fill_prologue(a, rows, n2, 1);
            a.g.out_so = d.nx; a.g.out_sq = 1; a.g.out_sp = n2;
            a.g.tw_big = big->p; a.g.tw_bigN = d.nx; a.g.tw_qdiv = 1; a.g.tw_qmod = n2;
            a.out_kind = B_W2;
            if (ca.T <= 64 && (ca.T & (ca.T - 1)) == 0 && a.threads % ca.T == 0 && env_ll("XRFTHIP_LEAN_COL", 1)) {
                a.g.lean_col = 2;
                if (d.ndim == 1 && real_in && !flip_x() && !(d.flags & (XRFTHIP_C2R_X | XRFTHIP_INVERSE))) a.g.lean_col |= 1;
            }
            out.push_back(a);
        }
        {
            Pass b;
            b.label = "x:four-step-B";
            rc = set_fft(b, (int)n2);
            if (rc) return rc;
            apply_tile(b, cb);
            b.g.n_out = (int)n2;
            b.g.tile_axis = 1;
            b.g.in_fast = 0;
            b.g.out_fast = 1;
            b.g.inner = n1;
            b.g.tiles_per_outer = (n1 + cb.T - 1) / cb.T;
            b.outer_per_slab = rows;
            b.in_kind = B_W2;
            b.g.in_so = d.nx; b.g.in_sq = n2; b.g.in_sp = 1;
            if (last) {
                fill_epilogue(b, raw, 0, 1);
                b.ep.q_mul = 1;  // kx = k1 + n1 * k2
                b.ep.p_mul = n1;
                if ((b.ep.mode == 0 || b.ep.mode == 1) && !b.ep.conj_out && !b.ep.real_out && !b.ep.mirror && cb.T <= 64 &&
                    (cb.T & (cb.T - 1)) == 0 && b.threads % cb.T == 0 && env_ll("XRFTHIP_LEAN_FINAL", 1))
                    b.g.lean_final = 2;
            } else {
                b.g.out_so = d.nx; b.g.out_sq = 1; b.g.out_sp = n1;
                b.out_kind = B_W;
            }
            out.push_back(b);
        }
        return XRFTHIP_OK;
    }

    // ---------------------------------------------------------------- y passes (strided axis of the intermediate)
    int build_y(std::vector<Pass>& out, bool raw) {
        const xrfthip_desc& d = P.d;
        const long long ny = d.ny, w = P.width;
        TileChoice c = choose_tile(ny, P.csize, true, w, hist_bytes(raw));
        const long long min_t = std::min<long long>(env_ll("XRFTHIP_Y_MIN_T", 4), w);
        bool four = (c.T < min_t || ny >= env_ll("XRFTHIP_Y_FOURSTEP_MIN", 1LL << 40)) && ny > 3;
        long long n1 = 0, n2 = 0;
        if (four && !split_two(ny, n1, n2)) four = false;
        if (!four) {
            if (c.T == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
            Pass ps;
            ps.label = "y:col";
            int rc = set_fft(ps, (int)ny);
            if (rc) return rc;
            apply_tile(ps, c);
            ps.g.n_out = (int)ny;
            ps.g.tile_axis = 1;
            ps.g.in_fast = 1;
            ps.g.out_fast = 1;
            ps.g.inner = w;
            ps.g.tiles_per_outer = (w + c.T - 1) / c.T;
            ps.outer_per_slab = 1;
            ps.in_kind = B_W;
            ps.g.in_so = ny * w; ps.g.in_sq = 1; ps.g.in_sp = w;
            fill_epilogue(ps, raw, 1, 1);
            if ((ps.ep.mode == 0 || ps.ep.mode == 1) && !ps.ep.conj_out && !ps.ep.real_out && c.T >= 1 && c.T <= 64 &&
                (c.T & (c.T - 1)) == 0 && ps.threads % c.T == 0 && env_ll("XRFTHIP_LEAN_FINAL", 1))
                ps.g.lean_final = 1;
            out.push_back(ps);
            return XRFTHIP_OK;
        }
        TileChoice ca = choose_tile(n1, P.csize, true, n2 * w, 0);
        TileChoice cb = choose_tile(n2, P.csize, true, w, hist_bytes(raw));
        if (ca.T == 0 || cb.T == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
        DevBuf* big = new DevBuf();
        P.extra.push_back(big);
        int rc = build_twiddle<T>(*big, ny, ny);
        if (rc) return rc;
        {
            Pass a;  // in place on W viewed as [slab][n1][n2*w]
            a.label = "y:four-step-A";
            rc = set_fft(a, (int)n1);
            if (rc) return rc;
            apply_tile(a, ca);
            a.g.n_out = (int)n1;
            a.g.tile_axis = 1;
            a.g.in_fast = 1;
            a.g.out_fast = 1;
            a.g.inner = n2 * w;
            a.g.tiles_per_outer = (n2 * w + ca.T - 1) / ca.T;
            a.outer_per_slab = 1;
            a.in_kind = B_W;
            a.out_kind = B_W;
            a.g.in_so = ny * w; a.g.in_sq = 1; a.g.in_sp = n2 * w;
            a.g.out_so = ny * w; a.g.out_sq = 1; a.g.out_sp = n2 * w;
            a.g.tw_big = big->p; a.g.tw_bigN = ny; a.g.tw_qdiv = w; a.g.tw_qmod = n2;
            out.push_back(a);
        }
        {
            Pass b;  // sequences (slab, k1, kx): o = slab*n1 + k1, q = kx, points i2 (stride w)
            b.label = "y:four-step-B";
            rc = set_fft(b, (int)n2);
            if (rc) return rc;
            apply_tile(b, cb);
            b.g.n_out = (int)n2;
            b.g.tile_axis = 1;
            b.g.in_fast = 1;
            b.g.out_fast = 1;
            b.g.inner = w;
            b.g.tiles_per_outer = (w + cb.T - 1) / cb.T;
            b.outer_per_slab = n1;
            b.in_kind = B_W;
            b.g.in_so = n2 * w; b.g.in_sq = 1; b.g.in_sp = w;
            fill_epilogue(b, raw, 1, n1);
            out.push_back(b);
        }
        return XRFTHIP_OK;
    }

    // XRFTHIP_AXIS_Y: one column pass that is first AND final -- reads the caller's [slab][ny][nx] array with the prologue
    // (point p = row, q = column) and writes the result in the same layout
    int build_yonly(std::vector<Pass>& out, bool raw) {
        const xrfthip_desc& d = P.d;
        TileChoice c = choose_tile(d.ny, P.csize, true, d.nx, 0);
        if (c.T == 0) return XRFTHIP_UNSUPPORTED_LENGTH;  // (longer columns: transpose on the caller's side and use a 1-D plan)
        Pass ps;
        ps.label = "y:col-only";
        int rc = set_fft(ps, (int)d.ny);
        if (rc) return rc;
        apply_tile(ps, c);
        ps.g.n_out = (int)d.ny;
        ps.g.tile_axis = 1;
        ps.g.in_fast = 1;
        ps.g.out_fast = 1;
        ps.g.inner = d.nx;
        ps.g.tiles_per_outer = (d.nx + c.T - 1) / c.T;
        ps.outer_per_slab = 1;
        fill_prologue(ps, 1, 0, 0);
        ps.pr.p_is_row = 1;
        fill_epilogue(ps, raw, 1, 1);
        out.push_back(ps);
        return XRFTHIP_OK;
    }

    int build_pipeline(std::vector<Pass>& out, bool raw) {
        cur_raw = raw;
        if (P.d.flags & XRFTHIP_AXIS_Y) return build_yonly(out, raw);
        int rc = build_x(out, raw);
        if (rc) return rc;
        if (P.d.ndim == 2) rc = build_y(out, raw);
        if (rc) return rc;
        // one row pass feeding one column pass: hand the intermediate over in tiles of the column pass's T columns
        if (out.size() == 2 && out[0].g.rowc_off > 0 && out[0].out_kind == B_W && out[1].in_kind == B_W && out[1].g.tile_axis == 1 &&
            out[1].g.T >= 2 && (out[1].g.T & (out[1].g.T - 1)) == 0 && env_ll("XRFTHIP_TILED_W", 1)) {
            const int tc = out[1].g.T;
            const long long wc = (P.width + tc - 1) / tc * tc;
            if (P.w_cols == 0 || P.w_cols == wc) {  // (the F0 pipeline of a cross spectrum picks the same T)
                P.w_cols = wc;
                out[0].g.out_tiled = tc; out[1].g.in_tiled = tc;
                out[0].g.til_stride = out[1].g.til_stride = P.d.ny * tc;
                out[0].g.til_slab = out[1].g.til_slab = (wc / tc) * P.d.ny * tc;
                out[0].g.til_ny = out[1].g.til_ny = (int)P.d.ny;
            }
        }
        // single-purpose kernel instantiations where every precondition of a lean path is known now
        if (env_ll("XRFTHIP_PATHS", 1) && !env_ll("XRFTHIP_DBG", 0)) {
            const xrfthip_desc& d = P.d;
            const bool no_iso_out = !(d.flags & (XRFTHIP_ISO | XRFTHIP_NO_SPECTRUM_OUT)), no_phase_in = !(d.flags & XRFTHIP_PHASE_IN);
            for (Pass& ps : out) {
                if (ps.generic) continue;
                if (ps.first && ps.g.tile_axis == 0 && ps.g.rowc_off > 0 && no_phase_in && (!ps.final_ || no_iso_out)) ps.path = 1;
                else if (!ps.first && ps.final_ && ps.g.in_tiled && ps.g.lean_final == 1 && (raw || no_iso_out)) ps.path = 2;
                else if (ps.first && !ps.final_ && ps.g.lean_col == 3 && no_phase_in) ps.path = 3;
                else if (!ps.first && ps.final_ && ps.g.lean_final == 2 && (raw || no_iso_out)) ps.path = 4;
            }
        }
        return XRFTHIP_OK;
    }
};

template <typename T>
int build_plan_t(xrfthip_plan& P) {
    Builder<T> B(P);
    P.w_cols = 0;
    int rc = B.build_pipeline(P.passes, false);
    if (rc) return rc;
    if (P.d.out_mode == XRFTHIP_OUT_CROSS || P.d.out_mode == XRFTHIP_OUT_PHASE) rc = B.build_pipeline(P.passes_f0, true);
    return rc;
}

void set_kernel_attrs_once() {
    static bool done = false;
    if (done) return;
    done = true;
    for (int f = 0; f < kFamilyCount; ++f)  // every row at its own place in the table
        if (family_ops((Family)f).family != (Family)f) { std::fprintf(stderr, "xrfthip: the row of Family %d is misplaced\n", f); std::abort(); }
    const int m = (int)kLdsMax;
    // the generic tile kernels live in this unit; every family sets its own (host_*.cpp)
#define SETA(TT, A, B, C) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_fft_kernel<TT, A, B, C, sizeof(TT) == 8 ? 512 : 1024, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, m)
#define SETP(TT, A, B, PP) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_fft_kernel<TT, A, B, false, sizeof(TT) == 8 ? 512 : 1024, PP>), hipFuncAttributeMaxDynamicSharedMemorySize, m)
#define SETPATHS(TT) SETP(TT, true, false, 1); SETP(TT, true, true, 1); SETP(TT, false, true, 2); SETP(TT, true, false, 3); SETP(TT, false, true, 4)
    SETPATHS(float);
    SETPATHS(double);
#undef SETPATHS
#undef SETP
#define SETALL(TT) SETA(TT, false, false, false); SETA(TT, false, false, true); SETA(TT, false, true, false); SETA(TT, false, true, true); \
                   SETA(TT, true, false, false); SETA(TT, true, false, true); SETA(TT, true, true, false); SETA(TT, true, true, true)
    SETALL(float);
    SETALL(double);
#undef SETALL
    set_attrs_fasty();
    set_attrs_fastm();
    set_attrs_fastg();
    set_attrs_rows();
    set_attrs_welch();
}

template <typename T>
void launch_tile(const Pass& ps, int grid, hipStream_t st) {
    const dim3 g((unsigned)grid), b((unsigned)ps.threads);
    // float64 plans run at most 512 threads per block (choose_tile) on the instantiation with 256 VGPRs per lane; float32
    // keeps the 128-VGPR one (its small tiles want four workgroups per CU)
    constexpr int MT = sizeof(T) == 8 ? 512 : 1024;
#define LP_(A, B, PP) do { auto k = &tile_fft_kernel<T, A, B, false, MT, PP>; XRFT_LAUNCH(k, g, b, ps.lds, st, ps.g, ps.pr, ps.ep); } while (0)
    if (ps.path && !ps.generic) {  // single-purpose instantiations (preconditions checked when the plan was built)
        if (ps.path == 1 && ps.first && !ps.final_) { LP_(true, false, 1); return; }
        if (ps.path == 1 && ps.first && ps.final_) { LP_(true, true, 1); return; }
        if (ps.path == 2 && !ps.first && ps.final_) { LP_(false, true, 2); return; }
        if (ps.path == 3 && ps.first && !ps.final_) { LP_(true, false, 3); return; }
        if (ps.path == 4 && !ps.first && ps.final_) { LP_(false, true, 4); return; }
    }
#undef LP_
#define L_(A, B, C) do { auto k = &tile_fft_kernel<T, A, B, C, MT, 0>; XRFT_LAUNCH(k, g, b, ps.lds, st, ps.g, ps.pr, ps.ep); } while (0)
    const int sel = (ps.first ? 4 : 0) | (ps.final_ ? 2 : 0) | (ps.generic ? 1 : 0);
    switch (sel) {
        case 0: L_(false, false, false); break;
        case 1: L_(false, false, true); break;
        case 2: L_(false, true, false); break;
        case 3: L_(false, true, true); break;
        case 4: L_(true, false, false); break;
        case 5: L_(true, false, true); break;
        case 6: L_(true, true, false); break;
        default: L_(true, true, true); break;
    }
#undef L_
}

void describe_passes(std::string& s, const std::vector<Pass>& v, const char* name) {
    for (const Pass& p : v) {
        appendf(s, "  [%s] %-16s n=%d radix=", name, p.label.c_str(), p.g.n);
        for (int i = 0; i < p.g.nr; ++i) appendf(s, "%s%d", i ? "x" : "", p.g.radix[i]);
        appendf(s, " T=%d threads=%d lds=%zuB%s%s%s%s\n", p.g.T, p.threads, p.lds, p.g.r2c ? " r2c" : "",
                p.first ? " first" : "", p.final_ ? " final" : "", p.generic ? " generic-radix" : "");
    }
}

}  // namespace

void appendf(std::string& s, const char* fmt, ...) {
    char buf[1024];  // (the longest describe line, [fastw], is about 800 characters)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}

int upload_real_table(xrfthip_plan* P, DevBuf& buf, const double* h, int64_t n, int cplx) {
    if (!h) { buf.clear(); return XRFTHIP_OK; }
    const size_t cnt = (size_t)n * (cplx ? 2 : 1);
    if (P->dbl) return buf.upload(h, cnt * sizeof(double));
    std::vector<float> f(cnt);
    for (size_t i = 0; i < cnt; ++i) f[i] = (float)h[i];
    return buf.upload(f.data(), cnt * sizeof(float));
}

// the specialised families' tables in the plan's precision: W_N^k (k < count), and a table of n ones (the windows' stand-in)
int plan_twiddle(xrfthip_plan* P, DevBuf& buf, long long N, long long count) {
    return P->dbl ? build_twiddle<double>(buf, N, count) : build_twiddle<float>(buf, N, count);
}
int plan_ones(xrfthip_plan* P, long long n) {
    const std::vector<double> ones((size_t)n, 1.0);
    return upload_real_table(P, P->ones4096, ones.data(), n, 0);
}

// Where a plan's tables hand it on (finalize_plan, xrfthip_plan_set_binmap).  decline: the chosen family cannot serve the plan, for good --
// FastS passes it to the FastY tables built beside it (256 x 256, try_fasts) or to the generic passes, every other family to the generic
// passes.  Then the one rule that is decided again whenever a table changes: a FastY isotropic cross spectrum with a true-phase factor that
// is not 1 runs the generic passes, and FastY again once the factor is 1.
void settle_family(xrfthip_plan* P, bool decline) {
    if (decline) P->chosen = (P->chosen == Family::FastS && P->tw_fy.p) ? Family::FastY : Family::Generic;
    P->family = (P->chosen == Family::FastY && cross_iso_phase(P)) ? Family::Generic : P->chosen;
}

// workgroups per slab of radial_binsum_det_kernel: chunks of <= 2^17 elements (its int64 sums hold 2^17 values), at most 128
int iso_chunk_count(long long total) {
    long long c = std::max<long long>(1, std::min<long long>(128, total / 16384));
    while ((total + c - 1) / c > (1LL << 17)) ++c;
    return (int)c;
}
// bins per launch: the int64 sums and the exponent table of a window of bins share 64 KB of LDS
static int iso_bin_window(bool cplx) { return (int)((64 * 1024) / (cplx ? 24 : 16)); }  // (+ 4 bytes per bin: the non-finite flags)

// radial sums of `bc` stored spectra [bc][ny][nxo] (rows / columns rotated by sy / sx) -> iso[bc][nbins (x2)], bit-reproducible
int run_radial_sums(int32_t dtype, const void* spec, const int32_t* d_binmap, long long bc, long long ny, long long nxo, int sy, int sx,
                           int nbins, int chunks, double* part, double* iso, hipStream_t st) {
    const bool dbl = dtype == XRFTHIP_F64 || dtype == XRFTHIP_C128, cplx = dtype >= XRFTHIP_C64;
    const int hw = cplx ? 2 : 1, win = iso_bin_window(cplx);
    const long long total = ny * nxo;
    const size_t esz = (dbl ? 8 : 4) * (size_t)hw;
    for (long long s0 = 0; s0 < bc; s0 += 32768) {  // grid.y limit
        const long long sc = std::min<long long>(32768, bc - s0);
        const void* src = (const char*)spec + (size_t)s0 * total * esz;
        double* pdst = part + (size_t)s0 * chunks * nbins * hw;
        for (int b0 = 0; b0 < nbins; b0 += win) {
            const int nb = std::min(win, nbins - b0);
            const dim3 grid((unsigned)chunks, (unsigned)sc), block(256);
            int ncopy = 1;  // copies of the tables (lanes spread over them: neighbouring samples share bins), as many as fit 32 KB
            while (ncopy < 8 && (size_t)nb * (cplx ? 20 : 12) * (2 * ncopy) <= 32 * 1024) ncopy *= 2;
            const size_t lds = (size_t)nb * (cplx ? 20 : 12) * ncopy + (size_t)nb * 4;
#define ISO_(TT, CC) do { auto k = &radial_binsum_det_kernel<TT, CC>; XRFT_LAUNCH(k, grid, block, lds, st, src, (const int*)d_binmap, total, (int)nxo, (int)ny, sy, sx, b0, nb, nbins, ncopy, pdst); } while (0)
            if (dbl) { if (cplx) ISO_(double, true); else ISO_(double, false); } else { if (cplx) ISO_(float, true); else ISO_(float, false); }
#undef ISO_
        }
        auto kr = &iso_reduce_kernel;
        XRFT_LAUNCH(kr, dim3((unsigned)((nbins * hw + 63) / 64), (unsigned)sc), dim3(256), 4 * 64 * sizeof(double), st, (const double*)pdst,
                    iso + (size_t)s0 * nbins * hw, chunks, nbins * hw, (const unsigned*)nullptr, hw);
    }
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

// the one-pass families (registers + LDS): no intermediate
void layout_one_pass(xrfthip_plan* P) {
    P->G = (int)std::max<long long>(1, std::min<long long>(P->d.batch, 1 << 30));
    P->ws_bytes = 0;
}

// the generic passes' layout (Generic, FastMX, FastMY) and, for the two y-first passes (two_pass_y), their intermediate, per-column sums and corrections
void layout_passes(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    const bool fast = two_pass_y(P);
    long long G = d.slabs_per_group > 0 ? d.slabs_per_group : P->tune_group;
    size_t slab_w = (size_t)d.ny * std::max(P->width, P->w_cols) * P->csize;
    if (fast) {
        slab_w = (size_t)P->y_nrow_pad * (size_t)(P->y_pitch > 0 ? P->y_pitch : P->ynx) * (fastm_pipeline(P) ? P->csize : sizeof(cf));
        if (G <= 0) G = P->tune_fast_group > 0 ? P->tune_fast_group : std::max<long long>(1, (64LL * 4096 * 4096) / (d.ny * d.nx));  // y-first, 4096^2: 16: 62.7, 32: 61.4 us per slab; 32 -> 64: 301-303 -> 306-307 GFFT/s (tails, launch gaps and the plane-fit bubble amortise)
    }
    if (G <= 0) {
        // the Infinity Cache adds no bandwidth, so groups are sized for launch efficiency, not residency
        const size_t target = (size_t)P->tune_group_bytes;
        G = (long long)std::max<size_t>(1, target / std::max<size_t>(slab_w, 1));
    }
    G = std::max<long long>(1, std::min<long long>(G, std::max<long long>(d.batch, 1)));
    // radial sums fused into the row pass (fasty always, fastm / fastn where fastm_iso_fused says so) end in iso_reduce_kernel with the group's slabs on grid.y: a larger
    // group -- only a caller's slabs_per_group asks for one -- runs as several.  Held for every y-first plan with radial sums, whether or not the sums are fused (which
    // is only known once the bin map is set; run_radial_sums chunks grid.y itself): the group, hence the workspace, does not depend on the map.  xrfthip_plan_describe
    // prints the group that runs
    if (fast && (d.flags & XRFTHIP_ISO)) G = std::min<long long>(G, 65535);
    P->G = (int)G;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const int nf = (d.out_mode == XRFTHIP_OUT_CROSS || d.out_mode == XRFTHIP_OUT_PHASE) ? 2 : 1;
    size_t off = 0;
    const size_t ncoef = (size_t)d.batch * ((d.flags & XRFTHIP_AXIS_Y) ? (size_t)d.nx : 1);  // trend per slab, or per column
    P->mom_chunks = (int)std::max<long long>(1, std::min<long long>(d.ny, (2048 + G - 1) / G));
    P->off_acc = off; off = al(off + (size_t)G * P->mom_chunks * 6 * sizeof(double) * nf);  // per-chunk partial sums of ONE group of slabs
    P->off_coef = off; off = al(off + ncoef * 6 * sizeof(double) * nf);
    bool need_w = d.ndim == 2 || fast, need_w2 = false;
    for (const Pass& p : P->passes) { if (p.out_kind == B_W2) need_w2 = true; if (p.out_kind == B_W) need_w = true; }
    P->off_w = off; if (need_w) off = al(off + (size_t)G * slab_w * (fast ? nf : 1));  // (y first: field 1's intermediate follows field 0's)
    P->off_w2 = off; if (need_w2) off = al(off + (size_t)G * d.ny * d.nx * P->csize);
    P->off_f0 = off; if (nf == 2 && !fast) off = al(off + (size_t)G * slab_w);
    const size_t nfit = (size_t)(fast ? 2 * P->ynx : d.ny);  // per-column sums + subtracted lines
    P->off_rowfit = off; if (fast) off = al(off + (size_t)G * nfit * 2 * sizeof(double) * nf);
    P->off_corr = off; if (fast) off = al(off + (size_t)G * nfit * 2 * sizeof(float) * nf);  // (16 bytes per column: fasty uses 8, fastm's float64 pairs all 16)
    P->p1_w = fast ? (size_t)G * slab_w : 0; P->p1_fit = fast ? (size_t)G * nfit * 2 * sizeof(double) : 0; P->p1_corr = fast ? (size_t)G * nfit * 2 * sizeof(float) : 0;  // (one field's share of the three)
    P->off_isopart = off;
    if (fast && !fastm_pipeline(P) && (d.flags & XRFTHIP_ISO)) {  // per-workgroup partial radial sums of one group of slabs (reduced in order)
        const bool two = d.out_mode == XRFTHIP_OUT_CROSS;
        const long long gx = fasty_rows_gx(P);  // YRows<NX>::GX
        const size_t upr = (size_t)P->y_nrow_pad / (two ? gx : 2 * gx);
        off = al(off + (size_t)G * upr * P->nbins * (two ? 2 : 1) * sizeof(double));
    }
    P->off_isotmp = off;
    if (fastm_iso_fused(P)) {  // fastm with the radial sums inside pass 2: one partial table per row workgroup
        const bool two = d.out_mode == XRFTHIP_OUT_CROSS;
        P->off_isopart = off;
        off = al(off + (size_t)G * (P->y_nrow_pad / fastm_rows_rpu(P)) * P->nbins * (two ? 2 : 1) * sizeof(double));
    } else if ((!fast || fastm_pipeline(P)) && (d.flags & XRFTHIP_ISO)) {  // generic and fastm kernels: the spectrum is stored (into the caller's array, or here), then summed
        const bool two = d.out_mode == XRFTHIP_OUT_CROSS;
        const size_t out_esz = two ? P->csize : P->rsize;
        const long long total = d.ny * P->nx_out;
        P->iso_chunks = iso_chunk_count(total);
        if (d.flags & XRFTHIP_NO_SPECTRUM_OUT) off = al(off + (size_t)G * total * out_esz);
        P->off_isopart = off;
        off = al(off + (size_t)G * P->iso_chunks * std::max(P->nbins, 1) * (two ? 2 : 1) * sizeof(double));
    }
    if (mean_plan(P) && P->family == Family::FastY) off = mean_layout(P, off, (long long)P->y_nrow_pad / (nf == 2 ? fasty_rows_gx(P) : 2 * fasty_rows_gx(P)), G);
    P->ws_bytes = off;
}

// A mean plan's runs per output and its partial sums (fasty_mean.h): P->mean_P is chosen only so that the launch fills the card -- `units` workgroups per slab,
// `slabs` slabs per launch, of which min(slabs, M) belong to one output -- and every run has a float64 (complex128) half spectrum of its own behind `off`.
size_t mean_layout(xrfthip_plan* P, size_t off, long long units, long long slabs) {
    const xrfthip_desc& d = P->d;
    const long long M = d.mean_batch, per_launch = std::max<long long>(1, slabs / M), cap = std::max<long long>(1, std::min(slabs, M));
    // (... and at most ny / 4 runs: the partials stay within (P + 1) results, a float64 half spectrum being one result and two rows).  XRFTHIP_MEAN_RUNS pins P
    // (1 .. min(slabs, M)) for measurements: long runs at 1, more workgroups than the rule gives above it
    // (a Welch plan, ny = 1: at most M / 2 runs -- a run holds a pair of segments at least; its partial is one spectrum of L values)
    const long long most = welch_plan(P) ? std::max<long long>(1, M / 2) : d.ny / 4;
    P->mean_P = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(cap, most), (4LL * kCUs) / std::max<long long>(1, units * per_launch)));
    if (P->tune_mean_runs > 0) P->mean_P = (int)std::min<long long>(cap, P->tune_mean_runs);
    P->mean_run = (cap + P->mean_P - 1) / P->mean_P;
    P->off_mean = off;
    // (doubles per sample: a power 1, a cross spectrum 2, a coherence 4 -- re C, im C, A, B)
    const size_t cols = welch_cols(P) ? (size_t)d.inner : 1;  // (the column layout of a Welch plan: every column an output)
    const size_t bytes = (size_t)(d.batch / M) * cols * (size_t)P->mean_P * (size_t)(d.ny / 2 + 1) * (size_t)d.nx * sizeof(double) * (P->coherence ? 4 : d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1);
    return (off + bytes + 255) & ~(size_t)255;
}

// ... and the pass that ends a mean plan's exec: the runs of every output summed in order, x 1 / M, every output row written once (mean_finish_kernel)
int run_mean_finish(const xrfthip_plan* P, const double* part, void* out, hipStream_t st) {
    const xrfthip_desc& d = P->d;
    const long long nout = d.batch / d.mean_batch;
    if (nout * d.ny > 0x7fffffffLL) return XRFTHIP_BAD_ARG;
    xrfthip_plan::ProfRec* rec = prof_begin(P, "mean_finish", st);
    const dim3 grid((unsigned)(nout * d.ny)), blk(256);
    const int sy = (d.flags & XRFTHIP_SHIFT_Y) ? (int)(d.ny / 2) : 0, sx = (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0;
    const double inv_m = 1.0 / (double)d.mean_batch;
    const cf *phy = reinterpret_cast<const cf*>(P->fph[0].p), *phx = reinterpret_cast<const cf*>(P->fph[1].p);
    if (P->coherence) { auto k = &mean_finish_coherence_kernel; XRFT_LAUNCH(k, grid, blk, 0, st, part, reinterpret_cast<float*>(out), (int)d.ny, (int)d.nx, P->mean_P, sy, sx); }  // (1 / M and the phase factors cancel)
    else if (d.out_mode == XRFTHIP_OUT_CROSS) { auto k = &mean_finish_kernel<true>; XRFT_LAUNCH(k, grid, blk, 0, st, part, out, (int)d.ny, (int)d.nx, P->mean_P, inv_m, sy, sx, phy, phx, (P->fph_on && phy && phx) ? 1 : 0); }
    else { auto k = &mean_finish_kernel<false>; XRFT_LAUNCH(k, grid, blk, 0, st, part, out, (int)d.ny, (int)d.nx, P->mean_P, inv_m, sy, sx, phy, phx, 0); }
    prof_end(rec, st);
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

xrfthip_plan::ProfRec* prof_begin(const xrfthip_plan* P, const std::string& label, hipStream_t st) {
    if (!P->prof || P->prof_recs.size() + 1 >= P->prof_recs.capacity()) return nullptr;
    xrfthip_plan* M = const_cast<xrfthip_plan*>(P);
    xrfthip_plan::ProfRec r;
    r.label = label;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return nullptr;
    (void)hipEventRecord(r.a, st);
    M->prof_recs.push_back(r);
    return &M->prof_recs.back();
}
void prof_end(xrfthip_plan::ProfRec* r, hipStream_t st) {
    if (r) (void)hipEventRecord(r->b, st);
}

template <typename T>
static int run_moments(const xrfthip_plan* P, const void* in, long long g0, long long gc, double* acc, double* coef, hipStream_t st) {
    const xrfthip_desc& d = P->d;
    const long long total = d.ny * d.nx;
    const long long chunks = P->mom_chunks;
    const size_t esz = P->cplx_in ? P->csize : P->rsize;
    if (d.flags & XRFTHIP_AXIS_Y) {  // one line (or mean) per column, straight into the coefficient table
        xrfthip_plan::ProfRec* recc = prof_begin(P, "column_fit", st);
        for (long long b0 = 0; b0 < gc; b0 += 32768) {
            const long long bc = std::min<long long>(32768, gc - b0);
            const dim3 grid((unsigned)((d.nx + 63) / 64), (unsigned)bc), block(256);  // (64 columns x 4 row parts per workgroup)
            const void* src = (const char*)in + (size_t)(g0 + b0) * total * esz;
            double* cdst = coef + (g0 + b0) * d.nx * 6;
            if (P->cplx_in) { auto k = &column_fit_kernel<T, true>; XRFT_LAUNCH(k, grid, block, 4 * 4 * 64 * sizeof(double), st, src, (long long)d.ny, (long long)d.nx, cdst, (int)d.detrend); }
            else { auto k = &column_fit_kernel<T, false>; XRFT_LAUNCH(k, grid, block, 4 * 4 * 64 * sizeof(double), st, src, (long long)d.ny, (long long)d.nx, cdst, (int)d.detrend); }
        }
        prof_end(recc, st);
        HIP_TRY(hipGetLastError());
        return XRFTHIP_OK;
    }
    const size_t lds = 6 * 256 * sizeof(double);
    xrfthip_plan::ProfRec* rec = prof_begin(P, "moments", st);
    for (long long b0 = 0; b0 < gc; b0 += 32768) {  // grid.y is limited to 65535 blocks
        const long long bc = std::min<long long>(32768, gc - b0);
        const dim3 grid((unsigned)chunks, (unsigned)bc), block(256);
        const void* src = (const char*)in + (size_t)(g0 + b0) * total * esz;
        if (P->cplx_in) { auto k = &slab_moments_kernel<T, true>; XRFT_LAUNCH(k, grid, block, lds, st, src, (long long)d.ny, (long long)d.nx, total, (long long)d.nx, acc + b0 * chunks * 6); }
        else { auto k = &slab_moments_kernel<T, false>; XRFT_LAUNCH(k, grid, block, lds, st, src, (long long)d.ny, (long long)d.nx, total, (long long)d.nx, acc + b0 * chunks * 6); }
    }
    prof_end(rec, st);
    rec = prof_begin(P, "finalize_coef", st);
    auto kf = &finalize_coef_kernel;
    XRFT_LAUNCH(kf, dim3((unsigned)gc), dim3(64), 0, st, (const double*)acc, coef + g0 * 6, gc, (long long)d.ny, (long long)d.nx, (int)d.detrend, (int)chunks);
    prof_end(rec, st);
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}


// Everything xrfthip_exec needs beyond the caller's buffers is built HERE, when the plan is created or one of its tables is
// set: window spectra and phase tables of the specialised paths (device allocations + blocking copies) and the workspace
// layout.  xrfthip_exec itself takes the plan as const: no allocation, no copy, no synchronisation, no getenv.
static int finalize_plan(xrfthip_plan* P) {
    const auto finalize = family_ops(P->chosen).finalize;
    const int rc = finalize ? finalize(P) : XRFTHIP_OK;
    if (rc) return rc;
    settle_family(P);
    // a strided plan runs the family the dense descriptor gets, or none: never a slower family because of the strides (the caller copies)
    if (in_strided(P) && !family_reads_strided(P)) return XRFTHIP_UNSUPPORTED_LENGTH;
    // ... and a half plan a family that reads 2-byte samples, or none (the caller widens): no other kernel may ever see the 2-byte buffer
    if (in_half(P) && !half_family(P)) return XRFTHIP_UNSUPPORTED_LENGTH;
    // ... and a mean plan a family with a mean form, or none (the caller composes: the plain plan, then xrfthip_reduce_axis)
    if (mean_plan(P) && !mean_family(P)) return XRFTHIP_UNSUPPORTED_LENGTH;
    if (const auto layout = family_ops(P->family).layout) layout(P);
    return XRFTHIP_OK;
}

template <typename T>
static int run_pipeline(const xrfthip_plan* P, const std::vector<Pass>& passes, const void* in, void* out, double* iso,
                        char* ws, const double* coef, long long g0, long long gc, hipStream_t st) {
    const xrfthip_desc& d = P->d;
    const size_t in_esz = P->cplx_in ? P->csize : P->rsize;
    const void* iso_src = nullptr;
    for (const Pass& p0 : passes) {
        Pass p = p0;
        p.g.n_outer = p.outer_per_slab * gc;
        p.g.n_tiles = p.g.tile_axis == 0 ? (p.g.n_outer + p.g.T - 1) / p.g.T : p.g.n_outer * p.g.tiles_per_outer;
        auto buf = [&](int kind) -> void* {
            switch (kind) {
                case B_W: return ws + P->off_w;
                case B_W2: return ws + P->off_w2;
                case B_F0: return ws + P->off_f0;
                default: return nullptr;
            }
        };
        if (p.first) {
            p.pr.in = (const char*)in + (size_t)g0 * d.ny * ((d.flags & XRFTHIP_C2R_X) ? d.nx / 2 + 1 : d.nx) * in_esz;
            p.pr.win_y = P->win[0].p;
            p.pr.win_x = P->win[1].p;
            p.pr.coef = coef ? coef + g0 * ((d.flags & XRFTHIP_AXIS_Y) ? d.nx : 1) * 6 : nullptr;
            if (!coef) p.pr.detrend = 0;
            if (d.flags & XRFTHIP_PHASE_IN) { p.pr.ph_y = P->phase[0].p; p.pr.ph_x = P->phase[1].p; }
        } else {
            p.g.in = buf(p.in_kind);
        }
        if (p.final_) {
            if (p.out_kind == B_F0) {
                p.ep.out = buf(B_F0);
            } else {
                const size_t out_esz = (d.out_mode == XRFTHIP_OUT_POWER || d.out_mode == XRFTHIP_OUT_PHASE || (d.flags & XRFTHIP_C2R_X)) ? P->rsize : P->csize;
                p.ep.out = out ? (char*)out + (size_t)g0 * d.ny * P->nx_out * out_esz : nullptr;
                if ((d.flags & XRFTHIP_ISO) && iso && !out) p.ep.out = ws + P->off_isotmp;  // isotropic spectra: the full spectrum of this group lives in the workspace
                iso_src = p.ep.out;
                if (!(d.flags & XRFTHIP_PHASE_IN)) { p.ep.ph_y = P->phase[0].p; p.ep.ph_x = P->phase[1].p; }
                p.ep.other = (d.out_mode == XRFTHIP_OUT_CROSS || d.out_mode == XRFTHIP_OUT_PHASE) ? buf(B_F0) : nullptr;
            }
        } else {
            p.g.out = buf(p.out_kind);
        }
        if (p.g.n_tiles <= 0) continue;
        const int grid = (int)std::min<long long>(p.g.n_tiles, P->tune_max_grid);
        xrfthip_plan::ProfRec* rec = prof_begin(P, p.label, st);
        launch_tile<T>(p, grid, st);
        prof_end(rec, st);
        HIP_TRY(hipGetLastError());
    }
    if ((d.flags & XRFTHIP_ISO) && iso && iso_src) {  // radial sums of the stored spectrum (xrft.py:895-906), bit-reproducible
        const bool two = d.out_mode == XRFTHIP_OUT_CROSS;
        const int32_t sdt = two ? (P->dbl ? XRFTHIP_C128 : XRFTHIP_C64) : (P->dbl ? XRFTHIP_F64 : XRFTHIP_F32);
        xrfthip_plan::ProfRec* rec = prof_begin(P, "radial_sums", st);
        const int rc = run_radial_sums(sdt, iso_src, (const int32_t*)P->binmap.p, gc, d.ny, P->nx_out, (d.flags & XRFTHIP_SHIFT_Y) ? (int)(d.ny / 2) : 0,
                                       (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0, P->nbins, P->iso_chunks, reinterpret_cast<double*>(ws + P->off_isopart),
                                       iso + (size_t)g0 * P->nbins * (two ? 2 : 1), st);
        prof_end(rec, st);
        if (rc) return rc;
    }
    return XRFTHIP_OK;
}

// ---------------------------------------------------------------- Generic: the tile passes' row, and the table of rows
static int run_generic(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d = P->d;
    hipStream_t st = a.stream;
    const bool cross = d.out_mode == XRFTHIP_OUT_CROSS || d.out_mode == XRFTHIP_OUT_PHASE;
    const bool det = d.detrend != XRFTHIP_DETREND_NONE;
    double* acc = (double*)(a.ws + P->off_acc);
    double* coef = (double*)(a.ws + P->off_coef);
    for (long long g0 = 0; g0 < d.batch; g0 += P->G) {
        const long long gc = std::min<long long>(P->G, d.batch - g0);
        int rc;
        if (cross) {
            if (det) {
                rc = P->dbl ? run_moments<double>(P, a.in0, g0, gc, acc, coef, st) : run_moments<float>(P, a.in0, g0, gc, acc, coef, st);
                if (rc) return rc;
            }
            rc = P->dbl ? run_pipeline<double>(P, P->passes_f0, a.in0, nullptr, nullptr, a.ws, det ? coef : nullptr, g0, gc, st)
                        : run_pipeline<float>(P, P->passes_f0, a.in0, nullptr, nullptr, a.ws, det ? coef : nullptr, g0, gc, st);
            if (rc) return rc;
        }
        const void* in_main = cross ? a.in1 : a.in0;
        double* acc_m = cross ? acc + (size_t)P->G * P->mom_chunks * 6 : acc;
        double* coef_m = cross ? coef + d.batch * ((d.flags & XRFTHIP_AXIS_Y) ? d.nx : 1) * 6 : coef;
        if (det) {
            rc = P->dbl ? run_moments<double>(P, in_main, g0, gc, acc_m, coef_m, st) : run_moments<float>(P, in_main, g0, gc, acc_m, coef_m, st);
            if (rc) return rc;
        }
        rc = P->dbl ? run_pipeline<double>(P, P->passes, in_main, a.out, a.iso, a.ws, det ? coef_m : nullptr, g0, gc, st)
                    : run_pipeline<float>(P, P->passes, in_main, a.out, a.iso, a.ws, det ? coef_m : nullptr, g0, gc, st);
        if (rc) return rc;
    }
    return XRFTHIP_OK;
}
static bool generic_uses_bluestein(const xrfthip_plan* P) {
    for (const Pass& ps : P->passes) if (ps.g.blue_n > 0) return true;
    for (const Pass& ps : P->passes_f0) if (ps.g.blue_n > 0) return true;
    return false;
}
static void generic_info(const xrfthip_plan*, int32_t* kind, int32_t* n) { *kind = XRFTHIP_K_GENERIC; *n = 0; }
// (describe: the header and the passes' lines that xrfthip_plan_describe prints for every plan with tile passes)
static const FamilyOps kOpsGeneric = {Family::Generic, run_generic, nullptr, generic_info, nullptr, layout_passes, nullptr, generic_uses_bluestein};

const FamilyOps& family_ops(Family f) {
    static const FamilyOps* const kRows[] = {  // in the order of enum class Family
        &kOpsGeneric, &kOpsComposite, &kOpsFusedInner, &kOpsFastS, &kOpsFastG, &kOpsFastGY, &kOpsFastMX, &kOpsFastMY, &kOpsFastR, &kOpsFastRComplex, &kOpsFastRRows,
        &kOpsFastW, &kOpsFastK, &kOpsFastYC, &kOpsFastYCFourStep, &kOpsFastY, &kOpsFastY1D, &kOpsFastM, &kOpsFastN, &kOpsFastH};
    static_assert(sizeof kRows / sizeof kRows[0] == kFamilyCount, "one row of FamilyOps per Family");
    return *kRows[(int)f];
}

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

int xrfthip_version(void) { return XRFTHIP_VERSION; }

const char* xrfthip_strerror(int status) {
    switch (status) {
        case XRFTHIP_OK: return "ok";
        case XRFTHIP_BAD_ARG: return "bad argument";
        case XRFTHIP_UNSUPPORTED_LENGTH: return "unsupported transform length (prime factor > 128 or does not fit LDS)";
        case XRFTHIP_WORKSPACE_TOO_SMALL: return "workspace too small";
        case XRFTHIP_HIP_ERROR: return "HIP runtime error (see xrfthip_last_hip_error)";
        case XRFTHIP_ALLOC_FAILED: return "device allocation failed";
        case XRFTHIP_MISSING_TABLE: return "a required table (window / phase / bin map) was not set";
        default: return "unknown status";
    }
}

int xrfthip_last_hip_error(void) { return g_last_hip_error; }


int xrfthip_plan_create(xrfthip_plan** plan, const xrfthip_desc* desc) {
    // (a descriptor of the version before `inner` was appended is accepted: inner = 1)
    // (... and of the versions before `mid` and before the input strides: mid = 1, strides 0)
    // (... and of the version before herm_ny / herm_nx: 0, 0)
    // (... and before each later group of fields, which then read 0: mean_batch; seg_hop / seg_reserved; seg_stride / seg_reserved2; seg_keep / seg_reserved3; seg_synth / seg_reserved4; seg_filter / seg_lead /
    // seg_in_len / seg_out_len; seg_tapers / seg_taper_len; seg_filter_cols / seg_reserved5 -- each group came together, no size between)
    static const uint32_t kDescSizes[] = {
        (uint32_t)sizeof(xrfthip_desc), (uint32_t)offsetof(xrfthip_desc, inner), (uint32_t)offsetof(xrfthip_desc, mid), (uint32_t)offsetof(xrfthip_desc, in_stride_y),
        (uint32_t)offsetof(xrfthip_desc, herm_ny), (uint32_t)offsetof(xrfthip_desc, mean_batch), (uint32_t)offsetof(xrfthip_desc, seg_hop), (uint32_t)offsetof(xrfthip_desc, seg_stride),
        (uint32_t)offsetof(xrfthip_desc, seg_keep), (uint32_t)offsetof(xrfthip_desc, seg_synth), (uint32_t)offsetof(xrfthip_desc, seg_filter), (uint32_t)offsetof(xrfthip_desc, seg_tapers),
        (uint32_t)offsetof(xrfthip_desc, seg_filter_cols)};
    if (!plan || !desc || std::find(std::begin(kDescSizes), std::end(kDescSizes), desc->struct_size) == std::end(kDescSizes)) return XRFTHIP_BAD_ARG;
    xrfthip_desc dcopy{};
    memcpy(&dcopy, desc, desc->struct_size);
    dcopy.struct_size = sizeof(xrfthip_desc);
    if (dcopy.inner < 0 || dcopy.mid < 0) return XRFTHIP_BAD_ARG;
    if (dcopy.inner == 0) dcopy.inner = 1;
    if (dcopy.mid == 0) dcopy.mid = 1;
    if (dcopy.in_stride_y < 0 || dcopy.in_stride_batch < 0) return XRFTHIP_BAD_ARG;
    if (dcopy.mean_batch < 0) return XRFTHIP_BAD_ARG;
    // seg_hop / seg_stride / seg_keep / seg_synth / seg_filter: the segments of a series (host_welch.inc).  With seg_keep, seg_synth or seg_filter, mean_batch is the
    // segments per series, 1 included, and nothing is averaged
    long long w_pitch = 0;
    if (seg_desc_check(dcopy, &w_pitch)) return XRFTHIP_BAD_ARG;
    const bool keep = dcopy.seg_keep == 1 || dcopy.seg_synth == 1 || dcopy.seg_filter == 1;
    if (dcopy.mean_batch == 1 && !keep) dcopy.mean_batch = 0;  // (the plain plan itself)
    {   // strides that say what a dense array says are the dense plan (any family serves it)
        const int64_t row = (dcopy.flags & XRFTHIP_C2R_X) ? dcopy.nx / 2 + 1 : dcopy.nx;
        if (dcopy.in_stride_y > 0 && dcopy.in_stride_y < row) return XRFTHIP_BAD_ARG;
        if (dcopy.in_stride_y == row) dcopy.in_stride_y = 0;
        if (dcopy.ndim == 1) dcopy.in_stride_y = 0;  // (one row per slab: nothing to stride over)
        if (dcopy.in_stride_y == 0 && dcopy.in_stride_batch == dcopy.ny * row) dcopy.in_stride_batch = 0;
    }
    // float16 / bfloat16 input: the float32 plan of the same descriptor, its input pass reading 2-byte samples (half_in.h).  From here on the descriptor says XRFTHIP_F32
    // -- every check, every table, the family and the workspace are the float32 plan's -- and in16 remembers what the input holds.
    const int in16 = dcopy.dtype == XRFTHIP_F16 ? 1 : dcopy.dtype == XRFTHIP_BF16 ? 2 : 0;
    if (in16) dcopy.dtype = XRFTHIP_F32;
    const xrfthip_desc& d = dcopy;
    if (d.ndim != 1 && d.ndim != 2) return XRFTHIP_BAD_ARG;
    if (d.batch < 0 || d.nx < 1 || d.ny < 1 || (d.ndim == 1 && d.ny != 1)) return XRFTHIP_BAD_ARG;
    if (d.nx > (1LL << 30) || d.ny > (1LL << 30) || d.nx * d.ny > (1LL << 31) - 1) return XRFTHIP_BAD_ARG;  // per-element index math is 32-bit
    if (d.dtype < XRFTHIP_F32 || d.dtype > XRFTHIP_C128) return XRFTHIP_BAD_ARG;
    if (dcopy.out_mode < XRFTHIP_OUT_COMPLEX || dcopy.out_mode > XRFTHIP_OUT_COHERENCE) return XRFTHIP_BAD_ARG;
    // XRFTHIP_OUT_COHERENCE: |<F0 conj F1>|^2 / (<|F0|^2> <|F1|^2>) over every mean_batch slabs.  It exists only as a mean plan (of one spectrum it is 1 everywhere, and
    // M = 1 was normalised to the plain plan above).  From here on the descriptor says XRFTHIP_OUT_CROSS -- every check, every table, the family, the workspace in front of
    // the partial sums and the column pass are the CROSS mean plan's -- and `coherence` remembers what the row pass sums; it is served by FastY's two passes only (finalize_plan)
    const bool coherence = dcopy.out_mode == XRFTHIP_OUT_COHERENCE;
    if (coherence) {
        if (dcopy.mean_batch <= 1) return XRFTHIP_BAD_ARG;
        dcopy.out_mode = XRFTHIP_OUT_CROSS;
    }
    if ((d.flags & (XRFTHIP_INVERSE | XRFTHIP_C2R_X | XRFTHIP_PHASE_IN)) && (d.dtype < XRFTHIP_C64 || d.out_mode != XRFTHIP_OUT_COMPLEX || d.detrend)) return XRFTHIP_BAD_ARG;
    if ((d.flags & XRFTHIP_C2R_X) && (!(d.flags & XRFTHIP_INVERSE) || (d.nx & 1) || (d.flags & (XRFTHIP_ISHIFT_X | XRFTHIP_FLIP_X)))) return XRFTHIP_BAD_ARG;
    if (d.detrend < XRFTHIP_DETREND_NONE || d.detrend > XRFTHIP_DETREND_LINEAR) return XRFTHIP_BAD_ARG;
    const bool cplx_in = d.dtype >= XRFTHIP_C64;
    if ((d.flags & XRFTHIP_HALF_X) && cplx_in) return XRFTHIP_BAD_ARG;
    if ((d.flags & XRFTHIP_HALF_X) && (d.flags & (XRFTHIP_SHIFT_X | XRFTHIP_SHIFT_Y))) return XRFTHIP_BAD_ARG;  // xrft.py:403
    if ((d.flags & XRFTHIP_HALF_Y) && (cplx_in || !(d.inner > 1 || d.mid > 1) || (d.flags & (XRFTHIP_HALF_X | XRFTHIP_SHIFT_X | XRFTHIP_SHIFT_Y | XRFTHIP_AXIS_Y)))) return XRFTHIP_BAD_ARG;
    if ((d.flags & XRFTHIP_REALDIM_X2) && (!(d.flags & (XRFTHIP_HALF_X | XRFTHIP_HALF_Y)) || d.out_mode == XRFTHIP_OUT_COMPLEX)) return XRFTHIP_BAD_ARG;
    if ((d.flags & XRFTHIP_ISO) && (d.ndim != 2 || d.out_mode == XRFTHIP_OUT_COMPLEX)) return XRFTHIP_BAD_ARG;
    if ((d.flags & XRFTHIP_NO_SPECTRUM_OUT) && !(d.flags & XRFTHIP_ISO)) return XRFTHIP_BAD_ARG;
    if (d.ndim == 1 && (d.flags & (XRFTHIP_SHIFT_Y | XRFTHIP_ISHIFT_Y | XRFTHIP_FLIP_Y))) return XRFTHIP_BAD_ARG;
    if ((d.flags & (XRFTHIP_FLIP0_Y | XRFTHIP_FLIP0_X)) && d.out_mode != XRFTHIP_OUT_CROSS && d.out_mode != XRFTHIP_OUT_PHASE) return XRFTHIP_BAD_ARG;
    if ((d.flags & XRFTHIP_FLIP0_Y) && d.ndim == 1) return XRFTHIP_BAD_ARG;
    // herm_ny / herm_nx: the columns of an AXIS_Y plan are the half spectrum of a real herm_ny x herm_nx grid (the last pass of a three-axis spectrum, fasth.h)
    const bool herm = d.herm_ny != 0 || d.herm_nx != 0, field = (d.flags & XRFTHIP_HERM_FIELD) != 0;  // (field: the last pass writes F itself)
    if (field && !herm) return XRFTHIP_BAD_ARG;
    if (herm) {
        if (d.herm_ny < 1 || d.herm_nx < 1 || d.herm_nx > (1LL << 30) || d.herm_ny > (1LL << 30)) return XRFTHIP_BAD_ARG;
        if (!(d.flags & XRFTHIP_AXIS_Y) || (d.flags & ~(XRFTHIP_AXIS_Y | XRFTHIP_SHIFT_Y | XRFTHIP_ISHIFT_Y | XRFTHIP_SHIFT_X | XRFTHIP_HERM_FIELD))) return XRFTHIP_BAD_ARG;
        const bool mode_ok = field ? d.out_mode == XRFTHIP_OUT_COMPLEX : (d.out_mode == XRFTHIP_OUT_POWER || d.out_mode == XRFTHIP_OUT_CROSS);
        if (d.ndim != 2 || !cplx_in || !mode_ok || d.detrend) return XRFTHIP_BAD_ARG;
        if (d.nx != d.herm_ny * (d.herm_nx / 2 + 1) || d.inner > 1 || d.mid > 1 || d.in_stride_y || d.in_stride_batch) return XRFTHIP_BAD_ARG;
    }
    if ((d.flags & XRFTHIP_AXIS_Y) && (d.ndim != 2 || (d.flags & XRFTHIP_FLIP0_X) || (d.flags & ((herm ? 0u : XRFTHIP_SHIFT_X) | XRFTHIP_ISHIFT_X | XRFTHIP_FLIP_X |
                                                                    XRFTHIP_ISO | XRFTHIP_NO_SPECTRUM_OUT | XRFTHIP_C2R_X)))) return XRFTHIP_BAD_ARG;  // (PHASE_IN: only where fastgy takes the plan, below)
    // AXIS_Y with HALF_X / REALDIM_X2 (ABI 0.1.4): real_dim along the ONE transformed axis -- ny / 2 + 1 rows per slab, unshifted; the one-pass kernels only (below)
    if ((d.flags & XRFTHIP_AXIS_Y) && (d.flags & (XRFTHIP_HALF_X | XRFTHIP_REALDIM_X2)) &&
        (cplx_in || !(d.flags & XRFTHIP_HALF_X) || (d.flags & (XRFTHIP_SHIFT_Y | XRFTHIP_FLIP_Y | XRFTHIP_INVERSE)))) return XRFTHIP_BAD_ARG;

    // mean_batch = M > 1: the mean over every M consecutive slabs inside the last pass (fasty_mean.h, fasts_mean.h); what has no mean form is "the caller composes"
    if (d.mean_batch > 1 && !keep) {
        if (d.batch % d.mean_batch != 0 || (d.out_mode != XRFTHIP_OUT_POWER && d.out_mode != XRFTHIP_OUT_CROSS) || (d.flags & XRFTHIP_ISO)) return XRFTHIP_BAD_ARG;
        if (!d.seg_hop && ((d.flags & (XRFTHIP_HALF_X | XRFTHIP_REALDIM_X2 | XRFTHIP_AXIS_Y)) || d.inner > 1 || d.mid > 1 || herm)) return XRFTHIP_UNSUPPORTED_LENGTH;  // (a Welch plan has its own half output)
        if ((d.batch / d.mean_batch) * d.ny > 0x7fffffffLL) return XRFTHIP_UNSUPPORTED_LENGTH;  // (mean_finish_kernel: one workgroup per output row, run_mean_finish; refused before anything runs)
    }
    const bool strided = d.in_stride_y != 0 || d.in_stride_batch != 0;
    if (strided && (d.inner > 1 || d.mid > 1 || (d.flags & XRFTHIP_AXIS_Y))) return XRFTHIP_BAD_ARG;  // (those layouts stay dense)
    if (strided) {  // "the caller copies": the in-slab index math is 32-bit (elements, and bytes as unsigned); every vector load stays one aligned instruction
        const int64_t esz = (d.dtype == XRFTHIP_F32 ? 4 : d.dtype == XRFTHIP_C128 ? 16 : 8);
        const int64_t pitch = d.in_stride_y ? d.in_stride_y : d.nx;
        if (pitch > ((1LL << 31) - 1) / d.ny || d.ny * pitch * esz > (1LL << 32) - 1) return XRFTHIP_UNSUPPORTED_LENGTH;
        if ((d.in_stride_y * esz) % 16 != 0 || (d.in_stride_batch * esz) % 16 != 0) return XRFTHIP_UNSUPPORTED_LENGTH;
    }

    // half input is read dense, by the trailing-axes families that half_family() names: everything else is "the caller widens" (xrfthip_convert, then the float32 plan)
    if (in16 && (strided || d.inner > 1 || d.mid > 1 || d.seg_stride || (d.flags & XRFTHIP_AXIS_Y))) return XRFTHIP_UNSUPPORTED_LENGTH;
    if ((d.inner > 1 && !d.seg_stride) || d.mid > 1) return create_inner_plan(plan, d);  // (inner with seg_stride: the columns of a Welch plan, fastw.h)

    xrfthip_plan* P = new (std::nothrow) xrfthip_plan();
    if (!P) return XRFTHIP_ALLOC_FAILED;
    P->d = d;
    P->tune_group = env_ll("XRFTHIP_GROUP", 0);
    P->tune_fast_group = env_ll("XRFTHIP_FAST_GROUP", 0);
    P->tune_mean_runs = env_ll("XRFTHIP_MEAN_RUNS", 0);
    P->tune_group_bytes = env_ll("XRFTHIP_GROUP_BYTES", 512LL << 20);
    P->tune_cols_grid = env_ll("XRFTHIP_FAST_COLS_GRID", kCUs);
    P->tune_max_grid = env_ll("XRFTHIP_MAX_GRID", 8 * kCUs * 4);
    P->cplx_in = cplx_in;
    P->in16 = in16;
    P->coherence = coherence;
    P->w_pitch = w_pitch;
    P->dbl = d.dtype == XRFTHIP_F64 || d.dtype == XRFTHIP_C128;
    P->rsize = P->dbl ? 8 : 4;
    P->csize = 2 * P->rsize;
    P->nxh = cplx_in ? d.nx : d.nx / 2 + 1;
    P->nx_out = ((d.flags & XRFTHIP_HALF_X) && !(d.flags & XRFTHIP_AXIS_Y)) ? d.nx / 2 + 1 : d.nx;  // (AXIS_Y: the half is along y)
    if (herm) P->nx_out = d.herm_ny * d.herm_nx;  // (the full grid behind every row along t)
    // width of the intermediate: the half spectrum for real input, unless the row does not fit one LDS tile
    // (four-step along x computes every kx) -- decided inside build_x through P->width.
    P->width = P->nxh;
    if (d.flags & XRFTHIP_AXIS_Y) P->width = d.nx;  // x is not transformed: every column is its own sequence
    else if (!cplx_in) {
        const long long n_try = (d.nx % 2 == 0 && d.nx >= 2) ? d.nx / 2 : d.nx;
        TileChoice c = choose_tile(n_try, P->csize, false, 1LL << 40, 0);
        if (c.T == 0 || n_try >= env_ll("XRFTHIP_X_FOURSTEP_MIN", 1LL << 40)) P->width = d.nx;
    }
    P->mirror = !cplx_in && !(d.flags & (XRFTHIP_HALF_X | XRFTHIP_AXIS_Y)) && P->width == d.nx / 2 + 1 && d.nx > 1;
    // the families in order of precedence: the first whose try_* does not decline serves the plan (its tables built); none: the generic passes
    static int (*const kTry[])(xrfthip_plan*) = {try_fastw, try_fasth, try_fasts, try_fastyc, try_fastr, try_fasty, try_fast1d, try_fastm, try_fastmx, try_fastmy, try_fastgy, try_fastg, try_fastn};
    int rc = kDeclined;
    if (!env_ll("XRFTHIP_NO_FAST", 0))
        for (auto try_family : kTry)
            if ((rc = try_family(P)) != kDeclined) break;
    if (rc == kDeclined) rc = XRFTHIP_OK;
    if (!rc && herm && P->family != Family::FastH) rc = XRFTHIP_UNSUPPORTED_LENGTH;  // (no other family reads a half spectrum as columns: the caller composes the stages)
    if (!rc && (d.seg_hop || d.seg_tapers) && P->family != Family::FastW && P->family != Family::FastK) rc = XRFTHIP_UNSUPPORTED_LENGTH;  // (no other family cuts segments out of a series: the caller composes)
    const bool one_axis = P->family == Family::FastGY || P->family == Family::FastMY;
    if (!rc && (d.flags & XRFTHIP_AXIS_Y) && (d.flags & XRFTHIP_PHASE_IN) && !one_axis) rc = XRFTHIP_BAD_ARG;  // (the generic column tiles have no input phase)
    if (!rc && (d.flags & XRFTHIP_AXIS_Y) && (d.flags & XRFTHIP_HALF_X) && !one_axis) rc = XRFTHIP_UNSUPPORTED_LENGTH;  // (... and no half output: the caller transposes)
    if (!rc) {
        set_kernel_attrs_once();
        // nbins must be known before tiles are sized (the LDS histogram shares the tile's allocation): ISO plans are
        // (re)built in xrfthip_plan_set_binmap.  Build now for everything else.
        if (!(d.flags & XRFTHIP_ISO) && !family_ops(P->family).no_generic_passes) rc = P->dbl ? build_plan_t<double>(*P) : build_plan_t<float>(*P);
    }
    if (!rc) rc = finalize_plan(P);
    if (rc) { delete P; return rc; }
    *plan = P;
    return XRFTHIP_OK;
}

int xrfthip_plan_destroy(xrfthip_plan* plan) {
    delete plan;
    return XRFTHIP_OK;
}

int xrfthip_plan_set_window(xrfthip_plan* plan, int axis, const double* h_window, int64_t n) {
    if (!plan || axis < 0 || axis > 1) return XRFTHIP_BAD_ARG;
    if (herm_plan(plan) && axis == 1) return XRFTHIP_BAD_ARG;  // (the two-axis stage that wrote the half spectrum windowed y and x)
    if (filter_plan(plan) && h_window) return XRFTHIP_BAD_ARG;  // (overlap-save takes no window: a windowed segment is not a linear filter's)
    if (plan && taper_plan(plan) && h_window) return XRFTHIP_BAD_ARG;  // (the tapers are the windows: xrfthip_plan_set_tapers)
    if (h_window && n != (axis == 0 ? plan->d.ny : plan->d.nx)) return XRFTHIP_BAD_ARG;
    if (plan->sub_x) return xrfthip_plan_set_window(axis == 0 ? plan->sub_y : plan->sub_x, (axis == 1 && plan->sub_x_1d) ? 1 : 0, h_window, n);  // (each one-axis plan transforms its "y"; a 1-D x stage its x)
    if (axis == 0) plan->host_win_y.assign(h_window ? h_window : nullptr, h_window ? h_window + n : nullptr);
    else plan->host_win_x.assign(h_window ? h_window : nullptr, h_window ? h_window + n : nullptr);
    int rc = upload_real_table(plan, plan->win[axis], h_window, n, 0);
    if (!rc) rc = finalize_plan(plan);
    return rc;
}

int xrfthip_plan_set_phase(xrfthip_plan* plan, int axis, const double* h_phase, int64_t n) {
    if (herm_field_plan(plan)) {  // the three output-phase tables of the field form: t, herm_ny, herm_nx (fasth.h carries the twins' own factors)
        if (axis < 0 || axis > 2) return XRFTHIP_BAD_ARG;
        const int64_t want3 = axis == 0 ? plan->d.ny : axis == 1 ? plan->d.herm_ny : plan->d.herm_nx;
        if (h_phase && n != want3) return XRFTHIP_BAD_ARG;
        plan->h_host_ph[axis].assign(h_phase ? h_phase : nullptr, h_phase ? h_phase + 2 * n : nullptr);
        return finalize_plan(plan);
    }
    if (!plan || axis < 0 || axis > 1 || herm_plan(plan)) return XRFTHIP_BAD_ARG;  // (herm: the twin of a sample at a Nyquist index does not carry the conjugate factor)
    if (synth_plan(plan) && h_phase) return XRFTHIP_BAD_ARG;  // (the synthesis has no phase: each segment's spectrum refers to its own first sample)
    if (filter_plan(plan)) {  // the filter's response: L / 2 + 1 entries on axis 1, kept as complex64 next to the plan's other tables (fastf.h reads phase[1])
        if (axis != 1 || (h_phase && n != plan->d.nx / 2 + 1)) return XRFTHIP_BAD_ARG;
        return upload_real_table(plan, plan->phase[1], h_phase, n, 1);
    }
    if (keep_plan(plan) && plan->d.out_mode == XRFTHIP_OUT_COMPLEX && h_phase) return XRFTHIP_UNSUPPORTED_LENGTH;  // (the "segments kept" form writes X itself: the caller composes)
    // an input phase of a c2r transform covers the stored half of the x axis only
    const int64_t want = axis == 0 ? plan->d.ny : ((plan->d.flags & XRFTHIP_C2R_X) ? plan->d.nx / 2 + 1 : plan->d.nx);
    if (h_phase && n != want) return XRFTHIP_BAD_ARG;
    if (plan->sub_x) return xrfthip_plan_set_phase(axis == 0 ? plan->sub_y : plan->sub_x, (axis == 1 && plan->sub_x_1d) ? 1 : 0, h_phase, n);
    plan->host_phase[axis].assign(h_phase ? h_phase : nullptr, h_phase ? h_phase + 2 * n : nullptr);
    int rc = upload_real_table(plan, plan->phase[axis], h_phase, n, 1);
    if (!rc) rc = finalize_plan(plan);  // (a non-trivial phase can take an isotropic cross spectrum off the specialised path: new layout)
    return rc;
}

// the taper table of a multitaper plan: [K][N] float32, weighted by the caller, kept beside the plan's other tables (fastt.h reads w_taps)
int xrfthip_plan_set_tapers(xrfthip_plan* plan, const float* h_tapers) {
    if (!plan || !taper_plan(plan)) return XRFTHIP_BAD_ARG;
    if (!h_tapers) { plan->w_taps.clear(); return XRFTHIP_OK; }
    return plan->w_taps.upload(h_tapers, (size_t)plan->d.seg_tapers * (size_t)plan->d.seg_taper_len * sizeof(float));
}

int xrfthip_plan_set_binmap(xrfthip_plan* plan, const int32_t* h_binmap, int64_t ny, int64_t nx_out, int32_t nbins) {
    if (!plan || !h_binmap || !(plan->d.flags & XRFTHIP_ISO)) return XRFTHIP_BAD_ARG;
    if (ny != plan->d.ny || nx_out != plan->nx_out || nbins < 1) return XRFTHIP_BAD_ARG;
    int rc = plan->binmap.upload(h_binmap, (size_t)ny * nx_out * sizeof(int32_t));
    if (rc) return rc;
    plan->nbins = nbins;
    const FamilyOps& ops = family_ops(plan->chosen);
    if (ops.binmap) rc = ops.binmap(plan, h_binmap);
    if (rc || ops.inner_layout) return rc;  // (FusedInner: no tile passes to rebuild)
    plan->passes.clear();
    plan->passes_f0.clear();
    int rcb = plan->dbl ? build_plan_t<double>(*plan) : build_plan_t<float>(*plan);
    if (!rcb) rcb = finalize_plan(plan);
    return rcb;
}

// The memory floor of the headline path, measured here and now (selftest.h): `reps` rounds of [pass-1 skeleton, pass-2 skeleton] over
// `nslab` 4096 x 4096 float32 slabs and `reps` plain copies of the same input, HIP events on `stream` around every launch.
// Synchronises (it is a measurement, not part of the hot path).  d_in: nslab x 4096 x 4096 float32; d_w2: nslab x 2052 x 4096 complex64
// (scratch); d_out: nslab x 4096 x 4096 float32 (overwritten).  us[0..2] = average microseconds PER SLAB of the copy, the column
// skeleton and the row skeleton.
int xrfthip_selftest_floor(const void* d_in, void* d_w2, void* d_out, int64_t nslab, int32_t reps, double* us, void* stream) {
    if (!d_in || !d_w2 || !d_out || !us || nslab < 1 || nslab > 4096 || reps < 1 || reps > 1000) return XRFTHIP_BAD_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    set_kernel_attrs_once();
    const size_t lds_c = ycols_geom(4096).lds, lds_r = yrows_geom(4096).lds;
    const int m = (int)kLdsMax;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&selftest_cols_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, m);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&selftest_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, m);
    hipEvent_t ev[4];
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    double acc[3] = {0.0, 0.0, 0.0};
    const size_t n16 = (size_t)nslab * 4096 * 4096 / 4;
    int rc = XRFTHIP_OK;
    for (int r = -1; r < reps && rc == XRFTHIP_OK; ++r) {  // (round -1: warm-up, not counted)
        auto kc = &selftest_copy_kernel;
        auto k1 = &selftest_cols_kernel;
        auto k2 = &selftest_rows_kernel;
        (void)hipEventRecord(ev[0], st);
        XRFT_LAUNCH(kc, dim3(2048), dim3(256), 0, st, reinterpret_cast<const F4*>(d_in), reinterpret_cast<F4*>(d_out), n16);
        (void)hipEventRecord(ev[1], st);
        XRFT_LAUNCH(k1, dim3((unsigned)(nslab * (4096 / SelfGeom::CW))), dim3(512), lds_c, st, reinterpret_cast<const float*>(d_in), reinterpret_cast<cf*>(d_w2), (int)nslab);
        (void)hipEventRecord(ev[2], st);
        XRFT_LAUNCH(k2, dim3((unsigned)(nslab * (SelfGeom::NROW_PAD / SelfGeom::RPU))), dim3(512), lds_r, st, reinterpret_cast<const cf*>(d_w2), reinterpret_cast<float*>(d_out), (int)nslab);
        (void)hipEventRecord(ev[3], st);
        if (hipEventSynchronize(ev[3]) != hipSuccess || hipGetLastError() != hipSuccess) { rc = XRFTHIP_HIP_ERROR; break; }
        if (r < 0) continue;
        for (int i = 0; i < 3; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            acc[i] += (double)ms;
        }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    for (int i = 0; i < 3; ++i) us[i] = acc[i] * 1e3 / ((double)reps * (double)nslab);
    return rc;
}

int xrfthip_plan_set_profiling(xrfthip_plan* plan, int enable) {
    if (!plan) return XRFTHIP_BAD_ARG;
    if (plan->sub_x) { const int rc = xrfthip_plan_set_profiling(plan->sub_x, enable); return rc ? rc : xrfthip_plan_set_profiling(plan->sub_y, enable); }
    plan->prof_clear();
    plan->prof_recs.reserve(1 << 16);  // prof_begin hands out pointers into this vector
    plan->prof = enable != 0;
    return XRFTHIP_OK;
}

int xrfthip_plan_profile_read(xrfthip_plan* plan, char* buf, size_t buflen) {
    if (!plan || !buf || !buflen) return XRFTHIP_BAD_ARG;
    if (plan->sub_x) {  // the two one-axis plans' records, one after the other
        const int n1 = xrfthip_plan_profile_read(plan->sub_x, buf, buflen);
        if (n1 < 0) return n1;
        const int n2 = xrfthip_plan_profile_read(plan->sub_y, buf + n1, buflen - (size_t)n1);
        return n2 < 0 ? n2 : n1 + n2;
    }
    std::vector<std::string> order;
    std::map<std::string, std::pair<long long, double>> agg;
    for (auto& r : plan->prof_recs) {
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        if (!agg.count(r.label)) order.push_back(r.label);
        agg[r.label].first += 1;
        agg[r.label].second += ms;
    }
    std::string s;
    for (auto& l : order) appendf(s, "%s %lld %.6f\n", l.c_str(), agg[l].first, agg[l].second);
    const size_t n = std::min(buflen - 1, s.size());
    memcpy(buf, s.data(), n);
    buf[n] = 0;
    return (int)n;
}

int xrfthip_plan_uses_bluestein(const xrfthip_plan* plan) {
    if (!plan) return 0;
    const auto uses = family_ops(plan->family).uses_bluestein;
    return uses && uses(plan);
}

int xrfthip_plan_kernel_info(const xrfthip_plan* plan, int32_t* kind, int32_t* per_workgroup) {
    if (!plan || !kind || !per_workgroup) return XRFTHIP_BAD_ARG;
    family_ops(plan->family).kernel_info(plan, kind, per_workgroup);
    return XRFTHIP_OK;
}

size_t xrfthip_workspace_bytes(const xrfthip_plan* plan) {
    if (!plan) return 0;
    return plan->ws_bytes;
}

int xrfthip_plan_describe(const xrfthip_plan* plan, char* buf, size_t buflen) {
    if (!plan || !buf || !buflen) return XRFTHIP_BAD_ARG;
    std::string s;
    const xrfthip_desc& d = plan->d;
    if (!inner_layout(plan))  // (FusedInner / Composite: a header of their own)
        appendf(s, "xrfthip plan: ndim=%d batch=%lld ny=%lld nx=%lld dtype=%d mode=%d detrend=%d flags=0x%x width=%lld nx_out=%lld mirror=%d group=%d ws=%zuB\n",
                d.ndim, (long long)d.batch, (long long)d.ny, (long long)d.nx, d.dtype, plan->coherence ? (int)XRFTHIP_OUT_COHERENCE : (int)d.out_mode, d.detrend, d.flags,
                plan->width, plan->nx_out, (int)plan->mirror, plan->G, plan->ws_bytes);
    // a strided plan: said on the line of the pass that reads the caller's input, by every family that family_reads_strided() names (empty on a dense plan)
    std::string in_note_;
    if (in_strided(plan)) appendf(in_note_, "; input read where it lies: in pitch %lld / slab %lld", in_pitch(plan), in_slab(plan));
    if (in_half(plan)) appendf(in_note_, "; %s input read where it lies (2 bytes per sample), widened to float32 in registers", plan->in16 == 2 ? "bfloat16" : "float16");
    const char* in_note = in_note_.c_str();
    if (const auto describe = family_ops(plan->family).describe) describe(plan, s, in_note);
    if (mean_plan(plan))
        appendf(s, "  [mean over the batch] mean_batch=%lld: %lld outputs, each the mean of %lld consecutive slabs summed inside the last pass (at most %d float32 terms in a row, then "
                   "float64), P=%d runs per output (run=%lld slabs at most per workgroup) with a float64 partial each (%zuB of the workspace), summed in order and written once by mean_finish; the spectra of the single slabs are never stored\n",
                (long long)d.mean_batch, (long long)(d.batch / d.mean_batch * (welch_cols(plan) ? d.inner : 1)), (long long)d.mean_batch, kMeanChain, plan->mean_P, plan->mean_run, plan->ws_bytes - plan->off_mean);
    if (mean_plan(plan) && plan->coherence)
        appendf(s, "  [coherence] the partial holds re C, im C, A, B per sample (C = sum F0 conj F1, A = sum |F0|^2, B = sum |F1|^2); mean_finish writes |C|^2 / (A B), real, "
                   "no clamp; scale, 1 / M and the phase tables cancel\n");
    if (!inner_layout(plan)) {
        describe_passes(s, plan->passes_f0, "f0");
        describe_passes(s, plan->passes, "main");
    }
    const size_t n = std::min(buflen - 1, s.size());
    memcpy(buf, s.data(), n);
    buf[n] = 0;
    return (int)n;
}

size_t xrfthip_plan_pass1_bytes(const xrfthip_plan* plan) {
    if (!plan) return 0;
    return fasty_pass1_bytes(plan);
}

int xrfthip_plan_pass1_signature(const xrfthip_plan* plan, int field, uint64_t* sig) {
    if (!plan || !sig || field < 0 || field > (plan_two(plan) ? 1 : 0) || !fasty_pass1_bytes(plan)) return XRFTHIP_BAD_ARG;
    *sig = fasty_pass1_signature(plan, field);
    return XRFTHIP_OK;
}

int xrfthip_exec_ex(const xrfthip_plan* plan, const xrfthip_exec_args* args) {
    if (!plan || !args || args->struct_size != sizeof(xrfthip_exec_args) || !args->d_in0) return XRFTHIP_BAD_ARG;
    const xrfthip_plan* P = plan;
    const xrfthip_desc& d = P->d;
    const void *d_in0 = args->d_in0, *d_in1 = args->d_in1;
    void *d_out = args->d_out, *d_iso = args->d_iso, *d_workspace = args->d_workspace;
    const bool cross = d.out_mode == XRFTHIP_OUT_CROSS || d.out_mode == XRFTHIP_OUT_PHASE;
    const bool iso = (d.flags & XRFTHIP_ISO) != 0;
    if (cross && !d_in1) return XRFTHIP_BAD_ARG;
    if (in_strided(P) && ((((uintptr_t)d_in0) & 15) || (cross && (((uintptr_t)d_in1) & 15)))) return XRFTHIP_BAD_ARG;  // (a strided plan's vector loads: 16-byte aligned fields)
    if (in_half(P)) {  // (a half plan's vector loads: 16-byte aligned fields, else "the caller widens"; and never a kernel that reads 4-byte samples)
        if (!half_family(P) || (((uintptr_t)d_in0) & 15) || (cross && (((uintptr_t)d_in1) & 15))) return XRFTHIP_UNSUPPORTED_LENGTH;
    }
    if (!d_out && !(d.flags & XRFTHIP_NO_SPECTRUM_OUT)) return XRFTHIP_BAD_ARG;
    if (iso && (!d_iso || !P->binmap.p)) return d_iso ? XRFTHIP_MISSING_TABLE : XRFTHIP_BAD_ARG;
    const bool inner = inner_layout(P);  // (always a workspace)
    if (taper_plan(P) && !P->w_taps.p) return XRFTHIP_BAD_ARG;  // (a multitaper plan without its table: xrfthip_plan_set_tapers)
    if (!inner && !family_ops(P->family).no_generic_passes && P->passes.empty()) return XRFTHIP_MISSING_TABLE;  // (the generic passes stand behind every other family)
    // pass-1 blocks: the fields of a plan that hands them over (fasty_pass1_bytes), whole, aligned, apart from each other and from the workspace
    ExecArgs a{d_in0, d_in1, nullptr, (double*)d_iso, (char*)d_workspace, (hipStream_t)args->stream};
    const int nf = cross ? 2 : 1;
    int handed = 0;
    for (int f = 0; f < 2; ++f) {
        const uint32_t mode = args->field[f].pass1_mode;
        if (mode > XRFTHIP_PASS1_CONSUME || (mode && f >= nf)) return XRFTHIP_BAD_ARG;
        if (!mode) continue;
        char* b = (char*)args->field[f].pass1_block;
        if (!fasty_pass1_bytes(P) || !b || (((uintptr_t)b) & 255)) return XRFTHIP_BAD_ARG;
        a.p1_block[f] = b; a.p1_mode[f] = mode;
        ++handed;
    }
    // ... with every field handed over nothing of pass 1 lies in the workspace: it shrinks by the fields' shares (the remaining parts move up, run_fasty)
    const size_t need = handed == nf ? P->ws_bytes - (size_t)nf * fasty_pass1_bytes(P) : P->ws_bytes;
    if (args->ws_bytes < need || (!d_workspace && (inner || need))) return XRFTHIP_WORKSPACE_TOO_SMALL;
    if (handed) {
        const size_t pb = fasty_pass1_bytes(P);
        auto apart = [](const char* x, size_t nx_, const char* y, size_t ny_) { return !nx_ || !ny_ || x + nx_ <= y || y + ny_ <= x; };
        for (int f = 0; f < nf; ++f)
            if (a.p1_block[f] && !apart(a.p1_block[f], pb, a.ws, args->ws_bytes)) return XRFTHIP_BAD_ARG;
        if (a.p1_block[0] && a.p1_block[1] && !apart(a.p1_block[0], pb, a.p1_block[1], pb)) return XRFTHIP_BAD_ARG;
    }
    if (d.batch == 0) return XRFTHIP_OK;
    a.out = (d.flags & XRFTHIP_NO_SPECTRUM_OUT) ? nullptr : d_out;
    if (iso && !inner) HIP_TRY(hipMemsetAsync(d_iso, 0, (size_t)d.batch * P->nbins * (cross ? 16 : 8), a.stream));
    return family_ops(P->family).run(P, a);
}

// (the all-private case of xrfthip_exec_ex: every field's pass 1 inside the workspace)
int xrfthip_exec(const xrfthip_plan* plan, const void* d_in0, const void* d_in1, void* d_out, void* d_iso,
                 void* d_workspace, size_t ws_bytes, void* stream) {
    xrfthip_exec_args args{};
    args.struct_size = sizeof args;
    args.d_in0 = d_in0; args.d_in1 = d_in1; args.d_out = d_out; args.d_iso = d_iso;
    args.d_workspace = d_workspace; args.ws_bytes = ws_bytes; args.stream = stream;
    return xrfthip_exec_ex(plan, &args);
}


}  // extern "C"
