// host_welch.inc -- a file of its own, compiled as the tail of host_rows.cpp's translation unit and not as a unit of its own: the unit lists live in the build scripts
// (__graft_entry__.py, tests/emu/build_emu.py), and the test tree of an earlier commit, run against these sources with its own build_emu.py, links only the units it lists.
// The segment families (xrfthip_desc.seg_hop): the overlapping L-sample segments of a series, read where they lie, detrended, windowed and transformed in an LDS tile.
//   FastW   Welch spectra (fastw.h): the mean power / cross spectrum of a series' segments, two segments packed per sequence (a + i b), float64 partial per run
//   FastK   spectrograms (xrfthip_desc.seg_keep, fastk.h): every segment's spectrum kept, a segment packed with itself as a sequence of L / 2 points, no workspace
//           ... and its way back, the synthesis (xrfthip_desc.seg_synth, fasto.h; the *_fasto entries below): the series rebuilt from its segments' half spectra --
//           inverse transform, window, overlap-add and the division by the summed squared windows in one pass, every output sample gathered by one thread; rows
//           layout only, no workspace.  It is a form of FastK and not an enum value of its own: the segment spectra's family, both directions
//           ... and both directions in one tile, the FIR filter by overlap-save (xrfthip_desc.seg_filter, fastf.h; the *_fastf entries below): a series' segments
//           transformed, multiplied by the response, transformed back, the samples that do not wrap around written once; no workspace; rows layout, or (xrfthip_desc.
//           seg_filter_cols with seg_stride) the column layout, its result in the array's own order
//   FastW   ... and its multitaper form (xrfthip_desc.seg_tapers, fastt.h; the *_fastt entries below): ONE series of N samples per output under K tapers, two tapers of the same
//           samples packed per sequence, a workgroup owns whole outputs -- no workspace, no finish kernel; rows layout only, seg_hop = 0
// FastW and FastK in the rows layout (one series per workgroup) or the column layout (xrfthip_desc.seg_stride: C adjacent columns of a (time, ..) block per workgroup).

// xrfthip_plan_create's checks of seg_hop / seg_stride / seg_keep (XRFTHIP_BAD_ARG; what try_fastw declines is "the caller composes"), on its own copy of the descriptor: seg_stride = 1 is the rows layout and becomes it;
// in_stride_batch is the series pitch here (any multiple of 4 bytes: the kernels load single samples) -- it is checked, returned as *pitch and cleared, so that
// nothing of the strided-view rules (16-byte strides and pointers) applies to such a plan.  mean_batch counts the segments of a series (1 included when they are kept)
int seg_desc_check(xrfthip_desc& s, long long* pitch) {
    *pitch = 0;
    // seg_tapers / seg_taper_len: the multitaper form (fastt.h) -- ONE series of N samples per output, no segments: seg_hop and every other seg_* word 0
    if (s.seg_tapers < 0 || (s.seg_tapers == 0 && s.seg_taper_len != 0)) return XRFTHIP_BAD_ARG;
    if (s.seg_tapers > 0) {
        if (s.seg_hop || s.seg_reserved || s.seg_stride || s.seg_reserved2 || s.seg_keep || s.seg_reserved3 || s.seg_synth || s.seg_reserved4 || s.seg_filter || s.seg_lead ||
            s.seg_in_len || s.seg_out_len || s.seg_filter_cols || s.seg_reserved5) return XRFTHIP_BAD_ARG;
        const uint32_t known = XRFTHIP_SHIFT_X | XRFTHIP_HALF_X | XRFTHIP_REALDIM_X2 | XRFTHIP_ISHIFT_X | XRFTHIP_FLIP_X | XRFTHIP_FLIP0_X;  // (the flips: try_fastt declines them)
        if (s.ndim != 1 || s.ny != 1 || s.nx < 1 || s.nx > (1LL << 30) || s.dtype != XRFTHIP_F32 || (s.out_mode != XRFTHIP_OUT_POWER && s.out_mode != XRFTHIP_OUT_CROSS) ||
            s.mean_batch > 1 || s.batch < 0 || s.inner > 1 || s.mid > 1 || s.herm_ny || s.herm_nx || s.in_stride_y || (s.flags & ~known)) return XRFTHIP_BAD_ARG;
        if (s.seg_taper_len < 1 || s.seg_taper_len > s.nx || (s.in_stride_batch != 0 && s.in_stride_batch < s.seg_taper_len)) return XRFTHIP_BAD_ARG;
        *pitch = s.in_stride_batch ? s.in_stride_batch : s.seg_taper_len;
        s.in_stride_batch = 0;
        s.mean_batch = 0;
        return XRFTHIP_OK;
    }
    if ((s.seg_filter != 0 && s.seg_filter != 1) || (!s.seg_filter && (s.seg_lead != 0 || s.seg_in_len != 0 || s.seg_out_len != 0))) return XRFTHIP_BAD_ARG;
    const bool filt = s.seg_filter == 1;
    // seg_filter_cols: the filter's column layout -- seg_stride = S >= inner, kept as it came (S = 1 with inner = 1 is one column, not the rows layout)
    if ((s.seg_filter_cols != 0 && s.seg_filter_cols != 1) || s.seg_reserved5 != 0 || (s.seg_filter_cols && !filt)) return XRFTHIP_BAD_ARG;
    const bool fcols = s.seg_filter_cols == 1;
    if (filt && (s.seg_hop <= 0 || s.seg_keep != 0 || s.seg_synth != 0 || (fcols ? s.seg_stride < 1 : s.seg_stride != 0))) return XRFTHIP_BAD_ARG;
    if ((s.seg_synth != 0 && s.seg_synth != 1) || s.seg_reserved4 != 0 || (s.seg_synth && (s.seg_hop <= 0 || s.seg_keep != 0))) return XRFTHIP_BAD_ARG;
    const bool synth = s.seg_synth == 1;
    if ((s.seg_keep != 0 && s.seg_keep != 1) || s.seg_reserved3 != 0 || (s.seg_keep && s.seg_hop <= 0)) return XRFTHIP_BAD_ARG;
    const bool keep = s.seg_keep == 1;
    if (s.seg_hop < 0 || s.seg_reserved != 0 || s.seg_stride < 0 || s.seg_reserved2 != 0) return XRFTHIP_BAD_ARG;
    if (s.seg_stride > 0 && (s.seg_hop == 0 || s.seg_stride < s.inner)) return XRFTHIP_BAD_ARG;
    if (s.seg_stride == 1 && !fcols) s.seg_stride = 0;
    if (s.seg_hop == 0) return XRFTHIP_OK;
    if (s.ndim != 1 || s.ny != 1 || s.nx < 1 || s.seg_hop > s.nx || (s.flags & (XRFTHIP_AXIS_Y | XRFTHIP_ISO)) || (s.inner > 1 && !s.seg_stride) || s.mid > 1 || s.herm_ny || s.herm_nx || s.in_stride_y) return XRFTHIP_BAD_ARG;
    if (s.mean_batch < (keep || synth || filt ? 1 : 2) || s.batch < 0 || s.batch % s.mean_batch != 0) return XRFTHIP_BAD_ARG;
    if (s.nx > (1LL << 30) || s.mean_batch > (1LL << 31) - 1) return XRFTHIP_BAD_ARG;
    if (filt) {  // a series of N samples in, n_out filtered samples out: K = L - V + 1 taps, at least half of every transform kept; the pitch counts samples
        const long long K = s.nx - s.seg_hop + 1, cap = 1LL << 60;
        if (s.dtype != XRFTHIP_F32 || s.out_mode != XRFTHIP_OUT_COMPLEX || s.detrend != XRFTHIP_DETREND_NONE || s.flags != 0 || 2 * s.seg_hop < s.nx) return XRFTHIP_BAD_ARG;
        if (s.seg_in_len < 1 || s.seg_in_len > cap || s.seg_out_len < 1 || s.seg_out_len > cap || s.seg_lead < 0 || s.seg_lead > K - 1) return XRFTHIP_BAD_ARG;
        if (s.seg_lead + s.seg_out_len > s.seg_in_len + K - 1 || s.mean_batch != (s.seg_out_len + s.seg_hop - 1) / s.seg_hop) return XRFTHIP_BAD_ARG;
        if (fcols) {  // [blocks][N][inner] columns, samples S apart: the pitch counts elements between blocks (the offsets stay far inside 64 bits, as in the other column forms)
            const long long lim = (1LL << 31) - 1;
            if (s.seg_stride > lim || s.inner > lim || s.seg_in_len > lim || s.seg_out_len > lim) return XRFTHIP_BAD_ARG;
            const long long dense = (s.seg_in_len - 1) * s.seg_stride + s.inner;  // the elements one block reaches
            if (s.in_stride_batch != 0 && s.in_stride_batch < dense) return XRFTHIP_BAD_ARG;
            *pitch = s.in_stride_batch ? s.in_stride_batch : s.seg_in_len * s.seg_stride;
            s.in_stride_batch = 0;
            return XRFTHIP_OK;
        }
        if (s.in_stride_batch != 0 && s.in_stride_batch < s.seg_in_len) return XRFTHIP_BAD_ARG;
        *pitch = s.in_stride_batch ? s.in_stride_batch : s.seg_in_len;
        s.in_stride_batch = 0;
        return XRFTHIP_OK;
    }
    if (synth) {  // half spectra in, the series out: the pitch counts complex elements, M (L / 2 + 1) of them a dense series (seg_stride: try_fastw declines)
        if (s.dtype != XRFTHIP_C64 || s.out_mode != XRFTHIP_OUT_COMPLEX || s.detrend != XRFTHIP_DETREND_NONE || s.flags != (XRFTHIP_INVERSE | XRFTHIP_C2R_X) || (s.nx & 1)) return XRFTHIP_BAD_ARG;
        const long long dense = s.mean_batch * (s.nx / 2 + 1);
        if (s.in_stride_batch != 0 && s.in_stride_batch < dense) return XRFTHIP_BAD_ARG;
        *pitch = s.in_stride_batch ? s.in_stride_batch : dense;
        s.in_stride_batch = 0;
        return XRFTHIP_OK;
    }
    if (s.out_mode != XRFTHIP_OUT_POWER && s.out_mode != (keep ? XRFTHIP_OUT_COMPLEX : XRFTHIP_OUT_CROSS)) return XRFTHIP_BAD_ARG;
    const long long span = (s.mean_batch - 1) * s.seg_hop + s.nx, S = s.seg_stride ? s.seg_stride : 1;
    // (the column layout: the offsets stay far inside 64 bits -- span < 2^62, S and inner below 2^31)
    if (s.seg_stride && (s.seg_stride > (1LL << 31) - 1 || s.inner > (1LL << 31) - 1 || span > (1LL << 31) - 1)) return XRFTHIP_BAD_ARG;
    const long long dense = s.seg_stride ? (span - 1) * S + s.inner : span;  // the samples one series (block of columns) reaches
    if (s.in_stride_batch != 0 && s.in_stride_batch < dense) return XRFTHIP_BAD_ARG;
    *pitch = s.in_stride_batch ? s.in_stride_batch : span * S;
    s.in_stride_batch = 0;
    return XRFTHIP_OK;
}

static int seg_n(const xrfthip_plan* P) { return (int)(keep_plan(P) || synth_plan(P) || filter_plan(P) ? P->d.nx / 2 : P->d.nx); }  // points of a tile sequence: a pair of segments, or a segment packed with itself

// The tile of a workgroup: C adjacent columns (32 -- 128 bytes of a time row -- where the tile holds them, else what it holds, whatever `inner` is: the order of a
// column's sums does not depend on its neighbours; 1 in the rows layout) times as many sequences of each as `need` asks for, a power of two, kWPoints points at most
static int seg_cols(const xrfthip_plan* P) { return welch_cols(P) ? std::min<int>(kWCols, kWPoints / seg_n(P)) : 1; }  // C
static long long seg_ngroups(const xrfthip_plan* P) { return welch_cols(P) ? (P->d.inner + seg_cols(P) - 1) / seg_cols(P) : 1; }  // groups of C columns per block
static SegGeom seg_geom(const xrfthip_plan* P, long long need) {
    const xrfthip_desc& d = P->d;
    const bool keep = keep_plan(P);
    const long long n = seg_n(P), cap = kWPoints / n;  // points of a sequence, sequences the tile holds
    SegGeom g;
    g.C = seg_cols(P);
    g.lgC = ilog2i(g.C);
    g.ngroups = seg_ngroups(P);
    g.seqs = g.C;
    while (g.seqs / g.C < need && g.seqs < cap) g.seqs *= 2;
    long long ss = n + (n >> 4) + 1;
    if ((ss & 1) == 0) ++ss;  // (an odd stride: the sequences of a tile start on different banks)
    g.stride = (int)ss;
    const size_t tile = (((size_t)g.seqs * (size_t)ss + 1) & ~(size_t)1) * sizeof(cf);
    // [tile per field][red: 2 kWThreads doubles][coef: 2 doubles per segment]
    g.lds = tile * (d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1) + (size_t)(2 * kWThreads + 2 * (keep ? 1 : 2) * g.seqs) * sizeof(double);
    const long long spr = g.seqs / g.C;  // FastK: segments of a column per round, one workgroup per (series or group of columns, round)
    g.rounds = keep ? (d.mean_batch + spr - 1) / spr : 1;
    return g;
}
static long long seg_units(const xrfthip_plan* P, const SegGeom& g) { return P->d.batch / P->d.mean_batch * g.ngroups; }  // series, or groups of columns over all blocks

// The synthesis form of FastK (seg_synth): R = ceil(L / H) segments meet in a sample, the tile holds NS = 8192 / L; a workgroup advances by F = NS - (R - 1) segments, max(M - R + 1, 1) / F (rounded
// up) of them serve a series (fasto.h).  Declined: 2 (R - 1) > NS -- more than half of a workgroup's transforms would be repeated
struct SynthGeom { long long R, NS, F, wgs, span; };
static SynthGeom synth_geom(const xrfthip_desc& d) {
    SynthGeom g;
    g.R = (d.nx + d.seg_hop - 1) / d.seg_hop;
    g.NS = 2 * kWPoints / d.nx;
    g.F = g.NS - (g.R - 1);
    g.wgs = g.F > 0 ? (std::max<long long>(d.mean_batch - g.R + 1, 1) + g.F - 1) / g.F : 0;
    g.span = (d.mean_batch - 1) * d.seg_hop + d.nx;
    return g;
}
static int try_fasto(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    const bool len_ok = d.nx >= 64 && d.nx <= 4096 && (d.nx & (d.nx - 1)) == 0;
    if (!len_ok || d.seg_stride || env_ll("XRFTHIP_FASTW", 1) == 0 || env_ll("XRFTHIP_FASTW_SYNTH", 1) == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
    const SynthGeom g = synth_geom(d);
    if (2 * (g.R - 1) > g.NS || g.span > 0x7fffffffLL) return XRFTHIP_UNSUPPORTED_LENGTH;
    const long long series = d.batch / d.mean_batch;
    if (series > 0 && g.wgs > 0x7fffffffLL / series) return XRFTHIP_UNSUPPORTED_LENGTH;  // (one launch; declined, never truncated)
    P->family = P->chosen = Family::FastK;
    FftTables& t = P->tables[seg_n(P)];
    const int rc = build_tables<float>(t, seg_n(P));
    if (rc) return rc;
    for (int r : t.radix) if (r != 2 && r != 4 && r != 8 && r != 16) return XRFTHIP_UNSUPPORTED_LENGTH;
    return plan_twiddle(P, P->w_twr, d.nx, d.nx / 2 + 1);  // (W_L^k, k <= L / 2, the packing)
}

// The filter form of FastK (seg_filter): the tile holds NS = 8192 / L segments, ceil(M / NS) workgroups serve a series (fastf.h); no segment is transformed twice
// The column layout (seg_filter_cols): a unit is C = min(kWCols, NS) adjacent columns of a block and the tile holds spr = NS / C consecutive segments of each
// (4, 2, 1, 1 at L = 64, 128, 256, 512): ceil(M / spr) workgroups serve a unit
static long long filter_wgs(const xrfthip_desc& d) {
    const long long NS = 2 * kWPoints / d.nx;
    const long long spr = d.seg_filter_cols == 1 ? NS / std::min<long long>(kWCols, NS) : NS;  // segments of one series (column) per tile
    return (d.mean_batch + spr - 1) / spr;
}
static int try_fastf(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    const bool cols = filter_cols(P);
    const bool len_ok = d.nx >= 64 && d.nx <= (cols ? kWColsMaxL : 4096) && (d.nx & (d.nx - 1)) == 0;
    if (!len_ok || env_ll("XRFTHIP_FASTW", 1) == 0 || env_ll("XRFTHIP_FASTW_FILTER", 1) == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
    if (cols && (env_ll("XRFTHIP_FASTW_COLS", 1) == 0 || env_ll("XRFTHIP_FASTW_FILTER_COLS", 1) == 0)) return XRFTHIP_UNSUPPORTED_LENGTH;  // (the caller arranges: one transposed copy, the rows layout)
    long long series = d.batch / d.mean_batch;  // series, or (the column layout) groups of columns over all blocks
    if (cols) {
        const long long groups = seg_ngroups(P);
        if (series > 0 && groups > 0x7fffffffLL / series) return XRFTHIP_UNSUPPORTED_LENGTH;
        series *= groups;
        // ... and by default only the classes that measured faster than the route they replace (profiles/r30_fir_filter_cols.txt): wide grids, 0.38 .. 0.47 of its
        // time.  A narrow grid lost -- (8192, 4096, 8) along dim 1 at L = 512, 8 of a group's 16 columns live, 3.4 against 2.8 ms: the dead columns of a group are
        // loaded as zeros, transformed and dropped, so the tile does half its work for nothing -- and a grid with less of its groups live wastes more.  Declined:
        // at most half of the groups' columns live (2 inner <= groups C).  XRFTHIP_MEAN_ALL=1: every class this kernel takes
        if (2 * d.inner <= groups * seg_cols(P) && env_ll("XRFTHIP_MEAN_ALL", 0) == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
    }
    if (series > 0 && filter_wgs(d) > 0x7fffffffLL / series) return XRFTHIP_UNSUPPORTED_LENGTH;  // (one launch; declined, never truncated)
    P->family = P->chosen = Family::FastK;
    FftTables& t = P->tables[seg_n(P)];
    const int rc = build_tables<float>(t, seg_n(P));
    if (rc) return rc;
    for (int r : t.radix) if (r != 2 && r != 4 && r != 8 && r != 16) return XRFTHIP_UNSUPPORTED_LENGTH;
    return plan_twiddle(P, P->w_twr, d.nx, d.nx / 2 + 1);  // (W_L^k, k <= L / 2, the unpacking and the packing)
}

// The multitaper form of FastW (seg_tapers = K, seg_taper_len = N; fastt.h): KP = ceil(K / 2) sequences of L points per series, G = 4096 / L in the tile; a workgroup takes
// NS = max(1, G / KP) consecutive series, or one series in ceil(KP / G) rounds.  tps: the threads per series of the detrend's sums, the largest power of two with
// NS tps <= 256 -- a function of (L, K) only
struct TaperGeom { int KP, G, NS, seqs, rounds, tps; long long wgs; };
static TaperGeom taper_geom(const xrfthip_desc& d) {
    TaperGeom g;
    g.KP = (int)((d.seg_tapers + 1) / 2);
    g.G = (int)(kWPoints / d.nx);
    g.NS = std::max(1, g.G / g.KP);
    g.seqs = g.KP <= g.G ? g.NS * g.KP : g.G;
    g.rounds = g.KP <= g.G ? 1 : (g.KP + g.G - 1) / g.G;
    g.tps = 1;
    while (2 * g.tps * g.NS <= kWThreads) g.tps *= 2;
    g.wgs = (d.batch + g.NS - 1) / g.NS;
    return g;
}
static int try_fastt(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    const bool len_ok = d.nx >= 64 && d.nx <= 4096 && (d.nx & (d.nx - 1)) == 0;
    if (!len_ok || d.seg_tapers > 2 * kMeanChain || (d.flags & (XRFTHIP_FLIP_X | XRFTHIP_FLIP0_X)) || env_ll("XRFTHIP_FASTW", 1) == 0 || env_ll("XRFTHIP_FASTW_TAPERS", 1) == 0)
        return XRFTHIP_UNSUPPORTED_LENGTH;  // (K <= 32: at most kMeanChain rounds, one float32 chain)
    if (taper_geom(d).wgs > 0x7fffffffLL) return XRFTHIP_UNSUPPORTED_LENGTH;  // (one launch; declined, never truncated)
    P->family = P->chosen = Family::FastW;
    FftTables& t = P->tables[(int)d.nx];
    const int rc = build_tables<float>(t, (int)d.nx);
    if (rc) return rc;
    for (int r : t.radix) if (r != 2 && r != 4 && r != 8 && r != 16) return XRFTHIP_UNSUPPORTED_LENGTH;
    return XRFTHIP_OK;
}

// FastW / FastK: float32 series, segments of 64 .. 4096 samples, a power of two (the column layout: up to 512 -- the tile holds 8 adjacent columns at least; beyond,
// the caller arranges the series as rows)
int try_fastw(xrfthip_plan* P) {
    const xrfthip_desc& d = P->d;
    if (taper_plan(P)) return try_fastt(P);
    if (!welch_plan(P)) return kDeclined;
    if (synth_plan(P)) return try_fasto(P);
    if (filter_plan(P)) return try_fastf(P);
    const bool cols = welch_cols(P), keep = keep_plan(P);
    const bool len_ok = d.nx >= 64 && d.nx <= (cols ? kWColsMaxL : 4096) && (d.nx & (d.nx - 1)) == 0;
    // (ISHIFT_X: (-1)^k on the transform, gone in |X|^2 and in X conj X')
    const uint32_t ok = XRFTHIP_SHIFT_X | XRFTHIP_HALF_X | (d.out_mode != XRFTHIP_OUT_COMPLEX ? (XRFTHIP_REALDIM_X2 | XRFTHIP_ISHIFT_X) : 0u);
    if (!len_ok || d.dtype != XRFTHIP_F32 || in_half(P) || (d.flags & ~ok) || env_ll("XRFTHIP_FASTW", 1) == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
    if ((keep && env_ll("XRFTHIP_FASTW_KEEP", 1) == 0) || (cols && env_ll("XRFTHIP_FASTW_COLS", 1) == 0)) return XRFTHIP_UNSUPPORTED_LENGTH;
    // one launch of at most 2^31 - 1 workgroups -- FastW: outputs x runs (at most 1024), one finish workgroup per output; FastK: units x rounds.  Declined, never truncated
    if (keep) {
        const SegGeom g = seg_geom(P, d.mean_batch);
        const long long units = seg_units(P, g);
        if (units > 0 && g.rounds > 0x7fffffffLL / units) return XRFTHIP_UNSUPPORTED_LENGTH;
        // ... and by default only the classes that measured faster than the composition they replace (profiles/r21_spectrogram.txt): fourteen of sixteen, 0.54 .. 0.92 of its
        // time.  L = 4096 without overlap lost -- (256, 4194304) 9.7 against 8.2 ms, one-sided 8.7 against 8.2: there the composition copies nothing (the segments are a
        // reshape) and runs the register-resident row kernel of fastr.h.  XRFTHIP_MEAN_ALL=1: every class this kernel takes
        if (d.nx == 4096 && d.seg_hop == d.nx && env_ll("XRFTHIP_MEAN_ALL", 0) == 0) return XRFTHIP_UNSUPPORTED_LENGTH;
    } else if (d.batch / d.mean_batch * (cols ? d.inner : 1) > 0x7fffffffLL / 1024) return XRFTHIP_UNSUPPORTED_LENGTH;
    P->family = P->chosen = keep ? Family::FastK : Family::FastW;
    FftTables& t = P->tables[seg_n(P)];
    const int rc = build_tables<float>(t, seg_n(P));  // W_n^k, the radices of the in-place passes, and where they leave frequency k
    if (rc) return rc;
    for (int r : t.radix) if (r != 2 && r != 4 && r != 8 && r != 16) return XRFTHIP_UNSUPPORTED_LENGTH;
    return keep ? plan_twiddle(P, P->w_twr, d.nx, d.nx / 2 + 1) : XRFTHIP_OK;  // (FastK: W_L^k, k <= L / 2, the unpacking)
}

// FastW's workspace: the float64 partial of every run of every output (one launch, one workgroup per run); then the tile: as many pairs of segments per round as
// the longest run has.  FastK: no workspace (every output element is written once by the thread that computed it), as many segments per round as a series has
static void layout_fastw(xrfthip_plan* P) {
    layout_one_pass(P);
    if (taper_plan(P)) {  // the multitaper form: no workspace; the tile holds the pairs of tapers of NS series (or G pairs of one), [red][coef: 2 NS doubles per field] behind it
        const TaperGeom g = taper_geom(P->d);
        const long long n = P->d.nx;
        long long ss = n + (n >> 4) + 1;
        if ((ss & 1) == 0) ++ss;  // (an odd stride, as seg_geom)
        P->w = SegGeom();
        P->w.seqs = g.seqs;
        P->w.stride = (int)ss;
        P->w.rounds = g.rounds;
        const size_t tile = (((size_t)g.seqs * (size_t)ss + 1) & ~(size_t)1) * sizeof(cf);
        P->w.lds = tile * (P->d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1) + (size_t)(2 * kWThreads + 4 * g.NS) * sizeof(double);
        return;
    }
    P->ws_bytes = mean_layout(P, 0, 1, P->d.batch * seg_ngroups(P));  // (the launch: groups x runs workgroups per block)
    P->w = seg_geom(P, (P->mean_run + 1) / 2);
}
// ... the synthesis: no workspace either; the tile holds the segments of one workgroup (all of a short series), nothing behind it
static void layout_fasto(xrfthip_plan* P) {
    layout_one_pass(P);
    P->w = seg_geom(P, std::min<long long>(P->d.mean_batch, synth_geom(P->d).NS));
    P->w.lds = (((size_t)P->w.seqs * (size_t)P->w.stride + 1) & ~(size_t)1) * sizeof(cf);
    P->w.rounds = synth_geom(P->d).wgs;
}
// ... the filter: the same
static void layout_fastf(xrfthip_plan* P) {
    layout_one_pass(P);
    P->w = seg_geom(P, std::min<long long>(P->d.mean_batch, 2 * kWPoints / P->d.nx / seg_cols(P)));  // (the column layout: C sequences per segment of the tile)
    P->w.lds = (((size_t)P->w.seqs * (size_t)P->w.stride + 1) & ~(size_t)1) * sizeof(cf);
    P->w.rounds = filter_wgs(P->d);
}
static void layout_fastk(xrfthip_plan* P) {
    if (synth_plan(P)) return layout_fasto(P);
    if (filter_plan(P)) return layout_fastf(P);
    layout_one_pass(P);
    P->w = seg_geom(P, P->d.mean_batch);
}

// the head of the two kernels' arguments (seg_tile.h)
static void seg_args(const xrfthip_plan* P, SegTile& p) {
    const xrfthip_desc& d = P->d;
    const FftTables& t = P->tables.at(seg_n(P));
    const bool cols = welch_cols(P);
    p.tw = (const cf*)t.tw.p; p.rev = (const unsigned*)t.rev.p;
    p.win = (const float*)P->win[1].p;
    p.pitch = P->w_pitch; p.hop = d.seg_hop; p.sstride = cols ? d.seg_stride : 1;
    p.L = (int)d.nx; p.M = (int)d.mean_batch;
    p.seq_stride = P->w.stride; p.pad_shift = 4;
    p.nr = (int)t.radix.size();
    for (int i = 0; i < p.nr; ++i) p.radix[i] = t.radix[i];
    p.detrend = d.detrend;
    p.scale = (float)d.scale;
    p.inner = cols ? (int)d.inner : 1; p.lgC = P->w.lgC; p.ngroups = (int)P->w.ngroups;
}

// the launch of a segment kernel, K<A, column layout>, over nwg workgroups under a profiling label
#define SEG_LAUNCH(K, A, LABEL, NWG, ARG) do { \
        const dim3 grid((unsigned)(NWG)), blk((unsigned)kWThreads); \
        xrfthip_plan::ProfRec* rec = prof_begin(P, LABEL, st); \
        if (welch_cols(P)) { if (A) { auto k = &K<true, true>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, ARG); } else { auto k = &K<false, true>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, ARG); } } \
        else if (A) { auto k = &K<true, false>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, ARG); } else { auto k = &K<false, false>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, ARG); } \
        prof_end(rec, st); \
        HIP_TRY(hipGetLastError()); } while (0)

// FastK: one launch, nothing else
static int run_fasto(const xrfthip_plan* P, const ExecArgs& a);
static int run_fastf(const xrfthip_plan* P, const ExecArgs& a);
static int run_fastk(const xrfthip_plan* P, const ExecArgs& a) {
    if (synth_plan(P)) return run_fasto(P, a);
    if (filter_plan(P)) return run_fastf(P, a);
    const xrfthip_desc& d = P->d;
    hipStream_t st = a.stream;
    FastK p{};
    seg_args(P, p.t);
    p.in = (const float*)a.in0; p.out = a.out;
    p.twr = (const cf*)P->w_twr.p;
    p.NS = P->w.seqs; p.rounds = (int)P->w.rounds;
    p.nx_out = (int)P->nx_out;
    p.shift = (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0;
    p.realdim2 = (d.flags & XRFTHIP_REALDIM_X2) ? 1 : 0;
    const long long nwg = seg_units(P, P->w) * P->w.rounds;
    if (nwg > 0x7fffffffLL) return XRFTHIP_BAD_ARG;  // (try_fastw declined it)
    SEG_LAUNCH(fastk_kernel, d.out_mode == XRFTHIP_OUT_POWER, "fastk_segments", nwg, p);
    return XRFTHIP_OK;
}

// ... the synthesis: one launch, nothing else
static int run_fasto(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d = P->d;
    hipStream_t st = a.stream;
    const SynthGeom g = synth_geom(d);
    FastO p{};
    seg_args(P, p.t);
    p.in = (const cf*)a.in0; p.out = (float*)a.out;
    p.twr = (const cf*)P->w_twr.p;
    p.NS = (int)g.NS; p.F = (int)g.F; p.R = (int)g.R; p.wgs = (int)g.wgs;
    p.span = g.span;
    const long long nwg = d.batch / d.mean_batch * g.wgs;
    if (nwg > 0x7fffffffLL || g.span > 0x7fffffffLL) return XRFTHIP_BAD_ARG;  // (try_fasto declined it)
    const dim3 grid((unsigned)nwg), blk((unsigned)kWThreads);
    xrfthip_plan::ProfRec* rec = prof_begin(P, "fasto_overlap_add", st);
    if (p.t.win) { auto k = &fasto_kernel<true>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
    else { auto k = &fasto_kernel<false>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
    prof_end(rec, st);
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

// ... the filter: one launch, nothing else
static int run_fastf(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d = P->d;
    hipStream_t st = a.stream;
    FastF p{};
    seg_args(P, p.t);
    p.in = (const float*)a.in0; p.out = (float*)a.out;
    p.twr = (const cf*)P->w_twr.p;
    p.resp = (const cf*)P->phase[1].p;
    p.NS = (int)(2 * kWPoints / d.nx); p.wgs = (int)filter_wgs(d);
    p.K = (int)(d.nx - d.seg_hop + 1);
    p.N = d.seg_in_len; p.n_out = d.seg_out_len; p.lead = d.seg_lead;
    const bool cols = filter_cols(P);
    const long long nwg = d.batch / d.mean_batch * (cols ? P->w.ngroups : 1) * filter_wgs(d);
    if (nwg > 0x7fffffffLL) return XRFTHIP_BAD_ARG;  // (try_fastf declined it)
    const dim3 grid((unsigned)nwg), blk((unsigned)kWThreads);
    xrfthip_plan::ProfRec* rec = prof_begin(P, cols ? "fastf_overlap_save_cols" : "fastf_overlap_save", st);
    if (cols) {
        if (p.resp) { auto k = &fastf_kernel<true, true>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
        else { auto k = &fastf_kernel<false, true>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
    }
    else if (p.resp) { auto k = &fastf_kernel<true>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
    else { auto k = &fastf_kernel<false>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
    prof_end(rec, st);
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

// ... the multitaper form: one launch, nothing else
static int run_fastt(const xrfthip_plan* P, const ExecArgs& a) {
    const xrfthip_desc& d = P->d;
    hipStream_t st = a.stream;
    const TaperGeom g = taper_geom(d);
    const bool two = d.out_mode == XRFTHIP_OUT_CROSS;
    if (!P->w_taps.p || g.wgs > 0x7fffffffLL) return XRFTHIP_BAD_ARG;  // (no table: xrfthip_plan_set_tapers; the launch: try_fastt declined it)
    FastT p{};
    const FftTables& t = P->tables.at((int)d.nx);
    p.t.tw = (const cf*)t.tw.p; p.t.rev = (const unsigned*)t.rev.p;
    p.t.win = nullptr;
    p.t.pitch = P->w_pitch; p.t.hop = 0; p.t.sstride = 1;
    p.t.L = (int)d.nx; p.t.M = 1;
    p.t.seq_stride = P->w.stride; p.t.pad_shift = 4;
    p.t.nr = (int)t.radix.size();
    for (int i = 0; i < p.t.nr; ++i) p.t.radix[i] = t.radix[i];
    p.t.detrend = d.detrend;
    p.t.scale = (float)d.scale;
    p.t.inner = 1; p.t.lgC = 0; p.t.ngroups = 1;
    p.in0 = (const float*)a.in0; p.in1 = (const float*)a.in1;
    p.tap = (const float*)P->w_taps.p;
    p.out = a.out;
    p.ph = reinterpret_cast<const cf*>(P->fph[1].p);
    p.ph_on = (two && P->fph_on && p.ph) ? 1 : 0;
    p.P = d.batch;
    p.K = (int)d.seg_tapers; p.KP = g.KP; p.N = (int)d.seg_taper_len;
    p.NS = g.NS; p.seqs = g.seqs; p.rounds = g.rounds; p.tps = g.tps;
    p.nx_out = (int)P->nx_out;
    p.shift = (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0;
    p.realdim2 = (d.flags & XRFTHIP_REALDIM_X2) ? 1 : 0;
    const dim3 grid((unsigned)g.wgs), blk((unsigned)kWThreads);
    xrfthip_plan::ProfRec* rec = prof_begin(P, "fastt_tapers", st);
    if (two) { auto k = &fastt_kernel<true>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
    else { auto k = &fastt_kernel<false>; XRFT_LAUNCH(k, grid, blk, P->w.lds, st, p); }
    prof_end(rec, st);
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

// FastW: the segments' launch, then one finish workgroup per output
static int run_fastw(const xrfthip_plan* P, const ExecArgs& a) {
    if (taper_plan(P)) return run_fastt(P, a);
    const xrfthip_desc& d = P->d;
    hipStream_t st = a.stream;
    const bool two = d.out_mode == XRFTHIP_OUT_CROSS;
    FastW p{};
    seg_args(P, p.t);
    p.in0 = (const float*)a.in0; p.in1 = (const float*)a.in1;
    p.part = reinterpret_cast<double*>(a.ws + P->off_mean);
    p.P = P->mean_P; p.G = P->w.seqs;
    const long long nout = d.batch / d.mean_batch * p.t.inner, nwg = seg_units(P, P->w) * P->mean_P;
    if (nwg > 0x7fffffffLL || nout > 0x7fffffffLL) return XRFTHIP_BAD_ARG;
    SEG_LAUNCH(fastw_kernel, two, "fastw_segments", nwg, p);
    xrfthip_plan::ProfRec* rec = prof_begin(P, "fastw_finish", st);
    const int nxo = (int)P->nx_out, shift = (d.flags & XRFTHIP_SHIFT_X) ? (int)(d.nx / 2) : 0, rd2 = (d.flags & XRFTHIP_REALDIM_X2) ? 1 : 0;
    const double half_inv_m = 0.5 / (double)d.mean_batch;
    const cf* ph = reinterpret_cast<const cf*>(P->fph[1].p);
    const dim3 fgrid((unsigned)nout), fblk(256);
    if (two) { auto k = &fastw_finish_kernel<true>; XRFT_LAUNCH(k, fgrid, fblk, 0, st, (const double*)p.part, a.out, p.t.L, nxo, p.P, half_inv_m, shift, rd2, ph, (P->fph_on && ph) ? 1 : 0); }
    else { auto k = &fastw_finish_kernel<false>; XRFT_LAUNCH(k, fgrid, fblk, 0, st, (const double*)p.part, a.out, p.t.L, nxo, p.P, half_inv_m, shift, rd2, ph, 0); }
    prof_end(rec, st);
    HIP_TRY(hipGetLastError());
    return XRFTHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the rows of FastW and FastK (plan.h, FamilyOps)
// ---------------------------------------------------------------------------------------------------------------
static std::string seg_radices(const xrfthip_plan* plan) {
    std::string rad;
    for (int r : plan->tables.at(seg_n(plan)).radix) appendf(rad, "%s%d", rad.empty() ? "" : "x", r);
    return rad;
}
// the column layout's line: `unit` ("pair" | "segment") is what a sequence of the tile holds, `units` its plural as the line says it
static void describe_cols(const xrfthip_plan* plan, std::string& s, const char* units, const char* unit, const char* tail) {
    const xrfthip_desc& d = plan->d;
    const SegGeom& g = plan->w;
    if (!welch_cols(plan)) return;
    appendf(s, "  [fastw columns] the series lie along a leading axis, read where they lie: %lld blocks of %lld adjacent columns, sample stride %lld (block pitch %lld); "
               "a workgroup takes %d adjacent columns (%lld groups per block; %d bytes of one time row per wave-load) and %d %s of each per round, "
               "sequence t = (column t %% %d, %s t / %d); %s\n",
            (long long)(d.batch / d.mean_batch), (long long)d.inner, (long long)d.seg_stride, plan->w_pitch, g.C, g.ngroups, 4 * g.C, g.seqs / g.C, units, g.C, unit, g.C, tail);
}
static void describe_fasto(const xrfthip_plan* plan, std::string& s, const char*);
static void describe_fastf(const xrfthip_plan* plan, std::string& s, const char*);
static void describe_fastk(const xrfthip_plan* plan, std::string& s, const char* note) {
    if (synth_plan(plan)) return describe_fasto(plan, s, note);
    if (filter_plan(plan)) return describe_fastf(plan, s, note);
    const xrfthip_desc& d = plan->d;
    const SegGeom& g = plan->w;
    appendf(s, "  [fastw segments kept] spectrograms, one pass: %lld series of %lld segments of %lld samples, hop %lld (series pitch %lld), each segment read where it lies with "
               "4-byte loads and its own spectrum written once (%s); one %d-thread workgroup per (series, round): %lld x %lld workgroups, %d segments per round, each packed "
               "with itself (x_2j + i x_2j+1) as a %lld-point sequence of an LDS tile, detrend and window in the tile, radix %s in place, unpacked X_k = E_k + W_L^k O_k, "
               "lanes store consecutive output elements; no workspace, no partial sums, no atomics; lds=%zuB; %s; %d algorithmic bytes per output element and 4 per "
               "sample read\n",
            (long long)(d.batch / d.mean_batch), (long long)d.mean_batch, (long long)d.nx, (long long)d.seg_hop, plan->w_pitch, d.out_mode == XRFTHIP_OUT_POWER ? "|X|^2, real" : "X, complex",
            kWThreads, seg_units(plan, g), g.rounds, g.seqs / g.C, (long long)d.nx / 2, seg_radices(plan).c_str(), g.lds, kKResources, d.out_mode == XRFTHIP_OUT_POWER ? 4 : 8);
    describe_cols(plan, s, "segments", "segment", "the result is [block][segment][frequency][column], stores coalesced across columns, no transposed copy");
}
static void describe_fasto(const xrfthip_plan* plan, std::string& s, const char*) {
    const xrfthip_desc& d = plan->d;
    const SynthGeom g = synth_geom(d);
    appendf(s, "  [fastw overlap-add] synthesis, one pass: %lld series of %lld half spectra of %lld bins (series pitch %lld complex elements) to %lld samples each, hop %lld; "
               "one %d-thread workgroup per (series, run): %lld x %lld workgroups, %lld segments per tile as %lld-point sequences (Z = E + i O from X_k and conj X_n-k), "
               "conj, radix %s in place, conj; a workgroup advances by %lld segments and repeats %lld of its predecessor's; every sample gathered by one thread: "
               "sum of w x scale over its %lld covering segments at most, ascending, / sum of w^2 where that is > 1e-10; lanes load consecutive bins and store consecutive "
               "samples; no workspace, no partial sums, no atomics; lds=%zuB; %s; 8 algorithmic bytes per bin read and 4 per sample written\n",
            (long long)(d.batch / d.mean_batch), (long long)d.mean_batch, (long long)d.nx / 2 + 1, plan->w_pitch, g.span, (long long)d.seg_hop, kWThreads,
            (long long)(d.batch / d.mean_batch), g.wgs, g.NS, (long long)d.nx / 2, seg_radices(plan).c_str(), g.F, g.R - 1, g.R, plan->w.lds, kOResources);
}
static void describe_fastf(const xrfthip_plan* plan, std::string& s, const char*) {
    const xrfthip_desc& d = plan->d;
    const bool cols = filter_cols(plan);
    appendf(s, "  [fastw overlap-save] FIR filter, one pass: %lld series of N = %lld samples (series pitch %lld) to %lld samples each from sample %lld of the full convolution, "
               "K = %lld taps, segments of L = %lld samples of which V = %lld are kept; one %d-thread workgroup per (series, run): %lld x %lld workgroups, %lld segments "
               "per tile, each read where it lies with guarded 4-byte loads (zeros outside the series) and packed with itself as a %lld-point sequence; radix %s in "
               "place, per pair (k, n - k) unpacked, multiplied by the response (%s), packed and conjugated in registers and stored in natural order, radix %s again; "
               "lanes store consecutive samples, each written once; no workspace, no second tile, no atomics; lds=%zuB; %s; 4 algorithmic bytes per sample read and 4 per "
               "sample written\n",
            (long long)(d.batch / d.mean_batch * (cols ? d.inner : 1)), (long long)d.seg_in_len, plan->w_pitch, (long long)d.seg_out_len, (long long)d.seg_lead, (long long)(d.nx - d.seg_hop + 1),
            (long long)d.nx, (long long)d.seg_hop, kWThreads, (long long)(d.batch / d.mean_batch * (cols ? plan->w.ngroups : 1)), filter_wgs(d), (long long)(2 * kWPoints / d.nx), (long long)d.nx / 2,
            seg_radices(plan).c_str(), plan->phase[1].p ? "L / 2 + 1 complex64 entries" : "none set: ones, a delay", seg_radices(plan).c_str(), plan->w.lds, kFResources);
    // (the column layout: the series above are the columns of all blocks, the pitch the block pitch, a "series" of the workgroup count a group of columns)
    if (cols) describe_cols(plan, s, "segments", "segment", (std::string("the result is [block][sample][column], the array's own order: loads and stores coalesced across columns, no transposed copy; ") + kFColsResources).c_str());
}
static void describe_fastt(const xrfthip_plan* plan, std::string& s) {
    const xrfthip_desc& d = plan->d;
    const TaperGeom g = taper_geom(d);
    std::string rad;
    for (int r : plan->tables.at((int)d.nx).radix) appendf(rad, "%s%d", rad.empty() ? "" : "x", r);
    appendf(s, "  [fastw tapers] multitaper spectra, one pass: %lld series of N = %lld samples (series pitch %lld) under K = %lld tapers (%s), zero-extended to L = %lld; "
               "one %d-thread workgroup per %d series: %lld workgroups, %d pairs of tapers per series packed (t_2q x + i t_2q+1 x) as %d sequences of an LDS tile in %d "
               "round(s), detrend over the N samples once per series (%d threads each, float64), radix %s in place, |Z|^2 (Z conj Z') summed in %d float32 registers per "
               "thread, then float64 per series and frequency, symmetrised, fftshift / half output in the same kernel; no workspace, no second kernel, no atomics; ",
            (long long)d.batch, (long long)d.seg_taper_len, plan->w_pitch, (long long)d.seg_tapers, plan->w_taps.p ? "table set" : "NO TABLE: xrfthip_plan_set_tapers",
            (long long)d.nx, kWThreads, g.NS, g.wgs, g.KP, g.seqs, g.rounds, g.tps, rad.c_str(), kWAcc * (d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1));
    appendf(s, "lds=%zuB; %s; 4 algorithmic bytes per sample read and one spectrum per series written\n", plan->w.lds, kTResources);
}
static void describe_fastw(const xrfthip_plan* plan, std::string& s, const char*) {
    if (taper_plan(plan)) return describe_fastt(plan, s);
    const xrfthip_desc& d = plan->d;
    const SegGeom& g = plan->w;
    appendf(s, "  [fastw] Welch spectra, one pass: %lld series of %lld segments of %lld samples, hop %lld (series pitch %lld), each segment read where it lies with 4-byte loads; "
               "one %d-thread workgroup per run, %d segments per round packed in pairs (a + i b) as %d sequences of an LDS tile, detrend and window in the tile, radix "
               "%s in place, |Z|^2 (Z conj Z') summed in %d float32 registers per thread, the pair symmetrised once by fastw_finish; lds=%zuB; "
               "fastw_kernel: 115 VGPRs, no scratch, 4 waves per SIMD (two fields: 164 VGPRs, 3 waves); 4 algorithmic bytes per sample of the series through memory\n",
            (long long)(d.batch / d.mean_batch), (long long)d.mean_batch, (long long)d.nx, (long long)d.seg_hop, plan->w_pitch, kWThreads, 2 * g.seqs, g.seqs,
            seg_radices(plan).c_str(), kWAcc * (d.out_mode == XRFTHIP_OUT_CROSS ? 2 : 1), g.lds);
    describe_cols(plan, s, "pairs of segments", "pair", (std::string("the float64 sums per column; fastw_kernel<cols>: ") + kWColsResources).c_str());
}
static void info_fastw(const xrfthip_plan* plan, int32_t* k, int32_t* n) { *k = XRFTHIP_K_FASTW; *n = taper_plan(plan) ? taper_geom(plan->d).NS : 2 * plan->w.seqs; }  // (per_workgroup: the segments of a round)
static void info_fastk(const xrfthip_plan* plan, int32_t* k, int32_t* n) { *k = XRFTHIP_K_FASTW; *n = plan->w.seqs; }
// (the entries in the order of struct FamilyOps; reads_strided is false -- the series pitch is w_pitch, d.in_stride_batch is 0 -- and the last entry, no_generic_passes, true)
static int finalize_fastk(xrfthip_plan* P) { return synth_plan(P) || filter_plan(P) ? XRFTHIP_OK : fast_phase_tables(P); }  // (the synthesis takes no phase table; the filter's is its response, read as it was set)
#ifndef __HIP_DEVICE_COMPILE__  /* host data: the device pass would emit a const object, and the launchers it points to do not exist there */
const FamilyOps kOpsFastW = {Family::FastW, run_fastw, describe_fastw, info_fastw, fast_phase_tables, layout_fastw, nullptr, nullptr, false, nullptr, false, false, false, false, true};
const FamilyOps kOpsFastK = {Family::FastK, run_fastk, describe_fastk, info_fastk, finalize_fastk, layout_fastk, nullptr, nullptr, false, nullptr, false, false, false, false, true};
#endif

// kernels of this unit that take more than 64 KB of dynamic LDS (two tiles of 4096 points and their padding): called once through set_kernel_attrs_once()
void set_attrs_welch() {
    const int m = (int)kLdsMax;
#define SETF(K) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, m)
    SETF((fastw_kernel<false>)); SETF((fastw_kernel<true>)); SETF((fastw_kernel<false, true>)); SETF((fastw_kernel<true, true>));
    SETF((fastt_kernel<false>)); SETF((fastt_kernel<true>));
    SETF((fastk_kernel<true, false>)); SETF((fastk_kernel<false, false>)); SETF((fastk_kernel<true, true>)); SETF((fastk_kernel<false, true>));
#undef SETF
}
