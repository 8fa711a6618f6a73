/*
 * xrft_hip.h -- C ABI of libxrft_hip.so: the MI355X (gfx950) spectral engine behind the xrft API.
 *
 * The reference (xgcm/xrft) is pure Python and has no FFI of its own.  The seam this library replaces is
 * the array-backend module returned by `_fft_module` (reference xrft/xrft.py:32-36) together with the
 * full-array numpy passes `xrft.fft` / `power_spectrum` / `cross_spectrum` / `isotropize` / `detrend`
 * wrap around it.  One plan executes, fused on the device, what the reference does in these steps:
 *
 *   detrend (constant | linear)            xrft/detrend.py:54-55, 64-71, 100-113
 *   window multiply                        xrft/xrft.py:96-103
 *   flip + ifftshift of the input          xrft/xrft.py:436-441   (true_phase)
 *   fftn / rfftn over the last 1-2 axes    xrft/xrft.py:439-444
 *   fftshift                               xrft/xrft.py:446-447
 *   x exp(-i 2 pi k lag), x prod(dx)       xrft/xrft.py:462-472
 *   |F|^2  or  F1 conj(F2), real-dim x2,
 *   / window correction, x prod(dk)        xrft/xrft.py:740-748, 825-833
 *   radial bin-sum                         xrft/xrft.py:895-906, 993-1004
 *
 * Conventions
 *   - every `d_*` pointer is a DEVICE pointer owned by the caller (e.g. torch tensor .data_ptr());
 *     every `h_*` pointer is a HOST pointer, copied during the call;
 *   - arrays are C-contiguous [batch][ny][nx] (ny == 1 for 1-D transforms); the transform runs over the
 *     last `ndim` axes; `batch` slabs are independent;
 *   - a plan is immutable once created and its tables are set: xrfthip_plan_create and the xrfthip_plan_set_* calls build
 *     every device table and the workspace layout (allocations, blocking copies, environment lookups happen THERE);
 *     xrfthip_exec takes the plan as const, never allocates, never copies from the host, never synchronises, reads no
 *     environment variable and enqueues everything on `stream` (a hipStream_t passed as void*; NULL = the default
 *     stream).  It can be captured into a hipGraph from its first call, and one plan can be executed from several
 *     threads at once, each with its own stream and workspace (exception: a plan with profiling switched on records
 *     events into itself and is not re-entrant);
 *   - all functions return 0 on success or a negative xrfthip_status; nothing throws or aborts.
 *
 * Python binding: xrft_amd/_lib.py (ctypes).  A reference-side binding sketch is in INTEGRATION.md.
 */
#ifndef XRFT_HIP_H
#define XRFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XRFTHIP_VERSION 106 /* 0.1.6: the inner / mid layouts take OUT_CROSS (two real fields) and XRFTHIP_HALF_X / REALDIM_X2 (real_dim along the second axis) on their fused passes; 0.1.5: xrfthip_selftest_floor; 0.1.4: XRFTHIP_AXIS_Y with XRFTHIP_HALF_X / REALDIM_X2 (real_dim along the one transformed axis); 0.1.3: xrfthip_desc.mid (two transform axes anywhere in a C-contiguous array); 0.1.2: xrfthip_plan_uses_bluestein, xrfthip_convert (0.1.1: xrfthip_desc.inner, xrfthip_reduce_axis, xrfthip_detrend_inner) */

typedef enum xrfthip_status {
    XRFTHIP_OK = 0,
    XRFTHIP_BAD_ARG = -1,
    XRFTHIP_UNSUPPORTED_LENGTH = -2, /* a prime factor above XRFTHIP_MAX_RADIX whose Bluestein transform (2^a 3^b 5^c >= 2n-1) does not fit the LDS */
    XRFTHIP_WORKSPACE_TOO_SMALL = -3,
    XRFTHIP_HIP_ERROR = -4, /* see xrfthip_last_hip_error() */
    XRFTHIP_ALLOC_FAILED = -5,
    XRFTHIP_MISSING_TABLE = -6 /* flag needs a table that was not set (window, phase, bin map) */
} xrfthip_status;

#define XRFTHIP_MAX_RADIX 128

typedef enum xrfthip_dtype { /* dtype of the input array; the arithmetic runs in the matching precision */
    XRFTHIP_F32 = 0,
    XRFTHIP_F64 = 1,
    XRFTHIP_C64 = 2,
    XRFTHIP_C128 = 3,
    /* Real half-precision input, read where it lies at 2 bytes per sample and widened to float32 in registers (exact: every float16 / bfloat16 value is a float32
     * value).  Accepted as xrfthip_desc.dtype and as dtype_in of xrfthip_convert only (no symbol and no version number tells the capability: an older library answers
     * XRFTHIP_BAD_ARG).  A plan with one of them IS the float32 plan of the same descriptor -- same family, kernels behind the loads, workspace, tables, and
     * float32 / complex64 output (d_iso float64 / complex128) -- and its result is bit-identical to that plan's on the widened samples, NaN payloads aside.
     *   XRFTHIP_UNSUPPORTED_LENGTH ("the caller widens": xrfthip_convert to XRFTHIP_F32, then the float32 plan) from xrfthip_plan_create, or from the xrfthip_plan_set_*
     *   call that moves the plan there: every family but the float32 ones that read 2-byte samples -- FASTY (two-pass slabs and the four-step 1-D form), FASTS, FASTR,
     *   FASTG / FASTG_ROWS with real input -- hence also XRFTHIP_AXIS_Y, inner / mid, and a non-zero in_stride_y / in_stride_batch: a strided half view is NOT read
     *   in place (copy it contiguous in half precision, 2 bytes per sample, or widen it).
     *   XRFTHIP_BAD_ARG as for real float32 input: XRFTHIP_INVERSE, XRFTHIP_C2R_X, XRFTHIP_PHASE_IN, herm_ny / herm_nx (complex input only).
     *   Alignment, in bytes: d_in0 (and d_in1) 16-byte aligned -- xrfthip_exec checks and answers XRFTHIP_UNSUPPORTED_LENGTH otherwise, reading nothing; the kernels issue
     *   aligned 8-byte (FASTY: four samples) and 4-byte (two samples) vector loads, 2-byte loads only for an odd row length of FASTG, and touch no byte outside
     *   [d_in, d_in + 2 * batch * ny * nx).  d_in0 and d_in1 of a CROSS / PHASE plan hold the same format. */
    XRFTHIP_F16 = 4, /* IEEE binary16 */
    XRFTHIP_BF16 = 5 /* bfloat16: the upper half of a float32 */
} xrfthip_dtype;

typedef enum xrfthip_out_mode {
    XRFTHIP_OUT_COMPLEX = 0, /* F                    -> complex (c64 | c128)          xrft.fft            */
    XRFTHIP_OUT_POWER = 1,   /* |F|^2 * scale        -> real    (f32 | f64)           xrft.power_spectrum */
    XRFTHIP_OUT_CROSS = 2,   /* F0 conj(F1) * scale  -> complex                       xrft.cross_spectrum */
    XRFTHIP_OUT_PHASE = 3,   /* arg(F0 conj(F1))     -> real, in [-pi, pi]            xrft.cross_phase (xrft.py:838-874) */
    XRFTHIP_OUT_COHERENCE = 4 /* |<F0 conj F1>|^2 / (<|F0|^2> <|F1|^2>) -> real (f32), <.> the mean over mean_batch slabs: mean plans only (xrfthip_desc.mean_batch) */
} xrfthip_out_mode;

typedef enum xrfthip_detrend_kind {
    XRFTHIP_DETREND_NONE = 0,
    XRFTHIP_DETREND_CONSTANT = 1, /* subtract the mean over the transform axes, per slab  detrend.py:54-55 */
    XRFTHIP_DETREND_LINEAR = 2    /* subtract the least-squares line (1-D) / plane (2-D)  detrend.py:64-113 */
} xrfthip_detrend_kind;

/* flags */
#define XRFTHIP_HALF_X 0x001u   /* rfftn: keep only kx = 0..nx/2 along the last axis (real input only; no shift) */
#define XRFTHIP_SHIFT_Y 0x002u  /* fftshift the output along y (xrft.py:446-447) */
#define XRFTHIP_SHIFT_X 0x004u  /* fftshift the output along x */
#define XRFTHIP_ISHIFT_Y 0x008u /* ifftshift the input along y (true_phase, xrft.py:440) */
#define XRFTHIP_ISHIFT_X 0x010u /* ifftshift the input along x */
/* On an XRFTHIP_INVERSE plan ISHIFT_* rotates the (fftshifted) input samples themselves; a window and an XRFTHIP_PHASE_IN table are indexed by the SOURCE position
 * of a sample, before the rotation: sample s is multiplied by window[s] (and phase[s]) and then moved to (s - n/2) mod n (n/2 rounded down), as
 * numpy.fft.ifftshift of the windowed input does.  A forward plan computes the same; a family may fold the rotation of an even n into the output as the sign (-1)^k.
 * The one-axis kernel families index a window by the transform's own sample: xrfthip_plan_set_window hands an inverse plan with ISHIFT along the windowed axis to
 * the generic passes (xrfthip_plan_kernel_info says so), and answers XRFTHIP_BAD_ARG, leaving the plan without that window, where there is no generic form
 * (XRFTHIP_AXIS_Y with XRFTHIP_PHASE_IN, below).
 * Without XRFTHIP_PHASE_IN the phase tables multiply the RESULT of an inverse plan as they do a forward plan's: out[k] = phase[k] * ifft(...)[k] * scale. */
#define XRFTHIP_FLIP_Y 0x020u   /* np.flip the input along y before the ifftshift (descending coordinate); CROSS/PHASE: field 1 (d_in1) */
#define XRFTHIP_FLIP_X 0x040u   /* np.flip the input along x; CROSS/PHASE: field 1 */
#define XRFTHIP_REALDIM_X2 0x080u /* with HALF_X and POWER|CROSS: multiply by [1,2,...,2,(1)] (xrft.py:673-682) */
#define XRFTHIP_ISO 0x100u      /* radial bin-sum of the POWER|CROSS result into d_iso (needs a bin map) */
#define XRFTHIP_NO_SPECTRUM_OUT 0x200u /* with ISO: do not write the full spectrum (d_out may be NULL) */
/* inverse transforms (xrft.ifft, xrft.py:479-646); complex input, out_mode COMPLEX */
#define XRFTHIP_INVERSE 0x400u   /* ifftn: conj(FFT(conj(z))); the caller folds 1/prod(N) into `scale` */
#define XRFTHIP_C2R_X 0x800u     /* irfftn: d_in0 is [batch][ny][nx/2+1] complex, Hermitian-extended on the fly; d_out is REAL [batch][ny][nx] */
#define XRFTHIP_PHASE_IN 0x1000u /* the phase tables multiply the INPUT (indexed by source position) instead of the output (xrft.py:574-576) */
/* Transform along a middle (or the first) axis in place, no transposed copy (the reference transforms any axes of the array
 * where they lie, xrft.py:395-409): with ndim = 2 the array is [batch][ny][nx] and ONLY y is transformed, once per (slab,
 * column); nx is the product of the trailing axes.  Detrending and the window act along y (one line / mean per column);
 * the *_X flags, ISO and C2R_X do not apply (HALF_X / REALDIM_X2: see below).  Output [batch][ny][nx] in the same layout.
 * Inverse transforms along the axis (xrft.ifft of one first / middle axis, xrft.py:479-646): XRFTHIP_INVERSE with complex input; ISHIFT_Y then
 * rotates the fftshifted INPUT rows, SHIFT_Y the output; XRFTHIP_PHASE_IN (the lag's phase on the input, axis 0 table) is accepted where a one-pass
 * kernel takes the plan (any smooth ny that fits a tile, Bluestein lengths included) and XRFTHIP_BAD_ARG otherwise -- the caller then transposes.
 * real_dim along the axis (0.1.4; xrft.py:400-404, 673-682): XRFTHIP_HALF_X with AXIS_Y keeps k = 0 .. ny/2 of the ONE transformed axis -- output
 * [batch][ny/2 + 1][nx], unshifted, real input, no SHIFT_Y / FLIP_Y / INVERSE -- and REALDIM_X2 counts 0 < k < ny/2 twice; accepted where a one-pass
 * kernel takes the plan, XRFTHIP_UNSUPPORTED_LENGTH otherwise (the caller transposes). */
#define XRFTHIP_AXIS_Y 0x2000u
/* CROSS/PHASE: the reference flips each field by its own coordinate (xrft.py:436-441): these flip field 0 (d_in0), FLIP_Y /
 * FLIP_X flip field 1 (d_in1).  The window always multiplies in the source order, before the flip (xrft.py:425-441). */
#define XRFTHIP_FLIP0_Y 0x4000u
#define XRFTHIP_FLIP0_X 0x8000u
/* inner / mid layouts only (ABI 0.1.6): real_dim along the FIRST of the two transform axes -- ky = 0..ny/2 is stored, output [batch][ny/2 + 1][mid][nx][inner], unshifted;
 * with REALDIM_X2 and POWER|CROSS 0 < ky < ny/2 counts twice.  Real input, no SHIFT_*, not together with HALF_X.  ny may be odd: ky = 0..(ny-1)/2 is stored
 * (numpy.fft.rfft's (ny-1)/2 + 1 rows, no Nyquist row), and every ky > 0 counts twice; XRFTHIP_UNSUPPORTED_LENGTH where only the composite of one-axis plans exists. */
#define XRFTHIP_HALF_Y 0x10000u
/* herm_ny / herm_nx descriptors only: the last pass writes the complex FIELD F itself (out_mode COMPLEX), not |F|^2 or F0 conj(F1) -- see herm_ny below. */
#define XRFTHIP_HERM_FIELD 0x20000u

typedef struct xrfthip_desc {
    uint32_t struct_size; /* = sizeof(xrfthip_desc) */
    int32_t ndim;         /* 1 or 2: number of trailing axes transformed */
    int64_t batch;        /* independent slabs */
    int64_t ny;           /* 1 when ndim == 1 */
    int64_t nx;
    int32_t dtype;    /* xrfthip_dtype of d_in0 / d_in1 */
    int32_t out_mode; /* xrfthip_out_mode */
    int32_t detrend;  /* xrfthip_detrend_kind */
    uint32_t flags;
    double scale;            /* COMPLEX: multiplies F (prod(dx) for true_amplitude); POWER/CROSS: multiplies the product */
    int32_t slabs_per_group; /* 0 = auto: slabs pushed through all passes together (keeps the intermediate in MALL); a two-pass plan with XRFTHIP_ISO runs at most 65535 per group (xrfthip_plan_describe: group=) */
    int32_t reserved;
    /* Layout with the independent elements INNERMOST: with inner > 1 the arrays are [batch][ny][nx][inner] and the transform runs over
     * (ny, nx) for every (batch, inner) element -- two ADJACENT transform axes anywhere in a C-contiguous array (the reference transforms
     * any axes where they lie, xrft/xrft.py:395-409), e.g. dim = ["y", "x"] of a (y, x, time) array: batch = 1, inner = nt.  No transposed
     * copy is made: x is transformed where it lies ([batch ny][nx][inner], as XRFTHIP_AXIS_Y does for one axis), then y
     * ([batch][ny][nx inner]); a detrend runs first as a pass of its own.  ndim = 2, out_mode COMPLEX | POWER, flags SHIFT_* /
     * ISHIFT_* / FLIP_*; windows, phases and `scale` as usual.  ABI 0.1.6: real input of a smooth shape (the two fused passes) also takes out_mode CROSS
     * (d_in1 = the second field, same layout) and XRFTHIP_HALF_X / REALDIM_X2 (real_dim along the SECOND transform axis: output [batch][ny][mid][nx/2 + 1][inner],
     * unshifted) or XRFTHIP_HALF_Y (along the FIRST: [batch][ny/2 + 1][mid][nx][inner]); XRFTHIP_UNSUPPORTED_LENGTH where only the composite of one-axis plans exists (the caller transposes).  0 or 1 = the trailing-axes layout.  A descriptor with the
     * struct_size of the version without this field is accepted (inner = 1).
     * The fused passes also take XRFTHIP_ISO (+ XRFTHIP_NO_SPECTRUM_OUT) with out_mode POWER | CROSS, under `inner` and under `mid`: every (batch, mid | inner) element is a
     * spectrum of its own with radial sums of its own, d_iso = float64 | complex128 [batch][ne][nbins], ne = inner or mid -- the order of the array's other dims, then the bins
     * (xrft/xrft.py:1076-1095) -- every entry written; a true-phase factor (xrfthip_plan_set_phase) is carried per sample.  Not with HALF_X / HALF_Y / REALDIM_X2; where the fused
     * passes decline the descriptor (mid > 1 AND inner > 1, a length outside 16 .. 8192 or with a prime factor they have no butterfly for, a flipped axis):
     * XRFTHIP_UNSUPPORTED_LENGTH, the caller transposes.  No symbol and no version number tells this capability apart: the status of xrfthip_plan_create does. */
    int64_t inner;
    /* ... and `mid` independent elements BETWEEN the two transform axes (ABI 0.1.3): with inner > 1 or mid > 1 the arrays are
     * [batch][ny][mid][nx][inner] -- batch = the product of the extents in front of the first transform axis, mid of those between the two, inner of those
     * behind the second -- which is every way two transform axes can lie in a C-contiguous array of any rank (xrft/xrft.py:395-409 transforms any axes where
     * they lie): dim = ["t", "x"] of a (t, y, x) array is batch = 1, ny = nt, mid = ny, nx = nx, inner = 1.  Same plan as `inner` alone: x where it lies, then y
     * where it lies, a detrend (one plane over (ny, nx) per (batch, mid, inner) element) first as a pass of its own; no transposed copy.  0 or 1 = none.
     * Descriptors with the struct_size of the versions without `mid` / without `inner` are accepted. */
    int64_t mid;
    /* Input strides: a box cut out of a larger field (da.isel(y=slice(..), x=slice(..)), the reference transforms any view numpy hands it, xrft/xrft.py:439-444) is
     * read where it lies, with no contiguous copy.  Both describe d_in0, and d_in1 of a CROSS / PHASE plan (one set of strides for the two fields); the x stride is
     * always 1; d_out, d_iso and the workspace stay dense.  xrfthip_exec never writes its input, so a batch stride SMALLER than a slab (overlapping windows of one
     * buffer) is legal.
     *   in_stride_y     elements of `dtype` between consecutive rows y of one slab; 0 = nx (nx/2 + 1 of a C2R_X plan)
     *   in_stride_batch elements between consecutive slabs; 0 = ny * nx
     * XRFTHIP_BAD_ARG: a negative stride; 0 < in_stride_y < the row length; a non-zero stride together with inner > 1, mid > 1 or XRFTHIP_AXIS_Y (those layouts stay
     * dense).  XRFTHIP_UNSUPPORTED_LENGTH means "the caller copies": ny * in_stride_y above 2^31 - 1 elements or 2^32 - 1 bytes (the index math inside a slab is 32-bit),
     * a stride that is not a multiple of 16 bytes (every vector load of the kernels stays one aligned instruction: there is no scalar path), or a kernel family that
     * does not read strided input.  The family is chosen as for the dense descriptor of the same shape and NEVER changed because of the strides: a strided plan runs
     * the same kernels, slabs_per_group and arithmetic as the dense plan, and its result is bit-identical to that plan's on a contiguous copy.  The families that read
     * strided input, real float32 / float64 data in every mode they serve: FastY, FastM, FastN (xrfthip_kernel_kind FASTY / FASTM / FASTN on 2-D plans), FastS, FastG
     * (slabs and row groups, real input) and FastR (real rows: in_stride_batch only).  A table set later that moves the plan to a family outside this list (the
     * generic passes) answers XRFTHIP_UNSUPPORTED_LENGTH from that xrfthip_plan_set_* call.  Strides equal to the dense ones are the dense plan.
     * A strided plan needs d_in0 (and d_in1) 16-byte aligned: xrfthip_exec checks and answers XRFTHIP_BAD_ARG.  The kernels touch no byte outside the rows of the view.
     * Descriptors with the struct_size of the three earlier versions are accepted (strides 0).  As with `inner` / `mid`, no symbol and no version number tells this
     * capability apart: the status of xrfthip_plan_create does (an older library answers XRFTHIP_BAD_ARG to the larger struct_size). */
    int64_t in_stride_y;
    int64_t in_stride_batch;
    /* The last stage of a power / cross spectrum over THREE axes (t, y, x) of a real field (xrft.power_spectrum(da, dim=["time", "y", "x"]), xrft/xrft.py:685-835; numpy's
     * fftn over three axes, xrft.py:439-447): the columns of an XRFTHIP_AXIS_Y plan are the HALF spectrum of a real herm_ny x herm_nx grid -- what a two-axis plan with
     * XRFTHIP_HALF_X and out_mode COMPLEX wrote, unshifted -- and the plan transforms them along t, takes |F|^2 * scale (POWER) or F0 conj(F1) * scale (CROSS, d_in1 = the
     * second field's half spectrum) and writes the FULL result, the redundant half from the Hermitian twin (-kt, -ky, -kx): the conjugate for CROSS.
     *   herm_ny, herm_nx   the real grid (0, 0 = off: both or neither); d_in0 / d_in1 are [batch][nt][herm_ny][herm_nx/2 + 1] complex,
     *                      d_out is real (POWER) or complex (CROSS) [batch][nt][herm_ny][herm_nx], every element written exactly once
     * Valid with XRFTHIP_AXIS_Y, ndim = 2, ny = nt, nx = herm_ny * (herm_nx/2 + 1), dtype C64 | C128, out_mode POWER | CROSS, no detrend.  Flags: XRFTHIP_SHIFT_Y fftshifts
     * the result along t and XRFTHIP_ISHIFT_Y rotates the input rows along t, as on every AXIS_Y plan; XRFTHIP_SHIFT_X here means "fftshift the two Hermitian axes of the
     * result" (the reference shifts all transform axes or none, xrft.py:446-447).  A window along t (axis 0) multiplies the source rows.
     * XRFTHIP_BAD_ARG: one of the two fields without the other or a negative one; any other flag, in_stride_*, inner / mid, a detrend, out_mode COMPLEX | PHASE, real input, an
     * nx that is not herm_ny * (herm_nx/2 + 1); xrfthip_plan_set_phase (the twin of a sample at a Nyquist index does not carry the conjugate phase factor) and a window on
     * axis 1.  XRFTHIP_UNSUPPORTED_LENGTH means "the caller composes the stages": an nt with a prime factor above 13, or whose tile of 128 output bytes per row does not fit
     * the LDS (nt above ~600).  One pass, no workspace, no sums: repeated calls return identical bits.
     * Descriptors with the struct_size of the four earlier versions are accepted (0, 0).  As with the strides, the status of xrfthip_plan_create tells the capability.
     * XRFTHIP_HERM_FIELD: the same pass writes the transform itself (xrft.fft(da, dim=["time", "y", "x"])): out_mode COMPLEX and nothing else (POWER | CROSS | PHASE
     * with the flag: XRFTHIP_BAD_ARG, as is the flag on a descriptor without herm_ny / herm_nx); d_out is complex [batch][nt][herm_ny][herm_nx], F * scale, the
     * columns 1 <= kx <= herm_nx - (herm_nx/2 + 1) also written as the twin conj(F) * scale at (-kt, -ky, herm_nx - kx).  Such a plan takes THREE output-phase tables,
     * xrfthip_plan_set_phase with axis = 0 (t: ny entries), 1 (herm_ny entries) and 2 (herm_nx entries: the FULL x axis, the twins lie above herm_nx/2), each indexed by
     * UNSHIFTED frequency index; an axis without a table counts as 1.  A twin is multiplied by the factors of its DESTINATION indices, not by the conjugate of its
     * sample's (an index n/2 of an even n is its own twin: fftfreq gives it -1/(2 dx) both times); without tables the twin is the plain conjugate, bit for bit.
     * axis 2 is XRFTHIP_BAD_ARG on every other plan; a window stays on axis 0 only.  The same lengths are declined (XRFTHIP_UNSUPPORTED_LENGTH); the tile is 128 nt
     * bytes.  Without the flag every answer a herm descriptor gets is what it was: out_mode COMPLEX and xrfthip_plan_set_phase stay XRFTHIP_BAD_ARG. */
    int64_t herm_ny;
    int64_t herm_nx;
    /* The mean over the batch inside the last pass: what the reference's users do with a batch of spectra (xrft.power_spectrum(..., chunks_to_segments=True).mean("x_segment"),
     * ps.mean(["time", "y_segment", "x_segment"]): the Parseval, chunk and MITgcm notebooks) without the spectra of the single slabs ever reaching memory.
     *   mean_batch = M > 1   every M consecutive slabs b = o * M + m give ONE output: d_out is [batch / M][ny][nx], real (POWER) or complex (CROSS), its value
     *                        (1 / M) sum_m of what the plan without the field writes for slab o * M + m; shifts, detrend, windows, `scale` and the phase tables of a
     *                        cross spectrum behave as on that plan.  0 or 1 = off; 1 is the plain plan itself, bit for bit (same family, same launches).
     * XRFTHIP_BAD_ARG: a negative M, batch % M != 0, out_mode COMPLEX | PHASE, XRFTHIP_ISO.  XRFTHIP_UNSUPPORTED_LENGTH means "the caller composes" (the plain plan, then
     * xrfthip_reduce_axis with scale = 1 / M): every kernel family without a mean form -- all but the two-pass float32 slabs (XRFTHIP_K_FASTY on 2-D plans; float16 /
     * bfloat16 and strided input included: the column pass is the plain plan's) and the one-pass float32 slabs of 64 | 128 points per axis (XRFTHIP_K_FASTS, dense
     * float32 input, POWER; a 256 x 256 mean plan is served by FASTY) -- hence also XRFTHIP_HALF_X / REALDIM_X2, XRFTHIP_AXIS_Y, inner / mid and herm_*, and more than 2^31 - 1 output rows ((batch / M) * ny); a later
     * xrfthip_plan_set_* call that would move the plan to such a family answers the same.  Of these classes a plan takes, by default, those whose mean form measured
     * not slower than the composition it replaces (profiles/r15_batch_mean.txt: every FASTY class; FASTS slabs of 128 rows); FASTS slabs of 64 rows answer
     * XRFTHIP_UNSUPPORTED_LENGTH as well unless XRFTHIP_MEAN_ALL=1 is in the environment when the plan is created (docs/TUNING.md).
     * Sums: no floating-point atomics; the order of every addition is fixed by the plan (M, the groups of slabs, the runs per output that xrfthip_plan_describe prints),
     * so repeated calls return identical bits; at most 16 float32 terms are added in a row before the sum continues in float64 (complex128); a non-finite value in one
     * slab makes exactly its own output non-finite.  The partial sums live in the workspace (xrfthip_workspace_bytes includes them: P float64 half spectra per output).
     * xrfthip_plan_pass1_bytes keeps working on a mean plan (the column pass is unchanged).
     * Descriptors with the struct_size of the five earlier versions are accepted (0).  As with the strides and herm_*, the status of xrfthip_plan_create tells the
     * capability: an older library answers XRFTHIP_BAD_ARG to the larger struct_size. */
    int64_t mean_batch;
    /* The magnitude-squared coherence of two fields, out_mode = XRFTHIP_OUT_COHERENCE: what a batch of cross spectra is averaged for, the other half of the pair that
     * XRFTHIP_OUT_PHASE begins.  Valid only with mean_batch = M > 1 (no new field: the mode is a value of out_mode, and the status of xrfthip_plan_create tells the
     * capability -- an older library answers XRFTHIP_BAD_ARG to out_mode 4).  Two real input fields (d_in0, d_in1, as CROSS; xrfthip_exec without d_in1 answers as
     * CROSS does); d_out is real float32 [batch / M][ny][nx],
     *   gamma^2 = |sum_m F0 conj(F1)|^2 / (sum_m |F0|^2  sum_m |F1|^2)   over the M slabs of an output,
     * from ONE row pass that reads each field's intermediate once and keeps four sums per sample (re C, im C, A, B) where CROSS keeps two; the composition it replaces
     * is three mean plans (CROSS, POWER of each field) and xrfthip_coherence.  Shifts, detrend and windows behave as on the CROSS mean plan; `scale` is applied inside
     * the sums (|scale| in A and B) to keep them in range and cancels in the result, as does 1 / M; phase tables are accepted and have no effect (a factor of modulus
     * one common to the M slabs leaves |<.>|^2 unchanged).  No clamp: a value may exceed 1 by rounding, and a zero denominator gives what IEEE division gives.
     * XRFTHIP_BAD_ARG: mean_batch <= 1 (of one spectrum the coherence is 1 everywhere; M = 1 is normalised to 0 and has no plain plan to stand for), batch % M != 0,
     * XRFTHIP_ISO, and every descriptor to which CROSS answers XRFTHIP_BAD_ARG (XRFTHIP_INVERSE, an unknown detrend, ...).  XRFTHIP_UNSUPPORTED_LENGTH ("the caller
     * composes"): every plan whose family is not the two-pass float32 slabs (XRFTHIP_K_FASTY on a 2-D plan) -- float64, complex fields, slabs of 64 | 128 points on an axis (the
     * one-pass kernel has no two-field form), XRFTHIP_HALF_X / REALDIM_X2, XRFTHIP_AXIS_Y, inner / mid, herm_* -- and a later xrfthip_plan_set_* call that would move
     * the plan to another family answers the same.  float16 / bfloat16 and strided input are taken as the CROSS mean plan takes them (the column pass is the plain
     * plan's).  Sums as above: no atomics, a fixed order, at most 16 float32 terms in a row, then float64; the partial is 4 float64 per sample and run
     * ([output][P][ny/2 + 1][nx][re C, im C, A, B], in xrfthip_workspace_bytes); a non-finite value in one slab makes exactly its own output non-finite.
     * xrfthip_plan_describe prints the [mean over the batch] line and the word "coherence".  XRFTHIP_MEAN_ALL and XRFTHIP_MEAN_RUNS apply as they do to CROSS. */
    /* Welch spectra: the mean spectrum of the OVERLAPPING segments of a long series, each segment read where it lies and no segment's spectrum ever stored -- Welch's
     * method (scipy.signal.welch / csd), the reference's power_spectrum(da, dim="time", chunks_to_segments=True, window="hann", detrend="linear").mean("time_segment")
     * with an overlap.  One in_stride_batch cannot say "series pitch and segment hop", hence the field.
     *   seg_hop = H >= 1   samples between the starts of consecutive segments.  Valid with ndim = 1, ny = 1, nx = L (the segment length), mean_batch = M >= 2 (the
     *                      segments per series), batch = P * M (P series), dtype XRFTHIP_F32, out_mode POWER | CROSS.  Input sample j of segment s of series p is
     *                      d_in0[p * in_stride_batch + s * H + j] (and d_in1 of a CROSS plan): in_stride_batch is HERE the series pitch, 0 = the dense span
     *                      (M - 1) * H + L.  d_out is [P][nx_out], real (POWER) or complex (CROSS), its value (1 / M) sum_s of what the plain 1-D plan writes for
     *                      segment s.  Any 1 <= H <= L: H = L is the reshape of chunks_to_segments, H = L / 2 Welch's usual half overlap.
     *                      0 = off: everything is as without the field (a 1-D mean_batch plan answers XRFTHIP_UNSUPPORTED_LENGTH).
     * Alignment: d_in0 / d_in1 4-byte aligned, whatever H and the pitch are (the kernel loads single samples); no byte outside [p * pitch, p * pitch + (M - 1) * H + L)
     * of each series is touched.  Accepted: detrend NONE | CONSTANT | LINEAR per segment, as the 1-D plans define it; a window on axis 1; `scale`; XRFTHIP_SHIFT_X;
     * XRFTHIP_HALF_X with or without XRFTHIP_REALDIM_X2 (the one-sided spectrum, nx_out = L / 2 + 1; not together with SHIFT_X); XRFTHIP_ISHIFT_X (a factor (-1)^k
     * that cancels in both products: no effect); a phase table on axis 1 for CROSS (the net factor multiplies the mean, once).
     * XRFTHIP_BAD_ARG: H < 0, H > L; seg_hop with ndim = 2, XRFTHIP_AXIS_Y, inner (without seg_stride, below) / mid, herm_*, XRFTHIP_ISO or in_stride_y; mean_batch < 2; batch % M != 0;
     * out_mode COMPLEX | PHASE | COHERENCE; a pitch smaller than the span.  XRFTHIP_UNSUPPORTED_LENGTH ("the caller composes": the segments copied out, the plain
     * 1-D plan, xrfthip_reduce_axis): L not a power of two in 64 .. 4096, float64 / complex / float16 / bfloat16 input, the FLIP flags.
     * Sums: no floating-point atomics; the order of every addition is fixed by the plan, so repeated calls return identical bits; at most 16 float32 terms are added in
     * a row before the sum continues in float64; a non-finite sample makes exactly its own series' output non-finite.  The runs per output (xrfthip_plan_describe;
     * XRFTHIP_MEAN_RUNS pins them) let a few long series fill the card; their float64 partials live in the workspace (xrfthip_workspace_bytes includes them).
     * Served by the Welch form of the rows family (xrfthip_plan_kernel_info: XRFTHIP_K_FASTW).  Descriptors with the struct_size of the six earlier versions are accepted (0).  As with mean_batch, the status of
     * xrfthip_plan_create tells the capability: an older library answers XRFTHIP_BAD_ARG to the larger struct_size. */
    int64_t seg_hop;
    int64_t seg_reserved; /* 0 (anything else: XRFTHIP_BAD_ARG).  Appended together with seg_hop: no struct_size between the two */
    /* Welch spectra along a LEADING axis, read where it lies: the layout of a (time, y, x) cube or of (member, time, lat, lon), the spectrum along time at every
     * grid point, without a transposed copy of the cube.
     *   seg_stride = S >= 1   elements between consecutive SAMPLES of a series.  Valid with seg_hop = H >= 1 (and everything seg_hop asks for: ndim = 1, ny = 1,
     *                         nx = L, mean_batch = M >= 2, batch = P * M, mid = 1); `inner` = C_in >= 1 is the number of adjacent series ("columns") of a block,
     *                         S >= inner.  Sample j of segment s of column e of block p is d_in0[p * in_stride_batch + (s * H + j) * S + e] (and d_in1 of a CROSS
     *                         plan); in_stride_batch = 0 means ((M - 1) * H + L) * S, any other value is at least ((M - 1) * H + L - 1) * S + inner.  d_out is
     *                         [P][inner][nx_out], frequency last, real (POWER) or complex (CROSS): each (p, e) holds what the rows form (seg_hop alone) writes for
     *                         that series.  S > inner is a box of a wider grid; S = 1 with inner = 1 is the rows form itself, the same plan and the same bits.
     *                         0 = off: `inner` > 1 with seg_hop stays XRFTHIP_BAD_ARG.
     * Alignment: d_in0 / d_in1 4-byte aligned, any S, any inner, any pitch.  No byte outside the addressed samples is read: the gap between inner and S is never touched.
     * Accepted: everything the rows form accepts (detrend per segment, a window, `scale`, SHIFT_X, HALF_X with or without REALDIM_X2, ISHIFT_X without effect, a phase
     * table for CROSS).  XRFTHIP_BAD_ARG: S < 0, S > 0 with seg_hop = 0, S < inner, a pitch below the span above, seg_reserved2 != 0, and everything seg_hop refuses.
     * XRFTHIP_UNSUPPORTED_LENGTH ("the caller arranges -- one transposed copy, then the rows form -- or composes"): L not a power of two in 64 .. 512, everything the
     * rows form declines, XRFTHIP_FASTW_COLS=0 in the environment when the plan is created.
     * The sums are the rows form's: pairs of segments of the SAME column packed as a + i b, at most 16 float32 terms in a row, then float64, no atomics, a fixed order
     * (repeated calls return identical bits); a non-finite sample makes exactly its own column's output non-finite.  The float64 partials in the workspace are
     * [P * inner][runs][L] (xrfthip_workspace_bytes includes them): a caller with a wide grid and a small workspace runs it in boxes of columns (S > inner).
     * Still XRFTHIP_K_FASTW: a second layout of the same form.  Descriptors with the struct_size of the seven earlier versions are accepted (0, 0); an older library
     * answers XRFTHIP_BAD_ARG to the larger struct_size.  Offsets are computed in 64 bits. */
    int64_t seg_stride;
    int64_t seg_reserved2; /* 0 (anything else: XRFTHIP_BAD_ARG).  Appended together with seg_stride: no struct_size between the two */
    /* Spectrograms: the spectrum of EVERY segment, kept -- the other half of what seg_hop cuts out of a series (scipy.signal.spectrogram / stft; the reference's
     * power_spectrum(da, dim="time", chunks_to_segments=True, ...) without .mean("time_segment"), with an overlap).  One pass reads the segments where they lie and
     * writes each segment's spectrum once: neither the copy of the segments (twice the series at half overlap) nor a transposed copy of a cube exists.
     *   seg_keep = 1   Valid with seg_hop = H >= 1 (and what seg_hop asks for: ndim = 1, ny = 1, nx = L, dtype XRFTHIP_F32), mean_batch = M >= 1 the segments per
     *                  series (ONE segment is allowed), batch = P * M.  out_mode POWER | COMPLEX.  d_out is [P][M][nx_out], element (p, s, c) what the plain 1-D plan
     *                  writes at place c for segment s of series p: |X_k|^2 scale, real float32 (POWER), or X_k scale, complex64 (COMPLEX); with seg_stride = S
     *                  (the column layout, `inner` adjacent series) d_out is [P][M][nx_out][inner], the columns innermost -- the place the time axis had.
     *                  0 = off: everything about the descriptor is as without the field (mean_batch = 1 and OUT_COMPLEX with seg_hop stay XRFTHIP_BAD_ARG).
     * Input addressing, alignment (4 bytes) and the pitch rules are seg_hop's / seg_stride's; no byte outside the addressed samples is read.  Accepted: detrend NONE |
     * CONSTANT | LINEAR per segment, a window on axis 1, `scale`, XRFTHIP_SHIFT_X, XRFTHIP_HALF_X (k = 0 .. L / 2; not with SHIFT_X) with or without XRFTHIP_REALDIM_X2
     * (POWER), XRFTHIP_ISHIFT_X with POWER (no effect: no bit changes).
     * XRFTHIP_BAD_ARG: seg_keep not 0 | 1, seg_keep without seg_hop, seg_reserved3 != 0, out_mode CROSS | PHASE | COHERENCE, XRFTHIP_REALDIM_X2 with COMPLEX, and
     * everything seg_hop / seg_stride refuse.  XRFTHIP_UNSUPPORTED_LENGTH ("the caller composes": the segments copied out, the plain 1-D plan): L not a power of two
     * in 64 .. 4096 (columns: 64 .. 512), input that is not float32, the FLIP flags, XRFTHIP_ISHIFT_X or a phase table (xrfthip_plan_set_phase) together with
     * COMPLEX, a launch beyond 2^31 - 1 workgroups, XRFTHIP_FASTW=0 or XRFTHIP_FASTW_KEEP=0 in the environment when the plan is created; and, by default, the one class
     * that measured slower than its composition (profiles/r21_spectrogram.txt): L = 4096 with H = L, unless XRFTHIP_MEAN_ALL=1 is in the environment (docs/TUNING.md).
     * Every segment is a transform of its own (packed with itself, x_2j + i x_2j+1, L / 2 points): a non-finite sample makes exactly the segments that hold it
     * non-finite, and every other (series, segment) keeps its bits.  No sums across segments, no atomics, no workspace (xrfthip_workspace_bytes is 0); repeated calls
     * return identical bits.  Still XRFTHIP_K_FASTW: a third form of the same family (xrfthip_plan_describe prints a [fastw segments kept] line).  Descriptors with the
     * struct_size of the eight earlier versions are accepted (0, 0); an older library answers XRFTHIP_BAD_ARG to the larger struct_size. */
    int64_t seg_keep;
    int64_t seg_reserved3; /* 0 (anything else: XRFTHIP_BAD_ARG).  Appended together with seg_keep: no struct_size between the two */
    /* Synthesis: the inverse of what seg_keep with COMPLEX and XRFTHIP_HALF_X writes -- a series rebuilt from the half spectra of its M overlapping segments in ONE pass
     * (scipy.signal.istft): every segment inverse-transformed, multiplied by the window, overlap-added at s * H and divided by the sum of the squared windows.  The
     * inverse-transformed segments (twice the series at half overlap) never reach memory.
     *   seg_synth = 1   Valid with seg_hop = H, 1 <= H <= L; ndim = 1, ny = 1, nx = L; dtype XRFTHIP_C64, out_mode XRFTHIP_OUT_COMPLEX, detrend NONE; flags exactly
     *                   XRFTHIP_INVERSE | XRFTHIP_C2R_X; mean_batch = M >= 1 the segments per series, batch = P * M; seg_keep = 0, seg_stride = 0, inner <= 1.
     *                   d_in0 is [P][M][L / 2 + 1] complex64, bin k of segment s of series p at d_in0[p * in_stride_batch + s * (L / 2 + 1) + k]: in_stride_batch is
     *                   HERE the pitch between series in complex elements, 0 = dense, M * (L / 2 + 1).  d_out is [P][span] float32, dense, span = (M - 1) * H + L:
     *                     out[p][n] = num / den  where den > 1e-10, else num (scipy's rule: the first sample under a periodic Hann window),
     *                     num = sum_s w[n - s H] x_s[n - s H] scale,  den = sum_s w^2[n - s H],  over the segments s that cover n, in ascending s, float32,
     *                   x_s the unnormalised inverse real transform of segment s (the caller folds 1 / L into `scale`, as for every XRFTHIP_INVERSE plan) and w the
     *                   window on axis 1 (xrfthip_plan_set_window, L values; none: ones).  The imaginary parts of bins 0 and L / 2 are ignored, as the other C2R_X
     *                   plans and numpy.fft.irfft ignore them.
     *                   0 = off: everything about the descriptor is as without the field (seg_hop with XRFTHIP_INVERSE stays XRFTHIP_BAD_ARG).
     * Alignment: d_in0 8-byte aligned, d_out 4-byte aligned.  No byte outside the addressed input is read; every output sample is written exactly once, by one thread:
     * no atomics, no partial sums, no workspace (xrfthip_workspace_bytes is 0), and a sample's bits depend on its own covering segments only -- not on P, on M or on
     * the workgroups.  A non-finite bin makes exactly the samples of its own segment non-finite.
     * XRFTHIP_BAD_ARG: seg_synth not 0 | 1, seg_synth without seg_hop or with seg_keep, seg_reserved4 != 0, any other out_mode, dtype, detrend or flag (XRFTHIP_ISO
     * included), a phase table (xrfthip_plan_set_phase), a pitch below M * (L / 2 + 1), and everything seg_hop refuses.  XRFTHIP_UNSUPPORTED_LENGTH ("the caller
     * composes or arranges"): L not a power of two in 64 .. 4096; seg_stride > 0 (a column layout of the synthesis does not exist); 2 (R - 1) > NS with
     * R = ceil(L / H) the segments that meet in a sample and NS = 8192 / L the segments of a workgroup's tile (a workgroup transforms again the last R - 1 segments
     * of its predecessor: at most half its work); span >= 2^31; a launch beyond 2^31 - 1 workgroups; XRFTHIP_FASTW=0 or XRFTHIP_FASTW_SYNTH=0 in the environment
     * when the plan is created (docs/TUNING.md).
     * Still XRFTHIP_K_FASTW: a fourth form of the same family (xrfthip_plan_describe prints a [fastw overlap-add] line).  Descriptors with the struct_size of the nine
     * earlier versions are accepted (0, 0); an older library answers XRFTHIP_BAD_ARG to the larger struct_size.  Offsets are computed in 64 bits. */
    int64_t seg_synth;
    int64_t seg_reserved4; /* 0 (anything else: XRFTHIP_BAD_ARG).  Appended together with seg_synth: no struct_size between the two */
    /* FIR filtering along a series by overlap-save in ONE pass (scipy.signal.convolve(x, h, mode) for K real taps h): every L-sample segment transformed, multiplied
     * by the response, transformed back, and the V = L - K + 1 samples that do not wrap around kept.  No window, no overlap-add, no division, no gather; nothing but
     * the series (4 bytes per sample read) and the filtered series (4 bytes per sample written) goes through memory.
     *   seg_filter = 1   Valid with seg_hop = V, L / 2 <= V <= L (K = L - V + 1 taps); ndim = 1, ny = 1, nx = L; dtype XRFTHIP_F32, out_mode XRFTHIP_OUT_COMPLEX,
     *                    flags = 0, detrend NONE, no window; seg_keep = seg_synth = seg_stride = 0, inner <= 1 (the column layout, seg_filter_cols below, apart).
     *   seg_in_len = N >= 1       samples per series.  d_in0 is [P] series of N float32, series p at d_in0 + p * in_stride_batch: in_stride_batch is HERE the series
     *                             pitch in samples, 0 = dense = N, any other value >= N.
     *   seg_out_len = n_out >= 1  samples per filtered series.  d_out is [P][n_out] float32, dense, NOT complex whatever out_mode says:
     *                               out[p][n'] = scale * sum_k h[k] x_p[n' + a - k],  x_p = 0 outside [0, N)
     *   seg_lead = a              0 <= a <= K - 1 and a + n_out <= N + K - 1: the first output sample within the full convolution (scipy's "full": a = 0,
     *                             n_out = N + K - 1; "same": a = (K - 1) / 2, n_out = N; "valid": a = K - 1, n_out = N - K + 1).
     *                    mean_batch = M = ceil(n_out / V) the segments per series, batch = P * M.  Segment s holds the samples s V + a - (K - 1) + j, j < L (zeros
     *                    outside [0, N)) and yields the outputs s V .. s V + V - 1.
     *                    0 = off: the three companion words must be 0 and everything about the descriptor is as without the fields.
     * The response: xrfthip_plan_set_phase(plan, 1, H, L / 2 + 1) with H = the L-point transform of the zero-extended taps, bins 0 .. L / 2 (numpy.fft.rfft(h, L)),
     * interleaved doubles; kept as complex64.  Any other n, or axis 0: XRFTHIP_BAD_ARG.  NULL clears; without a table the response counts as 1 (out[n'] =
     * scale x[n' + a]: a pure delay).  The imaginary parts of entries 0 and L / 2 are ignored.  The transforms are unnormalised: the caller folds 1 / L into `scale`.
     * Alignment: d_in0 and d_out 4-byte aligned.  No byte outside [0, N) of a series is read; every output sample is written exactly once, by one thread: no atomics,
     * no workspace (xrfthip_workspace_bytes is 0), and a sample's bits depend on its own segment's L inputs, on H and on `scale` only -- not on P, on M or on the
     * workgroups.  Every segment is a transform of its own: a non-finite sample makes exactly the outputs of the (at most two) segments that hold it non-finite.
     * XRFTHIP_BAD_ARG: seg_filter not 0 | 1, a companion word non-zero with seg_filter = 0, and every violation of the rules above.  XRFTHIP_UNSUPPORTED_LENGTH ("the
     * caller composes"): L not a power of two in 64 .. 4096; a launch beyond 2^31 - 1 workgroups; XRFTHIP_FASTW=0 or XRFTHIP_FASTW_FILTER=0 in the environment when
     * the plan is created (docs/TUNING.md).
     * Still XRFTHIP_K_FASTW: a fifth form of the same family (xrfthip_plan_describe prints a [fastw overlap-save] line).  Descriptors with the struct_size of the ten
     * earlier versions are accepted (0, 0, 0, 0); an older library answers XRFTHIP_BAD_ARG to the larger struct_size.  Offsets are computed in 64 bits. */
    int64_t seg_filter;
    int64_t seg_lead;    /* the four words were appended together: no struct_size between them */
    int64_t seg_in_len;
    int64_t seg_out_len;
    /* Multitaper spectra in ONE pass (Thomson's estimate: the series of N samples multiplied by K orthogonal tapers, zero-extended to L points, transformed K times, the
     * K spectra added): out[p][k] = scale * sum_j |sum_{n<N} t_j[n] y_p[n] exp(-2 pi i k n / L)|^2 (XRFTHIP_OUT_CROSS: sum_j X0_j conj(X1_j), times the phase table),
     * y_p the series after the detrend over its N samples, t_j the rows of the table xrfthip_plan_set_tapers carries.  Neither the K tapered copies nor the K spectra
     * reach memory: 4 bytes per sample read, one spectrum per series written.
     *   seg_tapers = K >= 1      Valid with ndim = 1, ny = 1, nx = L; dtype XRFTHIP_F32; out_mode XRFTHIP_OUT_POWER | XRFTHIP_OUT_CROSS; mean_batch <= 1, batch = P the
     *                            series; seg_hop = 0 and every other seg_* word 0; inner <= 1; detrend NONE | CONSTANT | LINEAR; the flags a Welch plan takes
     *                            (XRFTHIP_SHIFT_X, XRFTHIP_HALF_X, XRFTHIP_REALDIM_X2; XRFTHIP_ISHIFT_X is ignored); no window (xrfthip_plan_set_window:
     *                            XRFTHIP_BAD_ARG -- the tapers are the windows).
     *   seg_taper_len = N        1 <= N <= L samples per series.  d_in0 (d_in1) is [P] series of N float32, series p at d_in0 + p * in_stride_batch: in_stride_batch is
     *                            HERE the series pitch in samples, 0 = dense = N, any other value >= N.  d_out is [P][nx_out], real or complex64 (CROSS), dense.
     *                            0 = off: seg_taper_len must be 0 too and everything about the descriptor is as without the fields.
     * Alignment: d_in0, d_in1 and d_out 4-byte (CROSS d_out: 8-byte) aligned.  No byte outside the N samples of a series is read.  One workgroup owns whole outputs: no
     * workspace (xrfthip_workspace_bytes is 0), no second kernel, no atomics; an output's bits depend on its own series, the table, L and `scale` only -- not on P or
     * on the workgroups -- and a non-finite sample makes exactly its own series' output non-finite.
     * XRFTHIP_BAD_ARG: K < 1; N < 1 or N > L; seg_taper_len set while seg_tapers = 0; every violation of the rules above.  XRFTHIP_UNSUPPORTED_LENGTH ("the caller
     * composes"): L not a power of two in 64 .. 4096; K > 32; XRFTHIP_FLIP_X / XRFTHIP_FLIP0_X; more than 2^31 - 1 workgroups; XRFTHIP_FASTW=0 or
     * XRFTHIP_FASTW_TAPERS=0 in the environment when the plan is created (docs/TUNING.md).
     * Still XRFTHIP_K_FASTW: a form of the same family (xrfthip_plan_describe prints a [fastw tapers] line).  Descriptors with the struct_size of the eleven earlier
     * versions are accepted (0, 0); an older library answers XRFTHIP_BAD_ARG to the larger struct_size.  Offsets are computed in 64 bits. */
    int64_t seg_tapers;
    int64_t seg_taper_len; /* appended together with seg_tapers: no struct_size between the two */
    /* The COLUMN layout of the FIR filter (seg_filter = 1): the series lie along a leading axis of a (time, ..) array and are filtered where they lie; the result is
     * written in the array's own order.  No transposed copy comes in or goes out: 4 bytes per sample read and 4 written, as in the rows layout.
     *   seg_filter_cols = 1   Valid with seg_filter = 1 and everything it asks for, but: seg_stride = S >= inner >= 1 (S >= 1: S = 1 with inner = 1 is one column of
     *                         its own and is NOT turned into the rows layout).  d_in0 is [blocks][N][inner] float32 columns: sample t of column c of block b at
     *                         d_in0 + b * in_stride_batch + t * S + c.  in_stride_batch is HERE the block pitch in elements, 0 = dense = N * S, any other value
     *                         >= (N - 1) * S + inner.  d_out is [blocks][n_out][inner] float32, dense -- the final order.  batch = blocks * M, M = mean_batch =
     *                         ceil(n_out / V); seg_lead, seg_in_len = N and seg_out_len = n_out as in the rows layout.  S, inner, N and n_out at most 2^31 - 1.
     *                         0 = off: everything about the descriptor is as without the field.
     * A workgroup takes C = min(32, 8192 / L) adjacent columns of one block and 8192 / (L C) consecutive segments of each; the loads and the stores run column
     * fastest (consecutive lanes, consecutive addresses of one time row).  Nothing outside the columns [0, inner) and the time rows [0, N) of a block is read.  A
     * sample's bits depend on its own segment's L inputs, on H and on `scale` only: they are those of the rows layout on the transposed copy, whatever inner, S,
     * the block and the neighbouring columns are.  A non-finite sample stays in its own column and in the segments that hold it.
     * XRFTHIP_BAD_ARG: seg_filter_cols not 0 | 1; seg_reserved5 non-zero; seg_filter_cols without seg_filter; seg_stride = 0 or < inner; S, inner, N or n_out beyond
     * 2^31 - 1; a pitch below (N - 1) * S + inner.  XRFTHIP_UNSUPPORTED_LENGTH ("the caller arranges": one transposed copy, the rows layout): L > 512; a launch
     * beyond 2^31 - 1 workgroups; a narrow grid, at most half of the groups' columns live (2 inner <= ceil(inner / C) C; it measured slower than the arranged route,
     * profiles/r30_fir_filter_cols.txt; taken with XRFTHIP_MEAN_ALL=1); XRFTHIP_FASTW=0, XRFTHIP_FASTW_FILTER=0, XRFTHIP_FASTW_COLS=0 or XRFTHIP_FASTW_FILTER_COLS=0 in the environment when the plan is
     * created (docs/TUNING.md).
     * Still XRFTHIP_K_FASTW and the [fastw overlap-save] line, with a [fastw columns] line behind it.  Descriptors with the struct_size of the twelve earlier
     * versions are accepted (0, 0); an older library answers XRFTHIP_BAD_ARG to the larger struct_size.  Offsets are computed in 64 bits. */
    int64_t seg_filter_cols;
    int64_t seg_reserved5; /* 0 (anything else: XRFTHIP_BAD_ARG).  Appended together with seg_filter_cols: no struct_size between the two */
} xrfthip_desc;

typedef struct xrfthip_plan xrfthip_plan;

int xrfthip_version(void);
const char* xrfthip_strerror(int status);
int xrfthip_last_hip_error(void); /* hipError_t of the most recent XRFTHIP_HIP_ERROR on this thread */

int xrfthip_plan_create(xrfthip_plan** plan, const xrfthip_desc* desc);
int xrfthip_plan_destroy(xrfthip_plan* plan);

/* axis: 0 = y, 1 = x.  h_window: n doubles (scipy.signal.windows.<name>(n, sym=False)).  NULL clears. */
int xrfthip_plan_set_window(xrfthip_plan* plan, int axis, const double* h_window, int64_t n);
/* h_phase: n interleaved (re,im) doubles indexed by UNSHIFTED frequency index: exp(-i 2 pi f_k lag)
 * (for CROSS: the net factor phase0 * conj(phase1)).  With XRFTHIP_PHASE_IN (inverse transforms) the table multiplies
 * the INPUT and is indexed by source position; a C2R_X plan then takes nx/2 + 1 entries on axis 1.  NULL clears.
 * An XRFTHIP_HERM_FIELD plan: axis 0, 1, 2 = t, herm_ny, herm_nx (see xrfthip_desc.herm_ny); axis 2 is XRFTHIP_BAD_ARG on every other plan. */
int xrfthip_plan_set_phase(xrfthip_plan* plan, int axis, const double* h_phase, int64_t n);
/* The taper table of a multitaper plan (xrfthip_desc.seg_tapers = K, seg_taper_len = N): h_tapers is [K][N] float32, row j the taper d_j already multiplied by
 * sqrt(w_j) (w_j its weight in the sum: the kernel knows no weights), copied to the device beside the plan's other tables.  NULL clears.  Any other plan:
 * XRFTHIP_BAD_ARG.  xrfthip_exec of a multitaper plan without a table: XRFTHIP_BAD_ARG. */
int xrfthip_plan_set_tapers(xrfthip_plan* plan, const float* h_tapers);
/* h_binmap: [ny][nx_out] int32 bin codes indexed by UNSHIFTED frequency indices (nx_out = nx, or nx/2+1 with
 * HALF_X); negative = not binned.  The host computes it with the reference's float64 pd.cut expression.
 * An ISO plan of the inner / mid layouts: [ny][nx] in the plan's own axis order (the first axis in memory = y), and the map must be RADIAL -- every sample binned; along a
 * row the bin depends on |kx| only and never decreases with it (each bin of a row is one contiguous range of |kx|); the Hermitian twin (-ky, -kx) of a sample lies in
 * the sample's bin.  pd.cut of sqrt(ky^2 + kx^2) always is, for any spacings.  Any other map: XRFTHIP_BAD_ARG (there is no second path to the sums where the axes lie).
 * The plan's workspace grows by its partial sums, (ny/2 + 1) * ne * nbins * 8 bytes (x2 CROSS) per slab of a group: ask xrfthip_workspace_bytes after this call. */
int xrfthip_plan_set_binmap(xrfthip_plan* plan, const int32_t* h_binmap, int64_t ny, int64_t nx_out, int32_t nbins);

/* Per-pass timing with HIP events recorded on the exec stream around every kernel launch (bench.py's roofline
 * figure).  enable != 0 starts a fresh record; xrfthip_plan_profile_read synchronises the recorded events and
 * writes one line per pass: "<label> <launches> <total_ms>\n".  Off by default (no events are recorded). */
int xrfthip_plan_set_profiling(xrfthip_plan* plan, int enable);
int xrfthip_plan_profile_read(xrfthip_plan* plan, char* buf, size_t buflen);

/* 1 if a pass of the plan runs Bluestein's algorithm (a transform length with a prime factor that has no butterfly: numpy.fft takes
 * any length, xrft.py:439-444), else 0.  In float32 the chirp convolution leaves an error of a few 1e-7 of the spectrum's PEAK in every bin;
 * callers that hold small bins to 1e-3 run such plans in float64 (xrft_amd/engine.py does, with xrfthip_convert at both ends). */
int xrfthip_plan_uses_bluestein(const xrfthip_plan* plan);

/* Which kernel family serves the plan (decided when it is created; what xrfthip_plan_describe prints, as numbers -- callers that compose plans decide on
 * these, not on the text): *kind = xrfthip_kernel_kind, *per_workgroup = the independent sequences (columns, rows or slabs) one workgroup transforms
 * (0 where that is not a property of the plan).  ABI 0.1.3. */
typedef enum xrfthip_kernel_kind {
    XRFTHIP_K_GENERIC = 0,    /* tile_fft.h passes */
    XRFTHIP_K_FASTY = 1,      /* two-pass float32 powers of two (and the four-step 1-D form) */
    XRFTHIP_K_FASTM = 2,      /* two-pass table lengths */
    XRFTHIP_K_FASTN = 3,      /* two-pass, lengths as data (either pass may be a table kernel) */
    XRFTHIP_K_FASTM_Y = 4,    /* one axis, not the contiguous one, table lengths */
    XRFTHIP_K_FASTM_X = 5,    /* rows, table lengths */
    XRFTHIP_K_FASTG_Y = 6,    /* one axis, not the contiguous one, lengths as data */
    XRFTHIP_K_FASTG_ROWS = 7, /* groups of rows, lengths as data */
    XRFTHIP_K_FASTG = 8,      /* one pass over a small slab, lengths as data */
    XRFTHIP_K_FASTS = 9,      /* one pass over a small float32 slab in registers */
    XRFTHIP_K_FASTR = 10,     /* one pass over a long float32 row in registers */
    XRFTHIP_K_COMPOSITE = 11, /* xrfthip_desc.inner / .mid: two one-axis plans */
    XRFTHIP_K_FASTH = 12,     /* xrfthip_desc.herm_ny / herm_nx: the last pass of a three-axis spectrum, half spectrum in, full result out */
    XRFTHIP_K_FASTW = 13      /* xrfthip_desc.seg_hop: Welch spectra, overlapping segments of a series read in place and averaged in one pass */
} xrfthip_kernel_kind;
int xrfthip_plan_kernel_info(const xrfthip_plan* plan, int32_t* kind, int32_t* per_workgroup);

size_t xrfthip_workspace_bytes(const xrfthip_plan* plan);
/* human-readable pass list (kernel, tile, grid, LDS) for logs and DESIGN.md; returns bytes written */
int xrfthip_plan_describe(const xrfthip_plan* plan, char* buf, size_t buflen);

/*
 * d_in0 : [batch][ny][nx] input (dtype); with xrfthip_desc.in_stride_y / in_stride_batch: element (b, y, x) at d_in0[b * in_stride_batch + y * in_stride_y + x],
 *         and the pointer 16-byte aligned (XRFTHIP_BAD_ARG otherwise)
 * d_in1 : second field for CROSS, else NULL; the same strides and alignment as d_in0
 * d_out : COMPLEX/CROSS: complex [batch][ny][nx_out]; POWER: real [batch][ny][nx_out]; may be NULL with
 *         XRFTHIP_NO_SPECTRUM_OUT
 * d_iso : with XRFTHIP_ISO: float64 [batch][nbins] (POWER) or complex128 [batch][nbins] (CROSS), else NULL; inner / mid layouts: [batch][ne][nbins], ne = inner | mid
 * d_workspace / ws_bytes : >= xrfthip_workspace_bytes(plan), 256-byte aligned
 */
int xrfthip_exec(const xrfthip_plan* plan, const void* d_in0, const void* d_in1, void* d_out, void* d_iso,
                 void* d_workspace, size_t ws_bytes, void* stream);

/* A kept pass 1 (no new version number: the presence of the three symbols below tells the capability).  The auto and cross spectra of one pair of fields
 * (coherence, transfer functions: xrft.cross_spectrum, then xrft.isotropic_power_spectrum of each field) are computed back to back, each by a plan of its own, and
 * in the two-pass float32 family (XRFTHIP_K_FASTY) every one of those plans starts with the same column pass over the same field.  What that pass leaves for ONE
 * field -- the tiled half spectrum, the per-column sums and lines, the detrend corrections -- is one self-contained "pass-1 block", and a plan can be told to
 * write it into memory of the caller's, or to read it from there and launch neither the column kernel nor the fit kernel for that field.
 *
 * xrfthip_plan_pass1_bytes: the size of one field's block, a multiple of 256 -- or 0 where no block can be handed over: every kernel family other than FASTY's
 *   two-pass slabs (the four-step 1-D form included), a plan whose batch runs in more than one group of slabs (xrfthip_desc.slabs_per_group < batch), tuning builds
 *   whose column pass keeps rendezvous counters.  Ask after the plan's tables are set (a bin map can move a plan to another family).
 * xrfthip_plan_pass1_signature: *sig = a 64-bit hash of everything but the input's values that decides the bytes of the block of `field` (0, or 1 = d_in1 of a
 *   CROSS / PHASE plan): the column kernel's instantiation, ny, nx, batch, the rows of the intermediate and the kernel's geometry, the detrend kind, the values of
 *   the two windows, the field's flip flags, the input strides, the tuning word and XRFTHIP_VERSION.  Two plans with equal signatures write bit-identical blocks
 *   from the same input, whatever else differs between them (out_mode, shifts, scale, phases, ISO).  XRFTHIP_BAD_ARG where xrfthip_plan_pass1_bytes is 0.
 *   Whether the input IS the same -- pointer, strides, contents unchanged since the block was written, the stream that orders writer and reader -- is the caller's
 *   to know; xrft_amd/engine.py keeps a tag per block.
 * xrfthip_exec_ex: xrfthip_exec with its arguments in a struct (struct_size = sizeof(xrfthip_exec_args)) and, per field, where pass 1 lives:
 *   XRFTHIP_PASS1_PRIVATE  inside the workspace (xrfthip_exec is this for every field: same launches, same bytes)
 *   XRFTHIP_PASS1_PRODUCE  run pass 1 as usual, but into pass1_block (xrfthip_plan_pass1_bytes bytes, 256-byte aligned)
 *   XRFTHIP_PASS1_CONSUME  pass1_block holds the block a plan with the SAME signature produced from the same input, and every kernel that wrote it precedes this call
 *                          in stream order: no column pass, no fit kernel for the field (the profiling records then show no "fasty_cols" launch for it)
 *   With EVERY field of the plan in a mode other than PRIVATE the workspace needs only xrfthip_workspace_bytes(plan) - fields * xrfthip_plan_pass1_bytes(plan)
 *   bytes (fields = 2 for CROSS / PHASE, else 1).  XRFTHIP_BAD_ARG: a mode above 2; a mode other than PRIVATE on a plan whose xrfthip_plan_pass1_bytes is 0 or on
 *   field 1 of a one-field plan; a null block or one not 256-byte aligned; a block that overlaps [d_workspace, d_workspace + ws_bytes) or the other block.
 *   Like xrfthip_exec it neither allocates, nor synchronises, nor reads the environment, and it only reads a consumed block. */
#define XRFTHIP_PASS1_PRIVATE 0u
#define XRFTHIP_PASS1_PRODUCE 1u
#define XRFTHIP_PASS1_CONSUME 2u
typedef struct xrfthip_exec_args {
    uint32_t struct_size; /* = sizeof(xrfthip_exec_args) */
    uint32_t reserved;
    const void* d_in0; /* the arguments of xrfthip_exec */
    const void* d_in1;
    void* d_out;
    void* d_iso;
    void* d_workspace;
    size_t ws_bytes;
    void* stream;
    struct {
        void* pass1_block;   /* device memory, NULL with XRFTHIP_PASS1_PRIVATE */
        uint32_t pass1_mode; /* XRFTHIP_PASS1_* */
        uint32_t reserved;
    } field[2]; /* [0]: d_in0, [1]: d_in1 */
} xrfthip_exec_args;
size_t xrfthip_plan_pass1_bytes(const xrfthip_plan* plan);
int xrfthip_plan_pass1_signature(const xrfthip_plan* plan, int field, uint64_t* sig);
int xrfthip_exec_ex(const xrfthip_plan* plan, const xrfthip_exec_args* args);

/* Stand-alone detrend (xrft.detrend, detrend.py:11-97) over the last `ndim` axes: out = in - trend, same dtype.
 * d_workspace: >= xrfthip_detrend_workspace_bytes(batch) bytes. */
size_t xrfthip_detrend_workspace_bytes(int64_t batch);
int xrfthip_detrend(int32_t dtype, int32_t ndim, int64_t batch, int64_t ny, int64_t nx, int32_t detrend_type,
                    const void* d_in, void* d_out, void* d_workspace, size_t ws_bytes, void* stream);

/* The same with the independent elements innermost: [batch][ny][nx][inner], mean or least-squares plane over (ny, nx) for every
 * (batch, inner) element (ndim = 2), or line over nx of [batch][nx][inner] (ndim = 1, ny = 1) -- xrft.detrend over adjacent axes that
 * are not the trailing ones, without a transposed copy.  d_workspace: >= xrfthip_detrend_inner_workspace_bytes(dtype, batch, inner). */
size_t xrfthip_detrend_inner_workspace_bytes(int32_t dtype, int64_t batch, int64_t inner);
int xrfthip_detrend_inner(int32_t dtype, int32_t ndim, int64_t batch, int64_t ny, int64_t nx, int64_t inner, int32_t detrend_type,
                          const void* d_in, void* d_out, void* d_workspace, size_t ws_bytes, void* stream);

/* The same over the last THREE axes (n0, n1, n2) of [batch][n0][n1][n2]: mean, or the least-squares hyperplane
 * a0 + a1 i + a2 j + a3 k of xrft/detrend.py:116-138 (_detrend_3d_ufunc).  Same workspace size as xrfthip_detrend. */
int xrfthip_detrend3(int32_t dtype, int64_t batch, int64_t n0, int64_t n1, int64_t n2, int32_t detrend_type,
                     const void* d_in, void* d_out, void* d_workspace, size_t ws_bytes, void* stream);

/* Tail of power_spectrum / cross_spectrum (xrft.py:740, 825) on already transformed fields, for transforms over more
 * than two axes that are composed of several plans: d_out[e] = |d_a[e]|^2 * scale (real, d_b NULL) or
 * d_a[e] * conj(d_b[e]) * scale (complex).  dtype = XRFTHIP_C64 | XRFTHIP_C128 (type of d_a / d_b). */
int xrfthip_spectrum_tail(int32_t dtype, int64_t n, const void* d_a, const void* d_b, void* d_out, double scale, void* stream);

/* d_out[e] = arg(d_a[e]) in [-pi, pi], real of the same precision (dtype = XRFTHIP_C64 | XRFTHIP_C128): numpy.angle of a stored cross
 * spectrum, for xrft.cross_phase (xrft.py:838-874) on calls whose cross spectrum is composed of several plans. */
int xrfthip_angle(int32_t dtype, int64_t n, const void* d_a, void* d_out, void* stream);

/* d_out[e] = |d_cross[e]|^2 / (d_p0[e] * d_p1[e]): the magnitude-squared coherence from an averaged cross spectrum and the two averaged power spectra -- the tail
 * of the composed route where no XRFTHIP_OUT_COHERENCE plan takes the call.  dtype = XRFTHIP_C64 | XRFTHIP_C128 of d_cross; d_p0, d_p1 and d_out are real of the
 * matching precision.  Evaluated in float64 and rounded once; no clamp; a zero denominator gives what IEEE division gives (NaN for 0 / 0, else inf). */
int xrfthip_coherence(int32_t dtype, int64_t n, const void* d_cross, const void* d_p0, const void* d_p1, void* d_out, void* stream);

/* The same as xrfthip_spectrum_tail over [outer][na][inner] with the real-dim factor [1, 2, ..., 2, (1 if last_is_one)] along axis `na` (xrft.py:673-682):
 * the kept half of a real transform counts twice, except k = 0 and, for an even length, the Nyquist sample. */
int xrfthip_spectrum_tail_axis(int32_t dtype, int64_t outer, int64_t na, int64_t inner, int32_t last_is_one, const void* d_a, const void* d_b,
                               void* d_out, double scale, void* stream);

/* out[o][i][j] = in[o][src(i)][j] over [outer][n_out][inner] (source [outer][n_in][inner]), elem_bytes = 4 | 8 | 16:
 * src(i) = d_index[i] (device int64[n_out]) or, with d_index NULL, (i - roll) mod n_in (numpy.roll: n_out == n_in).
 * The fftshift / ifftshift of the backend module (xrft.py:446-447, 617-621) and the gather of spectra that are not stored
 * in fftshift order (xrft.ifft).  d_out must not alias d_in. */
int xrfthip_gather_axis(int32_t elem_bytes, int64_t outer, int64_t n_out, int64_t inner, int64_t n_in, const int64_t* d_index, int64_t roll,
                        const void* d_in, void* d_out, void* stream);

/* d_out[b][j] = (j < n_in ? d_in[b][j] : 0) * d_table[j], j < n_out: zero padding or truncation with a pointwise complex factor.
 * dtype of d_in F32|F64|C64|C128; d_table (min(n_in, n_out) entries) and d_out complex of that precision.  The pointwise steps of Bluestein's algorithm
 * through global memory, for lengths with a prime factor > XRFTHIP_MAX_RADIX that exceed the in-tile bound
 * (numpy.fft takes any length: xrft.py:398-447). */
int xrfthip_table_mul(int32_t dtype, int64_t batch, int64_t n_in, int64_t n_out, const void* d_in, const void* d_table, void* d_out, void* stream);

/* d_out[e] = (precision of dtype_out) d_in[e], e < n: F32 <-> F64 or C64 <-> C128 (n counts real or complex elements of dtype_in's kind).
 * The precision change around float32 plans that run in float64 (Bluestein lengths, see xrfthip_plan_uses_bluestein).
 * F16 -> F32 and BF16 -> F32: the exact widening of half-precision samples, one pass (subnormals, +-0, +-inf exact; NaN -> NaN), for the calls a half plan declines
 * with XRFTHIP_UNSUPPORTED_LENGTH.  d_in 2-byte aligned (4-byte: pairs of samples per load), d_out 4-byte aligned; no other direction. */
int xrfthip_convert(int32_t dtype_in, int32_t dtype_out, int64_t n, const void* d_in, void* d_out, void* stream);

/* d_out[o][i] = scale * sum_k d_in[o][k][i] over [outer][n][inner] -> [outer][inner], same dtype (F32|F64|C64|C128), accumulated in float64
 * in the order k = 0, 1, ...: the sum / mean over a batch dimension (scale = 1 / n), bit-reproducible.  What the reference's users do with
 * batches of isotropic spectra (`iso_ps.mean("time")`, xrft/tests/test_xrft.py:1011-1013) and, with scale = 1 / (slabs of ALL ranks), the
 * local term of the multi-GPU batch mean (xrft_amd/dist.py: one all_reduce(SUM) of nbins values finishes it). */
int xrfthip_reduce_axis(int32_t dtype, int64_t outer, int64_t n, int64_t inner, const void* d_in, void* d_out, double scale, void* stream);

/* The memory floor of the headline path (BASELINE.json configs[2]: xrft.power_spectrum of 4096 x 4096 float32 slabs, xrft/xrft.py:685-750),
 * measured on the spot: the access patterns of the two passes with the transforms removed (csrc/selftest.h), and a plain copy.
 * `reps` timed rounds after one warm-up; us[0..2] = microseconds per slab of the copy (nslab x 64 MB read + written), the column-pass
 * skeleton and the row-pass skeleton.  d_in: [nslab][4096][4096] float32; d_w2: scratch, nslab * 2052 * 4096 * 8 bytes; d_out:
 * [nslab][4096][4096] float32, overwritten.  Synchronises the stream: a measurement for bench.py, not part of the hot path. */
int xrfthip_selftest_floor(const void* d_in, void* d_w2, void* d_out, int64_t nslab, int32_t reps, double* us, void* stream);

/* Stand-alone radial bin-sum of an existing spectrum (xrft.isotropize, xrft.py:948-1010):
 * d_in [batch][ny][nx] (dtype F32|F64|C64|C128), d_binmap device int32 [ny][nx] (bin of each sample, < 0 = none),
 * d_iso float64|complex128 [batch][nbins] (every entry written).  The sums are bit-reproducible (per-workgroup integer
 * fixed-point sums, combined in a fixed order); d_workspace holds the per-workgroup tables,
 * xrfthip_isotropize_workspace_bytes(...) bytes (0 = bad arguments).  Any nbins >= 1. */
size_t xrfthip_isotropize_workspace_bytes(int32_t dtype, int64_t batch, int64_t ny, int64_t nx, int32_t nbins);
int xrfthip_isotropize(int32_t dtype, int64_t batch, int64_t ny, int64_t nx, const void* d_in,
                       const int32_t* d_binmap, int32_t nbins, void* d_iso, void* d_workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XRFT_HIP_H */
