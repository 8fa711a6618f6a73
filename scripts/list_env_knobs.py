#!/usr/bin/env python3
"""Regenerates docs/TUNING.md: every environment variable the library reads (env_ll in xrft_amd/csrc), where, and its default.  All of them are read ONCE, when a
plan is created (xrfthip_exec never calls getenv); none is needed for normal use -- they exist to A/B kernel families and launch shapes on one box."""
import glob, os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES = {
    "XRFTHIP_NO_FAST": "1: every specialised kernel family off -- the generic tiled passes (`tile_fft.h`) take the plan (the tests' second implementation)",
    "XRFTHIP_FASTM": "0: the table kernels of `fastm.h` off (the run-time-radix kernels or the generic passes take over)",
    "XRFTHIP_FASTN": "0: the run-time-radix two-pass kernels of `fastn.h` off",
    "XRFTHIP_FASTG": "0: the one-pass LDS kernels of `fastg.h` off",
    "XRFTHIP_FASTR": "0: the register-resident row kernels of `fastr.h` off",
    "XRFTHIP_FASTW": "0: the Welch kernel of `fastw.h` off: a plan with `xrfthip_desc.seg_hop` answers XRFTHIP_UNSUPPORTED_LENGTH and the API composes (segments unfolded, the plain plan, the mean)",
    "XRFTHIP_FASTW_COLS": "0: the column layout of the Welch kernel off: a plan with `xrfthip_desc.seg_stride` answers XRFTHIP_UNSUPPORTED_LENGTH, and the API (which reads the variable itself, per call) arranges a leading time axis first -- one transposed copy, then the rows layout: the route before the column layout, kept for measurements (profiles/r20_welch_cols.txt)",
    "XRFTHIP_FASTW_KEEP": "0: the segments-kept form of the Welch family (`fastk.h`) off: a plan with `xrfthip_desc.seg_keep` answers XRFTHIP_UNSUPPORTED_LENGTH, and the API (which reads the variable itself, per call) composes `spectrogram` / `stft` -- segments unfolded and copied, the plain 1-D plan, the dims moved: the route before the form, kept for measurements (profiles/r21_spectrogram.txt)",
    "XRFTHIP_FASTW_SYNTH": "0: the synthesis form of the Welch family (`fasto.h`) off: a plan with `xrfthip_desc.seg_synth` answers XRFTHIP_UNSUPPORTED_LENGTH, and the API (which reads the variable itself, per call) composes `istft` -- `ifft` of every segment, the window, R strided adds, the division: the route without the form, kept for measurements (profiles/r26_istft.txt)",
    "XRFTHIP_FASTW_FILTER": "0: the filter form of the Welch family (`fastf.h`) off: a plan with `xrfthip_desc.seg_filter` answers XRFTHIP_UNSUPPORTED_LENGTH, and the API (which reads the variable itself, per call) composes `fir_filter` -- a zero-extended copy, the segments unfolded, the real 1-D plan, the table product, the C2R plan, the kept samples sliced out: the route without the form, kept for measurements (profiles/r27_fir_filter.txt)",
    "XRFTHIP_FASTW_FILTER_COLS": "0: the column layout of the filter form (`fastf.h`, `fastf_kernel<.., true>`) off: a plan with `xrfthip_desc.seg_filter_cols` answers XRFTHIP_UNSUPPORTED_LENGTH, and the API (which reads the variable itself, per call) arranges a leading dim of `fir_filter` first -- one transposed copy, the rows layout, the result moved back as a view: the route before the layout, kept for measurements (profiles/r30_fir_filter_cols.txt)",
    "XRFTHIP_FASTW_TAPERS":"0: the multitaper form of the Welch family (`fastt.h`) off: a plan with `xrfthip_desc.seg_tapers` answers XRFTHIP_UNSUPPORTED_LENGTH, and the API (which reads the variable itself, per call) composes `multitaper_*` -- the library's detrend, a taper dim by broadcasting the table, zero-extension, `power_spectrum` / `cross_spectrum`, the weighted sum: the route without the form, kept for measurements (profiles/r29_multitaper.txt)",
    "XRFTHIP_FASTC": "0: complex rows of 2048 ... 16384 points leave `fastc_kernel`",
    "XRFTHIP_CROWS": "0: complex rows of 256 ... 4096 points leave the row pass of `fasty_c2c.h`",
    "XRFTHIP_FASTYC": "0: complex power-of-two slabs leave the two-pass pipeline of `fasty_c2c.h`",
    "XRFTHIP_FASTR_GRID": "workgroups of a row-kernel launch: 0 = one per row; default: a resident set (256 at 65536 / 32768 samples, 512 at 16384 for complex results) on long batches",
    "XRFTHIP_FASTR_STAGGER": "`classes << 8 | steps`: workgroup class c = (block / 8) % classes starts c x steps x 3.4 us late (profiles/r06_c2_stagger.txt, r06_rows_stagger.txt)",
    "XRFTHIP_FASTS_GRID": "workgroups of a small-slab launch: 0 = one per slab; default: 256 walking the slabs for >= 1024 slabs of 256 x 256 (profiles/r06_fasts_prefetch.txt)",
    "XRFTHIP_FASTS_STAGGER": "as XRFTHIP_FASTR_STAGGER, for the resident set of slab workgroups (default three classes 6.8 us apart)",
    "XRFTHIP_GROUP": "slabs per pass-1 / pass-2 launch pair of the two-pass pipelines (default: the whole batch up to the workspace cap)",
    "XRFTHIP_DBG": "1: plan-selection trace on stderr",
    "XRFTHIP_MEAN_RUNS": "runs per output of a mean plan (`xrfthip_desc.mean_batch`): each run is a workgroup (per unit of rows) with a float64 partial of its own; 0 = the rule of `mean_layout` (fill the card, at most ny / 4; a Welch plan: at most M / 2)",
    "XRFTHIP_MEAN_ALL": "1: a plan with `xrfthip_desc.mean_batch` takes the mean form of every class the kernels of `fasty_mean.h` / `fasts_mean.h` serve (default 0: only the classes that measured faster than the composition, profiles/r15_batch_mean.txt); likewise a plan with `xrfthip_desc.seg_keep` takes L = 4096 without overlap (profiles/r21_spectrogram.txt) and one with `xrfthip_desc.seg_filter_cols` a narrow grid (profiles/r30_fir_filter_cols.txt)",
}


def main():
    rows = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "xrft_amd/csrc/*.cpp")) + glob.glob(os.path.join(ROOT, "xrft_amd/csrc/*.h")) + glob.glob(os.path.join(ROOT, "xrft_amd/csrc/*.inc"))):
        for i, line in enumerate(open(f), 1):
            for m in re.finditer(r'env_ll\("(XRFTHIP_[A-Z0-9_]+)",\s*(.*?)\)(?=[\s;,)&|!=<>?:])', line):
                c = line.split("//", 1)[1].strip() if "//" in line else ""
                rows.setdefault(m.group(1), []).append((os.path.basename(f), i, m.group(2).strip(), c))
    out = ["# Environment variables of libxrft_hip.so (generated by scripts/list_env_knobs.py)", "",
           "Every variable is read when a plan is created (`xrfthip_plan_create`; `xrfthip_exec` never calls `getenv`). None is needed in normal use: they switch a kernel",
           "family off (the next one in `xrfthip_plan_create`'s order takes the plan -- how the tests hold two implementations against each other) or change a launch shape",
           "for A/B measurements on one box (`scripts/prof.py call ... --env K=V`).", "",
           "| variable | default | read at | what |", "|---|---|---|---|"]
    for name in sorted(rows):
        where = ", ".join(f"`{f}:{ln}`" for f, ln, _, _c in rows[name][:3]) + (" ..." if len(rows[name]) > 3 else "")
        default = rows[name][0][2].replace("|", "\\|")
        note = NOTES.get(name) or next((c for _f, _l, _d, c in rows[name] if c), "")  # (no note: the comment of the line that reads it)
        if not note:
            note = ("debug output of that family's plan builder" if name.endswith("_DBG") else
                    "geometry override of the run-time-radix kernels (threads / sequences per workgroup / largest radix), 0 = the builder's rule: measurements only" if name.startswith(("XRFTHIP_FASTN_", "XRFTHIP_FI_", "XRFTHIP_FASTGY_", "XRFTHIP_FASTG_")) else
                    "option of the generic tiled passes (`tile_fft.h`: lean loaders / epilogues, tables in LDS, radix set, four-step thresholds), 1 = on" if name.startswith(("XRFTHIP_LEAN_", "XRFTHIP_TW_", "XRFTHIP_REV_", "XRFTHIP_TILED_", "XRFTHIP_RADIX", "XRFTHIP_PATHS", "XRFTHIP_X_", "XRFTHIP_Y_", "XRFTHIP_GENERIC_", "XRFTHIP_LDS_", "XRFTHIP_COMPOSITE")) else
                    "0: that kernel family / form off (the next one takes the plan)" if rows[name][0][2] == "1" else
                    "launch-shape / grouping override of the two-pass pipelines: measurements only")
        note = (note[:200] + " ...") if len(note) > 204 else note
        out.append(f"| `{name}` | `{default}` | {where} | {note.replace('|', chr(92) + '|')} |")
    path = os.path.join(ROOT, "docs/TUNING.md")
    open(path, "w").write("\n".join(out) + "\n")
    print(f"{len(rows)} variables -> {path}")


if __name__ == "__main__":
    sys.exit(main())
