"""Times power_spectrum / cross_spectrum / fft over THREE axes on the fused routes (csrc/fasth.h) against the compositions they replace, in one process on one GPU:
every case runs with api._FUSE_THREE_AXES on and off, alternating, after a warm-up of both; each call is timed with device events around the whole product call
(detrend, both stages, the tail) and the peak device memory over the resident input is taken from torch's allocator.  Writes one table (profiles/r09_three_axes.txt;
the fft rows: profiles/r14_three_axis_fft.txt).  A shape of four entries has a leading batch dim; the small fft cubes are timed as the mean of 20 calls per round.

    python scripts/bench_three_axes.py [--rounds 7] [--out FILE] [--small] [--only fft]
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xrft_amd as xa  # noqa: E402
from xrft_amd import api  # noqa: E402

CASES = [  # (operation, dtype, (nt, ny, nx))
    ("power_spectrum", "float32", (64, 1024, 1024)),
    ("power_spectrum", "float32", (256, 512, 512)),
    ("power_spectrum", "float64", (120, 360, 720)),
    ("cross_spectrum", "float32", (64, 1024, 1024)),
    ("fft", "float32", (2, 64, 128, 128)),
    ("fft", "float64", (2, 30, 90, 72)),
    ("fft", "float32", (64, 1024, 1024)),
    ("fft", "float64", (120, 360, 720)),
]
SMALL = [("power_spectrum", "float32", (16, 32, 32)), ("cross_spectrum", "float64", (12, 10, 18)), ("fft", "float32", (2, 8, 6, 10))]


def one_call(op, fields, fuse, calls=1):
    api._FUSE_THREE_AXES = fuse
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            res = getattr(xa, op)(*fields, dim=["t", "y", "x"], detrend="linear", window="hann")
        b.record()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        tag = "[fasth]" in next(reversed(api._plan_cache.values())).describe()
        return a.elapsed_time(b) / calls, peak, tag, res
    finally:
        api._FUSE_THREE_AXES = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--only", default=None, help="the rows of one operation, e.g. fft")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "this script measures on a GPU"
    lines = [f"# three-axis spectra and transforms, linear detrend + Hann, one process, {torch.cuda.get_device_name(0)}; ms per call: median [min .. max] of {args.rounds} alternating rounds after a warm-up of both routes",
             "# fused = detrend3 -> two-axis plan (half spectrum out) -> fasth last pass (fft: its field form); composed = api._FUSE_THREE_AXES = False (the composition before round 9, the same build)",
             f"{'case':58s} {'fused ms':>26s} {'composed ms':>26s} {'ratio':>6s} {'peak fused MB':>14s} {'peak composed MB':>17s} {'max |diff| / max':>17s}"]
    for op, dtype, shape in (SMALL if args.small else CASES):
        if args.only and op != args.only:
            continue
        nt, ny, nx = shape[-3:]
        dims = ("b", "t", "y", "x")[-len(shape):]
        calls = 20 if int(np.prod(shape)) <= (1 << 22) else 1  # (a small cube: one call is a few launches -- the mean of 20)
        tdt = torch.float32 if dtype == "float32" else torch.float64
        g = torch.Generator(device="cuda").manual_seed(1)
        coords = {"t": np.arange(nt) * 1.0, "y": np.arange(ny) * 0.5, "x": np.arange(nx) * 0.25}
        fields = [xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=tdt), dims, coords) for _ in range(2 if op == "cross_spectrum" else 1)]
        times = {True: [], False: []}
        peaks = {}
        _, _, tag, rf = one_call(op, fields, True)   # warm-up: plans, tables, scratch
        assert tag, "the fused route did not take the case"
        _, _, tag0, rc = one_call(op, fields, False)
        assert not tag0
        diff = float((rf.data - rc.data).abs().max() / rc.data.abs().max())
        del rf, rc
        for _ in range(args.rounds):
            for fuse in (True, False):
                ms, peak, _, res = one_call(op, fields, fuse, calls)
                del res
                times[fuse].append(ms)
                peaks[fuse] = max(peaks.get(fuse, 0), peak)
        med = {k: float(np.median(v)) for k, v in times.items()}
        fmt = lambda k: f"{med[k]:8.3f} [{min(times[k]):7.3f} .. {max(times[k]):7.3f}]"
        lines.append(f"{op + ' ' + dtype + ' ' + str(shape):58s} {fmt(True):>26s} {fmt(False):>26s} {med[False] / med[True]:6.2f} {peaks[True] / 2**20:14.1f} {peaks[False] / 2**20:17.1f} {diff:17.2e}")
        print(lines[-1], flush=True)
        del fields
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
