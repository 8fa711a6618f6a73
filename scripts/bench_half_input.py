#!/usr/bin/env python
"""Time float32 against float16 input on the four routes that read 2-byte samples where they lie, and append the table to profiles/r12_half_input.txt.

    python scripts/bench_half_input.py [--steps 20] [--warmup 3] [--out profiles/r12_half_input.txt]

Routes (power spectrum, linear detrend + Hann, as bench.py's headline): the headline group of 4 x 4096^2 slabs (FastY), 256^2 slabs (FastS), 65 536-sample rows
(FastR), 50^2 slabs (FastG).  Each line: milliseconds per call (median of --steps, HIP events), the algorithmic bytes per point of the route with either input,
and the ratio of the two times.  The plans are executed directly (engine.SpectralPlan), so the figures are the kernels', not the host's.  bench.py is the yardstick
of the project and is not touched by this script."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import scipy.signal as sps
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from xrft_amd import _lib as L  # noqa: E402
from xrft_amd import engine  # noqa: E402

# (label, make arguments, bytes per point with float32 input, with half input)
ROUTES = [
    ("headline fasty 4 x 4096^2", dict(ndim=2, batch=4, ny=4096, nx=4096), 16.4, 14.4),
    ("fasts 4096 x 256^2", dict(ndim=2, batch=4096, ny=256, nx=256), 8.0, 6.0),
    ("fastr 2048 x 65536", dict(ndim=1, batch=2048, ny=1, nx=65536), 12.0, 10.0),
    ("fastg 65536 x 50^2", dict(ndim=2, batch=65536, ny=50, nx=50), 8.0, 6.0),
]


def time_plan(kw, dtype, steps, warmup):
    wins = dict(window_x=sps.windows.hann(kw["nx"], sym=False))
    if kw["ndim"] == 2:
        wins["window_y"] = sps.windows.hann(kw["ny"], sym=False)
    p = engine.SpectralPlan(dtype=dtype, out_mode=L.OUT_POWER, detrend=L.DETREND_LINEAR, flags=L.SHIFT_X | (L.SHIFT_Y if kw["ndim"] == 2 else 0), scale=1.0, **kw, **wins)
    shape = (kw["batch"], kw["ny"], kw["nx"]) if kw["ndim"] == 2 else (kw["batch"], kw["nx"])
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) + 1.0).to(torch.float16).to(dtype)
    out, _ = p.execute(x)
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        p.execute(x, out=out)
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), p.describe().splitlines()[1].strip()[:60], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r12_half_input.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L.load()
    lines = [f"## measured {time.strftime('%Y-%m-%d')} on {torch.cuda.get_device_name(0)}: power spectrum, linear detrend + Hann, median of {a.steps} calls (HIP events)",
             f"{'route':30s} {'float32 ms':>11s} {'float16 ms':>11s} {'f32/f16':>8s} {'B/pt f32':>9s} {'B/pt f16':>9s}  same bits"]
    for label, kw, b32, b16 in ROUTES:
        t32, d32, o32 = time_plan(kw, torch.float32, a.steps, a.warmup)
        t16, d16, o16 = time_plan(kw, torch.float16, a.steps, a.warmup)
        lines.append(f"{label:30s} {t32:11.4f} {t16:11.4f} {t32 / t16:8.3f} {b32:9.1f} {b16:9.1f}  {bool(torch.equal(o32, o16))}")
        del o32, o16
        engine.clear_workspaces()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "a") as fh:
        fh.write("\n" + text)


if __name__ == "__main__":
    main()
