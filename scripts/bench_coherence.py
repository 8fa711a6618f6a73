"""Times coherence(...) -- the magnitude-squared coherence from ONE row pass (XRFTHIP_OUT_COHERENCE; csrc/fasty_mean.h, fasty_rows_mean_kernel<NX, 3>) -- against
the composition it replaces on the same commit: mean_cross_spectrum, mean_power_spectrum of each field (three mean plans, three row passes, three results) and
xrfthip_coherence.  One process on one GPU, on the pattern of scripts/bench_batch_mean.py: every case runs both routes alternating after a warm-up of both; each call
is timed with device events around the whole product call, the median of the timed calls is reported, and the peak device memory over the resident inputs is taken from
torch's allocator.  Writes the table behind the marker line of profiles/r17_coherence.txt (what stands in front of it -- the kernels' resources -- is kept).

    python scripts/bench_coherence.py [--calls 12] [--out FILE] [--small]
"""
import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xrft_amd as xa  # noqa: E402
from xrft_amd import _lib, api, engine  # noqa: E402

MARK = "== timings (scripts/bench_coherence.py)"
KW = dict(dim=["y", "x"], detrend="linear", window="hann")
CASES = [(64, 4096, 4096), (256, 1024, 1024), (4096, 256, 256), (64, 2048, 2048)]  # float32, linear + Hann
SMALL = [(6, 256, 256), (4, 256, 512)]


def one_call(fields, fused):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if fused:
        res = xa.coherence(fields[0], fields[1], "time", **KW)
    else:
        res = engine.coherence(xa.mean_cross_spectrum(fields[0], fields[1], "time", **KW).data, xa.mean_power_spectrum(fields[0], "time", **KW).data,
                               xa.mean_power_spectrum(fields[1], "time", **KW).data)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    tag = fused and any(p.out_mode == _lib.OUT_COHERENCE for p in api._plan_cache.values())
    return a.elapsed_time(b), peak, tag, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12, help="timed calls per route (at least 10), after two warm-up calls of each")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "this script measures on a GPU"
    calls = max(args.calls, 10)
    # every call computes everything: with the reuse of the column pass on, each plan of the composed route reads the pass-1 blocks the plan before it has just left
    # for the same fields (the routes alternate), and the comparison would be of the row passes alone
    engine.reuse_column_pass(False)
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; float32, linear + Hann; median of {calls} calls per route, the two routes alternating, after 2 warm-up calls of "
             "each; reuse of the column pass off; peak = torch.cuda.max_memory_allocated over the resident inputs",
             f"{'case':28s} {'fused ms':>10s} {'composed ms':>12s} {'ratio':>7s} {'fused peak MB':>14s} {'composed peak MB':>17s}  route"]
    for shape in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {"time": np.arange(shape[0]), "y": np.arange(shape[1]) * 1.0, "x": np.arange(shape[2]) * 1.0}
        fields = [xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), ("time", "y", "x"), coords) for _ in range(2)]
        for _ in range(2):
            for fused in (True, False):
                one_call(fields, fused)
        t = {True: [], False: []}
        peak = {True: 0, False: 0}
        on = False
        for _ in range(calls):
            for fused in (True, False):
                ms, pk, tag, res = one_call(fields, fused)
                del res
                t[fused].append(ms)
                peak[fused] = max(peak[fused], pk)
                on = on or tag
        mf, mc = statistics.median(t[True]), statistics.median(t[False])
        lines.append(f"{'coherence ' + str(shape):28s} {mf:10.3f} {mc:12.3f} {mf / mc:7.3f} {peak[True] / 2**20:14.1f} {peak[False] / 2**20:17.1f}  {'coherence plan' if on else 'composed (the plan declined)'}")
        print(lines[-1], flush=True)
        del fields
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r17_coherence.txt")
    head = []
    if os.path.exists(out):
        with open(out) as fh:
            for ln in fh.read().splitlines():
                if ln.startswith(MARK):
                    break
                head.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(head + lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
