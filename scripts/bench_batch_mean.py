"""Times mean_power_spectrum / mean_cross_spectrum -- the mean over the batch inside the last pass (xrfthip_desc.mean_batch; csrc/fasty_mean.h, csrc/fasts_mean.h) --
against the composition they replace, power_spectrum(...).mean(dim) (the plain plan, then xrfthip_reduce_axis), in one process on one GPU: every case runs both
routes alternating after a warm-up of both; each call is timed with device events around the whole product call, the median of the timed calls is reported, and the
peak device memory over the resident input is taken from torch's allocator.  Writes the table behind the marker line of profiles/r15_batch_mean.txt (what stands
in front of it -- the kernels' resources -- is kept).

    python scripts/bench_batch_mean.py [--calls 12] [--out FILE] [--small]
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
from xrft_amd import api, engine  # noqa: E402

MARK = "== timings (scripts/bench_batch_mean.py)"
CASES = [  # (operation, (nt, ny, nx), keyword arguments)
    ("power", (64, 4096, 4096), dict(detrend="linear", window="hann")),
    ("power", (256, 1024, 1024), {}),
    ("power", (4096, 256, 256), {}),
    ("power", (16384, 128, 128), {}),
    ("power", (65536, 64, 64), {}),
    ("cross", (64, 2048, 2048), {}),
    # the classes between them: one leg per row kernel (nx) and mode of the two-pass pipeline, and the one-pass slabs with one 64-point axis
    ("power", (1024, 512, 512), {}),
    ("power", (128, 2048, 2048), {}),
    ("cross", (2048, 256, 256), {}),
    ("cross", (1024, 512, 512), {}),
    ("cross", (256, 1024, 1024), {}),
    ("cross", (32, 4096, 4096), {}),
    ("power", (32768, 64, 128), {}),
    ("power", (32768, 128, 64), {}),
]
SMALL = [("power", (8, 256, 256), dict(detrend="linear", window="hann")), ("power", (12, 64, 128), {}), ("cross", (6, 256, 256), {})]


def one_call(op, fields, kw, fused):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if op == "power":
        res = xa.mean_power_spectrum(fields[0], "time", dim=["y", "x"], **kw) if fused else xa.power_spectrum(fields[0], dim=["y", "x"], **kw).mean("time")
    else:
        res = xa.mean_cross_spectrum(fields[0], fields[1], "time", dim=["y", "x"], **kw) if fused else xa.cross_spectrum(fields[0], fields[1], dim=["y", "x"], **kw).mean("time")
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    p = next(reversed(api._plan_cache.values()))
    return a.elapsed_time(b), peak, p.mean_batch > 1, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12, help="timed calls per route (at least 10), after two warm-up calls of each")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "this script measures on a GPU"
    calls = max(args.calls, 10)
    # every call computes everything: with the reuse of the column pass on, the plain plan of the composed route reads the pass-1 block the mean plan has just left for
    # the same field (the two routes alternate), and its time comes out one column pass short
    engine.reuse_column_pass(False)
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; median of {calls} calls per route, the two routes alternating, after 2 warm-up calls of each; "
             "peak = torch.cuda.max_memory_allocated over the resident input(s)",
             f"{'case':44s} {'fused ms':>10s} {'composed ms':>12s} {'ratio':>7s} {'fused peak MB':>14s} {'composed peak MB':>17s}  route"]
    for op, shape, kw in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {"time": np.arange(shape[0]), "y": np.arange(shape[1]) * 1.0, "x": np.arange(shape[2]) * 1.0}
        fields = [xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), ("time", "y", "x"), coords) for _ in range(2 if op == "cross" else 1)]
        for _ in range(2):
            for fused in (True, False):
                one_call(op, fields, kw, fused)
        t = {True: [], False: []}
        peak = {True: 0, False: 0}
        on = False
        for _ in range(calls):
            for fused in (True, False):
                ms, pk, tag, res = one_call(op, fields, kw, fused)
                del res
                t[fused].append(ms)
                peak[fused] = max(peak[fused], pk)
                on = on or (fused and tag)
        mf, mc = statistics.median(t[True]), statistics.median(t[False])
        name = f"{op} {shape}" + (" linear + Hann" if kw else "")
        lines.append(f"{name:44s} {mf:10.3f} {mc:12.3f} {mf / mc:7.3f} {peak[True] / 2**20:14.1f} {peak[False] / 2**20:17.1f}  {'mean plan' if on else 'composed (the plan declined)'}")
        print(lines[-1], flush=True)
        del fields
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r15_batch_mean.txt")
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
