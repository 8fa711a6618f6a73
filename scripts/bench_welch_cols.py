"""Times welch_power_spectrum / welch_cross_spectrum along a LEADING time axis -- the (time, y, x) cube read where it lies by the column layout of the Welch plan
(xrfthip_desc.seg_stride; csrc/fastw.h) -- against the route of the commit before it, which stays reachable in the same build through XRFTHIP_FASTW_COLS=0 (one
transposed copy of the cube, then the rows layout), and against the composition (the segments unfolded, the plain 1-D plan, .mean).  One process on one GPU, on
the pattern of scripts/bench_welch.py: every case runs the three routes alternating after two warm-up calls of each; each call is timed with device events around
the whole product call, the median of the timed calls is reported, with the spread (min .. max) of the copy route, the yardstick; the peak device memory over the
resident input is taken from torch's allocator.  XRFTHIP_MEAN_ALL=1 is set: every class the kernel takes is measured, whatever the default routing keeps.
Writes the table behind the marker line of profiles/r20_welch_cols.txt (what stands in front of it is kept).

    python scripts/bench_welch_cols.py [--calls 10] [--out FILE] [--small] [--no-composed]
"""
import argparse
import os
import statistics
import sys
import warnings

os.environ.setdefault("XRFTHIP_MEAN_ALL", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xrft_amd as xa  # noqa: E402
from xrft_amd import api  # noqa: E402

MARK = "== timings (scripts/bench_welch_cols.py)"
KW = dict(detrend="linear", window="hann")
ROUTES = ("in place", "copy + rows", "composed")
# (shape, dims, nperseg, noverlap, two fields): float32, linear + Hann; the cube at every length of the column layout with half overlap and with none, one
# (member, time, y, x) array, one cross spectrum
CUBE = ((4096, 512, 512), ("time", "y", "x"))
CASES = [CUBE + (n, ov, False) for n in (64, 128, 256, 512) for ov in (n // 2, 0)] + [((4, 2048, 256, 256), ("member", "time", "y", "x"), 128, 64, False),
                                                                                      ((4096, 256, 256), ("time", "y", "x"), 128, 64, True)]
SMALL = [((512, 16, 16), ("time", "y", "x"), n, n // 2, False) for n in (64, 256, 512)] + [((2, 512, 8, 8), ("member", "time", "y", "x"), 128, 64, False),
                                                                                            ((512, 16, 16), ("time", "y", "x"), 128, 0, True)]


def composed(fields, nperseg, hop):
    segs = [api._welch_segments(f, "time", nperseg, hop) for f in fields]
    if len(segs) == 1:
        return xa.power_spectrum(segs[0], dim=["time"], **KW).mean("time_segment")
    return xa.cross_spectrum(segs[0], segs[1], dim=["time"], **KW).mean("time_segment")


def one_call(fields, nperseg, noverlap, route):
    os.environ["XRFTHIP_FASTW_COLS"] = "0" if route == "copy + rows" else "1"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if route == "composed":
        res = composed(fields, nperseg, nperseg - noverlap)
    elif len(fields) == 1:
        res = xa.welch_power_spectrum(fields[0], "time", nperseg, noverlap, **KW)
    else:
        res = xa.welch_cross_spectrum(fields[0], fields[1], "time", nperseg, noverlap, **KW)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    cols = any("[fastw columns]" in p.describe() for p in api._plan_cache.values())
    return a.elapsed_time(b), peak, cols, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="timed calls per route (at least 10), after two warm-up calls of each")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--no-composed", action="store_true", help="leave the composition out (it holds every segment's spectrum)")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "this script measures on a GPU"
    calls = max(args.calls, 10)
    routes = ROUTES[:2] if args.no_composed else ROUTES
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; float32, linear + Hann; median of {calls} calls per route, the routes alternating, after 2 warm-up calls of "
             "each; copy + rows = XRFTHIP_FASTW_COLS=0, the route of the commit before (its min .. max: the spread the verdict is held against); peak = "
             "torch.cuda.max_memory_allocated over the resident input; verdict: 'slower' where the in-place median lies above the copy route's max",
             f"{'case':58s} {'in place ms':>12s} {'copy+rows ms':>13s} {'(min .. max)':>20s} {'ratio':>7s} {'composed ms':>12s} {'in place peak MB':>17s} {'copy peak MB':>13s} {'composed peak MB':>17s}  verdict"]
    for shape, dims, nperseg, noverlap, two in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
        fields = [xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), dims, coords) for _ in range(2 if two else 1)]
        api.clear_plan_cache()
        t = {r: [] for r in routes}
        peak = {r: 0 for r in routes}
        on = False
        for i in range(calls + 2):
            for r in routes:
                ms, pk, cols, res = one_call(fields, nperseg, noverlap, r)
                del res
                if i >= 2:
                    t[r].append(ms)
                    peak[r] = max(peak[r], pk)
                on = on or cols
        mi, mp = statistics.median(t["in place"]), statistics.median(t["copy + rows"])
        mc = statistics.median(t["composed"]) if "composed" in t else float("nan")
        verdict = ("faster" if mi < min(t["copy + rows"]) else "slower" if mi > max(t["copy + rows"]) else "within the spread") if on else "the column plan declined"
        name = f"{'cross' if two else 'power'} {shape} L={nperseg} hop={nperseg - noverlap}"
        lines.append(f"{name:58s} {mi:12.3f} {mp:13.3f} {'(%.3f .. %.3f)' % (min(t['copy + rows']), max(t['copy + rows'])):>20s} {mi / mp:7.3f} {mc:12.3f} "
                     f"{peak['in place'] / 2**20:17.1f} {peak['copy + rows'] / 2**20:13.1f} {peak.get('composed', 0) / 2**20:17.1f}  {verdict}")
        print(lines[-1], flush=True)
        del fields
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    os.environ.pop("XRFTHIP_FASTW_COLS", None)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_welch_cols.txt")
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
