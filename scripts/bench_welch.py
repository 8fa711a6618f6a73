"""Times welch_power_spectrum / welch_cross_spectrum -- the overlapping segments of a series read in place and averaged in ONE pass (xrfthip_desc.seg_hop;
csrc/fastw.h) -- against the composition they replace on the same commit: the segments unfolded (tensor.unfold) and copied, the plain 1-D plan over the array of
segments, xrfthip_reduce_axis.  One process on one GPU, on the pattern of scripts/bench_coherence.py: every case runs both routes alternating after a warm-up of
both; each call is timed with device events around the whole product call, the median of the timed calls is reported, and the peak device memory over the resident
input is taken from torch's allocator.  Per case also the bytes the fused route moves per sample of the series (4 in, the result out) and the share of the measured
copy bandwidth (a device copy of the series: 8 bytes per sample) its time stands for.  XRFTHIP_MEAN_ALL=1 is set: every class the kernel takes is measured, whatever
the default routing keeps.  Writes the table behind the marker line of profiles/r19_welch.txt (what stands in front of it is kept).

    python scripts/bench_welch.py [--calls 12] [--out FILE] [--small]
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
from xrft_amd import _lib, api  # noqa: E402

MARK = "== timings (scripts/bench_welch.py)"
KW = dict(detrend="linear", window="hann")
# (series, samples, nperseg, noverlap, two fields): float32, linear + Hann; L x overlap classes 256 / 1024 / 4096 at 50 %, one without overlap, one cross spectrum
CASES = [(65536, 16384, 256, 128, False), (4096, 262144, 1024, 512, False), (256, 4194304, 4096, 2048, False), (4096, 262144, 1024, 0, False), (4096, 262144, 1024, 512, True)]
SMALL = [(8, 4096, 256, 128, False), (8, 4096, 64, 0, False), (4, 4096, 1024, 512, True)]


def composed(fields, nperseg, hop):
    segs = [api._welch_segments(f, "time", nperseg, hop) for f in fields]
    if len(segs) == 1:
        return xa.power_spectrum(segs[0], dim=["time"], **KW).mean("time_segment")
    return xa.cross_spectrum(segs[0], segs[1], dim=["time"], **KW).mean("time_segment")


def one_call(fields, nperseg, noverlap, fused):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if fused:
        res = xa.welch_power_spectrum(fields[0], "time", nperseg, noverlap, **KW) if len(fields) == 1 else xa.welch_cross_spectrum(fields[0], fields[1], "time", nperseg, noverlap, **KW)
    else:
        res = composed(fields, nperseg, nperseg - noverlap)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    tag = fused and any(p.kernel_info()[0] == _lib.K_FASTW for p in api._plan_cache.values())
    return a.elapsed_time(b), peak, tag, res


def copy_ms(t, calls):
    out = torch.empty_like(t)
    ms = []
    for i in range(calls + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out.copy_(t)
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12, help="timed calls per route (at least 10), after two warm-up calls of each")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "this script measures on a GPU"
    calls = max(args.calls, 10)
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; float32, linear + Hann; median of {calls} calls per route, the two routes alternating, after 2 warm-up calls of "
             "each; peak = torch.cuda.max_memory_allocated over the resident input; B/sample = bytes the fused route moves per sample of the series (4 in + the result); "
             "copy share = (fused bytes / fused time) / (8 bytes per sample / time of a device copy of the series)",
             f"{'case':52s} {'fused ms':>9s} {'composed ms':>12s} {'ratio':>7s} {'B/sample':>9s} {'copy GB/s':>10s} {'copy share':>11s} {'fused peak MB':>14s} {'composed peak MB':>17s}  route"]
    for ns, n, nperseg, noverlap, two in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {"x": np.arange(ns), "time": np.arange(n) * 1.0}
        fields = [xa.DataArray(torch.randn((ns, n), generator=g, device="cuda", dtype=torch.float32), ("x", "time"), coords) for _ in range(2 if two else 1)]
        cms = copy_ms(fields[0].data, calls)
        for _ in range(2):
            for fused in (True, False):
                one_call(fields, nperseg, noverlap, fused)
        t = {True: [], False: []}
        peak = {True: 0, False: 0}
        on = False
        for _ in range(calls):
            for fused in (True, False):
                ms, pk, tag, res = one_call(fields, nperseg, noverlap, fused)
                del res
                t[fused].append(ms)
                peak[fused] = max(peak[fused], pk)
                on = on or tag
        mf, mc = statistics.median(t[True]), statistics.median(t[False])
        samples = ns * n * len(fields)
        moved = 4.0 * samples + ns * nperseg * (8 if two else 4)
        copy_bw = 8.0 * ns * n / (cms * 1e-3)
        share = (moved / (mf * 1e-3)) / copy_bw
        name = f"{'cross' if two else 'power'} ({ns}, {n}) L={nperseg} hop={nperseg - noverlap}"
        lines.append(f"{name:52s} {mf:9.3f} {mc:12.3f} {mf / mc:7.3f} {moved / samples:9.3f} {copy_bw / 1e9:10.1f} {share:11.3f} {peak[True] / 2**20:14.1f} {peak[False] / 2**20:17.1f}  "
                     f"{'fastw plan' if on else 'composed (the plan declined)'}")
        print(lines[-1], flush=True)
        del fields
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_welch.txt")
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
