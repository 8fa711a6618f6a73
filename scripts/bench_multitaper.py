"""Times multitaper_power_spectrum / multitaper_cross_spectrum -- every taper's transform of a series in ONE pass (xrfthip_desc.seg_tapers; csrc/fastt.h: the series read
once, one spectrum per series written, neither the K tapered copies nor the K spectra stored) -- against the composed route on the same build: the library's detrend,
a taper dim by broadcasting the table, zero-extension, power_spectrum / cross_spectrum, the weighted sum (what a user of the library without the feature writes;
reached here with XRFTHIP_FASTW_TAPERS=0).  One process on one GPU, on the pattern of scripts/bench_fir_filter.py: every class runs both routes alternating after a
warm-up of both; each call is timed with device events around the whole product call (linear detrend: both routes pay its non-finite check); the median of the timed
calls is reported with the spread of the medians of three thirds of them; the peak device memory over the resident input is torch's allocator's.  Per class also
the share of the measured copy bandwidth (a device copy of the series, 4 bytes read and 4 written per sample) that the fused route's own traffic -- the series read,
the spectra written -- stands for.  Verdict per class: "faster" where composed - fused exceeds the two spreads, else "not faster".
Writes the table behind the marker line of profiles/r29_multitaper.txt (what stands in front of it is kept).

    python scripts/bench_multitaper.py [--calls 12] [--out FILE] [--small]
"""
import argparse
import os
import statistics
import sys
import warnings

os.environ.setdefault("XRFTHIP_MEAN_ALL", "1")  # every class the kernel takes is measured, whatever the default routing keeps

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xrft_amd as xa  # noqa: E402
from xrft_amd import api  # noqa: E402

MARK = "== timings (scripts/bench_multitaper.py)"
# (shape of the series, dims, K, cross?): float32 series, resident; NW = (K + 1) / 2, linear detrend, unity weights
CASES = [((1048576, 256), ("x", "time"), 7, False), ((262144, 1024), ("x", "time"), 7, False), ((65536, 4096), ("x", "time"), 5, False),
         ((65536, 4096), ("x", "time"), 15, False), ((262144, 1000), ("x", "time"), 7, False), ((262144, 1024), ("x", "time"), 7, True),
         ((1024, 256, 256), ("time", "y", "x"), 7, False)]
SMALL = [((64, 256), ("x", "time"), 7, False), ((8, 1000), ("x", "time"), 7, True), ((100, 8, 8), ("time", "y", "x"), 3, False)]


def one_call(da, da2, k, fused):
    os.environ["XRFTHIP_FASTW_TAPERS"] = "1" if fused else "0"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    kw = dict(NW=0.5 * (k + 1), K=k, detrend="linear")
    res = xa.multitaper_power_spectrum(da, "time", **kw) if da2 is None else xa.multitaper_cross_spectrum(da, da2, "time", **kw)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    tag = fused and any(getattr(p, "seg_tapers", 0) for p in api._plan_cache.values())
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


def spread(ms):
    k = len(ms) // 3
    meds = [statistics.median(ms[i * k:(i + 1) * k if i < 2 else len(ms)]) for i in range(3)]
    return max(meds) - min(meds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12, help="timed calls per route (at least 12), after two warm-up calls of each")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "this script measures on a GPU"
    calls = max(args.calls, 12)
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; float32 series, resident; NW = (K + 1) / 2, unity weights, linear detrend; median of {calls} calls per route, the two "
             "routes alternating, after 2 warm-up calls of each; +- = the spread of the medians of three thirds of the calls; peak = torch.cuda.max_memory_allocated over the "
             "resident series; copy share = ((input + result bytes) / fused time) / (bandwidth of a device copy of the series)",
             f"{'class':58s} {'L':>5s} {'fused ms':>9s} {'+-':>6s} {'composed ms':>12s} {'+-':>6s} {'ratio':>7s} {'copy GB/s':>10s} {'copy share':>11s} {'result MB':>10s} "
             f"{'fused peak MB':>14s} {'composed peak MB':>17s}  route, verdict"]
    for shape, dims, k, cross in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
        da = xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), dims, coords)
        da2 = xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), dims, coords) if cross else None
        cms = copy_ms(da.data, calls)
        n = shape[dims.index("time")]
        name = f"{'cross' if cross else 'power'} {shape} along {dims.index('time')} K={k}"
        api.clear_plan_cache()
        torch.cuda.empty_cache()
        try:
            for _ in range(2):
                for fused in (True, False):
                    one_call(da, da2, k, fused)
        except (RuntimeError, xa.XrftHipError) as e:  # (a class one of the routes cannot hold in memory: named, not measured)
            lines.append(f"{name}: not measured ({type(e).__name__}: {str(e)[:80]})")
            print(lines[-1], flush=True)
            continue
        t = {True: [], False: []}
        peak = {True: 0, False: 0}
        on, nres, l = False, 0, 0
        for _ in range(calls):
            for fused in (True, False):
                ms, pk, tag, res = one_call(da, da2, k, fused)
                nres, l = res.data.numel() * res.data.element_size(), res.shape[-1]
                del res
                t[fused].append(ms)
                peak[fused] = max(peak[fused], pk)
                on = on or tag
        mf, mc, sf, sc = statistics.median(t[True]), statistics.median(t[False]), spread(t[True]), spread(t[False])
        nin = da.data.numel() * da.data.element_size() * (2 if cross else 1)
        copy_bw = 2.0 * da.data.numel() * da.data.element_size() / (cms * 1e-3)
        share = (float(nin + nres) / (mf * 1e-3)) / copy_bw
        verdict = "faster" if mc - mf > sf + sc else "not faster"
        lines.append(f"{name:58s} {l:5d} {mf:9.3f} {sf:6.3f} {mc:12.3f} {sc:6.3f} {mf / mc:7.3f} {copy_bw / 1e9:10.1f} {share:11.3f} "
                     f"{nres / 2**20:10.1f} {peak[True] / 2**20:14.1f} {peak[False] / 2**20:17.1f}  {'fastw plan, tapers' if on else 'composed (the plan declined)'}, {verdict}")
        print(lines[-1], flush=True)
        del da, da2
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    os.environ.pop("XRFTHIP_FASTW_TAPERS", None)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r29_multitaper.txt")
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
