"""Times fir_filter -- FIR filtering along a dim by overlap-save in ONE pass (xrfthip_desc.seg_filter; csrc/fastf.h: the series read once, the filtered series written
once, no spectrum stored) -- against the composed route on the same build: a zero-extended copy, the segments unfolded, the real 1-D plan, the table product, the
C2R plan, the kept samples sliced out (what a user of the library without the feature writes; reached here with XRFTHIP_FASTW_FILTER=0).  One process on one GPU,
on the pattern of scripts/bench_istft.py: every class runs both routes alternating after a warm-up of both; each call is timed with device events around the whole
product call; the median of the timed calls is reported with the spread of the medians of three thirds of them; the peak device memory over the resident input is
torch's allocator's.  Per class also the share of the measured copy bandwidth (a device copy of the series: 4 bytes read and 4 written per sample, what the fused
route moves) its time stands for.  Verdict per class: "faster" where composed - fused exceeds the two spreads, else "not faster".  Every class is run at the default
``nfft`` and, per K, at every admitted power of two (K - 1 <= nfft / 2, 64 .. 4096): the sweep the default rule is set from.  XRFTHIP_MEAN_ALL=1 is set: every class
the kernel takes is measured, whatever the default routing keeps.
Writes the table behind the marker line of profiles/r27_fir_filter.txt (what stands in front of it is kept).

    python scripts/bench_fir_filter.py [--calls 12] [--out FILE] [--small]
"""
import argparse
import os
import statistics
import sys
import warnings

os.environ.setdefault("XRFTHIP_MEAN_ALL", "1")  # every class the kernel takes is measured, whatever the default routing keeps

import numpy as np  # noqa: E402
import scipy.signal  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xrft_amd as xa  # noqa: E402
from xrft_amd import _segments, api  # noqa: E402

MARK = "== timings (scripts/bench_fir_filter.py)"
# (shape of the series, dims, K): float32 series, resident; taps scipy.signal.firwin(K, 0.2), mode "same".  Trailing axis; and the leading axis of a cube (arranged
# first: one transposed copy of the cube)
CASES = [((65536, 16384), ("x", "time"), 17), ((65536, 16384), ("x", "time"), 65), ((65536, 16384), ("x", "time"), 129), ((4096, 262144), ("x", "time"), 257),
         ((256, 4194304), ("x", "time"), 1025), ((256, 4194304), ("x", "time"), 2049), ((4096, 256, 256), ("time", "y", "x"), 65)]
SMALL = [((8, 4096), ("x", "time"), 17), ((4, 8192), ("x", "time"), 257), ((1024, 8, 8), ("time", "y", "x"), 65)]


def one_call(da, taps, nfft, fused):
    os.environ["XRFTHIP_FASTW_FILTER"] = "1" if fused else "0"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = xa.fir_filter(da, "time", taps, "same", nfft=nfft)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    tag = fused and any(getattr(p, "seg_filter", 0) for p in api._plan_cache.values())
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
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; float32 series, resident; taps firwin(K, 0.2), mode 'same'; median of {calls} calls per route, the two routes "
             "alternating, after 2 warm-up calls of each; +- = the spread of the medians of three thirds of the calls; peak = torch.cuda.max_memory_allocated over the "
             "resident series; copy share = (8 bytes per sample / fused time) / (8 bytes per sample / time of a device copy of the series); nfft marked * is the default",
             f"{'class':52s} {'nfft':>6s} {'fused ms':>9s} {'+-':>6s} {'composed ms':>12s} {'+-':>6s} {'ratio':>7s} {'copy GB/s':>10s} {'copy share':>11s} {'result MB':>10s} "
             f"{'fused peak MB':>14s} {'composed peak MB':>17s}  route, verdict"]
    for shape, dims, k in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
        da = xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), dims, coords)
        taps = scipy.signal.firwin(k, 0.2)
        cms = copy_ms(da.data, calls)
        default = _segments._fir_default_nfft(k, shape[dims.index("time")])
        for nfft in [l for l in (64, 128, 256, 512, 1024, 2048, 4096) if 2 * (k - 1) <= l]:
            api.clear_plan_cache()
            torch.cuda.empty_cache()
            try:
                for _ in range(2):
                    for fused in (True, False):
                        one_call(da, taps, nfft, fused)
            except (RuntimeError, xa.XrftHipError) as e:  # (a class one of the routes cannot hold in memory: named, not measured)
                lines.append(f"fir_filter {shape} along {dims.index('time')} K={k} nfft={nfft}: not measured ({type(e).__name__}: {str(e)[:80]})")
                print(lines[-1], flush=True)
                continue
            t = {True: [], False: []}
            peak = {True: 0, False: 0}
            on, nres = False, 0
            for _ in range(calls):
                for fused in (True, False):
                    ms, pk, tag, res = one_call(da, taps, nfft, fused)
                    nres = res.data.numel() * res.data.element_size()
                    del res
                    t[fused].append(ms)
                    peak[fused] = max(peak[fused], pk)
                    on = on or tag
            mf, mc, sf, sc = statistics.median(t[True]), statistics.median(t[False]), spread(t[True]), spread(t[False])
            nin = da.data.numel() * da.data.element_size()
            copy_bw = 2.0 * nin / (cms * 1e-3)
            share = (float(nin + nres) / (mf * 1e-3)) / copy_bw
            name = f"fir_filter {shape} along {dims.index('time')} K={k}"
            verdict = "faster" if mc - mf > sf + sc else "not faster"
            lines.append(f"{name:52s} {str(nfft) + ('*' if nfft == default else ''):>6s} {mf:9.3f} {sf:6.3f} {mc:12.3f} {sc:6.3f} {mf / mc:7.3f} {copy_bw / 1e9:10.1f} {share:11.3f} "
                         f"{nres / 2**20:10.1f} {peak[True] / 2**20:14.1f} {peak[False] / 2**20:17.1f}  {'fastw plan, overlap-save' if on else 'composed (the plan declined)'}, {verdict}")
            print(lines[-1], flush=True)
        del da
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    os.environ.pop("XRFTHIP_FASTW_FILTER", None)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r27_fir_filter.txt")
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
