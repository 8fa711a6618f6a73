"""Times fir_filter along a LEADING dim -- the column layout of the overlap-save pass (xrfthip_desc.seg_filter_cols; csrc/fastf.h fastf_kernel<.., true>: the
columns read where they lie, the result written in the array's own order) -- against the route before it on the same build, reached with
XRFTHIP_FASTW_FILTER_COLS=0: one transposed copy of the array, the rows kernel, the result moved back as a view.  That view is made contiguous in the dims' own
order, so that both sides deliver the same thing ("arranged ms"); the time without that last step is reported too ("as a view ms").  One process on one GPU, on the
pattern of scripts/bench_fir_filter.py: every class runs the routes alternating after a warm-up of each; a call is timed with device events around the whole product
call; the median of the timed calls is reported with the spread of the medians of three thirds of them; the peak device memory over the resident input is torch's
allocator's.  Per class also the share of the measured copy bandwidth (a device copy of the array: 4 bytes read and 4 written per sample, what the column route moves)
its time stands for.  XRFTHIP_MEAN_ALL=1 is set: every class the kernel takes is measured, whatever the default routing keeps.  Verdict per class: "faster" where arranged - columns exceeds the two spreads, else "not faster".
Writes the table behind the marker line of profiles/r30_fir_filter_cols.txt (what stands in front of it is kept).

    python scripts/bench_fir_filter_cols.py [--calls 12] [--out FILE] [--small]
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

MARK = "== timings (scripts/bench_fir_filter_cols.py)"
# (shape, dims, slice of the last dim or None, K, nfft or None = the default): float32, resident; taps scipy.signal.firwin(K, 0.2), mode "same"
CUBE, DIMS = (4096, 256, 256), ("time", "y", "x")
CASES = [(CUBE, DIMS, None, 17, None), (CUBE, DIMS, None, 65, None), (CUBE, DIMS, None, 129, None),
         (CUBE, DIMS, None, 65, 128), (CUBE, DIMS, None, 65, 256), (CUBE, DIMS, None, 65, 512), (CUBE, DIMS, None, 257, 512),
         ((4, 2048, 256, 256), ("member", "time", "lat", "lon"), None, 65, None),
         ((4096, 65536 + 4096), ("time", "x"), slice(1024, 1024 + 65536), 65, None),  # a slice of the last dim: S > inner
         ((8192, 4096, 8), ("y", "time", "x"), None, 65, None)]  # a narrow grid: 8192 blocks of inner = 8 columns, half of every group of 16 live
SMALL = [((1024, 8, 8), DIMS, None, 65, None), ((2, 512, 4, 8), ("member", "time", "lat", "lon"), None, 17, 128), ((512, 40), ("time", "x"), slice(4, 36), 65, None),
         ((16, 512, 8), ("y", "time", "x"), None, 65, None)]


def one_call(da, taps, nfft, route):
    """route: "columns" | "arranged" (the knob off, the result made contiguous) | "view" (the knob off, the result as it comes)."""
    os.environ["XRFTHIP_FASTW_FILTER_COLS"] = "1" if route == "columns" else "0"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = xa.fir_filter(da, "time", taps, "same", nfft=nfft).data
    if route == "arranged":
        res = res.contiguous()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    newest = [p for p in api._plan_cache.values() if getattr(p, "seg_filter", 0)]
    tag = bool(newest) and newest[-1].seg_filter_cols == 1
    return a.elapsed_time(b), peak, tag, res


def copy_ms(t, calls):
    t = t.contiguous()
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
    routes = ("columns", "arranged", "view")
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; float32, resident; taps firwin(K, 0.2), mode 'same'; median of {calls} calls per route, the three routes "
             "alternating, after 2 warm-up calls of each; +- = the spread of the medians of three thirds of the calls; arranged = XRFTHIP_FASTW_FILTER_COLS=0 (the "
             "transposed copy, the rows kernel) and the result made contiguous in the dims' order; as a view = the same without that last step; peak = "
             "torch.cuda.max_memory_allocated over the resident input; copy share = (8 bytes per sample / columns time) / (8 bytes per sample / time of a device copy of "
             "the array); nfft marked * is the default",
             f"{'class':64s} {'nfft':>6s} {'columns ms':>11s} {'+-':>6s} {'arranged ms':>12s} {'+-':>6s} {'ratio':>7s} {'as a view ms':>13s} {'+-':>6s} {'copy GB/s':>10s} "
             f"{'copy share':>11s} {'result MB':>10s} {'columns peak MB':>16s} {'arranged peak MB':>17s} {'view peak MB':>13s}  route, verdict"]
    for shape, dims, cut, k, nfft in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
        t = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
        if cut is not None:
            t = t[..., cut]
            coords[dims[-1]] = coords[dims[-1]][cut]
        da = xa.DataArray(t, dims, coords)
        taps = scipy.signal.firwin(k, 0.2)
        cms = copy_ms(t, calls)
        default = _segments._fir_default_nfft(k, shape[dims.index("time")])
        l = default if nfft is None else nfft
        api.clear_plan_cache()
        torch.cuda.empty_cache()
        for _ in range(2):
            for route in routes:
                one_call(da, taps, l, route)
        ms = {r: [] for r in routes}
        peak = {r: 0 for r in routes}
        on, nres = False, 0
        for _ in range(calls):
            for route in routes:
                dt, pk, tag, res = one_call(da, taps, l, route)
                nres = res.numel() * res.element_size()
                del res
                ms[route].append(dt)
                peak[route] = max(peak[route], pk)
                on = on or (route == "columns" and tag)
        mc, ma, mv = (statistics.median(ms[r]) for r in routes)
        sc, sa, sv = (spread(ms[r]) for r in routes)
        nin = t.numel() * t.element_size()
        copy_bw = 2.0 * nin / (cms * 1e-3)
        share = (float(nin + nres) / (mc * 1e-3)) / copy_bw
        name = f"fir_filter {tuple(t.shape)} along {dims.index('time')} K={k}" + ("" if cut is None else f" (a slice of {shape[-1]})")
        verdict = "faster" if ma - mc > sc + sa else "not faster"
        lines.append(f"{name:64s} {str(l) + ('*' if l == default else ''):>6s} {mc:11.3f} {sc:6.3f} {ma:12.3f} {sa:6.3f} {mc / ma:7.3f} {mv:13.3f} {sv:6.3f} {copy_bw / 1e9:10.1f} "
                     f"{share:11.3f} {nres / 2**20:10.1f} {peak['columns'] / 2**20:16.1f} {peak['arranged'] / 2**20:17.1f} {peak['view'] / 2**20:13.1f}  "
                     f"{'fastw plan, overlap-save, columns' if on else 'arranged (no column plan)'}, {verdict}")
        print(lines[-1], flush=True)
        del da, t
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    os.environ.pop("XRFTHIP_FASTW_FILTER_COLS", None)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r30_fir_filter_cols.txt")
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
