"""Times spectrogram / stft -- every overlapping segment's spectrum from ONE pass that reads the segments where they lie (xrfthip_desc.seg_keep; csrc/fastk.h) --
against the composition they replace on the same build: the segments unfolded (tensor.unfold) and copied, the plain 1-D plan over the array of segments, the dims
moved (what a user of the library without the feature writes; reached here with XRFTHIP_FASTW_KEEP=0).  One process on one GPU, on the pattern of
scripts/bench_welch.py: every class runs both routes alternating after a warm-up of both; each call is timed with device events around the whole product call; the
median of the timed calls is reported with the spread of the medians of three thirds of them; the peak device memory over the resident input is torch's allocator's.
Per class also the bytes the fused route moves per sample of the series (4 per sample read, the result out) and the share of the measured copy bandwidth (a device
copy of the series: 8 bytes per sample) its time stands for.  Verdict per class: "faster" where composed - fused exceeds the two spreads, else "not faster".
XRFTHIP_MEAN_ALL=1 is set: every class the kernel takes is measured, whatever the default routing keeps.
Writes the table behind the marker line of profiles/r21_spectrogram.txt (what stands in front of it is kept).

    python scripts/bench_spectrogram.py [--calls 12] [--out FILE] [--small]
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

MARK = "== timings (scripts/bench_spectrogram.py)"
KW = dict(detrend="linear", window="hann")
# (shape, dims, nperseg, noverlap, one-sided output, stft): float32, linear + Hann.  Trailing axis: L = 256 / 1024 / 4096, each at 50 % overlap and at none, full and
# one-sided; the leading axis of a cube at L = 64 / 256 / 512; one stft class
ROWS = [((65536, 16384), 256), ((4096, 262144), 1024), ((256, 4194304), 4096)]
CASES = [(shape, ("x", "time"), L, ov, half, False) for shape, L in ROWS for ov in (L // 2, 0) for half in (False, True)]
CASES += [((4096, 512, 512), ("time", "y", "x"), L, L // 2, False, False) for L in (64, 256, 512)]
CASES += [((4096, 262144), ("x", "time"), 1024, 512, False, True)]
SMALL = [((8, 4096), ("x", "time"), 256, 128, False, False), ((8, 4096), ("x", "time"), 64, 0, True, False), ((512, 8, 8), ("time", "y", "x"), 64, 32, False, False),
         ((4, 4096), ("x", "time"), 1024, 512, False, True)]


def one_call(da, nperseg, noverlap, half, stft, fused):
    os.environ["XRFTHIP_FASTW_KEEP"] = "1" if fused else "0"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    kw = dict(KW, real_dim="time") if half else KW
    res = xa.stft(da, "time", nperseg, noverlap, **kw) if stft else xa.spectrogram(da, "time", nperseg, noverlap, **kw)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    tag = fused and any(getattr(p, "seg_keep", 0) for p in api._plan_cache.values())
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
    ap.add_argument("--calls", type=int, default=12, help="timed calls per route (at least 10), after two warm-up calls of each")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="toy shapes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    assert torch.cuda.is_available(), "this script measures on a GPU"
    calls = max(args.calls, 10)
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; float32, linear + Hann; median of {calls} calls per route, the two routes alternating, after 2 warm-up calls of "
             "each; +- = the spread of the medians of three thirds of the calls; peak = torch.cuda.max_memory_allocated over the resident input; B/sample = bytes the "
             "fused route moves per sample of the series (4 per sample read + the result); copy share = (fused bytes / fused time) / (8 bytes per sample / time of a "
             "device copy of the series)",
             f"{'class':58s} {'fused ms':>9s} {'+-':>6s} {'composed ms':>12s} {'+-':>6s} {'ratio':>7s} {'B/sample':>9s} {'copy GB/s':>10s} {'copy share':>11s} {'fused peak MB':>14s} "
             f"{'composed peak MB':>17s}  route, verdict"]
    for shape, dims, nperseg, noverlap, half, stft in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {d: np.arange(k) * 1.0 for d, k in zip(dims, shape)}
        da = xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), dims, coords)
        cms = copy_ms(da.data, calls)
        for _ in range(2):
            for fused in (True, False):
                one_call(da, nperseg, noverlap, half, stft, fused)
        t = {True: [], False: []}
        peak = {True: 0, False: 0}
        on, nres = False, 0
        for _ in range(calls):
            for fused in (True, False):
                ms, pk, tag, res = one_call(da, nperseg, noverlap, half, stft, fused)
                nres = res.data.numel() * res.data.element_size()
                del res
                t[fused].append(ms)
                peak[fused] = max(peak[fused], pk)
                on = on or tag
        mf, mc, sf, sc = statistics.median(t[True]), statistics.median(t[False]), spread(t[True]), spread(t[False])
        samples = int(np.prod(shape))
        moved = 4.0 * samples + nres
        copy_bw = 8.0 * samples / (cms * 1e-3)
        share = (moved / (mf * 1e-3)) / copy_bw
        name = f"{'stft' if stft else 'spectrogram'} {shape} along {dims.index('time')} L={nperseg} hop={nperseg - noverlap}{' one-sided' if half else ''}"
        verdict = "faster" if mc - mf > sf + sc else "not faster"
        lines.append(f"{name:58s} {mf:9.3f} {sf:6.3f} {mc:12.3f} {sc:6.3f} {mf / mc:7.3f} {moved / samples:9.3f} {copy_bw / 1e9:10.1f} {share:11.3f} {peak[True] / 2**20:14.1f} "
                     f"{peak[False] / 2**20:17.1f}  {'fastw plan, segments kept' if on else 'composed (the plan declined)'}, {verdict}")
        print(lines[-1], flush=True)
        del da
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    os.environ.pop("XRFTHIP_FASTW_KEEP", None)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r21_spectrogram.txt")
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
