"""Times istft -- a series rebuilt from its short-time transform by ONE pass (xrfthip_desc.seg_synth; csrc/fasto.h: inverse transform, window, overlap-add and the
division by the summed squared windows, no inverse-transformed segment stored) -- against the composed route on the same build: ifft of every segment, the window,
R strided adds, the division (what a user of the library without the feature writes; reached here with XRFTHIP_FASTW_SYNTH=0).  One process on one GPU, on the
pattern of scripts/bench_spectrogram.py: every class runs both routes alternating after a warm-up of both; each call is timed with device events around the whole
product call; the median of the timed calls is reported with the spread of the medians of three thirds of them; the peak device memory over the resident input (the
spectrogram) is torch's allocator's.  Per class also the bytes the fused route moves per sample of the result (8 per bin read, 4 per sample written) and the share
of the measured copy bandwidth (a device copy of the spectrogram) its time stands for.  Verdict per class: "faster" where composed - fused exceeds the two spreads,
else "not faster".  XRFTHIP_MEAN_ALL=1 is set: every class the kernel takes is measured, whatever the default routing keeps.
Writes the table behind the marker line of profiles/r26_istft.txt (what stands in front of it is kept).

    python scripts/bench_istft.py [--calls 12] [--out FILE] [--small]
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

MARK = "== timings (scripts/bench_istft.py)"
KW = dict(window="hann", real_dim="time")
# (shape of the series, dims, nperseg, noverlap): the classes of profiles/r21_spectrogram.txt turned round -- float32 series, their one-sided complex64 stft under a
# Hann window the resident input.  Trailing axis: L = 256 at 50 % and 75 % overlap, L = 1024 and 4096 at 50 %, L = 256 / 1024 without overlap; the leading axis of a
# cube (arranged first: one transposed copy of the spectrogram)
CASES = [((65536, 16384), ("x", "time"), 256, 128), ((65536, 16384), ("x", "time"), 256, 192), ((4096, 262144), ("x", "time"), 1024, 512),
         ((256, 4194304), ("x", "time"), 4096, 2048), ((65536, 16384), ("x", "time"), 256, 0), ((4096, 262144), ("x", "time"), 1024, 0),
         ((4096, 256, 256), ("time", "y", "x"), 256, 128)]
SMALL = [((8, 4096), ("x", "time"), 256, 128), ((8, 4096), ("x", "time"), 256, 192), ((4, 8192), ("x", "time"), 1024, 0), ((1024, 8, 8), ("time", "y", "x"), 256, 128)]


def one_call(st, noverlap, fused):
    os.environ["XRFTHIP_FASTW_SYNTH"] = "1" if fused else "0"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = xa.istft(st, "time", noverlap=noverlap, **KW)
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    tag = fused and any(getattr(p, "seg_synth", 0) for p in api._plan_cache.values())
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
    lines = [MARK, f"device: {torch.cuda.get_device_name(0)}; complex64 one-sided stft (Hann) of float32 series, resident; median of {calls} calls per route, the two routes "
             "alternating, after 2 warm-up calls of each; +- = the spread of the medians of three thirds of the calls; peak = torch.cuda.max_memory_allocated over the "
             "resident spectrogram; B/sample = bytes the fused route moves per sample of the result (8 per bin read + 4 per sample written); copy share = (fused bytes / "
             "fused time) / (16 bytes per bin / time of a device copy of the spectrogram)",
             f"{'class':58s} {'fused ms':>9s} {'+-':>6s} {'composed ms':>12s} {'+-':>6s} {'ratio':>7s} {'B/sample':>9s} {'copy GB/s':>10s} {'copy share':>11s} {'result MB':>10s} "
             f"{'fused peak MB':>14s} {'composed peak MB':>17s}  route, verdict"]
    for shape, dims, nperseg, noverlap in (SMALL if args.small else CASES):
        g = torch.Generator(device="cuda").manual_seed(3)
        coords = {d: np.arange(k) * 1.0 for d, k in zip(dims, shape)}
        da = xa.DataArray(torch.randn(shape, generator=g, device="cuda", dtype=torch.float32), dims, coords)
        st = xa.stft(da, "time", nperseg, noverlap, **KW)
        del da
        api.clear_plan_cache()
        torch.cuda.empty_cache()
        cms = copy_ms(st.data, calls)
        for _ in range(2):
            for fused in (True, False):
                one_call(st, noverlap, fused)
        t = {True: [], False: []}
        peak = {True: 0, False: 0}
        on, nres = False, 0
        for _ in range(calls):
            for fused in (True, False):
                ms, pk, tag, res = one_call(st, noverlap, fused)
                nres = res.data.numel() * res.data.element_size()
                del res
                t[fused].append(ms)
                peak[fused] = max(peak[fused], pk)
                on = on or tag
        mf, mc, sf, sc = statistics.median(t[True]), statistics.median(t[False]), spread(t[True]), spread(t[False])
        nin = st.data.numel() * st.data.element_size()
        moved = float(nin + nres)
        copy_bw = 2.0 * nin / (cms * 1e-3)
        share = (moved / (mf * 1e-3)) / copy_bw
        name = f"istft {shape} along {dims.index('time')} L={nperseg} hop={nperseg - noverlap}"
        verdict = "faster" if mc - mf > sf + sc else "not faster"
        lines.append(f"{name:58s} {mf:9.3f} {sf:6.3f} {mc:12.3f} {sc:6.3f} {mf / mc:7.3f} {moved / (nres / 4):9.3f} {copy_bw / 1e9:10.1f} {share:11.3f} {nres / 2**20:10.1f} "
                     f"{peak[True] / 2**20:14.1f} {peak[False] / 2**20:17.1f}  {'fastw plan, overlap-add' if on else 'composed (the plan declined)'}, {verdict}")
        print(lines[-1], flush=True)
        del st
        api.clear_plan_cache()
        torch.cuda.empty_cache()
    os.environ.pop("XRFTHIP_FASTW_SYNTH", None)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r26_istft.txt")
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
