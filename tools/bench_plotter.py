#!/usr/bin/env python3
"""Timing of the batch plotter's draw (csdr_plotter_batch_draw, K11) -- not the bench.py contract.

Shapes: 256 views over an FftBatch of 256 rows at 4096 and at 16384 points, average 1, 2 MS/s; 2D height 300, waterfall
height 300.  Two mixes of settings:
  "uniform": every view 1024 wide with the same span and dB range, view v on row v;
  "mixed":   8 distinct (span, dB range, width) groups, widths 300 ... 1920, 4 views per spectrum row on rows 0 ... 63
             of the same 256-row batch: 192 of its rows are watched by nobody.
HIP events around every call after warm-up, in the same process and alternating with two yardsticks on the same spectra:
  "pair": one csdr_fft_batch_get_waterfall_all plus one csdr_fft_batch_get_screen_all per distinct setting -- all the
          library could do on the device without the plotter; each call maps every row of the batch, 256 in both mixes
          (the calls take no row list), and nothing scrolls;
  "d2h":  the device-to-host copy of as many bytes as the averaged bels of the whole batch, 256 rows in both mixes, into
          pinned memory, the least a host that maps on the CPU and does not know which rows are watched must spend.
In the mixed mix both yardsticks therefore work on four times the rows the views read; a host that kept a 64-row batch
would pay a quarter of either.
Also the host time of one draw (settings, parameter slot, launch).

  python tools/bench_plotter.py [--calls 30] [--copies 5] [--views 256]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cutesdr_amd as ca
from cutesdr_amd._capi import lib, check

FS, H2D, WF_H = 2.0e6, 300, 300
UNIFORM = [(1800000, 0, 10, 1024)]                       # (span, MaxdB, dB step, width)
MIXED = [(2000000, 0, 10, 1024), (1000000, -10, 10, 1280), (500000, -20, 8, 800), (250000, 0, 12, 640),
         (1800000, -30, 6, 1920), (120000, -10, 10, 512), (60000, 0, 5, 1024), (900000, -40, 7, 300)]


def spectra(rows, n):
    g = torch.Generator(device="cuda").manual_seed(1)
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    tone = 3276.7 * torch.exp(2j * torch.pi * 0.1317 * i)
    x = tone.repeat(rows, 1) + 32.767 * torch.complex(torch.randn((rows, n), generator=g, device="cuda", dtype=torch.float64),
                                                      torch.randn((rows, n), generator=g, device="cuda", dtype=torch.float64))
    return x.to(torch.complex64).contiguous()


def measure(views, n, mix, calls, copies, warmup):
    groups = UNIFORM if mix == "uniform" else MIXED
    stream = torch.cuda.current_stream().cuda_stream
    f = ca.FftBatch(views)
    f.set_params(n, False, 0.0, FS); f.set_ave(1)
    x = spectra(views, n)
    f.put_display_ptr(x.data_ptr(), x.stride(0), 1, stream)
    p = ca.PlotterBatch(views)
    for v in range(views):
        span, max_db, step, w = groups[v % len(groups)]
        p.set_source(v if mix == "uniform" else v // 4, v)
        p.SetSpanFreq(span, v); p.SetMaxdB(max_db, v); p.SetdBStepSize(step, v)
        p.resizeEvent(w, H2D + WF_H, v)
    p.SetRunningState(True)
    wmax = max(g[3] for g in groups)
    scr = torch.zeros((views, wmax), dtype=torch.int32, device="cuda")
    rgb = torch.zeros((views, wmax), dtype=torch.int32, device="cuda")
    ov = torch.zeros(views, dtype=torch.int32, device="cuda")
    bels = torch.zeros((views, n), dtype=torch.float32, device="cuda")
    host = torch.empty(bels.shape, dtype=bels.dtype, pin_memory=True)

    def pair():
        for span, max_db, step, w in groups:
            lo, hi, min_db = -(span // 2), span // 2, float(max_db - 14 * step)
            check(lib().csdr_fft_batch_get_waterfall_all(f.h, w, float(max_db), min_db, lo, hi, C.c_void_p(rgb.data_ptr()), wmax,
                                                         C.c_void_p(ov.data_ptr()), C.c_void_p(stream)), "csdr_fft_batch_get_waterfall_all")
            check(lib().csdr_fft_batch_get_screen_all(f.h, H2D, w, float(max_db), min_db, lo, hi, C.c_void_p(scr.data_ptr()), wmax,
                                                      C.c_void_p(ov.data_ptr()), C.c_void_p(stream)), "csdr_fft_batch_get_screen_all")

    times, hostt = {"draw": [], "pair": [], "d2h": []}, []
    for it in range(warmup + calls):
        for name in ("d2h", "draw", "pair"):
            if name == "d2h" and it >= warmup + copies:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == "d2h":
                host.copy_(bels, non_blocking=True)
            elif name == "draw":
                t0 = time.perf_counter()
                drawn = p.draw(f, stream)
                dt = time.perf_counter() - t0
                assert drawn == views
            else:
                pair()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b) * 1e-3)
                if name == "draw":
                    hostt.append(dt)
    out = {"views": views, "n": n, "batch_rows": views, "watched_rows": views if mix == "uniform" else views // 4,
           "settings": len(groups), "widths": sorted({g[3] for g in groups}), "bel_bytes": bels.numel() * 4}
    for k, v in times.items():
        out[k + "_ms"] = statistics.median(v) * 1e3
        out[k + "_min_ms"] = min(v) * 1e3
    out["draw_host_us"] = statistics.median(hostt) * 1e6
    out["pair_over_draw"] = out["pair_ms"] / out["draw_ms"]
    out["d2h_over_draw"] = out["d2h_ms"] / out["draw_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--copies", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=256)
    a = ap.parse_args()
    res = {"%s_%d" % (mix, n): measure(a.views, n, mix, a.calls, a.copies, a.warmup)
           for n in (4096, 16384) for mix in ("uniform", "mixed")}
    print(json.dumps({"tool": "bench_plotter", "calls": a.calls, **res}))


if __name__ == "__main__":
    main()
