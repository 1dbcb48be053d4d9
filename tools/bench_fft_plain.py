#!/usr/bin/env python3
"""Timing of the batch plain transforms (csdr_fft_batch_fwd, fft_batch_plain_kernels.hip) -- not the bench.py contract.

For every size 512 ... 65536: 256 rows x (2^19 / n) frames of complex fp32 (1 GiB in, 1 GiB out), forward, out of place
and in place.  HIP events around every call after warm-up, medians, the legs alternating in one process:
  "fwd"      csdr_fft_batch_fwd, d_out another buffer
  "inplace"  csdr_fft_batch_fwd, d_out == d_in
  "display"  csdr_fft_batch_put_display of the same rows at the same size: the same input bytes, n floats out per row
             (at 512, 1024, 32768 and 65536 points the multi-launch transform through HBM)
  "copy"     a device-to-device copy of the same input + output bytes
and the bytes the transform must move (16 per point: 8 in, 8 out) over its time, against the 8 TB/s peak.

  python tools/bench_fft_plain.py [--calls 30] [--rows 256] [--sizes 512,32768]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cutesdr_amd as ca

FS, PEAK = 2.0e6, 8.0e12
SIZES = (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)


def measure(rows, n, per_row, calls, warmup):
    nframes = per_row // n
    stream = torch.cuda.current_stream().cuda_stream
    f = ca.FftBatch(rows)
    f.set_params(n, False, 0.0, FS); f.set_ave(1)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (3000.0 * torch.randn((rows, per_row, 2), generator=g, device="cuda", dtype=torch.float32)).contiguous()
    y = torch.empty_like(x)
    z = x.clone()                                            # the in-place leg's rows (they grow by n a call: re-filled)
    legs = {
        "fwd": lambda: f.fwd_ptr(x.data_ptr(), per_row, y.data_ptr(), per_row, nframes, stream),
        "inplace": lambda: f.fwd_ptr(z.data_ptr(), per_row, z.data_ptr(), per_row, nframes, stream),
        "display": lambda: f.put_display_ptr(x.data_ptr(), per_row, nframes, stream),
        "copy": lambda: y.copy_(x),
    }
    times = {k: [] for k in legs}
    for it in range(warmup + calls):
        for name, call in legs.items():
            if name == "inplace":
                z.copy_(x)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    moved = 16.0 * rows * per_row
    out = {"n": n, "rows": rows, "frames": nframes, "bytes": moved, "group": f.plain_group()}
    for k, v in times.items():
        out[k + "_ms"] = statistics.median(v)
        out[k + "_min_ms"] = min(v)
    for k in ("fwd", "inplace", "copy"):
        out[k + "_tbps"] = moved / (out[k + "_ms"] * 1e-3) / 1e12
        out[k + "_of_peak"] = moved / (out[k + "_ms"] * 1e-3) / PEAK
    out["display_over_fwd"] = out["display_ms"] / out["fwd_ms"]
    out["fwd_over_copy"] = out["fwd_ms"] / out["copy_ms"]
    out["fwd_us_per_frame"] = out["fwd_ms"] * 1e3 / (rows * nframes)
    out["display_us_per_frame"] = out["display_ms"] * 1e3 / (rows * nframes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--per-row", type=int, default=1 << 19)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    a = ap.parse_args()
    res = {}
    for n in (int(s) for s in a.sizes.split(",")):
        res[str(n)] = measure(a.rows, n, a.per_row, a.calls, a.warmup)
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "bench_fft_plain", "calls": a.calls, **res}))


if __name__ == "__main__":
    main()
