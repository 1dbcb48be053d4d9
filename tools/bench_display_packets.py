"""Display spectrum straight from datagrams against the unpack-first and fp32-row forms.

256 channels x 2185 24-bit datagrams (524400 samples, about 2^19) per call, 4096 points, average 1, at display skip
values 1 and 48 (SetMaxDisplayRate: 48 is 2 MS/s, 4096 points, 10 updates/s).  Device time per call with HIP events on
one stream, for three forms:
  unpack_stream   csdr_ingest_unpack(dc) into fp32 rows, then csdr_fft_batch_put_display_stream(dc = NULL)
  packets         csdr_fft_batch_put_display_packets(dc)
  put_display     csdr_fft_batch_put_display on fp32 rows, every whole frame of the call (no skip: the reference point)
Prints one JSON line.  Usage: python tools/bench_display_packets.py [--channels 256] [--calls 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--npackets", type=int, default=2185)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import cutesdr_amd as ca
    from cutesdr_amd._capi import lib
    Cn, npk, N, pkt = a.channels, a.npackets, a.size, 1444
    n = npk * 240
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    packets = torch.randint(0, 256, (Cn, npk, pkt), dtype=torch.uint8, device=dev, generator=g)
    rows = torch.empty((Cn, n, 2), dtype=torch.float32, device=dev)
    dc = torch.tensor([[3.5, -1.25]] * Cn, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    f = ca.FftBatch(Cn)
    f.set_params(N, False, 0.0, 2e6)
    f.set_ave(1)

    def unpack():
        r = lib().csdr_ingest_unpack(0, C.c_void_p(packets.data_ptr()), Cn, npk, pkt, C.c_void_p(rows.data_ptr()), n,
                                     C.c_void_p(dc.data_ptr()), sp)
        assert r == n, r

    forms = {
        "unpack_stream": lambda: (unpack(), f.put_display_stream_ptr(rows.data_ptr(), n, n, None, stream.cuda_stream))[1],
        "packets": lambda: f.put_display_packets_ptr(packets.data_ptr(), npk, pkt, dc.data_ptr(), stream.cuda_stream),
        "put_display": lambda: (f.put_display_ptr(rows.data_ptr(), n, n // N, stream.cuda_stream), n // N)[1],
    }
    unpack()
    out = {"tool": "bench_display_packets", "channels": Cn, "samples_per_call": n, "size": N, "pkt_len": pkt,
           "input_MB_per_call": round(Cn * npk * pkt / 1e6, 1)}
    for skip in (1, 48):
        for name, fn in forms.items():
            if name == "put_display" and skip != 1:
                continue
            f.set_display_rate(N * 10 * skip + 1.0, 10)
            f.stream_reset()
            ms, frames = [], []
            for i in range(a.warmup + a.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                k = fn()
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ms.append(e0.elapsed_time(e1)); frames.append(k)
            key = "%s_skip%d" % (name, skip)
            out[key + "_ms"] = round(float(np.median(ms)), 4)
            out[key + "_frames"] = round(float(np.mean(frames)), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
