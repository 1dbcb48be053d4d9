"""The row form of the spectrum batch on the display workload of the README: 256 rows x 2185 24-bit datagrams (524400
samples) per call, 4096 points, 2 MS/s.  One process, one stream; every version is warmed up, then the versions take
turns, `--calls` timed calls a turn, `--reps` turns each.  Device time per call from HIP events around the put call; host
time per put from the clock around the same call (it waits for nothing); the acknowledges come behind both.  With one
frame a call the stream is empty when the put arrives, so the event time contains the host's time to issue it.  Per version: the median over all timed calls, and
the spread as the smallest and largest per-turn median.
  a  uniform form: SetMaxDisplayRate(10) = skip 48, gated, acknowledged after every call (one frame a call)
  b  row form (entered through a _row setter) with those settings on every row, acknowledged row by row
  c  row form, mixed rows: display rates 488 / 244 / 81 / 40 / 10 = skips 1 / 2 / 6 / 12 / 48 and averages 1 / 2 / 3 / 4 / 8
     by settings class, every row gated, each acknowledged with probability 1/2 after a call (--seed)
  d  what c costs without the row form: one uniform object per settings class over its own block of rows (the rows are
     laid out class by class, so a block is a slice of the same datagrams), each acknowledged with probability 1/2
  --parent-lib PATH: a library built from the parent commit; version a then also runs through it twice (a_parent,
     a_parent_again: two objects of that library -- their difference is what repeating the parent alone shows)
Prints one JSON line.
Usage: python tools/bench_display_rows.py [--channels 256] [--calls 20] [--reps 5] [--warmup 5] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
FS, N, PKT, PER = 2.0e6, 4096, 1444, 240
CLASSES = [(488, 1), (244, 2), (81, 3), (40, 4), (10, 8)]        # (display rate, average): skips 1, 2, 6, 12, 48


def declare(L):
    """argtypes of the few calls used here, for a library opened by path"""
    vp, i, d, ll = C.c_void_p, C.c_int, C.c_double, C.c_longlong
    L.csdr_fft_batch_create.restype = vp
    L.csdr_fft_batch_create.argtypes = [i, i]
    L.csdr_fft_batch_destroy.restype = None
    L.csdr_fft_batch_destroy.argtypes = [vp]
    L.csdr_fft_batch_set_params.argtypes = [vp, i, i, d, d]
    L.csdr_fft_batch_set_ave.argtypes = [vp, i]
    L.csdr_fft_batch_set_display_rate.argtypes = [vp, d, i, i]
    L.csdr_fft_batch_screen_update_done.argtypes = [vp]
    L.csdr_fft_batch_put_display_packets.argtypes = [vp, vp, i, i, vp, vp]
    return L


class Obj:
    """a csdr_fft_batch through raw calls (so that two libraries can stand side by side)"""

    def __init__(self, L, channels, ave, rate, gated):
        self.L, self.channels = L, channels
        self.h = L.csdr_fft_batch_create(0, channels)
        assert self.h, "csdr_fft_batch_create failed"
        assert L.csdr_fft_batch_set_params(self.h, N, 0, 0.0, FS) == 0
        assert L.csdr_fft_batch_set_ave(self.h, ave) == 0
        assert L.csdr_fft_batch_set_display_rate(self.h, FS, rate, int(gated)) == 0

    def put(self, ptr, npk, dc, sp):
        k = self.L.csdr_fft_batch_put_display_packets(self.h, C.c_void_p(ptr), npk, PKT, C.c_void_p(dc), sp)
        assert k >= 0, k
        return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--npackets", type=int, default=2185)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    import cutesdr_amd as ca
    L = ca.lib()
    Cn, npk = a.channels, a.npackets
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    v = (torch.randn((Cn, npk, 480), device=dev, generator=g) * 1000.0 * 256.0).round().clamp(-(1 << 23), (1 << 23) - 1).to(torch.int32)
    packets = torch.zeros((Cn, npk, PKT), dtype=torch.uint8, device=dev)
    packets[:, :, 4:] = torch.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], dim=-1).to(torch.uint8).reshape(Cn, npk, 1440)
    del v
    dc = torch.tensor([[3.5, -1.25]] * Cn, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    rng = np.random.default_rng(a.seed)
    cls = np.sort(rng.integers(0, len(CLASSES), size=Cn))        # the rows class by class
    bounds = [(int(np.searchsorted(cls, k, "left")), int(np.searchsorted(cls, k, "right"))) for k in range(len(CLASSES))]
    row_bytes, dc_bytes = npk * PKT, 16
    versions = {}

    ua = Obj(L, Cn, 1, 10, True)

    def put_a(o=ua):
        return o.put(packets.data_ptr(), npk, dc.data_ptr(), sp)

    def ack_a(o=ua):
        o.L.csdr_fft_batch_screen_update_done(o.h)
    versions["a"] = (put_a, ack_a)

    fb = ca.FftBatch(Cn)
    fb.set_params(N, False, 0.0, FS); fb.set_display_rate(FS, 10, True)
    fb.set_ave_row(0, 2)
    fb.set_ave_row(-1, 1); fb.set_display_rate_row(-1, 10, True)
    assert fb.row_form()

    def put_b():
        return fb.put_display_packets_ptr(packets.data_ptr(), npk, PKT, dc.data_ptr(), stream.cuda_stream)

    def ack_b():
        for r in range(Cn):
            L.csdr_fft_batch_screen_update_done_row(fb.h, r)
    versions["b"] = (put_b, ack_b)

    fc = ca.FftBatch(Cn)
    fc.set_params(N, False, 0.0, FS); fc.set_display_rate(FS, 10, True)
    for r in range(Cn):
        rate, ave = CLASSES[cls[r]]
        fc.set_ave_row(r, ave); fc.set_display_rate_row(r, rate, True)
    emitted = {"c": [], "d": []}

    def put_c():
        return fc.put_display_packets_ptr(packets.data_ptr(), npk, PKT, dc.data_ptr(), stream.cuda_stream)

    def ack_c():
        emitted["c"].append(int(fc.emits().sum()))
        for r in np.nonzero(rng.random(Cn) < 0.5)[0]:
            L.csdr_fft_batch_screen_update_done_row(fc.h, int(r))
    versions["c"] = (put_c, ack_c)

    ud = [(Obj(L, hi - lo, CLASSES[k][1], CLASSES[k][0], True), lo) for k, (lo, hi) in enumerate(bounds) if hi > lo]

    last_d = []

    def put_d():
        last_d[:] = [o.put(packets.data_ptr() + lo * row_bytes, npk, dc.data_ptr() + lo * dc_bytes, sp) for o, lo in ud]
        return max(last_d)

    def ack_d():
        emitted["d"].append(sum(k * o.channels for k, (o, lo) in zip(last_d, ud)))
        for o, lo in ud:
            if rng.random() < 0.5:
                L.csdr_fft_batch_screen_update_done(o.h)
    versions["d"] = (put_d, ack_d)

    if a.parent_lib:
        P = declare(C.CDLL(os.path.abspath(a.parent_lib)))
        for name in ("a_parent", "a_parent_again"):
            versions[name] = (lambda o: (lambda: put_a(o), lambda: ack_a(o)))(Obj(P, Cn, 1, 10, True))

    for fn, ack in versions.values():
        for _ in range(a.warmup):
            fn(); ack()
    torch.cuda.synchronize()
    dev_ms = {k: [] for k in versions}
    host_us = {k: [] for k in versions}
    frames = {k: [] for k in versions}
    for rep in range(a.reps):
        for name, (fn, ack) in versions.items():
            ms, us = [], []
            for _ in range(a.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                k = fn()
                t1 = time.perf_counter()
                e1.record(stream)
                ack()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1)); us.append((t1 - t0) * 1e6); frames[name].append(k)
            dev_ms[name].append(ms); host_us[name].append(us)
    torch.cuda.synchronize()
    out = {"tool": "bench_display_rows", "channels": Cn, "samples_per_call": npk * PER, "size": N, "pkt_len": PKT,
           "calls": a.calls, "reps": a.reps, "rows_per_class": [hi - lo for lo, hi in bounds]}
    for name in versions:
        per_turn = [float(np.median(m)) for m in dev_ms[name]]
        out[name + "_ms"] = round(float(np.median(np.concatenate(dev_ms[name]))), 4)
        out[name + "_ms_spread"] = [round(min(per_turn), 4), round(max(per_turn), 4)]
        out[name + "_host_us"] = round(float(np.median(np.concatenate(host_us[name]))), 1)
        out[name + "_frames"] = round(float(np.mean(frames[name])), 2)
    for name in ("c", "d"):
        out[name + "_row_frames_per_call"] = round(float(np.mean(emitted[name])), 1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
