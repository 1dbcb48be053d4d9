"""Datagram sequence check beside the two existing calls it is to be compared with, on one buffer.

256 channels x 2185 datagrams per call (the shape of tools/bench_display_packets.py), 24 bit (1444 bytes) and then 16 bit
(1028 bytes).  Device time per call with HIP events on one stream, medians of --calls, for three calls on the SAME buffer:
  seqcheck         csdr_seqcheck_batch_put: one header word per datagram
  spurcal          csdr_ingest_spurcal_packets: the cheapest existing kernel that touches every datagram
  process_packets  csdr_demod_batch_process_packets without the blanker (FM / AM receivers at a 500 kHz input rate: their
                   decimation, 8 and 16, divides the call's samples at both packet lengths)
The headers carry a clean sequence with a lost datagram every ~100; the payload is random bytes.  Every seqcheck result
is compared with the sequential host walk (csdr__host_seq_walk) of the same buffer after the timed calls.
Prints one JSON line.  Usage: python tools/bench_seqcheck.py [--channels 256] [--npackets 2185] [--calls 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def headers(channels, npackets, seed):
    """int64 [channels, npackets]: consecutive numbers (65535 -> 1) from a start of the channel's own, ~1 % lost"""
    rng = np.random.default_rng(seed)
    lost = (rng.random((channels, npackets)) < 0.01).astype(np.int64) * rng.integers(1, 4, (channels, npackets))
    pos = rng.integers(1, 65536, (channels, 1)) - 1 + np.cumsum(1 + lost, axis=1) - 1       # positions in the cycle 1..65535
    return pos % 65535 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--npackets", type=int, default=2185)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__host_seq_walk.restype = None
    L.csdr__host_seq_walk.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.csdr__seqcheck_waves.restype = C.c_int
    Cn, npk = a.channels, a.npackets
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    out = {"tool": "bench_seqcheck", "channels": Cn, "npackets": npk, "calls": a.calls, "waves_per_receiver": L.csdr__seqcheck_waves()}
    base = dict(HiCut=5000, HiCutmin=5000, HiCutmax=15000, LowCut=-5000, LowCutmin=-15000, LowCutmax=-5000,
                FilterClickResolution=100, Offset=0, SquelchValue=0, AgcSlope=0, AgcThresh=-100, AgcManualGain=30,
                AgcDecay=200, AgcOn=1, AgcHangOn=0, Symetric=1)
    am = dict(base, HiCutmin=500, HiCutmax=10000, LowCutmax=-500, LowCutmin=-10000)
    for pkt, per, bits in ((1444, 240, 24), (1028, 256, 16)):
        n = npk * per
        g = torch.Generator(device=dev); g.manual_seed(bits)
        packets = torch.randint(0, 256, (Cn, npk, pkt), dtype=torch.uint8, device=dev, generator=g)
        seqs = headers(Cn, npk, bits)
        packets[:, :, 2] = torch.from_numpy((seqs & 0xff).astype(np.uint8)).to(dev)
        packets[:, :, 3] = torch.from_numpy((seqs >> 8).astype(np.uint8)).to(dev)
        dc = torch.zeros((Cn, 2), dtype=torch.float64, device=dev)
        sq = ca.SeqCheckBatch(Cn)
        b = ca.DemodBatch(Cn, 2048); b.set_input_rate(500e3)
        for c in range(Cn):
            b.set_demod(c, 0 if c % 2 else 2, ca.DemodInfo(**(am if c % 2 else base)))
        b.commit()
        cap = n // 8 + 8192
        aud = torch.empty((Cn, cap), dtype=torch.float32, device=dev)
        pp = C.c_void_p(packets.data_ptr())

        def seqcheck():
            sq.put(packets.data_ptr(), npk, pkt, stream.cuda_stream)

        def spurcal():
            assert L.csdr_ingest_spurcal_packets(0, pp, Cn, npk, pkt, C.c_void_p(dc.data_ptr()), sp) == 0, ca._capi.last_error()

        def chain():
            assert L.csdr_demod_batch_process_packets(b.h, pp, npk, pkt, None, C.c_void_p(aud.data_ptr()), cap, sp) == 0, \
                ca._capi.last_error()

        out["input_MB_%dbit" % bits] = round(Cn * npk * pkt / 1e6, 1)
        puts = 0
        for name, fn in (("seqcheck", seqcheck), ("spurcal", spurcal), ("process_packets", chain)):
            ms = []
            for i in range(a.warmup + a.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
            puts += (a.warmup + a.calls) * (name == "seqcheck")
            out["%s_%dbit_ms" % (name, bits)] = round(float(np.median(ms)), 4)
            out["%s_%dbit_min_ms" % (name, bits)] = round(float(np.min(ms)), 4)
        b.flush(stream.cuda_stream)
        torch.cuda.synchronize()
        # the same buffer `puts` times over through the sequential host walk
        raw = packets.cpu().numpy()
        missed, events, first_gap = sq.get_all()
        for c in range(Cn):
            l, m, e, gp = C.c_int(0), C.c_longlong(0), C.c_longlong(0), C.c_int(-1)
            for _ in range(puts):
                L.csdr__host_seq_walk(raw[c].ctypes.data, npk, pkt, *[C.cast(C.byref(x), C.c_void_p) for x in (l, m, e, gp)])
            assert (missed[c], events[c], first_gap[c]) == (m.value, e.value, gp.value), (c, missed[c], m.value)
            assert sq.get(c) == (m.value, e.value, gp.value, l.value), c
        out["seqcheck_%dbit_events_per_put" % bits] = round(float(events.sum()) / puts, 1)
        del sq, b
    print(json.dumps(out))


if __name__ == "__main__":
    main()
