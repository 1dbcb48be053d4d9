"""The datagram sequence bookkeeping of CUdpThread::OnreadyRead (reference interface/netiobase.cpp:484-496 for 24 bit,
:509-521 for 16 bit: the same text) restated as a plain sequential loop -- the yardstick of the sequence-check tests.
netiobase.cpp is Qt sockets and cannot be compiled for the tests, so the restatement is pinned by ANCHORS, worked out by
hand from the reference's text; tests/test_seqcheck_host.py asserts them on walk() before anything is compared to it.

    m_LastSeqNum is a quint16 that starts at 0 (:433), m_MissedPackets an int (held here unbounded), and per datagram
        seq = Buf[2] | Buf[3] << 8
        if (0 == seq) m_LastSeqNum = 0;
        if (seq != m_LastSeqNum) { m_MissedPackets += ((qint16)seq - (qint16)m_LastSeqNum); m_LastSeqNum = seq; }
        m_LastSeqNum++; if (0 == m_LastSeqNum) m_LastSeqNum = 1;
"""
import numpy as np


def _qint16(v):
    return v - 65536 if v >= 32768 else v


def walk(seqs, last=0, missed=0, events=0):
    """the sequence numbers of one receiver's datagrams in order -> (last, missed, events, first_gap); first_gap is the
    index of the first datagram of THIS walk whose number was not the expected one, or -1"""
    first_gap = -1
    for p, seq in enumerate(seqs):
        seq = int(seq)
        if seq == 0:
            last = 0
        if seq != last:
            missed += _qint16(seq) - _qint16(last)
            events += 1
            if first_gap < 0:
                first_gap = p
            last = seq
        last = (last + 1) & 0xffff
        if last == 0:
            last = 1
    return last, missed, events, first_gap


# (start last, sequence, {what the reference's text gives})
ANCHORS = [
    (0, [0, 1, 2, 4], dict(missed=1, events=1, first_gap=3, last=5)),
    (0, [100], dict(missed=100)),
    (32766, [32766, 32768], dict(missed=-65535)),
    (32766, [32766, 32767, 32768], dict(missed=0)),
    (65535, [65535, 1], dict(missed=0, last=2)),
    (65535, [65535, 0], dict(missed=0, last=1)),
    (7, [7, 0, 1], dict(missed=0)),
    (5, [5, 5], dict(missed=-1, events=1)),
    # a swap: 12 where 11 is expected (:491: 12 - 11 = +1, expected next 13), 11 where 13 is (-2, next 12), 13 where 12
    # is (+1) -- the signed sum reads as a clean stream, the three events do not.  (The issue that asked for these
    # anchors wrote this sum as 2 - 2 + 1 = 1; its first term is 12 - 11 by the reference's text, and by the issue's own
    # statement of the rule.)
    (10, [10, 12, 11, 13], dict(missed=1 - 2 + 1, events=3, first_gap=1, last=14)),
]


def check_anchors():
    for start, seqs, want in ANCHORS:
        got = dict(zip(("last", "missed", "events", "first_gap"), walk(seqs, last=start)))
        for k, v in want.items():
            assert got[k] == v, (start, seqs, k, got[k], v)


def datagrams(seqs, pkt_len, rng):
    """uint8 [len(seqs), pkt_len]: random bytes everywhere (a wrong byte offset reads noise), the numbers in bytes 2-3"""
    seqs = np.asarray(seqs, dtype=np.int64)
    raw = rng.integers(0, 256, (len(seqs), pkt_len), dtype=np.uint8)
    raw[:, 2] = seqs & 0xff
    raw[:, 3] = (seqs >> 8) & 0xff
    return raw


def clean(start, n):
    """n consecutive numbers as a radio sends them from `start`: 65535 is followed by 1"""
    out, s = [], start
    for _ in range(n):
        out.append(s)
        s = (s + 1) & 0xffff
        if s == 0:
            s = 1
    return out
