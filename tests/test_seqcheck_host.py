"""CPU checks of the datagram sequence check: the restatement in seq_ref.py is pinned to the reference's text by its
anchors before it judges anything; the library's sequential walk (cutesdr_amd/csrc/seq_host.hpp through the
csdr__host_seq_walk hook: the seq_step function the kernel evaluates) equals the restatement on the anchors and on
seeded random header streams of both packet lengths; and a walk cut anywhere, state carried, equals the walk in one
piece.  All comparisons are on integers and exact."""
import ctypes as C

import numpy as np
import pytest

import seq_ref as R

SYMBOLS = ["csdr_seqcheck_batch_" + s for s in ("create", "destroy", "put", "clear", "reset", "get", "get_all")]


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_seq_walk.restype = None
    lib.csdr__host_seq_walk.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    return lib


@pytest.fixture(scope="module", autouse=True)
def pinned():
    R.check_anchors()                                     # the yardstick first


def hook_walk(L, raw, last=0, missed=0, events=0):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    l, m, e, g = C.c_int(last), C.c_longlong(missed), C.c_longlong(events), C.c_int(-7)
    L.csdr__host_seq_walk(raw.ctypes.data, raw.shape[0], raw.shape[1], *[C.cast(C.byref(x), C.c_void_p) for x in (l, m, e, g)])
    return l.value, m.value, e.value, g.value


def random_stream(rng, n):
    """mostly consecutive numbers with losses, duplicates, late datagrams, restarts and jumps anywhere in 0..65535"""
    out, s = [], int(rng.integers(0, 65536))
    for _ in range(n):
        r = rng.random()
        if r < 0.05:
            s = (s + int(rng.integers(1, 5))) & 0xffff          # a loss
        elif r < 0.08:
            s = (s - int(rng.integers(1, 4))) & 0xffff          # a duplicate or a late one
        elif r < 0.10:
            s = 0                                               # the radio restarted
        elif r < 0.13:
            s = int(rng.choice([0x7ffe, 0x7fff, 0x8000, 0xfffe, 0xffff, 1]))
        elif r < 0.15:
            s = int(rng.integers(0, 65536))
        out.append(s)
        s = (s + 1) & 0xffff
        if s == 0:
            s = 1
    return out


def test_symbols_exported_and_bound(L):
    from cutesdr_amd import _capi
    names = _capi.declared_symbols()
    for s in SYMBOLS:
        assert s in names, s
        assert getattr(L, s).argtypes is not None, s
    import cutesdr_amd
    for slot in ("put", "clear", "reset", "get", "get_all", "get_all_ptr"):
        assert hasattr(cutesdr_amd.SeqCheckBatch, slot), slot


@pytest.mark.parametrize("pkt_len", [1028, 1444])
def test_walk_equals_the_restatement_on_the_anchors(L, pkt_len):
    rng = np.random.default_rng(pkt_len)
    for start, seqs, _ in R.ANCHORS:
        assert hook_walk(L, R.datagrams(seqs, pkt_len, rng), last=start) == R.walk(seqs, last=start), (start, seqs)


@pytest.mark.parametrize("pkt_len", [1028, 1444])
@pytest.mark.parametrize("seed", range(6))
def test_walk_equals_the_restatement_on_random_streams(L, pkt_len, seed):
    rng = np.random.default_rng(100 * seed + pkt_len)
    seqs = random_stream(rng, 400)
    start, m0, e0 = int(rng.integers(0, 65536)), int(rng.integers(-10**12, 10**12)), int(rng.integers(0, 10**12))
    want = R.walk(seqs, start, m0, e0)
    assert want[2] - e0 > 20                              # the stream is not a clean one
    assert hook_walk(L, R.datagrams(seqs, pkt_len, rng), start, m0, e0) == want


def test_walk_of_no_datagrams_keeps_the_state(L):
    assert hook_walk(L, np.zeros((0, 1028), dtype=np.uint8), 77, -5, 9) == (77, -5, 9, -1) == R.walk([], 77, -5, 9)


@pytest.mark.parametrize("pkt_len", [1028, 1444])
def test_walk_cut_anywhere_equals_the_walk_in_one_piece(L, pkt_len):
    rng = np.random.default_rng(7 + pkt_len)
    seqs = random_stream(rng, 40)
    seqs[0] = 3                                           # datagram 0 out of sequence: first_gap 0 in the whole walk
    raw = R.datagrams(seqs, pkt_len, rng)
    whole = hook_walk(L, raw)
    assert whole == R.walk(seqs) and whole[3] == 0
    for cut in range(41):
        a = hook_walk(L, raw[:cut])
        b = hook_walk(L, raw[cut:], *a[:3])
        assert b[:3] == whole[:3], cut
        assert a[3] == R.walk(seqs[:cut])[3] and b[3] == R.walk(seqs[cut:], *a[:3])[3], cut      # first_gap is per walk
