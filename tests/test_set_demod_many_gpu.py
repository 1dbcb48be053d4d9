"""Batch SetDemod: filters of many receivers designed on the device in one launch (csdr_fastfir_batch_setup_many,
csdr_demod_batch_set_demod_many, csdr_demod_shard_set_demod_many).

Bounds.  The design in fp64 against the oracle's CFastFIR coefficients: 1e-12 absolute (what tests/test_fastfir_gpu.py
holds the host design to) and 1e-9 * max|H| (an fp32 word's half ulp is 6e-8 of its value: a design error sixty times
smaller on the largest coefficient cannot be told from the host design after rounding except in the odd last bit).
Through the filter: the project's K1 bound, 2e-5 * max|x| per sample.  Through the chain: the helpers and bounds of
tests/test_batch_control_combinations_gpu.py (a same-mode SetDemod is a "control" event there), none of its own."""
import ctypes as C
import numpy as np
import pytest
from util_signals import tones_plus_noise
from test_postchain_gpu import MODES, info
from test_batch_control_combinations_gpu import Rig, _signal, _info_kw, _form, FS, LIM, N64

pytestmark = pytest.mark.gpu
TOL = 2e-5
EINVAL = -1
# CWL is not in the shared table: CWU mirrored (gui/mainwindow.cpp:1006-1050)
MODES.setdefault("CWL", (6, dict(HiCut=500, LowCut=-500, HiCutmin=50, HiCutmax=1000, LowCutmax=-50, LowCutmin=-1000,
                                 Offset=-700, Symetric=0)))


def _edge_sets(fs, count=18):
    """(flo, fhi, offset) per slot, all distinct: CW offsets of +-700 Hz, a USB / LSB pair, 100 Hz wide, edges within
    1 % of +-fs/2, then staggered pass bands"""
    h = fs / 2.0
    sets = [(-250.0, 250.0, 700.0), (-250.0, 250.0, -700.0), (100.0, 2800.0, 0.0), (-2800.0, -100.0, 0.0),
            (-50.0, 50.0, 0.0), (1000.0, 1100.0, 0.0), (-0.995 * h, 0.995 * h, 0.0), (0.5 * h, 0.992 * h, 0.0),
            (-0.998 * h, -0.7 * h, 0.0), (-5000.0, 5000.0, 0.0)]
    k = 0
    while len(sets) < count:
        sets.append((-4000.0 + 130.0 * k, 3000.0 + 170.0 * k, 0.0)); k += 1
    return sets


@pytest.mark.parametrize("n", [2048, 4096, 8192, 16384])
def test_device_design_matches_the_oracle_in_fp64(oracle, n):
    import cutesdr_amd as ca
    fs = 62500.0
    sets = _edge_sets(fs)
    Cn = len(sets)
    b = ca.FastFirBatch(Cn, n)
    b.setup(-5000, 5000, 0, fs)
    st = b.setup_many(np.arange(Cn), [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets], fs)
    assert (st == 1).all(), st
    worst_abs = worst_rel = 0.0
    for c, (lo, hi, off) in enumerate(sets):
        ff = oracle.CFastFIR(n)
        assert ff.SetupParameters(lo, hi, off, fs) == 1
        want, got = ff.coef(), b.response(c)
        err = np.abs(got - want).max()
        worst_abs, worst_rel = max(worst_abs, err), max(worst_rel, err / np.abs(want).max())
    print("device design, N = %d: max abs err %.3g, max err / max|H| %.3g" % (n, worst_abs, worst_rel))
    assert worst_abs <= 1e-12, worst_abs
    assert worst_rel <= 1e-9, worst_rel


def test_rejected_entries_keep_their_slot_while_the_others_apply(oracle):
    import cutesdr_amd as ca
    n, Cn, fs = 2048, 6, 62500.0
    x = np.stack([tones_plus_noise(40 + c, 5 * (n // 2), fs, [700.0 * (c % 5 + 1), -4100.0, 15000.0]) for c in range(Cn)])
    b = ca.FastFirBatch(Cn, n)
    for c in range(Cn):
        b.setup(200 + 10 * c, 3000 + 10 * c, 0, fs, channel=c)
    before = [b.response(c) for c in range(Cn)]
    #          ok            flo >= fhi   ok             edge at fs/2     beyond -fs/2 after the offset   ok
    lo = [-1000.0, 3000.0, 100.0, 100.0, -31000.0, -2000.0]
    hi = [1000.0, 3000.0, 2000.0, 31250.0, -30000.0, -100.0]
    off = [0.0, 0.0, 0.0, 0.0, -700.0, 0.0]
    st = b.setup_many(np.arange(Cn), lo, hi, off, fs)
    assert list(st) == [1, EINVAL, 1, EINVAL, EINVAL, 1]
    y = b.process(x)
    for c in range(Cn):
        ff = oracle.CFastFIR(n)
        cut = (lo[c], hi[c], off[c], fs) if st[c] == 1 else (200 + 10 * c, 3000 + 10 * c, 0, fs)
        assert ff.SetupParameters(*cut) == 1
        if st[c] != 1:
            assert np.array_equal(b.response(c), before[c]), c
        assert np.abs(y[c] - ff.ProcessData(x[c])).max() <= TOL * np.abs(x[c]).max(), c


@pytest.mark.parametrize("n,hops", [(2048, 5), (16384, 5)])
def test_filters_from_one_setup_many_through_the_kernel(oracle, n, hops):
    import cutesdr_amd as ca
    Cn, fs = 24, 62500.0
    T = hops * (n // 2)
    x = np.stack([tones_plus_noise(40 + c, T, fs, [700.0 * (c % 5 + 1), -4100.0, 15000.0]) for c in range(Cn)])
    sets = _edge_sets(fs, Cn)
    outs = []
    for _ in range(2):                                      # the same job list on two fresh objects: the same words
        b = ca.FastFirBatch(Cn, n)
        st = b.setup_many(np.arange(Cn), [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets], fs)
        assert (st == 1).all()
        outs.append(b.process(x))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    for c, (lo, hi, off) in enumerate(sets):
        ff = oracle.CFastFIR(n)
        ff.SetupParameters(lo, hi, off, fs)
        assert np.abs(outs[0][c] - ff.ProcessData(x[c])).max() <= TOL * np.abs(x[c]).max(), c


@pytest.mark.parametrize("n", [2048, 16384])
def test_the_later_call_wins(oracle, n):
    """setup then setup_many on a slot, setup_many then setup, and a slot named twice in one call: one process call
    later the filter is the later call's; untouched slots keep theirs"""
    import cutesdr_amd as ca
    Cn, fs = 4, 62500.0
    x = np.stack([tones_plus_noise(c, 3 * (n // 2), fs, [500.0 * (c + 1), -1500.0, -12000.0]) for c in range(Cn)])
    A, B, D = (100.0, 2800.0, 0.0), (-2800.0, -100.0, 0.0), (-250.0, 250.0, 700.0)
    b = ca.FastFirBatch(Cn, n)
    b.setup(-5000, 5000, 0, fs)
    for c in range(Cn):
        b.setup(-4000, 4000, 0, fs, channel=c)
    b.process(x)                                            # (the per-channel object has run once)
    b.reset()
    b.setup(*A, fs, channel=0)
    assert list(b.setup_many([0], [B[0]], [B[1]], [B[2]], fs)) == [1]            # slot 0: host design, then device
    assert list(b.setup_many([1], [A[0]], [A[1]], [A[2]], fs)) == [1]
    b.setup(*B, fs, channel=1)                                                  # slot 1: device, then host
    assert list(b.setup_many([2, 2], [A[0], D[0]], [A[1], D[1]], [A[2], D[2]], fs)) == [1, 1]   # slot 2: twice in one call
    y = b.process(x)
    want = [B, B, D, (-4000.0, 4000.0, 0.0)]
    for c, cut in enumerate(want):
        ff = oracle.CFastFIR(n)
        ff.SetupParameters(cut[0], cut[1], cut[2], fs)
        np.testing.assert_allclose(b.response(c), ff.coef(), atol=1e-12, err_msg=str(c))
        assert np.abs(y[c] - ff.ProcessData(x[c])).max() <= TOL * np.abs(x[c]).max(), c


def test_shared_filter_entries_and_the_switch_to_per_channel(oracle):
    import cutesdr_amd as ca
    n, Cn, fs = 2048, 3, 62500.0
    x = np.stack([tones_plus_noise(c, 3 * (n // 2), fs, [500.0 * (c + 1), -1500.0]) for c in range(Cn)])
    b = ca.FastFirBatch(Cn, n)
    assert list(b.setup_many([-1], [-3000.0], [3000.0], [0.0], fs)) == [1]
    assert list(b.setup_many([-1], [-3000.0], [3000.0], [0.0], fs)) == [0]       # the reference's early-out
    assert list(b.setup_many([1], [100.0], [2800.0], [0.0], fs)) == [1]          # turns the object per-channel
    y = b.process(x)
    for c in range(Cn):
        ff = oracle.CFastFIR(n)
        ff.SetupParameters(*((100.0, 2800.0, 0.0, fs) if c == 1 else (-3000.0, 3000.0, 0.0, fs)))
        np.testing.assert_allclose(b.response(c), ff.coef(), atol=1e-12)
        assert np.abs(y[c] - ff.ProcessData(x[c])).max() <= TOL * np.abs(x[c]).max(), c


# ---------------------------------------------------------------- through the chain

NAMES6 = ["AM", "USB", "FM", "SAM", "CWL", "USB"]
KIND6 = ["AM", "T", "FM", "AM", "T", "T"]
NEW_EDGES = {"AM": dict(HiCut=4000, LowCut=-4000), "SAM": dict(HiCut=3000, LowCut=-3000), "FM": dict(HiCut=3000, LowCut=-3000),
             "USB": dict(HiCut=2400, LowCut=300), "LSB": dict(HiCut=-300, LowCut=-2400), "CWL": dict(HiCut=300, LowCut=-300)}


def _many(rig, entries, batches=None):
    """entries: (receiver, mode name, overrides) -- one set_demod_many on the rig's batch(es), SetDemod on every oracle"""
    ca, oracle = rig.ca, rig.oracle
    ch, md, inf = [], [], []
    for c, name, over in entries:
        m, kw = _info_kw(name, **over)
        ch.append(c); md.append(m); inf.append(info(ca, **kw))
    sts = [b.set_demod_many(ch, md, inf) for b in (batches or rig.batches)]
    for c, name, over in entries:
        m, kw = _info_kw(name, **over)
        rig.refs[c].SetDemod(m, info(oracle, **kw))
        if name != rig.modes[c]:
            rig.tracks[c].restart(name)
        else:
            rig.tracks[c].control()
        rig.modes[c] = name
        assert rig.b.output_rate(c) == rig.refs[c].GetOutputRate(), (c, name)
    return sts


@pytest.mark.parametrize("form", [0, 1], ids=["strict", "chained"])
def test_new_edges_for_every_receiver_of_a_committed_batch(oracle, form):
    """48 receivers of mixed AM / SAM / FM / USB / CWL in four plan groups on three shared input rows: three calls, one
    set_demod_many that gives every receiver new edges (same modes), three more calls -- every receiver against its own
    oracle CDemodulator given the same SetDemod at the same sample index"""
    import cutesdr_amd as ca
    Cn = 48
    names = [NAMES6[c % 6] for c in range(Cn)]
    kinds = [KIND6[c % 6] for c in range(Cn)]
    rowk = ["AM", "T", "FM"]
    rows = [rowk.index(k) for k in kinds]
    rig = Rig(ca, oracle, names, kinds=kinds, rows=rows, form=form)
    assert rig.b.group_count()[0] >= 2
    g0 = rig.b.group_count()
    n, calls = 16 * LIM, 6
    src = [_signal(k, 0, calls * n, FS) for k in rowk]
    for k in range(calls):
        if k == 3:
            (st,) = _many(rig, [(c, names[c], NEW_EDGES[names[c]]) for c in range(Cn)])
            assert (st == 0).all(), st
            assert rig.b.group_count() == g0
        x = np.stack([s[k * n:(k + 1) * n] for s in src] + [np.zeros(n, dtype=np.complex64)] * (Cn - 3))
        got = rig.b.process(x)
        rig.check(got, rig.oracle_outs([x[rows[c]] for c in range(Cn)]), ("call", k))
    assert _form(rig.b) == {0: 0, 1: 3}[form]


def test_a_call_that_mixes_same_mode_changes_in_place_changes_and_a_mover(oracle):
    """Receiver 4 (USB) gets new edges by set_demod_many -- its filter now exists on the device only -- and one call
    later one set_demod_many holds: new edges for receiver 0, USB -> LSB for 1 and FM -> USB for 2 (both keep their row),
    USB -> AM for 4, which moves to another plan group and takes the response in use with it (the lazy mirror), and new
    edges for 7.  A twin batch gets the same entries from the one-receiver setter, in the same order: equal group layout;
    every receiver's audio against its oracle."""
    import cutesdr_amd as ca
    names = ["USB", "USB", "FM", "AM", "USB", "FM", "AM", "USB"]
    rig = Rig(ca, oracle, names)
    twin = ca.DemodBatch(len(names), 2048)
    twin.set_input_rate(FS)
    for c, name in enumerate(names):
        m, kw = _info_kw(name)
        twin.set_demod(c, m, info(ca, **kw))
    twin.commit()
    for c in range(len(names)):
        twin.set_freq(c, -100e3)
    steps = {2: [(c, names[c], NEW_EDGES[names[c]]) for c in range(len(names))],
             3: [(0, "USB", dict(HiCut=2600, LowCut=200)), (1, "LSB", {}), (2, "USB", {}), (4, "AM", {}),
                 (7, "USB", dict(HiCut=2000, LowCut=150))]}
    for k in range(6):
        for c, name, over in steps.get(k, []):
            m, kw = _info_kw(name, **over)
            twin.set_demod(c, m, info(ca, **kw))
        if k in steps:
            _many(rig, steps[k])
            assert rig.b.group_count() == twin.group_count(), k
            assert [rig.b.output_rate(c) for c in range(rig.C)] == [twin.output_rate(c) for c in range(rig.C)]
        if k == 3:
            assert rig.b.group_count()[0] > 3                    # receiver 4 opened a group
        x = np.stack([_signal(rig.kinds[c], 0, N64, FS) for c in range(rig.C)])
        got = rig.b.process(x)
        rig.check(got, rig.oracle_outs(x), ("call", k))
        tw = twin.process(x)
        assert [len(a) for a in tw] == [len(a) for a in got], k


@pytest.mark.parametrize("form", [1], ids=["chained"])
def test_set_demod_many_reaches_the_next_call_not_the_one_in_flight(form):
    import cutesdr_amd as ca
    Cn = 48
    names = [NAMES6[c % 6] for c in range(Cn)]
    rowk = ["AM", "T", "FM"]
    rows = [rowk.index(KIND6[c % 6]) for c in range(Cn)]
    calls, n = 3, N64
    xin = np.zeros((Cn, calls * n), dtype=np.complex64)
    for r, k in enumerate(rowk):
        xin[r] = _signal(k, 0, calls * n, FS)
    din = ca.DeviceBuffer(xin.nbytes)
    din.upload(xin)
    cap = n // 32 + 2048 + 4096
    outs = {}
    for touched in (False, True):
        b = ca.DemodBatch(Cn, 2048)
        b.set_input_rate(FS)
        b.set_input_rows(np.asarray(rows, dtype=np.int32))
        for c, name in enumerate(names):
            m, kw = _info_kw(name)
            b.set_demod(c, m, info(ca, **kw))
        b.commit()
        for c in range(Cn):
            b.set_freq(c, -100e3)
        b.set_pipelined(form)
        douts = [ca.DeviceBuffer(Cn * cap * 4) for _ in range(calls)]
        counts = []
        for k in range(calls):
            b.process_ptr(din.ptr + 8 * k * n, calls * n, n, douts[k].ptr, cap)
            counts.append([b.out_count(c) for c in range(Cn)])
            if touched and k == 1:                              # call 1 is in flight, nothing flushed
                ch, md, inf = [], [], []
                for c, name in enumerate(names):
                    m, kw = _info_kw(name, AgcThresh=-40, AgcDecay=1000, AgcSlope=10, **NEW_EDGES[name])
                    ch.append(c); md.append(m); inf.append(info(ca, **kw))
                assert (b.set_demod_many(ch, md, inf) == 0).all()
        b.flush()
        ca.sync()
        res = []
        for k in range(calls):
            o = douts[k].download(np.float32, Cn * cap).reshape(Cn, cap)
            res.append([o[c, :counts[k][c]].copy() for c in range(Cn)])
        outs[touched] = res
    for k in (0, 1):
        for c in range(Cn):
            assert np.array_equal(outs[True][k][c].view(np.uint32), outs[False][k][c].view(np.uint32)), (k, c)
    changed = sum(not np.array_equal(outs[True][2][c], outs[False][2][c]) for c in range(Cn))
    assert changed >= Cn // 2, changed                          # the new parameters did reach call 2


def _fresh(ca, names, many):
    b = ca.DemodBatch(len(names), 2048)
    b.set_input_rate(FS)
    ch, md, inf = [], [], []
    for c, name in enumerate(names):
        m, kw = _info_kw(name)
        ch.append(c); md.append(m); inf.append(info(ca, **kw))
    if many:
        assert (b.set_demod_many(ch, md, inf) == 0).all()
    else:
        for c in range(len(names)):
            b.set_demod(ch[c], md[c], inf[c])
    b.commit()
    for c in range(len(names)):
        b.set_freq(c, -100e3)
    return b


def test_before_commit_it_is_the_loop_of_single_calls():
    import cutesdr_amd as ca
    names = ["FM", "AM", "USB", "SAM", "FM", "AM", "USB", "LSB"]
    a, b = _fresh(ca, names, True), _fresh(ca, names, False)
    assert a.group_count() == b.group_count()
    kinds = {"FM": "FM", "AM": "AM", "SAM": "AM", "USB": "T", "LSB": "T"}
    for k in range(2):
        x = np.stack([_signal(kinds[m], 0, 2 * 8 * LIM, FS)[k * 8 * LIM:(k + 1) * 8 * LIM] for m in names])
        ga, gb = a.process(x), b.process(x)
        for c in range(len(names)):
            assert np.array_equal(ga[c].view(np.uint32), gb[c].view(np.uint32)), (k, c)


def test_three_shards_equal_one_batch_given_the_same_call():
    import cutesdr_amd as ca
    names = [NAMES6[c % 6] for c in range(12)]
    kinds = [KIND6[c % 6] for c in range(12)]
    wide = _fresh(ca, names, False)
    sh = ca.ShardedDemodBatch([0, 0, 0], len(names), 2048)
    sh.set_input_rate(FS)
    for c, name in enumerate(names):
        m, kw = _info_kw(name)
        sh.set_demod(c, m, info(ca, **kw))
    sh.commit()
    for c in range(len(names)):
        sh.set_freq(c, -100e3)
    n = 8 * LIM
    order = [7, 0, 11, 3, 4, 8, 1, 2, 5, 6, 9, 10]                  # global ids, not in shard order
    ch, md, inf = [], [], []
    for c in order:
        m, kw = _info_kw(names[c], **NEW_EDGES[names[c]])
        ch.append(c); md.append(m); inf.append(info(ca, **kw))
    for k in range(3):
        if k == 1:
            assert (wide.set_demod_many(ch, md, inf) == 0).all()
            assert (sh.set_demod_many(ch, md, inf) == 0).all()
        x = np.stack([_signal(kd, 0, 3 * n, FS)[k * n:(k + 1) * n] for kd in kinds])
        gw, gs = wide.process(x), sh.process(x)
        for c in range(len(names)):
            assert len(gw[c]) == len(gs[c]) and np.array_equal(gw[c].view(np.uint32), gs[c].view(np.uint32)), (k, c)


def test_bad_arguments_change_nothing():
    import cutesdr_amd as ca
    from cutesdr_amd._capi import lib
    L = lib()
    names = ["FM", "AM", "USB", "USB"]
    a, b = _fresh(ca, names, False), _fresh(ca, names, False)
    one, bad, neg = (C.c_int * 1)(0), (C.c_int * 1)(len(names)), (C.c_int * 1)(-1)
    mode, badmode = (C.c_int * 1)(2), (C.c_int * 1)(7)
    inf = info(ca, HiCut=2000, LowCut=-2000)
    st = (C.c_int * 1)(5)
    f = L.csdr_demod_batch_set_demod_many
    assert f(a.h, 0, None, None, None, None) == 0
    assert f(a.h, -1, one, mode, C.byref(inf), st) == EINVAL
    assert f(a.h, 1, None, mode, C.byref(inf), st) == EINVAL
    assert f(a.h, 1, one, None, C.byref(inf), st) == EINVAL
    assert f(a.h, 1, one, mode, None, st) == EINVAL
    assert f(a.h, 1, bad, mode, C.byref(inf), st) == EINVAL
    assert f(a.h, 1, neg, mode, C.byref(inf), st) == EINVAL
    assert f(a.h, 1, one, badmode, C.byref(inf), st) == EINVAL
    two = (C.c_int * 2)(0, 9)                                    # a good entry in front of a bad one: nothing applied
    modes2 = (C.c_int * 2)(2, 2)
    infs = (ca.DemodInfo * 2)(inf, inf)
    assert f(a.h, 2, two, modes2, infs, None) == EINVAL
    fb = ca.FastFirBatch(2, 2048)
    fb.setup(-5000, 5000, 0, 62500.0)
    before = fb.response(0)
    g = L.csdr_fastfir_batch_setup_many
    d = (C.c_double * 1)(100.0)
    d2 = (C.c_double * 1)(2000.0)
    z = (C.c_double * 1)(0.0)
    fs = (C.c_double * 1)(62500.0)
    assert g(fb.h, 0, None, None, None, None, None, None) == 0
    assert g(fb.h, -1, one, d, d2, z, fs, st) == EINVAL
    assert g(fb.h, 1, None, d, d2, z, fs, st) == EINVAL
    assert g(fb.h, 1, one, d, None, z, fs, st) == EINVAL
    assert g(fb.h, 1, (C.c_int * 1)(2), d, d2, z, fs, st) == EINVAL
    assert g(fb.h, 1, (C.c_int * 1)(-2), d, d2, z, fs, st) == EINVAL
    assert np.array_equal(fb.response(0), before)
    sh = ca.ShardedDemodBatch([0, 0], 4, 2048)
    s = L.csdr_demod_shard_set_demod_many
    assert s(sh.h, 0, None, None, None, None) == 0
    assert s(sh.h, 1, (C.c_int * 1)(4), mode, C.byref(inf), st) == EINVAL
    assert s(sh.h, -1, one, mode, C.byref(inf), st) == EINVAL
    assert s(sh.h, 1, one, mode, None, st) == EINVAL
    x = np.stack([_signal({"FM": "FM", "AM": "AM", "USB": "T"}[m], 0, 8 * LIM, FS) for m in names])
    ga, gb = a.process(x), b.process(x)
    for c in range(len(names)):
        assert np.array_equal(ga[c].view(np.uint32), gb[c].view(np.uint32)), c
