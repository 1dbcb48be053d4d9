"""The premises of the K9 word rule (k9_words.py), without a GPU: the cap on undecided words on every row of the GPU
file, the restatement inside its own band, the input guards (which kernel paths the streams take, from the
restatement's trace and the csdr__host_tg_* hooks only) and ten fault models that the old bound of
test_testgen_gpu.py lets through and the rule does not.  Run with -s for the figures."""
import ctypes as C
import math

import numpy as np
import pytest

import k9_words as K
from test_testgen_host import HostGen, L                                # noqa: F401  (L is the library fixture)
import testgen_ref as R

LD = np.longdouble
ROWS = [(K.MAIN, c) for c in range(len(K.RECEIVERS)) if K.RECEIVERS[c][6]] + \
       [(p, c) for p in K.NOISE.values() for c in range(len(K.NOISE_RECEIVERS))]
ROW_IDS = ["%s-%d" % (p.name, c) for p, c in ROWS]
FORMS = [(False, 2, 512), (True, 4, 1024)]                              # real, samples per lane, per workgroup


def test_longdouble_has_64_bits():
    assert np.finfo(LD).nmant >= 63


def test_exact_phase_forms_agree():
    """the (hi, lo) pair at every sample against the Fraction form, on the through-zero sweep at the odd rate"""
    d = K.reference(K.MAIN, K.THROUGH_ZERO)
    f = d["freq"][:2560]
    hi, lo = K.exact_turns_all(f, K.FS1)
    at = [0, 1, 2, 777, 1817, 1818, 1819, 2559]
    ex = K.exact_turns(f, K.FS1, at)
    for j in at:
        assert abs(float(ex[j]) - float(hi[j] + lo[j])) <= 2.0 ** -60
    f2 = d["freq"][-3072:]
    hi, lo = K.exact_turns_all(f2, K.FS2)
    ex = K.exact_turns(f2, K.FS2, [3071])
    assert abs(float(ex[3071]) - float(hi[3071] + lo[3071])) <= 2.0 ** -60
    assert d["restart"][0] and d["restart"][-3072] and np.count_nonzero(d["restart"]) == 2


# ------------------------------------------------------------------------------------------------- cap and band
@pytest.mark.parametrize("plan,c", ROWS, ids=ROW_IDS)
def test_cap_and_restatement_inside_its_band(plan, c):
    """per row, both forms: at most 8 % of the gate-open words undecided per component; the restatement's own fp64
    output inside [y - delta, y + delta] on every sample"""
    d = K.reference(plan, c)
    assert d["on"].any() and (d["on"] & d["gate"]).any()
    for real, _, _ in FORMS:
        share = K.undecided_share(d, real)
        y, delta = K.centre(d, real)
        ref = K.columns(d["ref_real"] if real else d["ref"], real)
        err = np.abs(ref.astype(LD) - y)[d["on"]]
        print("%s receiver %d %s: undecided %s %%, restatement within %.3g counts (delta up to %.3g)" %
              (plan.name, c, "real" if real else "complex", ", ".join("%.2f" % (100 * s) for s in share),
               float(err.max()), float(delta.max())))
        assert max(share) <= K.CAP
        assert (err <= delta[d["on"]]).all()


def test_restarts_are_where_the_slots_are():
    want = {0: [0, 5120], 5: [0, 4096, 5120], 12: [0, 2560, 4096, 5120], 13: [0, 2560, 5120], 14: [0, 4096, 5120],
            15: [0, 5120]}
    for c, at in want.items():
        assert list(np.nonzero(K.reference(K.MAIN, c)["restart"])[0]) == at, c
    d = K.reference(K.MAIN, 15)
    assert not d["on"][2560:4096].any() and d["on"][:2560].all() and d["on"][4096:].all()
    assert not K.reference(K.MAIN, K.OFF_ROW)["on"].any()


# ------------------------------------------------------------------------------------------------- the host half
def host_rows(L, plan, c, cut):
    """receiver c through the library's host state machine in the calls of a cut: phase words, gate, launches per call"""
    g = HostGen(L)
    R.configure(g, plan.receivers[c])
    ph, gate, launches = np.zeros(plan.n, dtype=np.uint64), np.zeros(plan.n, dtype=bool), []
    for events, m, fs, pos, _, _ in K.calls(plan, cut, 2)[0]:
        for rc, name, v in events:
            if rc == c:
                R.slot(g, name, v)
        if not g.on:
            launches.append(0)
            continue
        ph[pos:pos + m], gate[pos:pos + m], k = g.run(m, fs)
        launches.append(k)
    return ph, gate, launches


def launches_of_prefix(L, plan, c, cut, call, m_last):
    g = HostGen(L)
    R.configure(g, plan.receivers[c])
    for i, (events, m, fs, _, _, _) in enumerate(K.calls(plan, cut, 2)[0]):
        for rc, name, v in events:
            if rc == c:
                R.slot(g, name, v)
        if i == call:
            return g.run(m_last, fs)[2]
        if g.on:
            g.run(m, fs)


def launch_starts(L, plan, c, cut, call, m, launches):
    """j_lo of the call's launches behind the first: the largest prefix of the call that k launches still cover"""
    out = []
    for k in range(1, launches):
        lo, hi = 1, m                                                   # launches(lo) <= k < launches(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if launches_of_prefix(L, plan, c, cut, call, mid) <= k:
                lo = mid
            else:
                hi = mid
        out.append(lo)
    return out


@pytest.mark.parametrize("c", [c for c in range(len(K.RECEIVERS)) if K.RECEIVERS[c][6]])
def test_host_phase_and_gate_on_these_streams(L, c):
    """the library's 128-bit phase within 1.5e-12 rad of the exact one (its share of PHI) and its gate equal to the
    restatement's, on every sample of every cut; the words do not depend on the cut"""
    d = K.reference(K.MAIN, c)
    first = None
    for cut in K.CUTS:
        ph, gate, _ = host_rows(L, K.MAIN, c, cut)
        on = d["on"]
        assert np.array_equal(gate[on], d["gate"][on])
        diff = (ph[on].astype(LD) * LD(2.0) ** -64 - d["turns"][on].astype(LD) + LD(0.5)) % LD(1.0) - LD(0.5)
        err = float(np.abs(diff).max()) * 2.0 * math.pi              # (turns kept to 2^-53: 7e-16 rad)
        assert err <= 1.5e-12, (c, cut, err)
        if first is None:
            first = ph
        assert np.array_equal(ph, first)
    print("receiver %d: host phase within %.3g rad of exact" % (c, err))


# ------------------------------------------------------------------------------------------------- input guards
def boundaries(d):
    """samples whose frequency was reached by another exact increment than the sample before it"""
    f = d["freq"].astype(LD)
    e = np.diff(f)
    b = np.zeros(len(f), dtype=bool)
    b[2:] = e[1:] != e[:-1]
    ok = d["on"].copy()
    ok[2:] &= d["on"][1:-1] & d["on"][:-2]
    for i in np.nonzero(d["restart"])[0]:
        ok[i:i + 2] = False
    return b & ok


def test_guard_run_boundaries_cover_every_lane_position():
    for real, q, wg in FORMS:
        res, with_b, without_b = set(), 0, 0
        for cut in K.CUTS:
            _, jcall = K.positions(K.MAIN, cut, q)
            for c in (4, 5, 8, 12, 13):
                b = boundaries(K.reference(K.MAIN, c))
                res |= set(int(j) % q for j in jcall[b])
                for _, m, _, pos, _, _ in K.calls(K.MAIN, cut, q)[0]:
                    for w in range(0, m, wg):
                        if b[pos + w:pos + min(m, w + wg)].any():
                            with_b += 1
                        else:
                            without_b += 1
        print("%s: run boundaries at lane positions %s; %d workgroups with a boundary, %d without" %
              ("real" if real else "complex", sorted(res), with_b, without_b))
        assert res == set(range(q))
        assert with_b > 0 and without_b > 0


def test_guard_launches_and_their_starts(L):
    """the through-zero receiver's longest call takes >= 3 launches, and some launch starts off a lane's first sample"""
    c = K.THROUGH_ZERO
    starts = []
    for cut in K.CUTS:
        cs = K.calls(K.MAIN, cut, 2)[0]
        _, _, launches = host_rows(L, K.MAIN, c, cut)
        longest = max(range(len(cs)), key=lambda i: cs[i][1])
        print("through-zero receiver, cut %s: launches per call %s" % (cut, launches))
        if cut == "one":
            assert launches[longest] >= 3
        for i, k in enumerate(launches):
            if k > 1:
                starts += launch_starts(L, K.MAIN, c, cut, i, cs[i][1], k)
    print("launch starts j_lo:", starts)
    assert any(j % 2 for j in starts) and any(j % 4 for j in starts)
    assert len(set(j % 4 for j in starts)) >= 3


def test_guard_ragged_cut():
    for _, q, _ in FORMS:
        cs, width = K.calls(K.MAIN, "ragged", q)
        counts = [m for _, m, _, _, _, _ in cs]
        assert counts[:6] == [2, 6, 1022, 510, 333, 2560 - 1873]
        assert any(m % 2 for m in counts) and all(off % q == 0 for _, _, _, _, off, _ in cs)
        assert width > K.N                                              # odd counts leave gaps
        assert sum(1 for ev, *_ in cs if ev) == 3                       # slots between the calls
    assert sum(m for _, m, _, _, _, _ in K.calls(K.MAIN, "256", 2)[0]) == K.N


def test_guard_gate_edges(L):
    for real, q, wg in FORMS:
        res, across = set(), 0
        for cut in K.CUTS:
            _, jcall = K.positions(K.MAIN, cut, q)
            for c in (7, 8, 10, 14, 16):
                d = K.reference(K.MAIN, c)
                edge = np.zeros(K.N, dtype=bool)
                edge[1:] = (d["gate"][1:] != d["gate"][:-1]) & (jcall[1:] > 0)
                res |= set(int(j) % q for j in jcall[edge])
                across += int(np.count_nonzero(edge & (jcall % wg == 0)))
        print("%s: gate edges at lane positions %s, %d across a workgroup boundary" %
              ("real" if real else "complex", sorted(res), across))
        assert res == set(range(q)) and across > 0
        for cut in K.CUTS:                                              # the gate re-opens inside a call: the timer wrapped there
            _, jcall = K.positions(K.MAIN, cut, q)
            g = K.reference(K.MAIN, 7)["gate"]
            assert (g[1:] & ~g[:-1] & (jcall[1:] > 0)).any()
    # the timer wraps inside a call (receiver 7: period 100 samples) and never within the stream (receiver 10)
    k, w = C.c_ulonglong(), C.c_ulonglong()
    L.csdr__host_tg_pulse_pattern(K.FS1, K.RECEIVERS[7][4], K.RECEIVERS[7][3], C.byref(k), C.byref(w))
    assert (k.value, w.value) == (100, 7)
    L.csdr__host_tg_pulse_pattern(K.FS1, K.RECEIVERS[8][4], K.RECEIVERS[8][3], C.byref(k), C.byref(w))
    assert (k.value, w.value) == (101, 21)
    L.csdr__host_tg_pulse_pattern(K.FS1, K.RECEIVERS[10][4], K.RECEIVERS[10][3], C.byref(k), C.byref(w))
    assert k.value > K.N and w.value == 1025
    g = K.reference(K.MAIN, 10)["gate"]
    assert g[:1024].all() and not g[1024:5120].any()
    assert K.reference(K.MAIN, 9)["gate"].all()                         # width >= period


# ------------------------------------------------------------------------------------------------- fault models
def to_f32_toward_zero(x):
    f = x.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(x)
    return np.where(over, np.nextafter(f, np.float32(0.0)), f)


def model(d, real, fault=0):
    """the kernel's stated arithmetic in numpy fp64 from the exact phase (read at 2^-34 turn, amp * cos + namp * g,
    one rounding to fp32), with one of the faults of the list below; (n, 2) / (n, 1) values of fp32 words"""
    turns = d["turns"].copy()
    if fault == 2:                                                      # odd samples lag by one increment step
        step = np.zeros(K.N)
        step[1:] = (d["freq"][1:] - d["freq"][:-1]) / np.where(d["fs"][1:] > 0, d["fs"][1:], 1.0)
        step[~d["on"] | d["restart"]] = 0.0
        step[0::2] = 0.0
        turns = turns - step
    unit = 2.0 ** 24 if fault == 3 else 2.0 ** 34
    ang = 2.0 * math.pi * (np.floor(turns * unit) / unit)
    if fault == 1:
        ang = ang + 1e-6
    gate = d["gate"]
    if fault == 7:                                                      # gate one sample late
        gate = np.concatenate(([gate[0]], gate[:-1]))
    amp = np.where(gate, d["amp"], 0.0)
    if real:
        amp = (3.0 * amp).astype(np.float32).astype(np.float64) if fault == 10 else 3.0 * amp
    if fault == 4:
        amp = amp * (1.0 + 1e-6)
    g1, g2 = d["g1"], d["g2"]
    if fault == 8:                                                      # the radius from an fp32 log
        ln = -(g1 * g1 + g2 * g2) / 2.0                                # = ln r of the accepted attempt
        k = np.sqrt(np.where(ln < 0, ln.astype(np.float32).astype(np.float64) / np.where(ln < 0, ln, 1.0), 1.0))
        g1, g2 = g1 * k, g2 * k
    out = []
    for t, g in ((np.cos(ang), g1),) if real else ((np.cos(ang), g1), (np.sin(ang), g2)):
        if fault == 5:
            t = t.astype(np.float32).astype(np.float64)
        sig = amp * t
        if fault == 9:
            sig = sig.astype(np.float32).astype(np.float64)
        v = sig + d["namp"] * g
        out.append(to_f32_toward_zero(v) if fault == 6 else v.astype(np.float32))
    return np.stack(out, axis=1).astype(np.float64)


def swept(d):
    on = d["on"][1:] & d["on"][:-1] & ~d["restart"][1:]
    return bool(((d["freq"][1:] != d["freq"][:-1]) & on)[1::2].any())


def gated(d):
    return bool((d["on"] & ~d["gate"]).any())


def tripled_amp_inexact(d):
    a = 3.0 * d["amp"][d["on"]]
    return bool((np.abs(a.astype(np.float32).astype(np.float64) - a) > 1e-8 * a).all())


MAIN_ROWS = [(K.MAIN, c) for c in range(len(K.RECEIVERS)) if K.RECEIVERS[c][6]]
NOISE_ROWS = [(p, c) for p in K.NOISE.values() for c in range(len(K.NOISE_RECEIVERS))]
# fault: (name, rows it can apply to, the row's condition, forms)
FAULTS = {
    1: ("phase + 1e-6 rad", MAIN_ROWS, None, (False, True)),
    2: ("odd samples lag by one increment step on a sweep", MAIN_ROWS, swept, (False, True)),
    3: ("phase truncated to 2^-24 turn", MAIN_ROWS, None, (False, True)),
    4: ("gain 1 + 1e-6", MAIN_ROWS, None, (False, True)),
    5: ("cosine rounded to fp32 before the product", MAIN_ROWS, None, (False, True)),
    6: ("conversion to float truncates toward zero", MAIN_ROWS + NOISE_ROWS, None, (False, True)),
    7: ("gate one sample late", MAIN_ROWS, gated, (False, True)),
    # the fault moves a word by 1.5e-8 namp |g|: under the full-scale tone (receiver 2) that is 5e-6 counts against fp32
    # words 2e-3 counts and more apart, so it applies where the noise is the word: receivers 0, 1 and the gated 3
    8: ("noise radius from an fp32 log", [r for r in NOISE_ROWS if r[1] != 2], None, (False, True)),
    # on the -160 dB rows the rounding moves the centre by 2^-25 * 3.3e-4 = 1e-11 counts under noise whose fp32 words
    # are 1e-7 counts and more apart: no word can show it, so the fault applies to the rows with a signal
    9: ("signal rounded to fp32 before the noise is added", [r for r in NOISE_ROWS if r[1] >= 2], None, (False, True)),
    # 3 * 32767 = 98301 is an fp32 number: the fault changes nothing on the full-scale rows
    10: ("3 * amp rounded to fp32", MAIN_ROWS, tripled_amp_inexact, (True,)),
}


def test_the_unfaulted_model_passes_both():
    for plan, c in MAIN_ROWS + NOISE_ROWS:
        d = K.reference(plan, c)
        for real in (False, True):
            got = model(d, real)
            t = K.Tally("model, %s receiver %d %s" % (plan.name, c, "real" if real else "complex"), d, real, got)
            assert t.ok, str(t)
            assert K.passes_old_bound(d, real, got)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_fault_passes_the_old_bound_and_fails_the_rule(fault):
    name, rows, cond, forms = FAULTS[fault]
    old_passes, applied, counts = 0, 0, []
    for plan, c in rows:
        d = K.reference(plan, c)
        if cond is not None and not cond(d):
            continue
        for real in forms:
            applied += 1
            got = model(d, real, fault)
            old_passes += K.passes_old_bound(d, real, got)
            t = K.Tally("fault %d, %s receiver %d %s" % (fault, plan.name, c, "real" if real else "complex"), d, real, got)
            counts.append(t.bad)
            assert t.bad > 0, str(t)
    print("fault %d (%s): %d rows and forms, %d pass the old bound, %d ... %d words of a row outside their interval" %
          (fault, name, applied, old_passes, min(counts), max(counts)))
    assert applied > 0 and old_passes > 0
    if fault == 7:                                                      # the -160 dB row behind the gate
        d = K.reference(K.MAIN, K.GATED_TINY)
        assert gated(d) and K.passes_old_bound(d, False, model(d, False, 7))
    if fault == 2:
        assert applied >= 2 * 5
    if fault == 10:
        assert applied >= 5
