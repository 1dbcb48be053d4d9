"""CPU side of the K4 sample rule (tests/pc_samples_ref.py): the float64 model is the oracle's operation, every condition the
GPU file relies on holds on every one of its inputs, the fp32 yardstick passes the rule, and the yardstick with one thing wrong
does not -- with, per fault, whether the bounds K4 had (2e-5 of full scale, 0.01 dB) accept it.  Run with -s for the tables."""
import numpy as np
import pytest
import pc_paths_ref as P
import pc_samples_ref as S

F32, F64 = S.F32, S.F64
PIN = 1e-12                  # of a window's rms: float64 model against the oracle
PIN_DB = 1e-10               # dB, the S-meter's readings (log10 of numpy against libm's)


@pytest.fixture(scope="module")
def designs(oracle):
    return S.Designs(oracle)


@pytest.fixture(scope="module")
def rows():
    return S.leaf_rows()


_want = {}


def oracle_output(oracle, row):
    if row.name not in _want:
        _want[row.name] = row.run(row.build(oracle))
    return _want[row.name]


def test_float64_model_is_the_oracle(oracle, designs, rows):
    """counts equal, outputs within 1e-12 rms per window, exact zeros in the same places, squelch decisions equal call by call;
    the rows through the ragged cuts carry every state across calls of 1, 17, 1000, 1025, 2500, 1, 4099, 333 and 2048 samples"""
    worst = 0.0
    for row in rows.values():
        want = oracle_output(oracle, row)
        got, m = S.model_output(row, designs, F64)
        if row.stage == "smeter":
            for g, w in zip(got, want):
                assert np.abs(g - w).max() <= PIN_DB, (row.name, np.abs(g - w).max())
            continue
        assert got.shape == want.shape and got.dtype == want.dtype, row.name
        E, R = S.window_errors(got, want)
        assert (E <= PIN).all(), (row.name, E.max())
        np.testing.assert_array_equal(got == 0, want == 0, err_msg=row.name)
        worst = max(worst, float(E.max()))
        if row.stage == "fm":
            r = row.build(oracle)
            dec = []
            for p in S.split(row.x, row.calls):
                r.ProcessData(p, 5000.0, row.stereo); dec.append(r.squelched())
            assert dec == m.decisions, row.name
    print("float64 model against the oracle: largest max|e| / rms per window %.2e" % worst)


def test_post_chain_model_is_the_oracles_post_chain(oracle, designs):
    """the chain form (S-meter, AGC, demodulator as SetDemod configures them) against the oracle's objects in ragged calls"""
    import test_chain_taps_gpu as TC
    import test_postchain_gpu as T
    for mode, fs in (("AM", 31250.0), ("SAM", 31250.0), ("FM", 62500.0), ("USB", 15625.0), ("CWU", 15625.0)):
        kw = dict(T.MODES[mode][1])
        if mode == "USB":
            kw.update(AgcHangOn=1, AgcDecay=500)
        x = (S.fm_input("-12dBFS", 5000, fs) if mode == "FM" else S.am_input("-12dBFS", 5000, fs)) * 0.1
        post = TC._oracle_post_chain(oracle, mode, False, fs, kw)
        di = T.info(oracle, **kw)
        m = S.PostChain(designs, mode, {k: getattr(di, k) for k, _ in di._fields_}, fs, F64)
        sm = oracle.CSMeter()
        for part in S.split(x, [1, 1500, 1024, 2475]):
            want, got = post(part)[1], m.process(part)
            sm.ProcessData(part, fs)
            E, _ = S.window_errors(got, want)
            assert (E <= PIN).all(), (mode, E)
            assert abs(m.sm.get_ave() - sm.GetAve()) <= PIN_DB and abs(m.sm.get_peak() - sm.GetPeak()) <= PIN_DB, mode


def test_conditions_hold_on_every_gpu_input(designs, rows):
    """everything here is computed from the float64 statement alone"""
    left_out = 0
    for row in rows.values():
        out, m = S.model_output(row, designs, F64)
        if row.stage in ("fm", "sam") and row.carrier:
            lo = S.pll_windows_left_out(m.errs)
            assert len(lo) <= S.PLL_MAX_LEFT_OUT and all(w <= 1 for w in lo), (row.name, lo)
            left_out += len(lo)
        if row.stage == "fm":
            assert S.squelch_clear(m), (row.name, m.sq_aves, m.thresh)
            assert all(m.decisions) != row.carrier and any(m.decisions) != row.carrier, (row.name, m.decisions)   # open on a carrier, shut without
        if row.stage == "agc" and row.manual is None:
            if row.agc[0]:
                assert m.margin >= P.TIE, (row.name, m.margin)                 # hang: a tie would flip the timer
            elif not row.real:
                share = S.agc_undecided_share(m.p, row.x, row.calls)
                assert share <= P.UNDECIDED_CAP, (row.name, share)
        if row.stage != "smeter":
            _, R = S.window_errors(out, out)
            if row.carrier:
                assert (R >= S.MIN_RMS).all(), (row.name, R.min())             # scale: -100 dBFS tests scale, not a division by zero
            else:
                assert not out.any(), row.name                                 # no carrier: every word zero
    print("PLL windows left out over all leaf streams: %d" % left_out)
    assert left_out == 0


def test_levels_scale_as_the_stage_says(designs, rows):
    """FM does not care about the level; SAM's loop does not and its audio scales with it, as AM's and the manual gain's do;
    the S-meter moves by the dB"""
    ref = "-12dBFS"
    for lev in ("-60dBFS", "-100dBFS", "over"):
        k = S.LEVELS[lev] / S.LEVELS[ref]
        for w in ("mono", "stereo"):
            a, _ = S.model_output(rows["fm/%s/%s" % (w, ref)], designs, F64)
            b, _ = S.model_output(rows["fm/%s/%s" % (w, lev)], designs, F64)
            assert np.abs(a - b).max() <= 1e-4 * S._rms(a), (lev, w)            # (the inputs are rounded to fp32 after scaling)
            for st in ("am", "sam"):
                a, _ = S.model_output(rows["%s/%s/%s" % (st, w, ref)], designs, F64)
                b, _ = S.model_output(rows["%s/%s/%s" % (st, w, lev)], designs, F64)
                assert np.abs(a * k - b).max() <= 1e-4 * S._rms(b), (lev, w, st)
        a, _ = S.model_output(rows["smeter/" + ref], designs, F64)
        b, _ = S.model_output(rows["smeter/" + lev], designs, F64)
        assert abs(b[0][-1] - a[0][-1] - 20 * np.log10(k)) <= 1e-3, lev       # once the start from -120 dB is forgotten


def test_yardstick_passes_the_rule_and_resolves_fp32(oracle, designs, rows):
    """the yardstick is its own E_y, so it passes at any margin >= 1; what matters is that E_y is of fp32 size at every level
    (no window's yardstick error above 1e-5 of the window's rms, none exactly zero but the manual gains' exact products)"""
    table = {}
    for row in rows.values():
        want = oracle_output(oracle, row)
        y, _ = S.model_output(row, designs, F32)
        if row.stage == "smeter":
            for g, w in zip(y, want):
                E, Ey, ratio = S.db_rule(g, w, g)
                assert E <= S.M * Ey and Ey <= 2e-5, (row.name, Ey)
            table.setdefault(row.form, []).append(S.db_rule(y[0], want[0], y[0])[1])
            continue
        w = S.check_windows(y, want, y)
        assert w.passed and not w.low, (row.name, w)
        if row.manual is not None:
            assert (np.abs(y - want) <= S.manual_bound(want)).all(), row.name
        elif row.carrier:
            assert (w.Ey[w.compared] > 0).all() and (w.Ey[w.compared] <= 1e-5).all(), (row.name, w)
        if row.carrier:
            table.setdefault(row.form, []).append(float(w.Ey[w.compared].max()))
    print("E_y per form (largest window of each row: smallest ... largest over the rows; S-meter in dB)")
    for form, v in table.items():
        print("  %-12s %.2e ... %.2e" % (form, min(v), max(v)))


def test_every_fault_model_fails_the_rule(oracle, designs, rows):
    """the yardstick with one thing wrong, on every row it applies to: rejected by the rule (some window above m E_y), and
    what the bounds K4 had say to it"""
    report = {}
    for row in rows.values():
        want = oracle_output(oracle, row)
        y, m64 = S.model_output(row, designs, F32)[0], S.model_output(row, designs, F64)[1]
        for fault in row.faults():
            if fault == "agc_slope" and row.level in ("-60dBFS", "-100dBFS") and row.agc[2] > -100:
                continue                                        # under the knee the gain is the fixed one: no slope in it
            bad, _ = S.model_output(row, designs, F32, fault)
            if row.stage == "smeter":
                E, Ey, ratio = S.db_rule(bad[0], want[0], y[0])                # GetAve after each call
                old = bool(np.abs(bad[0] - want[0]).max() <= S.OLD_DB)
            else:
                w = S.check_windows(bad, want, y)
                ratio, old = w.worst, S.old_rule_accepts(bad, want)
                assert w.zeros_equal
            report.setdefault(fault, []).append((row.name, ratio / S.M, old))
    assert set(report) == set(S.FAULTS)
    print("fault: rows, smallest and largest E / (m E_y), rows the old bounds accept at -12 dBFS / -60 dBFS / all")
    missed = []
    for fault in S.FAULTS:
        v = report[fault]
        r = [x[1] for x in v]
        acc = lambda tag: "%d of %d" % (sum(o for n, _, o in v if tag in n), sum(1 for n, _, _ in v if tag in n))
        print("  %-10s %2d rows  %8.3g ... %8.3g   old accepts %s / %s / %s" % (fault, len(v), min(r), max(r), acc("-12dBFS"), acc("-60dBFS"), acc("")))
        missed += [(fault, n, x) for n, x, _ in v if not x > 1.0]
    assert not missed, missed


def test_fp32_phase_differences_in_the_locked_loop_scan_miss_the_rule(designs, rows):
    """The defect the rule found in pll_scan (postchain_kernels.hip), reproduced on the yardstick.  The kernels run the loops on
    theta = atan2f(im, re) / 2 pi, an fp32 number of turns: that form alone ("theta_turns") stays within 2 E_y on every FM row.
    Unwrapping the input phase per tile by wrapped differences taken IN FP32 ("theta_unwrap32", the scan as it was) rounds every
    difference across the half-turn wrap (|d| near 1 is one bit coarser than the angles); the roundings stay in the unwrapped
    phase until the next tile drops them as one step, and the audio answers with a transient six samples later: above m E_y on
    the FM rows (measured on the MI355X before the fix: 4.76 ... 5.18).  The differences are taken in float64 now."""
    worst = {"theta_turns": 0.0, "theta_unwrap32": 0.0}
    for row in rows.values():
        if row.stage == "fm" and row.carrier:
            want, y = S.model_output(row, designs, F64)[0], S.model_output(row, designs, F32)[0]
            for form in worst:
                w = S.check_windows(S.model_output(row, designs, F32, form)[0], want, y)
                worst[form] = max(worst[form], w.worst)
    print("FM rows, largest E / E_y: theta in fp32 turns %.2f, and unwrapped by fp32 differences %.2f" % (worst["theta_turns"], worst["theta_unwrap32"]))
    assert worst["theta_turns"] <= 2.0 and worst["theta_unwrap32"] > S.M, worst
