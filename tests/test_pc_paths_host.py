"""The CPU model of K4's path decisions (tests/pc_paths_ref.py), checked without a GPU: its sequential averagers are pinned to
oracle.CAgc through the AGC's output at the leaf bound, and for every AGC input of tests/test_pc_paths_gpu.py it predicts what
that test relies on -- the histogram of rounds per tile, none beyond PC_AGC_ROUNDS, tiles on both sides of every forced round
limit, a tile whose first scan converges and whose second does not at one wave per channel, at most 5 % of the tiles undecided."""
import numpy as np
import pytest
import pc_paths_ref as R

FULL_SCALE = 32767.0
STEADY = 2e-5 * FULL_SCALE          # the leaf bound of tests/test_postchain_gpu.py

_streams = {}


def stream(name):
    """(model output, per-tile records) of an AGC case: computed once, read-only"""
    if name not in _streams:
        y, rec = R.agc_stream(R.agc_params(name), R.agc_input(name), R.AGC_CALLS)
        y.setflags(write=False)
        _streams[name] = (y, tuple(rec))
    return _streams[name]


@pytest.mark.parametrize("name", sorted(R.AGC_CASES))
def test_the_models_sequential_averagers_are_the_oracles(oracle, name):
    """the gain argument max(attack, decay) is compared through the output: delayed input x gain, call by call"""
    fs, hang, thresh, slope, decay, seed = R.AGC_CASES[name]
    x = R.agc_input(name)
    r = oracle.CAgc()
    r.SetParameters(True, hang, thresh, 30, slope, decay, fs)
    want = np.concatenate([r.ProcessData(x[a:a + m]) for a, m in zip(np.cumsum([0] + R.AGC_CALLS[:-1]), R.AGC_CALLS)])
    got = stream(name)[0]
    err = np.abs(got - want).max()
    print("%s: model against oracle.CAgc %.3g of full scale (bound %.3g)" % (name, err / FULL_SCALE, STEADY / FULL_SCALE))
    assert np.abs(want).max() > 100.0 and err <= STEADY


def test_sliding_peaks_are_the_maximum_of_the_window():
    rng = np.random.default_rng(3)
    mg = rng.standard_normal(3000).astype(np.float32)
    for win in (1, 2, 17, 281, 1125):
        pk, hist = R.sliding_peaks(mg[:1700], win)
        pk2, _ = R.sliding_peaks(mg[1700:], win, hist)
        e = np.concatenate([np.full(win - 1, -16.0, dtype=np.float32), mg])
        want = np.array([e[i:i + win].max() for i in range(len(mg))])
        assert np.array_equal(np.concatenate([pk, pk2]), want), win


def test_tiles_are_cut_from_each_bursts_start():
    assert R.cut_tiles([1, 1500, 2048]) == [(0, 1), (1, 1024), (1025, 476), (1501, 1024), (2525, 1024)]
    assert R.cut_tiles([4096, 2048], burst=1024) == [(k * 1024, 1024) for k in range(6)]
    assert len(R.cut_tiles(R.AGC_CALLS)) == 24 and len(R.cut_tiles(R.PLL_CALLS)) == 41


def test_round_count_of_a_hand_made_tile():
    """a peak that steps up in mid-tile: the first guess (all selectors against the start average) is already the truth for a
    rising step; a step down that the average only crosses later needs a second round"""
    up = np.concatenate([np.full(100, -5.0), np.full(100, -3.0)])
    assert R._rounds(up, -5.5, 0.01, 0.004)[0] == 1
    down = np.concatenate([np.full(50, -3.0), np.full(150, -4.0)])       # the average rises above -4 on the way: selectors flip
    r, margin = R._rounds(down, -5.0, 0.05, 0.02)
    assert r == 2 and margin > R.TIE


@pytest.mark.parametrize("name", sorted(R.AGC_HISTOGRAMS))
def test_round_histograms_the_gpu_test_relies_on(name):
    rec = stream(name)[1]
    r2 = R.scan2_rounds(rec)
    print(name, "rounds per tile (attack, decay):", [(a, d) for a, d, _ in rec])
    assert R.histogram(r2) == R.AGC_HISTOGRAMS[name]
    assert all(r is not None and r <= R.AGC_ROUNDS for r in r2)
    und = sum(not d for d in R.decided(rec))
    assert und <= R.UNDECIDED_CAP * len(rec), (und, len(rec))


def test_forced_round_limits_leave_tiles_on_both_sides():
    """limit 1 and 2: scanned and walked tiles in one stream, 10 ... 50 % walked in the case the limit is tested on; limit 0:
    everything walks; one wave per channel: a tile whose attack scan converges within the limit and whose decay scan does not"""
    for name, limit in (("steps62k5", 1), ("steps15k6", 2)):
        rec = stream(name)[1]
        paths = [R.agc_path(a, d, limit, 4)[0] for a, d, _ in rec]
        walked = paths.count("walk_rounds") / len(paths)
        assert 0.10 <= walked <= 0.50 and paths.count("scan") > 0, (name, limit, walked)
        one = [R.agc_path(a, d, limit, 1) for a, d, _ in rec]
        assert any(p[2] == 2 for p in one) and any(p[0] == "scan" for p in one), (name, limit)
    for name in R.AGC_HISTOGRAMS:
        assert all(R.agc_path(a, d, 0, 4)[0] == "walk_rounds" for a, d, _ in stream(name)[1])


def test_census_words_decode():
    w = np.zeros(R.HEADER_WORDS + 2 * R.RECORD_WORDS, dtype=np.uint32)
    w[1], w[2], w[3], w[4], w[5] = 2, R.force_word(agc_limit=1, skip_scan=True, overlap_mod=3, overlap_rem=2), 4 | 1 << 8, 2, 1
    w[8:12] = [2 | 3 << 4 | 1 << 16, 1024 | 3 << 16 | 4 << 20 | 1 << 28, 1 | 0 << 16 | 5 << 24, 7]
    w[12:16] = [4 | 2 << 4 | 2 << 12 | 3 << 16 | 1 << 19 | 1 << 23, 476 | 0 << 16, 1, 8]
    head, recs = R.decode(w)
    assert head == dict(capacity=2, force=2 | 16 | 3 << 8 | 2 << 16, nw=4, lean=True, records=2, walks=1)
    assert (recs[0]["agc"], recs[0]["rounds"], recs[0]["pll"], recs[0]["n"], recs[0]["mode"], recs[0]["row"], recs[0]["ordinal"],
            recs[0]["nw"], recs[0]["lean"]) == ("scan", 3, "scan", 1024, 2, 5, 7, 4, True)
    assert (recs[1]["agc"], recs[1]["rounds"], recs[1]["failed"], recs[1]["pll"], recs[1]["zero_code"], recs[1]["overlap_forced"],
            recs[1]["scan_bad"], recs[1]["mode"]) == ("walk_rounds", 2, 2, "walk", True, True, False, -1)


def test_pll_segments_cover_the_paths_by_construction():
    for kind in ("fm", "sam"):
        x, tiles = R.pll_tile_expectations(kind)
        kinds = [k for _, _, k, _ in tiles]
        assert len(tiles) == 41 and {"scan", "zero", "never_scan", None} == set(kinds)
        zero = [(s, n) for s, n, k, _ in tiles if k == "zero"]
        assert zero and all((x[s:s + n] == 0).all() for s, n in zero)
        assert sum(1 for _, _, k, since in tiles if k == "scan" and since >= R.PLL_SETTLE[kind]) >= 4


# ---- the chain input of the GPU test, end to end: what an fp32 filter's error floor does to the ORACLE chain on it ---------------
_spread = {}


def chain_spread(oracle, c):
    """per-burst max |audio(disturbed filter output) - audio(fp64 filter output)| of receiver c's oracle chain on the GPU test's
    chain input, maximum over three seeds and the two disturbances of tests/startup_bounds.py, in units of full scale"""
    if c not in _spread:
        import test_pc_paths_gpu as P
        import test_postchain_gpu as T
        x = once_chain_input(P)[c].astype(np.complex128)

        def run(perturb=None):
            m, kw = P.chain_kw(c)
            r = oracle.CDemodulator(2048)
            r.SetInputSampleRate(P.CHAIN_FS); r.SetDemod(m, T.info(oracle, **kw)); r.SetDemodFreq(-100e3 - 1000.0 * c)
            if perturb:
                r.perturb_filter_output(*perturb)
            return np.concatenate([r.process_append(x[k * P.CHAIN_CALL:(k + 1) * P.CHAIN_CALL]) for k in range(P.CHAIN_CALLS)])
        base = run()
        worst = np.zeros(len(base) // 1024)
        for seed in (1, 2, 3):
            for p in ((3, 3e-7, seed), (4, 1e-8, 100 + seed)):
                worst = np.maximum(worst, T.burst_errors(run(p), base) / FULL_SCALE)
        _spread[c] = worst
    return _spread[c]


def once_chain_input(P):
    if "x" not in _spread:
        _spread["x"] = P.chain_input()
    return _spread["x"]


@pytest.mark.parametrize("c", [0, 1, 3, 4, 5], ids=["AM", "SAM", "FM", "USB-hang", "CWU"])
def test_chain_input_spread_of_the_oracle_behind_an_fp32_filter(oracle, c):
    """The bursts in which tests/test_pc_paths_gpu.py allows the chain more than the chain rule are those -- and only those --
    where the oracle chain moves by more than half the rule's steady bound when its own filter output is disturbed like an fp32
    filter's; the recorded spreads (pc_paths_ref.CHAIN_STEP_SPREAD) are reproduced within x 1/3 ... x 1.5, as
    tests/test_oracle_independent.py holds the start-up spreads.  FM, and USB with the hang timer, have no such burst."""
    import test_pc_paths_gpu as P
    import startup_bounds as SB
    name = P.CHAIN_NAMES[c]
    worst = chain_spread(oracle, c)
    rec = R.CHAIN_STEP_SPREAD.get(name, {})
    print(name, "spread per burst:", " ".join("%.1e" % v for v in worst))
    for b, s in rec.items():
        assert s / 3.0 <= worst[b] <= 1.5 * s, (name, b, worst[b], s)
        assert SB.FACTOR * s > 2e-5
    first = len(SB.FM_STARTUP) + 1 if name == "FM" else 2          # (in front of it the chain rule has its own start-up bounds)
    steady = (3e-5 if name == "FM" else 2e-5) / SB.FACTOR
    others = [b for b in range(first, len(worst)) if b not in rec]
    assert others and all(worst[b] <= steady for b in others), (name, [(b, worst[b]) for b in others if worst[b] > steady])
