"""Which path every tile of the post-chain walk (K4: S-meter -> AGC -> demodulator) took, and every path and handoff on purpose.

Each 1024-sample tile is first solved under a guess and re-done another way when the guess fails its check: the AGC averagers
by up to 8 rounds of guessed selectors, else a one-thread walk (always with the hang timer); the FM PLL by pll_scan, else
pll_overlap, else pll_walk; the SAM PLL by pll_scan, else pll_walk.  The other tests hold K4 to the oracle whichever path ran.
Here the diagnostic build cutesdr_amd/libcutesdr_mi_pccensus.so (-DPC_CENSUS, postchain.h) records the path of every tile and
takes a force word that picks a path -- never its arithmetic:

  1. with nothing forced its words are the product library's, byte for byte, so that its census speaks for the product;
  2. the census is what tests/pc_paths_ref.py predicts: the AGC round counts of every decided tile, the PLL path of every
     tile of a by-construction segment, "walked: hang" on every tile of a hang receiver, the (NW, LEAN) instantiation;
  3. under every force word both sides of the handoff it aims at ran -- asserted from the census -- and the output holds the
     existing bounds against the oracle: 2e-5 of full scale on the leaf objects (the AGC from the first sample; the PLLs on every
     tile of the carrier from reset, the exact zeros and the carrier behind them, and PLL_SETTLE tiles behind the jumps that
     follow an unlocked stretch; only the noise segment is left out), check_chain_bursts on every burst of the chain -- with
     twice the oracle's own spread in the few bursts where level steps make the oracle itself sensitive to an fp32 filter's
     error floor (check_chain_against_oracle) -- and K4 on the chain's own filter output against the oracle's stages;
  4. every forced run's output is the unforced run's to 1e-6 of full scale (the bound overlapped and sequential walks are
     already held to), FM squelch decisions identical;
  5. the inputs of the randomized sweeps (tests/test_randomized_gpu.py, imported) run once under the census: the table of
     paths they reach is printed, and FM and SAM must each show scanned and not-scanned tiles.

Every configuration (library, waves per channel, force word) runs in a child process of its own, one after the other, each
under a time limit; after a child that died nothing else starts.  Shapes: leaf objects on 24 (AGC) and 41 (PLL) tiles with
ragged calls, one batch chain of 6 receivers at the 2048-point filter in two calls of at least 4 bursts per receiver (mono: the
batch takes stereo for all its receivers, so SAM stereo is forced on the leaf object)."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import pc_paths_ref as R

pytestmark = pytest.mark.gpu
FULL_SCALE = 32767.0
STEADY = 2e-5 * FULL_SCALE
PATHS_AGREE = 1e-6 * FULL_SCALE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

CHAIN_NAMES = ["AM", "SAM", "SAM", "FM", "USB", "CWU"]         # USB with the hang timer
CHAIN_FS, CHAIN_CALL, CHAIN_CALLS = 2e6, 19968 * 32, 2

# name: (force word, what of the workload it runs)
FORCES = {
    "none": (R.force_word(), ("agc", "fm", "sam", "chain")),
    "agc0": (R.force_word(agc_limit=0), ("agc", "chain")),
    "agc1": (R.force_word(agc_limit=1), ("agc", "chain")),
    "agc2": (R.force_word(agc_limit=2), ("agc", "chain")),
    "skipscan": (R.force_word(skip_scan=True), ("fm", "sam", "chain")),
    "overlap3": (R.force_word(overlap_mod=3, overlap_rem=1), ("fm", "chain")),
    # (the chain's FM carrier is locked: only with pll_scan skipped do its tiles reach pll_overlap and, rejected there, pll_walk)
    "skipoverlap3": (R.force_word(skip_scan=True, overlap_mod=3, overlap_rem=1), ("fm", "chain")),
    "skipwalk": (R.force_word(skip_scan=True, overlap_mod=1, overlap_rem=0), ("fm", "chain")),
}
AGC_LIMIT = {"agc0": 0, "agc1": 1, "agc2": 2}


def chain_kw(c):
    import test_postchain_gpu as T
    m, kw = T.MODES[CHAIN_NAMES[c]]
    kw = dict(kw)
    if CHAIN_NAMES[c] == "USB":
        kw.update(AgcHangOn=1, AgcDecay=500)
    return m, kw


def chain_input():
    """[receiver, sample]: the chain tests' carriers under level steps of 6 dB every 25 ms and a 30 Hz modulation (the AGC
    averagers then cross the peak in most tiles: tests/pc_paths_ref.py)"""
    import test_postchain_gpu as T
    n = CHAIN_CALL * CHAIN_CALLS
    t = np.arange(n) / CHAIN_FS
    env = np.where((t % 0.05) < 0.025, 1.0, 0.5) * (1 + 0.3 * np.sin(2 * np.pi * 30 * t))
    return np.stack([T.make_input(CHAIN_NAMES[c], n, CHAIN_FS) * np.exp(2j * np.pi * 1000.0 * c * t) * env
                     for c in range(len(CHAIN_NAMES))]).astype(np.complex64)


# ---- the child ---------------------------------------------------------------------------------------------------------------
class Census:
    """the census buffer of the loaded library around one piece of work (nothing where the library has no census)"""

    def __init__(self, on, force, cap):
        import ctypes as C
        import cutesdr_amd as ca
        self.on, self.cap, self.words = on, cap, np.zeros(0, dtype=np.uint32)
        if not on:
            return
        self.L, self.C, self.ca = ca.lib(), C, ca
        self.L.csdr__pc_census_set.restype = C.c_int
        self.L.csdr__pc_census_set.argtypes = [C.c_void_p]
        w = np.zeros(R.HEADER_WORDS + R.RECORD_WORDS * cap, dtype=np.uint32)
        w[1], w[2] = cap, force
        self.buf = ca.DeviceBuffer(w.nbytes)
        self.buf.upload(w)
        assert self.L.csdr__pc_census_set(C.c_void_p(self.buf.ptr)) == 0

    def end(self):
        if not self.on:
            return self.words
        self.ca.sync()
        self.words = self.buf.download(np.uint32, R.HEADER_WORDS + R.RECORD_WORDS * self.cap)
        assert self.L.csdr__pc_census_set(None) == 0
        self.buf.free()
        return self.words


def run_config(out_path, census, force, work):
    """(in the child) the workload on the library this interpreter loaded -> out_path (.npz)"""
    import cutesdr_amd as ca
    import test_postchain_gpu as T
    out = {}
    if "agc" in work:
        for name, (fs, hang, thresh, slope, decay, seed) in R.AGC_CASES.items():
            x = R.agc_input(name)
            cen = Census(census, force, 64)
            g = ca.CAgc()
            g.SetParameters(True, hang, thresh, 30, slope, decay, fs)
            out["agc/" + name] = np.concatenate([g.ProcessData(x[a:a + m]) for a, m in zip(np.cumsum([0] + R.AGC_CALLS[:-1]), R.AGC_CALLS)])
            out["agc/" + name + "/census"] = cen.end()
            g.close()
    cuts = np.cumsum([0] + R.PLL_CALLS)
    if "fm" in work:
        x, _ = R.pll_tile_expectations("fm")
        cen = Census(census, force, 64)
        d = ca.CFmDemod(R.PLL_FS["fm"])
        d.SetSquelch(50)
        ys, sq = [], []
        for k in range(len(R.PLL_CALLS)):
            ys.append(d.ProcessData(x[cuts[k]:cuts[k + 1]], 5000.0, False))
            sq.append(int(d.squelched()))
        out["fm"], out["fm/squelched"], out["fm/census"] = np.concatenate(ys), np.array(sq), cen.end()
        d.close()
    if "sam" in work:
        x, _ = R.pll_tile_expectations("sam")
        for stereo in (False, True):
            key = "sam_stereo" if stereo else "sam_mono"
            cen = Census(census, force, 64)
            d = ca.CSamDemod(R.PLL_FS["sam"])
            out[key] = np.concatenate([d.ProcessData(x[cuts[k]:cuts[k + 1]], stereo) for k in range(len(R.PLL_CALLS))])
            out[key + "/census"] = cen.end()
            d.close()
    if "chain" in work:
        x = chain_input()
        Cn = len(CHAIN_NAMES)
        b = ca.DemodBatch(Cn, 2048)
        b.set_input_rate(CHAIN_FS)
        for c in range(Cn):
            m, kw = chain_kw(c)
            b.set_demod(c, m, T.info(ca, **kw))
        b.commit()
        for c in range(Cn):
            b.set_freq(c, -100e3 - 1000.0 * c)
        b.set_taps(2)
        cen = Census(census, force, 1024)
        got, taps = [[] for _ in range(Cn)], [[] for _ in range(Cn)]
        for k in range(CHAIN_CALLS):
            y = b.process(x[:, k * CHAIN_CALL:(k + 1) * CHAIN_CALL])
            for c in range(Cn):
                got[c].append(y[c]); taps[c].append(b.tap(c, 2))
        out["chain/census"] = cen.end()
        out["chain/rates"] = np.array([b.output_rate(c) for c in range(Cn)])
        for c in range(Cn):
            out["chain/%d" % c] = np.concatenate(got[c])
            out["chain/%d/tap" % c] = np.concatenate(taps[c])
            out["chain/%d/calls" % c] = np.array([len(v) for v in got[c]])
        b.close()
    np.savez(out_path, **out)
    print("config written: %d arrays" % len(out))


def child(lib_path, waves, census, force, work, out_path):
    env = dict(os.environ)
    for k in ("CSDR_LIB_PATH", "CSDR_POSTCHAIN_WAVES", "CSDR_PLL_OVERLAP", "CSDR_PC_LEAN", "CSDR_AGC_PRE", "CSDR_FM_DEFER", "CSDR_SM_CALL"):
        env.pop(k, None)
    if lib_path:
        env["CSDR_LIB_PATH"] = lib_path
    if waves == 1:
        env["CSDR_POSTCHAIN_WAVES"] = "1"
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_pc_paths_gpu as t; t.run_config(%r, %r, %d, %r)"
            % (ROOT, HERE, out_path, census, force, tuple(work)))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (lib_path, waves, force, r.stdout[-2000:] + r.stderr[-3000:])
    assert "config written" in r.stdout, r.stdout[-2000:]
    with np.load(out_path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(library, waves, force name): arrays}: the product library unforced and the census build under every force word, at
    four waves per channel and at one; every configuration in a fresh interpreter, one after the other (the first that fails
    ends the fixture: nothing starts after a child that died)"""
    from cutesdr_amd import _build
    path = _build.alt_path(_build.PCCENSUS[0])
    if not os.path.exists(path):
        assert _build.alt_lib(*_build.PCCENSUS) == path
    d = tmp_path_factory.mktemp("pcpaths")
    out = {}
    for waves in (4, 1):
        out[("product", waves, "none")] = child(None, waves, False, 0, FORCES["none"][1], str(d / ("product_%d.npz" % waves)))
        for name, (force, work) in FORCES.items():
            out[("census", waves, name)] = child(path, waves, True, force, work, str(d / ("census_%d_%s.npz" % (waves, name))))
    return out


# ---- what the parent knows ---------------------------------------------------------------------------------------------------
_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def leaf_records(arrays, key):
    head, recs = R.decode(arrays[key + "/census"])
    assert head["records"] == len(recs) <= head["capacity"], head
    assert [r["ordinal"] for r in recs] == list(range(len(recs)))
    return head, recs


def chain_records(arrays):
    """{receiver: its tiles' records in stream order}"""
    head, recs = R.decode(arrays["chain/census"])
    assert head["records"] == len(recs) <= head["capacity"], head
    per = {}
    for r in sorted(recs, key=lambda r: (r["walk"], r["ordinal"])):
        if r["n"]:
            per.setdefault(r["row"], []).append(r)
    return head, per


def agc_model(name):
    return once(("agc", name), lambda: R.agc_stream(R.agc_params(name), R.agc_input(name), R.AGC_CALLS)[1])


def chain_agc_model(arrays, c):
    """the model on what the GPU's filter handed receiver c's AGC (stage tap 2), in bursts of 1024"""
    def make():
        base = dict(AgcSlope=0, AgcThresh=-100, AgcDecay=200, AgcHangOn=0)       # test_postchain_gpu.info's defaults
        base.update(chain_kw(c)[1])
        p = R.AgcParams(base["AgcHangOn"], base["AgcThresh"], base["AgcSlope"], base["AgcDecay"], float(arrays["chain/rates"][c]))
        calls = [int(v) for v in arrays["chain/%d/calls" % c]]
        assert len(arrays["chain/%d/tap" % c]) == sum(calls)
        return R.agc_stream(p, arrays["chain/%d/tap" % c], calls, burst=1024)[1]
    return once(("chainagc", c), make)          # (the filter in front of K4 is the same in every configuration)


def check_agc_census(recs, model, limit, nw, what):
    """every decided tile's record is the model's prediction; returns (scanned, walked, first-ok-second-failed, undecided)"""
    assert len(recs) == len(model), (what, len(recs), len(model))
    scanned = walked = second = undecided = 0
    for k, (rec, (ra, rd, margin)) in enumerate(zip(recs, model)):
        if margin < R.TIE:
            undecided += 1
            continue
        path, rounds, failed = R.agc_path(ra, rd, limit, nw)
        assert rec["agc"] == path and rec["failed"] == failed, (what, k, rec, (ra, rd), limit)
        if path == "scan":
            scanned += 1
            assert (rec["rounds"] == rounds) if nw == 4 else ((rec["rounds"], rec["rounds2"]) == rounds), (what, k, rec, (ra, rd))
        else:
            walked += 1
            second += failed == 2
            if failed == 2:
                assert rec["rounds"] == ra, (what, k, rec, ra)
    assert undecided <= R.UNDECIDED_CAP * len(recs) + 1e-9, (what, undecided, len(recs))
    return scanned, walked, second, undecided


def leaf_reference(oracle, key):
    """the oracle's output of a leaf stream (and FM's squelch decisions): computed once, read-only"""
    def make():
        if key.startswith("agc/"):
            name = key[4:]
            fs, hang, thresh, slope, decay, seed = R.AGC_CASES[name]
            x = R.agc_input(name)
            r = oracle.CAgc()
            r.SetParameters(True, hang, thresh, 30, slope, decay, fs)
            y = np.concatenate([r.ProcessData(x[a:a + m]) for a, m in zip(np.cumsum([0] + R.AGC_CALLS[:-1]), R.AGC_CALLS)])
            return y, None
        kind = "fm" if key == "fm" else "sam"
        x, _ = R.pll_tile_expectations(kind)
        cuts = np.cumsum([0] + R.PLL_CALLS)
        ys, sq = [], []
        r = oracle.CFmDemod(R.PLL_FS[kind]) if kind == "fm" else oracle.CSamDemod(R.PLL_FS[kind])
        if kind == "fm":
            r.SetSquelch(50)
        for k in range(len(R.PLL_CALLS)):
            part = x[cuts[k]:cuts[k + 1]]
            ys.append(r.ProcessData(part, 5000.0, False) if kind == "fm" else r.ProcessData(part, key == "sam_stereo"))
            if kind == "fm":
                sq.append(int(r.squelched()))
        return np.concatenate(ys), np.array(sq)
    y, sq = once(("ref", key), make)
    y.setflags(write=False)
    return y, sq


def check_leaf_against_oracle(oracle, arrays, key, what):
    """the existing leaf bound, 2e-5 of full scale: AGC from the first sample; a PLL on every tile but the noise segment's and
    the first PLL_SETTLE tiles behind the two jumps that follow an unlocked stretch (below); FM's squelch decisions identical"""
    want, sq = leaf_reference(oracle, key)
    got = arrays[key]
    assert got.shape == want.shape, (what, key)
    if key.startswith("agc/"):
        err = np.abs(got - want).max()
        print("%s %s: max err %.3g of full scale" % (what, key, err / FULL_SCALE))
        assert err <= STEADY, (what, key, err / FULL_SCALE)
        return
    kind = "fm" if key == "fm" else "sam"
    x, tiles = R.pll_tile_expectations(kind)
    if kind == "fm":
        assert (arrays["fm/squelched"] == sq).all(), (what, arrays["fm/squelched"], sq)
    seg_len = 6 * R.PT
    worst, checked, per_tile = 0.0, 0, []
    for start, n, seg, since in tiles:
        err = np.abs(got[start:start + n] - want[start:start + n]).max()
        per_tile.append("%.0e" % (err / FULL_SCALE))
        # Deterministic from the first sample, acquisition included: the carrier from the reset state, the exact zeros behind it
        # (the reference's signed-zero law, pll_zero_err) and the carrier behind those -- every tile that ends in front of the
        # fourth segment, the ones that straddle two segments too.  The carrier outside the clamp and the carrier behind the
        # noise: from PLL_SETTLE tiles behind the jump, as in tests/test_postchain_gpu.py.  The noise segment, and the tiles
        # straddling it, are left out: an unlocked loop on noise is chaotic against an fp64 run.
        early = start + n <= 3 * seg_len
        settled = seg in ("scan", "never_scan") and start // seg_len in (3, 5) and since >= R.PLL_SETTLE[kind]
        if early or settled:
            worst = max(worst, err)
            checked += 1
    print("%s %s: max err %.3g of full scale on %d tiles; per tile %s" % (what, key, worst / FULL_SCALE, checked, " ".join(per_tile)))
    assert checked >= 24 and worst <= STEADY, (what, key, worst / FULL_SCALE)


def chain_reference(oracle):
    """every receiver's oracle CDemodulator over both calls: [receiver] -> audio of all calls; computed once"""
    def make():
        import test_postchain_gpu as T
        x = chain_input()
        rows = []
        for c in range(len(CHAIN_NAMES)):
            m, kw = chain_kw(c)
            r = oracle.CDemodulator(2048)
            r.SetInputSampleRate(CHAIN_FS); r.SetDemod(m, T.info(oracle, **kw)); r.SetDemodFreq(-100e3 - 1000.0 * c)
            rows.append(np.concatenate([r.process_append(x[c, k * CHAIN_CALL:(k + 1) * CHAIN_CALL].astype(np.complex128))
                                        for k in range(CHAIN_CALLS)]))
        return rows
    return once("chainref", make)


def chain_loop_reference(oracle, arrays):
    """the stages behind the filter as oracle objects on what the GPU's filter handed them (stage tap 2), burst by burst -- the
    loop-only check of tests/test_randomized_gpu.py::test_batch_chain_random_receivers; computed once (the filter in front of
    K4 is the same in every configuration)"""
    def make():
        from test_chain_taps_gpu import _oracle_post_chain
        rows = []
        for c, name in enumerate(CHAIN_NAMES):
            post = _oracle_post_chain(oracle, name, False, float(arrays["chain/rates"][c]), chain_kw(c)[1])
            tap = arrays["chain/%d/tap" % c]                 # (burst by burst, as CDemodulator hands them on: FM's squelch is per burst)
            rows.append(np.concatenate([post(tap[k:k + 1024])[1] for k in range(0, len(tap), 1024)]))
        return rows
    return once("chainloop", make)


def check_chain_against_oracle(oracle, arrays, what):
    """The whole chain against the oracle CDemodulator under check_chain_bursts, every burst of the stream from the first.  In
    the few bursts where the oracle chain ITSELF moves by more than half the steady bound when its filter output is disturbed like
    an fp32 filter's (pc_paths_ref.CHAIN_STEP_SPREAD, reproduced on the host: level steps in front of an AGC), the bound is
    twice that spread, as tests/startup_bounds.py derives the start-up bounds; everywhere else the rule is whole.  In addition K4
    on its own filter output against the oracle's stages, every burst from the first, at the bounds that check has (2e-5 of full
    scale, FM 3e-5): there the filter's rounding is on both sides, and no burst is special."""
    import test_postchain_gpu as T
    import startup_bounds as SB
    ref, loop = chain_reference(oracle), chain_loop_reference(oracle, arrays)
    for c, name in enumerate(CHAIN_NAMES):
        got = arrays["chain/%d" % c]
        calls = [int(v) for v in arrays["chain/%d/calls" % c]]
        assert len(got) == len(ref[c]) == len(loop[c]) and min(calls) >= 4 * 1024, (what, c, name, len(got), len(ref[c]), calls)
        own = T.burst_errors(got, loop[c])
        errs = T.burst_errors(got, ref[c])
        print("%s chain %d %s: on its own filter output %.3g of full scale; end to end per burst %s"
              % (what, c, name, own.max() / FULL_SCALE, " ".join("%.1e" % (v / FULL_SCALE) for v in errs)))
        assert (own <= (3e-5 if name == "FM" else 2e-5) * FULL_SCALE).all(), (what, c, name, own[:8] / FULL_SCALE)
        ruled = errs.copy()
        for b, spread in R.CHAIN_STEP_SPREAD.get(name, {}).items():
            assert errs[b] <= SB.FACTOR * spread * FULL_SCALE, (what, c, name, b, errs[b] / FULL_SCALE)
            ruled[b] = 0.0
        T.check_chain_bursts(ruled, name if name in ("FM", "SAM") else "other", 0, (what, c, name))


def tally(recs, field):
    h = {}
    for r in recs:
        h[r[field]] = h.get(r[field], 0) + 1
    return h


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [4, 1])
def test_the_census_build_unforced_is_the_product_byte_for_byte(runs, waves):
    a, b = runs[("product", waves, "none")], runs[("census", waves, "none")]
    keys = sorted(k for k in a if not k.endswith("/census"))
    assert keys == sorted(k for k in b if not k.endswith("/census")) and len(keys) >= 8 + 3 * len(CHAIN_NAMES)
    differ = [k for k in keys if a[k].tobytes() != b[k].tobytes()]
    print("%d arrays, %d bytes; differing: %s" % (len(keys), sum(a[k].nbytes for k in keys), differ))
    assert not differ
    assert all(np.abs(a[k]).max() > 0 for k in keys if not k.endswith("squelched"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [4, 1])
def test_unforced_census_is_the_models_prediction(runs, waves):
    arrays = runs[("census", waves, "none")]
    for name in R.AGC_HISTOGRAMS:
        head, recs = leaf_records(arrays, "agc/" + name)
        assert (head["nw"], head["lean"]) == (waves, False) and all((r["nw"], r["lean"]) == (waves, False) for r in recs)
        assert [r["n"] for r in recs] == [n for _, n in R.cut_tiles(R.AGC_CALLS)]
        s, w, _, u = check_agc_census(recs, agc_model(name), R.AGC_ROUNDS, waves, (waves, name))
        assert w == 0 and all(r["pll"] == "none" for r in recs)
        if waves == 4:
            assert tally([r for r, m in zip(recs, agc_model(name)) if m[2] >= R.TIE], "rounds") == \
                R.histogram([max(a, d) for a, d, m in agc_model(name) if m >= R.TIE]), name
    _, recs = leaf_records(arrays, "agc/hang62k5")
    assert len(recs) == 24 and all(r["agc"] == "walk_hang" for r in recs)
    for key, kind in (("fm", "fm"), ("sam_mono", "sam"), ("sam_stereo", "sam")):
        _, recs = leaf_records(arrays, key)
        _, tiles = R.pll_tile_expectations(kind)
        assert [r["n"] for r in recs] == [n for _, n, _, _ in tiles]
        for r, (start, n, seg, since) in zip(recs, tiles):
            assert r["agc"] == "off" and r["mode"] == (2 if kind == "fm" else 1) and not r["scan_skipped"] and not r["overlap_forced"]
            if seg == "scan" and since >= R.PLL_SETTLE[kind]:
                assert r["pll"] == "scan" and not r["zero_code"] and not r["scan_bad"], (key, start, r)
            elif seg == "never_scan" and n >= 256:          # (a tile of 1 or 37 samples may well keep the guess: no slip in it)
                assert r["pll"] in (("overlap", "walk") if kind == "fm" else ("walk",)) and r["scan_bad"] and not r["zero_code"], (key, start, r)
            elif seg == "zero":
                assert r["pll"] != "scan" and r["zero_code"], (key, start, r)
        print(waves, key, "paths:", tally(recs, "pll"))
    head, per = chain_records(arrays)
    assert sorted(per) == list(range(len(CHAIN_NAMES)))
    for c, name in enumerate(CHAIN_NAMES):
        recs = per[c]
        assert all((r["nw"], r["lean"]) == (waves, waves == 4) for r in recs), (c, name, recs[0])
        assert len(recs) == int(arrays["chain/%d/calls" % c].sum()) // 1024 and all(r["n"] == 1024 for r in recs)
        assert all(r["mode"] == chain_kw(c)[0] for r in recs)
        if name == "USB":
            assert all(r["agc"] == "walk_hang" for r in recs)
        else:
            s, w, _, u = check_agc_census(recs, chain_agc_model(arrays, c), R.AGC_ROUNDS, waves, (waves, "chain", c, name))
            assert w == 0
        assert all((r["pll"] != "none") == (name in ("FM", "SAM")) for r in recs)
        print(waves, "chain", c, name, "agc", tally(recs, "agc"), "rounds", tally(recs, "rounds"), "pll", tally(recs, "pll"))


# ---- 3 and 4 ------------------------------------------------------------------------------------------------------------------
def compare_with_unforced(runs, waves, name, keys):
    """test 4: a forced run against the unforced one, same library, same input; returns {key: max difference / full scale}"""
    a, b = runs[("census", waves, name)], runs[("census", waves, "none")]
    worst = {}
    for k in keys:
        assert a[k].shape == b[k].shape, k
        worst[k] = float(np.abs(a[k] - b[k]).max()) / FULL_SCALE
    print("waves %d, %s against unforced, max difference / full scale: %s" % (waves, name, json.dumps(worst)))
    if "fm/squelched" in a:
        assert (a["fm/squelched"] == b["fm/squelched"]).all()
    assert all(v <= PATHS_AGREE / FULL_SCALE for v in worst.values()), worst
    return worst


@pytest.mark.parametrize("waves", [4, 1])
@pytest.mark.parametrize("name", ["agc0", "agc1", "agc2"])
def test_forced_agc_round_limits(oracle, runs, waves, name):
    arrays, limit = runs[("census", waves, name)], AGC_LIMIT[name]
    total = np.zeros(3, dtype=int)
    for case in R.AGC_HISTOGRAMS:
        _, recs = leaf_records(arrays, "agc/" + case)
        assert all((r["nw"], r["lean"]) == (waves, False) for r in recs)
        s, w, second, _ = check_agc_census(recs, agc_model(case), limit, waves, (waves, name, case))
        print(waves, name, case, "scanned %d walked %d (first scan ok, second failed: %d)" % (s, w, second))
        total += (s, w, second)
        check_leaf_against_oracle(oracle, arrays, "agc/" + case, (waves, name))
    _, recs = leaf_records(arrays, "agc/hang62k5")
    assert all(r["agc"] == "walk_hang" for r in recs)
    check_leaf_against_oracle(oracle, arrays, "agc/hang62k5", (waves, name))
    # both sides of the handoff, from the census (limit 0: every tile walks with the hang off)
    assert total[1] > 0 and (total[0] > 0) == (limit > 0), (name, total)
    if waves == 1 and limit > 0:
        assert total[2] > 0, (name, total)
    head, per = chain_records(arrays)
    ctotal = np.zeros(2, dtype=int)
    for c, cname in enumerate(CHAIN_NAMES):
        if cname == "USB":
            assert all(r["agc"] == "walk_hang" for r in per[c])
            continue
        assert all((r["nw"], r["lean"]) == (waves, waves == 4) for r in per[c])
        s, w, _, _ = check_agc_census(per[c], chain_agc_model(runs[("census", waves, "none")], c), limit, waves, (waves, name, "chain", c))
        ctotal += (s, w)
    print(waves, name, "chain: scanned %d walked %d" % tuple(ctotal))
    # (limit 2 on the chain: walked tiles only where the model, run on the chain's own filter output, has a third round)
    assert (ctotal[1] > 0 or limit == 2) and (ctotal[0] > 0) == (limit > 0), (name, ctotal)
    check_chain_against_oracle(oracle, arrays, (waves, name))
    compare_with_unforced(runs, waves, name, ["agc/" + c for c in R.AGC_CASES] + ["chain/%d" % c for c in range(len(CHAIN_NAMES))])


@pytest.mark.parametrize("waves", [4, 1])
def test_forced_pll_scan_skipped(oracle, runs, waves):
    """FM: every tile goes to pll_overlap (and on to pll_walk where that rejects it); SAM mono and stereo: every tile is
    walked, with the sign flip and the radians <-> turns hand-back in every tile"""
    arrays = runs[("census", waves, "skipscan")]
    _, recs = leaf_records(arrays, "fm")
    assert all(r["scan_skipped"] and r["pll"] in ("overlap", "walk") for r in recs) and tally(recs, "pll").get("overlap", 0) >= 24
    print(waves, "fm", tally(recs, "pll"))
    for key in ("sam_mono", "sam_stereo"):
        _, recs = leaf_records(arrays, key)
        assert len(recs) == 41 and all(r["scan_skipped"] and r["pll"] == "walk" for r in recs), key
    for key in ("fm", "sam_mono", "sam_stereo"):
        check_leaf_against_oracle(oracle, arrays, key, (waves, "skipscan"))
    _, per = chain_records(arrays)
    for c, name in enumerate(CHAIN_NAMES):
        want = {"FM": ("overlap", "walk"), "SAM": ("walk",)}.get(name, ("none",))
        assert all(r["pll"] in want and r["scan_skipped"] == (name in ("FM", "SAM")) for r in per[c]), (c, name, tally(per[c], "pll"))
    assert tally(per[3], "pll").get("overlap", 0) > 0
    check_chain_against_oracle(oracle, arrays, (waves, "skipscan"))
    compare_with_unforced(runs, waves, "skipscan", ["fm", "sam_mono", "sam_stereo"] + ["chain/%d" % c for c in range(len(CHAIN_NAMES))])


@pytest.mark.parametrize("waves", [4, 1])
def test_forced_pll_overlap_mismatch_on_every_third_tile(oracle, runs, waves):
    """scan -> overlap -> walk in one stream: a tile that pll_scan gives up AND whose ordinal is 1 mod 3 is rejected by
    pll_overlap and walked by one thread -- also directly behind a zero-code tile, and a zero-code tile itself"""
    arrays = runs[("census", waves, "overlap3")]
    _, recs = leaf_records(arrays, "fm")
    t = tally(recs, "pll")
    print(waves, "fm", t)
    assert min(t.get("scan", 0), t.get("overlap", 0), t.get("walk", 0)) > 0, t
    for r in recs:
        if r["pll"] != "scan":
            # (unforced, pll_overlap rejects only tiles with a zero-sample code, and not all of them: a zero has no phase to
            # pull the warm-up in)
            assert r["overlap_forced"] == (r["ordinal"] % 3 == 1) and (r["pll"] == "walk") == (r["overlap_forced"] or (r["zero_code"] and r["pll"] == "walk")), r
    assert any(r["pll"] == "walk" and r["overlap_forced"] and not r["zero_code"] for r in recs)
    assert any(r["pll"] == "walk" and p["zero_code"] for p, r in zip(recs, recs[1:]))
    assert any(r["pll"] == "walk" and r["zero_code"] for r in recs)
    check_leaf_against_oracle(oracle, arrays, "fm", (waves, "overlap3"))
    _, per = chain_records(arrays)
    print(waves, "chain FM", tally(per[3], "pll"))
    assert all(r["pll"] in ("scan", "overlap", "walk") for r in per[3])
    check_chain_against_oracle(oracle, arrays, (waves, "overlap3"))
    compare_with_unforced(runs, waves, "overlap3", ["fm"] + ["chain/%d" % c for c in range(len(CHAIN_NAMES))])


@pytest.mark.parametrize("waves", [4, 1])
def test_forced_pll_scan_skipped_and_overlap_rejected_on_the_chain(oracle, runs, waves):
    """overlap accepted | overlap rejected -> pll_walk in the lean walk (four waves) and the one-wave walk of the chain, whose
    locked FM carrier reaches neither unforced: with pll_scan skipped and the mismatch on every third tile both sides run in
    one stream; with the mismatch on every tile every FM tile is walked by one thread, the stream's first ones -- zero-sample
    codes from the AGC's cleared delay line -- included"""
    for name in ("skipoverlap3", "skipwalk"):
        arrays = runs[("census", waves, name)]
        _, recs = leaf_records(arrays, "fm")
        _, per = chain_records(arrays)
        fm = per[3]
        assert all((r["nw"], r["lean"]) == (waves, waves == 4) and r["scan_skipped"] for r in fm)
        t, tl = tally(fm, "pll"), tally(recs, "pll")
        print(waves, name, "chain FM", t, "leaf FM", tl)
        if name == "skipoverlap3":
            assert set(t) == {"overlap", "walk"} and min(t.values()) >= 10, t
            assert set(tl) == {"overlap", "walk"}, tl
            for r in fm + recs:
                assert r["overlap_forced"] == (r["ordinal"] % 3 == 1) and (r["pll"] == "walk" or not r["overlap_forced"]), r
        else:
            assert set(t) == {"walk"} and set(tl) == {"walk"} and all(r["overlap_forced"] for r in fm + recs), (t, tl)
            assert fm[0]["zero_code"] and sum(r["zero_code"] for r in recs) >= 6
        for c, cname in enumerate(CHAIN_NAMES):
            if cname != "FM":
                assert all(r["pll"] == ("walk" if cname == "SAM" else "none") for r in per[c]), (c, cname)
        check_leaf_against_oracle(oracle, arrays, "fm", (waves, name))
        check_chain_against_oracle(oracle, arrays, (waves, name))
        compare_with_unforced(runs, waves, name, ["fm"] + ["chain/%d" % c for c in range(len(CHAIN_NAMES))])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def run_sweeps(out_path):
    """(in the child, census build) the randomized sweeps' own test functions, every seed, under the census"""
    from oracle import oracle as orc
    import test_randomized_gpu as Z
    orc.build()
    out = {}
    cen = Census(True, 0, 4096)
    for seed in range(12):
        Z.test_agc_random_settings_and_envelopes(orc, seed)
    out["agc"] = cen.end()
    cen = Census(True, 0, 4096)
    for seed in range(8):
        Z.test_fm_sam_random_offsets_and_levels(orc, seed)
    out["pll"] = cen.end()
    np.savez(out_path, **out)
    print("config written: %d arrays" % len(out))


def test_what_the_randomized_sweeps_reach(tmp_path):
    from cutesdr_amd import _build
    path = _build.alt_path(_build.PCCENSUS[0])
    if not os.path.exists(path):
        assert _build.alt_lib(*_build.PCCENSUS) == path
    env = dict(os.environ, CSDR_LIB_PATH=path)
    env.pop("CSDR_POSTCHAIN_WAVES", None)
    outp = str(tmp_path / "sweeps.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_pc_paths_gpu as t; t.run_sweeps(%r)" % (ROOT, HERE, outp)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "config written" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(outp) as z:
        agc, pll = R.decode(z["agc"])[1], R.decode(z["pll"])[1]
    table = {}
    for r_ in agc:
        key = "agc " + r_["agc"] + (" in %d rounds" % r_["rounds"] if r_["agc"] == "scan" else "")
        table[key] = table.get(key, 0) + 1
    for r_ in pll:
        why = "" if r_["pll"] == "scan" else " (%s)" % "+".join(w for w, on in (("check", r_["scan_bad"]), ("zero code", r_["zero_code"])) if on)
        key = "%s %s%s" % ("fm" if r_["mode"] == 2 else "sam", r_["pll"], why)
        table[key] = table.get(key, 0) + 1
    print("tiles per path, test_agc_random_settings_and_envelopes (12 seeds) and test_fm_sam_random_offsets_and_levels (8 seeds):")
    for k in sorted(table):
        print("  %-40s %d" % (k, table[k]))
    for mode in (2, 1):
        kinds = {r_["pll"] for r_ in pll if r_["mode"] == mode}
        assert "scan" in kinds and kinds - {"scan"}, (mode, kinds)
