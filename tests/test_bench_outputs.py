"""bench.py's plain run and --dump-outputs.  A plain run (no --full) times the steps it is asked for and prints the
result line with nothing of the secondary measurements; --dump-outputs writes what the last timed step computed, a
seeded sample of channels under a fixed byte budget, the same channels from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _json_lines(text):
    return [json.loads(l) for l in text.splitlines() if l.startswith("{")]


def test_dump_stays_under_the_budget_and_samples_the_same_channels(tmp_path):
    big = torch.arange(64 * (1 << 19) * 2, dtype=torch.float32).reshape(64, 1 << 19, 2)     # 256 MB
    small = torch.arange(6 * 10, dtype=torch.float64).reshape(6, 10)
    got = bench.dump_outputs(torch, str(tmp_path / "a"), {"big": big, "small": small})
    again = bench.dump_outputs(torch, str(tmp_path / "b"), {"big": big, "small": small})
    assert got == again
    total = 0
    for name in ("big", "small"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_BYTES <= 64 << 20
    assert got["big"]["shape"][1:] == [1 << 19, 2] and got["big"]["shape"][0] < 64
    rows = (np.load(tmp_path / "a" / "big.npy")[:, 0, 0] // (1 << 20)).astype(int)     # which channels were written
    assert list(rows) == sorted(set(rows)) and len(rows) == got["big"]["shape"][0]
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy().astype(np.float32))   # small: whole


def test_stub_accepts_full_and_times_the_steps_asked_for():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    for extra in ([], ["--full"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--steps", "5", "--warmup", "1"] + extra,
                           capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        line = _json_lines(r.stdout)[0]
        assert line["steps"] == 5 and line["ms_per_step"] >= 2.0          # the stub's step sleeps 2 ms


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_output(tmp_path):
    from oracle import oracle as orc
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line
    assert line["cpu_baseline"] is None
    for k in ("parity_checked", "chain_c4", "fastfir_sizes", "distinct_filters", "host_form"):
        assert k not in line
    y = np.load(out / "fastfir_out.npy")
    assert y.dtype == np.float32 and y.nbytes <= 64 << 20
    C, T = bench.CHANNELS, bench.T_PER_CH
    assert y.shape[1:] == (T, 2) and line["outputs_dumped"]["fastfir_out"]["shape"] == list(y.shape)
    chans = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(C, y.shape[0], replace=False))
    # the input of the first sampled channel, as C3Workload makes it; the stream is periodic, so the last step's output
    # is the oracle's second pass over the same samples
    g = torch.Generator(device="cuda")
    g.manual_seed(0xC0DE0000)
    x = torch.randn((C, T, 2), generator=g, device="cuda", dtype=torch.float32) * 3276.7
    xc = x[int(chans[0])].cpu().numpy().astype(np.float64)
    del x
    xc = xc[:, 0] + 1j * xc[:, 1]
    ff = orc.CFastFIR(bench.FFT_N)
    ff.SetupParameters(-5000, 5000, 0, bench.FS)
    ff.ProcessData(xc)
    ref = ff.ProcessData(xc)
    got = y[0].astype(np.float64)
    assert np.abs((got[:, 0] + 1j * got[:, 1]) - ref).max() <= 2e-5 * np.abs(xc).max()
