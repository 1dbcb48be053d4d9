"""CPU tests of the row form of the display stream (no GPU): display_rows_plan -- one plan per row over the shared frame
position, split into the gathered and the loaded launch -- against the literal transcription of ProcessIQData's display
loop (RefDisplayLoop, one per row), and the no-GPU failure of the row form's entry points."""
import ctypes as C
import numpy as np
import pytest
from test_display_stream_host import RefDisplayLoop


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_display_rows_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int,
                                                 C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.csdr__host_display_rows_plan.restype = None
    return lib


def rows_plan(L, states, ave, pos, n, N, loaders, first_loaded=0, sorted_=False):
    """-> (next states [R, 4], counts [R], gathered entries, loaded entries, split); an entry is (row, nframes, ave,
    start, step)"""
    R = len(states)
    st = np.ascontiguousarray(states, dtype=np.int32).copy()
    av = np.ascontiguousarray(ave, dtype=np.int32)
    counts = np.full(R, -7, dtype=np.int32)
    g = np.zeros((R, 6), dtype=np.int64); l = np.zeros((R, 6), dtype=np.int64)
    split = np.zeros(6, dtype=np.int32)
    L.csdr__host_display_rows_plan(st.ctypes.data, av.ctypes.data, R, pos, n, N, int(loaders), first_loaded, int(sorted_),
                                   counts.ctypes.data, g.ctypes.data, l.ctypes.data, split.ctypes.data)
    ng, nl = int(split[0]), int(split[1])
    return st, counts, [tuple(int(v) for v in e[:5]) for e in g[:ng]], [tuple(int(v) for v in e[:5]) for e in l[:nl]], split


@pytest.mark.parametrize("N", [8, 128])
@pytest.mark.parametrize("loaders", [False, True])
def test_rows_plan_matches_reference_loop_per_row(L, N, loaders):
    skips = [0, 1, 2, 7, 48, 0, 1, 2, 7, 48]
    gated = [0] * 5 + [1] * 5
    ave = [1 + r for r in range(10)]
    R = len(skips)
    rng = np.random.default_rng(77 * N + loaders)
    refs = [RefDisplayLoop(N, skips[r], bool(gated[r])) for r in range(R)]
    states = np.array([[skips[r], 0, gated[r], 1] for r in range(R)], dtype=np.int32)
    pos, pos_abs = 0, 0
    for call in range(300):
        for r in range(R):                                     # each listener acknowledges at its own times
            if gated[r] and rng.random() < 0.3:
                refs[r].finished = True
                states[r, 3] = 1
        rem = N - pos
        n = int(rng.choice([rng.integers(1, max(rem, 2)), rng.integers(1, 3 * N + 1), rem, 0, rng.integers(1, 60 * N)]))
        want = [ref.process(n) for ref in refs]
        nxt, counts, gath, load, split = rows_plan(L, states, ave, pos, n, N, loaders, sorted_=(call % 2 == 1))
        got = [[] for _ in range(R)]
        for table in (gath, load):                             # launch order: the gathered frames, then the loaded ones
            seen = set()
            for row, nframes, av, start, step in table:
                assert nframes >= 1, "a row without a frame is in no table"
                assert row not in seen and av == ave[row]
                seen.add(row)
                assert step % N == 0 and start >= -pos and start + (nframes - 1) * step + N <= n
                got[row] += [pos_abs + start + k * step for k in range(nframes)]
        for row, nframes, av, start, step in load:
            assert loaders and start >= 0                      # the loaders read the call's samples only
        if loaders:
            for row, nframes, av, start, step in gath:
                assert nframes == 1 and start < 0              # only the frame that begins in the carry
        assert got == want, (call, n)
        assert [len(w) for w in want] == list(counts)
        assert split[4] == max(counts) and split[0] == len(gath) and split[1] == len(load)
        assert split[2] == max([e[1] for e in gath], default=0) and split[3] == max([e[1] for e in load], default=0)
        if call % 2 == 1:
            for table in (gath, load):
                assert [e[1] for e in table] == sorted([e[1] for e in table], reverse=True)
        pos_abs += n
        pos = int(split[5])
        states = nxt
        for r in range(R):
            assert pos * 2 == refs[r].fft_buf_pos
            assert states[r, 1] == refs[r].counter
            assert bool(states[r, 3]) == refs[r].finished
            assert states[r, 0] == skips[r] and states[r, 2] == gated[r]


def test_rows_plan_first_loaded_moves_frames_to_the_gather(L):
    """frames whose first sample lies in front of first_loaded are gathered, the rest loaded, in order"""
    N = 64
    st, counts, gath, load, split = rows_plan(L, [[1, 0, 0, 1], [3, 0, 0, 1], [0, 0, 1, 0]], [2, 5, 1], 0, 10 * N, N, True,
                                              first_loaded=70)
    assert list(counts) == [10, 3, 0]
    assert gath == [(0, 2, 2, 0, N)]                            # row 1's first frame starts at 2 N >= 70: all loaded
    assert load == [(0, 8, 2, 2 * N, N), (1, 3, 5, 2 * N, 3 * N)]
    frames = {0: [], 1: []}
    for table in (gath, load):
        for row, nframes, av, start, step in table:
            frames[row] += [start + k * step for k in range(nframes)]
    assert frames[0] == [k * N for k in range(10)] and frames[1] == [2 * N, 5 * N, 8 * N]
    assert all(s >= 70 for row, nf, av, s, step in load)
    assert all(row != 2 for row, *_ in gath + load)


def test_row_entry_points_fail_cleanly_without_gpu(L):
    from cutesdr_amd import _capi
    if L.csdr_device_count() > 0:
        pytest.skip("GPU present")
    EINVAL, EHIP = _capi.CSDR_EINVAL, _capi.CSDR_EHIP
    assert L.csdr_fft_batch_set_ave_row(None, 0, 2) == EHIP
    assert L.csdr_fft_batch_reset_row(None, 0) == EHIP
    assert L.csdr_fft_batch_set_display_rate_row(None, 0, 10, 1) == EHIP
    assert L.csdr_fft_batch_screen_update_done_row(None, -1) == EHIP
    assert L.csdr_plotter_batch_draw_emitted(None, None, None) == EHIP
    assert b"no HIP device" in L.csdr_last_error()
    out = (C.c_int * 4)()
    assert L.csdr_fft_batch_get_emits(None, out) == EINVAL      # host state only: nothing to ask the device for
    assert L.csdr_fft_batch_row_form(None) == EINVAL
