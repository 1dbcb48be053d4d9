"""The library reports how its 16384-point overlap-save kernels talk to HBM (fastfir2_kernels.hip: K1_RUNEND, K1_PROLOGUE,
K1_TW2LDS, K1_LDSPREAD; no GPU): the product ships the first and the last, the copies tests/test_fastfir_runend_gpu.py holds
it against, word for word, none and all four.  Bit 0: no fetch behind a run's last block and the history tail stored inside the
call's last block; bit 1: one round trip in front of the block loop; bit 2: the real-gain kernel keeps no twiddle table in LDS
-- and is launched with 8 KiB less of it; bit 3: a block's loads in four pairs."""
import ctypes as C

LDS_DATA = (16384 + 2 * (16384 // 32)) * 8        # the padded image of one block, bytes
TABLE = 32 * 32 * 8                               # the 32 x 32 pass twiddles


def report(path):
    L = C.CDLL(path)
    L.csdr__host_fastfir2_hbm_knobs.restype = C.c_int
    L.csdr__host_fastfir2_gain_lds_bytes.restype = C.c_int
    return L.csdr__host_fastfir2_hbm_knobs(), L.csdr__host_fastfir2_gain_lds_bytes()


def test_the_product_reports_its_hbm_knobs():
    from cutesdr_amd import _build
    knobs, lds = report(_build.build())
    assert knobs == 1 | 8, knobs
    assert lds == LDS_DATA + TABLE


def test_the_knobs_off_copy_reports_none():
    from cutesdr_amd import _build
    knobs, lds = report(_build.alt_lib(*_build.RUNEND0))
    assert knobs == 0
    assert lds == LDS_DATA + TABLE


def test_the_knobs_on_copy_reports_all_four():
    from cutesdr_amd import _build
    knobs, lds = report(_build.alt_lib(*_build.HBMALL))
    assert knobs == 15
    assert lds == LDS_DATA
