"""The K1_TWREG = 3 build of K1 (fastfir2_kernels.hip: the pass twiddles k1 = 1, 2 and 3 of F2 / I2 stay in registers)
under the parity cases of the product's build.  The product keeps all sixteen (K1_TWREG = 16, the default, timed against
this build and against 0: HISTORY.md); 3 is the build in which some pass twiddles come from registers and the rest from
LDS in the same pass, the path the default no longer takes."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu


def test_real_gain_cases_on_the_k1_twreg_3_build():
    """cutesdr_amd/libcutesdr_mi_twreg3.so (built here when __graft_entry__.build() has not: a missing compiler is an
    error) in one fresh interpreter through tests/test_fastfir_realgain_gpu.py, which asserts the kernel of every launch
    and, told by CSDR_EXPECT_K1_TWREG, that the library it loaded was compiled with K1_TWREG = 3"""
    from cutesdr_amd import _build
    name, flags = _build.TWREG3
    path = _build.alt_path(name)
    if not os.path.exists(path):
        assert _build.alt_lib(name, flags) == path
    env = dict(os.environ, CSDR_LIB_PATH=path, CSDR_EXPECT_K1_TWREG="3")
    here = os.path.dirname(__file__)
    code = ("import sys; sys.path.insert(0, %r); import pytest; "
            "sys.exit(pytest.main(['-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider', %r]))"
            % (here, os.path.join(here, "test_fastfir_realgain_gpu.py")))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" not in r.stdout, r.stdout[-2000:]
