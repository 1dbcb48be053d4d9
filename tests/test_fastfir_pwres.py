"""The product library keeps the outer-pass twiddle powers of the 16384-point real-gain overlap-save kernel in registers for
the whole run (fastfir2_kernels.hip: K1_PWRES, K1Cfg::PW_RESIDENT; no GPU).  What the resident build computes is held word
for word against the K1_PWRES = 0 build in tests/test_fastfir_pwres_gpu.py."""
import ctypes as C


def test_the_product_keeps_the_outer_powers_resident():
    from cutesdr_amd import _build, _capi
    _build.build()
    L = _capi.lib()
    L.csdr__host_fastfir2_pwres.restype = C.c_int
    assert L.csdr__host_fastfir2_pwres() == 1
