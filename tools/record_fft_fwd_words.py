#!/usr/bin/env python3
"""Records tests/golden/fft_fwd_fp32_words.json: sha256 digests of the words csdr_fft_fwd / _rev return for a fixed integer
input at 2048 and 65536 points (tests/test_fft_plain64_gpu.py holds the one-receiver fp32 transforms to them).

Plain ctypes on the library given, so that a library of an EARLIER commit can be the source -- the point of the fixture is
that the fp32 words do not move; record it from the commit before a change, never from the change itself, and only when
the fp32 transforms are meant to change:
  python tools/record_fft_fwd_words.py path/to/libcutesdr_mi.so [out.json]
Needs a GPU.  Prints the digests; writes out.json (default: the fixture)."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2048, 65536)


def fixed_input(n):
    """integers below 2001 in both parts, the same on every machine"""
    i = np.arange(n, dtype=np.int64)
    return (((i * 7919) % 4001 - 2000) + 1j * ((i * 104729) % 3989 - 1994)).astype(np.complex128)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint64).tobytes()).hexdigest()


def record(lib_path):
    L = C.CDLL(lib_path)
    L.csdr_fft_create.restype = C.c_void_p
    L.csdr_fft_create.argtypes = [C.c_int]
    L.csdr_fft_set_params.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
    L.csdr_fft_destroy.argtypes = [C.c_void_p]
    for fn in (L.csdr_fft_fwd, L.csdr_fft_rev):
        fn.argtypes = [C.c_void_p, C.c_void_p]
        fn.restype = C.c_int
    out = {}
    for n in SIZES:
        f = L.csdr_fft_create(0)
        if not f or L.csdr_fft_set_params(f, n, 0, 0.0, 48000.0) != 0:
            raise RuntimeError("csdr_fft_create / set_params failed (no GPU?)")
        for name, fn in (("fwd", L.csdr_fft_fwd), ("rev", L.csdr_fft_rev)):
            a = fixed_input(n)
            if fn(f, a.ctypes.data) != 0:
                raise RuntimeError("csdr_fft_%s failed" % name)
            out["%s_%d" % (name, n)] = digest(a)
        L.csdr_fft_destroy(f)
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    res = record(os.path.abspath(sys.argv[1]))
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "fft_fwd_fp32_words.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))
