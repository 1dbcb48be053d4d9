#!/usr/bin/env python3
"""Builds a copy of the library whose K1 (fastfir2_kernels.hip) is compiled with extra flags, for A/B runs of
kernel experiments in one GPU visit:   python tools/altlib.py NAME [unit.hip[,unit2.hip]] [-DFLAG ...]
  -> cutesdr_amd/libcutesdr_mi_NAME.so;   then   CSDR_LIB_PATH=<that> python tools/ab_fastfir.py 0,2
(cutesdr_amd/_build.py: alt_lib does the work)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cutesdr_amd import _build

name, extra = sys.argv[1], sys.argv[2:]
units = ["fastfir2_kernels"]
if extra and extra[0].endswith(".hip"):
    units, extra = [u[:-4] for u in extra[0].split(",")], extra[1:]
print(_build.alt_lib(name, extra, units=tuple(units)))
