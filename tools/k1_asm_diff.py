#!/usr/bin/env python3
"""Same instruction stream?   python tools/k1_asm_diff.py REV [--unit fastfir2_kernels.hip] [-DFLAG ...]
Compiles the unit as it is in git revision REV and as it is in the working tree to gfx950 device assembly, with the
flags cutesdr_amd/_build.py compiles it with plus the extra ones, drops the lines that carry the compilation unit's id
(__hip_cuid_*) and prints the diff: nothing and exit status 0 when the two are the same, kernel resources (VGPRs,
scratch, LDS) included.  No GPU is needed.  It names no instruction and looks for none: it is a diff."""
import difflib, io, os, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cutesdr_amd import _build

args = sys.argv[1:]
unit = "fastfir2_kernels.hip"
if "--unit" in args:
    i = args.index("--unit")
    unit = args[i + 1]
    del args[i:i + 2]
rev, extra = args[0], args[1:]


def device_asm(csrc, out):
    # (-Wall stays out: the warnings of a diagnostic flag set are not what is compared)
    flags = [f for f in _build.FLAGS if f != "-Wall"] + _build.FILE_FLAGS.get(unit, []) + ["-I", _build.OBJ] + extra
    subprocess.check_call([_build._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, unit), "-o", out])
    return [l for l in open(out) if "__hip_cuid_" not in l]


with tempfile.TemporaryDirectory() as tmp:
    tar = subprocess.check_output(["git", "-C", ROOT, "archive", rev, "cutesdr_amd/csrc", "include"])
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
    with ThreadPoolExecutor(2) as pool:
        then = pool.submit(device_asm, os.path.join(tmp, "cutesdr_amd", "csrc"), os.path.join(tmp, "then.s"))
        now = pool.submit(device_asm, _build.CSRC, os.path.join(tmp, "now.s"))
        then, now = then.result(), now.result()
diff = list(difflib.unified_diff(then, now, "%s:%s" % (rev, unit), unit, n=2))
sys.stdout.writelines(diff)
print("%s %s: %d lines of device assembly, %s" % (unit, " ".join(extra) or "(product flags)", len(now),
                                                   "DIFFERENT from %s" % rev if diff else "identical to %s" % rev),
      file=sys.stderr)
sys.exit(1 if diff else 0)
