"""vm_set_option("border_fuse"): 0, 1 and 2 are accepted, the values next to them rejected with the key named.  CPU
only; the options are process-global, so the calls run in a child interpreter (as tests/test_options.py)."""

import os
import subprocess
import sys

from conftest import REPO

LIB = os.path.join(REPO, "video-matting_amd", "vmatting", "libvmatting.so")

CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.vm_set_option.restype = ctypes.c_int
lib.vm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_long]
lib.vm_last_error.restype = ctypes.c_char_p
lib.vm_conv3x3_last_border_fused.restype = ctypes.c_int
bad = []
for v in (0, 1, 2):
    if lib.vm_set_option(b"border_fuse", v) != 0:
        bad.append("border_fuse=%d rejected: %s" % (v, lib.vm_last_error().decode()))
for v in (-1, 3, 1 << 40):
    if lib.vm_set_option(b"border_fuse", v) != -1 or "border_fuse" not in lib.vm_last_error().decode():
        bad.append("border_fuse=%d: expected VM_EINVAL naming the key" % v)
if lib.vm_conv3x3_last_border_fused() != 0:
    bad.append("last_border_fused before any call")
print("\n".join(bad))
sys.exit(1 if bad else 0)
"""


def test_border_fuse_values():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    r = subprocess.run([sys.executable, "-c", CHILD, LIB], capture_output=True, text=True)
    assert r.returncode == 0, "vm_set_option:\n" + r.stdout + r.stderr
