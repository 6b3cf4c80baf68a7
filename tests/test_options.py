"""vm_set_option, key by key: every key's accepted values, its nearest rejected values (VM_EINVAL, the key named in
vm_last_error()), unknown / NULL / study-only keys.  CPU only: the library loads and validates without a GPU.  The
options are process-global, so the calls run in a child interpreter.  The key lists are written out by hand on
purpose: a key that the library drops fails here."""

import os
import subprocess
import sys

from conftest import REPO

LIB = os.path.join(REPO, "video-matting_amd", "vmatting", "libvmatting.so")

# key -> closed range [lo, hi]
RANGES = {
    "conv_kernel": (0, 3),
    "softmax_kernel": (0, 6),
    "softmax_blocks": (1, 1 << 20),
    "softmax_f32p": (0, 7),
    "cband": (0, 2),
    "ngroup": (0, 64),
    "thin_rounds": (0, 64),
    "pack_frames": (0, 1),
    "up_skip": (0, 1),
    "src_span_limit": (1, 0x7ffffff0),
    "conv_prio": (0, 1),
    "thin_twalk": (0, 1),
    "thin_rowreuse": (0, 1),
    "thin_dma": (0, 4),
    "thin_dma_rounds": (1, 64),
    "narrowin_kernel": (0, 1),
    "thin_kernel": (0, 1),
    "pair_xin_wide": (0, 1),
    "patch_repi": (0, 1),
    "persist_rounds": (0, 64),
    "persist_up_rounds": (0, 64),
    "persist_all": (0, 2),
    "persist_rot": (0, 2),
    "up_skip_mask": (0, 3),
    "patch_persist": (0, 1),
    "pair_strip_pin": (0, 1),
    "pair_strip": (0, 1),
    "pair_kernel": (0, 1),  # the shipped build (the study build adds 10..18)
    "head_kernel": (0, 2),
    "bn_blocks": (1, 8192),
}

# key -> the only accepted values
SETS = {
    "rows_kernel": (0, 1, 8, 16),
    "thin_th": (4, 8, 16),
    "border_ks": (1, 2, 4),
    "glds_rb": (64, 128),
    "head_th": (8, 16),
    "patch_cfg": (0, 19, 22, 25, 30),  # the shipped build (the study build takes 0..31)
}

# keys that take any value
FREE = (
    "cband_bytes", "pack_tiled", "persist_half", "rows_up", "rows_min_cin", "rows_min_blocks", "thin_blocks",
    "conv_min_tiles", "splitk_tiles", "bn_vec_fwd",
    "wgrad_reduce4", "wgrad_variant", "wgrad_taps", "wgrad_dma", "bn_vec", "relu_bias_vec", "resize_bwd_2x",
    "relu_bias_iters", "wgrad_mfma_pipe", "wgrad_wide_pipe", "wgrad_wide_target", "wgrad_wide_cs", "wgrad_wide_dbuf",
    "wgrad_dma_cfg",
)

# keys of the study build only (make study): unknown to the shipped library
STUDY_ONLY = ("patch_ablate", "softmax_abl", "patch_rowslot", "pair_strip_abl")

CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.vm_set_option.restype = ctypes.c_int
lib.vm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_long]
lib.vm_last_error.restype = ctypes.c_char_p
RANGES, SETS, FREE, STUDY_ONLY = eval(sys.argv[2])
VM_OK, VM_EINVAL = 0, -1
bad = []

def accept(key, v):
    rc = lib.vm_set_option(key.encode(), v)
    if rc != VM_OK:
        bad.append("%s=%d: rc %d (%s), expected VM_OK" % (key, v, rc, lib.vm_last_error().decode()))

def reject(key, v):
    rc = lib.vm_set_option(key.encode() if key is not None else None, v)
    msg = lib.vm_last_error().decode()
    if rc != VM_EINVAL:
        bad.append("%s=%d: rc %d, expected VM_EINVAL" % (key, v, rc))
    elif key is not None and key not in msg:
        bad.append("%s=%d: the message does not name the key: %r" % (key, v, msg))

for key, (lo, hi) in RANGES.items():
    accept(key, lo)
    accept(key, hi)
    accept(key, (lo + hi) // 2)
    reject(key, lo - 1)
    reject(key, hi + 1)
    reject(key, -(1 << 40))
    reject(key, 1 << 40)
for key, vals in SETS.items():
    for v in vals:
        accept(key, v)
    for v in vals:
        for w in (v - 1, v + 1):
            if w not in vals:
                reject(key, w)
    reject(key, -(1 << 40))
    reject(key, 1 << 40)
for key in FREE:
    for v in (0, 1, -1, 7, 123456789012, -(1 << 40)):
        accept(key, v)
for key in STUDY_ONLY:
    reject(key, 0)
    reject(key, 1)
reject("no_such_option", 0)
reject("", 0)
reject("conv_kerne", 0)
reject("conv_kernel_", 0)
reject(None, 0)
print("\n".join(bad))
sys.exit(1 if bad else 0)
"""


def test_key_lists_are_disjoint():
    keys = list(RANGES) + list(SETS) + list(FREE) + list(STUDY_ONLY)
    assert len(keys) == len(set(keys)) == 30 + 6 + 24 + 4


def test_every_option_key_and_its_bounds():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    tables = repr((RANGES, SETS, FREE, STUDY_ONLY))
    r = subprocess.run([sys.executable, "-c", CHILD, LIB, tables], capture_output=True, text=True)
    assert r.returncode == 0, "vm_set_option:\n" + r.stdout + r.stderr
