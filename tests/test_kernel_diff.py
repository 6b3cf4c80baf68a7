"""tools/kernel_diff.py, the per-kernel disassembly comparison that kernel moves between translation units are checked
with (no GPU involved): the normaliser on hand-written snippets, and the shipped library against itself."""

import os
import shutil
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "video-matting_amd", "vmatting", "libvmatting.so")
sys.path.insert(0, os.path.join(REPO, "tools"))

# one kernel as llvm-objdump -d prints it, at two load addresses; the second is followed by alignment padding
_A = """
0000000000001900 <_ZN2vm1kEPf>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001900: C0060002 00000000
	v_mov_b32_e32 v1, 0                                        // 000000001908: 7E020280
	s_waitcnt lgkmcnt(0)                                       // 00000000190C: BF8CC07F
	global_store_dword v1, v0, s[0:1]                          // 000000001910: DC708000 00000001
	s_endpgm                                                   // 000000001918: BF810000
"""
_B = """
0000000000002a00 <_ZN2vm1kEPf>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000002A00: C0060002 00000000
	v_mov_b32_e32 v1, 0                                        // 000000002A08: 7E020280
	s_waitcnt lgkmcnt(0)                                       // 000000002A0C: BF8CC07F
	global_store_dword v1, v0, s[0:1]                          // 000000002A10: DC708000 00000001
	s_endpgm                                                   // 000000002A18: BF810000
	s_nop 0                                                    // 000000002A1C: BF800000
	s_nop 0                                                    // 000000002A20: BF800000
	s_nop 0                                                    // 000000002A24: BF800000
"""


def _seq(text):
    import kernel_diff as kd
    import lds_barrier_check as chk
    return {name: kd.normalise(insts) for name, (_, insts) in chk.functions(text).items()}


def test_normaliser_ignores_addresses_and_trailing_padding():
    import kernel_diff as kd
    a, b = _seq(_A), _seq(_B)
    assert list(a) == ["_ZN2vm1kEPf"] and len(a["_ZN2vm1kEPf"]) == 5
    assert a["_ZN2vm1kEPf"][-1] == ("s_endpgm", "")
    assert kd.compare(a, b) == ([], [], ["_ZN2vm1kEPf"], [])


def test_normaliser_reports_a_changed_operand():
    import kernel_diff as kd
    a, c = _seq(_A), _seq(_B.replace("v_mov_b32_e32 v1, 0 ", "v_mov_b32_e32 v1, 1 "))
    only_a, only_c, same, differ = kd.compare(a, c)
    assert (only_a, only_c, same) == ([], [], [])
    assert differ == [("_ZN2vm1kEPf", 5, 5, 1, (("v_mov_b32_e32", "v1, 0"), ("v_mov_b32_e32", "v1, 1")))]
    # a kernel on one side only is reported as such
    assert kd.compare(a, {}) == (["_ZN2vm1kEPf"], [], [], [])


@pytest.mark.skipif(not os.path.exists(LIB) or shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin") is None,
                    reason="needs the built library and ROCm's llvm-objdump")
def test_shipped_library_equals_itself():
    import kernel_diff as kd
    k = kd.kernels(LIB)
    only_a, only_b, same, differ = kd.compare(k, k)
    assert len(same) >= 1 and len(same) == len(k)
    assert not only_a and not only_b and not differ
    assert any("conv3x3_first_softmax_strip" in n for n in k) and any("conv3x3_head_mfma" in n for n in k)
    # one kernel of each conv unit split off conv3x3.hip (conv_patch, conv_thin, conv_pack, conv_up2x) and of conv_pair
    for name in ("conv3x3_patch_persist", "conv3x3_thin", "pack_weights_tiled", "conv3x3_up2x_border",
                 "conv3x3_pair_persist"):
        assert any(name in n for n in k), name
    # ... and no kernel defined in two units (a second copy is keyed "name#2"): the one every unit reaches
    assert sum("splitk_reduce_kernel" in n for n in k) == 1
    # one kernel of each weight-gradient unit (wgrad, wgrad_mfma, wgrad_taps, wgrad_wide); the reduction every unit
    # launches exists once, and no weight-gradient kernel has a second copy
    for name in ("wgrad_kernel", "wgrad_mfma_kernel", "wgrad_taps_kernel", "wgrad_taps_dma_kernel", "wgrad_wide_kernel",
                 "wgrad_wide_f32_kernel"):
        assert any(name in n for n in k), name
    assert sum("wgrad_reduce4_kernel" in n for n in k) == 1
    assert not [n for n in k if "wgrad" in n and "#" in n]
