"""CPU checks of the argument helpers the frame ops share: the integer check, the options merge behind
ops.flow_options, ops.plate_options and ops.guided_options, and the two checks of the layer above the ops: the array
check of host arrays and device tensors, and the ``flow`` / ``flow_options`` check of the streams and the scorer."""

import numpy as np
import pytest
import torch


def test_check_int():
    from vmatting import ops
    for bad in (True, np.bool_(True), 2.0, "2", None):
        with pytest.raises(TypeError, match="t: v must be an integer"):
            ops.check_int("t", "v", bad)
        with pytest.raises(TypeError, match="t: v must be an integer"):
            ops.check_int("t", "v", bad, 0, 4)
    got = ops.check_int("t", "v", np.int64(3), 0, 4)
    assert got == 3 and type(got) is int
    assert ops.check_int("t", "v", -7) == -7                                   # no range: any integer
    assert ops.check_int("t", "v", 1, 1, 4) == 1 and ops.check_int("t", "v", 4, 1, 4) == 4   # both ends belong
    assert ops.check_int("t", "v", 1, 1) == 1 and ops.check_int("t", "v", 4, hi=4) == 4
    for v, lo, hi in ((0, 1, 4), (5, 1, 4), (0, 1, None), (5, None, 4), (np.int32(-1), 0, None)):
        with pytest.raises(ValueError, match="t: v must be"):
            ops.check_int("t", "v", v, lo, hi)


def test_options_over_defaults():
    from vmatting import ops
    faces = [  # the family's face, its defaults, a partial override, a bad value and what the family's checker raises
        (lambda o: ops.flow_options("t", 32, 48, o), ops.FLOW_DEFAULTS, {"iters": np.int64(5)},
         [({"iters": 0}, ValueError), ({"warps": 2.5}, TypeError), ({"alpha": 0.0}, ValueError)]),
        (lambda o: ops.plate_options("t", o), ops.PLATE_DEFAULTS, {"hi": 60, "r_fg": 0},
         [({"lo": 48}, ValueError), ({"hi": 48.0}, TypeError), ({"r_bg": 33}, ValueError)]),
        (lambda o: ops.guided_options("t", o), ops.GUIDED_DEFAULTS, {"eps": 0.5},
         [({"r": 0}, ValueError), ({"r": 2.0}, TypeError), ({"eps": "1e-3"}, TypeError)]),
    ]
    for face, defaults, part, bad in faces:
        assert face(None) == defaults and face({}) == defaults and face(None) is not defaults
        got = face(part)
        assert got == dict(defaults, **part) and list(got) == list(defaults)    # the defaults' key order
        assert all(type(v) is type(defaults[k]) for k, v in got.items())        # checked: numpy integers come back int
        with pytest.raises(ValueError) as e:
            face(dict(part, sweeps=3))
        assert "t takes" in str(e.value) and "'sweeps'" in str(e.value)
        assert all(repr(k) in str(e.value) for k in defaults)                   # the accepted keys are named
        for options, exc in bad:
            with pytest.raises(exc, match="t: "):
                face(options)
    with pytest.raises(ValueError, match="16 x 16"):                            # the estimator's smallest frame
        ops.flow_options("t", 15, 48, None)


class Refused(Exception):
    """What a caller asks check_array to raise for a wrong type or dtype (neither a TypeError nor a ValueError)."""


def test_check_array_on_host_arrays_and_host_tensors():
    from vmatting import ops
    u8 = (torch.uint8,)
    shapes = "n,h,w | n,h,w,1 | h,w"

    def check(a, dtypes=u8, accept=ops.NUMPY, wrong=TypeError, **dims):
        return ops.check_array("t", "v", a, dtypes, shapes, accept, wrong, **dims)

    for shape in ((2, 4, 6), (2, 4, 6, 1), (4, 6)):                             # every alternative, as ints
        got = check(np.zeros(shape, np.uint8))
        assert got == shape and all(type(v) is int for v in got)
    assert check(np.zeros((4, 6), np.float64), (torch.float32, torch.float64)) == (4, 6)
    assert check(np.zeros((4, 12), np.uint8)[:, ::2]) == (4, 6)                 # numpy strides are the stager's business
    # a named size must agree, in whichever alternative names it
    assert check(np.zeros((2, 4, 6), np.uint8), n=2, h=4, w=6) == (2, 4, 6)
    assert check(np.zeros((4, 6), np.uint8), n=2, h=4, w=6) == (4, 6)
    for dims in (dict(n=3), dict(h=5), dict(w=4)):
        with pytest.raises(ValueError, match=r"t: v must be \[n,h,w\] or \[n,h,w,1\] or \[h,w\] with "):
            check(np.zeros((2, 4, 6), np.uint8), **dims)
    # an unnamed letter is any size >= 1, a number stands for itself; a shape is a ValueError whatever ``wrong`` is
    for shape in ((0, 4, 6), (2, 4, 6, 2), (6,), (2, 4, 6, 1, 1)):
        with pytest.raises(ValueError, match="t: v must be"):
            check(np.zeros(shape, np.uint8), wrong=Refused)
    # a wrong type or dtype raises what the caller asked for; a numpy-only site refuses a tensor
    for wrong in (TypeError, ValueError, Refused):
        for bad in ([[0]], None, torch.zeros((4, 6), dtype=torch.uint8), np.zeros((4, 6), np.int8),
                    np.zeros((4, 6), np.float32), np.zeros((4, 6), np.uint16)):
            with pytest.raises(wrong, match="t: v must be"):
                check(bad, wrong=wrong)
    with pytest.raises(Refused, match="a numpy array, got Tensor"):
        check(torch.zeros((4, 6), dtype=torch.uint8), wrong=Refused)
    # tensors, on the host here: dtype, shape and strides show without a device, which is looked at last
    t = torch.zeros((2, 4, 6), dtype=torch.uint8)
    for accept in (ops.DEVICE, ops.EITHER):
        with pytest.raises(Refused, match="torch.uint8, got torch.float32"):
            check(t.float(), accept=accept, wrong=Refused)
        with pytest.raises(ValueError, match="t: v must be"):
            check(t[0, 0], accept=accept, wrong=Refused)
        with pytest.raises(ValueError, match="h=4"):
            check(t.transpose(1, 2), accept=accept, wrong=Refused, h=4)         # [2,6,4]
        with pytest.raises(ValueError, match="contiguous"):
            check(t.transpose(1, 2), accept=accept, wrong=Refused)
        with pytest.raises(Refused, match="host tensor"):
            check(t, accept=accept, wrong=Refused)                              # all is right but the device
        # strided=True (the consumer copies): a tensor's strides are its own business, and the device is what is left
        with pytest.raises(Refused, match="host tensor"):
            ops.check_array("t", "v", t.transpose(1, 2), u8, shapes, accept, Refused, strided=True)
        with pytest.raises(ValueError, match="h=4"):
            ops.check_array("t", "v", t.transpose(1, 2), u8, shapes, accept, Refused, strided=True, h=4)
    assert check(np.zeros((2, 4, 6), np.uint8), accept=ops.EITHER) == (2, 4, 6)
    with pytest.raises(Refused, match="a ROCm device tensor, got ndarray"):     # a device-only site refuses numpy
        check(np.zeros((2, 4, 6), np.uint8), accept=ops.DEVICE, wrong=Refused)
    # the one dtype table
    assert ops.torch_dtype(np.zeros(1, np.float32)) is torch.float32 and ops.torch_dtype(t) is torch.uint8
    assert ops.torch_dtype(np.zeros(1, np.float64)) is torch.float64
    assert ops.torch_dtype(np.zeros(1, np.int16)) == np.dtype(np.int16)         # no twin here: in no caller's dtypes
    # _check_tensor reads the same grammar
    assert ops._check_tensor("t", "v", t, u8, shapes, n=2) == (2, 4, 6)
    with pytest.raises(ValueError, match=r"t: v must be \[n,h,w\] or \[n,h,w,1\] or \[h,w\] with n=3"):
        ops._check_tensor("t", "v", t, u8, shapes, n=3)


def test_check_flow_mode_for_the_three_callers():
    from vmatting import ops
    callers = (("FrameStream", (None,) + ops.FLOW_MODES, "estimate"),           # None: estimated
               ("ClipStream", ops.FLOW_MODES, None),
               ("MatteScorer", (None,) + ops.FLOW_MODES, None))                 # None: no flow at all
    for who, modes, default in callers:
        def check(flow, options=None, h=32, w=48):
            return ops.check_flow_mode(who, flow, options, h, w, modes, default)

        assert check("estimate") == ops.FLOW_DEFAULTS and check("estimate") is not ops.FLOW_DEFAULTS
        got = check("estimate", {"iters": np.int64(5)})
        assert got == dict(ops.FLOW_DEFAULTS, iters=5) and type(got["iters"]) is int
        assert check("given") is None
        estimated = ["estimate"]
        if None in modes:
            assert check(None) == (ops.FLOW_DEFAULTS if default == "estimate" else None)
            estimated += [None] if default == "estimate" else []
        for flow in modes:
            if flow not in estimated:
                with pytest.raises(ValueError, match="%s: flow_options go with flow='estimate'" % who):
                    check(flow, {"iters": 5})                                   # options with a non-estimate mode
                with pytest.raises(ValueError, match="flow_options go with"):
                    check(flow, {})
                assert check(flow, None, 8, 8) is None                          # only the estimator has a smallest frame
        for flow in ("estimated", "", 1, False) + (() if None in modes else (None,)):
            with pytest.raises(ValueError, match="%s: flow must be one of" % who):
                check(flow)
            with pytest.raises(ValueError, match="%s: flow must be one of" % who):
                check(flow, {"sweeps": 3}, 8, 8)                                # the mode is looked at first
        for flow in estimated:
            with pytest.raises(ValueError) as e:
                check(flow, {"sweeps": 3})                                      # an unknown key
            assert "%s: flow_options takes" % who in str(e.value) and "'sweeps'" in str(e.value)
            with pytest.raises(TypeError, match="%s: flow_options: warps" % who):
                check(flow, {"warps": 2.5})
            for h, w in ((15, 48), (32, 15)):
                with pytest.raises(ValueError, match="16 x 16"):
                    check(flow, None, h, w)
            assert check(flow, None, 16, 16) == ops.FLOW_DEFAULTS
    assert ops.check_flow_mode("t", "given", None, 32, 48) is None              # by default the streams' two modes
    with pytest.raises(ValueError, match="t: flow must be one of"):
        ops.check_flow_mode("t", None, None, 32, 48)
