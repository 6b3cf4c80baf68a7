"""CPU checks of the argument helpers the frame ops share: the integer check, and the options merge behind
ops.flow_options, ops.plate_options and ops.guided_options."""

import numpy as np
import pytest


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
