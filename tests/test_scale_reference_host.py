"""The numpy restatement of the operand scale (tests/scale_reference.py) on hand-worked values, so that the GPU contract
tests (test_scale_contract_gpu.py) compare the kernels with something that is itself pinned."""
import math

import numpy as np
import pytest

from scale_reference import bits_f32, expected_scale, f32_bits, finite_absmax, scale_from_bits

FLT_MAX = float(np.finfo(np.float32).max)
DENORM = float(np.float32(2.0 ** -140))


@pytest.mark.parametrize("amax,target,s", [
    (0.0, 10, 1.0),                     # e == 0: zero
    (DENORM, 10, 1.0),                  # e == 0: denormal
    (2.0 ** -126, 10, 2.0 ** 127),      # se = 127 + 10 + 126 = 263 -> clamped to 254
    (2.0 ** -117, 10, 2.0 ** 127),      # se = 254 exactly: the last unclamped value
    (2.0 ** -116, 10, 2.0 ** 126),
    (1.0, 10, 2.0 ** 10),
    (1.5, 10, 2.0 ** 10),
    (1000.0, 10, 2.0),                  # 1000 = 1.95 * 2^9: s = 2^(10 - 9)
    (1000.0, 6, 2.0 ** -3),
    (1024.0, 10, 1.0),
    (FLT_MAX, 10, 2.0 ** -117),         # e = 254: se = 127 + 10 - 127 = 10
    (FLT_MAX, -20, 2.0 ** -126),        # se = 127 - 20 - 127 = -20 -> clamped to 1
    (2.0 ** 120, -20, 2.0 ** -126),     # se = 127 - 20 - 120 = -13 -> clamped to 1
    (2.0 ** 106, -20, 2.0 ** -126),     # se = 1 exactly
    (2.0 ** 105, -20, 2.0 ** -125),
])
def test_scale_from_bits_hand_worked(amax, target, s):
    assert scale_from_bits(f32_bits(amax), target) == s


def test_scale_puts_the_maximum_in_its_binade():
    for k in range(-116, 128):
        for target in (10, 9, 6):
            m = 1.75 * 2.0 ** k if k < 127 else FLT_MAX
            s = scale_from_bits(f32_bits(m), target)
            if -126 <= target - k <= 127:      # unclamped: m s in [2^target, 2^(target + 1))
                assert 2.0 ** target <= m * s < 2.0 ** (target + 1), (k, target, s)
            assert math.log2(s) == round(math.log2(s))


def test_non_finite_and_all_non_finite():
    assert scale_from_bits(f32_bits(np.inf), 10) == 1.0
    assert scale_from_bits(f32_bits(np.nan), 10) == 1.0
    x = np.array([1.0, -7e3, np.nan, np.inf, -np.inf, 3.0], dtype=np.float32)
    assert finite_absmax([x]) == np.float32(7e3)
    s, inv, bits = expected_scale([x], 10)
    assert (s, inv, bits) == (2.0 ** -2, 4.0, f32_bits(7e3))            # 7e3 = 1.71 * 2^12
    assert expected_scale([np.array([np.nan, np.inf, -np.inf], dtype=np.float32)], 10) == (1.0, 1.0, 0)
    assert expected_scale([np.zeros(5, dtype=np.float32)], 10) == (1.0, 1.0, 0)
    # the joint maximum of several tensors; 1/s is exact because s is a power of two
    s, inv, bits = expected_scale([np.array([2.0]), np.array([-96.0, np.nan])], 9)
    assert bits_f32(bits) == 96.0 and s == 2.0 ** 3 and inv == 2.0 ** -3
