"""numpy restatement of the power-of-two operand scale (``pow2_scale_from_bits`` in csrc/e3_tp_mfma_core.h; the contract
is written above ``e3_pow2_scale`` in include/e3gnn.h), used by tests/test_scale_*.py.  TEST INFRASTRUCTURE ONLY.

The scale ``{s, 1/s, bits of max |x|}`` is taken over the FINITE elements only: NaN and +-inf never enter the maximum."""
import numpy as np


def f32_bits(v) -> int:
    return int(np.asarray(v, dtype=np.float32).reshape(()).view(np.uint32))


def bits_f32(b: int) -> float:
    return float(np.asarray(b, dtype=np.uint32).reshape(()).view(np.float32))


def scale_from_bits(amax_bits: int, target: int) -> float:
    """s = 2^(se - 127), se = clamp(127 + target - (e - 127), 1, 254), e the biased exponent of max |x|; e == 0 (zero or
    denormal maximum) and e == 255 give s = 1."""
    e = (int(amax_bits) >> 23) & 0xFF
    if e == 0 or e == 0xFF:
        return 1.0
    se = min(max(127 + target - (e - 127), 1), 254)
    return bits_f32(se << 23)


def finite_absmax(arrays) -> np.float32:
    """max |x| over the finite elements of every array (0 if there are none), in fp32."""
    m = np.float32(0.0)
    for a in arrays:
        a = np.abs(np.asarray(a, dtype=np.float32)).ravel()
        a = a[np.isfinite(a)]
        if a.size:
            m = max(m, np.float32(a.max()))
    return np.float32(m)


def expected_scale(arrays, target: int):
    """(s, 1/s, bits of max |x|) as ``e3_pow2_scale`` returns them in out4[0], out4[1] and out4[2]."""
    bits = f32_bits(finite_absmax(arrays))
    s = scale_from_bits(bits, target)
    return s, float(np.float32(1.0) / np.float32(s)), bits
