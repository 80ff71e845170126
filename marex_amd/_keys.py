"""The order-preserving uint32 key of float32 values that the device maxima work on, and its inverse (NumPy only)."""
import numpy as np


def float_key(a) -> np.ndarray:
    """The order-preserving uint32 key of float32 values that the device maximum works on: ``bits | 2^31`` for a clear
    sign bit, ``~bits`` otherwise.  Strictly monotone from -inf to +inf (-0 below +0); no finite value and neither infinity
    maps to 0, which the kernel keeps for "no finite cell"."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_float(k) -> np.ndarray:
    """Inverse of :func:`float_key`; key 0 gives a NaN."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)
