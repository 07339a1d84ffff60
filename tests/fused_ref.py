"""Helpers the GPU operator tests share (plain module, like canon.py): bit views, order-free inputs, the SwiGLU epilogue, result rows."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def order_free(rng, shape, amp=32):
    """multiples of 2^-4 in [-amp / 16, amp / 16] (amp = 32: [-2, 2]): sums of squares of up to 2^14 of them are exact in fp32 in any order"""
    return (rng.integers(-amp, amp + 1, size=shape).astype(np.float32) / np.float32(16.0)).astype(np.float32)


def silu_mul(a, b):
    a = a.astype(np.float32)
    with np.errstate(over="ignore"):            # exp(-a) beyond fp32 is +inf on the device too: silu = a * 0
        return (a * (np.float32(1) / (np.float32(1) + np.exp(-a.astype(np.float64)).astype(np.float32))) * b).astype(np.float32)


def rows_total(kind, rows):
    """rows of a launch's result: the tensors one after the other (kind 2, SwiGLU: the two matrices share theirs)"""
    return rows[0] if kind == 2 else sum(rows)
