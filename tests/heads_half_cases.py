"""Inputs and references shared by the tests of the fp16 / bf16-feature multi-head entries
(host and device; include/spmm_hip.h).

The operands are heads_cases' random fp32 values rounded to the storage type and widened
back, so the widening is the identity on them. The reference of every bit comparison is the
existing fp32 host form (prep.sddmm_heads / prep.csrmm_heads on float32 arrays) on the
widened operands, never the new code. Everything is cached: treat what comes back as
read-only."""
from __future__ import annotations

import functools

import numpy as np

import heads_cases as hc
import sddmm_cases as sd
from heads_cases import F

TYPES = ["f16", "bf16"]


def to_bits(a, ty):
    """float32 array -> uint16 patterns of `ty`, round to nearest even (finite inputs inside
    the type's range; bf16 on the bit pattern, numpy having no bfloat16)."""
    a = np.ascontiguousarray(a, F)
    if ty == "f16":
        return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits, ty):
    """uint16 patterns of `ty` -> float32, exact."""
    bits = np.ascontiguousarray(bits, np.uint16)
    if ty == "f16":
        return bits.view(np.float16).astype(F)
    return (bits.astype(np.uint32) << 16).view(F)


def stored(bits, ty):
    """(the array prep takes for these patterns, its keyword arguments)."""
    bits = np.ascontiguousarray(bits, np.uint16)
    return (bits.view(np.float16), {}) if ty == "f16" else (bits, {"bf16": True})


def rounded(a, ty):
    """(patterns, widened) of a float32 array, both read-only."""
    b = to_bits(a, ty)
    w = widen(b, ty)
    b.setflags(write=False)
    w.setflags(write=False)
    return b, w


# The edge values of each type: (name, pattern). The smallest subnormal, the largest finite
# value, the zeros, the infinities and a quiet NaN.
EDGE_BITS = {
    "f16": [("+0", 0x0000), ("-0", 0x8000), ("min subnormal", 0x0001), ("-min subnormal", 0x8001),
            ("max finite", 0x7bff), ("-max finite", 0xfbff), ("+inf", 0x7c00), ("-inf", 0xfc00),
            ("nan", 0x7e00)],
    "bf16": [("+0", 0x0000), ("-0", 0x8000), ("min subnormal", 0x0001),
             ("-min subnormal", 0x8001), ("max finite", 0x7f7f), ("-max finite", 0xff7f),
             ("+inf", 0x7f80), ("-inf", 0xff80), ("nan", 0x7fc0)],
}


# ------------------------------------------------------------------ sampled product
@functools.lru_cache(maxsize=None)
def sddmm_operands(m, k, heads, d, ty):
    """(X patterns, Y patterns, X widened, Y widened): [m, heads, d] and [k, heads, d]."""
    X, Y = hc.sddmm_operands(m, k, heads, d)
    xb, xw = rounded(X, ty)
    yb, yw = rounded(Y, ty)
    return xb, yb, xw, yw


@functools.lru_cache(maxsize=None)
def sddmm_reference(name, heads, d, ty, epilogue=False):
    """[nnz, heads]: the fp32 host form on the widened operands; outside the pattern NaN
    (the old values with the epilogue: alpha, beta of heads_cases)."""
    from spmm_hip import prep
    m, k, rp, ci = sd.pattern(name)
    _, _, xw, yw = sddmm_operands(m, k, heads, d, ty)
    if epilogue:
        out = prep.sddmm_heads(m, d, k, heads, rp, ci, xw, yw, alpha=hc.ALPHA, beta=hc.BETA,
                               out=hc.sddmm_old(ci.size, heads).copy())
    else:
        out = prep.sddmm_heads(m, d, k, heads, rp, ci, xw, yw,
                               out=np.full((ci.size, heads), np.nan, F))
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ product
@functools.lru_cache(maxsize=None)
def product_operands(heads, d, ty, small=False):
    """(m, k, rowptr, colind, val, B patterns, B widened, old C) on heads_cases' pattern."""
    m, k, rp, ci = hc.product_pattern(small)
    val, B, C = hc.product_operands(ci.size, k, m, heads, d)
    bb, bw = rounded(B, ty)
    return m, k, rp, ci, val, bb, bw, C


@functools.lru_cache(maxsize=None)
def product_reference(heads, d, ty, epilogue=False, small=False):
    """[m, heads, d]: the fp32 host form on the widened B."""
    from spmm_hip import prep
    m, k, rp, ci, val, _, bw, C = product_operands(heads, d, ty, small)
    if epilogue:
        out = prep.csrmm_heads(m, d, k, heads, rp, ci, val, bw, C=C.copy(), alpha=hc.ALPHA,
                               beta=hc.BETA)
    else:
        out = prep.csrmm_heads(m, d, k, heads, rp, ci, val, bw)
    out = np.asarray(out).reshape(m, heads, d)
    out.setflags(write=False)
    return out


def padded16(a, ld, offset=0, fill=0x7fff):
    """(flat uint16 buffer, view): the rows of the patterns a ([rows, w]) at leading dimension
    ld, `offset` elements into the buffer, the padding filled with `fill` (a NaN of
    either type)."""
    rows, w = a.shape
    buf = np.full(offset + max(rows, 1) * ld, fill, np.uint16)
    view = buf[offset:offset + rows * ld].reshape(rows, ld)
    view[:, :w] = a
    return buf, view
