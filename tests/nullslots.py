"""Rewrite the bytes under the NULLs of a PyChunk's fixed-width columns.

PyChunk zero-fills its buffers and append_row(None) clears only the bitmap
bit, so every NULL slot the suite builds holds 00..00. The reference's
Column.AppendNull appends elemBuf instead -- the previously appended value --
and the engine uploads bound chunks verbatim. A result must therefore not
depend on those bytes: call fill_null_slots after the last append_row and
before bind_chunks, and compare with the zero-filled run.

Var-len columns stay untouched: a NULL var-len value has zero length in the
reference layout, there is nothing under it.
"""
import struct

import numpy as np

from tests.gxlib import GX_TYPE_DECIMAL, GX_TYPE_F64, GX_TYPE_TIME

MODES = ("zero", "stale", "ones", "extreme", "random")
POISON_MODES = MODES[1:]

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _dec_65_nines(negative):
    """A well-formed MyDecimal of 65 nines: digitsInt 65, digitsFrac 0, eight
    words (99, then seven of 999999999). It parses, and overflows int128."""
    return struct.pack("<bbbB9i", 65, 0, 0, 1 if negative else 0,
                       99, *([999999999] * 7), 0)


def _extreme(typ, k):
    if typ == GX_TYPE_DECIMAL:
        return _dec_65_nines(k % 2 == 1)
    if typ == GX_TYPE_F64:
        return struct.pack("<d", float("nan") if k % 2 else float("inf"))
    if typ == GX_TYPE_TIME:
        return struct.pack("<Q", 0xFFFFFFFFFFFFFFF0)
    return struct.pack("<q", INT64_MAX if k % 2 else INT64_MIN)


def fill_null_slots(chunk, mode, seed=0):
    """Returns how many slots were rewritten (0 in mode 'zero')."""
    assert mode in MODES, mode
    if mode == "zero":
        return 0
    rng = np.random.default_rng(seed)
    n_written = 0
    for col in chunk.columns:
        if col.offsets is not None:
            continue
        elem = 40 if col.typ == GX_TYPE_DECIMAL else 8
        prev = bytes(elem)
        k = 0  # NULLs seen in this column
        for i in range(col.length):
            slot = slice(i * elem, (i + 1) * elem)
            if (col.null_bitmap[i // 8] >> (i % 8)) & 1:
                prev = bytes(col.data[slot])
                continue
            if mode == "stale":
                fill = prev
            elif mode == "ones":
                fill = b"\xff" * elem
            elif mode == "extreme":
                fill = _extreme(col.typ, k)
            else:
                fill = rng.integers(0, 256, elem, dtype=np.uint8).tobytes()
            col.data[slot] = np.frombuffer(fill, dtype=np.uint8)
            k += 1
            n_written += 1
    return n_written


def count_null_slots(chunk, col):
    """NULLs of one fixed-width column: what a fill rewrites there."""
    c = chunk.columns[col]
    assert c.offsets is None
    return sum(1 for i in range(c.length)
               if not (c.null_bitmap[i // 8] >> (i % 8)) & 1)
