"""Checksum over hand-made key/value shapes (kernels.hip k_crc64_reg,
d_crc64_stream).

k_crc64_reg is the only CRC kernel. One lane digests key||value of one row as
two aligned 8-byte word streams with a funnel shift: 64-byte register chunks
while a whole chunk remains, then single words, then the tail bytes. The
region pairs every key length with every value length of LENGTHS, so either
stream meets: nothing at all, tail bytes alone (1..7), the word loop alone
(8, 9, 15..63), exactly one chunk (64), one chunk plus a remainder (65, 71,
72, 127), two chunks (128) and two chunks plus a remainder (129, 200).
region_raw takes empty keys and empty values, so the lengths start at 0.
Every comparison with the oracle's checksum is exact.
"""
import ctypes as C

import pytest

from test_dev_chunk import _orc

LENGTHS = tuple(range(10)) + (15, 16, 17, 63, 64, 65, 71, 72, 127, 128, 129,
                              200)


def blob(seed, n):
    """n bytes that differ from row to row and from byte to byte; a value
    never starts like a row-v1 cell (8) or a row-v2 row (128)"""
    out = bytearray((seed * 131 + j * 29 + (j >> 3) * 7) & 0xFF
                    for j in range(n))
    if out and out[0] in (8, 128):
        out[0] = 0x41
    return bytes(out)


def pairs():
    """every (key length, value length) of LENGTHS x LENGTHS. The rotation of
    the value lengths by the key's index mixes the running offsets of both
    streams; test_all_lengths_and_alignments asserts what that has to give."""
    n = len(LENGTHS)
    return [(blob(2 * (a * n + b), LENGTHS[a]),
             blob(2 * (a * n + b) + 1, LENGTHS[(a + b) % n]))
            for a in range(n) for b in range(n)]


def raw_of(kv):
    keys = b"".join(k for k, _ in kv)
    vals = b"".join(v for _, v in kv)
    ko, vo = [0], [0]
    for k, v in kv:
        ko.append(ko[-1] + len(k))
        vo.append(vo[-1] + len(v))
    kb = (C.c_uint8 * max(len(keys), 1)).from_buffer_copy(keys or b"\0")
    vb = (C.c_uint8 * max(len(vals), 1)).from_buffer_copy(vals or b"\0")
    return (C.cast(kb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(ko))(*ko),
            C.cast(vb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(vo))(*vo),
            len(kv), (kb, vb)), ko, vo


def both(engine, raw):
    want = _orc().checksum(*raw[:5])
    rgn = engine.region_raw(*raw[:5])
    try:
        got = engine.checksum([rgn])
    finally:
        rgn.close()
    return want, got


def long_starts(offs):
    """start alignments of the entries of at least 64 bytes"""
    return {offs[i] & 7 for i in range(len(offs) - 1)
            if offs[i + 1] - offs[i] >= 64}


@pytest.mark.gpu
def test_all_lengths_and_alignments(engine):
    kv = pairs()
    raw, ko, vo = raw_of(kv)
    assert {(len(k), len(v)) for k, v in kv} == \
        {(a, b) for a in LENGTHS for b in LENGTHS}
    # every start alignment of either stream occurs with a chunked length
    assert long_starts(ko) == set(range(8))
    assert long_starts(vo) == set(range(8))
    want, got = both(engine, raw)
    assert want[1] == len(kv) and want[2] == ko[-1] + vo[-1]
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257])
def test_one_row_and_one_past_a_block(engine, n):
    """a single lane, and 256 lanes plus one row in a second block"""
    kv = [p for p in pairs() if len(p[0]) >= 64 and len(p[1]) >= 64][:1] \
        if n == 1 else pairs()[:n]
    assert len(kv) == n
    raw, ko, vo = raw_of(kv)
    want, got = both(engine, raw)
    assert want[1] == n
    assert got == want
