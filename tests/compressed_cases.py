"""Kaldi compressed matrices built directly from random bytes (no compressor needed: any sorted percentiles and any data bytes are a
valid entry), for the tests of the device decode - tests/test_compressed_host.py, tests/test_gpu_decode_compressed.py,
tests/test_gpu_pipeline_compressed.py.  Not collected by pytest.

A BODY is what follows the token on disk: the 16-byte global header {float min, float range, int32 rows, int32 cols}, then
    'CM '  cols x 4 uint16 percentiles, cols x rows bytes column-major
    'CM2'  rows x cols uint16 row-major
    'CM3'  rows x cols uint8 row-major
"""

import io
import struct

import numpy as np

TOKENS = {1: b"CM ", 2: b"CM2 ", 3: b"CM3 "}


def _header(gmin, grange, rows, cols):
    return struct.pack("<ffii", gmin, grange, rows, cols)


def cm_body(rng, rows, cols, gmin=-12.5, grange=31.0, percentiles=None):
    """'CM ' body: random sorted uint16 percentiles per column (or `percentiles`, four values used for every column), random data
    bytes; from 256 rows on every column starts with a permutation of 0...255, so every byte value occurs in every column."""
    if percentiles is None:
        pct = np.sort(rng.randint(0, 65536, size=(cols, 4)), axis=1).astype("<u2")
    else:
        pct = np.tile(np.asarray(percentiles, dtype="<u2")[None], (cols, 1))
    data = rng.randint(0, 256, size=(cols, rows)).astype(np.uint8)
    if rows >= 256:
        for c in range(cols):
            data[c, :256] = rng.permutation(256)
    return _header(gmin, grange, rows, cols) + pct.tobytes() + data.tobytes()


def cm2_body(rng, rows, cols, gmin=-12.5, grange=31.0):
    q = rng.randint(0, 65536, size=(rows, cols)).astype("<u2")
    if rows * cols >= 2:
        q.flat[0], q.flat[-1] = 0, 65535
    return _header(gmin, grange, rows, cols) + q.tobytes()


def cm3_body(rng, rows, cols, gmin=-12.5, grange=31.0):
    q = rng.randint(0, 256, size=(rows, cols)).astype(np.uint8)
    if rows * cols >= 256:
        q.flat[:256] = rng.permutation(256)
    return _header(gmin, grange, rows, cols) + q.tobytes()


BODY = {1: cm_body, 2: cm2_body, 3: cm3_body}


def host_decode(fmt, body):
    """The host reader on a body with its token in front (libs.support.kaldi_io.read_mat: the arithmetic the device has to
    reproduce bit for bit)."""
    from libs.support import kaldi_io
    return np.ascontiguousarray(kaldi_io.read_mat(io.BytesIO(b"\0B" + TOKENS[fmt] + body)), dtype=np.float32)


def pack(bodies, front=0, back=0, fill=0xA5):
    """The bodies back to back, each at a 16-byte boundary, with `front` / `back` margin bytes (multiples of 16) of `fill` around and
    in the gaps: (uint8 array, byte offsets int64 [n])."""
    assert front % 16 == 0 and back % 16 == 0
    offs, at = [], front
    for b in bodies:
        offs.append(at)
        at += (len(b) + 15) // 16 * 16
    buf = np.full(at + back, fill, dtype=np.uint8)
    for o, b in zip(offs, bodies):
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return buf, np.asarray(offs, dtype=np.int64)


def write_ark(path, entries):
    """entries: (key, payload bytes from `\\0B` on) -> the ark file `path`; returns the scp lines 'key path:offset' (no newline)."""
    lines = []
    with open(path, "wb") as f:
        for key, payload in entries:
            f.write((key + " ").encode())
            lines.append("%s %s:%d" % (key, path, f.tell()))
            f.write(payload)
    return lines


def compressed_payload(fmt, body):
    return b"\0B" + TOKENS[fmt] + body


def float_payload(mat):
    """`\\0BFM ` (float32) or `\\0BDM ` (float64) entry of a matrix."""
    mat = np.ascontiguousarray(mat)
    tag = b"FM " if mat.dtype == np.float32 else b"DM "
    return b"\0B" + tag + struct.pack("<bibi", 4, mat.shape[0], 4, mat.shape[1]) + mat.tobytes()
