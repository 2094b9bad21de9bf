"""Reader for a classic BGEO v5 frame with FLOAT / VECTOR / INT point attributes, the layout partio writes (Externals/partio/io/BGEO.cpp:311-407):
the 41-byte header, per attribute {16-bit name length, name, 16-bit size, 32-bit Houdini type 0 / 5 / 1, `size` zero defaults}, per point x y z
w = 1 and the attributes' values - float32, or int32 for an INT attribute -, all big-endian, and the two trailing bytes 00 ff."""
import struct

import numpy as np


def read_bgeo(path):
    """(xyz float32 (n, 3), {name: (n, size) float32, or int32 for an INT attribute}, [(name, size, houdini type)] in file order)"""
    raw = open(path, "rb").read()
    magic, vchar, version, npoints = struct.unpack(">IcII", raw[:13])
    assert magic == 0x4267656F and vchar == b"V" and version == 5
    nprims, npg, nprg, nattr, nva, npa, na = struct.unpack(">7I", raw[13:41])
    assert (nprims, npg, nprg, nva, npa, na) == (0, 0, 0, 0, 0, 0)
    at, attrs = 41, []
    for _ in range(nattr):
        ln = struct.unpack(">H", raw[at:at + 2])[0]
        name = raw[at + 2:at + 2 + ln].decode()
        size, kind = struct.unpack(">Hi", raw[at + 2 + ln:at + 8 + ln])
        assert kind in (0, 1, 5), kind
        assert raw[at + 8 + ln:at + 8 + ln + 4 * size] == b"\x00" * (4 * size), "defaults are zero"
        attrs.append((name, size, kind))
        at += 8 + ln + 4 * size
    width = 4 + sum(s for _, s, _ in attrs)
    body = raw[at:at + 4 * width * npoints]
    assert len(body) == 4 * width * npoints and raw[at + 4 * width * npoints:] == b"\x00\xff"
    f = np.frombuffer(body, dtype=">f4").reshape(npoints, width)
    i = np.frombuffer(body, dtype=">i4").reshape(npoints, width)
    assert np.all(f[:, 3] == 1.0)
    out, col = {}, 4
    for name, size, kind in attrs:
        out[name] = (i if kind == 1 else f)[:, col:col + size].astype(np.int32 if kind == 1 else np.float32)
        col += size
    return f[:, :3].astype(np.float32), out, attrs
