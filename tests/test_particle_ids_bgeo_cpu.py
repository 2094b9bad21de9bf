"""The BGEO writer's INT point attribute (claymore_amd/host/particle_io.hpp) without a GPU: a frame with "id" written by a small program built from
the writer's header and parsed back here, field by field against partio's layout (Externals/partio/io/BGEO.cpp:343-407: Houdini type 1, 16-bit
size 1, one zero default, values as big-endian int32); and the frames without it - position-only, "v", stress - byte for byte what they were (the
partio-written fixtures under tests/golden)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from bgeo_reader import read_bgeo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "claymore_amd", "host")
GOLD = os.path.join(ROOT, "tests", "golden")


def _build(tmp_path, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Werror", "-o", str(exe), os.path.join(HOST, name + ".cpp")])
    return str(exe)


@pytest.mark.parametrize("with_v", [False, True])
def test_frame_with_the_int_attribute_id(tmp_path, with_v):
    exe = _build(tmp_path, "bgeo_ids_selftest")
    rng = np.random.default_rng(5)
    n = 257
    xyz = rng.uniform(0.1, 0.9, (n, 3)).astype(np.float32)
    vel = rng.normal(size=(n, 3)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int32)
    ids[:3] = [-1, 2 ** 31 - 1, -(2 ** 31)]                                   # the sign and every byte of the word
    xyz.tofile(tmp_path / "p.f32")
    vel.tofile(tmp_path / "v.f32")
    ids.tofile(tmp_path / "i.i32")
    out = tmp_path / "ids.bgeo"
    subprocess.check_call([exe, str(tmp_path / "p.f32"), str(tmp_path / "i.i32"), str(out)] + ([str(tmp_path / "v.f32")] if with_v else []))
    raw = open(out, "rb").read()
    # the attribute's definition, byte for byte
    id_def = struct.pack(">H", 2) + b"id" + struct.pack(">Hii", 1, 1, 0)
    v_def = struct.pack(">H", 1) + b"v" + struct.pack(">Hi3i", 3, 5, 0, 0, 0)
    defs = (v_def if with_v else b"") + id_def
    assert struct.unpack(">7I", raw[13:41]) == (0, 0, 0, 2 if with_v else 1, 0, 0, 0)
    assert raw[41:41 + len(defs)] == defs
    width = 4 + (3 if with_v else 0) + 1
    assert len(raw) == 41 + len(defs) + 4 * width * n + 2
    # the first point's id word: big-endian int32
    first = 41 + len(defs)
    assert raw[first + 4 * (width - 1):first + 4 * width] == struct.pack(">i", -1)
    got_xyz, attrs, order = read_bgeo(out)
    assert order == ([("v", 3, 5)] if with_v else []) + [("id", 1, 1)]
    assert np.array_equal(got_xyz.view(np.uint32), xyz.view(np.uint32))
    assert attrs["id"].dtype == np.int32 and np.array_equal(attrs["id"][:, 0], ids)
    if with_v:
        assert np.array_equal(attrs["v"].view(np.uint32), vel.view(np.uint32))


def test_frames_without_the_attribute_are_byte_for_byte_what_they_were(tmp_path):
    exe = _build(tmp_path, "host_selftest")
    pts = os.path.join(GOLD, "g10_points.f32")
    for args, want in ((["--bgeo-from", pts], "g10_partio.bgeo"),
                       (["--bgeo-v-from", pts, os.path.join(GOLD, "g10_velocity.f32")], "g10_partio_v.bgeo"),
                       (["--bgeo-stress-from", pts, os.path.join(GOLD, "g10_stress.f32")], "g10_partio_stress.bgeo")):
        out = tmp_path / ("mine_" + want)
        subprocess.check_call([exe] + args + [str(out)])
        assert open(out, "rb").read() == open(os.path.join(GOLD, want), "rb").read(), want
