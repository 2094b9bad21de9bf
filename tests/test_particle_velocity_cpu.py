"""Per-particle velocity output, the parts that need no GPU: the library exports mpm_retrieve_velocity and the header declares it, the
Python layer binds it, and the BGEO writer's frame with a "v" point attribute is byte for byte the one partio writes
(tests/golden/g10_partio_v.bgeo, made by tests/golden/gen/gen_bgeo_v.sh with the reference's own partio)."""
import os
import re
import struct
import subprocess

import numpy as np

from claymore_amd import _ffi
from claymore_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "claymore_amd", "host")
GOLD = os.path.join(ROOT, "tests", "golden")


def read_bgeo_v(path):
    """Reader for a classic BGEO v5 frame with exactly one point attribute, the 3-float vector "v" (Externals/partio/io/BGEO.cpp:311-407)."""
    raw = open(path, "rb").read()
    magic, vchar, version, npoints = struct.unpack(">IcII", raw[:13])
    assert magic == 0x4267656F and vchar == b"V" and version == 5
    assert struct.unpack(">7I", raw[13:41]) == (0, 0, 0, 1, 0, 0, 0)      # nPrims, groups, ONE point attribute, nothing else
    assert raw[41:62] == struct.pack(">h", 1) + b"v" + struct.pack(">Hi3i", 3, 5, 0, 0, 0)   # name, size 3, vector, zero defaults
    pts = np.frombuffer(raw[62:62 + 28 * npoints], dtype=">f4").reshape(npoints, 7)
    assert np.all(pts[:, 3] == 1.0)
    assert raw[62 + 28 * npoints:] == b"\x00\xff"
    return pts[:, :3].astype(np.float32), pts[:, 4:].astype(np.float32)


def test_library_exports_retrieve_velocity_and_header_declares_it():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    assert re.search(r"\bT mpm_retrieve_velocity$", out, re.M), "mpm_retrieve_velocity is not exported"
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert re.search(r"int mpm_retrieve_velocity\(mpm_ctx\* ctx, int model, float\* xyz, float\* vel, float\* affine9, size_t\* n\);", hdr)
    assert "retrieve_velocity" in _ffi.HIP_ONLY and "retrieve_velocity" not in _ffi.SIGNATURES     # (the oracle has no velocity readout)
    api = _ffi.load_hip()
    assert api.retrieve_velocity.restype is _ffi.C.c_int and len(api.retrieve_velocity.argtypes) == 6
    assert callable(Engine.retrieve_velocity) and callable(Engine.kinetic_energy)


def test_library_abi_number_is_unchanged():
    assert _ffi.load_hip().build_info().decode().startswith("claymore_hip abi7 ")


def _selftest(tmp_path):
    exe = tmp_path / "host_selftest"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", str(exe), os.path.join(HOST, "host_selftest.cpp")])
    return str(exe)


def test_bgeo_writer_with_velocity_equals_partio_byte_for_byte(tmp_path):
    exe = _selftest(tmp_path)
    out = tmp_path / "mine_v.bgeo"
    subprocess.check_call([exe, "--bgeo-v-from", os.path.join(GOLD, "g10_points.f32"), os.path.join(GOLD, "g10_velocity.f32"), str(out)])
    want = open(os.path.join(GOLD, "g10_partio_v.bgeo"), "rb").read()
    got = open(out, "rb").read()
    assert len(got) == len(want) == 41 + 21 + 28 * 1000 + 2
    assert got == want
    xyz, v = read_bgeo_v(os.path.join(GOLD, "g10_partio_v.bgeo"))
    assert np.array_equal(xyz, np.fromfile(os.path.join(GOLD, "g10_points.f32"), dtype=np.float32).reshape(-1, 3))
    assert np.array_equal(v.view(np.uint32), np.fromfile(os.path.join(GOLD, "g10_velocity.f32"), dtype=np.float32).reshape(-1, 3).view(np.uint32))


def test_bgeo_writer_without_velocity_is_unchanged(tmp_path):
    """The position-only path still writes partio's position-only frame (the existing fixture), next to the new one."""
    exe = _selftest(tmp_path)
    out = tmp_path / "mine.bgeo"
    subprocess.check_call([exe, "--bgeo-from", os.path.join(GOLD, "g10_points.f32"), str(out)])
    assert open(out, "rb").read() == open(os.path.join(GOLD, "g10_partio.bgeo"), "rb").read()
