"""Per-particle stress output, the parts that need no GPU: the library exports mpm_retrieve_stress and mpm_stress_totals and the header
declares them, the Python layer binds them, and the BGEO writer's frame with the point attributes "stress" (6 floats), "J", "pressure" and
"vonmises" is byte for byte the one partio writes (tests/golden/g10_partio_stress.bgeo, made by tests/golden/gen/gen_bgeo_stress.sh with the
reference's own partio)."""
import os
import re
import struct
import subprocess

import numpy as np

from claymore_amd import _ffi
from claymore_amd.engine import Engine
from claymore_amd.mgsp import MgspGroupRank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "claymore_amd", "host")
GOLD = os.path.join(ROOT, "tests", "golden")
STRESS_ATTRS = (("stress", 6), ("J", 1), ("pressure", 1), ("vonmises", 1))


def read_bgeo_attrs(path):
    """Reader for a classic BGEO v5 frame with float / vector point attributes (Externals/partio/io/BGEO.cpp:311-407): (xyz, {name: (n, size)})."""
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
        assert kind in (0, 5) and raw[at + 8 + ln:at + 8 + ln + 4 * size] == b"\x00" * (4 * size)       # float or vector, zero defaults
        attrs.append((name, size))
        at += 8 + ln + 4 * size
    width = 4 + sum(s for _, s in attrs)
    pts = np.frombuffer(raw[at:at + 4 * width * npoints], dtype=">f4").reshape(npoints, width)
    assert np.all(pts[:, 3] == 1.0) and raw[at + 4 * width * npoints:] == b"\x00\xff"
    out, col = {}, 4
    for name, size in attrs:
        out[name] = pts[:, col:col + size].astype(np.float32)
        col += size
    return pts[:, :3].astype(np.float32), out


def test_library_exports_the_stress_readouts_and_header_declares_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    assert re.search(r"\bT mpm_retrieve_stress$", out, re.M), "mpm_retrieve_stress is not exported"
    assert re.search(r"\bT mpm_stress_totals$", out, re.M), "mpm_stress_totals is not exported"
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert "int mpm_retrieve_stress(mpm_ctx* ctx, int model, float* xyz, float* stress6, float* scalars3, size_t* n);" in hdr
    assert "int mpm_stress_totals(mpm_ctx* ctx, int model /* -1: all */, double out[8]);" in hdr
    for name, nargs in (("retrieve_stress", 6), ("stress_totals", 3)):
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES          # (the oracle has no stress readout)
        fn = getattr(_ffi.load_hip(), name)
        assert fn.restype is _ffi.C.c_int and len(fn.argtypes) == nargs
    assert callable(Engine.retrieve_stress) and callable(Engine.stress_totals)
    assert callable(MgspGroupRank.retrieve_stress) and callable(MgspGroupRank.stress_totals)


def test_library_abi_number_is_unchanged():
    assert _ffi.load_hip().build_info().decode().startswith("claymore_hip abi7 ")


def _selftest(tmp_path):
    exe = tmp_path / "host_selftest"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", str(exe), os.path.join(HOST, "host_selftest.cpp")])
    return str(exe)


def test_bgeo_writer_with_stress_attributes_equals_partio_byte_for_byte(tmp_path):
    exe = _selftest(tmp_path)
    out = tmp_path / "mine_stress.bgeo"
    subprocess.check_call([exe, "--bgeo-stress-from", os.path.join(GOLD, "g10_points.f32"), os.path.join(GOLD, "g10_stress.f32"), str(out)])
    want = open(os.path.join(GOLD, "g10_partio_stress.bgeo"), "rb").read()
    got = open(out, "rb").read()
    header = sum(2 + len(name) + 2 + 4 + 4 * size for name, size in STRESS_ATTRS)
    assert len(got) == len(want) == 41 + header + (4 + 9) * 4 * 1000 + 2
    assert got == want
    xyz, attrs = read_bgeo_attrs(os.path.join(GOLD, "g10_partio_stress.bgeo"))
    assert [(k, v.shape[1]) for k, v in attrs.items()] == list(STRESS_ATTRS)
    assert np.array_equal(xyz, np.fromfile(os.path.join(GOLD, "g10_points.f32"), dtype=np.float32).reshape(-1, 3))
    nine = np.fromfile(os.path.join(GOLD, "g10_stress.f32"), dtype=np.float32).reshape(-1, 9)
    assert np.array_equal(np.concatenate(list(attrs.values()), axis=1).view(np.uint32), nine.view(np.uint32))


def test_bgeo_writer_without_the_attributes_is_unchanged(tmp_path):
    """The position-only path still writes partio's position-only frame (the existing fixture), next to the new one."""
    exe = _selftest(tmp_path)
    out = tmp_path / "mine.bgeo"
    subprocess.check_call([exe, "--bgeo-from", os.path.join(GOLD, "g10_points.f32"), str(out)])
    assert open(out, "rb").read() == open(os.path.join(GOLD, "g10_partio.bgeo"), "rb").read()
