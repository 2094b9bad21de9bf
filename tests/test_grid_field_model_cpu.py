"""The Eulerian readouts without a GPU: tests/grid_field_model.py against the definitions it restates, the ABI
surface of mpm_sample_grid / mpm_grid_volume / mpm_grid_box_totals, and the NumPy writer of the gmpm driver (claymore_amd/host/particle_io.hpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_field_model as gfm
from claymore_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "claymore_amd", "host")
BITS = 5                                     # 32 nodes, 8 blocks per axis
N = 1 << BITS
EPS = 2.0 ** -24


def neighbourhood(centre=(3, 3, 3)):
    return np.array([[centre[0] + a, centre[1] + b, centre[2] + c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.int32)


# ---- sample -------------------------------------------------------------------------------------------------------------------------------
def test_partition_of_unity_on_a_full_neighbourhood():
    """Constant mass 1 on the 3 x 3 x 3 blocks around block (3, 3, 3) - nodes 8 .. 19 per axis - samples to 1 wherever the stencil (nodes
    base .. base + 2, base = lround(p) - 1) stays inside: p in [8.5, 18.5)."""
    keys = neighbourhood()
    blocks = np.zeros((27, 4, 64), np.float32)
    blocks[:, 0] = 1.0
    m = gfm.GridField(keys, blocks, BITS)
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.uniform(8.5, 18.5, (20000, 3)), [[8.5, 8.5, 8.5], [18.499, 18.499, 18.499], [12.0, 12.5, 13.5]]])
    ref, S = m.sample((p / N).astype(np.float32))
    assert np.abs(ref[:, 0] - 1.0).max() <= 64 * EPS and not ref[:, 1:].any()
    assert np.array_equal(ref[:, 0], S[:, 0])
    # ... and falls off outside: a stencil with a row of nodes beyond the neighbourhood loses that row's weight
    ref, _ = m.sample(np.float32([[8.25 / N, 12.0 / N, 12.0 / N]]))             # base 7: node 7 holds nothing; fd = 1.25
    assert abs(ref[0, 0] - (1.0 - 0.5 * (1.5 - 1.25) ** 2)) < 1e-12


def test_lround_ties_pick_the_base_the_device_function_picks():
    """lround_pos is rint (ties to even) + 1 where p - rint(p) == +0.5 exactly: round half away from zero, for even and odd k - against
    floor(p + 0.5) in float64, which is exact for these float32 p."""
    k = np.arange(0, 130, dtype=np.float32)
    for p in (k + np.float32(0.5), np.nextafter(k + np.float32(0.5), np.float32(0)), np.nextafter(k + np.float32(0.5), np.float32(1e9)), k):
        assert np.array_equal(gfm.lround_pos(p), np.floor(p.astype(np.float64) + 0.5).astype(np.int64))
    assert gfm.lround_pos(np.float32([0.5, 1.5, 2.5, 3.5])).tolist() == [1, 2, 3, 4]          # even k: rint gives k, the tie rule adds one
    m = gfm.GridField(neighbourhood(), np.zeros((27, 4, 64), np.float32), BITS)
    valid, base, fd = m.stencil(np.float32([[10.5 / N, 11.5 / N, 0.5 / N], [0.0, 0.49 / N, (N - 0.5) / N]]))
    assert valid.all() and base.tolist() == [[10, 11, 0], [-1, -1, N - 1]] and fd[0].tolist() == [0.5, 0.5, 0.5]
    bad = np.float32([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], [-1e-9, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, 3e38]])
    assert not m.stencil(bad)[0].any()
    ref, S = m.sample(bad)
    assert not ref.any() and not S.any()


# ---- volume and totals --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hashed():
    """nbc = 30 hashed blocks: the neighbourhood of (3, 3, 3), two blocks at the upper corner of the domain and one at its upper y face; a 31st key stands
    for an EXTERIOR block (a number >= nbc in the table): the model is built from the first nbc alone, as mpm_dump_grid gives them."""
    keys = np.concatenate([neighbourhood(), [[7, 7, 7], [7, 7, 6], [1, 7, 6]], [[5, 5, 5]]]).astype(np.int32)
    nbc = 30
    return keys, nbc, gfm.GridField(keys[:nbc], gfm.hashed_blocks(nbc, 9), BITS)


@pytest.mark.parametrize("origin", [(0, 0, 0), (3, 5, 6), (-5, -2, -7)])
@pytest.mark.parametrize("s", [2, 4])
def test_strided_volumes_conserve_the_stride_1_total(hashed, s, origin):
    _, _, m = hashed
    dims = [(N + 8) // s] * 3
    fine = m.volume(origin, [s * d for d in dims], 1).astype(np.float64)
    want = fine.reshape(4, dims[0], s, dims[1], s, dims[2], s).sum(axis=(2, 4, 6))
    mag = np.abs(fine).reshape(4, dims[0], s, dims[1], s, dims[2], s).sum(axis=(2, 4, 6))
    got = m.volume(origin, dims, s)
    assert got.dtype == np.float32 and got.shape == (4,) + tuple(dims)
    assert (np.abs(got.astype(np.float64) - want) <= s ** 3 * EPS * mag).all()
    assert (mag > 0).sum() > 100
    assert abs(got.astype(np.float64).sum() - fine.sum()) <= s ** 3 * EPS * np.abs(fine).sum()


def test_box_leaving_the_domain_exterior_block_and_empty_box(hashed):
    keys, nbc, m = hashed
    v = m.volume((-3, N - 6, 20), (10, 9, 20), 1)                                # leaves through the lower x, upper y and upper z faces
    assert v.shape == (4, 10, 9, 20)
    assert not v[:, :3].any() and not v[:, :, 6:].any() and not v[:, :, :, 12:].any()
    assert np.array_equal(v[:, 3:, :6, :12].view(np.uint32), m.dense[:, 0:7, N - 6:N, 20:32]) and v[:, 3:, :6, :12].any()
    # the exterior-only block (5, 5, 5): nothing in the volume, nothing at a point whose stencil lies wholly inside it, nothing in its totals
    ex = keys[nbc]
    assert not m.volume(4 * ex, (4, 4, 4), 1).any()
    ref, S = m.sample(np.float32([(4 * ex + 1.5) / N]))                           # stencil: nodes 4 ex + {1, 2, 3}, in block ex alone
    assert not ref.any() and not S.any()
    out, mag = m.box_totals(4 * ex, 4 * ex + 4)
    assert not out.any() and not mag.any()
    # a registered block next to it does count; the whole domain is every block's sum
    out, mag = m.box_totals((-100, -100, -100), (1000, 1000, 1000))
    want = m.values().astype(np.float64)
    assert np.allclose(out[:4], want.reshape(4, -1).sum(axis=1), rtol=0, atol=1e-9 * mag[:4].max()) and out[0] > 0 and out[4] > 0
    assert mag[0] == out[0]                                                       # masses are positive
    for lo, hi in (((4, 4, 4), (4, 9, 9)), ((9, 9, 9), (4, 4, 4)), ((N, 0, 0), (N + 5, 5, 5)), ((-9, 0, 0), (0, 5, 5))):
        out, mag = m.box_totals(lo, hi)
        assert not out.any() and not mag.any(), (lo, hi)
    one, _ = m.box_totals((9, 10, 11), (10, 11, 12))
    node = m.values()[:, 9, 10, 11].astype(np.float64)
    assert np.array_equal(one[:4], node) and one[4] == (node[1] ** 2 + node[2] ** 2 + node[3] ** 2) / (2 * node[0])


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------------------
DECLARATIONS = ["int mpm_sample_grid(mpm_ctx* ctx, const float* xyz, size_t n, float* out4);",
                "int mpm_grid_volume(mpm_ctx* ctx, const int origin[3], const int dims[3], int stride, float* out);",
                "int mpm_grid_box_totals(mpm_ctx* ctx, const int lo[3], const int hi[3], double out[5]);"]
NAMES = ["sample_grid", "grid_volume", "grid_box_totals"]


def test_header_library_and_ffi_table():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "claymore_amd.h")).read(), flags=re.S)
    lines = [" ".join(l.split()) for l in txt.splitlines()]
    for d in DECLARATIONS:
        assert lines.count(d) == 1, d
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True).split()
    for n in NAMES:
        assert "mpm_" + n in exported, n
        assert n in _ffi.HIP_ONLY and n not in _ffi.SIGNATURES, n                 # HIP library only: the oracle has no counterpart
    hip = _ffi.load_hip()
    assert hip.build_info().decode().startswith("claymore_hip abi7 ")             # additive exports do not bump the ABI
    # before any context exists the three answer NOT_READY (a NULL context), without touching a device
    assert hip.sample_grid(None, None, 0, None) == _ffi.MPM_ERR_NOT_READY
    assert hip.grid_volume(None, None, None, 1, None) == _ffi.MPM_ERR_NOT_READY
    assert hip.grid_box_totals(None, None, None, None) == _ffi.MPM_ERR_NOT_READY


# ---- the NumPy writer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 1, 1, 1), (4, 8, 4, 2)])
def test_npy_writer_round_trip(tmp_path, shape):
    exe = tmp_path / "host_selftest"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", str(exe), os.path.join(HOST, "host_selftest.cpp")])
    bits = (np.arange(int(np.prod(shape)), dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x7FC00001)   # any pattern: NaNs, -0 ...
    bits[:3] = [0x80000000, 0x7FC01234, 0xFF800000]
    raw = tmp_path / "raw.f32"
    bits.tofile(raw)
    out = tmp_path / "grid_frame[1].npy"
    subprocess.check_call([str(exe), "--npy-from", str(raw)] + [str(d) for d in shape[1:]] + [str(out)])
    data = open(out, "rb").read()
    assert data[:8] == b"\x93NUMPY\x01\x00"                                       # format 1.0
    hlen = int.from_bytes(data[8:10], "little")
    assert (10 + hlen) % 64 == 0 and data[10 + hlen - 1:10 + hlen] == b"\n" and b"'descr': '<f4'" in data[10:10 + hlen] and b"'fortran_order': False" in data[10:10 + hlen]
    assert len(data) == 10 + hlen + 4 * bits.size
    got = np.load(out)
    assert got.dtype == np.dtype("<f4") and got.shape == shape and got.flags.c_contiguous
    assert np.array_equal(got.view(np.uint32).reshape(-1), bits)
    # a wrong element count is refused
    assert subprocess.run([str(exe), "--npy-from", str(raw), "9", "9", "9", str(tmp_path / "bad.npy")]).returncode == 5
