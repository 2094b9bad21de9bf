"""The lane mapping of the 6^3 node cube (claymore_amd/csrc/mpm_cube_lane.hpp: cube_lane), restated in numpy and checked exhaustively.

Both G2P2G kernels stage the grid velocities of the block's 2 x 2 x 2 grid blocks into the gather arena and write the two scatter arenas back to the next
grid through this mapping: pass p = 0 .. 3 handles octants 2 p and 2 p + 1, lanes 0 .. 26 carry octant 2 p, lanes 32 .. 58 octant 2 p + 1, the node within an
octant is (i, j, k) = (l / 9, (l / 3) % 3, l % 3) with l = lane & 31, lanes with l >= 27 idle.  The node <-> (grid block, cell) correspondence has to be the one of
the per-octant loops this replaces (`for(lb = 0; lb < 8; ++lb)`, lane = cell, restated below from that source): low octant a = c - 1, high octant a = c + 3.

Also checked: the x86 build of the header (tools/hostcheck/check_cube.cpp) returns what the numpy restatement says.  (The write-back keeps one zero test per
channel, so nothing here has to argue that a zero mass sum implies zero momentum sums.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

G2P_STRIDE = (6, 1, 36)       # mpm_g2p2g.hpp: kG2PStrideX / Y / Z
P2G_STRIDE = (36, 6, 1)       # kP2GStrideX / Y, z = 1


def cube_lane(p, lane):
    """(on, octant, cell, gather-arena index, scatter-arena index) of (pass, lane): the new mapping"""
    l, h = lane & 31, (p >> 1, p & 1, lane >> 5)
    if l >= 27:
        return False, 0, 0, 0, 0
    n = (l // 9, (l // 3) % 3, l % 3)
    a = [n[d] + 3 * h[d] for d in range(3)]
    c = [n[d] + 1 - h[d] for d in range(3)]
    return True, 4 * h[0] + 2 * h[1] + h[2], 16 * c[0] + 4 * c[1] + c[2], sum(a[d] * G2P_STRIDE[d] for d in range(3)), sum(a[d] * P2G_STRIDE[d] for d in range(3))


def parent_nodes():
    """The per-octant loops of the parent: octant lb, lane = cell (cx, cy, cz) = (lane >> 4, (lane >> 2) & 3, lane & 3), arena coordinate
    a = c + (4 if the octant's bit is set) - 1, kept if 0 <= a < 6 on every axis.  -> {(octant, cell): (gather index, scatter index)}"""
    out = {}
    for lb in range(8):
        for lane in range(64):
            c = (lane >> 4, (lane >> 2) & 3, lane & 3)
            a = (c[0] + (4 if lb & 4 else 0) - 1, c[1] + (4 if lb & 2 else 0) - 1, c[2] + (4 if lb & 1 else 0) - 1)
            if all(0 <= x < 6 for x in a):
                out[lb, lane] = (a[0] * G2P_STRIDE[0] + a[1] * G2P_STRIDE[1] + a[2] * G2P_STRIDE[2], a[0] * P2G_STRIDE[0] + a[1] * P2G_STRIDE[1] + a[2] * P2G_STRIDE[2])
    return out


def test_the_active_lanes_hit_every_arena_node_exactly_once():
    rows = [cube_lane(p, lane) for p in range(4) for lane in range(64)]
    on = [r for r in rows if r[0]]
    assert len(on) == 4 * 54
    assert sorted(r[3] for r in on) == list(range(216))       # gather arena: a permutation of its 216 nodes
    assert sorted(r[4] for r in on) == list(range(216))       # scatter arenas
    for p in range(4):
        for lane in range(64):
            assert cube_lane(p, lane)[0] == ((lane & 31) < 27)


def test_each_pair_lands_where_the_per_octant_loop_put_it():
    old = parent_nodes()
    assert len(old) == 216
    new = {}
    for p in range(4):
        for lane in range(64):
            on, octant, cell, g, s = cube_lane(p, lane)
            if on:
                assert octant == 2 * p + (lane >> 5)          # lanes 0 .. 26: octant 2 p, lanes 32 .. 58: octant 2 p + 1
                assert 0 <= cell < 64
                assert (octant, cell) not in new
                new[octant, cell] = (g, s)
    assert new == old


def test_an_instruction_touches_three_cell_runs_in_two_rows():
    """What a two-octant atomic or load looks like to the memory system: per half, nine runs of three consecutive cells in ONE 256-B channel row."""
    for p in range(4):
        for half in range(2):
            cells = sorted(cube_lane(p, 32 * half + l)[2] for l in range(27))
            runs = [cells[i:i + 3] for i in range(0, 27, 3)]
            assert all(r[1] == r[0] + 1 and r[2] == r[0] + 2 for r in runs), (p, half, cells)


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    """tools/hostcheck/check_cube.cpp: mpm_cube_lane.hpp built for x86."""
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostcube.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "hostcheck"), "-I" + entry.CSRC, "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "check_cube.cpp")])
    return C.CDLL(out)


def test_the_header_says_what_the_model_says(hostlib):
    out = (C.c_int * 5)()
    for p in range(4):
        for lane in range(64):
            hostlib.host_cube_lane(p, lane, out)
            on, octant, cell, g, s = cube_lane(p, lane)
            assert bool(out[0]) == on, (p, lane)
            if on:
                assert tuple(out[1:5]) == (octant, cell, g, s), (p, lane, tuple(out))
            else:
                assert tuple(out[2:5]) == (0, 0, 0), (p, lane, tuple(out))     # idle lanes address node 0 / cell 0: inside every buffer

