// mpm_cube_lane.hpp — which node of the 6^3 node cube a lane carries when a G2P2G kernel stages the grid in or writes its arenas back.
//
// The cube (nodes 1..6 per axis of the 8^3 nodes around a particle block) lies across the block's 2 x 2 x 2 grid blocks ("octants"; octant o sits in lane
// 54 + o of the block's info row, o = 4 x-high + 2 y-high + z-high); an octant holds 3 x 3 x 3 of its nodes: cells 1..3 per axis of a low grid block,
// cells 0..2 of a high one.  A wave-instruction handles TWO octants: pass p = 0..3 takes octants 2 p (lanes 0..26) and 2 p + 1 (lanes 32..58), which differ in
// z only; the node within the octant is (i, j, k) = (l / 9, (l / 3) % 3, l % 3), l = lane & 31; lanes with l >= 27 are idle.  54 of 64 lanes work, four passes
// cover the cube; with lane = cell of ONE octant per instruction (27 of 64 lanes, eight passes) it took twice the instructions.
// Plain integer arithmetic, also built for x86 (tools/hostcheck/check_cube.cpp, tests/test_cube_lane_model.py).
#pragma once

namespace mpm {

struct CubeLane {
	bool on;	// the lane carries a node (idle lanes: every index below is 0, a valid address)
	int octant; // its grid block: lane 54 + octant of the info row
	int cell;	// its cell in that grid block (4 x 4 x 4, x slowest: the position in a 64-float channel row)
	int g2p;	// its node in the gather arena (strides 6 / 1 / 36)
	int p2g;	// its node in a scatter arena (strides 36 / 6 / 1)
};

#if defined(__HIPCC__)
__host__ __device__
#endif
	inline CubeLane
	cube_lane(int pass, int lane) {
	const int l = lane & 31;
	const int hx = pass >> 1, hy = pass & 1, hz = lane >> 5;// the octant's halves
	// (i, j, k) = (l / 9, (l / 3) % 3, l % 3) by comparisons: the compiler's small divisions are byte-select multiplies whose constants have to sit in vector
	// registers, and it keeps those across the particle loop
	const int i = (l >= 9) + (l >= 18), r = l - 9 * i;
	const int j = (r >= 3) + (r >= 6), k = r - 3 * j;
	const int ax = i + 3 * hx, ay = j + 3 * hy, az = k + 3 * hz;// arena coordinate: low a = c - 1, high a = c + 3
	const int cx = i + 1 - hx, cy = j + 1 - hy, cz = k + 1 - hz;
	CubeLane c;
	c.on	 = l < 27;
	c.octant = 4 * hx + 2 * hy + hz;
	c.cell	 = c.on ? cx * 16 + cy * 4 + cz : 0;
	c.g2p	 = c.on ? ax * 6 + ay + az * 36 : 0;
	c.p2g	 = c.on ? ax * 36 + ay * 6 + az : 0;
	return c;
}

}// namespace mpm
