"""Rigid bodies (claymore_amd/csrc/mpm_rigid_body.hpp) restated.  Not a test: tests/test_rigid_body_cpu.py judges the x86
build of the header against this model on bits and this model against closed forms; tests/test_rigid_body_gpu.py judges the kernels against it.

Two parts.  body_step and its helpers in float64, statement for statement from the header: Python floats are IEEE doubles, every operation is
rounded once and nothing is contracted, math.sqrt is correctly rounded - the bits are the header's.  And the float32 wrapper a body slot puts
around its collider's response, on top of collision_shape_model / collision_volume_model (material_point, query, respond) and
collider_load_model's rows."""
import math

import numpy as np

import collider_load_model as lm
import collision_shape_model as sm
import collision_volume_model as cvm
import grid_update_model as gm

F32 = np.float32
LOCKS = {"x": 1, "y": 2, "z": 4, "rx": 8, "ry": 16, "rz": 32}


# ---- float64: the step ------------------------------------------------------------------------------------------------------------------------
def rotation(q):
    """body_rotation: R(q) row-major, q = (w, x, y, z)."""
    w, x, y, z = (float(v) for v in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
            2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]


def world_apply(R, M, a):
    """body_world_apply: R M R^T a, every dot product (p0 + p1) + p2."""
    t = [(R[i] * a[0] + R[3 + i] * a[1]) + R[6 + i] * a[2] for i in range(3)]
    u = [(M[3 * i] * t[0] + M[3 * i + 1] * t[1]) + M[3 * i + 2] * t[2] for i in range(3)]
    return [(R[3 * i] * u[0] + R[3 * i + 1] * u[1]) + R[3 * i + 2] * u[2] for i in range(3)]


def finite(a):
    return (a - a) == 0.0


def invert_spd(M):
    """body_invert_spd: the inverse by cofactors in the header's order, or None."""
    c00, c01, c02 = M[4] * M[8] - M[5] * M[7], M[5] * M[6] - M[3] * M[8], M[3] * M[7] - M[4] * M[6]
    det = M[0] * c00 + M[1] * c01 + M[2] * c02
    if not (M[0] > 0.0) or not (M[0] * M[4] - M[1] * M[3] > 0.0) or not (det > 0.0) or not finite(det):
        return None
    return [c00 / det, (M[2] * M[7] - M[1] * M[8]) / det, (M[1] * M[5] - M[2] * M[4]) / det,
            c01 / det, (M[0] * M[8] - M[2] * M[6]) / det, (M[2] * M[3] - M[0] * M[5]) / det,
            c02 / det, (M[1] * M[6] - M[0] * M[7]) / det, (M[0] * M[4] - M[1] * M[3]) / det]


def constants(mass, inertia, com, gravity=True, lock=0, force=(0, 0, 0), torque=(0, 0, 0)):
    """body_constants on the float32 fields of mpm_rigid_body -> dict (None where the install refuses)."""
    mass = float(F32(mass))
    xx, yy, zz, xy, xz, yz = (float(F32(v)) for v in inertia)
    Ib = [xx, xy, xz, xy, yy, yz, xz, yz, zz]
    inv = invert_spd(Ib)
    if not (mass > 0.0) or not finite(mass) or inv is None:
        return None
    lock = sum(LOCKS[w] for w in lock.split()) if isinstance(lock, str) else int(lock)
    return dict(mass=mass, inv_mass=1.0 / mass, Ib=Ib, Ib_inv=inv, com=[float(F32(v)) for v in com], force=[float(F32(v)) for v in force],
                torque=[float(F32(v)) for v in torque], gravity=1 if gravity else 0, lock=lock)


def new_state():
    return dict(x=[0.0] * 3, q=[1.0, 0.0, 0.0, 0.0], v=[0.0] * 3, omega=[0.0] * 3, l=[0.0] * 3, J=[0.0] * 3, L=[0.0] * 3, touched_mass=0.0, max_mass_ratio=0.0,
                touched_nodes=0, updates=0)


def omega_of(s, c):
    """body_omega: omega = R Ib^-1 R^T l; locked components 0 and then l = R Ib R^T omega."""
    R = rotation(s["q"])
    s["omega"] = world_apply(R, c["Ib_inv"], s["l"])
    if c["lock"] & 56:
        for d in range(3):
            if c["lock"] & (8 << d):
                s["omega"][d] = 0.0
        s["l"] = world_apply(R, c["Ib"], list(s["omega"]))


def body_step(s, c, J, L, n_touched, m_touched, h, gravity):
    """body_step, in place; -> ok (every input and the new state finite)."""
    J, L, h, gravity = [float(v) for v in J], [float(v) for v in L], float(h), float(gravity)
    for d in range(3):
        s["v"][d] = s["v"][d] + (J[d] + h * c["force"][d]) * c["inv_mass"]
        if d == 1 and c["gravity"]:
            s["v"][d] = s["v"][d] + gravity * h
        if c["lock"] & (1 << d):
            s["v"][d] = 0.0
        s["x"][d] = s["x"][d] + h * s["v"][d]
    for d in range(3):
        s["l"][d] = (s["l"][d] + L[d]) + h * c["torque"][d]
    omega_of(s, c)
    w, x, y, z = s["q"]
    ox, oy, oz = s["omega"]
    hh = 0.5 * h
    dw = 0.0 - ((ox * x + oy * y) + oz * z)
    dx = (ox * w + oy * z) - oz * y
    dy = (oy * w + oz * x) - ox * z
    dz = (oz * w + ox * y) - oy * x
    nw, nx, ny, nz = w + hh * dw, x + hh * dx, y + hh * dy, z + hh * dz
    s2 = ((nw * nw + nx * nx) + ny * ny) + nz * nz
    ln = math.sqrt(s2) if s2 >= 0 else float("nan")
    with np.errstate(all="ignore"):
        s["q"] = [float(np.float64(v) / np.float64(ln)) for v in (nw, nx, ny, nz)]
    s["J"], s["L"] = list(J), list(L)
    s["touched_mass"] = float(m_touched)
    s["touched_nodes"] = int(n_touched)
    s["updates"] += 1
    ratio = float(m_touched) * c["inv_mass"]
    if ratio > s["max_mass_ratio"]:
        s["max_mass_ratio"] = ratio
    return all(finite(v) for v in J + L + s["x"] + s["v"] + s["l"] + s["omega"] + s["q"])


def pose_of(s):
    """body_pose: rot = float32 R^T in CollisionPose::rot's layout, shift, vel, omega float32."""
    R = rotation(s["q"])
    rot = np.array([R[3 * j + i] for i in range(3) for j in range(3)], dtype=np.float64).astype(np.float32)
    return dict(rot=rot, shift=np.array(s["x"]).astype(np.float32), vel=np.array(s["v"]).astype(np.float32), omega=np.array(s["omega"]).astype(np.float32), inv=F32(1), growth=F32(0))


def quaternion(R):
    """body_quaternion (Shepperd's branches, normalised)."""
    tr = R[0] + R[4] + R[8]
    if tr >= R[0] and tr >= R[4] and tr >= R[8]:
        q = [1.0 + tr, R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    elif R[0] >= R[4] and R[0] >= R[8]:
        q = [R[7] - R[5], 1.0 + R[0] - R[4] - R[8], R[1] + R[3], R[2] + R[6]]
    elif R[4] >= R[8]:
        q = [R[2] - R[6], R[1] + R[3], 1.0 - R[0] + R[4] - R[8], R[5] + R[7]]
    else:
        q = [R[3] - R[1], R[2] + R[6], R[5] + R[7], 1.0 - R[0] - R[4] + R[8]]
    ln = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v / ln for v in q]


def start(collider, c, t=0.0):
    """body_start: the state of a body made of `collider` (collision_shape_model's dict) while the clock stands at t."""
    p = sm.pose(collider, t)
    rot, shift = p["rot"].astype(np.float64), p["shift"].astype(np.float64)
    R = [float(rot[3 * j + i]) for i in range(3) for j in range(3)]
    s = new_state()
    s["q"] = quaternion(R)
    tr = collider["trans"].astype(np.float64)
    d = [c["com"][k] - float(tr[k]) for k in range(3)]
    for i in range(3):
        s["x"][i] = float(shift[i]) + ((R[3 * i] * d[0] + R[3 * i + 1] * d[1]) + R[3 * i + 2] * d[2])
        s["v"][i] = float(collider["trans_vel"][i])
    s["l"] = world_apply(rotation(s["q"]), c["Ib"], [float(v) for v in collider["omega"]])
    omega_of(s, c)
    return s


def state_of(d):
    """Engine.collider_body's dict as a model state."""
    return dict(x=d["position"].tolist(), q=d["orientation"].tolist(), v=d["velocity"].tolist(), omega=d["omega"].tolist(), l=d["angular_momentum"].tolist(),
                J=d["last_impulse"].tolist(), L=d["last_angular_impulse"].tolist(), touched_mass=d["last_touched_mass"], max_mass_ratio=d["max_mass_ratio"],
                touched_nodes=d["last_touched_nodes"], updates=d["updates"])


def state_words(s):
    """A state as the 26 float64 / int64 words of mpm_rigid_body_state, for comparisons on bits."""
    f = np.array(s["x"] + s["q"] + s["v"] + s["omega"] + s["l"] + s["J"] + s["L"] + [s["touched_mass"], s["max_mass_ratio"]], dtype=np.float64).view(np.uint64)
    return np.concatenate([f, np.array([s["touched_nodes"], s["updates"]], dtype=np.int64).view(np.uint64)])


# ---- float32: a body slot in the grid update ----------------------------------------------------------------------------------------------------
def body_collider(c, com):
    """The slot's collider as it travels with a body installed: trans = com, trans_vel = omega = 0."""
    return {**c, "trans": sm.f3(com), "trans_vel": sm.f3((0, 0, 0)), "omega": sm.f3((0, 0, 0))}


def body_resolve(c, p, X, vel):
    """The wrapper of mpm_rigid_body.hpp's load_cell around <shape|volume>_resolve: c = body_collider(...), p = pose_of(state).
       r = X - shift;  vb = vel + omega x r;  rel = velocity - vb;  r2 = resolve(rel);  velocity = r2 + vb where r2 differs from rel in its bits (a NaN differs)."""
    X, vel = np.asarray(X, np.float32), np.asarray(vel, np.float32)
    m = lambda a, b: (a * b).astype(np.float32)  # noqa: E731
    with np.errstate(all="ignore"):
        r = (X - p["shift"][None]).astype(np.float32)
        w, v = p["omega"], p["vel"]
        vb = np.stack([(v[0] + (m(w[1], r[:, 2]) - m(w[2], r[:, 1])).astype(np.float32)).astype(np.float32),
                       (v[1] + (m(w[2], r[:, 0]) - m(w[0], r[:, 2])).astype(np.float32)).astype(np.float32),
                       (v[2] + (m(w[0], r[:, 1]) - m(w[1], r[:, 0])).astype(np.float32)).astype(np.float32)], axis=1)
        rel = (vel - vb).astype(np.float32)
        xmt, x = sm.material_point(c, p, X)
        sdis, n = cvm.query(c, x) if c["kind"] == "volume" else sm.query(c, x)
        r2 = sm.respond(c, p, xmt, x, n, rel, sdis <= 0)
        changed = (r2.view(np.uint32) != rel.view(np.uint32)).any(axis=1) | np.isnan(r2).any(axis=1)   # on bits; a NaN differs
        out = np.where(changed[:, None], (r2 + vb).astype(np.float32), vel).astype(np.float32)
    return out, changed


def node_rows(keys, G, boundary, gravity, dt, grid, colliders, t, dx, field=None, bodies=None):
    """collider_load_model.node_rows with bodies: bodies = {slot: (com, pose)}; a body slot's collider is given as installed (before the re-pivot)."""
    bodies = bodies or {}
    grid = np.ascontiguousarray(grid, dtype=np.float32)
    n = len(keys) * 64
    w = gm.wall_flags(keys, G, boundary)
    wx, wy, wz = (np.broadcast_to(w[:, d, None], grid[:, 0].shape) for d in range(3))
    live, (v0, v1s, _, v2) = gm.cell_update(grid[:, 0], grid[:, 1], grid[:, 2], grid[:, 3], wx, wy, wz, gm.gdt32(gravity, dt))
    lv = live.reshape(-1)
    m = grid[:, 0].reshape(-1)
    with np.errstate(all="ignore"):
        inv = (F32(1.0) / np.where(live, grid[:, 0], F32(1.0))).astype(np.float32)
        quot = [gm.mul32(grid[:, 1 + d], inv) for d in range(3)]
        wall_dv = np.stack([np.where(wd, (F32(0.0) - q).astype(np.float32), F32(0.0)).reshape(-1) for wd, q in zip((wx, wy, wz), quot)], axis=1).astype(np.float32)
    nodes = gm.node_coords(keys).transpose(0, 2, 1).reshape(-1, 3)
    X = (nodes.astype(np.float32) * F32(dx)).astype(np.float32)
    vel = np.stack([v0.reshape(-1), v1s.reshape(-1), v2.reshape(-1)], axis=1).astype(np.float32)
    zero = np.zeros((n, 3), np.float32)
    dv, after, touched, used = [zero] * lm.ROWS, [zero] * lm.ROWS, [np.zeros(n, bool)] * lm.ROWS, [lm.WALLS]

    def touch(d):
        return lv & ~((d[:, 0] == 0) & (d[:, 1] == 0) & (d[:, 2] == 0))

    dv[lm.WALLS], after[lm.WALLS] = np.where(lv[:, None], wall_dv, zero), vel.copy()
    touched[lm.WALLS] = touch(dv[lm.WALLS])
    acting = ([(0, field)] if field is not None else []) + [(1 + s, c) for s, c in enumerate(colliders) if c is not None]
    for r, c in acting:
        with np.errstate(all="ignore"):
            if r == 0:
                new, _ = sm.field_resolve(c[0], t, nodes, dx, boundary, G, c[1], c[2], vel)
            elif r - 1 in bodies:
                com, p = bodies[r - 1]
                new, _ = body_resolve(body_collider(c, com), p, X, vel)
            else:
                new, _ = cvm.resolve(c, t, X, vel)
            new = np.where(lv[:, None], new, vel).astype(np.float32)
            dv[r] = np.where(lv[:, None], (new - vel).astype(np.float32), zero)
        vel = new
        after[r], touched[r] = vel.copy(), touch(dv[r])
        used.append(r)
    return dict(nodes=nodes, X=X, m=m, live=lv, dv=dv, after=after, touched=touched, used=used, v_final=vel)


# ---- float64 closed forms of the mass properties -------------------------------------------------------------------------------------------------
def sphere_mass(rho, r):
    m = rho * 4.0 / 3.0 * math.pi * r ** 3
    return m, [0.4 * m * r * r] * 3 + [0.0] * 3


def box_mass(rho, b):
    m = rho * 8.0 * b[0] * b[1] * b[2]
    return m, [m * (b[1] ** 2 + b[2] ** 2) / 3, m * (b[0] ** 2 + b[2] ** 2) / 3, m * (b[0] ** 2 + b[1] ** 2) / 3, 0.0, 0.0, 0.0]


def capsule_quadrature(rho, a, b, r, n):
    """Mass and the inertia tensor (3, 3) about the centre of a capsule by the midpoint rule over n slices along the axis: each slice a disc of
    radius rho(s) = sqrt(r^2 - (distance beyond the segment)^2), whose own inertia is known in closed form."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ln = np.linalg.norm(b - a)
    u = (b - a) / ln
    s = (np.arange(n) + 0.5) / n * (ln + 2 * r) - (ln / 2 + r)                              # along the axis, from the centre
    over = np.maximum(np.abs(s) - ln / 2, 0.0)
    rad2 = r * r - over * over
    dm = rho * math.pi * rad2 * (ln + 2 * r) / n
    m = dm.sum()
    Ia = (0.5 * dm * rad2).sum()
    It = (0.25 * dm * rad2 + dm * s * s).sum()
    uu = np.outer(u, u)
    return m, It * (np.eye(3) - uu) + Ia * uu, 0.5 * (a + b)
