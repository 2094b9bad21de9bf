"""The analytic collision shapes of claymore_amd/csrc/mpm_collision_shapes.hpp and the response of mpm_collision.hpp, restated with numpy
float32 arrays statement for statement from the headers' comments (every operation rounded to float32, no contraction), and beside them the
float64 closed forms of include/claymore_amd.h.  Not a test: tests/test_collision_shapes_cpu.py judges the x86 build of the headers against
this model and this model against the closed forms; tests/test_collision_shapes_gpu.py judges the kernels against it.

The pose (collision_pose, computed by the library on the host once per grid update) calls libm's cosf / sinf; the model calls the same
two functions through ctypes, so a pose at T != 0 has the library's bits."""
import ctypes as C
import ctypes.util

import numpy as np

import grid_update_model as gm

F32 = np.float32
HALFSPACE, SPHERE, BOX, CAPSULE = 1, 2, 3, 4
KINDS = {"halfspace": HALFSPACE, "sphere": SPHERE, "box": BOX, "capsule": CAPSULE}
STICKY, SLIP, SEPARATE = 0, 1, 2
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _fn in (_libm.cosf, _libm.sinf):
    _fn.restype, _fn.argtypes = C.c_float, [C.c_float]


def f3(v):
    return np.asarray(v, dtype=np.float32).reshape(3)


def collider(kind, a=(0, 0, 0), b=(0, 0, 0), radius=0.0, inside_out=False, type=STICKY, friction=0.3, scale=1.0, dsdt=0.0, trans=(0, 0, 0),
             trans_vel=(0, 0, 0), omega=(0, 0, 0), rot_mat=None, time=0.0):
    """One collider as the library holds it after install: float32 fields, a half-space's normal normalised (b / sqrtf(b . b)); b_given is
    what the caller hands to the library."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    b = b_given = f3(b)
    if kind == HALFSPACE:
        b = (b / np.sqrt(F32(F32(b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]))).astype(np.float32)
    return dict(kind=kind, a=f3(a), b=b, b_given=b_given, radius=F32(radius), inside_out=bool(inside_out), type=int(type), friction=F32(friction), scale=F32(scale),
                dsdt=F32(dsdt), trans=f3(trans), trans_vel=f3(trans_vel), omega=f3(omega),
                rot=(np.eye(3, dtype=np.float32).ravel() if rot_mat is None else np.asarray(rot_mat, dtype=np.float32).ravel().copy()), time=F32(time))


def engine_kwargs(c):
    """The collider as keyword arguments of Engine.set_collision_shape."""
    return dict(kind=c["kind"], a=c["a"], b=c["b_given"], radius=float(c["radius"]), inside_out=c["inside_out"], type=c["type"], friction=float(c["friction"]),
                scale=float(c["scale"]), dsdt=float(c["dsdt"]), trans=c["trans"], trans_vel=c["trans_vel"], omega=c["omega"], rot_mat=c["rot"], time=float(c["time"]))


def pose(c, t):
    """collision_pose: shift = trans + trans_vel t; inv = 1 / (1 + dsdt t); growth = dsdt / scale; rot = start orientation x Rx Ry Rz."""
    t = F32(t)
    p = dict(shift=(c["trans"] + c["trans_vel"] * t).astype(np.float32), inv=F32(F32(1) / F32(F32(1) + c["dsdt"] * t)), growth=F32(c["dsdt"] / c["scale"]))
    rot = c["rot"].copy()
    if t != 0:
        for dim in range(3):
            tmp = np.zeros(9, np.float32)
            ang = F32(c["omega"][dim] * t)
            co, si = F32(_libm.cosf(float(ang))), F32(_libm.sinf(float(ang)))
            if dim == 0:
                tmp[0], tmp[4], tmp[8], tmp[7], tmp[5] = 1, co, co, si, -si
            elif dim == 1:
                tmp[4], tmp[0], tmp[8], tmp[2], tmp[6] = 1, co, co, si, -si
            else:
                tmp[8], tmp[0], tmp[4], tmp[3], tmp[1] = 1, co, co, si, -si
            prev = rot.copy()
            for j in range(3):
                for i in range(3):
                    rot[3 * j + i] = F32(F32(F32(prev[i] * tmp[3 * j]) + F32(prev[3 + i] * tmp[3 * j + 1])) + F32(prev[6 + i] * tmp[3 * j + 2]))
    p["rot"] = rot
    return p


def _dot3(a0, a1, a2, b0, b1, b2):
    """(a0 b0 + a1 b1) + a2 b2, every operation rounded."""
    return ((a0 * b0).astype(np.float32) + (a1 * b1).astype(np.float32)).astype(np.float32) + (a2 * b2).astype(np.float32)


def material_point(c, p, X):
    """collision_material_point: X (n, 3) float32 -> xmt, x."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        xmt = (X - p["shift"][None]).astype(np.float32)
        x0 = (xmt * p["inv"]).astype(np.float32)
        r = p["rot"]
        x = np.stack([_dot3(r[3 * i], r[3 * i + 1], r[3 * i + 2], x0[:, 0], x0[:, 1], x0[:, 2]) for i in range(3)], axis=1).astype(np.float32)
        x = ((x * c["scale"]).astype(np.float32) + c["trans"][None]).astype(np.float32)
    return xmt, x


def _round(d, r):
    """shape_round."""
    ln = np.sqrt(_dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2]).astype(np.float32)).astype(np.float32)
    sdis = (ln - r).astype(np.float32)
    pos = ln > 0
    n = np.where(pos[:, None], (d / np.where(pos, ln, F32(1))[:, None]).astype(np.float32), F32(0)).astype(np.float32)
    return sdis, n


def query(c, x):
    """shape_query: x (n, 3) float32 material points -> sdis (n,), n (n, 3)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    a, b, kind = c["a"], c["b"], c["kind"]
    with np.errstate(all="ignore"):
        if kind == HALFSPACE:
            d = (x - a[None]).astype(np.float32)
            sdis = _dot3(d[:, 0], d[:, 1], d[:, 2], b[0], b[1], b[2]).astype(np.float32)
            n = np.broadcast_to(b[None], x.shape).astype(np.float32)
        elif kind == SPHERE:
            sdis, n = _round((x - a[None]).astype(np.float32), c["radius"])
        elif kind == BOX:
            p = (x - a[None]).astype(np.float32)
            q = (np.abs(p) - b[None]).astype(np.float32)
            sg = np.where(p < 0, F32(-1), F32(1)).astype(np.float32)
            inside = (q[:, 0] <= 0) & (q[:, 1] <= 0) & (q[:, 2] <= 0)
            one = q[:, 1] > q[:, 0]
            m1 = np.where(one, q[:, 1], q[:, 0])
            two = q[:, 2] > m1
            s_in = np.where(two, q[:, 2], m1)
            zero = np.zeros_like(s_in)
            n_in = np.stack([np.where(~one & ~two, sg[:, 0], zero), np.where(one & ~two, sg[:, 1], zero), np.where(two, sg[:, 2], zero)], axis=1)
            o = np.where(q < 0, F32(0), q).astype(np.float32)
            ln = np.sqrt(_dot3(o[:, 0], o[:, 1], o[:, 2], o[:, 0], o[:, 1], o[:, 2]).astype(np.float32)).astype(np.float32)
            pos = ln > 0
            n_out = np.where(pos[:, None], (sg * (o / np.where(pos, ln, F32(1))[:, None]).astype(np.float32)).astype(np.float32), F32(0))
            sdis = np.where(inside, s_in, ln).astype(np.float32)
            n = np.where(inside[:, None], n_in, n_out).astype(np.float32)
        elif kind == CAPSULE:
            e = (b - a).astype(np.float32)
            p = (x - a[None]).astype(np.float32)
            den = F32(F32(F32(e[0] * e[0]) + F32(e[1] * e[1])) + F32(e[2] * e[2]))
            t = (_dot3(p[:, 0], p[:, 1], p[:, 2], e[0], e[1], e[2]).astype(np.float32) / den).astype(np.float32)
            t = np.where(t < 0, F32(0), t)
            t = np.where(t > 1, F32(1), t).astype(np.float32)
            d = (p - (t[:, None] * e[None]).astype(np.float32)).astype(np.float32)
            sdis, n = _round(d, c["radius"])
        else:
            raise ValueError(kind)
        if c["inside_out"]:
            sdis, n = (-sdis).astype(np.float32), (-n).astype(np.float32)
    return sdis, n


def _cross(a, b):
    """col_cross (sic): plus signs.  a (3,) or (n, 3), b (n, 3)."""
    a = np.broadcast_to(np.asarray(a, np.float32), b.shape)
    return np.stack([((a[:, 1] * b[:, 2]).astype(np.float32) + (a[:, 2] * b[:, 1]).astype(np.float32)).astype(np.float32),
                     ((a[:, 2] * b[:, 0]).astype(np.float32) + (a[:, 0] * b[:, 2]).astype(np.float32)).astype(np.float32),
                     ((a[:, 0] * b[:, 1]).astype(np.float32) + (a[:, 1] * b[:, 0]).astype(np.float32)).astype(np.float32)], axis=1)


def respond(c, p, xmt, x, n, vel, hit):
    """collision_respond on the rows where `hit`; the other rows keep their bits."""
    vel = np.asarray(vel, dtype=np.float32).reshape(-1, 3)
    r, typ, fr = p["rot"], c["type"], c["friction"]
    with np.errstate(all="ignore"):
        v_obj = _cross(c["omega"], xmt)
        v_obj = (v_obj + (xmt * p["growth"]).astype(np.float32)).astype(np.float32)
        radius = (x - c["trans"][None]).astype(np.float32)
        mat_vel = (_cross(c["omega"], radius) + c["trans_vel"][None]).astype(np.float32)
        rv = np.stack([_dot3(r[i], r[3 + i], r[6 + i], mat_vel[:, 0], mat_vel[:, 1], mat_vel[:, 2]) for i in range(3)], axis=1).astype(np.float32)
        v_obj = (v_obj + ((rv * c["scale"]).astype(np.float32) + c["trans_vel"][None]).astype(np.float32)).astype(np.float32)
        v = (vel - v_obj).astype(np.float32)
        zero = np.zeros_like(v)
        if typ == STICKY:
            out = (zero + v_obj).astype(np.float32)
        else:
            early = (n == 0).all(axis=1) if typ == SEPARATE else np.zeros(len(v), bool)
            nr = np.stack([_dot3(r[i], r[3 + i], r[6 + i], n[:, 0], n[:, 1], n[:, 2]) for i in range(3)], axis=1).astype(np.float32)
            vdn = _dot3(nr[:, 0], nr[:, 1], nr[:, 2], v[:, 0], v[:, 1], v[:, 2]).astype(np.float32)
            project = np.ones(len(v), bool) if typ == SLIP else (vdn < 0)
            w = (v - (nr * vdn[:, None]).astype(np.float32)).astype(np.float32)
            fric = ((fr > 0) & (vdn < 0)) if typ == SLIP else np.full(len(v), fr != 0)
            vn = np.sqrt(_dot3(w[:, 0], w[:, 1], w[:, 2], w[:, 0], w[:, 1], w[:, 2]).astype(np.float32)).astype(np.float32)
            slide = ((-vdn) * fr).astype(np.float32) < vn
            wf = (w + ((w / vn[:, None]).astype(np.float32) * (vdn * fr).astype(np.float32)[:, None]).astype(np.float32)).astype(np.float32)
            w = np.where((project & fric)[:, None], np.where(slide[:, None], wf, zero), w)
            v = np.where(project[:, None], w, v)
            out = np.where(early[:, None], zero, (v + v_obj).astype(np.float32)).astype(np.float32)
    res = vel.copy()
    res[hit] = out[hit]
    return res


def resolve(c, t, X, vel):
    """shape_resolve of one collider at time t on the domain points X: -> velocities, touched."""
    p = pose(c, t)
    xmt, x = material_point(c, p, X)
    sdis, n = query(c, x)
    hit = sdis <= 0                       # (a NaN touches nothing)
    return respond(c, p, xmt, x, n, vel, hit), hit


def field_resolve(c, t, nodes, dx, boundary, G, sdf, grad, vel):
    """collision_resolve (the level set) for an object whose pose takes every node to node * dx exactly (identity pose at bits 6): the
    trilinear interpolation returns the node's own sample {sdf, grad}; the gradient is normalised again; query_sdf's box applies."""
    p = pose(c, t)
    X = (nodes.astype(np.float32) * F32(dx)).astype(np.float32)
    xmt, x = material_point(c, p, X)
    lo, hi = F32(F32(F32(boundary) * F32(dx)) * F32(4)), F32(F32(F32(G - boundary) * F32(4)) * F32(dx))
    inbox = ((x >= lo) & (x < hi)).all(axis=1)
    nd = np.clip(nodes, 0, sdf.shape[0] - 1)
    s = sdf[nd[:, 0], nd[:, 1], nd[:, 2]].astype(np.float32)
    g = np.stack([grad[d][nd[:, 0], nd[:, 1], nd[:, 2]] for d in range(3)], axis=1).astype(np.float32)
    with np.errstate(all="ignore"):
        nn = np.sqrt(_dot3(g[:, 0], g[:, 1], g[:, 2], g[:, 0], g[:, 1], g[:, 2]).astype(np.float32)).astype(np.float32)
        n = (g / nn[:, None]).astype(np.float32)
    hit = inbox & (s <= 0)
    return respond(c, p, xmt, x, n, vel, hit), hit


def sample_field(c, N, dx):
    """The level set of a shape sampled at the nodes (identity pose) FROM THE FLOAT32 MODEL: sdf (N, N, N), grad (3, N, N, N)."""
    idx = np.stack(np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij"), axis=-1).reshape(-1, 3)
    sdis, n = query(c, (idx.astype(np.float32) * F32(dx)).astype(np.float32))
    return sdis.reshape(N, N, N), np.ascontiguousarray(n.T.reshape(3, N, N, N))


def grid_update(keys, G, boundary, gravity, dt, grid, colliders, t, dx, field=None):
    """grid_cell(ShapeArgs) over a whole grid: walls and gravity (the strict statements), the level-set object `field` = (collider, sdf, grad) if
    given, then the colliders in order (None: an empty slot), all at time t.  -> live, the grid afterwards, the returned doubled maximum, and
    per collider the touched live cells (nbc, 64)."""
    live, out, _ = gm.plain(keys, G, boundary, gravity, dt, grid)
    out = out.copy()
    nodes = gm.node_coords(keys).transpose(0, 2, 1).reshape(-1, 3)             # (nbc * 64, 3), row = block * 64 + cell
    vel = np.ascontiguousarray(out[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    X = (nodes.astype(np.float32) * F32(dx)).astype(np.float32)
    lv = live.reshape(-1)
    hits = []
    if field is not None:
        new, hit = field_resolve(field[0], t, nodes, dx, boundary, G, field[1], field[2], vel)
        vel = np.where(lv[:, None], new, vel)
        hits.append((hit & lv).reshape(live.shape))
    for c in colliders:
        if c is None:
            continue
        new, hit = resolve(c, t, X, vel)
        vel = np.where(lv[:, None], new, vel)
        hits.append((hit & lv).reshape(live.shape))
    out[:, 1:4] = vel.reshape(len(keys), 64, 3).transpose(0, 2, 1)
    q = gm.collision_q32(out[:, 1], out[:, 2], out[:, 3])[live]
    return live, out, (F32(q.max()) if q.size else F32(0.0)), hits


# ---- the float64 closed forms (include/claymore_amd.h) ------------------------------------------------------------------------------------
def closed_form(c, x):
    """sdis, n in float64 at the material points x (n, 3) for the collider's float32 parameters."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    a, b, r = c["a"].astype(np.float64), c["b"].astype(np.float64), float(c["radius"])
    with np.errstate(all="ignore"):
        if c["kind"] == HALFSPACE:
            bh = b / np.linalg.norm(b)
            sdis, n = (x - a) @ bh, np.broadcast_to(bh, x.shape).copy()
        elif c["kind"] in (SPHERE, CAPSULE):
            d = x - a
            if c["kind"] == CAPSULE:
                e = b - a
                t = np.clip((d @ e) / (e @ e), 0.0, 1.0)
                d = d - t[:, None] * e
            ln = np.linalg.norm(d, axis=1)
            sdis, n = ln - r, np.where(ln[:, None] > 0, d / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
        else:
            p = x - a
            q = np.abs(p) - b
            sg = np.where(p < 0, -1.0, 1.0)
            inside = (q <= 0).all(axis=1)
            ax = np.argmax(q, axis=1)                                                           # (ties: the lowest axis)
            n_in = np.zeros_like(x)
            n_in[np.arange(len(x)), ax] = sg[np.arange(len(x)), ax]
            o = np.maximum(q, 0.0)
            ln = np.linalg.norm(o, axis=1)
            n_out = np.where(ln[:, None] > 0, sg * o / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
            sdis, n = np.where(inside, q.max(axis=1), ln), np.where(inside[:, None], n_in, n_out)
        if c["inside_out"]:
            sdis, n = -sdis, -n
    return sdis, n


def extent(c):
    """The length scale errors of a shape are measured in: the largest magnitude among its parameters and the points queried is taken by
    the caller; this is the shape's own part."""
    return float(max(np.abs(c["a"]).max(), np.abs(c["b"]).max() if c["kind"] != SPHERE else 0.0, float(c["radius"])))


# ---- the colliders and points both test files use (bits 6: dx = 1 / 64, every coordinate below a multiple of dx) ----------------------------
DX = 1.0 / 64
_cz, _sz, _cx, _sx = np.cos(0.3), np.sin(0.3), np.cos(0.2), np.sin(0.2)
TILT = (np.array([[_cz, -_sz, 0], [_sz, _cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, _cx, -_sx], [0, _sx, _cx]])).astype(np.float32).ravel()
T_MOVED = 0.37
# translated + rotated + scaled + growing, turning about the domain's centre; evaluated with the clock stopped at T_MOVED
MOVED = dict(trans=(0.5, 0.5, 0.5), trans_vel=(0.1, -0.05, 0.02), omega=(1.0, -0.5, 1.5), rot_mat=TILT, scale=1.125, dsdt=0.5, time=T_MOVED)
SHAPES = {
    # the solid is y <= 32 dx; node row 32 lies ON the surface (sdis == 0 touches)
    "halfspace": dict(kind="halfspace", a=(0.25, 32 * DX, 0.75), b=(0.0, 2.0, 0.0)),
    "halfspace_tilted": dict(kind="halfspace", a=(0.5, 0.5, 0.5), b=(1.0, -2.0, 0.5)),
    # its surface crosses the central blocks at z = 34 dx; node (32, 32, 34) lies ON it
    "sphere": dict(kind="sphere", a=(32 * DX, 32 * DX, 4 * DX), radius=30 * DX),
    # faces on node planes (x 2, 34 - through the central blocks; y, z 4, 60): sdis == 0 nodes, and ties of q wherever |y - 32| == |z - 32|
    "box": dict(kind="box", a=(18 * DX, 32 * DX, 32 * DX), b=(16 * DX, 28 * DX, 28 * DX)),
    "capsule": dict(kind="capsule", a=(30 * DX, 10 * DX, 12 * DX), b=(34 * DX, 12 * DX, 50 * DX), radius=21 * DX),
    "container": dict(kind="sphere", a=(32 * DX, 32 * DX, 60 * DX), radius=30 * DX, inside_out=True),
}
KIND_CASES = ("halfspace", "sphere", "box", "capsule")


def make(name, moved=False, **kw):
    return collider(**{**SHAPES[name], **(MOVED if moved else {}), **kw})


def special_points(c):
    """Material points where a shape's definition has a corner: (n, 3) float32."""
    a, b, r = c["a"].astype(np.float64), c["b"].astype(np.float64), float(c["radius"])
    pts = [a, a + [DX, 0, 0], a - [0, DX, 0]]
    if c["kind"] == SPHERE:
        pts += [a + [r, 0, 0], a - [0, r, 0], a + [0, 0, r]]                                                # the centre (n = 0) and the surface
    elif c["kind"] == CAPSULE:
        e = b - a
        pts += [a + s * e for s in (0.0, 0.25, 0.5, 1.0)]                                                   # axis points: n = 0
        pts += [a - 0.5 * e, a - 2 * e + [DX, 0, 0], b + 0.5 * e, b + 3 * e - [0, DX, 0]]                   # t clamped at both ends
        pts += [a + [0, 0, 0] + r * np.array([e[1], -e[0], 0]) / np.hypot(e[0], e[1])]                      # (near) the surface
    elif c["kind"] == BOX:
        pts += [a + b * s for s in ([1, 0, 0], [0, -1, 0], [0, 0, 1], [1, 1, 0], [-1, 1, 1], [1, -1, -1])]  # faces, an edge, corners: sdis == 0
        pts += [a + np.array(s) * b.min() * 0.5 for s in ([1, 1, 0], [1, -1, 0], [0, 1, 1], [-1, 0, 1], [1, 1, 1], [-1, -1, -1])]
        pts += [a + (b - 4 * DX) * s for s in ([1, 1, 0], [0, 1, -1], [1, 1, 1], [-1, 0, 1])]               # ties of q in two and three axes
        pts += [a + b * [2, 0.5, 0], a + b * [-2, -3, 0.5], a + b * [1.5, 1.5, -1.5]]                       # outside: face, edge and corner regions
    else:
        bh = b / np.linalg.norm(b)
        pts += [a + np.cross(bh, [0.3, 0.1, -0.2]), a + bh * DX, a - bh * DX]                               # on the plane and either side
    pts += [[np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [np.nan] * 3]
    return np.array(pts, dtype=np.float64).astype(np.float32)


def seeded_points(seed, n=4096):
    """Domain points in [-0.25, 1.25)^3, and every 16th one snapped to a node."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * 1.5 - 0.25
    p[::16] = np.rint(p[::16] * 64) / 64
    return p.astype(np.float32)
