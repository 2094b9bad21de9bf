"""The volume collider of claymore_amd/csrc/mpm_collision_volume.hpp - a local level-set box in a slot - restated with numpy float32 arrays
statement for statement from the header's comments (every operation rounded to float32, no contraction), on top of collision_shape_model's pose,
material_point and respond, heightfield_model's slots of mixed kinds and collision_mesh_model's field value at a point; beside it the float64
closed form: exact trilinear interpolation of the float32 table.  Not a test: tests/test_collision_volume_cpu.py judges the x86 build of the
header against this model and this model against the closed form; tests/test_collision_volume_gpu.py judges the kernels against it."""
import numpy as np

import collision_mesh_model as cm
import collision_shape_model as sm
import grid_update_model as gm
import heightfield_model as hm

F32 = np.float32
DX = sm.DX
MAX_SAMPLES, MAX_TABLE = 1024, 1 << 27


def volume(table, origin=(0.0, 0.0, 0.0), spacing=DX, inside_out=False, type=sm.STICKY, friction=0.3, scale=1.0, dsdt=0.0, trans=(0, 0, 0), trans_vel=(0, 0, 0),
           omega=(0, 0, 0), rot_mat=None, time=0.0):
    """One volume as the library holds it after install (collision_shape_model.collider's object fields, kind = "volume"); table (d0, d1, d2, 4)."""
    T = np.ascontiguousarray(table, dtype=np.float32)
    assert T.ndim == 4 and T.shape[3] == 4 and min(T.shape[:3]) >= 2
    return dict(kind="volume", table=T, origin=sm.f3(origin), spacing=F32(spacing), inside_out=bool(inside_out), type=int(type), friction=F32(friction), scale=F32(scale),
                dsdt=F32(dsdt), trans=sm.f3(trans), trans_vel=sm.f3(trans_vel), omega=sm.f3(omega),
                rot=(np.eye(3, dtype=np.float32).ravel() if rot_mat is None else np.asarray(rot_mat, dtype=np.float32).ravel().copy()), time=F32(time))


def engine_kwargs(c):
    """The volume as keyword arguments of Engine.set_collision_volume."""
    return dict(field4=c["table"], origin=tuple(float(v) for v in c["origin"]), spacing=float(c["spacing"]), inside_out=c["inside_out"], type=c["type"],
                friction=float(c["friction"]), scale=float(c["scale"]), dsdt=float(c["dsdt"]), trans=c["trans"], trans_vel=c["trans_vel"], omega=c["omega"], rot_mat=c["rot"],
                time=float(c["time"]))


def _mul(a, b):
    return (a * b).astype(np.float32)


def query(c, x):
    """volume_query: x (n, 3) float32 material points -> sdis (n,), n (n, 3)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    T, sp, dims = c["table"], c["spacing"], c["table"].shape[:3]
    with np.errstate(all="ignore"):
        xl = (x - c["origin"][None]).astype(np.float32)
        u = (xl / sp).astype(np.float32)
        inside = np.ones(len(x), bool)
        for d in range(3):
            inside &= (u[:, d] >= 0) & (u[:, d] <= F32(dims[d] - 1))                      # (a NaN is outside)
        cid, w = [], []
        for d in range(3):
            us = np.where(inside, u[:, d], F32(0))
            xs = np.where(inside, xl[:, d], F32(0))
            ci = np.minimum(us.astype(np.int32), dims[d] - 2)                              # (int) u truncates; u >= 0
            dis = (xs - _mul(ci.astype(np.float32), sp)).astype(np.float32)
            w1 = (dis / sp).astype(np.float32)
            cid.append(ci)
            w.append(((F32(1) - w1).astype(np.float32), w1))
        acc = np.zeros((len(x), 4), np.float32)
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    ww = _mul(_mul(w[0][i], w[1][j]), w[2][k])
                    v = T[cid[0] + i, cid[1] + j, cid[2] + k]
                    acc = (acc + _mul(ww[:, None], v)).astype(np.float32)
        sdis, g = acc[:, 0], acc[:, 1:]
        nn = np.sqrt(((_mul(g[:, 0], g[:, 0]) + _mul(g[:, 1], g[:, 1])).astype(np.float32) + _mul(g[:, 2], g[:, 2])).astype(np.float32)).astype(np.float32)
        n = (g / nn[:, None]).astype(np.float32)
        if c["inside_out"]:
            sdis, n = (-sdis).astype(np.float32), (-n).astype(np.float32)
        sdis = np.where(inside, sdis, F32(np.nan)).astype(np.float32)
        n = np.where(inside[:, None], n, F32(0)).astype(np.float32)
    return sdis, n


def footprint(c, x):
    """The query's footprint test alone: True where the material points x are inside."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = ((x - c["origin"][None]).astype(np.float32) / c["spacing"]).astype(np.float32)
    return np.all((u >= 0) & (u <= np.array(c["table"].shape[:3], np.float32)[None] - F32(1)), axis=1)


def resolve(c, t, X, vel):
    """volume_resolve (heightfield_resolve / shape_resolve for the other kinds) at time t on the domain points X: -> velocities, touched."""
    if c["kind"] != "volume":
        return hm.resolve(c, t, X, vel)
    p = sm.pose(c, t)
    xmt, x = sm.material_point(c, p, X)
    sdis, n = query(c, x)
    hit = sdis <= 0                                                                        # (a NaN touches nothing)
    return sm.respond(c, p, xmt, x, n, vel, hit), hit


def grid_update(keys, G, boundary, gravity, dt, grid, colliders, t, dx, field=None):
    """grid_cell(VolumeColliderArgs) over a whole grid: heightfield_model.grid_update with volumes among the slots' kinds.
    -> live, the grid afterwards, the returned doubled maximum, and per collider (the field first) the touched live cells (nbc, 64)."""
    live, out, _ = gm.plain(keys, G, boundary, gravity, dt, grid)
    out = out.copy()
    nodes = gm.node_coords(keys).transpose(0, 2, 1).reshape(-1, 3)
    vel = np.ascontiguousarray(out[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    X = (nodes.astype(np.float32) * F32(dx)).astype(np.float32)
    lv = live.reshape(-1)
    hits = []
    if field is not None:
        new, hit = sm.field_resolve(field[0], t, nodes, dx, boundary, G, field[1], field[2], vel)
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


# ---- the samples' positions, the auto-sized box, a table from a mesh ------------------------------------------------------------------------------
def sample_points(origin, spacing, dims):
    """p_d = origin_d + (float) i_d * spacing (one multiplication, one addition) of every sample, x slowest: (d0 d1 d2, 3) float32."""
    o, sp = sm.f3(origin), F32(spacing)
    ax = [(o[d] + _mul(np.arange(dims[d]).astype(np.float32), sp)).astype(np.float32) for d in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def autosize(verts, spacing, pad=2):
    """The host's box of a mesh install with dims == 0: float64 on the float32 vertices and spacing, the origin stored as float32.
    -> origin (3,) float32, dims (3 ints), ok (within the limits)."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    sp = float(F32(spacing))
    mn, mx = v.min(axis=0), v.max(axis=0)
    origin = (mn - pad * sp).astype(np.float32)
    dims = [int(np.ceil((mx[d] - mn[d]) / sp) + 2 * pad + 1) for d in range(3)]
    ok = all(2 <= n <= MAX_SAMPLES for n in dims) and dims[0] * dims[1] * dims[2] <= MAX_TABLE
    return origin, dims, ok


def mesh_table(mesh, origin, spacing, dims):
    """The table mpm_set_collision_volume_mesh builds: collision_mesh_model's field value (outward-signed) at every sample.
    -> table (d0, d1, d2, 4) float32, collision_mesh_model.Mesh.field's dict (for check_signs), the samples' positions."""
    p = sample_points(origin, spacing, dims)
    res = mesh.field(p)
    return res["out"].reshape(tuple(dims) + (4,)).astype(np.float32), res, p


# ---- the float64 closed form -------------------------------------------------------------------------------------------------------------------
def closed_form(c, x):
    """The four interpolated channels {sdis, g} (g NOT normalised, inside_out NOT applied) in float64 at the material points x (n, 3): exact
    trilinear interpolation of the float32 table.  -> val (n, 4), inside."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    T, sp, dims = c["table"].astype(np.float64), float(c["spacing"]), c["table"].shape[:3]
    u = (x - c["origin"].astype(np.float64)[None]) / sp
    inside = np.all((u >= 0) & (u <= np.array(dims)[None] - 1), axis=1)
    us = np.where(inside[:, None], u, 0.0)
    ci = np.minimum(us.astype(np.int64), np.array(dims)[None] - 2)
    f = us - ci
    val = np.zeros((len(x), 4))
    for i in range(2):
        for j in range(2):
            for k in range(2):
                w = (f[:, 0] if i else 1 - f[:, 0]) * (f[:, 1] if j else 1 - f[:, 1]) * (f[:, 2] if k else 1 - f[:, 2])
                val += w[:, None] * T[ci[:, 0] + i, ci[:, 1] + j, ci[:, 2] + k]
    return val, inside


# ---- the tables and points the test files use (bits 6: dx = 1 / 64) -------------------------------------------------------------------------------
def icosphere_mesh(centre=(0.47, 0.52, 0.55), radius=0.21, subdivisions=2):
    """claymore_amd.scenes.icosphere as a collision_mesh_model.Mesh: 320 triangles at two subdivisions."""
    from claymore_amd import scenes
    v, f = scenes.icosphere(centre, radius, subdivisions)
    return cm.Mesh(v, f)


_CACHE = {}


def tables():
    """name -> (table, origin, spacing).  "ico": the 13 x 9 x 18 samples, 0.037 apart (no multiple of dx), of a 320-triangle icosphere's field
    that the box cuts on several faces; "2x2x2": one cell of a seeded, tilted plane."""
    if not _CACHE:
        o, sp, dims = (0.26, 0.37, 0.21), 0.037, (13, 9, 18)
        _CACHE["ico"] = (mesh_table(icosphere_mesh(), o, sp, dims)[0], o, sp)
        pts = sample_points((0.25, 0.375, 0.25), 0.5, (2, 2, 2)).astype(np.float64)
        nrm = np.array([0.48, 0.6, -0.64])
        t = np.concatenate([((pts - 0.5) @ nrm)[:, None], np.broadcast_to(nrm, (8, 3))], axis=1).reshape(2, 2, 2, 4).astype(np.float32)
        _CACHE["2x2x2"] = (t, (0.25, 0.375, 0.25), 0.5)
    return _CACHE


def make(name, moved=False, **kw):
    T, origin, spacing = tables()[name]
    return volume(T, **{**dict(origin=origin, spacing=spacing), **(sm.MOVED if moved else {}), **kw})


def sphere_volume(dims=(45, 45, 45), origin=(-0.4, -0.4, -0.4), spacing=0.041, shape="sphere", moved=False, **kw):
    """The field of one of collision_shape_model's shapes (sdis and unit normal of the float32 model at the samples) as a volume: the body of
    the cell-by-cell tests, wider than the domain at both poses."""
    s = sm.make(shape)
    sd, n = sm.query(s, sample_points(origin, spacing, dims))
    T = np.concatenate([sd[:, None], n], axis=1).reshape(tuple(dims) + (4,)).astype(np.float32)
    return volume(T, **{**dict(origin=origin, spacing=spacing), **(sm.MOVED if moved else {}), **kw})


def special_points(c):
    """Material points where the query's definition has a corner: on samples, on cell faces, u = 0 and u = dims - 1 exactly and one float
    outside each on every axis, far outside, NaN coordinates (last three rows).  (n, 3) float32."""
    o, sp, dims = c["origin"], c["spacing"], c["table"].shape[:3]
    ax = [(o[d] + _mul(np.arange(dims[d]).astype(np.float32), sp)).astype(np.float32) for d in range(3)]
    inf = F32(np.inf)
    rng = np.random.default_rng(5)
    pts = []
    for _ in range(48):
        i, j, k = (int(rng.integers(0, dims[d])) for d in range(3))
        pts.append([ax[0][i], ax[1][j], ax[2][k]])                                                                  # on a sample
        if i + 1 < dims[0]:
            pts.append([F32(0.5) * (ax[0][i] + ax[0][i + 1]), ax[1][j], ax[2][k]])                                 # on a cell edge
        if k + 1 < dims[2]:
            pts.append([ax[0][i], ax[1][j], F32(0.25) * ax[2][k] + F32(0.75) * ax[2][k + 1]])
    mid = [ax[d][dims[d] // 2] for d in range(3)]
    for d in range(3):
        for v in (np.nextafter(ax[d][0], -inf), ax[d][0], ax[d][-1], np.nextafter(ax[d][-1], inf), ax[d][0] - sp, ax[d][-1] + sp):
            p = list(mid)
            p[d] = v
            pts.append(p)
    pts += [[ax[0][0], ax[1][0], ax[2][0]], [ax[0][-1], ax[1][-1], ax[2][-1]], [1e30, 0.0, 0.0], [0.0, 0.0, -1e30]]
    pts += [[np.nan, mid[1], mid[2]], [mid[0], np.nan, mid[2]], [np.nan] * 3]
    return np.array(pts, dtype=np.float64).astype(np.float32)


def seeded_points(c, t, seed=7, n=4096):
    """n seeded domain points: half of them anywhere in [-0.25, 1.25)^3 (every 16th snapped to a node), half of them with material points over
    the table's footprint widened by a tenth."""
    rng = np.random.default_rng(seed)
    free = sm.seeded_points(seed, n // 2)
    dims, o, sp = np.array(c["table"].shape[:3]), c["origin"].astype(np.float64), float(c["spacing"])
    x = o[None] + ((dims - 1) * sp)[None] * (1.2 * rng.random((n - n // 2, 3)) - 0.1)
    return np.concatenate([free, domain_points_of(c, t, x)]).astype(np.float32)


def domain_points_of(c, t, x):
    """Domain points X whose material points are (about) x: X = R (x - trans) / (scale inv) + shift, in float64."""
    p = sm.pose(c, t)
    R = p["rot"].astype(np.float64).reshape(3, 3)
    x0 = (np.asarray(x, np.float64) - c["trans"].astype(np.float64)) / float(c["scale"])
    return ((x0 @ R) / float(p["inv"]) + p["shift"].astype(np.float64)).astype(np.float32)


def query_points(c, t, moved):
    sp = special_points(c)
    return np.concatenate([seeded_points(c, t), sp if not moved else domain_points_of(c, t, sp)])
