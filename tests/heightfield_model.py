"""The heightfield collider of claymore_amd/csrc/mpm_collision_heightfield.hpp restated with numpy float32 arrays statement for statement from
the header's comments (every operation rounded to float32, no contraction), on top of collision_shape_model's pose, material_point and respond,
and beside it the float64 closed form: exact bilinear interpolation of the float32 table.  Not a test: tests/test_collision_heightfield_cpu.py
judges the x86 build of the header against this model and this model against the closed form; tests/test_collision_heightfield_gpu.py judges
the kernels against it."""
import numpy as np

import collision_shape_model as sm
import grid_update_model as gm

F32 = np.float32
DX = sm.DX


def build_table(H, spacing):
    """heightfield_build: heights (nx, nz) -> table (nx, nz, 4) = {H, gx, gz, 0}."""
    H = np.ascontiguousarray(H, dtype=np.float32)
    sp = F32(spacing)
    two = F32(F32(2) * sp)
    with np.errstate(all="ignore"):
        gx, gz = np.empty_like(H), np.empty_like(H)
        gx[1:-1] = ((H[2:] - H[:-2]).astype(np.float32) / two).astype(np.float32)
        gx[0] = ((H[1] - H[0]).astype(np.float32) / sp).astype(np.float32)
        gx[-1] = ((H[-1] - H[-2]).astype(np.float32) / sp).astype(np.float32)
        gz[:, 1:-1] = ((H[:, 2:] - H[:, :-2]).astype(np.float32) / two).astype(np.float32)
        gz[:, 0] = ((H[:, 1] - H[:, 0]).astype(np.float32) / sp).astype(np.float32)
        gz[:, -1] = ((H[:, -1] - H[:, -2]).astype(np.float32) / sp).astype(np.float32)
    return np.stack([H, gx, gz, np.zeros_like(H)], axis=-1).astype(np.float32)


def heightfield(heights, origin=(0.0, 0.0), spacing=DX, inside_out=False, type=sm.STICKY, friction=0.3, scale=1.0, dsdt=0.0, trans=(0, 0, 0),
                trans_vel=(0, 0, 0), omega=(0, 0, 0), rot_mat=None, time=0.0):
    """One heightfield as the library holds it after install (collision_shape_model.collider's object fields, kind = "heightfield")."""
    H = np.ascontiguousarray(heights, dtype=np.float32)
    assert H.ndim == 2 and min(H.shape) >= 2
    return dict(kind="heightfield", heights=H, table=build_table(H, spacing), origin=np.asarray(origin, np.float32).reshape(2), spacing=F32(spacing),
                inside_out=bool(inside_out), type=int(type), friction=F32(friction), scale=F32(scale), dsdt=F32(dsdt), trans=sm.f3(trans), trans_vel=sm.f3(trans_vel),
                omega=sm.f3(omega), rot=(np.eye(3, dtype=np.float32).ravel() if rot_mat is None else np.asarray(rot_mat, dtype=np.float32).ravel().copy()), time=F32(time))


def engine_kwargs(c):
    """The heightfield as keyword arguments of Engine.set_collision_heightfield."""
    return dict(heights=c["heights"], origin=tuple(float(v) for v in c["origin"]), spacing=float(c["spacing"]), inside_out=c["inside_out"], type=c["type"],
                friction=float(c["friction"]), scale=float(c["scale"]), dsdt=float(c["dsdt"]), trans=c["trans"], trans_vel=c["trans_vel"], omega=c["omega"], rot_mat=c["rot"],
                time=float(c["time"]))


def _mul(a, b):
    return (a * b).astype(np.float32)


def query(c, x, want_h=False):
    """heightfield_query: x (n, 3) float32 material points -> sdis (n,), n (n, 3)  (and h with want_h)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    T, sp, (nx, nz) = c["table"], c["spacing"], c["heights"].shape
    with np.errstate(all="ignore"):
        u = ((x[:, 0] - c["origin"][0]).astype(np.float32) / sp).astype(np.float32)
        w = ((x[:, 2] - c["origin"][1]).astype(np.float32) / sp).astype(np.float32)
        inside = (u >= 0) & (u <= F32(nx - 1)) & (w >= 0) & (w <= F32(nz - 1))          # (a NaN is outside)
        us, ws = np.where(inside, u, F32(0)), np.where(inside, w, F32(0))
        i = np.minimum(us.astype(np.int32), nx - 2)                                    # (int) u truncates; u >= 0
        k = np.minimum(ws.astype(np.int32), nz - 2)
        fu, fw = (us - i.astype(np.float32)).astype(np.float32), (ws - k.astype(np.float32)).astype(np.float32)
        cu, cw = (F32(1) - fu).astype(np.float32), (F32(1) - fw).astype(np.float32)
        w00, w10, w01, w11 = _mul(cu, cw), _mul(fu, cw), _mul(cu, fw), _mul(fu, fw)
        t00, t10, t01, t11 = T[i, k], T[i + 1, k], T[i, k + 1], T[i + 1, k + 1]

        def chan(ch):
            return ((_mul(w00, t00[:, ch]) + _mul(w10, t10[:, ch])).astype(np.float32) + _mul(w01, t01[:, ch])).astype(np.float32) + _mul(w11, t11[:, ch])

        h, gx, gz = chan(0).astype(np.float32), chan(1).astype(np.float32), chan(2).astype(np.float32)
        ln = np.sqrt(((_mul(gx, gx) + F32(1)).astype(np.float32) + _mul(gz, gz)).astype(np.float32)).astype(np.float32)
        n = np.stack([((-gx) / ln).astype(np.float32), (F32(1) / ln).astype(np.float32), ((-gz) / ln).astype(np.float32)], axis=1)
        sdis = ((x[:, 1] - h).astype(np.float32) / ln).astype(np.float32)
        if c["inside_out"]:
            sdis, n = (-sdis).astype(np.float32), (-n).astype(np.float32)
        sdis = np.where(inside, sdis, F32(np.nan)).astype(np.float32)
        n = np.where(inside[:, None], n, F32(0)).astype(np.float32)
    return (sdis, n, np.where(inside, h, F32(np.nan)).astype(np.float32)) if want_h else (sdis, n)


def resolve(c, t, X, vel):
    """heightfield_resolve (or shape_resolve for a shape collider) at time t on the domain points X: -> velocities, touched."""
    if c["kind"] != "heightfield":
        return sm.resolve(c, t, X, vel)
    p = sm.pose(c, t)
    xmt, x = sm.material_point(c, p, X)
    sdis, n = query(c, x)
    hit = sdis <= 0                                                                    # (a NaN touches nothing)
    return sm.respond(c, p, xmt, x, n, vel, hit), hit


def grid_update(keys, G, boundary, gravity, dt, grid, colliders, t, dx, field=None):
    """grid_cell(TerrainArgs) over a whole grid: collision_shape_model.grid_update with shape and heightfield colliders mixed in slot order.
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


def sample_field(c, N, dx):
    """The level set of a heightfield whose samples sit on the grid nodes (origin 0, spacing dx, at least N samples per axis, floor),
    sampled at the nodes FROM THE FLOAT32 MODEL: sdf (N, N, N) = the model's sdis, grad (3, N, N, N) = (-gx, 1, -gz) of the table, NOT
    normalised.  At identity pose the level-set kernel's interpolation returns a node's own sample and normalises the gradient by
    sqrtf((gx gx + 1) + gz gz) - heightfield_query's own len, in its own order - so that the two kernels compute the same bits."""
    assert float(c["spacing"]) == dx and (c["origin"] == 0).all() and min(c["heights"].shape) >= N and not c["inside_out"]
    idx = np.stack(np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij"), axis=-1).reshape(-1, 3)
    sdis, _ = query(c, (idx.astype(np.float32) * F32(dx)).astype(np.float32))
    assert not np.isnan(sdis).any()
    T = c["table"]
    grad = np.empty((3, N, N, N), np.float32)
    grad[0] = (-T[:N, :N, 1])[:, None, :]
    grad[1] = F32(1)
    grad[2] = (-T[:N, :N, 2])[:, None, :]
    return sdis.reshape(N, N, N), grad


# ---- the float64 closed form ------------------------------------------------------------------------------------------------------------------
def closed_form(c, x):
    """h, sdis, n in float64 at the material points x (n, 3): exact bilinear interpolation of the float32 table's three channels."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    T, sp, (nx, nz) = c["table"].astype(np.float64), float(c["spacing"]), c["heights"].shape
    u, w = (x[:, 0] - float(c["origin"][0])) / sp, (x[:, 2] - float(c["origin"][1])) / sp
    inside = (u >= 0) & (u <= nx - 1) & (w >= 0) & (w <= nz - 1)
    us, ws = np.where(inside, u, 0.0), np.where(inside, w, 0.0)
    i, k = np.minimum(us.astype(np.int64), nx - 2), np.minimum(ws.astype(np.int64), nz - 2)
    fu, fw = us - i, ws - k
    val = ((1 - fu) * (1 - fw))[:, None] * T[i, k] + (fu * (1 - fw))[:, None] * T[i + 1, k] + ((1 - fu) * fw)[:, None] * T[i, k + 1] + (fu * fw)[:, None] * T[i + 1, k + 1]
    h, gx, gz = val[:, 0], val[:, 1], val[:, 2]
    ln = np.sqrt(gx * gx + 1.0 + gz * gz)
    n = np.stack([-gx / ln, 1.0 / ln, -gz / ln], axis=1)
    sdis = (x[:, 1] - h) / ln
    if c["inside_out"]:
        sdis, n = -sdis, -n
    return np.where(inside, h, np.nan), np.where(inside, sdis, np.nan), np.where(inside[:, None], n, 0.0), inside


# ---- the tables and points both test files use (bits 6: dx = 1 / 64) -------------------------------------------------------------------------------
def terrain(nx, nz, seed, spacing, origin=(0.0, 0.0), base=0.5, slope=(-0.35, 0.15), bumps=0.04):
    """A seeded ramp plus bumps: h = base + slope . (x - 0.5, z - 0.5) + bumps (sum of three sines with seeded phases), float32 (nx, nz)."""
    rng = np.random.default_rng(seed)
    ph = rng.random(6) * 2 * np.pi
    X = origin[0] + np.arange(nx)[:, None] * float(spacing)
    Z = origin[1] + np.arange(nz)[None, :] * float(spacing)
    h = base + slope[0] * (X - 0.5) + slope[1] * (Z - 0.5)
    h = h + bumps * (np.sin(11 * X + ph[0]) * np.cos(7 * Z + ph[1]) + 0.5 * np.sin(23 * X + 5 * Z + ph[2]) + 0.25 * np.cos(31 * Z - 13 * X + ph[3]))
    return h.astype(np.float32)


def tables():
    """The tables of the CPU test: name -> (heights, origin, spacing)."""
    rng = np.random.default_rng(21)
    return {
        "2x2": (np.array([[0.375, 0.5], [0.625, 0.4375]], np.float32), (0.25, 0.25), 0.5),
        "5x3": ((0.3 + 0.4 * rng.random((5, 3))).astype(np.float32), (0.1, 0.2), 0.2),
        "65x65": (terrain(65, 65, 1, DX), (0.0, 0.0), DX),
        "33x17": (terrain(33, 17, 2, 0.013, origin=(-0.05, 0.3)), (-0.05, 0.3), 0.013),
    }


def make(name, moved=False, **kw):
    H, origin, spacing = tables()[name]
    return heightfield(H, **{**dict(origin=origin, spacing=spacing), **(sm.MOVED if moved else {}), **kw})


def special_points(c):
    """Material points where the query's definition has a corner: on samples, on cell edges, u = 0 and u = nx - 1 exactly and one nextafter
    outside each (likewise w), exactly on the surface at samples (sdis == 0), NaN coordinates (last three rows).  (n, 3) float32."""
    H, o, sp, (nx, nz) = c["heights"], c["origin"], c["spacing"], c["heights"].shape
    xs = (o[0] + np.arange(nx).astype(np.float32) * sp).astype(np.float32)
    zs = (o[1] + np.arange(nz).astype(np.float32) * sp).astype(np.float32)
    inf = F32(np.inf)
    pts = []
    ii, kk = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    sel = np.random.default_rng(5).permutation(nx * nz)[:64]
    for i, k in zip(ii.ravel()[sel], kk.ravel()[sel]):
        pts += [[xs[i], H[i, k], zs[k]], [xs[i], np.nextafter(H[i, k], inf), zs[k]], [xs[i], np.nextafter(H[i, k], -inf), zs[k]]]   # on the surface at a sample, and either side
        if i + 1 < nx:
            pts += [[F32(0.5) * (xs[i] + xs[i + 1]), H[i, k], zs[k]]]                                                           # on a cell edge
        if k + 1 < nz:
            pts += [[xs[i], H[i, k], F32(0.25) * zs[k] + F32(0.75) * zs[k + 1]]]
    xr = [np.nextafter(xs[0], -inf), xs[0], xs[-1], np.nextafter(xs[-1], inf), xs[nx // 2]]
    zr = [np.nextafter(zs[0], -inf), zs[0], zs[-1], np.nextafter(zs[-1], inf), zs[nz // 2]]
    pts += [[a, F32(0.4), b] for a in xr for b in zr]
    pts += [[xs[0] - sp, 0.4, zs[0]], [xs[-1] + sp, 0.4, zs[-1]], [1e30, 0.0, 0.0], [0.0, 0.0, -1e30]]
    pts += [[np.nan, 0.5, zs[0]], [xs[0], np.nan, zs[0]], [np.nan] * 3]
    return np.array(pts, dtype=np.float64).astype(np.float32)
