"""The force fields of claymore_amd/csrc/mpm_force_field.hpp, restated with numpy float32 arrays statement for statement from the header's
comments (every operation rounded to float32, no contraction, every sum in the written association), and beside them the float64 closed
forms of INTEGRATION.md section 5.  Not a test: tests/test_force_field_model_cpu.py judges the x86 build of the header against this model and
this model against the closed forms; tests/test_force_field_gpu.py judges the kernels against it.

A field is a dict as the library holds it after install (field()): float32 numbers, the vortex axis in `vec` normalised, the region a collider
dict of tests/collision_shape_model.py (its half-space normal normalised) or None."""
import numpy as np

import collision_shape_model as sm
import grid_update_model as gm

F32 = np.float32
UNIFORM, POINT, VORTEX, DRAG = 1, 2, 3, 4
KINDS = {"uniform": UNIFORM, "point": POINT, "vortex": VORTEX, "drag": DRAG}
MAX_FIELDS = 4
DX = sm.DX


def f3(v):
    return np.asarray(v, dtype=np.float32).reshape(3)


def field(kind, vec=(0, 0, 0), centre=(0, 0, 0), strength=0.0, swirl=0.0, pull=0.0, lift=0.0, soft=0.0, falloff=0, region=None, feather=0.0):
    """One field as installed.  region: None or keyword arguments of collision_shape_model.collider (kind, a, b, radius, inside_out).
    vec_given / region's b_given are what the caller hands to the library."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    vec = given = f3(vec)
    if kind == VORTEX:
        ln = np.sqrt(F32(F32(F32(vec[0] * vec[0]) + F32(vec[1] * vec[1])) + F32(vec[2] * vec[2])))
        vec = (vec / ln).astype(np.float32)
    return dict(kind=kind, vec=vec, vec_given=given, centre=f3(centre), strength=F32(strength), swirl=F32(swirl), pull=F32(pull), lift=F32(lift), soft=F32(soft),
                falloff=int(falloff), feather=F32(feather), region=None if region is None else sm.collider(**region))


def engine_kwargs(f):
    """The field as keyword arguments of Engine.set_force_field."""
    r = f["region"]
    region = None if r is None else dict(kind=r["kind"], a=r["a"], b=r["b_given"], radius=float(r["radius"]), inside_out=r["inside_out"])
    return dict(kind=f["kind"], vec=f["vec_given"], centre=f["centre"], strength=float(f["strength"]), swirl=float(f["swirl"]), pull=float(f["pull"]),
                lift=float(f["lift"]), soft=float(f["soft"]), falloff=f["falloff"], region=region, feather=float(f["feather"]))


def _r(x):
    return np.asarray(x).astype(np.float32)


def weight(f, X):
    """force_weight: X (n, 3) float32 domain points -> w (n,) float32."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    if f["region"] is None:
        return np.ones(len(X), np.float32)
    with np.errstate(all="ignore"):
        sdis, _ = sm.query(f["region"], X)
        if f["feather"] > 0:
            t = _r(_r(F32(0) - sdis) / f["feather"])
            return np.where(sdis < 0, np.where(t < 1, t, F32(1)), F32(0)).astype(np.float32)
        return np.where(sdis <= 0, F32(1), F32(0)).astype(np.float32)


def acceleration(f, X):
    """a (n, 3) float32 of the three acceleration kinds at X."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        if f["kind"] == UNIFORM:
            return np.broadcast_to(f["vec"][None], X.shape).astype(np.float32)
        if f["kind"] == POINT:
            r = _r(f["centre"][None] - X)
            d2 = _r(sm._dot3(r[:, 0], r[:, 1], r[:, 2], r[:, 0], r[:, 1], r[:, 2]).astype(np.float32) + F32(f["soft"] * f["soft"]))
            d = _r(np.sqrt(d2))
            den = d if f["falloff"] == 0 else (d2 if f["falloff"] == 1 else _r(d2 * d))
            a = _r(f["strength"] * _r(r / den[:, None]))
            return np.where((d == 0)[:, None], F32(0), a).astype(np.float32)
        if f["kind"] == VORTEX:
            n = f["vec"]
            r = _r(X - f["centre"][None])
            h = sm._dot3(r[:, 0], r[:, 1], r[:, 2], n[0], n[1], n[2]).astype(np.float32)
            rp = _r(r - _r(h[:, None] * n[None]))
            c = np.stack([_r(_r(n[1] * rp[:, 2]) - _r(n[2] * rp[:, 1])), _r(_r(n[2] * rp[:, 0]) - _r(n[0] * rp[:, 2])), _r(_r(n[0] * rp[:, 1]) - _r(n[1] * rp[:, 0]))], axis=1)
            return _r(_r(_r(f["swirl"] * c) - _r(f["pull"] * rp)) + _r(f["lift"] * n)[None])
    raise ValueError(f["kind"])


def apply_one(f, X, dt, m, p):
    """One slot on {m (n,), p (n, 3)} at X: -> p afterwards, acted (n,) bool.  Rows with w == 0 keep their bits."""
    dt = F32(dt)
    w = weight(f, X)
    act = w != 0
    with np.errstate(all="ignore"):
        if f["kind"] == DRAG:
            s = _r(w * F32(f["strength"] * dt))
            new = _r(_r(p + _r(s[:, None] * _r(m[:, None] * f["vec"][None]))) / _r(F32(1) + s)[:, None])
        else:
            a = acceleration(f, X)
            g = _r(w * dt)
            new = _r(p + _r(m[:, None] * _r(a * g[:, None])))
    out = p.view(np.uint32).copy()
    out[act] = new.view(np.uint32)[act]
    return out.view(np.float32), act


def force_cell(fields, X, dt, mp4):
    """force_cell: the slots in order (None: an empty slot) on mp4 (n, 4) = {m, p} at X (n, 3) -> (n, 4), acted (n,) bool (any slot)."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    mp4 = np.ascontiguousarray(mp4, dtype=np.float32).reshape(-1, 4)
    m, p = mp4[:, 0].copy(), np.ascontiguousarray(mp4[:, 1:4])
    acted = np.zeros(len(X), bool)
    for f in fields:
        if f is None:
            continue
        p, act = apply_one(f, X, dt, m, p)
        acted |= act
    out = mp4.view(np.uint32).copy()
    out[:, 1:4] = p.view(np.uint32)
    return out.view(np.float32), acted


def force_model(keys, fields, dt, grid, dx=DX):
    """grid_force_kernel over a whole grid (nbc, 4, 64) of float32 words: every cell with m > 0 through force_cell at X = (float) node * dx.
    -> the grid afterwards (cells without mass, the mass channel and cells no slot acted on keep their bits), acted (nbc, 64)."""
    grid = np.ascontiguousarray(grid, dtype=np.float32)
    nodes = gm.node_coords(keys).transpose(0, 2, 1).reshape(-1, 3)
    X = (nodes.astype(np.float32) * F32(dx)).astype(np.float32)
    mp4 = np.ascontiguousarray(grid.transpose(0, 2, 1).reshape(-1, 4))
    with np.errstate(all="ignore"):
        live = mp4[:, 0] > 0
    new, acted = force_cell(fields, X, dt, mp4)
    acted &= live
    out = mp4.view(np.uint32).copy()
    out[acted] = new.view(np.uint32)[acted]
    return np.ascontiguousarray(out.view(np.float32).reshape(len(keys), 64, 4).transpose(0, 2, 1)), acted.reshape(len(keys), 64)


# ---- the float64 closed forms ---------------------------------------------------------------------------------
def closed_weight(f, X):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    if f["region"] is None:
        return np.ones(len(X))
    sdis, _ = sm.closed_form(f["region"], X)
    if f["feather"] > 0:
        return np.where(sdis < 0, np.minimum(1.0, -sdis / float(f["feather"])), 0.0)
    return np.where(sdis <= 0, 1.0, 0.0)


def closed_acceleration(f, X):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    vec, c = f["vec"].astype(np.float64), f["centre"].astype(np.float64)
    if f["kind"] == UNIFORM:
        return np.broadcast_to(vec, X.shape).copy()
    if f["kind"] == POINT:
        r = c - X
        d2 = (r * r).sum(axis=1) + float(f["soft"]) ** 2
        d = np.sqrt(d2)
        den = (d, d2, d2 * d)[f["falloff"]]
        with np.errstate(all="ignore"):
            return np.where((d == 0)[:, None], 0.0, float(f["strength"]) * r / den[:, None])
    if f["kind"] == VORTEX:
        n = vec                                                # (the axis as installed: unit length to float32 rounding, not normalised again)
        r = X - c
        rp = r - (r @ n)[:, None] * n
        return float(f["swirl"]) * np.cross(np.broadcast_to(n, rp.shape), rp) - float(f["pull"]) * rp + float(f["lift"]) * n
    raise ValueError(f["kind"])


def closed_apply(f, X, dt, m, p, w=None):
    """One slot in float64 (w: the weight to use, default the closed form's)."""
    m, p = np.asarray(m, np.float64), np.asarray(p, np.float64)
    w = closed_weight(f, X) if w is None else np.asarray(w, np.float64)
    if f["kind"] == DRAG:
        s = w * float(f["strength"]) * float(dt)
        return (p + s[:, None] * m[:, None] * f["vec"].astype(np.float64)) / (1 + s)[:, None]
    return p + m[:, None] * closed_acceleration(f, X) * (w * float(dt))[:, None]


# ---- the fields and points the test files share (bits 6: dx = 1 / 64) ------------------------------------------------------------------------
# The regions are collision_shape_model's: their faces cut through the central blocks and pass exactly through nodes (its SHAPES' comments).
REGIONS = {name: sm.SHAPES[name] for name in ("halfspace", "sphere", "box", "capsule")}
FEATHER = 3 * DX
KIND_CASES = {
    "uniform": dict(kind="uniform", vec=(0.75, -9.8, 2.5)),
    "point0": dict(kind="point", centre=(0.5, 0.5, 0.5), strength=3.0, falloff=0, soft=0.0),          # (the centre is node (32, 32, 32): d == 0)
    "point1": dict(kind="point", centre=(0.5, 0.5, 0.5), strength=-0.5, falloff=1, soft=2 * DX),
    "point2": dict(kind="point", centre=(0.25, 0.5, 0.75), strength=0.01, falloff=2, soft=0.0),       # (a node too)
    "vortex": dict(kind="vortex", vec=(0.5, 2.0, -0.25), centre=(0.5, 0.25, 0.5), swirl=30.0, pull=4.0, lift=-1.5),
    "drag": dict(kind="drag", vec=(3.0, -0.5, 0.25), strength=200.0),
}


def make(name, region=None, inside_out=False, feather=0.0, **kw):
    reg = None if region is None else {**REGIONS[region], "inside_out": inside_out}
    return field(**{**KIND_CASES[name], "region": reg, "feather": feather, **kw})


def case_list():
    """(id, field) for every kind and falloff without a region and in each of the four region shapes, and inside_out and feather variants."""
    out = []
    for i, name in enumerate(KIND_CASES):
        out.append((name, make(name)))
        for j, reg in enumerate(REGIONS):
            io, fe = bool((i + j) & 1), (FEATHER if (i + j) % 3 == 0 else 0.0)
            out.append((f"{name}-{reg}{'-io' if io else ''}{'-feather' if fe else ''}", make(name, reg, inside_out=io, feather=fe)))
    for reg in REGIONS:                                                                  # every shape with a feather and inside out at least once
        out.append((f"drag-{reg}-io-feather", make("drag", reg, inside_out=True, feather=FEATHER)))
        out.append((f"uniform-{reg}-feather", make("uniform", reg, feather=FEATHER)))
    return out


def adversarial_points(fields, seed, n=2048):
    """Points and {m, p} for the function-level comparisons: seeded domain points (every 16th on a node), the special points of every region
    (faces, edges, centres, NaN), the fields' centres (d == 0), and momenta of every class of grid_update_model.generate - denormal, huge,
    +-0, inf, NaN - over ordinary, FLT_MIN, denormal and infinite masses."""
    pts = [sm.seeded_points(seed, n)]
    for f in fields:
        if f is None:
            continue
        pts.append(np.stack([f["centre"], f["centre"] + F32(DX) * f3((1, 0, 0))]).astype(np.float32))
        if f["region"] is not None:
            sp = sm.special_points(f["region"])
            pts.append(sp)
            if f["feather"] > 0:                                                        # half-way through and at the end of the feather, inward
                sd, nr = sm.query(f["region"], sp)
                pts.append((sp - nr * (f["feather"] * F32(0.5))).astype(np.float32))
                pts.append((sp - nr * f["feather"]).astype(np.float32))
    X = np.concatenate(pts).astype(np.float32)
    pat = gm.generate((len(X) + 63) // 64, seed, "full")[0]
    mp4 = np.ascontiguousarray(pat.transpose(0, 2, 1).reshape(-1, 4)[:len(X)]).view(np.float32)
    return X, mp4
