"""What mpm_remove_particles promises, stated in NumPy (tests/test_particle_remove_model_cpu.py, tests/test_particle_remove_gpu.py), and the sweep
rule of scenes.Sink stated a second time, from its definition.

The removal takes particles out of a context at a substep boundary.  Afterwards
  - a live particle of a selected model is gone when collision_shape_model.query of any region gives sdis <= 0 at its float32 position, or its id
    is listed (selected); the others are there with the bits they had (split);
  - a grid node that no removed particle's 27-node stencil reaches (particle_emit_model.reached_nodes) holds the bits it held; a reached node with
    m_old > 0 holds the survivors' set-up mass m' (particle_init_model.setup_nodes) and the momenta p_old m' / m_old, exact zeros where m' == 0;
    a reached node with !(m_old > 0) holds the bits it held (expected_grid);
  - the model's n stays, its bucketed count shrinks, the books balance through the bias (books_after).
The predicate is evaluated in float32 statement for statement as the device evaluates it, so its decision on positions read back is exact and no
margin around a surface is needed.

Test infrastructure only."""
import numpy as np

import collision_shape_model as csm
import particle_emit_model as pem
import particle_init_model as pim

U = pim.U

# the scene files' keys for the two vectors of a region
ALIAS = {"point": "a", "center": "a", "normal": "b", "half_extents": "b"}


# ---- the predicate ---------------------------------------------------------------------------------------------------------------------------------
def region(d):
    """A region dict of Engine.remove as the library holds it (collision_shape_model.collider: float32, a half-space's normal normalised)"""
    r = {ALIAS.get(k, k): v for k, v in d.items()}
    return csm.collider(r.get("kind", r.get("shape")), a=r.get("a", (0, 0, 0)), b=r.get("b", (0, 0, 0)), radius=r.get("radius", 0.0), inside_out=r.get("inside_out", False))


def selected(xyz, regions=(), ids=None, listed=()):
    """(n,) bool: which of the live particles xyz (n, 3) float32 - with ids (n,) or None - a removal by `regions` (region dicts) and the id list
    `listed` takes.  A NaN sdis compares false and selects nothing."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    hit = np.zeros(x.shape[0], bool)
    for d in regions:
        with np.errstate(invalid="ignore"):
            hit |= csm.query(region(d), x)[0] <= 0
    if ids is not None and len(listed):
        hit |= np.isin(np.asarray(ids), np.asarray(listed))
    return hit


def split(p, gone):
    """a particle dict of particle_emit_model (xyz, state9, logjp, ids or None) into (survivors, removed) by the mask `gone`"""
    def take(mask):
        return {k: (None if v is None else np.ascontiguousarray(np.asarray(v)[mask])) for k, v in p.items()}
    return take(~gone), take(gone)


def books_after(books, removed):
    """books: {"n": [...], "bucketed": [...], "lost", "dropped", "bias"}; removed: per model - n stays, bucketed shrinks, the bias takes the sum"""
    out = {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in books.items()}
    for m, k in enumerate(removed):
        out["bucketed"][m] -= k
    out["bias"] += sum(removed)
    return out


# ---- the grid --------------------------------------------------------------------------------------------------------------------------------------
def survivor_scene(bits, models):
    """models: [(material params {"volume", "rho"}, xyz (n, 3) float32)] - the survivors of all models as a scene particle_init_model rasterises (v0 = 0)"""
    return {"bits": bits, "models": [{"xyz": np.asarray(x, np.float32), "v0": (0.0, 0.0, 0.0), "params": dict(p)} for p, x in models if np.asarray(x).shape[0]]}


def expected_grid(old_flat, old_val, removed_xyz, scene_survivors):
    """The grid after a removal, over the nodes of the old grid (old_flat ascending, old_val (K, 4) float32):
    -> (reached (K,) bool, exact (K,) bool, want (K, 4) float64, bound (K, 4)).
    exact: the node's four channels are known bit for bit - want holds them (as float64 of the float32 bits): an unreached node and a reached node
    with !(m_old > 0) keep theirs, a reached node with m' == 0 holds +0.  Elsewhere want = {m', p_old m' / m_old} and
    bound = {the set-up rasteriser's bound on m' (particle_init_model.node_bounds), |p_old| (m' / m_old) (eps_m' + 2 u)}: m' enters the ratio with
    its relative error eps_m', the division and the product round once each; a product below float32's normal range may be flushed (2^-126)."""
    bits = scene_survivors["bits"]
    n = 1 << bits
    old = old_val.astype(np.float64)
    reached = np.isin(old_flat, pem.reached_nodes(removed_xyz, bits))
    m1, nb = np.zeros(old_flat.size), np.zeros(old_flat.size)
    if scene_survivors["models"]:
        g = pim.setup_nodes(scene_survivors)
        flat = (g["nodes"][:, 0] * n + g["nodes"][:, 1]) * n + g["nodes"][:, 2]
        assert np.isin(flat, old_flat).all(), "a node the survivors give mass to lies in no block of the old grid"
        at = np.searchsorted(old_flat, flat)
        m1[at], nb[at] = g["val"][:, 0], pim.node_bounds(g)[:, 0]
    live = reached & (old_val[:, 0] > 0)
    rescaled = live & (m1 > 0)
    exact = ~rescaled
    want, bound = old.copy(), np.zeros_like(old)
    want[live & (m1 == 0)] = 0.0
    ratio = m1[rescaled] / old[rescaled, 0]
    want[rescaled, 0], bound[rescaled, 0] = m1[rescaled], nb[rescaled]
    want[rescaled, 1:] = old[rescaled, 1:] * ratio[:, None]
    bound[rescaled, 1:] = np.abs(old[rescaled, 1:]) * ratio[:, None] * (nb[rescaled] / m1[rescaled] + 2 * U)[:, None] + 2.0 ** -126
    return reached, exact, want, bound


def check_grid(old_flat, old_val, new_flat, new_val, removed_xyz, scene_survivors):
    """Assert the contract node by node; a node of the old grid whose block was dropped must be one that holds exact zeros.  Returns the worst
    error / bound per channel over the rescaled nodes (0 if there are none)."""
    reached, exact, want, bound = expected_grid(old_flat, old_val, removed_xyz, scene_survivors)
    assert np.isin(new_flat, old_flat).all(), "the new grid holds a node the old one did not"
    kept = np.isin(old_flat, new_flat)
    dropped_ok = (want[~kept] == 0).all(axis=1) & exact[~kept]
    assert dropped_ok.all(), ("a dropped block held a node that should have survived", old_flat[~kept][~dropped_ok][:5])
    got = new_val[np.searchsorted(new_flat, old_flat[kept])]
    ex, wa, bo = exact[kept], want[kept], bound[kept]
    same = np.array_equal(got[ex].view(np.uint32), wa[ex].astype(np.float32).view(np.uint32))
    assert same, ("a node that keeps its bits (or is emptied) changed", np.argwhere(got[ex].view(np.uint32) != wa[ex].astype(np.float32).view(np.uint32))[:5])
    err = np.abs(got[~ex].astype(np.float64) - wa[~ex])
    assert (err <= bo[~ex]).all(), ("a rescaled node is off", np.argwhere(err > bo[~ex])[:5])
    return (err / np.maximum(bo[~ex], 2.0 ** -149)).max(axis=0) if err.size else np.zeros(4)


# ---- the sink's sweep rule, from its definition --------------------------------------------------------------------------------------------------------
def sweep_times(start, end, period):
    """t_k = start + k period for every k >= 0 with t_k < end"""
    out, k = [], 0
    while start + k * period < end:
        out.append(start + k * period)
        k += 1
    return np.array(out)


def expected_sweeps(start, end, period, times):
    """What a sink serves at the substep boundaries `times` (ascending): per boundary the list of sweep numbers - every sweep once, at the first
    boundary with t >= t_k; a boundary with a non-empty list makes one call."""
    tk = sweep_times(start, end, period)
    out, nxt = [], 0
    for t in times:
        now = []
        while nxt < tk.size and tk[nxt] <= t:
            now.append(nxt)
            nxt += 1
        out.append(now)
    return out
