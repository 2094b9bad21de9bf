"""Host-side mirror of the reference's GmpmSimulator surface (Projects/GMPM/gmpm_simulator.cuh:25-783)
on top of the C ABI.  Method names follow the reference: init_model, update_fr_parameters,
update_j_fluid_parameters, update_nacc_parameters, main_loop / substep, output_model."""
import ctypes as C
import math

import numpy as np

from . import _ffi


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mpm status {code}: {msg}")
        self.code = code


def momentum_dict(out):
    """The five doubles of mpm_particle_momentum / mpm_group_particle_momentum as a dict."""
    return {"count": int(out[0]), "momentum": np.array(out[1:4], dtype=np.float64), "kinetic": float(out[4])}


def stress_totals_dict(out):
    """The eight doubles of mpm_stress_totals as a dict."""
    return {"count": int(out[0]), "stress_integral": np.array(out[1:7], dtype=np.float64), "max_von_mises": float(out[7])}


def skew(omega):
    """The 3 x 3 matrix W with W x = omega x x (float64)."""
    wx, wy, wz = (float(x) for x in omega)
    return np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])


def _position_keys(xyz):
    """The position bits of every row as one sortable record."""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    return x.view(np.uint32).view([("x", np.uint32), ("y", np.uint32), ("z", np.uint32)]).ravel()


def join_by_position(id_xyz, ids, xyz, *arrays):
    """Rows (xyz, *arrays) of a readout joined to (id_xyz, ids) of retrieve_ids on the position bits; returns (ids, xyz, *arrays) in
    ascending id order.  Both sides must hold the same multiset of positions.  Bit-identical positions are handed out in id order."""
    ka, kb = _position_keys(id_xyz), _position_keys(xyz)
    if ka.shape != kb.shape:
        raise ValueError(f"order_by_id: {kb.shape[0]} rows against {ka.shape[0]} ids")
    ids = np.asarray(ids)
    oa = np.lexsort((ids, ka["z"], ka["y"], ka["x"]))  # by position, ties by id
    ob = np.lexsort((kb["z"], kb["y"], kb["x"]))       # by position, stable: ties as they stand
    if not np.array_equal(ka[oa], kb[ob]):
        raise ValueError("order_by_id: the readout's positions are not those of retrieve_ids (taken at another substep boundary?)")
    rank = np.argsort(ids[oa], kind="stable")
    rows = ob[rank]
    return (ids[oa][rank],) + tuple(np.asarray(a)[rows] for a in (xyz,) + arrays)


class Engine:
    """One simulation context on one device.

    api: a bound _ffi.Api.  The product always uses the HIP library (`Engine(cfg)`); tests may hand in
    the oracle's Api to drive the checker through the same call sequence.

    track_ids=True (HIP library only): every particle carries a persistent id - its index in the array its model was added with
    (retrieve_ids, order_by_id).  Off by default: an untracked engine allocates and launches nothing for it.
    """

    def __init__(self, cfg=None, device=0, api=None, domain_bits=None, track_ids=False, **overrides):
        self.api = api if api is not None else _ffi.load_hip()
        if cfg is None:
            cfg = _ffi.Config()
            self._check(self.api.default_config(int(domain_bits), C.byref(cfg)))
        for k, v in overrides.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.ctx = C.c_void_p()
        rc = self.api.create(C.byref(cfg), int(device), C.byref(self.ctx))
        if rc != 0:
            raise EngineError(rc, "mpm_create failed (no usable HIP device? there is no CPU fallback)")
        self.dx = 1.0 / (1 << cfg.domain_bits)
        self.track_ids = bool(track_ids)
        if self.track_ids:
            self._check(self.api.track_particle_ids(self.ctx, 1))
        self.models = []
        self._slot_geom = {}  # slot -> what set_collider_body(density=...) integrates over (_slot_geometry)
        self.emitters = []    # scenes.Emitter objects, served by main_loop (serve_emitters)
        self.sinks = []       # scenes.Sink objects, served by main_loop before the emitters (serve_sinks)
        self.forces = []      # scenes.ForceEntry objects, served by main_loop before the sinks (serve_forces)
        self.cur_time = 0.0
        self.dt = None

    # ---- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.api.destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self.api.last_error(self.ctx).decode() if getattr(self, "ctx", None) else ""
            raise EngineError(rc, msg)

    # ---- model setup (gmpm_simulator.cuh:168-254) -------------------------------------------------
    def default_material(self, material):
        p = _ffi.MaterialParams()
        self._check(self.api.default_material(int(material), self.cfg.domain_bits, C.byref(p)))
        return p

    def init_model(self, material, positions, v0=(0.0, 0.0, 0.0), params=None, velocity=None, affine=None, state=None, logjp=None,
                   state_kind="b", **param_overrides):
        """Add a model.  The four keyword arrays are its per-particle initial conditions (mpm_add_model_particles, HIP library only), in the
        order of `positions`; with all of them None this is mpm_add_model.
        velocity (n, 3): v_p in world units (None: v0 for every particle).  affine (n, 3, 3): the APIC matrix, affine[p, r, c] = C_rc as
        retrieve_velocity(affine=True) returns it (None: 0).  state (n, 9) or (n, 3, 3): what retrieve_state returns - b = F F^T with the
        reflection mark in the sign of entry 0, J in entry 0 for the J-fluid - with state_kind "b", or the deformation gradient
        F[p, r, c] with state_kind "f" (None: stress-free).  logjp (n,): sand / NACC (None: the material's log_jp0)."""
        xyz = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        p = params if params is not None else self.default_material(material)
        for k, v in param_overrides.items():
            setattr(p, k, v)
        v = (C.c_float * 3)(*[float(x) for x in v0])
        mid = C.c_int(-1)
        n = xyz.shape[0]
        if velocity is None and affine is None and state is None and logjp is None:
            self._check(self.api.add_model(self.ctx, int(material), C.byref(p), xyz.ctypes.data_as(C.c_void_p), n, v, C.byref(mid)))
        else:
            if not hasattr(self.api, "add_model_particles"):
                raise EngineError(_ffi.MPM_ERR_INVALID, "init_model: per-particle initial conditions need the HIP library (this API has no add_model_particles)")
            init, keep = self._particle_init("init_model", n, velocity, affine, state, logjp, state_kind)   # (keep: the arrays live until the call returns)
            self._check(self.api.add_model_particles(self.ctx, int(material), C.byref(p), xyz.ctypes.data_as(C.c_void_p), n, v, C.byref(init), C.byref(mid)))
        self.models.append({"material": int(material), "n": n, "params": p, "removed": 0})
        return mid.value

    @staticmethod
    def _particle_init(who, n, velocity, affine, state, logjp, state_kind):
        """The four per-particle arrays of init_model / emit as an mpm_particle_init, and the float32 arrays it points into."""
        if state_kind not in _ffi.STATE_KINDS:
            raise ValueError(f"{who}: state_kind {state_kind!r} ('b' or 'f')")
        keep = []

        def col(a, width, name, transpose=False):
            if a is None:
                return None
            a = np.asarray(a, dtype=np.float32)
            if a.size != n * width:
                raise ValueError(f"{who}: {name} holds {a.size} values for {n} particles ({n * width} expected)")
            if transpose and a.ndim == 3:                            # [p, r, c] -> the library's column-major 9 floats (index 3 c + r)
                a = a.transpose(0, 2, 1)
            a = np.ascontiguousarray(a).reshape(n, width)
            keep.append(a)
            return a.ctypes.data
        init = _ffi.ParticleInit()
        init.velocity = col(velocity, 3, "velocity")
        init.affine9 = col(affine, 9, "affine", transpose=True)
        init.state9 = col(state, 9, "state", transpose=(state_kind == "f"))
        init.logjp = col(logjp, 1, "logjp")
        init.state_kind = _ffi.STATE_KINDS[state_kind]
        return init, keep

    def emit(self, model, positions, v0=(0.0, 0.0, 0.0), velocity=None, affine=None, state=None, logjp=None, state_kind="b"):
        """Add particles to `model` of an engine that has been set up, at a substep boundary (mpm_emit_particles, HIP library only): an inflow.
        The arguments are init_model's - positions (n, 3), v0 for every particle unless `velocity` (n, 3) is given, `affine`, `state`, `logjp`
        and `state_kind` as there.  Returns first_id: the new particles are numbers first_id .. first_id + n - 1 of the model (their ids in a
        track_ids engine).  Every old particle keeps its state bit for bit, the grid gains the new particles' set-up P2G; the call costs a
        re-lay of all particles, so emit a layer at a time, not a particle at a time."""
        if not hasattr(self.api, "emit_particles"):
            raise EngineError(_ffi.MPM_ERR_INVALID, "emit needs the HIP library (this API has no emit_particles)")
        xyz = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        init, keep = self._particle_init("emit", n, velocity, affine, state, logjp, state_kind)
        first = C.c_int32(-1)
        self._check(self.api.emit_particles(self.ctx, int(model), xyz.ctypes.data_as(C.c_void_p), n, (C.c_float * 3)(*[float(x) for x in v0]),
                                            C.byref(init), C.byref(first)))
        self.models[model]["n"] += n
        return first.value

    @staticmethod
    def _sink_regions(who, regions):
        """A list of region dicts as an array of mpm_collision_shape: set_collision_shape's keywords (kind, a, b, radius, inside_out), or the scene
        files' keys - "point" / "normal" (half-space), "center" (sphere, box), "half_extents" (box); a capsule has a, b and radius only."""
        regions = [] if regions is None else ([regions] if isinstance(regions, dict) else list(regions))
        arr = (_ffi.CollisionShape * max(1, len(regions)))()
        alias = {"point": "a", "center": "a", "normal": "b", "half_extents": "b"}
        for sh, reg in zip(arr, regions):
            r = {alias.get(k, k): v for k, v in reg.items()}
            unknown = set(r) - {"kind", "shape", "a", "b", "radius", "inside_out"}
            if unknown:
                raise ValueError(f"{who}: unknown region keys {sorted(unknown)}")
            kind = r.get("kind", r.get("shape"))
            sh.kind = _ffi.SHAPE_NAMES[kind] if isinstance(kind, str) else int(kind)
            sh.inside_out = 1 if r.get("inside_out") else 0
            a, b = r.get("a", (0.0, 0.0, 0.0)), r.get("b", (0.0, 0.0, 0.0))
            for d in range(3):
                sh.a[d], sh.b[d] = float(a[d]), float(b[d])
            sh.radius = float(r.get("radius", 0.0))
        return arr, len(regions)

    def count_in(self, regions, model=-1):
        """How many live particles of each model lie in the regions (mpm_count_particles_in, HIP library only): the predicate of `remove` alone,
        nothing is written.  regions: one dict or a list of up to 8, as `remove` takes them; model: one model, or -1 for all.  Returns a list with
        one count per model."""
        if not hasattr(self.api, "count_particles_in"):
            raise EngineError(_ffi.MPM_ERR_INVALID, "count_in needs the HIP library (this API has no count_particles_in)")
        arr, n = self._sink_regions("count_in", regions)
        out = (C.c_int64 * 8)()
        self._check(self.api.count_particles_in(self.ctx, int(model), arr, n, out))
        return [int(out[m]) for m in range(len(self.models))]

    def remove(self, regions=None, ids=None, model=-1, return_removed=False):
        """Take particles out of an engine that has been set up, at a substep boundary (mpm_remove_particles, HIP library only): a sink.  A live
        particle of `model` (-1: every model) goes when it lies in any of the `regions` - dicts with set_collision_shape's keywords (kind, a, b,
        radius, inside_out) or the scene files' keys (point / normal, center, half_extents), in domain coordinates - or when its id is in `ids`
        (track_ids engines, model >= 0).  Returns {"removed": per-model counts, "mass", "momentum": what left the grid, "relaid"} and, with
        return_removed, "xyz" (k, 3), "ids" (k,) (-1 untracked) and "model" (k,) of the removed particles in unspecified order.  Survivors keep
        their state bit for bit and the velocity field they were in; a call that selects nothing costs one counting pass and changes nothing
        (relaid False).  models[m]["n"] stays - removed ids are never reused -, models[m]["removed"] accumulates."""
        if not hasattr(self.api, "remove_particles"):
            raise EngineError(_ffi.MPM_ERR_INVALID, "remove needs the HIP library (this API has no remove_particles)")
        arr, n = self._sink_regions("remove", regions)
        what = _ffi.Removal()
        what.regions, what.nregions = arr, n
        idarr = None
        if ids is not None:
            idarr = np.ascontiguousarray(ids, dtype=np.int32).ravel()
            what.ids, what.nids = idarr.ctypes.data, idarr.size
        res = _ffi.RemovalResult()
        xyz = rid = rmodel = None
        if return_removed:
            if ids is None:                                                # the regions alone: their count sizes the arrays
                cap = sum(self.count_in(regions, model)) if n else 0
            else:                                                          # ids too: no more than every live particle of the model
                cap = int(self.counts().particles[model]) if model >= 0 else 0
            xyz, rid, rmodel = np.empty((cap, 3), np.float32), np.empty(cap, np.int32), np.empty(cap, np.int32)
            what.removed_xyz, what.removed_ids, what.removed_model, what.capacity = xyz.ctypes.data, rid.ctypes.data, rmodel.ctypes.data, cap
        self._check(self.api.remove_particles(self.ctx, int(model), C.byref(what), C.byref(res)))
        removed = [int(res.removed[m]) for m in range(len(self.models))]
        for m, k in enumerate(removed):
            self.models[m]["removed"] = self.models[m].get("removed", 0) + k
        out = {"removed": removed, "mass": float(res.mass), "momentum": np.array(list(res.momentum)), "relaid": bool(res.relaid)}
        if return_removed:
            k = sum(removed)
            out.update(xyz=xyz[:k].copy(), ids=rid[:k].copy(), model=rmodel[:k].copy())
        return out

    def set_model_velocity_field(self, model, v0=(0.0, 0.0, 0.0), grad=None, omega=None, pivot=(0.0, 0.0, 0.0)):
        """Start a model that has been added (init_model or init_model_mesh, before initial_setup) in the linear velocity field
        v_p = v0 + G (x_p - pivot), C_p = G (mpm_set_model_velocity_field, HIP library only).  grad: G as a 3 x 3 array, grad[r][c] = dv_r / dx_c;
        omega: shorthand for the skew matrix of a rigid rotation, v = v0 + omega x (x - pivot).  Giving both adds them."""
        if not hasattr(self.api, "set_model_velocity_field"):
            raise EngineError(_ffi.MPM_ERR_INVALID, "set_model_velocity_field needs the HIP library")
        G = np.zeros((3, 3), dtype=np.float64)
        if grad is not None:
            G += np.asarray(grad, dtype=np.float64).reshape(3, 3)
        if omega is not None:
            G += skew(omega)
        g9 = (C.c_float * 9)(*[float(x) for x in G.T.ravel()])          # column-major
        self._check(self.api.set_model_velocity_field(self.ctx, int(model), (C.c_float * 3)(*[float(x) for x in v0]), g9,
                                                      (C.c_float * 3)(*[float(x) for x in pivot])))

    def snapshot_models(self):
        """The models as they stand, ready for build_engine: a list of {material, params, xyz, velocity, affine, state, logjp, state_kind: "b"}
        per model, the rows of retrieve_state and retrieve_velocity(affine=True) joined on the position bits.  A context built from them -
        with another GPU count, max_ppc or capacity - starts from the same positions and the same material state, bit for bit.  Its
        velocities are RE-SAMPLED from the grid of the last P2G (what retrieve_velocity reads, before the next grid update): this is a
        re-seed, not a restart - the bit-exact restart is the checkpoint (save_checkpoint / load_checkpoint)."""
        out = []
        for mi, m in enumerate(self.models):
            xs, st, lj = self.retrieve_state(mi)
            xv, vel, aff = self.retrieve_velocity(mi, affine=True)
            ks, kv = _position_keys(xs), _position_keys(xv)
            os_, ov = np.lexsort((ks["z"], ks["y"], ks["x"])), np.lexsort((kv["z"], kv["y"], kv["x"]))
            if not np.array_equal(ks[os_], kv[ov]):
                raise ValueError("snapshot_models: the two readouts hold different positions")
            p = m["params"]
            prm = {name: getattr(p, name) for name, _ in _ffi.MaterialParams._fields_ if name != "reserved"}
            has_lj = m["material"] in (_ffi.SAND, _ffi.NACC)
            out.append({"material": m["material"], "params": prm, "xyz": xs[os_].copy(), "velocity": vel[ov].copy(), "affine": aff[ov].copy(),
                        "state": st[os_].copy(), "logjp": lj[os_].copy() if has_lj else None, "state_kind": "b"})
        return out

    @staticmethod
    def _mesh_fill_args(vertices, faces, margin, box, who):
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"{who}: vertices must be (nv, 3) and faces (nt, 3), got {v.shape} and {f.shape}")
        opt = _ffi.MeshFill()
        opt.margin = float(margin)
        if box is not None:
            opt.use_box = 1
            for d in range(3):
                opt.lo[d], opt.hi[d] = int(box[0][d]), int(box[1][d])
        return v, f, opt

    @staticmethod
    def sample_mesh(domain_bits, vertices, faces, margin=0.0, box=None, device=0, api=None):
        """The lattice particles inside a closed triangle mesh, sampled on the device (mpm_sample_mesh, HIP library only; needs no engine):
        (n, 3) float32 in the order that is the particles' id - tiles of 4^3 nodes ascending, nodes in a tile, the 8 candidates of a node
        (include/claymore_amd.h).  vertices / faces: as for set_collision_mesh.  margin >= 0 keeps particles off the surface (inside <=>
        sdis < -margin); box = (lo, hi): only the nodes lo <= (i, j, k) < hi.  For several GPUs: scenes.split_slabs on the result, then
        init_model per rank."""
        api = api if api is not None else _ffi.load_hip()
        v, f, opt = Engine._mesh_fill_args(vertices, faces, margin, box, "sample_mesh")
        n = C.c_size_t(0)
        args = (int(domain_bits), v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0], C.byref(opt))
        rc = api.sample_mesh(*args, None, C.byref(n), int(device))                                    # count, then fetch
        xyz = np.empty((n.value, 3), dtype=np.float32)
        if rc == 0 and n.value:
            rc = api.sample_mesh(*args, xyz.ctypes.data, C.byref(n), int(device))
        if rc != 0:
            raise EngineError(rc, "mpm_sample_mesh refused the call (an invalid mesh, margin or box; or no device memory)")
        return xyz

    def init_model_mesh(self, material, vertices, faces, v0=(0.0, 0.0, 0.0), margin=0.0, box=None, params=None, **param_overrides):
        """init_model with the positions sampled inside a closed triangle mesh on the device, straight into the model's array
        (mpm_add_model_mesh, HIP library only): the particles and their order are sample_mesh's.  Returns the model id."""
        v, f, opt = self._mesh_fill_args(vertices, faces, margin, box, "init_model_mesh")
        p = params if params is not None else self.default_material(material)
        for k, val in param_overrides.items():
            setattr(p, k, val)
        vel = (C.c_float * 3)(*[float(x) for x in v0])
        mid, n = C.c_int(-1), C.c_size_t(0)
        self._check(self.api.add_model_mesh(self.ctx, int(material), C.byref(p), v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0], C.byref(opt),
                                            vel, C.byref(mid), C.byref(n)))
        self.models.append({"material": int(material), "n": int(n.value), "params": p, "removed": 0})
        return mid.value

    def initial_setup(self):
        self._check(self.api.initial_setup(self.ctx))

    # ---- phases (gmpm_simulator.cuh:326-579) ------------------------------------------------------
    def grid_update(self, dt):
        mv = C.c_float(0)
        self._check(self.api.grid_update(self.ctx, dt, C.byref(mv)))
        return mv.value

    def compute_dt(self, max_vel, cur, nxt, dt_default):
        return self.api.compute_dt(self.ctx, max_vel, cur, nxt, dt_default)

    def g2p2g(self, dt, next_dt):
        self._check(self.api.g2p2g(self.ctx, dt, next_dt))

    def rebuild_partition(self):
        c = _ffi.Counts()
        self._check(self.api.rebuild_partition(self.ctx, C.byref(c)))
        return c

    def substep(self, dt, step_time, frame_time, dt_default):
        nd, mv = C.c_float(0), C.c_float(0)
        self._check(self.api.substep(self.ctx, dt, step_time, frame_time, dt_default, C.byref(nd), C.byref(mv)))
        return nd.value, mv.value

    def run_fixed(self, nsteps, dt):
        self._check(self.api.run_fixed(self.ctx, int(nsteps), dt))

    def serve_emitters(self, t=None):
        """Emit what every attached emitter (scenes.Emitter; build_engine attaches a scene's "emitters") has due at the substep boundary `t`
        (default: cur_time).  Returns the number of particles emitted."""
        t = self.cur_time if t is None else t
        total = 0
        for em in self.emitters:
            pts = em.due(t)
            if pts.shape[0]:
                self.emit(em.model, pts, v0=em.velocity)
                total += pts.shape[0]
        return total

    def serve_sinks(self, t=None):
        """Sweep every attached sink (scenes.Sink; build_engine attaches a scene's "sinks") that has a sweep due at the substep boundary `t`
        (default: cur_time): one Engine.remove per sink, however many of its sweeps are due.  Returns the number of particles removed."""
        t = self.cur_time if t is None else t
        total = 0
        for sk in self.sinks:
            if sk.due(t):
                total += sum(self.remove(regions=[sk.region], model=sk.model)["removed"])
        return total

    def main_loop(self, nframes, fps, dt_default, on_frame=None):
        """GmpmSimulator::main_loop (gmpm_simulator.cuh:303-592): adaptive dt, `nframes` frames.  Attached force entries, sinks and emitters
        are served after set-up and after every substep, in that order."""
        spf = 1.0 / fps
        max_v0 = 0.0
        dt = self.compute_dt(max_v0, 0.0, spf, dt_default)
        self.initial_setup()
        if self.forces:
            self.serve_forces()
        if self.sinks:
            self.serve_sinks()
        if self.emitters:
            self.serve_emitters()
        steps = 0
        for frame in range(1, nframes + 1):
            t = 0.0
            while t < spf:
                next_dt, _ = self.substep(dt, t, spf, dt_default)
                t += dt
                self.cur_time += dt
                dt = next_dt
                steps += 1
                if self.forces:
                    self.serve_forces()
                if self.sinks:
                    self.serve_sinks()
                if self.emitters:
                    self.serve_emitters()
            if on_frame:
                on_frame(frame, self)
        return steps

    # ---- output (gmpm_simulator.cuh:594-634) ------------------------------------------------------
    def retrieve_positions(self, model=0):
        n = C.c_size_t(self.models[model]["n"])
        xyz = np.empty((n.value, 3), dtype=np.float32)
        self._check(self.api.retrieve_positions(self.ctx, model, xyz.ctypes.data_as(C.c_void_p), C.byref(n)))
        return xyz[: n.value]

    def retrieve_state(self, model=0):
        n = C.c_size_t(self.models[model]["n"])
        xyz = np.empty((n.value, 3), dtype=np.float32)
        st = np.empty((n.value, 9), dtype=np.float32)
        lj = np.empty((n.value,), dtype=np.float32)
        self._check(self.api.retrieve_state(self.ctx, model, xyz.ctypes.data_as(C.c_void_p),
                                            st.ctypes.data_as(C.c_void_p), lj.ctypes.data_as(C.c_void_p), C.byref(n)))
        k = n.value
        return xyz[:k], st[:k], lj[:k]

    def retrieve_velocity(self, model=0, affine=False):
        """Per-particle velocity read out from the grid of the last P2G (mpm_retrieve_velocity, HIP library only): (xyz, v) or, with
        affine=True, (xyz, v, C) in one particle order.  v_p = sum_i w_ip p_i / m_i over G2P's stencil, before the next grid update
        (no gravity, walls or collision object); C: (n, 3, 3) with C[p, r, c] = C_rc = D^-1 sum_i w_ip v_ir (x_i - x_p)_c."""
        n = C.c_size_t(self.models[model]["n"])
        xyz = np.empty((n.value, 3), dtype=np.float32)
        vel = np.empty((n.value, 3), dtype=np.float32)
        aff = np.empty((n.value, 9), dtype=np.float32) if affine else None
        self._check(self.api.retrieve_velocity(self.ctx, model, xyz.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p),
                                               aff.ctypes.data_as(C.c_void_p) if affine else None, C.byref(n)))
        k = n.value
        if not affine:
            return xyz[:k], vel[:k]
        # the library's column-major 9 floats (index 3 c + r) -> C[p, r, c]
        return xyz[:k], vel[:k], aff[:k].reshape(k, 3, 3).transpose(0, 2, 1)

    def kinetic_energy(self, model=None):
        """1/2 sum_p m_p |v_p|^2 in float64 from retrieve_velocity (m_p as model_mass); all models when model is None."""
        ids = range(len(self.models)) if model is None else [model]
        e = 0.0
        for mi in ids:
            _, v = self.retrieve_velocity(mi)
            e += 0.5 * self.model_mass(mi) * float(np.sum(v.astype(np.float64) ** 2))
        return e

    def particle_momentum(self, model=None):
        """Totals of the velocity readout, summed on the device in float64 (mpm_particle_momentum, HIP library only): {"count", "momentum":
        sum_p m_p v_p (3,), "kinetic": sum_p 1/2 m_p |v_p|^2}; all models when model is None."""
        out = (C.c_double * 5)()
        self._check(self.api.particle_momentum(self.ctx, -1 if model is None else int(model), out))
        return momentum_dict(out)

    def retrieve_stress(self, model=0):
        """Per-particle stress evaluated from the stored state (mpm_retrieve_stress, HIP library only): (xyz, stress6, scalars3) in one
        particle order.  stress6: the Cauchy stress {xx, yy, zz, xy, xz, yz}; scalars3: {J, pressure = -tr sigma / 3, von Mises q}.  xyz has
        the bits retrieve_state returns, so the two can be joined on them.  The J-fluid's stress is its Tait pressure alone."""
        n = C.c_size_t(self.models[model]["n"])
        xyz = np.empty((n.value, 3), dtype=np.float32)
        s6 = np.empty((n.value, 6), dtype=np.float32)
        sc = np.empty((n.value, 3), dtype=np.float32)
        self._check(self.api.retrieve_stress(self.ctx, model, xyz.ctypes.data_as(C.c_void_p), s6.ctypes.data_as(C.c_void_p),
                                             sc.ctypes.data_as(C.c_void_p), C.byref(n)))
        k = n.value
        return xyz[:k], s6[:k], sc[:k]

    def stress_totals(self, model=None):
        """Totals of the stress readout, reduced on the device (mpm_stress_totals, HIP library only): {"count", "stress_integral":
        sum_p V0 tau_p = sum_p V_p sigma_p (6,), "max_von_mises"}; all models when model is None."""
        out = (C.c_double * 8)()
        self._check(self.api.stress_totals(self.ctx, -1 if model is None else int(model), out))
        return stress_totals_dict(out)

    def retrieve_ids(self, model=0):
        """(xyz, ids) of every bucketed particle of `model` in one order (mpm_retrieve_ids; a track_ids=True engine only).  ids: int32, the
        particle's index in the positions init_model was given; xyz has the bits every other readout returns for that particle."""
        n = C.c_size_t(self.models[model]["n"])
        xyz = np.empty((n.value, 3), dtype=np.float32)
        ids = np.empty((n.value,), dtype=np.int32)
        self._check(self.api.retrieve_ids(self.ctx, model, xyz.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), C.byref(n)))
        return xyz[: n.value], ids[: n.value]

    def order_by_id(self, model, xyz, *arrays):
        """Join a readout of `model` - its positions `xyz` and any arrays in the same row order (retrieve_state, retrieve_velocity,
        retrieve_stress, taken at the same substep boundary as this call) - to the ids on the position bits: returns (ids, xyz, *arrays)
        with the rows in ascending id order.  Particles of one model whose positions are bit-identical cannot be told apart by the join:
        among them the rows are handed out in ascending id order, as they stand in the readout."""
        return join_by_position(*self.retrieve_ids(model), xyz, *arrays)

    def save_particle_ids(self):
        """The companion of save_checkpoint as a numpy byte array: one int32 per slot of every model's source bins behind a small
        header (mpm_particle_ids_save).  The checkpoint buffer itself carries no ids."""
        n = C.c_size_t(0)
        self._check(self.api.particle_ids_size(self.ctx, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        w = C.c_size_t(0)
        self._check(self.api.particle_ids_save(self.ctx, buf.ctypes.data, buf.size, C.byref(w)))
        return buf[: w.value]

    def load_particle_ids(self, buf):
        """After load_checkpoint on a tracked engine: bring back the ids saved with that checkpoint (until then retrieve_ids refuses)."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._check(self.api.particle_ids_load(self.ctx, buf.ctypes.data, buf.size))

    def counts(self):
        c = _ffi.Counts()
        self._check(self.api.get_counts(self.ctx, C.byref(c)))
        return c

    def set_collision_object(self, sdf=None, grad=None, animate=False, **fields):
        """Install the level-set collision object of the MGSP grid update (MgspBenchmark::init_boundary,
        mgsp_benchmark.cuh:257-266).  sdf: (N, N, N) float32 node values, grad: (3, N, N, N); fields: type, friction, scale,
        dsdt, trans, trans_vel, omega, rot_mat, time.  sdf=None removes the object.  The object's clock is left stopped at
        `time`; animate=True starts it there (set_collision_clock): the object then moves with every grid update."""
        if sdf is None:
            self._check(self.api.set_collision_object(self.ctx, None, None, None, None, None))
            return
        obj = _ffi.CollisionObject()
        self._check(self.api.default_collision_object(C.byref(obj)))
        for k, v in fields.items():
            cur = getattr(obj, k)
            if hasattr(cur, "__len__"):
                for i, x in enumerate(np.asarray(v, dtype=np.float32).ravel()):
                    cur[i] = float(x)
            else:
                setattr(obj, k, v)
        n = 1 << self.cfg.domain_bits
        sdf = np.ascontiguousarray(sdf, dtype=np.float32)
        grad = np.ascontiguousarray(grad, dtype=np.float32)
        assert sdf.shape == (n, n, n) and grad.shape == (3, n, n, n), (sdf.shape, grad.shape)
        self._check(self.api.set_collision_object(self.ctx, C.byref(obj), sdf.ctypes.data, grad[0].ctypes.data,
                                                  grad[1].ctypes.data, grad[2].ctypes.data))
        if animate:
            self.set_collision_clock(True, float(obj.time))

    def set_collision_shape(self, slot, kind=None, *, a=(0.0, 0.0, 0.0), b=(0.0, 0.0, 0.0), radius=0.0, inside_out=False, animate=False, **fields):
        """Install an analytic collision shape in slot 0 .. 3 (mpm_set_collision_shape, HIP engine only).  kind: "halfspace" (a: a point of
        the plane, b: outward normal), "sphere" (a: centre, radius), "box" (a: centre, b: half extents), "capsule" (a, b: end points,
        radius) or the MPM_SHAPE_* number; kind=None empties the slot.  fields: those of set_collision_object (type, friction, scale, dsdt,
        trans, trans_vel, omega, rot_mat, time).  The shape is given in the coordinates a level set's samples would be given in.  Every
        install leaves the one clock stopped at `time`: install all colliders, then start it - or pass animate=True with the last one."""
        if kind is None:
            self._check(self.api.set_collision_shape(self.ctx, int(slot), None, None))
            self._slot_geometry(slot, None)
            return
        obj = _ffi.CollisionObject()
        self._check(self.api.default_collision_object(C.byref(obj)))
        for k, v in fields.items():
            cur = getattr(obj, k)
            if hasattr(cur, "__len__"):
                for i, x in enumerate(np.asarray(v, dtype=np.float32).ravel()):
                    cur[i] = float(x)
            else:
                setattr(obj, k, v)
        sh = _ffi.CollisionShape()
        sh.kind = _ffi.SHAPE_NAMES[kind] if isinstance(kind, str) else int(kind)
        sh.inside_out = 1 if inside_out else 0
        for d in range(3):
            sh.a[d], sh.b[d] = float(a[d]), float(b[d])
        sh.radius = float(radius)
        self._check(self.api.set_collision_shape(self.ctx, int(slot), C.byref(obj), C.byref(sh)))
        self._slot_geometry(slot, ("shape", sh))
        if animate:
            self.set_collision_clock(True, float(obj.time))

    def set_force_field(self, slot, kind=None, *, vec=(0.0, 0.0, 0.0), centre=(0.0, 0.0, 0.0), strength=0.0, swirl=0.0, pull=0.0, lift=0.0, soft=0.0,
                        falloff=0, region=None, feather=0.0):
        """Install a force field in slot 0 .. 3 (mpm_set_force_field, HIP engine only) at a substep boundary; kind=None empties the slot.  kind:
        "uniform" (vec: the acceleration), "point" (centre, strength, falloff 0..2, soft), "vortex" (vec: the axis through centre; swirl, pull,
        lift), "drag" (toward the velocity vec at the rate strength) or the MPM_FORCE_* number.  region: a dict in the vocabulary
        Engine.remove(regions=...) takes, in domain coordinates (None: everywhere), with a soft edge `feather` wide.  Every grid update then
        applies the installed fields to every grid node with mass before walls, gravity and colliders, slots in order."""
        if kind is None:
            self._check(self.api.set_force_field(self.ctx, int(slot), None))
            return
        f = _ffi.ForceField()
        f.kind = _ffi.FORCE_NAMES[kind] if isinstance(kind, str) else int(kind)
        f.falloff = int(falloff)
        for d in range(3):
            f.vec[d], f.centre[d] = float(vec[d]), float(centre[d])
        f.strength, f.swirl, f.pull, f.lift, f.soft, f.feather = float(strength), float(swirl), float(pull), float(lift), float(soft), float(feather)
        if region is not None:
            f.region = self._sink_regions("set_force_field", region)[0][0]
        self._check(self.api.set_force_field(self.ctx, int(slot), C.byref(f)))

    def force_fields(self):
        """The four slots as installed (mpm_get_force_field: unit axis, unit region normal): a list of dicts with set_force_field's keywords,
        None for an empty slot."""
        names = {v: k for k, v in _ffi.FORCE_NAMES.items()}
        shapes = {v: k for k, v in _ffi.SHAPE_NAMES.items()}
        out = []
        for slot in range(_ffi.MAX_FORCE_FIELDS):
            f = _ffi.ForceField()
            self._check(self.api.get_force_field(self.ctx, slot, C.byref(f)))
            if f.kind == 0:
                out.append(None)
                continue
            r = f.region
            region = None if r.kind == 0 else {"kind": shapes[r.kind], "a": tuple(r.a), "b": tuple(r.b), "radius": r.radius, "inside_out": bool(r.inside_out)}
            out.append({"kind": names[f.kind], "vec": tuple(f.vec), "centre": tuple(f.centre), "strength": f.strength, "swirl": f.swirl, "pull": f.pull,
                        "lift": f.lift, "soft": f.soft, "falloff": f.falloff, "region": region, "feather": f.feather})
        return out

    def serve_forces(self, t=None):
        """Install or remove what every attached force entry (scenes.ForceEntry; build_engine attaches a scene's "forces", entry i in slot i) asks
        for at the substep boundary `t` (default: cur_time).  Returns the number of slots changed."""
        t = self.cur_time if t is None else t
        changed = 0
        for slot, fe in enumerate(self.forces):
            act = fe.due(t)
            if act > 0:
                self.set_force_field(slot, **fe.field)
            elif act < 0:
                self.set_force_field(slot, None)
            changed += act != 0
        return changed

    def set_collision_heightfield(self, slot, heights=None, *, origin=(0.0, 0.0), spacing=None, inside_out=False, animate=False, **fields):
        """Install a heightfield - terrain y = h(x, z) in material coordinates - in slot 0 .. 3 (mpm_set_collision_heightfield, HIP engine
        only).  heights: a 2-D array of shape [nx, nz], sample (i, k) at material (origin[0] + i spacing, origin[1] + k spacing);
        heights=None empties the slot.  inside_out: the solid is above the surface (a ceiling).  fields: those of set_collision_object (type,
        friction, scale, dsdt, trans, trans_vel, omega, rot_mat, time).  Outside the table's footprint the collider touches nothing.  The
        slots are the shapes' (set_collision_shape); every install leaves the one clock stopped at `time`."""
        if heights is None:
            self._check(self.api.set_collision_heightfield(self.ctx, int(slot), None, None, None))
            self._slot_geometry(slot, None)
            return
        if spacing is None:
            raise ValueError("set_collision_heightfield: spacing is required")
        obj = _ffi.CollisionObject()
        self._check(self.api.default_collision_object(C.byref(obj)))
        for k, v in fields.items():
            cur = getattr(obj, k)
            if hasattr(cur, "__len__"):
                for i, x in enumerate(np.asarray(v, dtype=np.float32).ravel()):
                    cur[i] = float(x)
            else:
                setattr(obj, k, v)
        h = np.ascontiguousarray(heights, dtype=np.float32)
        if h.ndim != 2:
            raise ValueError(f"set_collision_heightfield: heights must be 2-D [nx, nz], got shape {h.shape}")
        hf = _ffi.Heightfield()
        hf.nx, hf.nz = h.shape
        hf.origin[0], hf.origin[1] = float(origin[0]), float(origin[1])
        hf.spacing = float(spacing)
        hf.inside_out = 1 if inside_out else 0
        self._check(self.api.set_collision_heightfield(self.ctx, int(slot), C.byref(obj), C.byref(hf), h.ctypes.data))
        self._slot_geometry(slot, None)
        if animate:
            self.set_collision_clock(True, float(obj.time))

    def set_collision_mesh(self, vertices, faces, inside_out=False, animate=False, **fields):
        """Install the level-set collision object from a closed triangle mesh (mpm_set_collision_mesh, HIP engine only): the field is built
        on the device - exact point-triangle distance, sign from angle-weighted pseudonormals - with no N^3 host array.  vertices: (nv, 3)
        in the coordinates a level set's samples are given in (node (i, j, k) samples (i, j, k) dx); faces: (nt, 3) vertex indices,
        counter-clockwise seen from outside - what isosurface(weld=True) returns.  inside_out: the solid is the complement (a container).
        fields: those of set_collision_object.  It replaces a level-set object installed either way; set_collision_object() removes it."""
        obj = _ffi.CollisionObject()
        self._check(self.api.default_collision_object(C.byref(obj)))
        for k, v in fields.items():
            cur = getattr(obj, k)
            if hasattr(cur, "__len__"):
                for i, x in enumerate(np.asarray(v, dtype=np.float32).ravel()):
                    cur[i] = float(x)
            else:
                setattr(obj, k, v)
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"set_collision_mesh: vertices must be (nv, 3) and faces (nt, 3), got {v.shape} and {f.shape}")
        opt = _ffi.CollisionMesh()
        opt.inside_out = 1 if inside_out else 0
        self._check(self.api.set_collision_mesh(self.ctx, C.byref(obj), C.byref(opt), v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0]))
        if animate:
            self.set_collision_clock(True, float(obj.time))

    def _collision_obj(self, fields):
        obj = _ffi.CollisionObject()
        self._check(self.api.default_collision_object(C.byref(obj)))
        for k, v in fields.items():
            cur = getattr(obj, k)
            if hasattr(cur, "__len__"):
                for i, x in enumerate(np.asarray(v, dtype=np.float32).ravel()):
                    cur[i] = float(x)
            else:
                setattr(obj, k, v)
        return obj

    def set_collision_volume(self, slot, field4=None, *, origin=(0.0, 0.0, 0.0), spacing=None, inside_out=False, animate=False, **fields):
        """Install a volume - a local level-set box - in slot 0 .. 3 (mpm_set_collision_volume, HIP engine only).  field4: an array of shape
        [d0, d1, d2, 4] = {sdis, gx, gy, gz} per sample, sample (i, j, k) at material origin + (i, j, k) spacing; field4=None empties the
        slot.  inside_out: sdis and n change sign at the query.  fields: those of set_collision_object (type, friction, scale, dsdt, trans,
        trans_vel, omega, rot_mat, time).  Outside the table's footprint the collider touches nothing.  The slots are the shapes'
        (set_collision_shape); every install leaves the one clock stopped at `time`."""
        if field4 is None:
            self._check(self.api.set_collision_volume(self.ctx, int(slot), None, None, None))
            self._slot_geometry(slot, None)
            return
        if spacing is None:
            raise ValueError("set_collision_volume: spacing is required")
        obj = self._collision_obj(fields)
        t = np.ascontiguousarray(field4, dtype=np.float32)
        if t.ndim != 4 or t.shape[3] != 4:
            raise ValueError(f"set_collision_volume: field4 must be [d0, d1, d2, 4], got shape {t.shape}")
        vol = _ffi.CollisionVolume()
        for d in range(3):
            vol.dims[d], vol.origin[d] = t.shape[d], float(origin[d])
        vol.spacing = float(spacing)
        vol.inside_out = 1 if inside_out else 0
        self._check(self.api.set_collision_volume(self.ctx, int(slot), C.byref(obj), C.byref(vol), t.ctypes.data))
        self._slot_geometry(slot, None)
        if animate:
            self.set_collision_clock(True, float(obj.time))

    def set_collision_volume_mesh(self, slot, vertices, faces, *, spacing=None, origin=None, dims=None, pad=2, inside_out=False, animate=False, **fields):
        """Install a volume built on the device from a closed triangle mesh (mpm_set_collision_volume_mesh, HIP engine only).  vertices: (nv, 3)
        in material coordinates; faces: (nt, 3), counter-clockwise seen from outside.  dims=None: the box is sized from the mesh's bounding
        box with `pad` cells of margin (origin is then not used); else origin and dims give the box.  collision_volume(slot) returns the
        descriptor as installed.  fields: those of set_collision_object."""
        if spacing is None:
            raise ValueError("set_collision_volume_mesh: spacing is required")
        if dims is not None and origin is None:
            raise ValueError("set_collision_volume_mesh: dims without origin")
        obj = self._collision_obj(fields)
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"set_collision_volume_mesh: vertices must be (nv, 3) and faces (nt, 3), got {v.shape} and {f.shape}")
        vol = _ffi.CollisionVolume()
        for d in range(3):
            vol.dims[d] = 0 if dims is None else int(dims[d])
            vol.origin[d] = 0.0 if dims is None else float(origin[d])
        vol.spacing = float(spacing)
        vol.inside_out = 1 if inside_out else 0
        vol.pad = int(pad)
        self._check(self.api.set_collision_volume_mesh(self.ctx, int(slot), C.byref(obj), C.byref(vol), v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0]))
        self._slot_geometry(slot, ("mesh", v, f))
        if animate:
            self.set_collision_clock(True, float(obj.time))

    def collision_volume(self, slot, lo=None, shape=None):
        """The volume in `slot` (mpm_get_collision_volume): (descriptor, array) with descriptor = dict(dims, origin, spacing, inside_out, pad)
        as installed and array = (b0, b1, b2, 4) float32 {sdis, gx, gy, gz} of the samples lo + [0, shape), bit for bit.  lo=None: from
        sample (0, 0, 0); shape=None: to the end of the table."""
        vol = _ffi.CollisionVolume()
        self._check(self.api.get_collision_volume(self.ctx, int(slot), C.byref(vol), None, None, None))
        desc = dict(dims=tuple(vol.dims), origin=tuple(np.float32(x) for x in vol.origin), spacing=np.float32(vol.spacing), inside_out=bool(vol.inside_out), pad=int(vol.pad))
        lo = [0, 0, 0] if lo is None else [int(x) for x in lo]
        shape = [desc["dims"][d] - lo[d] for d in range(3)] if shape is None else [int(x) for x in shape]
        out = np.empty(tuple(shape) + (4,) if min(shape) >= 1 else (1,), dtype=np.float32)
        self._check(self.api.get_collision_volume(self.ctx, int(slot), None, (C.c_int * 3)(*lo), (C.c_int * 3)(*shape), out.ctypes.data))
        return desc, out

    def collision_field(self, lo=(0, 0, 0), shape=None):
        """The installed level-set field, however it was installed (mpm_get_collision_field): (d0, d1, d2, 4) float32 {sdis, gx, gy, gz} of
        the nodes lo + [0, shape), bit for bit.  shape=None: from lo to the end of the domain."""
        n = 1 << self.cfg.domain_bits
        lo = [int(v) for v in lo]
        shape = [n - v for v in lo] if shape is None else [int(v) for v in shape]
        out = np.empty(tuple(shape) + (4,) if min(shape) >= 1 else (1,), dtype=np.float32)
        self._check(self.api.get_collision_field(self.ctx, (C.c_int * 3)(*lo), (C.c_int * 3)(*shape), out.ctypes.data))
        return out

    def set_collision_clock(self, running=True, time=0.0):
        """Set the collision object's time and start (or stop) its clock: a running clock advances by dt with every grid update,
        the update of a substep sees the object at the time the substep starts (HIP engine only)."""
        self._check(self.api.set_collision_clock(self.ctx, 1 if running else 0, float(time)))

    def collision_time(self):
        """The collision object's current time: where the next grid update will see it (HIP engine only)."""
        t = C.c_float(0)
        self._check(self.api.get_collision_time(self.ctx, C.byref(t), None))
        return t.value

    def collision_clock_running(self):
        running = C.c_int(0)
        self._check(self.api.get_collision_time(self.ctx, None, C.byref(running)))
        return bool(running.value)

    def save_checkpoint(self):
        """Full state at the current substep boundary as a numpy byte array (HIP engine only)."""
        n = C.c_size_t(0)
        self._check(self.api.checkpoint_size(self.ctx, C.byref(n)))
        buf = np.zeros(n.value, dtype=np.uint8)  # (zeros: the padding between the sections is no part of what the library writes)
        w = C.c_size_t(0)
        self._check(self.api.checkpoint_save(self.ctx, buf.ctypes.data, buf.size, C.byref(w)))
        return buf[: w.value]

    def load_checkpoint(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._check(self.api.checkpoint_load(self.ctx, buf.ctypes.data, buf.size))

    def capacity(self):
        """(block capacity, per-model bin capacities, number of growth events) - HIP engine only."""
        blocks, bins, events = C.c_int64(0), (C.c_int64 * 8)(), C.c_int(0)
        self._check(self.api.get_capacity(self.ctx, C.byref(blocks), bins, C.byref(events)))
        return blocks.value, list(bins), events.value

    def model_mass(self, model=0):
        """Particle mass of a model: volume * rho (particle_buffer.cuh:158,:186,:252)."""
        p = self.models[model]["params"]
        return float(np.float32(p.volume) * np.float32(p.rho))

    def diagnostics(self):
        """Particles / P2G contributions the reference would have lost silently, and `still_rebuilds`: the rebuilds of run_fixed that kept the
        partition because no particle had changed its block (config `still_rebuild=-1` switches that off).  HIP library only."""
        d = _ffi.Diagnostics()
        self._check(self.api.get_diagnostics(self.ctx, C.byref(d)))
        return d

    def timers(self):
        t = _ffi.Timers()
        self._check(self.api.get_timers(self.ctx, C.byref(t)))
        return t

    def grid_totals(self):
        out = (C.c_double * 4)()
        self._check(self.api.grid_totals(self.ctx, out))
        return np.array(list(out))

    def dump_grid(self):
        cnt = self.counts()
        n = C.c_size_t(cnt.neighbor_blocks)
        keys = np.empty((n.value, 3), dtype=np.int32)
        blocks = np.empty((n.value, 4, 64), dtype=np.float32)
        self._check(self.api.dump_grid(self.ctx, keys.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p), C.byref(n)))
        return keys[: n.value], blocks[: n.value]

    def dump_block_rows(self, model=0):
        """The 64-int look-up rows of `model`, one per particle block of the current numbering (mpm_dump_block_rows; HIP library only):
        (particle blocks, 64) int32 - [0, 27) source bin offsets, [27, 54) destination block numbers, [54, 62) grid block numbers."""
        n = C.c_size_t(self.counts().particle_blocks)
        rows = np.empty((n.value, 64), dtype=np.int32)
        self._check(self.api.dump_block_rows(self.ctx, int(model), rows.ctypes.data_as(C.c_void_p), C.byref(n)))
        return rows[: n.value]

    # ---- Eulerian readouts (mpm_sample_grid, mpm_grid_volume, mpm_grid_box_totals; HIP library only) ------------------------------
    def sample_grid(self, xyz):
        """The grid of the last P2G sampled at arbitrary world-space points with G2P's 27-node B-spline stencil (mpm_sample_grid):
        {"mass": sum W m (n,) float32, "momentum": sum W p (n, 3) float32, "density": mass / dx^3 (n,) float64, "velocity": momentum / mass
        where mass > 0, else 0 (n, 3) float64 - the mass-weighted velocity, not retrieve_velocity's sum W (p / m)}.  Points outside the
        domain (or not finite) give zeros."""
        pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((pts.shape[0], 4), dtype=np.float32)
        self._check(self.api.sample_grid(self.ctx, pts.ctypes.data_as(C.c_void_p), pts.shape[0], out.ctypes.data_as(C.c_void_p)))
        mass, mom = out[:, 0].copy(), out[:, 1:4].copy()
        m64 = mass.astype(np.float64)
        vel = np.zeros(mom.shape, dtype=np.float64)
        np.divide(mom.astype(np.float64), m64[:, None], out=vel, where=(m64 > 0)[:, None])
        return {"mass": mass, "momentum": mom, "density": m64 / self.dx ** 3, "velocity": vel}

    def grid_volume(self, origin=(0, 0, 0), shape=None, stride=1):
        """A dense box of the grid of the last P2G (mpm_grid_volume): a (4, d0, d1, d2) float32 array {mass, px, py, pz}, cell (X, Y, Z) the
        sum over the stride^3 nodes at origin + stride (X, Y, Z) (stride 1: the node's words, bit for bit).  shape=None: the whole domain
        at that stride, from `origin` (0, 0, 0).  Nodes outside the domain or in no registered block read zero."""
        stride = int(stride)
        if shape is None:
            if stride not in (1, 2, 4):
                raise EngineError(_ffi.MPM_ERR_INVALID, f"grid_volume: stride {stride} (1, 2 or 4)")
            shape = ((1 << self.cfg.domain_bits) // stride,) * 3
        o = (C.c_int * 3)(*[int(v) for v in origin])
        d = (C.c_int * 3)(*[int(v) for v in shape])
        # (a dims entry < 1 is the library's to refuse, before it writes anything: it gets a one-word array)
        out = np.empty((4,) + tuple(d) if min(d) >= 1 else (1,), dtype=np.float32)
        self._check(self.api.grid_volume(self.ctx, o, d, stride, out.ctypes.data_as(C.c_void_p)))
        return out

    def grid_box_totals(self, lo, hi):
        """Totals over the nodes of the half-open node box [lo, hi), clipped to the domain (mpm_grid_box_totals), in float64: {"mass",
        "momentum" (3,), "kinetic": sum over nodes with mass > 0 of |p|^2 / (2 m)}."""
        out = (C.c_double * 5)()
        self._check(self.api.grid_box_totals(self.ctx, (C.c_int * 3)(*[int(v) for v in lo]), (C.c_int * 3)(*[int(v) for v in hi]), out))
        return {"mass": float(out[0]), "momentum": np.array(out[1:4], dtype=np.float64), "kinetic": float(out[4])}

    def isosurface(self, density=None, iso_mass=None, box=None, velocity=False, weld=True):
        """The iso-surface of the mass grid of the last P2G (mpm_grid_isosurface): marching tetrahedra over the registered blocks, watertight.
        Exactly one of `density` (mass per volume; the iso value is density * dx^3) and `iso_mass` (node mass) is given.  box = (lo, hi): only
        the cells lo <= (i, j, k) < hi.  weld=True: (V (nv, 3) float32, F (nf, 3) int32[, vel (nv, 3) float32]) - vertices welded on their
        position bits (shared edges give identical bits), the velocity of a vertex taken from its first occurrence, triangles with two
        equal indices dropped; the normals point out of the material.  weld=False: the raw soup (nt, 3, 3) float32[, velocities (nt, 3, 3)]."""
        if (density is None) == (iso_mass is None):
            raise EngineError(_ffi.MPM_ERR_INVALID, "isosurface: give exactly one of density and iso_mass")
        iso = float(np.float32(iso_mass if density is None else density * self.dx ** 3))
        lo = hi = None
        if box is not None:
            lo, hi = ((C.c_int * 3)(*[int(v) for v in b]) for b in box)
        n = C.c_size_t(0)
        self._check(self.api.grid_isosurface(self.ctx, iso, lo, hi, None, None, C.byref(n)))          # count, then fetch
        tris = np.empty((n.value, 3, 3), dtype=np.float32)
        vel = np.empty((n.value, 3, 3), dtype=np.float32) if velocity else None
        if n.value:
            self._check(self.api.grid_isosurface(self.ctx, iso, lo, hi, tris.ctypes.data_as(C.c_void_p),
                                                 vel.ctypes.data_as(C.c_void_p) if velocity else None, C.byref(n)))
        if not weld:
            return (tris, vel) if velocity else tris
        return weld_triangles(tris, vel)

    # ---- collider loads (mpm_collider_loads.hpp) ----
    @staticmethod
    def _load_options(pivots):
        """pivots: None, or {row name or number: (x, y, z)} -> mpm_load_options or None."""
        if not pivots:
            return None
        opt = _ffi.LoadOptions()
        for key, p in pivots.items():
            r = _ffi.LOAD_ROW_NAMES.index(key) if isinstance(key, str) else int(key)
            if not 0 <= r < _ffi.LOAD_ROWS:
                raise EngineError(_ffi.MPM_ERR_INVALID, f"collider loads: no row {key!r}")
            opt.has_pivot[r] = 1
            for d in range(3):
                opt.pivot[r][d] = float(p[d])
        return C.byref(opt)

    @staticmethod
    def _load_rows(out, seconds):
        """[row][8] impulses -> {row name: {count, impulse, angular_impulse, force, torque, mass}}; force and torque are the impulses over `seconds`."""
        a = np.ctypeslib.as_array(out).reshape(_ffi.LOAD_ROWS, 8).astype(np.float64)
        with np.errstate(all="ignore"):
            return {name: {"count": int(a[r, 0]) if np.isfinite(a[r, 0]) else a[r, 0], "impulse": a[r, 1:4].copy(), "angular_impulse": a[r, 4:7].copy(),
                           "force": a[r, 1:4] / seconds, "torque": a[r, 4:7] / seconds, "mass": float(a[r, 7])} for r, name in enumerate(_ffi.LOAD_ROW_NAMES)}

    def collider_loads(self, dt, pivots=None):
        """What the next grid update with this dt will put on every collider (mpm_collider_loads; read-only, the grid must hold the last P2G's
        momenta): {"field", "slot0" .. "slot3", "walls"} -> {count: touched nodes, impulse (3,), angular_impulse (3,) about the row's pivot,
        force = impulse / dt, torque = angular_impulse / dt, mass: touched mass}, all float64, the loads ON the collider.  pivots: {row: (x, y, z)}
        replaces a row's default pivot (the collider's trans + trans_vel T; the origin for the walls)."""
        out = (C.c_double * 8 * _ffi.LOAD_ROWS)()
        self._check(self.api.collider_loads(self.ctx, float(dt), self._load_options(pivots), out))
        return self._load_rows(out, float(np.float32(dt)))

    def collider_contacts(self, dt):
        """The contact map behind collider_loads (mpm_collider_contacts): (nodes (n, 3) int32, rows (n,) int32, mass (n,) float32, dv (n, 3)
        float32, v_after (n, 3) float32), one entry per touched (node, row), in no particular order."""
        n = C.c_size_t(0)
        self._check(self.api.collider_contacts(self.ctx, float(dt), None, None, C.byref(n)))               # count, then fetch
        nr = np.empty((n.value, 4), dtype=np.int32)
        rec = np.empty((n.value, 8), dtype=np.float32)
        if n.value:
            self._check(self.api.collider_contacts(self.ctx, float(dt), nr.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), C.byref(n)))
        return nr[:, :3].copy(), nr[:, 3].copy(), rec[:, 0].copy(), rec[:, 1:4].copy(), rec[:, 4:7].copy()

    def load_gauge(self, on=True, pivots=None):
        """Switch the load gauge (mpm_load_gauge): on, every grid update of grid_update / substep / run_fixed adds its loads to accumulators on
        the device first, and run_fixed applies every update in a kernel of its own (same results).  Switching it on zeroes the accumulators."""
        self._check(self.api.load_gauge(self.ctx, 1 if on else 0, self._load_options(pivots)))

    def read_load_gauge(self, reset=True):
        """-> (rows, elapsed, updates): collider_loads' rows summed over the `updates` grid updates since the gauge was zeroed, force and torque
        the impulses over `elapsed`, the float64 sum of their dts (nan before the first update)."""
        out = (C.c_double * 8 * _ffi.LOAD_ROWS)()
        elapsed, updates = C.c_double(0), C.c_int(0)
        self._check(self.api.load_gauge_read(self.ctx, out, C.byref(elapsed), C.byref(updates), 1 if reset else 0))
        return self._load_rows(out, elapsed.value), elapsed.value, updates.value

    # ---- rigid bodies (mpm_rigid_body.hpp) ----
    def _slot_geometry(self, slot, what):
        """What set_collider_body(density=...) integrates over: the analytic shape or the mesh the slot was given (None: neither)."""
        self._slot_geom[int(slot)] = what

    @staticmethod
    def shape_mass_properties(kind, density, a=(0.0, 0.0, 0.0), b=(0.0, 0.0, 0.0), radius=0.0, api=None):
        """mass, inertia (6,) {xx yy zz xy xz yz} about com, com (3,) of a homogeneous sphere, box or capsule (mpm_shape_mass_properties; no device)."""
        api = api if api is not None else _ffi.load_hip()
        sh = _ffi.CollisionShape()
        sh.kind = _ffi.SHAPE_NAMES[kind] if isinstance(kind, str) else int(kind)
        for d in range(3):
            sh.a[d], sh.b[d] = float(a[d]), float(b[d])
        sh.radius = float(radius)
        out = _ffi.RigidBody()
        rc = api.shape_mass_properties(C.byref(sh), float(density), C.byref(out))
        if rc:
            raise EngineError(rc, "shape_mass_properties: the shape has no mass properties (unbounded, degenerate or density <= 0)")
        return float(out.mass), np.array(out.inertia[:], dtype=np.float32), np.array(out.com[:], dtype=np.float32)

    @staticmethod
    def mesh_mass_properties(vertices, faces, density, api=None):
        """The same of a closed, outward-oriented triangle mesh (mpm_mesh_mass_properties; float64 polyhedral integrals, no device)."""
        api = api if api is not None else _ffi.load_hip()
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"mesh_mass_properties: vertices must be (nv, 3) and faces (nt, 3), got {v.shape} and {f.shape}")
        out = _ffi.RigidBody()
        rc = api.mesh_mass_properties(v.ctypes.data, v.shape[0], f.ctypes.data, f.shape[0], float(density), C.byref(out))
        if rc:
            raise EngineError(rc, "mesh_mass_properties: the mesh is refused (not closed, degenerate, no positive volume) or density <= 0")
        return float(out.mass), np.array(out.inertia[:], dtype=np.float32), np.array(out.com[:], dtype=np.float32)

    def set_collider_body(self, slot, mass=None, inertia=None, com=None, density=None, gravity=True, lock="", force=(0.0, 0.0, 0.0), torque=(0.0, 0.0, 0.0)):
        """Make the collider in `slot` a rigid body (mpm_set_collider_body): from now on its pose and velocity are state on the device, advanced at
        every grid update by the impulse the material puts on it.  mass, inertia (6 values xx yy zz xy xz yz, body frame, about com) and com
        (material coordinates) are given, or density= fills those not given from the slot's analytic shape or the mesh of
        set_collision_volume_mesh.  lock: a string such as "x z rx ry" (world translations x y z, rotations rx ry rz) or the bit mask.  force,
        torque: constant, world.  mass=None and density=None: the slot is prescribed again, at rest at the pose it has reached."""
        if mass is None and density is None:
            if inertia is not None or com is not None or lock or tuple(force) != (0.0, 0.0, 0.0) or tuple(torque) != (0.0, 0.0, 0.0):
                raise EngineError(_ffi.MPM_ERR_INVALID, "set_collider_body: constants without mass= or density= (with neither the slot is released from its body)")
            self._check(self.api.set_collider_body(self.ctx, int(slot), None))
            return
        if density is not None:
            geom = self._slot_geom.get(int(slot))
            if geom is None:
                raise EngineError(_ffi.MPM_ERR_INVALID, "set_collider_body: density= needs a slot holding an analytic shape or a volume built from a mesh")
            if geom[0] == "shape":
                sh = geom[1]
                m, i6, c = self.shape_mass_properties(sh.kind, density, sh.a[:], sh.b[:], sh.radius, api=self.api)
            else:
                m, i6, c = self.mesh_mass_properties(geom[1], geom[2], density, api=self.api)
            mass = m if mass is None else mass
            inertia = i6 if inertia is None else inertia
            com = c if com is None else com
        if inertia is None or com is None:
            raise EngineError(_ffi.MPM_ERR_INVALID, "set_collider_body: mass, inertia and com are given together (or density=)")
        body = _ffi.RigidBody()
        body.mass = float(mass)
        for i, x in enumerate(np.asarray(inertia, dtype=np.float32).ravel()[:6]):
            body.inertia[i] = float(x)
        for d in range(3):
            body.com[d], body.force[d], body.torque[d] = float(com[d]), float(force[d]), float(torque[d])
        body.gravity = 1 if gravity else 0
        body.lock = int(lock) if not isinstance(lock, str) else sum(_ffi.BODY_LOCKS[w] for w in lock.split())
        self._check(self.api.set_collider_body(self.ctx, int(slot), C.byref(body)))

    def collider_body(self, slot):
        """The body in `slot` (mpm_get_collider_body): its constants and its float64 state - position, orientation (w x y z), velocity, omega,
        angular_momentum, last_impulse, last_angular_impulse, last_touched_mass, last_touched_nodes, max_mass_ratio, updates."""
        b, st = _ffi.RigidBody(), _ffi.RigidBodyState()
        self._check(self.api.get_collider_body(self.ctx, int(slot), C.byref(b), C.byref(st)))
        out = {"mass": float(b.mass), "inertia": np.array(b.inertia[:], dtype=np.float32), "com": np.array(b.com[:], dtype=np.float32), "gravity": bool(b.gravity),
               "lock": int(b.lock), "force": np.array(b.force[:], dtype=np.float32), "torque": np.array(b.torque[:], dtype=np.float32)}
        for name in ("position", "orientation", "velocity", "omega", "angular_momentum", "last_impulse", "last_angular_impulse"):
            out[name] = np.array(getattr(st, name)[:], dtype=np.float64)
        out.update(last_touched_mass=float(st.last_touched_mass), max_mass_ratio=float(st.max_mass_ratio), last_touched_nodes=int(st.last_touched_nodes), updates=int(st.updates))
        return out

    def set_collider_body_state(self, slot, position=None, orientation=None, velocity=None, omega=None):
        """A restart (mpm_set_collider_body_state): any of position (3), orientation (w x y z), velocity (3), omega (3) replaces that part of the state."""
        def arr(v, n):
            return None if v is None else (C.c_double * n)(*[float(x) for x in v])
        self._check(self.api.set_collider_body_state(self.ctx, int(slot), arr(position, 3), arr(orientation, 4), arr(velocity, 3), arr(omega, 3)))

    def last_g2p2g_ms(self):
        ms = C.c_float(0)
        self._check(self.api.last_g2p2g_ms(self.ctx, C.byref(ms)))
        return ms.value


def weld_triangles(tris, vel=None):
    """A triangle soup (nt, 3, 3) float32 as an indexed mesh: (V (nv, 3) float32, F (nf, 3) int32[, vel (nv, 3) float32]).  Vertices are equal
    when their position bits are; V is sorted by those bits; a vertex's velocity is that of its first occurrence in the soup; triangles
    with two equal indices are dropped."""
    pts = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3)
    if pts.shape[0] == 0:
        empty = (pts.copy(), np.zeros((0, 3), dtype=np.int32))
        return empty if vel is None else empty + (np.zeros((0, 3), dtype=np.float32),)
    _, first, inverse = np.unique(pts.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    faces = inverse.reshape(-1, 3).astype(np.int32)
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])]
    if vel is None:
        return pts[first], faces
    return pts[first], faces, np.ascontiguousarray(vel, dtype=np.float32).reshape(-1, 3)[first]


def build_engine(scene, device=0, api=None):
    """Create an Engine for a scene dict (claymore_amd.scenes) and add its models (no setup yet).  scene["track_ids"]: Engine's track_ids;
    scene["emitters"]: particle sources (scenes.Emitter.from_dict), attached as Engine.emitters and served by Engine.main_loop;
    scene["sinks"]: particle sinks (scenes.Sink.from_dict), attached as Engine.sinks and served there before the emitters;
    scene["forces"]: force fields (scenes.ForceEntry.from_dict, entry i for slot i), attached as Engine.forces and served there first."""
    cfg = _ffi.Config()
    a = api if api is not None else _ffi.load_hip()
    rc = a.default_config(scene["bits"], C.byref(cfg))
    if rc:
        raise EngineError(rc, "default_config")
    for k, v in scene.get("config", {}).items():
        setattr(cfg, k, v)
    eng = Engine(cfg=cfg, device=device, api=a, track_ids=bool(scene.get("track_ids", False)))
    for m in scene["models"]:
        if "mesh" in m:  # {"vertices", "faces"[, "margin", "box"]}: filled on the device (init_model_mesh)
            eng.init_model_mesh(m["material"], v0=m.get("v0", (0, 0, 0)), **m["mesh"], **m.get("params", {}))
        else:  # "velocity", "affine", "state", "logjp" (+ "state_kind"): per-particle initial conditions, in the order of "xyz"
            eng.init_model(m["material"], m["xyz"], m.get("v0", (0, 0, 0)), velocity=m.get("velocity"), affine=m.get("affine"), state=m.get("state"),
                           logjp=m.get("logjp"), state_kind=m.get("state_kind", "b"), **m.get("params", {}))
        if m.get("omega") is not None or m.get("velocity_gradient") is not None:  # a linear velocity field about "pivot"; "v0" is its constant part
            eng.set_model_velocity_field(len(eng.models) - 1, m.get("v0", (0, 0, 0)), grad=m.get("velocity_gradient"), omega=m.get("omega"),
                                         pivot=m.get("pivot", (0, 0, 0)))
    if scene.get("collision"):
        eng.set_collision_object(**{**scene["collision"], "animate": False})
    if scene.get("collision_mesh"):  # the level-set object from a triangle mesh (it and "collision" are one object: the later install wins)
        eng.set_collision_mesh(**{**scene["collision_mesh"], "animate": False})
    colliders = scene.get("colliders") or []
    for slot, c in enumerate(colliders):
        body, c = c.get("body"), {k: v for k, v in c.items() if k != "body"}  # "body": {...}: Engine.set_collider_body's keywords, installed behind the collider
        if c.get("kind") == "heightfield":
            eng.set_collision_heightfield(slot, **{**{k: v for k, v in c.items() if k != "kind"}, "animate": False})
        elif c.get("kind") == "volume":
            eng.set_collision_volume(slot, **{**{k: v for k, v in c.items() if k != "kind"}, "animate": False})
        elif c.get("kind") == "volume_mesh":
            eng.set_collision_volume_mesh(slot, **{**{k: v for k, v in c.items() if k != "kind"}, "animate": False})
        else:
            eng.set_collision_shape(slot, **{**c, "animate": False})
        if body is not None:
            eng.set_collider_body(slot, **body)
    # one clock for all colliders: started once, after the last install (every install stops it)
    fields = [scene[k] for k in ("collision", "collision_mesh") if scene.get(k)]
    moving = [c for c in fields + list(colliders) if c.get("animate")]
    if moving:
        eng.set_collision_clock(True, float(moving[0].get("time", 0.0)))
    if scene.get("emitters"):  # particle sources (scenes.Emitter), served by main_loop at the substep boundaries
        from .scenes import Emitter
        eng.emitters = [Emitter.from_dict(scene["bits"], e) for e in scene["emitters"]]
    if scene.get("sinks"):  # particle sinks (scenes.Sink), served by main_loop at the substep boundaries, before the emitters
        from .scenes import Sink
        eng.sinks = [Sink.from_dict(scene["bits"], e) for e in scene["sinks"]]
    if scene.get("forces"):  # force fields (scenes.ForceEntry), installed and removed by main_loop at the substep boundaries, before the sinks
        from .scenes import ForceEntry
        if len(scene["forces"]) > _ffi.MAX_FORCE_FIELDS:
            raise ValueError(f"a scene holds at most {_ffi.MAX_FORCE_FIELDS} forces")
        eng.forces = [ForceEntry.from_dict(e) for e in scene["forces"]]
    return eng
