"""ctypes mirror of include/claymore_amd.h.

`bind(lib, prefix)` attaches argument/return types for every entry point the header declares; the
product binds libclaymore_hip.so with prefix "mpm_", the tests additionally bind the CPU oracle
(oracle/libmpm_oracle.so) with prefix "mpmo_" so both are driven through identical call sequences.
"""
import ctypes as C
import os

MPM_OK, MPM_ERR_INVALID, MPM_ERR_DEVICE, MPM_ERR_CAPACITY, MPM_ERR_NONFINITE, MPM_ERR_NOT_READY, MPM_ERR_INTERNAL = range(7)
J_FLUID, FIXED_COROTATED, SAND, NACC = range(4)
MATERIAL_NAMES = {"jfluid": J_FLUID, "fixed_corotated": FIXED_COROTATED, "sand": SAND, "nacc": NACC}


class Config(C.Structure):
    _fields_ = [("domain_bits", C.c_int), ("max_ppc", C.c_int), ("boundary_blocks", C.c_int),
                ("gravity", C.c_float), ("cfl", C.c_float), ("max_blocks", C.c_int64),
                ("grow", C.c_int), ("drop_overflow", C.c_int), ("sync_interval", C.c_int), ("still_rebuild", C.c_int),
                ("reserved", C.c_int * 2)]


class MaterialParams(C.Structure):
    _fields_ = [("rho", C.c_float), ("volume", C.c_float), ("youngs_modulus", C.c_float),
                ("poisson_ratio", C.c_float), ("bulk", C.c_float), ("gamma", C.c_float),
                ("viscosity", C.c_float), ("beta", C.c_float), ("xi", C.c_float),
                ("cohesion", C.c_float), ("yield_surface", C.c_float), ("msqr", C.c_float),
                ("log_jp0", C.c_float), ("volume_correction", C.c_int), ("hardening_on", C.c_int),
                ("reserved", C.c_int * 5)]


class CollisionObject(C.Structure):
    _fields_ = [("type", C.c_int), ("friction", C.c_float), ("scale", C.c_float), ("dsdt", C.c_float),
                ("trans", C.c_float * 3), ("trans_vel", C.c_float * 3), ("omega", C.c_float * 3),
                ("rot_mat", C.c_float * 9), ("time", C.c_float), ("reserved", C.c_int * 3)]


class CollisionShape(C.Structure):
    _fields_ = [("kind", C.c_int), ("inside_out", C.c_int), ("a", C.c_float * 3), ("b", C.c_float * 3), ("radius", C.c_float),
                ("reserved", C.c_int * 5)]


SHAPE_HALFSPACE, SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE = 1, 2, 3, 4
SHAPE_NAMES = {"halfspace": SHAPE_HALFSPACE, "sphere": SHAPE_SPHERE, "box": SHAPE_BOX, "capsule": SHAPE_CAPSULE}
MAX_COLLISION_SHAPES = 4


class Heightfield(C.Structure):
    _fields_ = [("nx", C.c_int), ("nz", C.c_int), ("origin", C.c_float * 2), ("spacing", C.c_float), ("inside_out", C.c_int),
                ("reserved", C.c_int * 6)]


HEIGHTFIELD_MAX_SAMPLES = 4096


class CollisionMesh(C.Structure):
    _fields_ = [("inside_out", C.c_int), ("reserved", C.c_int * 7)]


MESH_MAX_TRIANGLES = MESH_MAX_VERTICES = 1 << 22


class CollisionVolume(C.Structure):
    _fields_ = [("dims", C.c_int * 3), ("origin", C.c_float * 3), ("spacing", C.c_float), ("inside_out", C.c_int), ("pad", C.c_int),
                ("reserved", C.c_int * 7)]


VOLUME_MAX_SAMPLES = 1024


class MeshFill(C.Structure):
    _fields_ = [("margin", C.c_float), ("lo", C.c_int * 3), ("hi", C.c_int * 3), ("use_box", C.c_int), ("reserved", C.c_int * 8)]


STATE_F, STATE_B = 0, 1                # MPM_STATE_F, MPM_STATE_B
STATE_KINDS = {"f": STATE_F, "b": STATE_B}


class ParticleInit(C.Structure):
    _fields_ = [("velocity", C.c_void_p), ("affine9", C.c_void_p), ("state9", C.c_void_p), ("logjp", C.c_void_p),
                ("state_kind", C.c_int), ("reserved", C.c_int * 3)]


MAX_SINK_REGIONS = 8                   # MPM_MAX_SINK_REGIONS


class Removal(C.Structure):
    _fields_ = [("regions", C.POINTER(CollisionShape)), ("nregions", C.c_int), ("ids", C.c_void_p), ("nids", C.c_size_t),
                ("removed_xyz", C.c_void_p), ("removed_ids", C.c_void_p), ("removed_model", C.c_void_p), ("capacity", C.c_size_t),
                ("reserved", C.c_int * 4)]


class RemovalResult(C.Structure):
    _fields_ = [("removed", C.c_int64 * 8), ("mass", C.c_double), ("momentum", C.c_double * 3), ("relaid", C.c_int), ("reserved", C.c_int * 3)]


LOAD_ROWS = 6                          # MPM_LOAD_ROWS
LOAD_ROW_NAMES = ("field", "slot0", "slot1", "slot2", "slot3", "walls")


class LoadOptions(C.Structure):
    _fields_ = [("has_pivot", C.c_int * LOAD_ROWS), ("pivot", C.c_float * 3 * LOAD_ROWS)]


class RigidBody(C.Structure):
    _fields_ = [("mass", C.c_float), ("inertia", C.c_float * 6), ("com", C.c_float * 3), ("gravity", C.c_int), ("lock", C.c_int),
                ("force", C.c_float * 3), ("torque", C.c_float * 3), ("reserved", C.c_int * 8)]


class RigidBodyState(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("orientation", C.c_double * 4), ("velocity", C.c_double * 3), ("omega", C.c_double * 3),
                ("angular_momentum", C.c_double * 3), ("last_impulse", C.c_double * 3), ("last_angular_impulse", C.c_double * 3),
                ("last_touched_mass", C.c_double), ("max_mass_ratio", C.c_double), ("last_touched_nodes", C.c_int64), ("updates", C.c_int64)]


BODY_LOCKS = {"x": 1, "y": 2, "z": 4, "rx": 8, "ry": 16, "rz": 32}


FORCE_UNIFORM, FORCE_POINT, FORCE_VORTEX, FORCE_DRAG = 1, 2, 3, 4   # MPM_FORCE_*
FORCE_NAMES = {"uniform": FORCE_UNIFORM, "point": FORCE_POINT, "vortex": FORCE_VORTEX, "drag": FORCE_DRAG}
MAX_FORCE_FIELDS = 4                   # MPM_MAX_FORCE_FIELDS


class ForceField(C.Structure):
    _fields_ = [("kind", C.c_int), ("falloff", C.c_int), ("vec", C.c_float * 3), ("centre", C.c_float * 3), ("strength", C.c_float),
                ("swirl", C.c_float), ("pull", C.c_float), ("lift", C.c_float), ("soft", C.c_float), ("feather", C.c_float),
                ("region", CollisionShape), ("reserved", C.c_int * 6)]


class Counts(C.Structure):
    _fields_ = [("particle_blocks", C.c_int), ("neighbor_blocks", C.c_int), ("exterior_blocks", C.c_int),
                ("model_count", C.c_int), ("bins", C.c_int64 * 8), ("particles", C.c_int64 * 8)]


class Diagnostics(C.Structure):
    _fields_ = [("lost_particles", C.c_int64), ("discarded_p2g", C.c_int64), ("overflow_flags", C.c_int),
                ("dropped_particles", C.c_int), ("reserved", C.c_int * 3), ("still_rebuilds", C.c_int)]


class Timers(C.Structure):
    _fields_ = [("grid_update_ms", C.c_float), ("g2p2g_ms", C.c_float), ("partition_ms", C.c_float),
                ("halo_ms", C.c_float), ("total_ms", C.c_float), ("reserved", C.c_float * 3)]


_P = C.POINTER
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_fp, _ip = _P(C.c_float), _P(C.c_int)

# name -> (restype, argtypes); names are without prefix.  Keep in sync with include/claymore_amd.h.
SIGNATURES = {
    "default_config": (_i, [_i, _P(Config)]),
    "default_material": (_i, [_i, _i, _P(MaterialParams)]),
    "create": (_i, [_P(Config), _i, _P(_vp)]),
    "destroy": (None, [_vp]),
    "last_error": (C.c_char_p, [_vp]),
    "add_model": (_i, [_vp, _i, _P(MaterialParams), _vp, _sz, _fp, _ip]),
    "initial_setup": (_i, [_vp]),
    "grid_update": (_i, [_vp, _f, _fp]),
    "compute_dt": (_f, [_vp, _f, _f, _f, _f]),
    "g2p2g": (_i, [_vp, _f, _f]),
    "rebuild_partition": (_i, [_vp, _P(Counts)]),
    "substep": (_i, [_vp, _f, _f, _f, _f, _fp, _fp]),
    "run_fixed": (_i, [_vp, _i, _f]),
    "retrieve_positions": (_i, [_vp, _i, _vp, _P(_sz)]),
    "retrieve_state": (_i, [_vp, _i, _vp, _vp, _vp, _P(_sz)]),
    "state_kind": (_i, []),
    "get_counts": (_i, [_vp, _P(Counts)]),
    "get_timers": (_i, [_vp, _P(Timers)]),
    "grid_totals": (_i, [_vp, _P(C.c_double)]),
    "dump_grid": (_i, [_vp, _vp, _vp, _P(_sz)]),
    "check_table": (_i, [_vp]),
    "default_collision_object": (_i, [_P(CollisionObject)]),
    "set_collision_object": (_i, [_vp, _P(CollisionObject), _vp, _vp, _vp, _vp]),
    "test_eig": (_i, [_vp, _sz, _vp, _i]),
    "test_stress": (_i, [_i, _P(MaterialParams), _vp, _vp, _sz, _vp, _i]),
}
HALO = {
    "halo_keys": (_i, [_vp, _vp, _i, _ip]),
    "halo_tag_begin": (_i, [_vp]),
    "halo_tag_peer": (_i, [_vp, _i, _vp, _i]),
    "halo_tag_end": (_i, [_vp, _ip, _ip]),
    "g2p2g_halo": (_i, [_vp, _f, _f]),
    "g2p2g_interior": (_i, [_vp, _f, _f]),
    "halo_collect": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip]),
    "halo_reduce": (_i, [_vp, _i, _vp, _vp, _i]),
    "mgsp_begin": (_i, [_vp, _f, _f]),
    "mgsp_rebuild_export": (_i, [_vp, _vp, _i]),
    "mgsp_tag": (_i, [_vp, _vp, _i, _i, _i]),
    "mgsp_end": (_i, [_vp, _ip, _ip, _ip, _fp]),
}
SIGNATURES.update(HALO)
# entry points only the HIP library has (stream plumbing + kernel timing)
HIP_ONLY = {
    "build_info": (C.c_char_p, []),
    "last_g2p2g_ms": (_i, [_vp, _fp]),
    "still_launch_sizes": (_i, [C.c_char_p, _i, _i, _i, _ip, _ip]),
    "streams": (_i, [_vp, _P(_vp), _P(_vp)]),
    "sync": (_i, [_vp]),
    "get_capacity": (_i, [_vp, _P(C.c_int64), _P(C.c_int64), _ip]),
    "get_diagnostics": (_i, [_vp, _P(Diagnostics)]),
    "retrieve_velocity": (_i, [_vp, _i, _vp, _vp, _vp, _P(_sz)]),
    "particle_momentum": (_i, [_vp, _i, _P(C.c_double)]),
    "retrieve_stress": (_i, [_vp, _i, _vp, _vp, _vp, _P(_sz)]),
    "stress_totals": (_i, [_vp, _i, _P(C.c_double)]),
    "sample_grid": (_i, [_vp, _vp, _sz, _vp]),
    "grid_volume": (_i, [_vp, _P(C.c_int), _P(C.c_int), _i, _vp]),
    "grid_box_totals": (_i, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_double)]),
    "grid_isosurface": (_i, [_vp, _f, _P(C.c_int), _P(C.c_int), _vp, _vp, _P(_sz)]),
    "collider_loads": (_i, [_vp, _f, _P(LoadOptions), _P(C.c_double * 8)]),
    "collider_contacts": (_i, [_vp, _f, _vp, _vp, _P(_sz)]),
    "load_gauge": (_i, [_vp, _i, _P(LoadOptions)]),
    "load_gauge_read": (_i, [_vp, _P(C.c_double * 8), _P(C.c_double), _ip, _i]),
    "set_collider_body": (_i, [_vp, _i, _P(RigidBody)]),
    "get_collider_body": (_i, [_vp, _i, _P(RigidBody), _P(RigidBodyState)]),
    "set_collider_body_state": (_i, [_vp, _i, _P(C.c_double), _P(C.c_double), _P(C.c_double), _P(C.c_double)]),
    "shape_mass_properties": (_i, [_P(CollisionShape), _f, _P(RigidBody)]),
    "mesh_mass_properties": (_i, [_vp, _sz, _vp, _sz, _f, _P(RigidBody)]),
    "set_force_field": (_i, [_vp, _i, _P(ForceField)]),
    "get_force_field": (_i, [_vp, _i, _P(ForceField)]),
    "test_force_field": (_i, [_P(ForceField), _i, _f, _f, _vp, _vp, _sz, _vp, _i]),
    "halo_dump": (_i, [_vp, _vp, _vp, _ip, _vp]),
    "dump_block_rows": (_i, [_vp, _i, _vp, _P(_sz)]),
    "set_collision_clock": (_i, [_vp, _i, _f]),
    "get_collision_time": (_i, [_vp, _fp, _ip]),
    "set_collision_shape": (_i, [_vp, _i, _P(CollisionObject), _P(CollisionShape)]),
    "test_collision_shape": (_i, [_P(CollisionObject), _P(CollisionShape), _f, _f, _vp, _sz, _vp, _i]),
    "set_collision_heightfield": (_i, [_vp, _i, _P(CollisionObject), _P(Heightfield), _vp]),
    "test_collision_heightfield": (_i, [_P(CollisionObject), _P(Heightfield), _vp, _f, _vp, _sz, _vp, _i]),
    "set_collision_mesh": (_i, [_vp, _P(CollisionObject), _P(CollisionMesh), _vp, _sz, _vp, _sz]),
    "get_collision_field": (_i, [_vp, _P(C.c_int), _P(C.c_int), _vp]),
    "set_collision_volume": (_i, [_vp, _i, _P(CollisionObject), _P(CollisionVolume), _vp]),
    "set_collision_volume_mesh": (_i, [_vp, _i, _P(CollisionObject), _P(CollisionVolume), _vp, _sz, _vp, _sz]),
    "get_collision_volume": (_i, [_vp, _i, _P(CollisionVolume), _P(C.c_int), _P(C.c_int), _vp]),
    "test_collision_volume": (_i, [_P(CollisionObject), _P(CollisionVolume), _vp, _f, _vp, _sz, _vp, _i]),
    "sample_mesh": (_i, [_i, _vp, _sz, _vp, _sz, _P(MeshFill), _vp, _P(_sz), _i]),
    "add_model_mesh": (_i, [_vp, _i, _P(MaterialParams), _vp, _sz, _vp, _sz, _P(MeshFill), _fp, _ip, _P(_sz)]),
    "test_mesh_fill": (_i, [_i, _vp, _sz, _vp, _sz, _P(MeshFill), _P(C.c_double), _i]),
    "add_model_particles": (_i, [_vp, _i, _P(MaterialParams), _vp, _sz, _fp, _P(ParticleInit), _ip]),
    "set_model_velocity_field": (_i, [_vp, _i, _fp, _fp, _fp]),
    "emit_particles": (_i, [_vp, _i, _vp, _sz, _fp, _P(ParticleInit), _P(C.c_int32)]),
    "count_particles_in": (_i, [_vp, _i, _P(CollisionShape), _i, _P(C.c_int64)]),
    "remove_particles": (_i, [_vp, _i, _P(Removal), _P(RemovalResult)]),
    "checkpoint_size": (_i, [_vp, _P(_sz)]),
    "checkpoint_save": (_i, [_vp, _vp, _sz, _P(_sz)]),
    "checkpoint_load": (_i, [_vp, _vp, _sz]),
    "track_particle_ids": (_i, [_vp, _i]),
    "retrieve_ids": (_i, [_vp, _i, _vp, _vp, _P(_sz)]),
    "particle_ids_size": (_i, [_vp, _P(_sz)]),
    "particle_ids_save": (_i, [_vp, _vp, _sz, _P(_sz)]),
    "particle_ids_load": (_i, [_vp, _vp, _sz]),
    "group_unique_id": (_i, [_vp]),
    "group_create": (_i, [_vp, _i, _i, _vp, _P(_vp)]),
    "group_create_local": (_i, [_P(_vp), _i, _P(_vp)]),
    "group_destroy": (None, [_vp]),
    "group_last_error": (C.c_char_p, [_vp]),
    "group_transport": (C.c_char_p, [_vp]),
    "group_initial_setup": (_i, [_vp]),
    "group_resume": (_i, [_vp]),
    "group_substep": (_i, [_vp, _f, _f, _fp]),
    "group_run_fixed": (_i, [_vp, _i, _f]),
    "group_compute_dt": (_f, [_vp, _f, _f, _f, _f]),
    "group_main_loop": (_i, [_vp, _i, _i, _f, _vp, _vp, _ip]),
    "group_stats": (_i, [_vp, _ip, _ip, _fp]),
    "group_retrieve_velocity": (_i, [_vp, _i, _vp, _vp, _vp, _P(_sz)]),
    "group_particle_momentum": (_i, [_vp, _i, _P(C.c_double)]),
}


class Api:
    """Namespace of bound functions without their prefix (api.create, api.substep ...)."""

    def __init__(self, lib, prefix, names):
        self.lib, self.prefix = lib, prefix
        for name, (res, args) in names.items():
            fn = getattr(lib, prefix + name)  # AttributeError if the symbol is missing: fail loudly
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)


def bind(lib, prefix, hip=False):
    names = dict(SIGNATURES)
    if hip:
        names.update(HIP_ONLY)
    return Api(lib, prefix, names)


def repo_root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HIP_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libclaymore_hip.so")


def load_hip():
    """Load the HIP engine.  No fallback: a missing library is an error."""
    if not os.path.exists(HIP_LIB_PATH):
        raise RuntimeError(
            f"{HIP_LIB_PATH} not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback in the product path)")
    lib = C.CDLL(HIP_LIB_PATH, mode=C.RTLD_GLOBAL)
    return bind(lib, "mpm_", hip=True)
