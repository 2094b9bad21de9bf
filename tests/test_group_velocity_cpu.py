"""Velocity output of a multi-GPU group, the parts that need no GPU: the library exports mpm_group_retrieve_velocity,
mpm_group_particle_momentum and mpm_particle_momentum, the header declares them, the Python layer binds them, and the group entry points
refuse a NULL group with MPM_ERR_INVALID before touching a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from claymore_amd import _ffi
from claymore_amd.engine import Engine
from claymore_amd.mgsp import MgspGroupRank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "mpm_group_retrieve_velocity": r"int mpm_group_retrieve_velocity\(mpm_group\* g, int model, float\* xyz, float\* vel, float\* affine9, size_t\* n\);",
    "mpm_group_particle_momentum": r"int mpm_group_particle_momentum\(mpm_group\* g, int model, double out\[5\]\);",
    "mpm_particle_momentum": r"int mpm_particle_momentum\(mpm_ctx\* ctx, int model, double out\[5\]\);",
}


def test_library_exports_the_group_readout_and_header_declares_it():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    for sym, decl in DECLS.items():
        assert re.search(rf"\bT {sym}$", out, re.M), f"{sym} is not exported"
        assert re.search(decl, hdr), f"{sym} is not declared"
    api = _ffi.load_hip()
    for name, nargs in (("group_retrieve_velocity", 6), ("group_particle_momentum", 3), ("particle_momentum", 3)):
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES           # (the oracle has no velocity readout)
        fn = getattr(api, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert callable(Engine.particle_momentum)
    assert callable(MgspGroupRank.retrieve_velocity) and callable(MgspGroupRank.particle_momentum)


def test_null_group_is_refused_without_a_gpu():
    api = _ffi.load_hip()
    xyz = np.zeros((4, 3), dtype=np.float32)
    n = C.c_size_t(4)
    out = (C.c_double * 5)()
    p = xyz.ctypes.data_as(C.c_void_p)
    assert api.group_retrieve_velocity(None, 0, p, p, None, C.byref(n)) == _ffi.MPM_ERR_INVALID
    assert api.group_particle_momentum(None, -1, out) == _ffi.MPM_ERR_INVALID
    assert api.particle_momentum(None, -1, out) == _ffi.MPM_ERR_NOT_READY
