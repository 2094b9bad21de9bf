"""The launch-size rule of the rebuild's three look-and-leave kernels (claymore_hip.hip: still_launch_rule, exported as mpm_still_launch_sizes): a pure
function of the still streak at the last read-back, whether the still path is on, the particle block count and the MPM_STILL_LAUNCH setting.  It
returns the workgroups of the rebuild's own prepare launch (T) and of its two registration launches (R); 0 stands for the full size.  CPU only:
the function needs no device.  (R: the registrations measured no faster at any size - profiles/substep_fixed_cost.txt - and keep their full size under
`auto`; only thin:N sets it.)

What the table must say:
  * auto (the default, also for an unset or unknown setting): thin from a streak of two on, and only with the still path on; full again at streak 0;
  * T >= ceil(particle blocks / 64) at every size - a wave of the streak path looks at 64 blocks, so the path stays one trip -, and T is the same fixed
    number for every scene small enough; R stays the full size;
  * full: never thin; thin:N: always N for all three, whatever the streak (tests and A/B)."""
import ctypes as C

import pytest

from claymore_amd import _ffi


def sizes(setting, streak, still_on, pbc):
    hip = _ffi.load_hip()
    t, r = C.c_int(-1), C.c_int(-1)
    assert hip.still_launch_sizes(None if setting is None else setting.encode(), streak, still_on, pbc, C.byref(t), C.byref(r)) == 0
    return t.value, r.value


FULL = (0, 0)
C3_PBC = 83_800          # the sand column of bench.py, about


@pytest.mark.parametrize("setting", [None, "auto", "", "thin:", "thin:0", "thin:-4", "thin:12x", "THIN:4", "something"])
def test_auto_follows_the_streak(setting):
    for pbc in (0, 1, 64, 65, 1000, C3_PBC):
        assert sizes(setting, 0, 1, pbc) == FULL
        assert sizes(setting, 1, 1, pbc) == FULL        # (the first still rebuild of a streak writes every row: prepare's skip loop starts with the second)
        thin = sizes(setting, 2, 1, pbc)
        assert thin[0] > 0 and thin[1] == 0
        assert sizes(setting, 3, 1, pbc) == sizes(setting, 10 ** 6, 1, pbc) == thin
        assert sizes(setting, 5, 0, pbc) == FULL        # still path off (mpm_config.still_rebuild = -1, a grouped context): nothing to follow
    t0, r0 = sizes(setting, 2, 1, 1)
    assert sizes(setting, 2, 1, C3_PBC) == (t0, r0), "one fixed size for every scene up to the flagship's"
    assert r0 == 0 and t0 >= 6144, "the full path under a thin launch still fills the chip's 6 144 prepare wave slots"


@pytest.mark.parametrize("pbc", [1, 63, 64, 65, 4095, 4096, 4097, C3_PBC, 64 * 8192 - 1, 64 * 8192, 64 * 8192 + 1, 3_000_000, 16_777_216])
def test_the_streak_path_stays_one_trip(pbc):
    t, r = sizes("auto", 2, 1, pbc)
    assert t >= -(-pbc // 64), (pbc, t)
    assert r == 0
    # ... and the launch grows no faster than it must: beyond the fixed size, at most one workgroup per 64 blocks of the launch's own margin (1/16 + 64 blocks)
    assert t == sizes("auto", 2, 1, 1)[0] or t <= -(-(pbc + pbc // 16 + 64) // 64)


def test_back_to_full_at_streak_zero():
    seq = [sizes("auto", s, 1, C3_PBC) for s in (0, 1, 2, 3, 0, 1, 2)]
    assert seq[0] == seq[1] == seq[4] == seq[5] == FULL and seq[2] == seq[3] == seq[6] != FULL


def test_full_and_thin_overrides():
    for streak in (0, 1, 2, 50):
        for on in (0, 1):
            assert sizes("full", streak, on, C3_PBC) == FULL
            for n in (1, 2, 3, 4096, 16384):
                assert sizes(f"thin:{n}", streak, on, C3_PBC) == (n, n)


def test_null_outputs_are_refused():
    hip = _ffi.load_hip()
    t = C.c_int()
    assert hip.still_launch_sizes(b"auto", 2, 1, 100, None, C.byref(t)) == _ffi.MPM_ERR_INVALID
    assert hip.still_launch_sizes(b"auto", 2, 1, 100, C.byref(t), None) == _ffi.MPM_ERR_INVALID
