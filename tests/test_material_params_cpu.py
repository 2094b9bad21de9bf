"""tests/material_variants.py - the parameter axis of tests/test_material_params_gpu.py - judged without a GPU, the oracle standing in for the
device:
  * the licence of the block-level bounds: at every variant, scene and tier the GPU tests use, the oracle agrees with the block model
    (tests/g2p2g_model.py at the variant's parameters) in every integer output with no row left out, the final positions are at least 1e-3 cell
    apart, and the oracle's own deviation from the model stays within g2p2g_model.bound() - or, where it does not, is what
    material_variants.BLOCK_YARDSTICK says it is (the bound there is max(gm.bound, 3 x that));
  * the yardstick tables and profiles/material_params_yardstick.txt hold what is measured here (`python tests/test_material_params_cpu.py`
    prints the file's lines);
  * the function-level comparison keeps its rows (at most 1 % left out, 20 per branch / case) and accepts the oracle at every variant;
  * both comparisons SEE the parameters: the oracle run at the default parameters is rejected when judged against the model of S1, S2, S3 / N1."""
import os
import sys
import types

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import g2p2g_model as gm
import material_variants as mv
from test_g2p2g_model_cpu import deviations, integers_agree, oracle_as_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_FILE = os.path.join(ROOT, "profiles", "material_params_yardstick.txt")
_BLOCK = {}


def measure_block(vid, scene, tier):
    """The oracle against the block model at variant `vid` on one scene and tier: what the licence needs"""
    if (vid, scene, tier) not in _BLOCK:
        material, over = mv.block_overrides(vid)
        pos, st = gm.scene_state(scene, material, overrides=over)
        m = gm.model_scene(material, pos, st, tier, overrides=over)
        of, oi = gm.oracle_scene(material, pos, st, tier, overrides=over)
        o = gm.oracle_view(material, of, oi)
        left_out = int((~(m["finite"] & np.isfinite(of).all(axis=1)) | m["unstable"]).sum())
        keep = np.ones(pos.shape[0], bool)
        _BLOCK[vid, scene, tier] = dict(material=material, rows=pos.shape[0], left_out=left_out, ties=integers_agree(m, o, keep) if not left_out else -1,
                                        discarded=int(m["discarded"].sum()), minsep=gm.min_separation(m["pos"]), dev=deviations(material, m, o, keep),
                                        labels=np.bincount(m["label"], minlength=4).tolist())
    return _BLOCK[vid, scene, tier]


def block_cases():
    return [(vid, scene, tier) for vid, _, _ in mv.BLOCK_VARIANTS for scene, tier in mv.BLOCK_CASES] + [mv.MIXED]


def measured_block_yardstick():
    """{(variant, scene, tier, quantity): the oracle's deviation} where it exceeds gm.bound"""
    out = {}
    for vid, scene, tier in block_cases():
        r = measure_block(vid, scene, tier)
        for q, v in r["dev"].items():
            if not v <= gm.bound(q, tier, r["material"]):
                out[vid, scene, tier, q] = v
    return out


def oracle_function_level(vid, material, delta, ref_delta=None, tag=""):
    """compare_function_level with the oracle's rows at `delta` in the device's place (ref_delta: the parameters of the yardstick run, default the same)"""
    from oracle_ffi import oracle_api
    api = oracle_api()
    F, lj = mv.inputs(material)
    p = mv.params(api, material, delta if ref_delta is None else ref_delta)
    ref = mv.stress_rows(api, material, p, F, lj)
    got = ref if ref_delta is None else mv.stress_rows(api, material, mv.params(api, material, delta), F, lj)
    with np.errstate(all="ignore"):
        return mv.compare_function_level(vid, material, p, F, lj, mv.bform(got[:, 0:9]), got[:, 9:18].astype(np.float64), got[:, 18], ref, tag, absolute=False)


def measured_e1_yardstick():
    out = {}
    for vid, material, delta in mv.FUNCTION_VARIANTS:
        if vid == "E1":
            _, figs = oracle_function_level(vid, material, delta)
            out[gm.NAMES[material], "stress"] = figs["e_ref"]
            if "f_ref" in figs:
                out[gm.NAMES[material], "b"] = figs["f_ref"]
    return out


def same_to_three_digits(measured, constants, what):
    assert set(measured) == set(constants), (what, "measured", sorted(measured), "constants", sorted(constants))
    for key, v in measured.items():
        assert abs(v - constants[key]) <= 0.006 * constants[key], (what, key, "measured %.3g" % v, "constant %.3g" % constants[key])


@pytest.mark.parametrize("vid", [v[0] for v in mv.BLOCK_VARIANTS])
def test_the_oracle_stays_inside_the_block_level_bounds_at_every_variant(vid):
    """The licence of tests/test_material_params_gpu.py's block-level bounds, modelled on test_the_slab_scene_keeps_the_reference_inside_the_gpu_bounds:
    per scene and tier no row is left out, the integer outputs agree, the minimum separation is at least 1e-3 cell, nothing is discarded, and the
    oracle's deviation from the model is at most block_bound() - which is gm.bound unless BLOCK_YARDSTICK holds the oracle's own figure."""
    for v, scene, tier in block_cases():
        if v != vid:
            continue
        r = measure_block(vid, scene, tier)
        print(f"{vid} {scene} {tier}: {r['rows']} rows, left out {r['left_out']}, ties {r['ties']}, discarded {r['discarded']}, min separation {r['minsep']:.3g}, rows by branch / case {r['labels']}")
        assert r["left_out"] == 0 and r["ties"] == 0 and r["discarded"] == 0 and r["minsep"] >= 1e-3
        for q, dev in r["dev"].items():
            plain, bnd = gm.bound(q, tier, r["material"]), mv.block_bound(vid, scene, tier, q, r["material"])
            print(f"    {q}: oracle {dev:.3g} = {dev / plain:.2f} of gm.bound {plain:.3g}; bound used {bnd:.3g}")
            assert dev <= bnd, (vid, scene, tier, q, dev, bnd)
            assert (dev > plain) == ((vid, scene, tier, q) in mv.BLOCK_YARDSTICK), "BLOCK_YARDSTICK holds exactly the cases where the oracle leaves gm.bound"


def test_the_yardstick_tables_and_file_hold_what_is_measured():
    same_to_three_digits(measured_block_yardstick(), mv.BLOCK_YARDSTICK, "BLOCK_YARDSTICK")
    same_to_three_digits(measured_e1_yardstick(), mv.E1_YARDSTICK, "E1_YARDSTICK")
    with open(YARDSTICK_FILE) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip() and not ln.startswith("#")]
    assert lines == mv.yardstick_lines()


@pytest.mark.parametrize("vid,material,delta", mv.FUNCTION_VARIANTS, ids=[mv.vname(v, m) for v, m, _ in mv.FUNCTION_VARIANTS])
def test_the_function_level_comparison_keeps_its_rows_and_accepts_the_oracle(vid, material, delta):
    """At most 1 % of the class <= 5 rows left out, at least 20 rows per sand branch / NACC case - and the oracle, its own yardstick, passes."""
    fails, _ = oracle_function_level(vid, material, delta)
    assert not fails, fails


@pytest.mark.parametrize("vid", ["S1", "S2", "S3", "N1"])
def test_the_function_level_comparison_sees_the_parameters(vid):
    """The oracle run at the DEFAULT parameters - an engine that ignores the variant's - fails the comparison at the variant, by the rules that
    are relative to the yardstick alone (the absolute ones, which the oracle's SVD misses at any parameters, are left out of this judgement)."""
    material, delta = mv.BY_ID[vid]
    fails, _ = oracle_function_level(vid, material, {}, ref_delta=delta, tag="ignored: ")
    print(fails)
    assert fails and not any(f[0] in ("rows left out", "a branch / case holds fewer than 20 rows") for f in fails)


def block_check(vid, scene, tier, engine_overrides):
    """check() of the block-level GPU tests on what the oracle computes at `engine_overrides`, judged against the model of variant `vid`"""
    import test_material_params_gpu as T
    material, over = mv.block_overrides(vid)
    pos, st = gm.scene_state(scene, material, overrides=over)
    bench = types.SimpleNamespace(parts=[(material, pos)], bits=gm.BITS)
    models = [gm.model_scene(material, pos, st, tier, overrides=over)]
    res = oracle_as_engine([(material, pos, st)], tier, overrides=[engine_overrides])
    T.check_variant(bench, res, models, tier, [(vid, scene)], f"{vid} {scene}")


@pytest.mark.parametrize("vid", ["S1", "S2", "S3", "N1"])
def test_the_block_level_comparison_accepts_the_oracle_and_sees_the_parameters(vid):
    """check() accepts the oracle at the variant and rejects the oracle run at the default parameters: it can see a parameter the kernel ignores."""
    material, over = mv.block_overrides(vid)
    block_check(vid, "cluster", "flow", over)
    with pytest.raises(AssertionError):
        block_check(vid, "cluster", "flow", gm.material_overrides(material))


if __name__ == "__main__":
    print("\n".join(mv.yardstick_lines(measured_e1_yardstick(), measured_block_yardstick())))
    for case in block_cases():
        r = measure_block(*case)
        print("#", *case, "left out", r["left_out"], "ties", r["ties"], "minsep %.3g" % r["minsep"], {q: "%.2f" % (v / gm.bound(q, case[2], r["material"])) for q, v in r["dev"].items()})
