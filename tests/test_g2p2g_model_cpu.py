"""tests/g2p2g_model.py - the float64 statement of one particle's G2P2G substep that tests/test_g2p2g_blocks_gpu.py holds the real kernels to -
judged without a GPU: against the oracle's particle body (mpmo_fn_particle_step, tied to the reference's statements by
tests/test_oracle_golden.py) on every generated scene, tier and material, and against the 960 golden rows themselves.  What the float32
reference side deviates from the model by is the yardstick Y of the GPU tests' bounds: measured here, held in g2p2g_model.Y and in
profiles/g2p2g_blocks_yardstick.txt (`python tests/test_g2p2g_model_cpu.py` prints the measured table in that file's format).  Also here: the
checkpoint patcher of tests/ckpt_format.py on a synthetic buffer built from the layout arithmetic."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ckpt_format as cf
import g2p2g_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_FILE = os.path.join(ROOT, "profiles", "g2p2g_blocks_yardstick.txt")
TIE = 1e-5              # cells: a new position this close to N + 0.5 may round to either node in float32 (ulp(64 cells) = 7.6e-6)
MAX_EXCLUDED = 0.01     # share of rows per material and tier that may be left out (unstable branch, non-finite on the torn tier)


def quantities(material):
    return ("pos", "stencil") + (("J",) if material == gm.J_FLUID else ("b",) + (("logjp",) if material != gm.FC else ()))


def deviations(material, m, o, keep):
    """The oracle's deviation from the model per quantity over the rows `keep` (stencils only where both use the same base and keep the particle)."""
    out = {"pos": float(gm.err_pos(o["pos"], m["pos"])[keep].max())}
    st = keep & (m["new_base"] == o["new_base"]).all(axis=1) & ~m["discarded"]
    out["stencil"] = float(gm.err_stencil(o["stencil"][st], m["stencil"][st]).max())
    if material == gm.J_FLUID:
        out["J"] = float(gm.err_J(o["J"], m["J"])[keep].max())
    else:
        out["b"] = float(gm.err_b(o["b6"], m["b6"])[keep].max())
        if material != gm.FC:
            out["logjp"] = float(np.abs(o["logjp"] - m["logjp"])[keep].max())
    return out


def integers_agree(m, o, keep):
    """base, discarded and new base equal - except where the model's new position sits within TIE of a tie value: there the two may differ by one
    node (and with it in the discard decision).  Returns the number of such rows."""
    assert np.array_equal(m["base"][keep], o["base"][keep])
    d = np.abs(m["new_base"] - o["new_base"])
    frac = np.abs(m["pos"] - np.floor(m["pos"]) - 0.5)
    differs = (d != 0).any(axis=1) & keep
    assert (d[keep] <= 1).all() and ((frac < TIE) | (d == 0))[keep].all(), "the new base differs away from a tie"
    same = keep & ~differs
    assert np.array_equal(m["discarded"][same], o["discarded"][same]) and np.array_equal(m["dirtag"][same], o["dirtag"][same])
    return int(differs.sum())


def measure_generated():
    """{(tier, material): {"Y": {quantity: value}, "excluded", "ties", "crossed", "discarded", "labels", "rows"}} over all scenes."""
    res = {}
    for material in gm.MATERIALS:
        data = {name: gm.scene_state(name, material) for name in gm.SCENES}
        for tier in gm.TIERS:
            acc = dict(Y={}, rows=0, excluded=0, nonfinite=0, ties=0, crossed=0, discarded=0, oracle_discarded=0, labels=np.zeros(4, np.int64), minsep=np.inf)
            for name, (pos, st) in data.items():
                m = gm.model_scene(material, pos, st, tier)
                of, oi = gm.oracle_scene(material, pos, st, tier)
                o = gm.oracle_view(material, of, oi)
                fin = m["finite"] & np.isfinite(of).all(axis=1)
                if tier != "torn":
                    assert fin.all(), (name, tier, material, "non-finite rows below the torn tier")
                keep = fin & ~m["unstable"]
                acc["ties"] += integers_agree(m, o, keep)
                for q, v in deviations(material, m, o, keep).items():
                    acc["Y"][q] = max(acc["Y"].get(q, 0.0), v)
                acc["rows"] += pos.shape[0]
                acc["excluded"] += int((~keep).sum())
                acc["nonfinite"] += int((~fin).sum())
                acc["crossed"] += int((o["dirtag"] != 13).sum())
                acc["discarded"] += int(m["discarded"][keep].sum())
                acc["oracle_discarded"] += int(o["discarded"][keep].sum())
                acc["labels"] += np.bincount(m["label"], minlength=4)
                acc["minsep"] = min(acc["minsep"], gm.min_separation(m["pos"][fin]))
            res[tier, material] = acc
    return res


def measure_golden():
    """{(tier, material): {"Y", ...}} with tier "golden" (arenas 0 .. 2, which abide by the CFL condition) and "golden_violent" (arenas 3, 4)."""
    P, arenas, rin, wf, wi = gm.golden_rows()
    res = {}
    for material in gm.MATERIALS:
        rows = np.flatnonzero(rin[:, 0] == material)
        m = gm.golden_model(material, P, arenas, rin[rows])
        o = gm.oracle_view(material, wf[rows], wi[rows], bits=int(P["bits"]))
        fin = m["finite"] & np.isfinite(wf[rows]).all(axis=1)
        for tier, sel in (("golden", rin[rows, 1] < 3), ("golden_violent", rin[rows, 1] >= 3)):
            keep = fin & ~m["unstable"] & sel
            plain = undeformed(material, rin[rows])
            res[tier, material] = dict(Y=deviations(material, m, o, keep), rows=int(sel.sum()), excluded=int((sel & ~keep).sum()), excluded_deformed=int((sel & ~keep & ~plain).sum()),
                                       nonfinite=int((sel & ~fin).sum()), ties=integers_agree(m, o, keep), deformed=int((sel & keep & ~plain).sum()))
    return res


def undeformed(material, rin):
    """The rows the existing one-particle test replays: F = I (J = 1) and the model's initial log Jp."""
    eye = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32) if material != gm.J_FLUID else np.array([1, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    return np.all(rin[:, 5:14] == eye, axis=1) & (rin[:, 14] == np.float32(-0.01 if material == gm.NACC else 0.0))


def table(res):
    """{(quantity, tier, material name): value} of a measurement"""
    return {(q, tier, gm.NAMES[material]): v for (tier, material), r in res.items() for q, v in r["Y"].items()}


def yardstick_lines(Y):
    return ["%-8s %-15s %-7s %.3g" % (q, tier, mat, v) for (q, tier, mat), v in sorted(Y.items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0]))]


@pytest.fixture(scope="module")
def generated():
    return measure_generated()


@pytest.fixture(scope="module")
def golden():
    return measure_golden()


def test_model_against_the_oracle_on_every_tier_and_material(generated):
    """Integer outputs equal (planted and chance ties counted), at most 1 % of the rows of a material and tier left out, final positions at least
    1e-3 cell apart, and the float deviations - the yardstick - what g2p2g_model.Y says they are."""
    for (tier, material), r in sorted(generated.items()):
        print(tier, gm.NAMES[material], "rows", r["rows"], "excluded", r["excluded"], "non-finite", r["nonfinite"], "ties", r["ties"], "crossed", r["crossed"],
              "discarded", r["discarded"], "min separation %.3g" % r["minsep"], {q: "%.3g" % v for q, v in r["Y"].items()})
        assert r["excluded"] <= MAX_EXCLUDED * r["rows"], (tier, material, r["excluded"], r["rows"])
        assert r["ties"] <= 0.005 * r["rows"]
        assert r["minsep"] >= 1e-3
        assert r["discarded"] == r["oracle_discarded"]
    check_constants(table(generated))


def test_model_against_the_golden_rows(golden):
    """The same on the 960 rows the reference's own statements produced (deformed ones included): the rows the GPU replay uses are arenas 0 .. 2."""
    for (tier, material), r in sorted(golden.items()):
        print(tier, gm.NAMES[material], "rows", r["rows"], "excluded", r["excluded"], "of them deformed", r["excluded_deformed"], "non-finite", r["nonfinite"], "ties", r["ties"], "deformed rows kept", r["deformed"], {q: "%.3g" % v for q, v in r["Y"].items()})
    assert sum(r["rows"] for r in golden.values()) == 960
    for material in gm.MATERIALS:
        r = golden["golden", material]
        # None of the deformed rows - the ones the GPU replay adds - is left out.  The undeformed sand rows (F = I, log Jp = 0) sit ON the tip condition
        # tr >= 0 of the return mapping, so the 1 +- 1e-5 rule flags a third of them; they stay with the existing one-particle test, which compares
        # them with the reference's statements directly.
        assert r["rows"] == 144 and r["deformed"] == 84 and r["excluded_deformed"] == 0 and r["nonfinite"] == 0, (material, r)
        assert r["excluded"] == 0 or material == gm.SAND, (material, r)
    check_constants(table(golden))


def check_constants(measured):
    for key, v in measured.items():
        assert key in gm.Y, ("g2p2g_model.Y lacks", key, "%.3g" % v)
        assert abs(v - gm.Y[key]) <= 0.006 * gm.Y[key], (key, "measured %.3g" % v, "constant %.3g" % gm.Y[key])      # equal to the three digits written


def test_the_yardstick_file_holds_the_constants():
    with open(YARDSTICK_FILE) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip() and not ln.startswith("#")]
    assert lines == yardstick_lines(gm.Y)


def test_the_generator_covers_what_it_claims(generated):
    """Every NACC case and every sand branch holds at least 1 % of the rows, at least 3 % of the rows change block on the flow tier, the torn tier
    discards, every block size is present, the planted particles sit on their tie values."""
    for material, nlab in ((gm.SAND, 3), (gm.NACC, 4)):
        for tier in gm.TIERS:
            print(gm.NAMES[material], tier, "rows by sand branch / NACC case", generated[tier, material]["labels"][:nlab].tolist())
        labels, total = sum(generated[tier, material]["labels"] for tier in gm.TIERS), sum(generated[tier, material]["rows"] for tier in gm.TIERS)
        assert (labels[:nlab] >= 0.01 * total).all(), (material, labels, total)
    for material in gm.MATERIALS:
        assert generated["flow", material]["crossed"] >= 0.03 * generated["flow", material]["rows"]
        assert generated["rest", material]["crossed"] <= 0.005 * generated["rest", material]["rows"]
        assert generated["torn", material]["discarded"] >= 5
        assert generated["fast", material]["discarded"] == 0 and generated["fast", material]["crossed"] >= 0.1 * generated["fast", material]["rows"]
    pos = gm.scene_block_sizes()
    _, counts = np.unique(gm.block_keys(pos), axis=0, return_counts=True)
    assert sorted(counts.tolist()) == sorted(gm.BLOCK_SIZES)
    one = gm.scene_one_cell()
    _, counts = np.unique(gm.stencil_base(one), axis=0, return_counts=True)
    assert sorted(counts.tolist()) == [256, 257, 513] and len(np.unique(gm.block_keys(one), axis=0)) == 2
    _, counts = np.unique(gm.block_keys(gm.scene_cluster()), axis=0, return_counts=True)
    assert len(counts) == 8 and counts.min() >= 185 and counts.max() <= 215
    iso = gm.scene_isolated()
    assert iso.shape[0] == 48 and len(np.unique(gm.block_keys(iso), axis=0)) == 48
    frac = iso.astype(np.float64) - np.floor(iso.astype(np.float64))
    assert ((frac == 0.5).any(axis=1)).sum() >= 6                                            # planted ties
    for material in (gm.FC, gm.SAND):
        st = gm.scene_state("block_sizes", material)[1]
        assert 0.03 < st["reflected"].mean() < 0.07
    # the field: order-free and the same in every grid block that holds a node
    k = np.array([[3, 4, 5]])
    assert np.array_equal(gm.grid_of(k, "flow")[0].reshape(3, 4, 4, 4), gm.cube_of(k[0], "flow")[:, :4, :4, :4])
    assert np.array_equal(gm.grid_of(k + 1, "flow")[0].reshape(3, 4, 4, 4), gm.cube_of(k[0], "flow")[:, 4:, 4:, 4:])


@pytest.mark.parametrize("material", gm.MATERIALS)
def test_the_slab_scene_keeps_the_reference_inside_the_gpu_bounds(material):
    """The slab of tests/test_g2p2g_split_gpu.py is not one of the yardstick's scenes (g2p2g_model.EXTRA_SCENES: Y stays what the others measure).
    What licenses it: on rest, flow and fast the oracle agrees with the model in every integer output with no row left out, the final positions
    are at least 1e-3 cell apart, and the oracle's own deviation from the model stays within the bound the GPU test applies, g2p2g_model.bound().
    The scene is long enough to be cut: particles change block on flow and fast, some across the plane between the x-keys 6 and 7."""
    assert "slab" not in gm.SCENES and "slab" in gm.EXTRA_SCENES
    pos, st = gm.scene_state("slab", material)
    keys, counts = np.unique(gm.block_keys(pos), axis=0, return_counts=True)
    assert sorted(map(tuple, keys.tolist())) == sorted(gm.SLAB) and counts.min() >= 185 and counts.max() <= 215
    for tier in ("rest", "flow", "fast"):
        m = gm.model_scene(material, pos, st, tier)
        of, oi = gm.oracle_scene(material, pos, st, tier)
        o = gm.oracle_view(material, of, oi)
        assert m["finite"].all() and np.isfinite(of).all() and not m["unstable"].any() and not m["discarded"].any(), (tier, "a row would have to be left out")
        keep = np.ones(pos.shape[0], bool)
        ties = integers_agree(m, o, keep)
        sep = gm.min_separation(m["pos"])
        moved = int((m["dirtag"] != 13).sum())
        cut = int(((gm.block_keys(pos)[:, 0] <= 6) != (gm.block_keys(m["pos"])[:, 0] <= 6)).sum())
        print(f"slab {gm.NAMES[material]} {tier}: {pos.shape[0]} rows, ties {ties}, changed block {moved}, across the cut {cut}, min separation {sep:.3g}")
        assert ties == 0 and sep >= 1e-3
        if tier != "rest":
            assert moved >= 0.03 * pos.shape[0] and cut >= 10
        for q, v in deviations(material, m, o, keep).items():
            bnd = gm.bound(q, tier, material)
            print(f"    {q}: measured {v:.3g} = {v / gm.Y[q, tier, gm.NAMES[material]]:.2f} Y, bound {bnd:.3g} ({v / bnd:.2f} of it)")
            assert v <= bnd, (tier, q, v, bnd)


def test_the_grid_gather_reads_what_the_field_wrote():
    """gather_grid() on blocks filled by grid_of() returns gather_field(): the velocities a model run is fed from a dumped grid."""
    pos = gm.scene_cluster()
    keys = np.unique(np.concatenate([gm.block_keys(pos) + np.array(d) for d in [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]]), axis=0)
    blocks = np.zeros((len(keys), 4, 64), np.float32)
    blocks[:, 1:4] = gm.grid_of(keys, "flow", seed=3)
    perm = np.random.default_rng(0).permutation(len(keys))
    assert np.array_equal(gm.gather_grid(pos, keys[perm], blocks[perm]), gm.gather_field(pos, "flow", seed=3))
    with pytest.raises(KeyError):
        gm.gather_grid(pos, keys[1:], blocks[1:])


def test_the_assembler_and_the_grid_comparison():
    """assemble() sums the kept particles' stencils per node; compare_grid() accepts that sum, rejects one node moved by more than its bound, a
    node nobody contributes to, and a missing node."""
    pos, st = gm.scene_state("cluster", gm.FC)
    m = gm.model_scene(gm.FC, pos, st, "fast")
    exp = gm.assemble([m], [1e-5])
    assert exp["n"].sum() == 27 * int((~m["discarded"]).sum()) and exp["n"].max() > 27
    assert abs(exp["sum"][:, 0].sum() - gm.constants(gm.FC, gm.material_overrides(gm.FC))["mass"] * pos.shape[0]) < 1e-12 * pos.shape[0]
    keys = gm.unpack_nodes(exp["key"]) // 4
    uk = np.unique(keys, axis=0)
    blocks = np.zeros((len(uk), 4, 64))
    index = {tuple(k): i for i, k in enumerate(uk.tolist())}
    nodes = gm.unpack_nodes(exp["key"])
    for node, v in zip(nodes.tolist(), exp["sum"]):
        blocks[index[tuple(c // 4 for c in node)], :, (node[0] & 3) * 16 + (node[1] & 3) * 4 + (node[2] & 3)] = v
    gk, gv = gm.grid_nodes(uk, blocks.astype(np.float32))
    assert np.array_equal(gk, exp["key"])
    ratio, bad, _ = gm.compare_grid(exp, gk, gv)
    assert bad == 0 and ratio < 1.0
    moved = gv.copy()
    moved[7, 2] += 1e-4 * np.abs(gv[:, 2]).max()
    assert gm.compare_grid(exp, gk, moved)[1] == 1
    heavy = int(np.argmax(gv[:, 0]))
    assert gm.compare_grid(exp, np.delete(gk, heavy), np.delete(gv, heavy, axis=0))[1] == 1
    extra_k = np.concatenate([[gm.pack_nodes(np.array([1, 1, 1]))], gk])
    assert gm.compare_grid(exp, extra_k, np.concatenate([[[1e-12, 0, 0, 0]], gv]))[1] == 1


# ---- the GPU file's comparison, with the oracle standing in for the engine ----------------------------------------------------------------
def oracle_as_engine(parts_states, tier, overrides=None):
    """What Bench.step() of tests/test_g2p2g_blocks_gpu.py returns, made from the oracle's particle body: the particles in another order, the grid
    summed in float32 and cut into 4^3 blocks, the books.  overrides: per model the parameters the oracle runs at (default: the scenes')."""
    import types

    import exact_models as em
    state, allk, allv, disc = [], [], [], 0
    for i, (material, pos, st) in enumerate(parts_states):
        of, oi = gm.oracle_scene(material, pos, st, tier, overrides=overrides[i] if overrides else None)
        o = gm.oracle_view(material, of, oi)
        perm = np.random.default_rng(5).permutation(pos.shape[0])
        d = dict(pos=(of[:, 12:15] * np.float32(2.0 ** gm.BITS))[perm], logjp=of[perm, 24], J=of[perm, 15], b6=np.zeros((pos.shape[0], 6), np.float32), reflected=np.zeros(pos.shape[0], bool))
        if material != gm.J_FLUID:
            d.update(b6=o["b6"].astype(np.float32)[perm], reflected=(np.linalg.det(em.to_mats(of[:, 15:24].astype(np.float64))) < 0)[perm])
        state.append(d)
        keep = ~o["discarded"]
        allk.append(gm.pack_nodes((o["new_base"][:, None, :] + gm.OFFS[None])[keep]).reshape(-1))
        allv.append(of[keep, 46:154].reshape(-1, 4))
        disc += int(o["discarded"].sum())
    k, v = np.concatenate(allk), np.concatenate(allv)
    uk, inv = np.unique(k, return_inverse=True)
    s = np.zeros((uk.size, 4), np.float32)
    for i in np.argsort(inv, kind="stable"):
        s[inv[i]] += v[i]                                      # float32 accumulation, one contribution at a time
    nodes = gm.unpack_nodes(uk)
    ub, binv = np.unique(nodes // 4, axis=0, return_inverse=True)
    blocks = np.zeros((len(ub), 4, 64), np.float32)
    blocks[binv.reshape(-1), :, (nodes[:, 0] & 3) * 16 + (nodes[:, 1] & 3) * 4 + (nodes[:, 2] & 3)] = s
    cnt = types.SimpleNamespace(particles=[p.shape[0] for _, p, _ in parts_states],
                                particle_blocks=len(np.unique(np.concatenate([gm.block_keys(d["pos"]) for d in state]), axis=0)))
    return dict(counts=cnt, lost=0, discarded=disc, grid=(ub, blocks), state=state)


@pytest.mark.parametrize("material", gm.MATERIALS)
def test_the_gpu_comparison_accepts_the_oracle_and_rejects_small_faults(material):
    """check() of tests/test_g2p2g_blocks_gpu.py, run here on what the oracle computes for the cluster (fast tier) and the torn scene: the float32
    reference passes every bound (they are max(existing, 3 Y): it must), and the same result with one small fault planted does not - the state of
    two particles swapped, one particle's mass taken off one node, a particle counted as discarded, a node that nobody contributed to."""
    import types

    import test_g2p2g_blocks_gpu as T
    for scene, tier in (("cluster", "fast"), ("torn", "torn")):
        pos, st = gm.scene_state(scene, material)
        bench = types.SimpleNamespace(parts=[(material, pos)], bits=gm.BITS)
        models = [gm.model_scene(material, pos, st, tier)]
        res = oracle_as_engine([(material, pos, st)], tier)
        T.check(bench, res, models, tier, scene)

        def faulty(change):
            bad = dict(res, state=[{k: v.copy() for k, v in res["state"][0].items()}], grid=(res["grid"][0].copy(), res["grid"][1].copy()))
            change(bad)
            with pytest.raises(AssertionError):
                T.check(bench, bad, models, tier, scene + ", faulty")
        key = "J" if material == gm.J_FLUID else "b6"

        def swap(bad):
            x = bad["state"][0][key]
            i = int(np.argmax(np.abs(x.reshape(x.shape[0], -1) - x.reshape(x.shape[0], -1)[0]).max(axis=1)))      # the particle least like particle 0
            x[[0, i]] = x[[i, 0]]
        faulty(swap)

        def lighter(bad):
            g = bad["grid"][1]
            b, c = np.unravel_index(np.argmax(g[:, 0]), g[:, 0].shape)
            g[b, 0, c] -= np.float32(0.3 * gm.constants(material, gm.material_overrides(material))["mass"] * 0.4)     # a third of one particle's largest weight
        faulty(lighter)
        faulty(lambda bad: bad.update(discarded=bad["discarded"] + 1))

        def stray(bad):
            g = bad["grid"][1]
            b, c = np.argwhere(g[:, 0] == 0)[0]
            g[b, 1, c] = np.float32(1e-12)
        faulty(stray)


# ---- tests/ckpt_format.py: the particle-state patcher on a synthetic checkpoint ----------------------------------------------------------
def synthetic_checkpoint(nch, sizes, rng, max_ppc=16, permute=True):
    """A checkpoint of one model built from the layout arithmetic alone: particle blocks on a diagonal, each with its bins in a shuffled order of
    the previous numbering, every slot filled with distinct positions and a recognisable state; one record per particle (direction tag 13)."""
    pbc = len(sizes)
    keys = np.array([[2 + b, 3 + b, 4 + b] for b in range(pbc)] + [[12, 12, 12]], np.int32)           # one more exterior block
    ebc = nbc = len(keys)
    order = rng.permutation(pbc) if permute else np.arange(pbc)       # previous numbering: block order[i] of the current one
    prev_keys = keys[order]
    nbins = (np.asarray(sizes) + 63) // 64
    binoff_prev = np.concatenate([[0], np.cumsum(nbins[order])]).astype(np.int32)
    bincount = int(binoff_prev[-1])
    ppb = 64 * max_ppc
    pid_bits = ppb.bit_length() - 1
    model = dict(material=1, nch=nch, list_in=0, layout=0, n=int(np.sum(sizes)), bincount=bincount, bincount_src=bincount, bucketed=int(np.sum(sizes)))
    h = dict(domain_bits=6, max_ppc=max_ppc, nmodels=1, rollid=0, pbc=pbc, nbc=nbc, ebc=ebc, prev_count=pbc, prev_pbc=pbc, models=[model])
    sections, end = cf.layout(h)
    buf = rng.integers(0, 256, end, dtype=np.uint8)                    # padding and unused slots hold noise: the patcher must leave it alone
    head = np.zeros(cf.HEADER_BYTES, np.uint8)
    head[:8].view(np.uint64)[0] = cf.MAGIC
    head[8:40].view(np.int32)[:] = [6, max_ppc, 1, 0, pbc, nbc, ebc, pbc]
    head[40:48].view(np.uint64)[0] = end
    head[56:60].view(np.int32)[0] = pbc
    head[60:64].view(np.int32)[0] = 0
    head[64:80].view(np.int32)[:] = [1, nch, 0, 0]
    head[80:112].view(np.int64)[:] = [model["n"], bincount, bincount, model["bucketed"]]
    buf[:cf.HEADER_BYTES] = head

    def put(name, arr):
        at, n = sections[name]
        buf[at:at + n] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    put("cur_keys", keys)
    put("prev_keys", prev_keys)
    put(("size", 0), np.concatenate([sizes, [0, 0]]).astype(np.int32))
    put(("row_of", 0), np.arange(ebc + 1, dtype=np.int32))
    put(("binoff_src", 0), binoff_prev)
    binoff_cur = np.zeros(ebc + 1, np.int32)
    binoff_cur[:pbc + 1] = np.concatenate([[0], np.cumsum(nbins)])
    put(("binoff_dst", 0), binoff_cur)
    recs = np.concatenate([(13 << (pid_bits + cf.K_KEY_BITS)) | (rng.integers(0, 216, s) << pid_bits) | rng.permutation(s) for s in sizes]).astype(np.int32)
    put(("lists", 0), recs)
    B = cf.bins(buf, 0)
    rec = cf.rec_floats(nch)
    n_slots = bincount * 64
    B[:] = rng.uniform(1.0, 2.0, B.shape).astype(np.float32)
    pos = (np.arange(n_slots * 3, dtype=np.float32).reshape(n_slots, 3) * np.float32(0.25) + np.float32(8.0))      # all distinct
    for c in range(3):
        B[:, c:64 * rec:rec] = pos[:, c].reshape(bincount, 64)
    return buf


@pytest.mark.parametrize("nch", [4, 9, 10])
def test_particle_state_patcher_on_a_synthetic_checkpoint(nch):
    """Round trip, and "only the requested slots changed": every byte outside the state floats of the requested particles is as it was - positions,
    the state of the other particles, padding slots, lists and every other section."""
    rng = np.random.default_rng(nch)
    sizes = np.array([1, 64, 65, 130, 3])
    buf = synthetic_checkpoint(nch, sizes, rng)
    h = cf.parse(buf)
    assert cf.bins(buf, 0).shape == (h["models"][0]["bincount_src"], nch * 64)
    before = cf.particle_state(buf, 0)
    n = before["xyz_cells"].shape[0]
    assert n == sizes.sum() and len({tuple(p) for p in before["xyz_cells"].tolist()}) == n
    pick = rng.permutation(n)[:101]
    xyz = before["xyz_cells"][pick]
    if nch == 4:
        new = dict(J=rng.uniform(0.8, 1.1, pick.size).astype(np.float32))
    else:
        new = dict(b=rng.uniform(0.5, 1.5, (pick.size, 6)).astype(np.float32), reflected=rng.random(pick.size) < 0.3)
        if nch == 10:
            new["logjp"] = rng.uniform(-0.03, 0.01, pick.size).astype(np.float32)
    out = cf.with_particle_state(buf, 0, xyz, **new)
    after = cf.particle_state(out, 0)
    assert np.array_equal(after["xyz_cells"].view(np.uint32), before["xyz_cells"].view(np.uint32))
    rest = np.setdiff1d(np.arange(n), pick)
    for k in ("b", "logjp", "J", "reflected"):
        if before[k] is None:
            assert after[k] is None
            continue
        want = before[k].copy()
        if k in new:
            want[pick] = new[k]
        assert np.array_equal(after[k], want) and np.array_equal(after[k][rest], before[k][rest]), k
    # byte for byte: the changed bytes are exactly the state floats of the requested particles
    changed = np.flatnonzero(out != buf)
    at, _ = h["sections"]["bins", 0]
    bin_, slot = cf.particle_slots(buf, 0)
    rec, row = cf.rec_floats(nch), nch - cf.rec_floats(nch)
    allowed = set()
    for i in pick:
        base = at + 4 * (int(bin_[i]) * nch * 64)
        floats = [int(slot[i]) * rec + c for c in range(3, rec)] + [64 * rec + int(slot[i]) * row + c for c in range(row)]
        allowed.update(base + 4 * f + k for f in floats for k in range(4))
    assert set(changed.tolist()) <= allowed and len(changed) > 0
    # nothing requested, nothing changed; a position that is not there, or there twice, is refused
    assert np.array_equal(cf.with_particle_state(buf, 0, xyz[:0]), buf)
    with pytest.raises(AssertionError):
        cf.with_particle_state(buf, 0, xyz[:1] + np.float32(0.125), **{k: v[:1] for k, v in new.items()})
    with pytest.raises(AssertionError):
        cf.with_particle_state(buf, 0, np.concatenate([xyz[:1], xyz[:1]]), **{k: np.concatenate([v[:1], v[:1]]) for k, v in new.items()})
    # leaving an argument out leaves those floats alone
    if nch == 10:
        only = cf.particle_state(cf.with_particle_state(buf, 0, xyz, logjp=new["logjp"]), 0)
        assert np.array_equal(only["b"], before["b"]) and np.array_equal(only["reflected"], before["reflected"]) and np.array_equal(only["logjp"][pick], new["logjp"])


if __name__ == "__main__":
    Ym = table(measure_generated())
    Ym.update(table(measure_golden()))
    print("\n".join(yardstick_lines(Ym)))
