"""All eight model slots, without a GPU: the generators of tests/model_slot_scenes.py keep what they promise; the comparison of
tests/test_g2p2g_blocks_gpu.py (check) accepts the oracle's result on eight models (the oracle's particle body run model by model, summed on one grid) - empty models in slots 0, 3
and 7 included: the oracle takes them as they are, no slot is left out - inside g2p2g_model.bound, and rejects four faults planted in slots 4 .. 7 only; the checkpoint
tools of tests/ckpt_format.py read and patch a synthetic eight-model checkpoint with mixed list layouts and an empty model."""
import types

import numpy as np
import pytest

import ckpt_format as cf
import g2p2g_model as gm
import model_slot_scenes as ms
import rebuild_scenes as rs
import test_g2p2g_blocks_gpu as T
from test_g2p2g_model_cpu import oracle_as_engine


# ---- 1. the generators ------------------------------------------------------------------------------------------------------------------------------
def test_the_block_census_of_the_scenes():
    eight = ms.scene("eight", "rest")
    assert [m for m, _ in eight["parts"]] == ms.MATERIALS == [gm.FC, gm.SAND, gm.NACC, gm.J_FLUID, gm.J_FLUID, gm.NACC, gm.SAND, gm.FC]
    assert sorted(ms.MATERIALS[:4]) == sorted(ms.MATERIALS[4:]) == sorted(gm.MATERIALS)      # every kernel once in the low and once in the high slots
    n = [p.shape[0] for _, p in eight["parts"]]
    print("eight: particles by slot", n)
    assert all(100 <= k <= 500 for k in n) and len(set(n)) == 8
    cen = ms.census(eight)
    shared = [k for k, v in cen.items() if sum(c > 0 for c in v) >= 3]
    assert len(shared) >= 8 and sorted(shared) == sorted(gm.CLUSTER)
    assert all(min(cen[k]) > 0 for k in gm.CLUSTER)                                            # all eight models in each of them
    for slot in range(ms.NSLOTS):                                                              # a private block each, on its own site
        assert ms.PRIVATE[slot] in gm.SITES and len(set(ms.PRIVATE)) == ms.NSLOTS
        want = [0] * ms.NSLOTS
        want[slot] = ms.PRIVATE_SIZE[slot]
        assert cen[ms.PRIVATE[slot]] == want, (slot, cen[ms.PRIVATE[slot]])
    assert len(cen) == 16
    assert sum(1 for v in cen.values() if v[0] == 0) >= 3                                      # slot 0 absent from occupied blocks
    # the private blocks' node cubes (nodes 4 k .. 4 k + 7 per axis) are clear of each other's and of the cluster's
    cubes = [np.array(k) for k in ms.PRIVATE] + [np.array(k) for k in gm.CLUSTER]
    for i, a in enumerate(cubes[:ms.NSLOTS]):
        assert all((np.abs(a - b) >= 2).any() for j, b in enumerate(cubes) if j != i)
    holes, last = ms.scene("holes", "rest"), ms.scene("last_only", "rest")
    for slot in range(ms.NSLOTS):
        same = lambda sc: np.array_equal(sc["parts"][slot][1].view(np.uint32), eight["parts"][slot][1].view(np.uint32))
        assert (holes["parts"][slot][1].shape == (0, 3)) if slot in (0, 3, 7) else same(holes)
        assert same(last) if slot == 7 else last["parts"][slot][1].shape == (0, 3)
        assert holes["parts"][slot][0] == last["parts"][slot][0] == ms.MATERIALS[slot]
    assert ms.occupied("holes") == (1, 2, 4, 5, 6) and ms.occupied("last_only") == (7,)
    # the tiers share positions and states
    flow = ms.scene("eight", "flow")
    for (_, a), (_, b), sa, sb in zip(eight["parts"], flow["parts"], eight["states"], flow["states"]):
        assert np.array_equal(a, b) and all(np.array_equal(sa[k], sb[k]) for k in sa if sa[k] is not None)


@pytest.mark.parametrize("tier", ms.TIERS)
def test_no_row_on_a_brink_and_few_on_a_sort_key_tie(tier):
    """Per model, not pooled: no `unstable` row in g2p2g_model.step's result, every row finite and kept, at most rebuild_scenes.TIE_CAP of the
    model's particles with a predicted sort key that hangs on a rounding tie; final positions far enough apart for nearest-neighbour matching."""
    sc = ms.scene("eight", tier)
    crossed = 0
    for slot, ((mat, pos), m) in enumerate(zip(sc["parts"], ms.models(sc))):
        ties = int((~rs.decided(m, tier, mat)).sum())
        print(f"eight {tier} slot {slot} {gm.NAMES[mat]}: {pos.shape[0]} particles, {ties} on a tie, {int((m['dirtag'] != 13).sum())} change block")
        assert not m["unstable"].any() and m["finite"].all() and not m["discarded"].any()
        assert ties <= rs.TIE_CAP * pos.shape[0], (slot, ties)
        assert gm.min_separation(m["pos"]) >= 1e-3
        crossed += int((m["dirtag"] != 13).sum())
    if tier == "flow":
        assert crossed >= 0.03 * sum(p.shape[0] for _, p in sc["parts"])
    empty = ms.models(ms.scene("holes", tier))[0]
    assert empty["pos"].shape == (0, 3) and empty["stencil"].shape == (0, 27, 4) and empty["unstable"].shape == (0,)


def test_the_pipeline_forms():
    for name in ("eight", "holes"):
        sc = ms.pipeline(name)
        n = [m["xyz"].shape[0] for m in sc["models"]]
        print(name, "pipeline form: particles by slot", n, "total", sum(n))
        assert [m["material"] for m in sc["models"]] == ms.MATERIALS and sc["bits"] == ms.BITS
        assert sum(n) <= 5000 and [k > 0 for k in n] == [s in ms.occupied(name) for s in range(ms.NSLOTS)]
        for a in range(0, ms.NSLOTS, 2):                                                         # pairs: thrown at each other, apart from the other pairs
            va, vb = sc["models"][a]["v0"], sc["models"][a + 1]["v0"]
            assert va[0] > 0 > vb[0] and va[1:] == vb[1:] == (0.0, 0.0)
        xyz = np.concatenate([m["xyz"] for m in sc["models"]]).astype(np.float64) * 2.0 ** ms.BITS
        assert xyz.min() >= 10 and xyz.max() <= 54                                               # clear of the wall zone
        assert len(np.unique(xyz, axis=0)) == xyz.shape[0]
    sc = ms.pipeline("eight")
    for first, second in ((0, 7), (1, 6)):                                                       # the second FC and the second SAND: other parameters
        pa, pb = sc["models"][first]["params"], sc["models"][second]["params"]
        assert sc["models"][first]["material"] == sc["models"][second]["material"]
        assert any(pa.get(k) != v for k, v in pb.items())
    gap = sc["models"][1]["xyz"][:, 0].min() - sc["models"][0]["xyz"][:, 0].max()
    assert 0.5 <= gap * 2.0 ** ms.BITS <= 1.5                                                    # their stencils overlap from the first substep on


# ---- 2. the GPU comparison accepts the oracle on eight models ---------------------------------------------------------------------------------------
def oracle_result(name, tier):
    """(bench stand-in, what Bench.step() would return - made by the oracle -, the models) of a scene"""
    sc = ms.scene(name, tier)
    res = oracle_as_engine([(m, p, st) for (m, p), st in zip(sc["parts"], sc["states"])], tier)
    return types.SimpleNamespace(parts=sc["parts"], bits=gm.BITS), res, ms.models(sc)


@pytest.mark.parametrize("tier", ms.TIERS)
@pytest.mark.parametrize("name", ["eight", "holes"])
def test_the_gpu_comparison_accepts_the_oracle_on_eight_models(name, tier):
    """check() of tests/test_g2p2g_blocks_gpu.py on the oracle's result for all eight slots, inside g2p2g_model.bound with no new constant.
    oracle_as_engine runs the oracle's particle body model by model and sums the eight contributions on one grid in float32 (its counts are
    the input sizes: check() is what is on trial here, not the oracle's books).  It accepts an empty model: `holes` runs with its empty
    slots in place, and check() must cope with their zero rows."""
    bench, res, models = oracle_result(name, tier)
    assert len(res["state"]) == len(models) == ms.NSLOTS
    assert [s["pos"].shape[0] for s in res["state"]] == [m["pos"].shape[0] for m in models] == [p.shape[0] for _, p in bench.parts]
    T.check(bench, res, models, tier, name)


# ---- 3. faults in the high slots ------------------------------------------------------------------------------------------------------------------
def _copy(res):
    return dict(res, state=[{k: v.copy() for k, v in s.items()} for s in res["state"]], grid=(res["grid"][0].copy(), res["grid"][1].copy()),
                counts=types.SimpleNamespace(particles=list(res["counts"].particles), particle_blocks=res["counts"].particle_blocks))


def drop_one_of_slot_7(bad, with_count):
    bad["state"][7] = {k: v[1:] for k, v in bad["state"][7].items()}
    if with_count:
        bad["counts"].particles[7] -= 1


def exchange_slots_5_and_6(bad):
    bad["state"][5], bad["state"][6] = bad["state"][6], bad["state"][5]


def scale_the_mass_of_slot_4(bad, sc, tier):
    """Slot 4's own P2G result (the oracle on that model alone) times 2^-10, added to the mass channel of the shared grid."""
    mat, pos = sc["parts"][4]
    own = oracle_as_engine([(mat, pos, sc["states"][4])], tier)
    at = {tuple(k): i for i, k in enumerate(bad["grid"][0].tolist())}
    for k, blk in zip(own["grid"][0].tolist(), own["grid"][1]):
        bad["grid"][1][at[tuple(k)], 0] += np.float32(2.0 ** -10) * blk[0]


def report_7_in_3(bad):
    p = bad["counts"].particles
    p[3], p[7] = p[7], p[3]


FAULTS = ["dropped", "dropped_and_counted", "exchanged", "mass", "counts"]


@pytest.mark.parametrize("fault", FAULTS)
def test_the_comparison_rejects_faults_in_the_high_slots(fault):
    """Four faults (the first in two forms), one at a time, each applied to the oracle's result on `eight` (flow tier) in slots 3 .. 7 only:
    one particle dropped from slot 7 (with and without its count), the states of slots 5 and 6 exchanged, slot 4's P2G mass scaled by 1 + 2^-10,
    counts.particles[7] reported in particles[3].  check() passes on the untouched result and fails on every one."""
    tier = "flow"
    bench, res, models = oracle_result("eight", tier)
    T.check(bench, res, models, tier, "eight, untouched")
    bad = _copy(res)
    if fault.startswith("dropped"):
        drop_one_of_slot_7(bad, fault == "dropped_and_counted")
    elif fault == "exchanged":
        exchange_slots_5_and_6(bad)
    elif fault == "mass":
        scale_the_mass_of_slot_4(bad, ms.scene("eight", tier), tier)
        assert not np.array_equal(bad["grid"][1], res["grid"][1])
    else:
        report_7_in_3(bad)
        assert bad["counts"].particles != res["counts"].particles
    with pytest.raises(AssertionError) as e:
        T.check(bench, bad, models, tier, "eight, " + fault)
    print(fault, "->", str(e.value)[:300])


# ---- 4. the checkpoint tools on eight models ----------------------------------------------------------------------------------------------------------
NCH = {gm.J_FLUID: 4, gm.FC: 9, gm.SAND: 10, gm.NACC: 10}


def synthetic_checkpoint8(sizes, layouts, rng, max_ppc=16):
    """test_g2p2g_model_cpu.synthetic_checkpoint for eight models that share the block numbering: sizes[m][b] particles of model m in block b
    (a model of all zeros is empty), layouts[m] its layout word (non-zero: the pair layout, with a pairinfo section).  Every section that is not set holds noise."""
    sizes = np.asarray(sizes, np.int64)
    nm, pbc = sizes.shape
    keys = np.array([[2 + b, 3 + b, 4 + b] for b in range(pbc)] + [[12, 12, 12]], np.int32)
    ebc = nbc = len(keys)
    order = rng.permutation(pbc)
    ppb = 64 * max_ppc
    pid_bits = ppb.bit_length() - 1
    nbins = (sizes + 63) // 64
    mods = []
    for m in range(nm):
        bincount = int(nbins[m].sum())
        mods.append(dict(material=ms.MATERIALS[m], nch=NCH[ms.MATERIALS[m]], list_in=0, layout=int(layouts[m]), n=int(sizes[m].sum()), bincount=bincount,
                         bincount_src=bincount, bucketed=int(sizes[m].sum())))
    h = dict(domain_bits=6, max_ppc=max_ppc, nmodels=nm, rollid=0, pbc=pbc, nbc=nbc, ebc=ebc, prev_count=pbc, prev_pbc=pbc, models=mods)
    sections, end = cf.layout(h)
    buf = rng.integers(0, 256, end, dtype=np.uint8)
    head = np.zeros(cf.HEADER_BYTES, np.uint8)
    head[:8].view(np.uint64)[0] = cf.MAGIC
    head[8:40].view(np.int32)[:] = [6, max_ppc, nm, 0, pbc, nbc, ebc, pbc]
    head[40:48].view(np.uint64)[0] = end
    head[56:60].view(np.int32)[0] = pbc
    for m, M in enumerate(mods):
        at = 64 + cf.MODEL_BYTES * m
        head[at:at + 16].view(np.int32)[:] = [M["material"], M["nch"], 0, M["layout"]]
        head[at + 16:at + 48].view(np.int64)[:] = [M["n"], M["bincount"], M["bincount"], M["bucketed"]]
    buf[:cf.HEADER_BYTES] = head

    def put(name, arr):
        at, n = sections[name]
        buf[at:at + n] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    put("cur_keys", keys)
    put("prev_keys", keys[order])
    first = 8.0
    for m, M in enumerate(mods):
        put(("size", m), np.concatenate([sizes[m], [0, 0]]).astype(np.int32))
        put(("row_of", m), np.arange(ebc + 1, dtype=np.int32))
        put(("binoff_src", m), np.concatenate([[0], np.cumsum(nbins[m][order])]).astype(np.int32))
        dst = np.zeros(ebc + 1, np.int32)
        dst[:pbc + 1] = np.concatenate([[0], np.cumsum(nbins[m])])
        put(("binoff_dst", m), dst)
        recs = [(13 << (pid_bits + cf.K_KEY_BITS)) | (rng.integers(0, 216, s) << pid_bits) | rng.permutation(s) for s in sizes[m]]
        put(("lists", m), np.concatenate(recs).astype(np.int32) if M["bucketed"] else np.zeros(0, np.int32))
        B = cf.bins(buf, m)
        rec = cf.rec_floats(M["nch"])
        n_slots = M["bincount"] * 64
        B[:] = rng.uniform(1.0, 2.0, B.shape).astype(np.float32)
        pos = np.arange(n_slots * 3, dtype=np.float32).reshape(n_slots, 3) * np.float32(0.25) + np.float32(first)
        for c in range(3):
            B[:, c:64 * rec:rec] = pos[:, c].reshape(M["bincount"], 64)
    return buf


@pytest.mark.parametrize("mask", [0x5, 0xA])
def test_checkpoint_tools_on_eight_models_with_mixed_layouts(mask):
    """cf.parse reads all eight CkptModel records and places every section - the pairinfo sections of the models in the pair layout, none for
    the others, nothing for the empty model - and cf.with_particle_state patches one model's particles and leaves every byte of the other seven."""
    rng = np.random.default_rng(mask)
    sizes = rng.integers(0, 140, (8, 5))
    sizes[:, 0] = [1, 64, 65, 130, 3, 0, 129, 70]
    sizes[3] = 0                                                                              # an empty model in the middle
    sizes[0, 1:] = 0                                                                          # a model absent from most blocks
    layouts = [2 * ((mask >> m) & 1) for m in ms.MATERIALS]                                 # 2: kPairLayoutId (mpm_checkpoint.inc), 0: sliced
    assert 0 < sum(layouts) < 16
    buf = synthetic_checkpoint8(sizes, layouts, rng)
    h = cf.parse(buf)
    assert h["nmodels"] == 8 and [M["layout"] for M in h["models"]] == layouts and [M["material"] for M in h["models"]] == ms.MATERIALS
    assert [M["n"] for M in h["models"]] == sizes.sum(axis=1).tolist() and h["models"][3]["n"] == 0
    for m in range(8):
        assert h["sections"]["pairinfo", m][1] == (4 * h["pbc"] * cf.K_PAIR_CHUNKS if layouts[m] else 0)
        assert h["sections"]["bins", m][1] == 4 * h["models"][m]["bincount_src"] * NCH[ms.MATERIALS[m]] * 64
    ends = sorted((at, at + n) for at, n in h["sections"].values())
    assert ends[0][0] == cf.HEADER_BYTES and all(b[0] == cf.pad16(a[1]) for a, b in zip(ends, ends[1:])) and cf.pad16(ends[-1][1]) == h["end"]
    before = [cf.particle_state(buf, m) for m in range(8)]
    assert [b["xyz_cells"].shape[0] for b in before] == sizes.sum(axis=1).tolist()
    assert np.array_equal(cf.with_particle_state(buf, 3, np.zeros((0, 3), np.float32), J=np.zeros(0, np.float32)), buf)       # the empty model: nothing to patch
    out = buf
    new = []
    for m, mat in enumerate(ms.MATERIALS):
        n = before[m]["xyz_cells"].shape[0]
        pick = rng.permutation(n)[:max(n // 2, min(n, 1))]
        xyz = before[m]["xyz_cells"][pick]
        if mat == gm.J_FLUID:
            st = dict(J=rng.uniform(0.8, 1.1, pick.size).astype(np.float32))
        else:
            st = dict(b=rng.uniform(0.5, 1.5, (pick.size, 6)).astype(np.float32), reflected=rng.random(pick.size) < 0.3)
            if mat != gm.FC:
                st["logjp"] = rng.uniform(-0.03, 0.01, pick.size).astype(np.float32)
        patched = cf.with_particle_state(out, m, xyz, **st)
        changed = np.flatnonzero(patched != out)
        at, nbytes = h["sections"]["bins", m]
        assert changed.size == 0 if n == 0 else (changed.size > 0 and at <= changed.min() and changed.max() < at + nbytes), (m, "bytes outside the model's bins changed")
        out = patched
        new.append((pick, st))
    assert np.array_equal(out[:cf.HEADER_BYTES], buf[:cf.HEADER_BYTES]) and cf.parse(out)["sections"] == h["sections"]
    for m in range(8):
        after = cf.particle_state(out, m)
        pick, st = new[m]
        assert np.array_equal(after["xyz_cells"].view(np.uint32), before[m]["xyz_cells"].view(np.uint32))
        for k in ("b", "logjp", "J", "reflected"):
            if before[m][k] is None:
                assert after[k] is None
                continue
            want = before[m][k].copy()
            if k in st:
                want[pick] = st[k]
            assert np.array_equal(after[k], want), (m, k)


# ---- check_books on a loaded state ------------------------------------------------------------------------------------------------------------------
def test_check_books_holds_a_loaded_state_to_the_identity_row_of():
    """mpm_checkpoint_load lays the lists out anew, block b's in row b (unpack_lists_kernel writes row_of[b] = b): check_books(loaded=True) holds
    row_of to the identity where check_books() holds it to the block's previous number.  On the model's books (tests/rebuild_model.py): the
    rebuild's own row_of passes the one rule and fails the other, the identity the other way round, and one entry off the identity is reported."""
    import rebuild_books as rb
    import rebuild_model as rmod
    from test_rebuild_books_cpu import BITS, MAX_PPC, case
    prev, moves = case(1)
    ckpt, rows = rmod.rebuild(prev, moves, seed=1)
    h = cf.parse(ckpt)
    assert rb.check_books(ckpt, rows, BITS, MAX_PPC) == []
    assert {f[0] for f in rb.check_books(ckpt, rows, BITS, MAX_PPC, loaded=True)} == {"row_of"}
    loaded = ckpt.copy()
    for m in range(h["nmodels"]):
        cf.section(loaded, h, ("row_of", m), np.int32)[:h["pbc"]] = np.arange(h["pbc"])
    assert rb.check_books(loaded, rows, BITS, MAX_PPC, loaded=True) == []
    assert {f[0] for f in rb.check_books(loaded, rows, BITS, MAX_PPC)} == {"row_of"}
    cf.section(loaded, h, ("row_of", 1), np.int32)[2] = 3
    found = rb.check_books(loaded, rows, BITS, MAX_PPC, loaded=True)
    assert [f[:3] for f in found] == [("row_of", 1, [2])], found
