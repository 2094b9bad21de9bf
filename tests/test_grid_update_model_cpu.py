"""The model and the tools of tests/test_grid_update_kernels_gpu.py, judged without a GPU: tests/grid_update_model.py against the golden
cells of the reference's own grid-update statements (G19), tests/ckpt_format.py's layout arithmetic, and the generator's coverage."""
import struct

import numpy as np
import pytest

import ckpt_format as cf
import grid_update_model as gm
from test_oracle_golden import f32, kernel_rows

SEEDS = (1, 2, 3)            # the seeds tests/test_grid_update_kernels_gpu.py uses


def test_strict_model_reproduces_the_references_golden_cells():
    """G19 (tests/golden/g19_gridcell_*.f32: 512 cells through the reference's own statements, gravity -9.8, the arenas' dt): the strict
    variant gives the velocities of every live cell and |v|^2 of every cell bit for bit (NaNs as NaNs: grid_update_model's note)."""
    P = kernel_rows()[0]
    cells = f32("g19_gridcell_in.f32").reshape(-1, 5)
    want = f32("g19_gridcell_out.f32").reshape(-1, 4)
    flags = cells[:, 4].astype(np.int64)
    live, (v0, v1s, v1f, v2) = gm.cell_update(cells[:, 0], cells[:, 1], cells[:, 2], cells[:, 3], (flags & 4) != 0, (flags & 2) != 0, (flags & 1) != 0,
                                              gm.gdt32(-9.8, P["dt"]))
    assert np.array_equal(live, cells[:, 0] > 0) and live.sum() >= 300 and (~live).sum() >= 100
    for got, col in ((v0, 0), (v1s, 1), (v2, 2)):
        assert np.array_equal(gm.canon(got[live]), gm.canon(want[live, col])), col
    q = np.where(live, gm.plain_q32(v0, v1s, v2), np.float32(0.0))
    assert np.array_equal(gm.bits(q), gm.bits(want[:, 3]))
    assert np.isinf(want[:, 3]).sum() >= 6
    # the set tells the two v1 candidates apart (so `strict` above is a statement about the reference), and the float64 Q the GPU tests use
    # lies within the derived bound of the reference's float32 |v|^2
    assert (gm.bits(v1f[live]) != gm.bits(v1s[live])).sum() >= 10
    fin = live & np.isfinite(want[:, 3])
    Q = v0[fin].astype(np.float64) ** 2 + v1s[fin].astype(np.float64) ** 2 + v2[fin].astype(np.float64) ** 2
    assert (np.abs(want[fin, 3].astype(np.float64) - Q) <= gm.PLAIN_MAX_ULPS * gm.ulp32(Q)).all()


def test_fused_candidate_is_one_rounding():
    """fma32 against exact rational arithmetic on products that cancel against the addend, ties of the float64 sum included."""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)
    c[::7] = np.float32(2.0 ** 40) * a[::7]
    c[::11] = np.float32(2.0 ** -60)
    got = gm.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                       # (float(Fraction) rounds once to float64; used only to find the two neighbours)
        cand = sorted({float(np.nextafter(lo, np.float32(-np.inf))), float(lo), float(np.nextafter(lo, np.float32(np.inf)))})
        best = min(cand, key=lambda x: (abs(Fraction(x) - exact), int(np.float32(x).view(np.uint32)) & 1))
        assert float(got[i]) == best, (i, a[i], b[i], c[i], got[i], best)


def test_ulp32_and_the_wall_rule():
    assert gm.ulp32(1.0) == 2.0 ** -23 and gm.ulp32(1.999) == 2.0 ** -23 and gm.ulp32(2.0) == 2.0 ** -22 and gm.ulp32(1e-45) == 2.0 ** -149 and gm.ulp32(0.0) == 2.0 ** -149
    keys = np.array([[0, 1, 2], [13, 14, 15]])
    assert gm.wall_flags(keys, 16, 2).tolist() == [[True, True, False], [False, True, True]]
    assert gm.wall_flags(keys, 16, 1).tolist() == [[True, False, False], [False, False, True]]
    assert gm.wall_class(keys, 16, 2).tolist() == [[0, 0, 1], [1, 2, 2]]
    nd = gm.node_coords(np.array([[1, 2, 3]]))
    assert nd[0, :, 0].tolist() == [4, 8, 12] and nd[0, :, 63].tolist() == [7, 11, 15] and nd[0, :, 0b011011].tolist() == [5, 10, 15]


def test_skipped_cells_and_wall_components():
    """The model's own rules on hand-made cells: masses +0 / -0 / negative / NaN leave all four channels alone; a wall component is +0 and
    a y wall still receives gravity * dt; FLT_MIN, a denormal and +inf are live."""
    u = lambda *x: np.array(x, dtype=np.uint32)
    grid = np.zeros((2, 4, 64), np.uint32)
    grid[:, 0, :8] = u(0, 0x80000000, 0xBF800000, 0x7FC12345, 0x00800000, 0x00000001, 0x7F800000, 0x3F800000)
    grid[:, 1:, :8] = u(0xFFC54321, 0x7F800000, 0x3F800000, 0x00000001, 0x00000003, 0x00000001, 0x3F800000, 0xC0000000)
    keys = np.array([[7, 7, 7], [0, 15, 1]])
    live, strict, fused = gm.plain(keys, 16, 2, -9.8, 1e-4, grid.view(np.float32))
    assert live[0, :8].tolist() == [False] * 4 + [True] * 4 and not live[:, 8:].any()
    assert np.array_equal(gm.bits(strict)[:, :, :4], grid[:, :, :4]) and np.array_equal(gm.bits(strict)[:, 0], grid[:, 0])
    g = gm.gdt32(-9.8, 1e-4)
    assert (gm.bits(strict)[1, 1, 4:8] == 0).all() and (gm.bits(strict)[1, 3, 4:8] == 0).all() and (strict[1, 2, 4:8] == g).all()
    assert strict[0, 1, 4] == np.float32(3 * 2.0 ** -149 * 2.0 ** 126) and np.isinf(strict[0, 1, 5]) and strict[0, 1, 6] == 0 and strict[0, 1, 7] == -2
    assert gm.max_q64(strict, live) == np.inf and gm.max_q64(strict[1:], live[1:]) == float(g) ** 2


def _header(nmodels, pbc, nbc, ebc, prev_count, models, grid_velocity=0, total=None):
    """CkptHeader bytes (mpm_checkpoint.inc) for made-up counts; models: (material, nch, list_in, layout, n, bincount, bincount_src, bucketed)."""
    h = struct.pack("<Q4i4iQQ2i", cf.MAGIC, 6, 128, nmodels, 0, pbc, nbc, ebc, prev_count, 0, 0x1234, pbc, grid_velocity)
    for m in range(8):
        h += struct.pack("<4i4q", *(models[m] if m < nmodels else (0,) * 8))
    assert len(h) == cf.HEADER_BYTES
    hd = cf.header(np.frombuffer(h, np.uint8))
    end = cf.layout(hd)[1] if total is None else total
    return np.frombuffer(h[:40] + struct.pack("<Q", end) + h[48:], np.uint8).copy()


def test_checkpoint_layout_arithmetic():
    """Padding, section order, two models with different nch, a sliced and a pair-layout model."""
    assert [cf.pad16(n) for n in (0, 1, 15, 16, 17, 4 * 3 * 7)] == [0, 16, 16, 16, 32, 96]
    models = [(1, 8, 0, 2, 1000, 30, 29, 990), (0, 4, 1, 0, 77, 5, 6, 77)]
    head = _header(2, 5, 7, 11, 9, models)
    h = cf.header(head)
    assert (h["pbc"], h["nbc"], h["ebc"], h["prev_count"], h["prev_pbc"], h["grid_velocity"]) == (5, 7, 11, 9, 5, 0)
    assert [m["nch"] for m in h["models"]] == [8, 4] and h["models"][0]["bucketed"] == 990 and h["models"][1]["bincount_src"] == 6
    sec, end = cf.layout(h)
    want, o = [], 448
    for name, nbytes in [("cur_keys", 132), ("prev_keys", 108), ("grid", 7168),
                         (("size", 0), 48), (("row_of", 0), 48), (("binoff_src", 0), 40), (("binoff_dst", 0), 48), (("bins", 0), 4 * 29 * 8 * 64), (("lists", 0), 3960), (("pairinfo", 0), 320),
                         (("size", 1), 48), (("row_of", 1), 48), (("binoff_src", 1), 40), (("binoff_dst", 1), 48), (("bins", 1), 4 * 6 * 4 * 64), (("lists", 1), 308), (("pairinfo", 1), 0)]:
        want.append((name, (o, nbytes)))
        o += (nbytes + 15) // 16 * 16
    assert list(sec.items()) == want and end == o == h["total_bytes"]
    assert all(at % 16 == 0 for at, _ in sec.values())
    # a whole buffer: grid() is a view of the right bytes, with_grid() changes those bytes only
    buf = np.concatenate([head, (np.arange(end - 448) % 251).astype(np.uint8)])
    g = cf.grid(buf)
    assert g.shape == (7, 4, 64) and g.base is not None and np.array_equal(g.view(np.uint8).reshape(-1), buf[sec["grid"][0]:sec["grid"][0] + 7168])
    assert np.array_equal(cf.cur_keys(buf).view(np.uint8).reshape(-1), buf[448:448 + 132])
    new = np.arange(7 * 256, dtype=np.uint32).reshape(7, 4, 64) | np.uint32(0x7FC00000)
    out = cf.with_grid(buf, new)
    assert np.array_equal(cf.grid(out).view(np.uint32), new) and out is not buf
    at = sec["grid"][0]
    assert np.array_equal(out[:at], buf[:at]) and np.array_equal(out[at + 7168:], buf[at + 7168:])
    with pytest.raises(AssertionError):
        cf.with_grid(buf, new[:6])


def test_checkpoint_parse_refuses_what_it_must():
    models = [(1, 8, 0, 2, 10, 1, 1, 10)]
    ok = _header(1, 1, 8, 27, 27, models)
    body = np.zeros(cf.header(ok)["total_bytes"] - 448, np.uint8)
    cf.parse(np.concatenate([ok, body]))
    with pytest.raises(AssertionError):
        cf.parse(np.concatenate([ok, body[:-16]]))                                          # truncated
    with pytest.raises(AssertionError):
        cf.parse(np.concatenate([_header(1, 1, 8, 27, 27, models, grid_velocity=1), body]))   # an updated grid
    with pytest.raises(AssertionError):
        cf.parse(np.concatenate([_header(1, 1, 8, 27, 27, models, total=body.size + 448 + 16), body]))


def test_scene_blocks():
    """The scene's neighbour blocks: 222 (no multiple of 4 or 16), all 27 wall classes for boundary 2 and 1; its particles sit in the blocks
    the model says (face_scenes.kernel_axis) and share no stencil node."""
    import face_scenes as fs
    keys = gm.scene_keys()
    assert len(keys) == 222 and len(keys) % 16 and len(keys) % 4
    for boundary in (2, 1):
        assert len({tuple(c) for c in gm.wall_class(keys, gm.G_BLOCKS, boundary).tolist()}) == 27
    cells = gm.scene_cells()
    _, base, key, _ = fs.kernel_axis(cells)
    assert sorted(map(tuple, key.tolist())) == gm.scene_particle_blocks()
    nodes = set()
    for b in base:
        mine = {(b[0] + i, b[1] + j, b[2] + k) for i in range(3) for j in range(3) for k in range(3)}
        assert not (nodes & mine)
        nodes |= mine
    assert min(min(n) for n in nodes) >= 0 and max(max(n) for n in nodes) < 64


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("tier", gm.TIERS)
@pytest.mark.parametrize("boundary", [2, 1])
def test_generator_covers_every_class_in_every_wall_class(boundary, tier, seed):
    """A condition on the GPU tests' inputs, checked here so that they cannot pass by leaving a class out: on every seed used, every mass class
    and - in live cells - every momentum class of every component occurs in each of the 27 wall classes; the classes are what they claim."""
    keys = gm.scene_keys()
    pat, mcls, pcls = gm.generate(len(keys), seed, tier)
    assert gm.coverage_gaps(keys, gm.G_BLOCKS, boundary, mcls, pcls, tier) == []
    v = pat.view(np.float32)
    m, names = v[:, 0], gm.MASS_CLASSES
    with np.errstate(all="ignore"):
        checks = {"ordinary": (m >= 2.0 ** -27) & (m < 2.0 ** -6), "flt_min": pat[:, 0] == 0x00800000, "denormal": (m > 0) & (m < 2.0 ** -126),
                  "+0": pat[:, 0] == 0, "-0": pat[:, 0] == 0x80000000, "negative": m < 0, "nan": np.isnan(m), "+inf": pat[:, 0] == 0x7F800000}
        for i, n in enumerate(names):
            assert checks[n][mcls == i].all(), n
        live = m > 0
        assert np.array_equal(live, np.isin(mcls, gm.LIVE_MASS))
        inv = np.float32(1.0) / np.where(live, m, np.float32(1.0))
        for d in range(3):
            p, c = v[:, 1 + d], pcls[:, d]
            assert (pat[:, 1 + d][c == 1] == 0).all() and (pat[:, 1 + d][c == 2] == 0x80000000).all()
            assert ((np.abs(p[c == 3]) < 2.0 ** -126) & (p[c == 3] != 0)).all()
            assert np.isposinf(p[c == 5]).all() and np.isneginf(p[c == 6]).all() and np.isnan(p[c == 7]).all()
            assert np.isinf((p * inv)[(c == 4) & (mcls == 0)]).all() and np.isfinite(p[c == 4]).all()
            if tier != "full":
                vel = (p * inv)[live]
                assert np.isfinite(vel).all() and (np.abs(vel) < (16 if tier == "finite" else 2.0 ** -12)).all()
    if tier == "full":
        assert (mcls == 7).any() and np.isin(pcls[:, :, :], (4, 5, 6, 7)).any()
    else:
        assert not np.isin(mcls, (6, 7)).any()
    # another seed gives another grid
    assert not np.array_equal(pat, gm.generate(len(keys), seed + 100, tier)[0])
