"""The injection bench of the block-level GPU tests (tests/test_g2p2g_blocks_gpu.py, tests/test_rebuild_books_gpu.py): one context, set up,
checkpointed and re-loaded with injected particle state and grid velocities (tests/ckpt_format.py), stepped through mpm_g2p2g + mpm_rebuild_partition.

Test infrastructure only."""
import numpy as np

import ckpt_format as cf
import g2p2g_model as gm
from claymore_amd.engine import build_engine


def st9_to_b6(st9):
    """mpm_retrieve_state's symmetric 3 x 3 -> ({00, 11, 22, 10, 20, 21} with |b00|, the reflected mark)"""
    s = np.asarray(st9)
    return np.stack([np.abs(s[:, 0]), s[:, 4], s[:, 8], s[:, 1], s[:, 2], s[:, 5]], axis=1), np.signbit(s[:, 0])


def by_position_bits(xyz):
    x = np.ascontiguousarray(xyz, np.float32).view(np.uint32)
    return np.lexsort((x[:, 2], x[:, 1], x[:, 0]))


class Bench:
    """One context holding one model per (material, positions in cells): set up, checkpointed, and re-loaded with injected state and grid."""

    def __init__(self, parts, bits=gm.BITS, max_ppc=gm.MAX_PPC, overrides=None):
        self.bits, self.dx = bits, 0.5 ** bits
        self.parts = [(m, np.ascontiguousarray(p, np.float32)) for m, p in parts]
        self.over = [overrides[i] if overrides else gm.material_overrides(m, bits) for i, (m, _) in enumerate(self.parts)]
        sc = {"name": "g2p2g_blocks", "bits": bits, "dt": gm.DT, "config": {"max_ppc": max_ppc},
              "models": [{"material": m, "xyz": p * np.float32(self.dx), "v0": (0.0, 0.0, 0.0), "params": dict(o)} for (m, p), o in zip(self.parts, self.over)]}
        self.eng = build_engine(sc)
        self.eng.initial_setup()
        self.ckpt = self.eng.save_checkpoint().copy()
        self.consts = [gm.constants(m, o) for (m, _), o in zip(self.parts, self.over)]

    def close(self):
        self.eng.close()

    def read(self, i):
        """Model i as mpm_retrieve_state returns it: positions in cells (exact), b6, reflected, log Jp, J"""
        x, st, lj = self.eng.retrieve_state(i)
        assert x.shape[0] == self.parts[i][1].shape[0], "a particle is missing from the buckets"
        b6, refl = st9_to_b6(st)
        return dict(pos=x * np.float32(2.0 ** self.bits), b6=b6, reflected=refl, logjp=lj.copy(), J=st[:, 0].copy())

    def load(self, buf, vgrid):
        """Load `buf` with channels 1 .. 3 of its grid replaced: vgrid(keys (nbc, 3)) -> (nbc, 3, 64).  The mass channel is left as saved."""
        g = cf.grid(buf).copy()
        g[:, 1:4] = vgrid(cf.cur_keys(buf)[:g.shape[0]])
        self.eng.load_checkpoint(cf.with_grid(buf, g))

    def inject(self, states, vgrid):
        """The set-up checkpoint with the states patched in and the grid's velocity channels from vgrid; asserts that the context then holds the injected
        b, reflected mark, log Jp and J bit for bit."""
        buf = self.ckpt
        for i, ((m, p), st) in enumerate(zip(self.parts, states)):
            buf = cf.with_particle_state(buf, i, p, J=st["J"]) if m == gm.J_FLUID else cf.with_particle_state(buf, i, p, b=st["b6"], logjp=st["logjp"], reflected=st["reflected"])
        self.load(buf, vgrid)
        for i, ((m, p), st) in enumerate(zip(self.parts, states)):
            got = self.read(i)
            og, ow = by_position_bits(got["pos"]), by_position_bits(p)
            assert np.array_equal(got["pos"][og].view(np.uint32), p[ow].view(np.uint32)), "the positions changed"
            for k in ("J",) if m == gm.J_FLUID else ("b6", "reflected") + (("logjp",) if st["logjp"] is not None else ()):
                a, b = np.ascontiguousarray(got[k][og]), np.ascontiguousarray(st[k][ow])
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, "the context does not hold the injected state bit for bit")

    def step(self):
        """mpm_g2p2g(dt, new_dt) + mpm_rebuild_partition -> what came out"""
        d0 = self.eng.diagnostics()
        before = (int(d0.lost_particles), int(d0.discarded_p2g))
        self.eng.g2p2g(gm.DT, gm.NEW_DT)
        cnt = self.eng.rebuild_partition()
        d1 = self.eng.diagnostics()
        gk, gb = self.eng.dump_grid()
        return dict(counts=cnt, lost=int(d1.lost_particles) - before[0], discarded=int(d1.discarded_p2g) - before[1], grid=(gk, gb),
                    state=[self.read(i) for i in range(len(self.parts))])
