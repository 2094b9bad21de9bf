#!/usr/bin/env bash
# Resource / instruction summary of the four g2p2g instantiations, of the readout kernels, of the grid kernels and of the particle-id kernels (the plain grid update and carry-overs, and the two collider frames for the level-set object, the shapes and the terrain).  usage: tools/kstat.sh [extra hipcc flags...]
D=$(mktemp -d); trap 'rm -rf $D' EXIT
cd "$(dirname "$0")/../claymore_amd/csrc"
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics -Wno-unused-value -fno-slp-vectorize "$@" -save-temps=obj -o $D/x.so claymore_hip.hip 2>&1 | grep -E "error|warning: v" | head
S=$D/claymore_hip-hip-amdgcn-amd-amdhsa-gfx950.s
for m in 0 1 2 3 P0 P1 P2 P3; do
  case $m in P*) sym="_ZN3mpm17g2p2g_pair_kernelILi${m#P}E";; *) sym="_ZN3mpm12g2p2g_kernelILi${m}E";; esac   # (P*: two particles per lane, mpm_g2p2g_pair.hpp)
  awk "/^${sym}/,/\.end_amdhsa_kernel/" $S > $D/k$m.s
  [ -n "$KEEP" ] && cp $D/k$m.s $KEEP.$m.s
  echo "MAT $m: valu $(grep -cE '^\s+v_' $D/k$m.s) pk $(grep -cE '^\s+v_pk' $D/k$m.s) salu $(grep -cE '^\s+s_' $D/k$m.s) lds $(grep -cE '^\s+ds_' $D/k$m.s) vmem $(grep -cE '^\s+(global|buffer|scratch)_' $D/k$m.s) scratch_ops $(grep -cE '^\s+scratch_' $D/k$m.s) | $(grep -E 'next_free_vgpr|private_segment_fixed_size|group_segment_fixed_size' $D/k$m.s | awk '{printf "%s=%s ", $1, $2}')"
done
for k in 0 1 2 3 4 5; do   # readout_kernel<kReadState .. kReadStressTotals, kReadIds>, mpm_readout.hpp
  awk "/^_ZN3mpm14readout_kernelILNS_11ReadoutKindE${k}E/,/\.end_amdhsa_kernel/" $S > $D/r.s
  echo "readout $k: valu $(grep -cE '^\s+v_' $D/r.s) salu $(grep -cE '^\s+s_' $D/r.s) lds $(grep -cE '^\s+ds_' $D/r.s) vmem $(grep -cE '^\s+(global|buffer|scratch)_' $D/r.s) | $(grep -E 'next_free_vgpr|private_segment_fixed_size|group_segment_fixed_size' $D/r.s | awk '{printf "%s=%s ", $1, $2}')"
done
for k in grid_update=_ZN3mpm18grid_update_kernelE "carry<false>=_ZN3mpm17carry_grid_kernelILb0ENS_11NoCollisionEEE" "carry<true>=_ZN3mpm17carry_grid_kernelILb1ENS_11NoCollisionEEE" \
    "grid_update<CollisionArgs>=_ZN3mpm27grid_update_collider_kernelINS_13CollisionArgsEEE" "carry<true,CollisionArgs>=_ZN3mpm17carry_grid_kernelILb1ENS_13CollisionArgsEEE" \
    "grid_update<ShapeArgs>=_ZN3mpm27grid_update_collider_kernelINS_9ShapeArgsEEE" "carry<true,ShapeArgs>=_ZN3mpm17carry_grid_kernelILb1ENS_9ShapeArgsEEE" \
    "grid_update<TerrainArgs>=_ZN3mpm27grid_update_collider_kernelINS_11TerrainArgsEEE" "carry<true,TerrainArgs>=_ZN3mpm17carry_grid_kernelILb1ENS_11TerrainArgsEEE"; do
  awk "/^${k#*=}/,/\.end_amdhsa_kernel/" $S > $D/g.s
  echo "${k%%=*}: valu $(grep -cE '^\s+v_' $D/g.s) salu $(grep -cE '^\s+s_' $D/g.s) vmem $(grep -cE '^\s+(global|buffer|scratch)_' $D/g.s) scratch_ops $(grep -cE '^\s+scratch_' $D/g.s) | $(grep -E 'next_free_vgpr|next_free_sgpr|private_segment_fixed_size' $D/g.s | awk '{printf "%s=%s ", $1, $2}')"
done
for k in move_ids=_ZN3mpm15move_ids_kernelE fill_ids=_ZN3mpm15fill_ids_kernelE; do   # mpm_particle_ids.hpp
  awk "/^${k#*=}/,/\.end_amdhsa_kernel/" $S > $D/g.s
  echo "${k%%=*}: valu $(grep -cE '^\s+v_' $D/g.s) salu $(grep -cE '^\s+s_' $D/g.s) lds $(grep -cE '^\s+ds_' $D/g.s) vmem $(grep -cE '^\s+(global|buffer|scratch)_' $D/g.s) scratch_ops $(grep -cE '^\s+scratch_' $D/g.s) | $(grep -E 'next_free_vgpr|next_free_sgpr|private_segment_fixed_size|group_segment_fixed_size' $D/g.s | awk '{printf "%s=%s ", $1, $2}')"
done
