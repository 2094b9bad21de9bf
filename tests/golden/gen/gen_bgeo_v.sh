#!/usr/bin/env bash
# Regenerates tests/golden/g10_velocity.f32 and g10_partio_v.bgeo: the point set of g10_points.f32 (gen_bgeo.sh) with a deterministic
# velocity per point, written with a "v" point attribute by the reference's own partio library (Externals/partio/core/*.cpp + io/*.cpp
# compiled where they lie, no zlib: uncompressed .bgeo needs none).  Runs only where /root/reference is mounted; tests read the
# committed files.
set -euo pipefail
REF=${REF:-/root/reference}
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(cd "$HERE/.." && pwd)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
P="$REF/Externals/partio"
g++ -std=c++11 -O1 -w -I"$P" "$HERE/gen_bgeo_v.cpp" "$P"/core/*.cpp "$P"/io/*.cpp -o "$TMP/gen_bgeo_v" -lpthread
python3 - "$OUT/g10_velocity.f32" <<'PY'
import sys, numpy as np
# 1000 deterministic velocities: signed values of several magnitudes, zeros, a negative zero, extremes that need all 4 bytes
i = np.arange(1000, dtype=np.float64)
v = np.stack([np.cos(0.91 * i) * 2.5, -9.8 * ((i * 0.7548776662) % 1.0), np.sin(0.13 * i) * 1e-3], axis=1).astype(np.float32)
v[0] = (0.0, -0.0, 1.0)
v[1] = (np.float32(-3.4e38), np.float32(1e-30), np.float32(7.5e-8))
v[2] = (0.3, -0.7, 1.1)
v.tofile(sys.argv[1])
PY
"$TMP/gen_bgeo_v" "$OUT/g10_points.f32" "$OUT/g10_velocity.f32" "$TMP/g10_partio_v.bgeo"
cp "$TMP/g10_partio_v.bgeo" "$OUT/g10_partio_v.bgeo"
ls -l "$OUT/g10_velocity.f32" "$OUT/g10_partio_v.bgeo"
