#!/usr/bin/env bash
# Regenerates tests/golden/g10_stress.f32 and g10_partio_stress.bgeo: the point set of g10_points.f32 (gen_bgeo.sh) with nine deterministic
# values per point {stress6, J, pressure, von Mises}, written as the point attributes "stress" (6 floats), "J", "pressure" and "vonmises"
# by the reference's own partio library (Externals/partio/core/*.cpp + io/*.cpp compiled where they lie, no zlib: uncompressed .bgeo needs
# none), following gen_bgeo_v.sh.  Runs only where the reference is checked out (REF names it); tests read the committed files.
set -euo pipefail
REF=${REF:?set REF to the checkout of the reference project}
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(cd "$HERE/.." && pwd)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
P="$REF/Externals/partio"
g++ -std=c++11 -O1 -w -I"$P" "$HERE/gen_bgeo_stress.cpp" "$P"/core/*.cpp "$P"/io/*.cpp -o "$TMP/gen_bgeo_stress" -lpthread
python3 - "$OUT/g10_stress.f32" <<'PY'
import sys, numpy as np
# 1000 deterministic rows: stresses of several signs and magnitudes, J around 1, zeros, a negative zero, extremes that need all 4 bytes
i = np.arange(1000, dtype=np.float64)
s = np.stack([np.cos(0.91 * i) * 2.5e3, -9.8e2 * ((i * 0.7548776662) % 1.0), np.sin(0.13 * i) * 1e-3, np.sin(0.37 * i) * 40.0,
              np.cos(0.53 * i) * 7.0, -np.sin(0.71 * i) * 300.0, 1.0 + 0.2 * np.sin(0.29 * i), 1.7e3 * np.cos(0.17 * i),
              np.abs(np.sin(0.61 * i)) * 3.1e3], axis=1).astype(np.float32)
s[0] = (0.0, -0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
s[1] = (np.float32(-3.4e38), np.float32(1e-30), np.float32(7.5e-8), 1.0, 2.0, 3.0, np.float32(0.1), np.float32(-1e-30), np.float32(3.4e38))
s.tofile(sys.argv[1])
PY
"$TMP/gen_bgeo_stress" "$OUT/g10_points.f32" "$OUT/g10_stress.f32" "$TMP/g10_partio_stress.bgeo"
cp "$TMP/g10_partio_stress.bgeo" "$OUT/g10_partio_stress.bgeo"
ls -l "$OUT/g10_stress.f32" "$OUT/g10_partio_stress.bgeo"
