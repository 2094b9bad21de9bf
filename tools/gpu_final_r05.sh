#!/usr/bin/env bash
# round 5: [tests selected by $1] + smoke + the driver's bench line + the profile set (tools/gpu_profile_r05.sh all)
# the bench line (bench.py --full) is written in place: profiles/r05_bench_default_line.json
cd "$(dirname "$0")/.."
mkdir -p gpurun_out
export TMPDIR=/tmp
cat build_stamp.txt
if [ -n "$1" ]; then
  timeout 1500 python -m pytest tests -m gpu -q -k "$1" > gpurun_out/r05_select_pytest.log 2>&1; echo "pytest rc $?" >> gpurun_out/r05_select_pytest.log
  grep -E "^(FAILED|ERROR)|passed|failed|pytest rc" gpurun_out/r05_select_pytest.log | tail -12
fi
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > gpurun_out/r05_smoke.log 2>&1; tail -1 gpurun_out/r05_smoke.log
# the profile set first: bench.py attaches the counters of profiles/r05_pmc.json only if they were taken with the library it loads
bash tools/gpu_profile_r05.sh all > gpurun_out/r05_profile.log 2>&1
tail -3 gpurun_out/r05_profile.log
python tools/make_pmc_json.py gpurun_out/prof_r05 profiles/r05_pmc.json > /dev/null && cp profiles/r05_pmc.json gpurun_out/r05_pmc.json
timeout 900 python bench.py --full --steps 20 --warmup 5 > profiles/r05_bench_default_line.json; echo "bench rc $?"
tail -c 300 profiles/r05_bench_default_line.json
