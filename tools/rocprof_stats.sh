#!/usr/bin/env bash
# rocprofv3 --kernel-trace --stats of bench.py --full (op only), summary -> $RK_PROFILE_DIR/<name>/
# usage (on the GPU box): RK_PROFILE_DIR=<output dir> bash tools/rocprof_stats.sh <name> [bench args]
set -u
name=$1; shift
root=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
out="${RK_PROFILE_DIR:?set RK_PROFILE_DIR to the output directory}/$name"; mkdir -p "$out"; out=$(cd "$out" && pwd)
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$out" -o "$name" -- \
    python "$root/bench.py" --steps 30 --warmup 5 --full --models none --no-cpu --no-legs "$@" > "$out/bench.json" 2> "$out/bench.err"
echo "rocprofv3 rc=$?"
ls "$out"
f=$(find "$out" -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && head -8 "$f"
