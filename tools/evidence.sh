#!/bin/bash
# everything profiles/ is refreshed from, in one call:  tools/evidence.sh <tag>
TAG=$1
cd $GRAFT_REPO_ROOT
O=${LJ_OUT_DIR:-out}   # where the profiles and logs go (relative to the repository root)
mkdir -p $O
bash tools/prof_bench_1lane.sh $TAG > $O/evidence_1lane_$TAG.txt 2>&1 && echo "1-lane stats done" &&
bash tools/prof_bench.sh $TAG > $O/evidence_default_$TAG.txt 2>&1 && echo "default stats + PMC done" &&
timeout -k 10 300 python3 bench.py --full > $O/bench_default_$TAG.json 2> $O/bench_default_$TAG.err && echo "default bench done" && tail -1 $O/bench_default_$TAG.json | cut -c1-200 &&
: > $O/bench_configs_$TAG.jsonl &&
for c in disney_bsdf_test/disney_bsdf.xml:256 veach_mi/mi.xml:512 sponza/sponza.xml:1024; do
  timeout -k 10 300 python3 bench.py --full --scene scenes/${c%%:*} --spp ${c##*:} --steps 3 --no-cpu-baseline 2>/dev/null | tail -1 >> $O/bench_configs_$TAG.jsonl && echo "config ${c%%:*} done" || exit 1
done
cut -c1-160 $O/bench_configs_$TAG.jsonl
