#!/bin/bash
# profiles/rebuild_time.txt: tools/rebuild_time.py scene by scene, each GPU step under its own time limit; stops at the first failure.
#   tools/rebuild_time.sh [output file, default profiles/rebuild_time.txt]
set -euo pipefail
cd "$(dirname "$0")/.."
OUT="${1:-profiles/rebuild_time.txt}"
TMP="${LJ_OUT_DIR:-out}/rebuild_time"
mkdir -p "$TMP" "$(dirname "$OUT")"
for scene in cbox disney_bsdf sponza; do
    timeout -k 10 420 python tools/rebuild_time.py --scenes "$scene" --out "$TMP/$scene.txt" > "$TMP/$scene.log" 2>&1 || { rc=$?; tail -20 "$TMP/$scene.log"; echo "rebuild_time: $scene failed ($rc)"; exit "$rc"; }
done
{ head -4 "$TMP/cbox.txt"; for scene in cbox disney_bsdf sponza; do tail -n +5 "$TMP/$scene.txt"; done; } > "$OUT"
cat "$OUT"
