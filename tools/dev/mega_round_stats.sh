#!/bin/bash
# how full the test rounds of k_mega's leaf scan run: items and rounds per pass, and the item count of every pass's last round in eight bins
# of eight (what splitting a short last round by primitive can save: profiles/mega_round_ab.txt).  Needs the instrumented variant:
#   LJ_VARIANT=rstats LJ_EXTRA_HIPCC_FLAGS="-DLJ_MEGA_ROUND_STATS=1" python -m lajolla_public_amd.build      (build container; the .so travels)
cd "$(dirname "$0")/../.."
export LJ_NO_REBUILD=1 LJ_VARIANT=rstats
for c in cbox/cbox.xml:256 veach_mi/mi.xml:64; do
  echo "== ${c%%:*} @ ${c##*:} spp"
  timeout -k 10 300 python3 tools/render_once.py scenes/${c%%:*} ${c##*:} 1 0 2>&1 | grep -v Warning || exit 1
done
