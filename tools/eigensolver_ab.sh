#!/bin/bash
# A/B of two BUILDS of the library on one box, for a change that must compute the same and run as fast:
#   tools/eigensolver_ab.sh <part> <variant> <variant>     (tools/ab/libscanpy_amd_<variant>.so; parts: cases dumps speed spectral)
# Every run is a fresh process under its own time limit; the first failure ends the script.  Raw lines go to $OUT (build/ab).
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"; cd "$R"
PART="$1"; A="$2"; B="$3"; OUT="${OUT:-build/ab}"; mkdir -p "$OUT"
KEEP="$(mktemp)"; cp scanpy_amd/_lib/libscanpy_amd.so "$KEEP"
trap 'cp "$KEEP" scanpy_amd/_lib/libscanpy_amd.so; rm -f "$KEEP"' EXIT
use() { cp "tools/ab/libscanpy_amd_$1.so" scanpy_amd/_lib/libscanpy_amd.so; }
case "$PART" in
cases)   # the case table of tests/eigensolver_cases.py: counters and hashes of every output
  for V in $A $B; do timeout -k 10 300 python tools/eigensolver_ab.py --gpu "tools/ab/libscanpy_amd_$V.so" > "$OUT/cases_$V.txt" || exit $?; done
  diff "$OUT/cases_$A.txt" "$OUT/cases_$B.txt" && echo "cases: $A and $B equal" ;;
dumps)   # bench.py --dump-outputs on the three structures: 13 files each, compared by sha256
  for ST in planted weak none; do for V in $A $B; do
    use $V; timeout -k 10 400 python bench.py --gpus 1 --steps 3 --warmup 1 --structure $ST --dump-outputs "$OUT/dump_${ST}_$V" | tail -1 > "$OUT/dump_${ST}_$V.json" || exit $?
    (cd "$OUT/dump_${ST}_$V" && sha256sum *) > "$OUT/dump_${ST}_$V.sha"; rm -r "$OUT/dump_${ST}_$V"
  done; diff "$OUT/dump_${ST}_$A.sha" "$OUT/dump_${ST}_$B.sha" && echo "dump $ST: $(wc -l < "$OUT/dump_${ST}_$A.sha") files, $A and $B equal" || exit 1; done ;;
speed)   # five alternations of the timed workload
  for I in 1 2 3 4 5; do for V in $A $B; do
    use $V; timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/speed_${V}_$I.json" || exit $?; echo "speed $V #$I done"
  done; done ;;
spectral)  # the "spectral init" line of tools/umap_profile.py
  for I in 1 2 3 4 5; do for V in $A $B; do
    use $V; timeout -k 10 300 python tools/umap_profile.py | grep "spectral init" > "$OUT/spectral_${V}_$I.txt" || exit $?; echo "spectral $V #$I: $(cat "$OUT/spectral_${V}_$I.txt")"
  done; done ;;
*) echo "unknown part $PART"; exit 2 ;;
esac
