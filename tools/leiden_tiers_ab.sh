#!/bin/bash
# A/B of two BUILDS of the library on one box, for a change to the decide tiers of csrc/leiden.hip that must compute the same:
#   tools/leiden_tiers_ab.sh <part> <variant> <variant>   (tools/ab/libscanpy_amd_<variant>.so; parts: profile dumps speed leiden)
# Every run is a fresh process under its own time limit; the first failure ends the script.  Raw lines go to $OUT (build/ab).
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"; cd "$R"
PART="$1"; A="$2"; B="$3"; OUT="${OUT:-build/ab}"; mkdir -p "$OUT"; OUT="$(cd "$OUT" && pwd)"
KEEP="$(mktemp)"; cp scanpy_amd/_lib/libscanpy_amd.so "$KEEP"
trap 'cp "$KEEP" scanpy_amd/_lib/libscanpy_amd.so; rm -f "$KEEP"' EXIT
use() { cp "tools/ab/libscanpy_amd_$1.so" scanpy_amd/_lib/libscanpy_amd.so; }
case "$PART" in
profile)  # per-kernel table of the timed workload (3 steps after 1 warm-up: 4 passes), the Leiden kernels' rows
  for V in $A $B; do
    use $V; D="$(mktemp -d)"
    timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$D" -o bench -- python bench.py --gpus 1 --steps 3 --warmup 1 > "$OUT/profile_$V.log" 2>&1 < /dev/null || exit $?
    cp "$(find "$D" -name 'bench_kernel_stats.csv' | head -1)" "$OUT/profile_${V}_kernel_stats.csv" || exit $?
    rm -r "$D"; echo "== $V"; grep -E '^"Name"|ld_(move|requeue|refine_propose|apply|compact_cls|refine_candidates)' "$OUT/profile_${V}_kernel_stats.csv" | sed -E 's/^"[^"]*(ld_[a-z_]+(<[0-9]+>)?)[^"]*"/"\1"/' | cut -d, -f1-5
  done ;;
dumps)    # bench.py --dump-outputs on the three structures, compared by sha256; labels_sha of the result lines
  for ST in planted weak none; do for V in $A $B; do
    use $V; timeout -k 10 400 python bench.py --gpus 1 --steps 3 --warmup 1 --structure $ST --dump-outputs "$OUT/dump_${ST}_$V" | tail -1 > "$OUT/dump_${ST}_$V.json" || exit $?
    (cd "$OUT/dump_${ST}_$V" && sha256sum *) > "$OUT/dump_${ST}_$V.sha"; rm -r "$OUT/dump_${ST}_$V"
    echo "$ST $V labels_sha $(grep -o '"labels_sha": *"[0-9a-f]*"' "$OUT/dump_${ST}_$V.json" | head -1)"
  done; diff "$OUT/dump_${ST}_$A.sha" "$OUT/dump_${ST}_$B.sha" && echo "dump $ST: $(wc -l < "$OUT/dump_${ST}_$A.sha") files, $A and $B equal" || exit 1; done ;;
speed)    # five alternations of the timed workload
  for I in 1 2 3 4 5; do for V in $A $B; do
    use $V; timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$OUT/speed_${V}_$I.json" || exit $?
    echo "speed $V #$I: $(python -c "import json,sys; r=json.load(open(sys.argv[1])); print('ms_per_step', r['ms_per_step'], 'leiden', r['stage_ms_per_step']['leiden'])" "$OUT/speed_${V}_$I.json")"
  done; done ;;
leiden)   # Leiden alone at 1M cells, ${REPS:-5} alternations per structure; the line carries the launch and round-trip counts
  for ST in ${STRUCTS:-planted weak none}; do for I in $(seq 1 ${REPS:-5}); do for V in $A $B; do
    use $V; timeout -k 10 300 python tools/leiden_only.py 1000000 $ST 3 2>&1 | grep "leiden n=" > "$OUT/leiden_${ST}_${V}_$I.txt" || exit $?
    echo "$V #$I $(cut -c1-400 "$OUT/leiden_${ST}_${V}_$I.txt")"
  done; done; done ;;
*) echo "unknown part $PART"; exit 2 ;;
esac
