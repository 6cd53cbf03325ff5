# A/B of two builds of this repository on the bench workload, alternating:
#   tools/ab_builds.sh OUTDIR OTHER_TREE ROUNDS [bench args]
# OTHER_TREE is a built checkout of the commit to compare with (its own bench.py and library).
# Every run is a process of its own under its own time limit; the first failure ends the script.
# One JSON line per run in OUTDIR/{other,this}_<round>.jsonl, the values echoed as they come.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
O=$1; OTHER=$(cd "$2" && pwd); N=$3
shift 3
mkdir -p "$O"
O=$(cd "$O" && pwd)
for r in $(seq 1 "$N"); do
  for v in other this; do
    if [ $v = other ]; then D=$OTHER; else D=$ROOT; fi
    ( cd "$D" && timeout -k 10 150 python -u bench.py "$@" > "$O/${v}_$r.jsonl" 2> "$O/${v}_$r.err" ) || { echo "FAILED $v $r"; tail -5 "$O/${v}_$r.err"; exit 1; }
    echo "$v $r $(python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['value'], d['unit'], d['config']['fallbacks'], d['config']['pipeline'])" "$O/${v}_$r.jsonl")"
  done
done
