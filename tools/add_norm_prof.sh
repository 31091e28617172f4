#!/bin/bash
# MambaLayer(fused_add_norm=True) against the default, on the GPU: launches and GPU time of one layer forward + backward per stage
# shape of configs[1] (tools/layer_prof.py under rocprofv3 --kernel-trace --stats).  Flag off, on, off again: the two flag-off runs
# give the run-to-run spread the difference has to be read against.     bash tools/add_norm_prof.sh <report file>
set -e -o pipefail
root=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
report=$(realpath -m "${1:?report file}")
mkdir -p "$(dirname "$report")"
out=$(mktemp -d)                                  # traces and logs of the twelve runs; removed at the end
cd /tmp && export TMPDIR=/tmp
iters=10
for s in 0 1 2 3; do
  for run in off1:0 on:1 off2:0; do
    tag=${run%%:*}
    echo "stage $s, flag $tag"
    timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/addnorm_${s}_$tag" -o k -- \
        python3 "$root/tools/layer_prof.py" $s $iters ${run##*:} > "$out/addnorm_${s}_$tag.log" 2>&1 \
        || { tail -n 20 "$out/addnorm_${s}_$tag.log"; exit 1; }
  done
done
python3 - "$out" $((iters + 2)) > "$report" <<'PY'
import csv, glob, sys
out, n = sys.argv[1], int(sys.argv[2])
print("# tools/add_norm_prof.sh, MI355X: one MambaLayer forward + backward at the four stage shapes of BASELINE configs[1] (B 3, 5 frames, bf16")
print("# autocast), rocprofv3 --kernel-trace --stats, %d iterations per run; flag = MambaLayer(fused_add_norm=...); off twice: the spread." % n)
for s in range(4):
    res = {}
    for tag in ("off1", "on", "off2"):
        rows = list(csv.DictReader(open(glob.glob("%s/addnorm_%d_%s/**/*kernel_stats.csv" % (out, s, tag), recursive=True)[0])))
        res[tag] = (sum(int(r["Calls"]) for r in rows) / n, sum(float(r["TotalDurationNs"]) for r in rows) / n / 1e3, rows)
    off = (res["off1"][1] + res["off2"][1]) / 2
    print("== stage %d: launches per iteration off %.1f / on %.1f / off %.1f;  GPU us per layer fwd + bwd off %.1f / on %.1f / off %.1f"
          "  (on - mean off = %+.1f us, spread of off = %.1f us)"
          % (s, res["off1"][0], res["on"][0], res["off2"][0], res["off1"][1], res["on"][1], res["off2"][1], res["on"][1] - off,
             abs(res["off1"][1] - res["off2"][1])))
    names = {}
    for tag in ("off1", "on"):
        for r in res[tag][2]:
            names.setdefault(r["Name"], {})[tag] = (int(r["Calls"]) / n, float(r["TotalDurationNs"]) / n / 1e3)
    for name, d in sorted(names.items(), key=lambda kv: -abs(kv[1].get("on", (0, 0))[1] - kv[1].get("off1", (0, 0))[1]))[:10]:
        a, b = d.get("off1", (0, 0)), d.get("on", (0, 0))
        if a[0] != b[0]:
            print("   %-100s off x%-5.1f %7.1f us   on x%-5.1f %7.1f us" % (name[:100], a[0], a[1], b[0], b[1]))
PY
rm -rf "$out"
cat "$report"
