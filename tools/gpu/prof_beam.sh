set -o pipefail
R=${R:-r03}   # round tag of the output files
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
export OUT=${OUT:-out}; mkdir -p "$OUT"   # output directory (default: out/ in the repository)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_beam -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-concurrency --no-roofline > $OUT/prof_beam.json 2> $OUT/prof_beam.log || { tail -20 $OUT/prof_beam.log; exit 1; }
R=$R python3 - <<'PY'
import csv, glob, os
f=[x for x in glob.glob(os.environ["OUT"] + "/prof_beam/**/*kernel_stats.csv", recursive=True)]
rows=list(csv.DictReader(open(f[0])))
rows.sort(key=lambda r:-float(r["TotalDurationNs"]))
for r in rows[:60]:
    n=r["Name"]
    if "itts" in n:
        print(f'{float(r["TotalDurationNs"])/1e6:9.2f} ms n={r["Calls"]:>7} avg={float(r["AverageNs"])/1e3:8.2f} us  {n[:130]}')
PY
cp "$(find $OUT/prof_beam -name "*kernel_stats.csv" | head -1)" $OUT/${R}_beam_kernel_stats.csv
rm -rf $OUT/prof_beam   # the per-dispatch trace is > 64 MiB: only the stats summary is kept
echo ALLDONE
