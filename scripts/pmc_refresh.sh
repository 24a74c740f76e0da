set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=/root/repo/gpurun_out/pmcfinal
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 900 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c -- python "$ROOT/bench.py" --steps 6 --warmup 3 --full --no-cpu-baseline --no-roofline --no-graph > $OUT/pmc_$c.log 2>&1
done
cd /root/repo
{ python scripts/pmc_summary.py $OUT/pmc_FETCH_SIZE 25; python scripts/pmc_summary.py $OUT/pmc_WRITE_SIZE 25; } > $OUT/pmc_step_summary.txt
python - <<'PY'
import csv, glob, json
out = '/root/repo/gpurun_out/pmcfinal'
def fam_avg(d, counter):
    n = s = 0
    for f in glob.glob(d + '/**/*counter_collection.csv', recursive=True):
        for r in csv.DictReader(open(f)):
            if ('gemm2_' in r['Kernel_Name'] or 'gemm_nt_kernel' in r['Kernel_Name']) and r['Counter_Name'] == counter:
                n += 1; s += float(r['Counter_Value'])
    return n, (s / n if n else None)
nf, f = fam_avg(out + '/pmc_FETCH_SIZE', 'FETCH_SIZE')
nw, w = fam_avg(out + '/pmc_WRITE_SIZE', 'WRITE_SIZE')
json.dump({'kernel': 'gemm2_kernel + gemm2_group_kernel + gemm_nt_kernel', 'launches_counted': nf,
           'fetch_kb_per_launch_reported': f, 'write_kb_per_launch_reported': w,
           'read_bytes_per_launch': f * 1024 * 2, 'write_bytes_per_launch': w * 1024,
           'traffic_bytes_per_launch': f * 1024 * 2 + w * 1024,
           'corrections': 'FETCH_SIZE (KB) doubled: gfx950 rocprofv3 tallies 128-B requests at 64 B for 16-B/lane reads (MI355X_MICROARCH.md, HBM); '
                          'WRITE_SIZE (KB) x1, calibrated on act_bwd (23,307 KB reported for a 23,040 KB store). FETCH_SIZE counts L2-miss requests on the '
                          'fabric side, Infinity-Cache hits included: an upper bound on HBM bytes.',
           'command': 'rocprofv3 --pmc <FETCH_SIZE|WRITE_SIZE> --kernel-trace -- python bench.py --steps 6 --warmup 3 --no-graph (two separate passes)'},
          open(out + '/pmc_gemm_traffic.json', 'w'), indent=1)
PY
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE
cat $OUT/pmc_gemm_traffic.json | head -8
