# Kernel trace of the N > 1 code path with a 1-rank RCCL group (bench.py --force-dist).
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
: "${OUT:?set OUT to the directory for the logs}"
export OUT
rm -rf "$OUT/proffd"; mkdir -p "$OUT/proffd"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/proffd" -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --force-dist > "$OUT/proffd/bench.log" 2>&1
echo rc=$?
python3 - <<'PY'
import csv,glob,json,os
out=os.environ['OUT']+'/proffd'
f=sorted(glob.glob(out+'/*/*_kernel_stats.csv'))[-1]
for r in csv.DictReader(open(f)):
    if float(r['Percentage'])>0.5: print(r['Name'][:70].ljust(71), r['Calls'], 'avg_ms=%.3f'%(float(r['AverageNs'])/1e6), r['Percentage'])
for l in open(out+'/bench.log'):
    if l.startswith('{'):
        d=json.loads(l); print('value G/s', round(d['value']/1e9,2), 'ms/step', round(d['ms_per_step'],2), d['config']['check'])
PY
