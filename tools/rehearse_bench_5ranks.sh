out=${1:?usage: bash tools/rehearse_bench_5ranks.sh OUTDIR}; mkdir -p $out
BENCH_SHARE_GPU=1 BENCH_DIST_BACKEND=gloo timeout -k 10 700 python bench.py --gpus 5 --full --gb 0.2 --steps 1 --warmup 1 --cpu-seconds 0 > $out/bench_5ranks.json 2> $out/bench_5ranks.err
tail -c 300 $out/bench_5ranks.err
python - $out/bench_5ranks.json <<PY
import json, sys
d=json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
print(d["n_gpus"], d["value"], d["union_across_ranks"]["hashes"], d["union_across_ranks"]["union_ms"])
c=d["compare"]
for k in ("families","one_component","one_family"):
    v=c[k]; print(k, round(v["seconds"]*1e3,2), v["self_jaccard_is_1"], v["route"], {a:round(b,2) for a,b in v["rank0_phase_ms"].items()})
PY
