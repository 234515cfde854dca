# the whole -m gpu suite + the driver's bench line with every side figure (--full), into $OUT (default: out/)
TAG=${TAG:-r03}
OUT=${OUT:-out}
mkdir -p $OUT
python -m pytest tests -q -m gpu -x 2>&1 | tail -8 > $OUT/${TAG}_gputests.txt
cat $OUT/${TAG}_gputests.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${TAG}_bench_driver.json 2> $OUT/${TAG}_bench_driver.err
python - <<PY
import json
d=json.load(open("$OUT/${TAG}_bench_driver.json"))
print({k:d[k] for k in ("value","ms_per_step","host_resident_events","float_order_lk","repeats")})
print(d["roofline"]); print(d["cpu_baseline"]["value"], d["cpu_baseline"].get("all_cores"))
PY
