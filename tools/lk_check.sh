# LK parity in both modes, the per-level / per-iteration constants, three cold bench runs
OUT=${OUT:-out}; mkdir -p $OUT
timeout 900 python -m pytest tests/test_parity_gpu.py tests/test_lk_float_order_gpu.py -m gpu -x -q -k "lk or end_to_end or float" 2>&1 | tail -3; ESVIO_LK_ACCUM=1 timeout 600 python -m pytest tests/test_parity_gpu.py -m gpu -x -q -k "lk or end_to_end" 2>&1 | tail -2; python tools/lk_const_probe.py 2 2>&1 | tail -1; python tools/lk_const_probe.py 1 2>&1 | tail -1; for i in 1 2 3; do timeout 300 python bench.py --full --steps 20 --warmup 5 --cpu-frames 0 --no-host-pass --no-sae-pass > $OUT/lk_bench_$i.json 2>/dev/null; python -c "
import json,sys
d=json.load(open(sys.argv[1])); print(d[\"ms_per_step\"], d[\"repeats\"][\"ms_per_step\"], (d.get(\"exact_sum_lk\") or {}).get(\"ms_per_step\"))" $OUT/lk_bench_$i.json; done
