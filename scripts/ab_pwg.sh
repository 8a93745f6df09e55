export COBEL_DEBUG=1
OUT=${OUT:-build/ab}
mkdir -p "$OUT"
run() { # name, env..., args
  name=$1; shift
  env "$@" timeout -k 10 200 python bench.py --full --print-full --also "" --min-seconds 0 --no-cpu-baseline $ARGS > "$OUT/$name.json" 2> "$OUT/$name.err" || { echo FAIL $name; tail -5 "$OUT/$name.err"; exit 1; }
  python -c "
import json,sys
r=json.load(open('$OUT/$name.json'))
print('$name', '%.4g'%r['value'], r['roofline']['launch_ms_all'])"
}
