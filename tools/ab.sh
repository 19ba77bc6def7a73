#!/bin/bash
# tools/ab.sh <libA> <libB> ...: bench.py with each engine build in turn (twice, alternating) on the same box; stops at the first run that fails
# AB_JSON_DIR=<dir>: keeps every run's JSON line there as <round>_<library>.json (ms_by_iteration and the rest of the line)
set -o pipefail
for round in 1 2; do
  for lib in "$@"; do
    j=$(MVS_ENGINE_LIB=$lib timeout -k 10 300 python bench.py --steps 3 --warmup 1 --cpu-seconds 0 --no-config5 --no-config4 2>/dev/null) || exit 1
    [ -n "$AB_JSON_DIR" ] && echo "$j" > "$AB_JSON_DIR/${round}_$(basename $(dirname $lib))_$(basename $lib .so).json"
    v=$(echo "$j" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('%.0f patches/s  %.1f ms/step  sweep %.1f ms  by iteration %s' % (d['value'], d['ms_per_step'], d['roofline']['sweep_ms']/d['steps'], ' '.join('%.1f' % x for x in d['ms_by_iteration'])))") || exit 1
    echo "$(basename $(dirname $lib))/$(basename $lib): $v"
  done
done
