#!/bin/bash
# tools/ab.sh libA.so libB.so ... -- on the GPU box: kernel time of in-tree builds, same inputs (default shape and NW=8 at B=768, B=256)
# A run that fails (or runs into its time limit) ends the script with its status and the end of its output: nothing more is started.
for lib in "$@"; do
  for cfg in "1024:" "768:8" "256:8"; do
    b=${cfg%%:*}; nw=${cfg##*:}
    log=$(KBEST_LIB=$lib KBEST_NWAVES=$nw timeout -k 10 200 python bench.py --steps 10 --warmup 2 --batch $b --no-cpu 2>&1)
    rc=$?
    if [ $rc -ne 0 ]; then echo "tools/ab.sh: $lib B=$b NW=${nw:-auto}: bench.py ended with status $rc" >&2; echo "$log" | tail -8 >&2; exit $rc; fi
    r=$(echo "$log" | grep '^{' | tail -1 | python3 -c "import sys,json; j=json.loads(sys.stdin.read()); print('%.3f ms' % j['kernel_ms'])") || exit 1
    echo "$lib B=$b NW=${nw:-auto}: $r"
  done
done
