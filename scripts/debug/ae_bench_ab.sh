J=$(mktemp)
for i in 1 2; do
  for t in build_var/head .; do
    (cd $t && timeout -k 10 200 python3 bench.py --full --mode ae-train --cpu-seconds 0 > $J 2>/dev/null; python3 -c "import json;d=json.load(open('$J'));print('$t', round(d['value'],1), round(d['ms_per_step'],2), d.get('kernels_ms_per_step'))")
  done
done
rm -f $J
