#!/bin/bash
# A/B of the headline kernel's layer 2 (csrc/nplda_fwd_v6.h): the split form (default) against NPLDA_FWD_V6_L2=f32, in
# alternating fresh processes, REPS runs each: v6_l2_ab.sh [REPS] [extra bench.py arguments].  One line per run.
R=$(cd "$(dirname "$0")/.." && pwd); REPS=${1:-3}; shift
for rep in $(seq "$REPS"); do for form in split f32; do
  if [ "$form" = f32 ]; then export NPLDA_FWD_V6_L2=f32; else unset NPLDA_FWD_V6_L2; fi
  line=$(timeout -k 10 300 python "$R/bench.py" --no-cpu-baseline "$@" | grep '^{') || { echo "rep $rep $form: bench.py failed"; exit 1; }
  echo "$line" | python -c "import json,sys; d=json.loads(sys.stdin.readline()); r=d['roofline']
print('rep $rep %-5s ms_per_step %.4f  pairs/s %.4g  kernel_ms %.4f  frac %.4f  sclk %s' % ('$form', d['ms_per_step'], d['value'],
      r['kernel_ms'], r['frac'], r.get('sclk_mhz_under_kernel')))"
done; done
unset NPLDA_FWD_V6_L2
