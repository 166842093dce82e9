#!/bin/bash
# A/B of the headline kernel's layer 1: the hybrid form (csrc/nplda_fwd_v6h.h) at each S1 of $S1S (default "2 3 4":
# NPLDA_FWD_V6_L1S) against NPLDA_FWD_V6_L1=f32 (csrc/nplda_fwd_v6.h), in alternating fresh processes, REPS runs each:
# v6_l1_ab.sh [REPS] [extra bench.py arguments].  One line per run; with --full the line carries the shader clock.
R=$(cd "$(dirname "$0")/.." && pwd); REPS=${1:-3}; shift
for rep in $(seq "$REPS"); do for form in f32 ${S1S:-2 3 4}; do
  unset NPLDA_FWD_V6_L1 NPLDA_FWD_V6_L1S
  if [ "$form" = f32 ]; then export NPLDA_FWD_V6_L1=f32; else export NPLDA_FWD_V6_L1S=$form; fi
  line=$(timeout -k 10 300 python "$R/bench.py" --no-cpu-baseline "$@" | grep '^{') || { echo "rep $rep $form: bench.py failed"; exit 1; }
  echo "$line" | python -c "import json,sys; d=json.loads(sys.stdin.readline()); r=d['roofline']
print('rep $rep L1 %-3s ms_per_step %.4f  pairs/s %.4g  kernel_ms %.4f  frac %.4f  sclk %s  %s' % ('$form', d['ms_per_step'], d['value'],
      r['kernel_ms'], r['frac'], r.get('sclk_mhz_under_kernel'), r['kernel'][33:95]))"
done; done
unset NPLDA_FWD_V6_L1 NPLDA_FWD_V6_L1S
