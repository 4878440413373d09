#!/bin/bash
# The light tracer's pass time (k_lt_photon) on cornell-box.bling: as its commented renderer line
# has it (light passPhotons 100000) and at 2 M photons.  One rocprofv3 kernel trace gives the
# kernel time; a run without the profiler gives photons/s and photon + shadow rays per second, with
# the CPU restatement's time for the same pass on 16 host cores beside it.
#   bash tools/gpu/light_time.sh OUTDIR      (a directory outside version control)
set -e -o pipefail
export TMPDIR=/tmp
O=${1:?usage: light_time.sh OUTDIR}; mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -o prof -- python3 tools/light_probe.py --config X5 --photons 2000000 --passes 3 > $O/trace.log 2>&1 &&
timeout -k 10 300 python3 tools/light_probe.py --config X5 --photons 100000 --passes 3 --ref-threads 16 > $O/p100k.log 2>&1 &&
timeout -k 10 300 python3 tools/light_probe.py --config X5 --photons 2000000 --passes 3 --ref-threads 16 > $O/p2m.log 2>&1 &&
echo light tracer timing done
