#!/bin/bash
# usage: [MODELS="0 1"] tools/build_variant.sh <name> [extra hipcc flags]  -> mcsas_amd/lib/libmcsas_<name>.so from the CURRENT sources of the host
# translation units (mcsas_hip.hip, host_decide.hip, host_plugin.hip, host_calls.hip, host_hist.hip, host_analyse.hip, host_rows.hip) and the pipeline kernels (kern_pipe.hip: chain_pipe.h and the pipe_*.h under it) of the models in MODELS (default: the sphere; the other objects are taken from build/csrc:
# run `make release` first)
set -e
cd $(dirname $0)/../mcsas_amd/csrc
name=$1; shift
B=../../build/csrc; V=../../build/variant_$name; mkdir -p $V
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-value -I$B $*"
make --no-print-directory $B/embedded_headers.inc
HOST="mcsas_hip host_decide host_plugin host_calls host_hist host_analyse host_rows"
for u in $HOST; do /opt/rocm/bin/hipcc $F -c -o $V/$u.o $u.hip & done
MODELS=${MODELS:-0}
for m in $MODELS; do /opt/rocm/bin/hipcc $F -DMCSAS_M=$m -c -o $V/kern_pipe_m$m.o kern_pipe.hip & done
wait
# the release library's object list (Makefile: print-objs), with the objects compiled above in place of the release ones
objs=""
for o in $(make --no-print-directory print-objs BUILD=$B); do
  if [ -e $V/$(basename $o) ]; then objs="$objs $V/$(basename $o)"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../lib/libmcsas_$name.so $objs -lhiprtc
ls -la ../lib/libmcsas_$name.so
