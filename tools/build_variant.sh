#!/bin/bash
# A/B variant of the batched pipeline kernels (diagnostics, tools/ab.py): the Makefile's
# `variant` target, so the shipped flags and the product's object list. Compiles the
# kernels_w4_t8 unit (the 512-wide policies' and GRU-256's instantiations; UNITS="t2 t4 t8"
# for more; SRC=<another checkout>/go2_onnx_controller_amd/csrc for a parent commit's kernels)
# with the extra compiler flags / defines into lib/diag/libgo2pi_<name>.so.
#   tools/build_variant.sh nopre -DGO2PI_SOME_SWITCH=1
set -e
name=$1
shift
exec make -C "$(dirname "$0")/../go2_onnx_controller_amd/csrc" -j4 variant NAME="$name" EXTRA="$*" \
  ${UNITS:+UNITS="$UNITS"} ${SRC:+SRC="$SRC"}
