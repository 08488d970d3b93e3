#!/bin/bash
# Timing-only variant libraries (wrong results) for A/B runs through AST_HIP_LIB:
#   bash scripts/build_variants.sh NAME "-DFLAG=1 ..." [source.hip]
# rebuilds SOURCE (default mb_ed4.hip; a csrc file name, or a path to another version of one, e.g.
# build_var/src_old/conv_x3.hip from git show) with the flags and links it with the other
# in-tree objects into build_var/libast_hip_NAME.so. Run `make -C arbitrarystyletransfer_amd/csrc` first.
# The 3x3 conv kernels are one file per family (conv_common.h lists them): the stamped build of the
# split-bf16 kernel is  stamp "-DX3_STAMP=1" conv_x3.hip,  of the collapsed upsampled one
# stamp_up2c "-DX3_STAMP=1" conv_up2c.hip  (one stamped file per library). X3_HS_PAD and X3_STAGED_EPI
# are conv_x3.hip's; X3_STAGED_EPI=0 also makes ast_conv3x3_dgrad_f32 (conv3x3_igemm.hip) refuse 24-27,
# which a variant of conv_x3.hip alone does not rebuild: forward timing only (or make FLAGS=... both).
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
NAME="$1"; FLAGS="$2"; SRCP="${3:-mb_ed4.hip}"
C="$ROOT/arbitrarystyletransfer_amd/csrc"; OUT="$ROOT/build_var"; mkdir -p "$OUT/$NAME"
case "$SRCP" in */*) ;; *) SRCP="$C/$SRCP" ;; esac
SRC="$(basename "$SRCP")"
extra=""; [ "$SRC" = mb_ed4.hip ] && extra="-fno-slp-vectorize"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I"$ROOT/include" -I"$C" $extra \
  -Xclang -target-feature -Xclang -packed-fp32-ops $FLAGS -c "$SRCP" -o "$OUT/$NAME/${SRC%.hip}.o" 2>&1 \
  | { grep -v "not a recognized feature" || true; }
objs=""
for o in "$C"/build/*.o; do
  b=$(basename "$o"); [ "$b" = "${SRC%.hip}.o" ] && o="$OUT/$NAME/$b"; [ "$b" = torch_ops.o ] && continue; objs="$objs $o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libast_hip_$NAME.so" $objs
echo "$OUT/libast_hip_$NAME.so"
