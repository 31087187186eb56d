#!/bin/bash
# timing-only variants of fthe_padic_m37 for the standalone harness (tools/bin/m37_<variant>.hsaco); the variant
# "base" is the default schedule, "t" the four-tile body fthe_padic_m37t, "s" fthe_padic_m37s (the four-tile body
# on product 1's shifted operand) and "l" fthe_padic_m37l (on the limb-fed operand):
#   M37_AB="base t s l" bash tools/build_m37_ab.sh
set -e
L=/opt/rocm/lib/llvm/bin
for v in ${M37_AB:-noswap nonop nomfma noswap,nonop}; do
  n=${v//,/_}; n=${n/pingpong/pp}
  if [ "$v" = t ]; then      # the four-tile body, run as fthe_padic_m37t (m37_ab.sh); base: M37_AB="base t" with base = ""
    python3 fedtree_amd/csrc/gen_padic_mfma.py --name fthe_padic_m37t --top-est -o /tmp/m37_$n.s
  elif [ "$v" = s ]; then
    python3 fedtree_amd/csrc/gen_padic_mfma.py --name fthe_padic_m37s --top-est --q1-shift 8 -o /tmp/m37_$n.s
  elif [ "$v" = l ]; then
    python3 fedtree_amd/csrc/gen_padic_mfma.py --name fthe_padic_m37l --top-est --limb-op -o /tmp/m37_$n.s
  elif [[ $v == l,* ]]; then     # fthe_padic_m37l under generator switches, e.g. l,clampbr -> m37_l_clampbr.hsaco
    FTHE_GEN_M37_AB=${v#l,} python3 fedtree_amd/csrc/gen_padic_mfma.py --name fthe_padic_m37l --top-est --limb-op -o /tmp/m37_$n.s
  else
    FTHE_GEN_M37_AB=${v/#base/} python3 fedtree_amd/csrc/gen_padic_mfma.py -o /tmp/m37_$n.s
  fi
  $L/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=gfx950 -c /tmp/m37_$n.s -o /tmp/m37_$n.o
  $L/ld.lld -shared /tmp/m37_$n.o -o tools/bin/m37_$n.hsaco
done
