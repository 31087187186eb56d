#!/bin/bash
# timing-only variants of fthe_padic_m37 for the standalone harness (tools/bin/m37_<variant>.hsaco); a variant is
# [body,]switches: "base" is the default schedule of fthe_padic_m37, "t" the four-tile body fthe_padic_m37t, "s"
# fthe_padic_m37s (the four-tile body on product 1's shifted operand), "l" fthe_padic_m37l (on the limb-fed
# operand) and "k" fthe_padic_m37k (m37l with MUL's cross term by Karatsuba);
# switches (gen_padic_mfma.py SWITCHES, for k also K_SWITCHES) follow a body's letter after a comma, or stand alone
# for m37:   M37_AB="base t s l l,noclampbr k k,nomulkara k,fill0 nokara" bash tools/build_m37_ab.sh
set -e
mkdir -p tools/bin
L=/opt/rocm/lib/llvm/bin
for v in ${M37_AB:-noswap nonop nomfma noswap,nonop}; do
  n=${v//,/_}
  case $v in
    base) body=m37 ab= ;;
    t|s|l|k) body=m37$v ab= ;;
    t,*|s,*|l,*|k,*) body=m37${v%%,*} ab=${v#?,} ;;   # e.g. l,clampbr -> m37_l_clampbr.hsaco
    *) body=m37 ab=$v ;;
  esac
  python3 fedtree_amd/csrc/gen_padic_mfma.py --body $body --ab "$ab" -o /tmp/m37_$n.s
  $L/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=gfx950 -c /tmp/m37_$n.s -o /tmp/m37_$n.o
  $L/ld.lld -shared /tmp/m37_$n.o -o tools/bin/m37_$n.hsaco
done
