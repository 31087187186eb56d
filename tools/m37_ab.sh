#!/bin/bash
# A/B/... of fthe_padic_m37 code objects in the standalone harness (tools/bin/test_padic, checked against
# GMP on sampled lanes), round-robin over the variants three times; stops at the first failure.
#   bash tools/m37_ab.sh TAG V1 V2 [V3 ...]     (tools/bin/m37_V.hsaco; lanes: M37_LANES, default 393216)
# A variant named t or t_* holds the four-tile body fthe_padic_m37t (gen_padic_mfma.py --body m37t), so
#   bash tools/m37_ab.sh TAG base t     runs m37 and m37t round-robin in one series.
# A variant named s or s_* holds fthe_padic_m37s (--body m37s) and reads the shifted tile image:
#   bash tools/m37_ab.sh TAG t s
# A variant named l or l_* holds fthe_padic_m37l (--body m37l) and reads the limb-fed tile image:
#   bash tools/m37_ab.sh TAG s l
# A variant named k or k_* holds fthe_padic_m37k (--body m37k) and reads the same image:
#   bash tools/m37_ab.sh TAG l k k_nomulkara k_fill0
T=${1:?tag}; shift
N=${M37_LANES:-393216}
mkdir -p gpurun_out
for r in 1 2 3; do
  for v in "$@"; do
    # variants named pp* are ping-pong schedules (512-thread workgroups)
    blk=256; [[ $v == pp* ]] && blk=512
    # variants generated with s1lo112 read the tile image of the window that starts at column 112
    export M37_S1LO=128; [[ $v == *s1lo112* ]] && export M37_S1LO=112
    # the harness looks up M37_KERNEL, when set, in place of the kernel named on its command line
    unset M37_KERNEL; [[ $v == t || $v == t_* ]] && export M37_KERNEL=fthe_padic_m37t
    export M37_QSHIFT=0; [[ $v == s || $v == s_* ]] && export M37_KERNEL=fthe_padic_m37s M37_QSHIFT=8
    export M37_LIMB=0; [[ $v == l || $v == l_* ]] && export M37_KERNEL=fthe_padic_m37l M37_LIMB=1
    [[ $v == k || $v == k_* ]] && export M37_KERNEL=fthe_padic_m37k M37_LIMB=1
    M37_BLOCK=$blk timeout -k 10 120 tools/bin/test_padic tools/bin/m37_$v.hsaco $N 0 fthe_padic_m37 > gpurun_out/${T}_one.json
    rc=$?
    # timing-only variants (nomfma, noswap, nonop: wrong results by design) may report bad lanes (rc 1)
    if [ $rc -ne 0 ] && ! { [ $rc -eq 1 ] && [[ $v == nomfma* || $v == noswap* || $v == nonop* ]]; }; then
      echo "m37 $v failed (rc $rc)"; cat gpurun_out/${T}_one.json; exit 1
    fi
    echo "{\"variant\": \"$v\", \"run\": $r, \"res\": $(tail -1 gpurun_out/${T}_one.json)}" >> gpurun_out/${T}_m37ab.jsonl
  done
done
cat gpurun_out/${T}_m37ab.jsonl
