# schedule knobs of the hand-scheduled attention kernel: bitwise check + timing per configuration (DEFER NEXP_ODD WEIGHTED)
# RECORD (profiles/r03_attention_experiments.md, the variants table): needs the tree of commit 687900d (the last one whose generator
# read ATTN_ASM_* switches); on later sources the variables it sets select nothing and every configuration is the product kernel.
cd $GRAFT_REPO_ROOT
hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I opencv-simpleslam_amd/csrc scripts/ubench/attn_bench.hip -o /tmp/attn_b 2>/dev/null
for rep in 1 2; do
for cfg in "0 4 0" "0 4 1" "1 4 0" "1 4 1" "1 3 1" "1 5 1" "0 3 1" "0 5 1"; do
  set -- $cfg
  ATTN_ASM_DEFER=$1 ATTN_ASM_NEXP_ODD=$2 ATTN_ASM_WEIGHTED=$3 python3 opencv-simpleslam_amd/csrc/gen_lg_attention_asm.py > /tmp/a.s
  /opt/rocm/lib/llvm/bin/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=gfx950 -c /tmp/a.s -o /tmp/a.o && /opt/rocm/lib/llvm/bin/ld.lld -shared /tmp/a.o -o /tmp/a.hsaco || continue
  if [ $rep = 1 ]; then echo -n "[defer $1 nexp_odd $2 weighted $3] "; ATTN_HSACO=/tmp/a.hsaco ATTN_PP=4 ATTN_CMP=1 ATTN_CROSS=1 ATTN_N1=1333 timeout -k 5 60 /tmp/attn_b 1900 2 1 1 | grep bitwise; fi
  echo -n "[defer $1 nexp_odd $2 weighted $3] "; ATTN_HSACO=/tmp/a.hsaco ATTN_PP=4 timeout -k 5 120 /tmp/attn_b 2048 8 1 5
done
done
