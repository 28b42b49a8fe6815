#!/bin/bash
# Round-4 measurement bundle (GPU box, via gpurun): bench line, rocprofv3 kernel stats of the headline and of BASELINE configs
# [0], [2], [3], [4], the towers alone, PMC passes of the headline (HBM traffic: FETCH_SIZE / WRITE_SIZE in separate passes; SQ
# counters), config sweep, parity reports.    bash tools/r04_profile.sh [tag]   -> gpurun_out/<tag>/   (copy what is judged into profiles/)
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
TAG=${1:-r04}; O=gpurun_out/$TAG; mkdir -p $O
timeout 900 python bench.py --full --steps 40 --warmup 8 2>$O/bench.err | tail -1 > $O/bench_line.json
bash tools/r03_profile_headline.sh $TAG > /dev/null 2>&1
pmc() {   # name, bench args...
  local name=$1; shift
  timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/pf_$name -o p -- python bench.py --no-cpu-baseline --no-kernel-timing --no-trim-extra "$@" > /dev/null 2>&1
  timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/pw_$name -o p -- python bench.py --no-cpu-baseline --no-kernel-timing --no-trim-extra "$@" > /dev/null 2>&1
  python tools/traffic_from_pmc.py $(ls $O/pf_$name/*.db | head -1) $(ls $O/pw_$name/*.db | head -1) "$name: bench.py $*" > $O/gemm_hbm_traffic_$name.json
  timeout 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_BUSY_CYCLES --kernel-trace -d $O/ps_$name -o p -- python bench.py --no-cpu-baseline --no-kernel-timing --no-trim-extra "$@" > /dev/null 2>&1
  python tools/mfma_util.py $(ls $O/ps_$name/*.db | head -1) > $O/kernel_pmc_$name.md
  rm -rf $O/pf_$name $O/pw_$name $O/ps_$name
}
pmc headline --steps 3 --warmup 2
if [ "${FULL:-1}" = "1" ]; then
  bash tools/r03_profile_cfgs.sh $TAG > /dev/null 2>&1
  pmc cfg3 --method vpt --classes 1000 --steps 2 --warmup 1
  pmc cfg4 --method upt --classes 2191 --steps 2 --warmup 1
  pmc cfg5 --arch ViT-L/14@336px --method upt --classes 1151 --batch 128 --steps 2 --warmup 1
  bash tools/config_sweep.sh > $O/config_sweep.txt 2>&1
fi
python tools/parity_report.py fp16 2>&1 | grep -v amdgpu.ids > $O/parity_fp16.txt
python tools/inference_parity.py fp16 2>&1 | grep -v amdgpu.ids > $O/inference_parity.txt
ls -la $O
