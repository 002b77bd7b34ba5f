#!/bin/bash
# round 6: VGG16 per-dispatch SQ counter table.  (Its first part, the LDS-window bound of r06_conv_window_bound.txt, needed the
# A/B build and went with it; see profiles/README.md.)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=gpurun_out
for i in 1 2; do
  [ $i = 1 ] && C="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES"
  [ $i = 2 ] && C="SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INST_LEVEL_VMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU SQ_WAIT_ANY"
  rm -rf $out/pmcv_$i
  timeout 300 rocprofv3 --kernel-trace --pmc $C --kernel-include-regex 'conv_igemm|cam_head_kernel' -d $out/pmcv_$i -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-pipeline --quick --workload cam --arch vgg16 --batch 16 > $out/r06_pmcv_$i.log 2>&1
done
{ echo "# rocprofv3 --kernel-trace --pmc <SQ set 1 | SQ set 2> --kernel-include-regex 'conv_igemm|cam_head_kernel' -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-pipeline --quick --workload cam --arch vgg16 --batch 16   (VGG16-CAM, 32 samples at 321^2, f16x3: one forward pass)"
  python profiles/conv_pmc_generic.py $out/pmcv_1/*/*_results.db $out/pmcv_2/*/*_results.db 40; } > $out/r06_pmc_conv_vgg16.txt 2>&1
rm -rf $out/pmcv_1 $out/pmcv_2
tail -45 $out/r06_pmc_conv_vgg16.txt
