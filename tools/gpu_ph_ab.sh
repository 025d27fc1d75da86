# GPU box: phase stamps (tools/mid_phases.py) of k_commit_step per library build
# hd-gnn_amd/csrc/ab_<tag>.so ("orig" = libhdgnn.so), two runs each, interleaved.
# Variants load through HDG_LIB_PATH; the in-tree libhdgnn.so is never overwritten.
set -o pipefail
mkdir -p gpurun_out/ph
for rep in 1 2; do
for tag in "$@"; do
  if [ $tag = orig ]; then LP=; else LP=$(pwd)/hd-gnn_amd/csrc/ab_$tag.so; fi
  HDG_LIB_PATH=$LP timeout -k 10 200 python tools/mid_phases.py > gpurun_out/ph/$tag.$rep.log 2>&1 || exit 1
  # the node chains and row reductions: M1/M2 (2->3), M12 reload + chain (17->19), M13 (19->20),
  # E2 from the end of wave 0's M13 tile (20->21), dV1 (14->15), M9 (10->12), and the median block
  L=$(echo */ph/$tag.$rep.log)
  echo "$tag $rep: $(awk '$1 == "phase" { sub(/-> +/, "->"); split($2, a, "->"); d[a[1] + 0] = $3 }
    END { printf "2->3 %.2f  17->19 %.2f  19->20 %.2f  20->21 %.2f  14->15 %.2f  10->12 %.2f", d[2], d[17] + d[18], d[19], d[20], d[14], d[10] + d[11] }' $L)  total $(grep 'total' $L | awk '{print $4}')"
done
done
