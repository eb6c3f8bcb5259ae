#!/bin/bash
# Where K1's time goes: knock-in / knock-out builds of the lane-per-state kernel, each timed on the
# bench batch (tools/scene_bench.py).  A phase that runs twice costs its own time once more; a phase left out shows what
# is left.  Run the build part in the build container, the timing part on the GPU box:
#   bash tools/k1_knock.sh build ; gpurun -- 'bash tools/k1_knock.sh time'
set -e
cd "$(dirname "$0")/.."
SRC=mopa_rl_amd/csrc
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -mfma -Wno-unused-function"
# (noresident: the baked kernel without its resident pairs; noresident_nodrain next to nodrain: what the resident pairs take out
#  of the drain phase.  noaxis: the baked pass A with the bounding-radius constants for every static pair, no axis table;
#  noaxis_nodrain next to nodrain: what the axis extents take out of the drain phase.  nosparse: the baked walk in its dense form only,
#  no guard; nosparse_fk2 next to fk2: what the sparse form takes out of the walk.  onetile: every scene drains tile by tile (no pair
#  drain); onetile_nodrain next to nodrain, and onetile next to the baseline: what the pair drain takes out of the drain phase, apart
#  from what pulling two tiles at once does to the rest.  flatslab: the baked walk's pose stores and the cold walk's loads through
#  generic pointers (FLAT instructions) again.  fullstage: a baked scene stages the whole scene blob and pair table again.
#  timeline: not a knock-out -- the library tools/k1_wave_timeline.py needs (every wave stamps the clock where its life changes
#  phase).  K1_KNOCK_VARIANTS="a b": only these)
VARIANTS="fk2:-DMOPA_V5_FK_REPS=2 cull2:-DMOPA_V5_CULL_REPS=2 nodrain:-DMOPA_V5_KO_DRAIN nopassb:-DMOPA_V5_KO_DRAIN,-DMOPA_V5_KO_PASSB noresident:-DMOPA_V5_NO_RESIDENT noresident_nodrain:-DMOPA_V5_NO_RESIDENT,-DMOPA_V5_KO_DRAIN noaxis:-DMOPA_V5_NO_AXIS_CULL noaxis_nodrain:-DMOPA_V5_NO_AXIS_CULL,-DMOPA_V5_KO_DRAIN nosparse:-DMOPA_V5_NO_SPARSE_FK nosparse_fk2:-DMOPA_V5_NO_SPARSE_FK,-DMOPA_V5_FK_REPS=2 onetile:-DMOPA_V5_TILES_PER_DRAIN=1 onetile_nodrain:-DMOPA_V5_TILES_PER_DRAIN=1,-DMOPA_V5_KO_DRAIN flatslab:-DMOPA_V5_FLAT_SLAB fullstage:-DMOPA_V5_FULL_STAGING timeline:-DMOPA_V5_TIMELINE"
if [ -n "$K1_KNOCK_VARIANTS" ]; then
    VARIANTS=$(for v in $VARIANTS; do for w in $K1_KNOCK_VARIANTS; do if [ "${v%%:*}" = "$w" ]; then echo "$v"; fi; done; done)
fi
if [ "$1" = build ]; then
    for v in $VARIANTS; do
        /opt/rocm/bin/hipcc $FLAGS $(echo ${v#*:} | tr , ' ') -c -o /tmp/mopa_knock_${v%%:*}.o $SRC/mopa_hip.hip
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $SRC/libmopa_knock_${v%%:*}.so /tmp/mopa_knock_${v%%:*}.o $SRC/mopa_envdyn.o   # (the env / dynamics TU as built by make)
    done
else
    PAT=${2:-SawyerPush}
    echo "baseline:"; python tools/scene_bench.py 2>&1 | grep -E "$PAT"
    for v in $VARIANTS; do
        echo "${v%%:*}:"; MOPA_HIP_LIB=$PWD/$SRC/libmopa_knock_${v%%:*}.so python tools/scene_bench.py 2>&1 | grep -E "$PAT"
    done
fi
