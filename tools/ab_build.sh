#!/bin/bash
# Build libyouth_icp.so of a git revision into tools/ab/<name>/ so two versions
# can be timed in ONE call on one box (tools/ab_run.sh; devices differ by
# several % on this VALU-bound kernel: never compare across boxes).
# Usage: tools/ab_build.sh <name> <git-rev | file.hip>
#   <git-rev>   that revision's slam-rgbd_amd/ and include/, built by its own
#               Makefile: whatever units the library had then, it has here
#   <file.hip>  a copy of the working tree with this file in place of
#               csrc/icp_kernels.hip (tools/phase_patch.py ...)
# env HIPFLAGS_EXTRA: extra hipcc flags (-D knobs) for the kernel units, handed to
#   the tree's Makefile as a variable of that name; a revision whose Makefile
#   does not know it builds without them.
# env JOBS: make's -j (default 8, at most 16).
# Only icp_kernels.hip can be swapped: a variant of another unit (the old
# VIEWER_SRC) is built by committing it on a branch and naming that revision.
set -euo pipefail
NAME=$1; SRC=$2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/tools/ab/$NAME
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
rm -rf "$OUT/slam-rgbd_amd" "$OUT/include"
mkdir -p "$OUT"
if [ -f "$SRC" ]; then
    (cd "$ROOT" && git ls-files -z -co --exclude-standard slam-rgbd_amd include |
        tar -c --null -T - --ignore-failed-read) | tar -x -C "$OUT"
    cp "$SRC" "$OUT/slam-rgbd_amd/csrc/icp_kernels.hip"
else
    git -C "$ROOT" archive "$SRC" slam-rgbd_amd include | tar -x -C "$OUT"
fi
make -s -C "$OUT/slam-rgbd_amd" -j"${JOBS:-8}" HIPCC="$HIPCC" HIPFLAGS_EXTRA="${HIPFLAGS_EXTRA:-}" \
    libyouth_icp.so
cp "$OUT/slam-rgbd_amd/libyouth_icp.so" "$OUT/libyouth_icp.so"
echo "$OUT/libyouth_icp.so"
