#!/bin/bash
# Build vyomai_amd/lib/libvyom_hip_ab.so with one or more source files taken from another git revision, for
# same-box A/B timing (devices differ by several percent):  tools/ab_lib.sh <rev> <file.hip> [<file.hip> ...]
# then on the box:  VY_LIB_PATH=$PWD/vyomai_amd/lib/libvyom_hip_ab.so python bench.py ...
# vy_common.h comes from the revision too, every other header from the tree.
set -e
rev=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
mkdir -p $tmp/vyomai_amd/csrc $tmp/include
cp $root/vyomai_amd/csrc/*.h $tmp/vyomai_amd/csrc/
cp $root/include/vyom_hip.h $tmp/include/
git -C $root show $rev:vyomai_amd/csrc/vy_common.h > $tmp/vyomai_amd/csrc/vy_common.h
swapped=""
for f in "$@"; do
  git -C $root show $rev:vyomai_amd/csrc/$f > $tmp/vyomai_amd/csrc/$f
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c $tmp/vyomai_amd/csrc/$f -o $tmp/${f%.hip}.o &
  swapped="$swapped ${f%.hip}.o"
done
wait
objs=""
for o in $root/vyomai_amd/lib/*.o; do
  case " $swapped " in
    *" $(basename $o) "*) objs="$objs $tmp/$(basename $o)" ;;
    *) objs="$objs $o" ;;
  esac
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $root/vyomai_amd/lib/libvyom_hip_ab.so $objs -ldl
rm -rf $tmp
echo built $root/vyomai_amd/lib/libvyom_hip_ab.so
