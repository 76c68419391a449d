#!/bin/bash
# Build libsrs_amd.so from a git revision's sources into
# simd-radix-sort_amd/lib/variants/<name>/ (A/B timing against the work tree).
# Takes every csrc/*.hip and csrc/*.h the revision has, so it builds
# revisions from before and after a unit was split off.
# usage: tools/build_rev_variant.sh <name> <rev> [extra hipcc flags]
set -e
cd "$(dirname "$0")/.."
name=$1; rev=$2; shift 2
src=$(mktemp -d)
mkdir -p $src/include $src/pkg/csrc
units=()
for p in $(git ls-tree --name-only $rev simd-radix-sort_amd/csrc/); do
  f=$(basename $p)
  case $f in
    *.hip) units+=(${f%.hip}) ;;
    *.h) ;;
    *) continue ;;
  esac
  git show $rev:$p > $src/pkg/csrc/$f
done
git show $rev:include/srs_c_api.h > $src/include/srs_c_api.h
out=simd-radix-sort_amd/lib/variants/$name; mkdir -p $out
pids=()
for f in "${units[@]}"; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics "$@" \
    -c $src/pkg/csrc/$f.hip -o $src/$f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p || { echo "FAILED $name"; exit 1; }; done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $out/libsrs_amd.so $src/*.o -ldl \
  -Wl,-rpath,/opt/rocm/lib
rm -rf $src
echo "built $name from $rev"
