#!/bin/bash
# Build libolpe.so of a git revision into diag/<name>/ for same-box A/B runs
# (tools/ab_libs.sh <name>, or OLPE_LIB=diag/<name>/libolpe.so).
# usage: tools/build_rev.sh <rev> <name> [extra hipcc flags]
set -e
rev=$1; name=$2; shift 2
tmp=$(mktemp -d)
trap 'rm -rf $tmp' EXIT
mkdir -p $tmp/olpefit_amd/csrc $tmp/include
for f in $(git ls-tree --name-only -r $rev olpefit_amd/csrc include); do git show $rev:$f > $tmp/$f; done
mkdir -p diag/$name
# the revision's sources: every HIP unit it has, and olpe_csv.cpp from its introduction on
srcs=$(ls $tmp/olpefit_amd/csrc/*.hip)
[ -f $tmp/olpefit_amd/csrc/olpe_csv.cpp ] && srcs="$srcs $tmp/olpefit_amd/csrc/olpe_csv.cpp"
/opt/rocm/bin/hipcc $(python -m olpefit_amd.build --print-flags) "$@" \
  -o diag/$name/libolpe.so $srcs -lrccl
