#!/bin/bash
# Experiment helper: build the product library with extra -D flags into yart_amd/_variants/NAME.so
# (git-ignored; travels to the GPU box). Usage: tools/build_variant.sh NAME "-DFOO=1 ..."
# Drives csrc/Makefile (its flags, its five translation units, in parallel) with the extra flags, an object directory of the
# variant's own and the variant's output path; the product's objects and libraries are not touched.
cd "$(dirname "$0")/../yart_amd/csrc" || exit 1
mkdir -p ../_variants _gen
if ! make -j8 EXTRA="-w $2" GEN=_gen/variant_$1 OUT=../_variants/$1.so ../_variants/$1.so > _gen/variant_$1.log 2>&1; then
  echo "build_variant $1: the build failed"; grep -h -m3 -i "error" _gen/variant_$1.log | cut -c1-300; rm -rf _gen/variant_$1 _gen/variant_$1.log; exit 1
fi
rm -rf _gen/variant_$1 _gen/variant_$1.log
echo built $1
