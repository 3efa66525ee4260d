# Experiment libraries (not the product): libnkvmerkle_<tag>.so with extra -D flags.
#   bash tools/build_exp.sh <tag> -DFOO=1 ...
# The sources are the product's (nakevaleng_amd/build.py SOURCES).
set -e
tag=$1; shift
cd "$(dirname "$0")/.."
srcs=$(python3 -c "from nakevaleng_amd.build import SOURCES; print(' '.join('nakevaleng_amd/csrc/' + f for f in SOURCES))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -pthread -Wall -Wno-unused-result \
  -I include -I nakevaleng_amd/csrc "$@" $srcs -L/opt/rocm/lib -lrccl -lhsa-runtime64 \
  -o tools/libnkvmerkle_$tag.so
