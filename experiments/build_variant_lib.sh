# experiments/bin/<name>.so: the library with extra compiler flags for ONE translation unit
#   bash experiments/build_variant_lib.sh <name> <file.hip> <flags...>
# (<file.hip> relative to ndt_2d_amd/csrc; every other object is the one `python -m ndt_2d_amd.build`
# left beside its source, the test-hooks objects excluded)
set -e
R=$(cd $(dirname $0)/.. && pwd)
NAME=$1; FILE=$2; shift 2
C=$R/ndt_2d_amd/csrc
mkdir -p $R/experiments/bin/obj_$NAME
OWN=$R/experiments/bin/obj_$NAME/$(basename ${FILE%.hip}).o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC "$@" -I $R/include -I $C -c $C/$FILE -o $OWN
OBJS=""
for o in $C/*.o $C/*/*.o; do
  case $o in
    *.hooks.o) ;;
    $C/${FILE%.hip}.o) OBJS="$OBJS $OWN" ;;
    *) OBJS="$OBJS $o" ;;
  esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS -ldl -lpthread -o $R/experiments/bin/$NAME.so
