#!/bin/bash
# Experiment builds: libmrirt_<name>.so under build_exp/ with extra -D flags applied to ONE source file
# (objects of the other sources are cached).  Select at run time with MRIRT_LIB=build_exp/libmrirt_<name>.so.
#   bash tools/build_variant.sh <name> <source.hip> [extra hipcc flags...]
# The sources are _lib.HIP_SOURCES (the list the library itself is built from); a cached object is stale against its
# source and against every header of csrc/ and include/.
set -e
NAME=$1; SRC=$2; shift 2
REPO=$(cd "$(dirname "$0")/.." && pwd)
CS=$REPO/mri-raytracer_amd/csrc
OUT=$REPO/build_exp
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p $OUT/obj
# (_lib.py alone, not the package: the list needs no torch)
SOURCES=$(python3 -c "import importlib.util as u, sys; s = u.spec_from_file_location('_lib', sys.argv[1]); m = u.module_from_spec(s); s.loader.exec_module(m); print(' '.join(m.HIP_SOURCES))" $REPO/mri-raytracer_amd/_lib.py)
case " $SOURCES " in *" $SRC "*) ;; *) echo "$SRC is not one of: $SOURCES" >&2; exit 2;; esac
FLAGS="-O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -std=c++17 -Wall -I$REPO/include"
OBJS=""
for f in $SOURCES; do
  if [ "$f" == "$SRC" ]; then
    O=$OUT/obj/${f}_$NAME.o
    $HIPCC $FLAGS "$@" -c $CS/$f -o $O
  else
    O=$OUT/obj/$f.o
    STALE=""
    for d in $CS/$f $CS/*.h $REPO/include/mrirt.h; do
      if [ ! -f $O ] || [ $d -nt $O ]; then STALE=1; fi
    done
    if [ -n "$STALE" ]; then $HIPCC $FLAGS -c $CS/$f -o $O; fi
  fi
  OBJS="$OBJS $O"
done
$HIPCC --offload-arch=gfx950 -shared -fPIC $OBJS -o $OUT/libmrirt_$NAME.so
echo built $OUT/libmrirt_$NAME.so
