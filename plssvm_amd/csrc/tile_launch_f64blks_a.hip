/* the sixteen-vector symmetric fp64 kernel on 1 ... 6 chunks, its entry points and its packing kernel: tile_launch_f64blks.hip as a translation unit of its own (see there) */
#define LSSVM_TU_HALF 1
#include "tile_launch_f64blks.hip"
