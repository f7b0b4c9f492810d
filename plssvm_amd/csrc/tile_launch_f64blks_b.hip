/* the sixteen-vector symmetric fp64 kernel on 7 ... 16 chunks: tile_launch_f64blks.hip as a translation unit of its own (see there) */
#define LSSVM_TU_HALF 2
#include "tile_launch_f64blks.hip"
