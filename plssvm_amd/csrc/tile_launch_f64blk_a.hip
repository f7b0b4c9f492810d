/* the sixteen-vector full-square fp64 kernel on 1 ... 6 chunks, its entry points and its packing kernel: tile_launch_f64blk.hip as a translation unit of its own (see there) */
#define LSSVM_TU_HALF 1
#include "tile_launch_f64blk.hip"
