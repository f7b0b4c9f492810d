/* the two-vector symmetric instantiations of tile_launch_f64.hip as a translation unit of their own (see there) */
#define LSSVM_TU_HALF 3
#include "tile_launch_f64.hip"
