/* the two-vector full-square instantiations of tile_launch_f64.hip as a translation unit of their own (see there) */
#define LSSVM_TU_HALF 5
#include "tile_launch_f64.hip"
