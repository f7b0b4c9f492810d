/* the f16x3 half of tile_launch_f32v2ws.hip as a translation unit of its own (see there) */
#define LSSVM_TU_HALF 1
#include "tile_launch_f32v2ws.hip"
