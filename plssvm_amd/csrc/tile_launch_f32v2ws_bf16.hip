/* the bf16x6 half of tile_launch_f32v2ws.hip, and its entry point, as a translation unit of its own (see there) */
#define LSSVM_TU_HALF 2
#include "tile_launch_f32v2ws.hip"
