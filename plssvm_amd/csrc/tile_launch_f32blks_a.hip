/* the sixteen-vector symmetric fp32 kernel on f16x3 planes, its entry points and its packing kernel: tile_launch_f32blks.hip as a translation unit of its own (see there) */
#define LSSVM_TU_HALF 1
#include "tile_launch_f32blks.hip"
