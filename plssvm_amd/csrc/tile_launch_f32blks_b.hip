/* the sixteen-vector symmetric fp32 kernel on bf16x6 planes: tile_launch_f32blks.hip as a translation unit of its own (see there) */
#define LSSVM_TU_HALF 2
#include "tile_launch_f32blks.hip"
