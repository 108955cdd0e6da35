// The fused task + QP kernel for models with obstacle slots
// (drc_model_set_obstacles): fused_kernel.hip's kernel with
// task_instance<0, false, OBST = true>, built apart so that the plain unit is
// not compiled next to it.  Reference: no counterpart.
#define DRC_FUSED_OBST 1
#include "fused_kernel.hip"
