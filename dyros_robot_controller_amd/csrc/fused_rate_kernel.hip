// The fused task + QP kernel for models with obstacle slots whose slots move
// (a twist per slot): fused_kernel.hip's kernel with
// task_instance<0, false, OBST = true, RATE = true>, built apart so that
// neither the plain nor the obstacle unit is compiled next to it.
// Reference: no counterpart.
#define DRC_FUSED_RATE 1
#include "fused_kernel.hip"
