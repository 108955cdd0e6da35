// The persistent reach seeds kernel for models with obstacle slots
// (drc_model_set_obstacles): reach_seeds_kernel.hip's kernel with
// task_instance<0, false, OBST = true> and the call's poses, built apart so
// that the plain unit is not compiled next to it.  Reference: no counterpart.
#define DRC_REACH_SEEDS_OBST 1
#include "reach_seeds_kernel.hip"
