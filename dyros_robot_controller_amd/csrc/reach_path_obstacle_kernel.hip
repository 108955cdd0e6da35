// The persistent reach path kernel for models with obstacle slots
// (drc_model_set_obstacles): reach_path_kernel.hip's kernel with
// task_instance<0, false, OBST = true> and the call's poses, built apart so
// that the plain unit is not compiled next to it.  Reference: no counterpart.
#define DRC_REACH_PATH_OBST 1
#include "reach_path_kernel.hip"
