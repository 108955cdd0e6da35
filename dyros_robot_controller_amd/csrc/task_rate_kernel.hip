// The QPIK task stage for models with obstacle slots whose slots move
// (drc_qpik_*moving_obstacles_batch with a twist): task_obstacle_kernel.hip's
// kernel with task_instance<0, false, OBST = true, RATE = true>, whose obstacle
// lanes also load their slot's twist and whose distance for the QP carries the
// winner's dd/dt (task_stage.hpp), built apart so that the unit without twists
// is not compiled next to it.  Reference: no counterpart.
#define DRC_TASK_RATE 1
#include "task_obstacle_kernel.hip"
