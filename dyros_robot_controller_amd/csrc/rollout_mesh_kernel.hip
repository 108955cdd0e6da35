// The persistent rollout kernel for models with convex-hull collision
// geometry: rollout_kernel.hip's kernel with task_instance<0, MESH = true>,
// built apart so that the mesh-free unit is not compiled next to it.
#define DRC_ROLLOUT_MESH 1
#include "rollout_kernel.hip"
