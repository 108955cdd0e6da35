// The fused task + QP kernel for models with convex-hull collision geometry:
// fused_kernel.hip's kernel with task_instance<0, MESH = true>, built apart so
// that the mesh-free unit is not compiled next to it.
#define DRC_FUSED_MESH 1
#include "fused_kernel.hip"
