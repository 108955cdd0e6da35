// The certified-clearance kernel for models with convex-hull geometry:
// certify_kernel.hip's kernel with task_instance<3, MESH = true> (the two-wave
// register budget, as every hull build), built apart so that the plain unit is
// not compiled next to it.  Reference: no counterpart.
#define DRC_CERT_MESH 1
#include "certify_kernel.hip"
