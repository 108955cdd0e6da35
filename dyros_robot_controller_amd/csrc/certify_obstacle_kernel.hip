// The certified-clearance kernel for models with obstacle slots
// (drc_model_set_obstacles): certify_kernel.hip's kernel with task_instance<3,
// false, OBST = true> and the call's poses, static along the path; built apart
// so that the plain unit is not compiled next to it.  Reference: no counterpart.
#define DRC_CERT_OBST 1
#include "certify_kernel.hip"
