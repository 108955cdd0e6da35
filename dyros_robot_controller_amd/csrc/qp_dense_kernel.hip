// The QP kernel of the two manipulator shapes with the dense G loops
// (Dims<..., dense = true>): the reference build of drc_debug_qp_dense and
// tests/test_gpu_qp_sparse.py, built apart so that the shipped QP unit is not
// compiled next to it.
#define DRC_QP_DENSE_UNIT 1
#include "qp_kernel.hip"
