// SpMM forward kernels for value type f16, index type int32_t (spmm_forward_rules.h).
#pragma clang fp contract(off)

#include "spmm_forward_rules.h"

OFX_SPMM_INSTANTIATE(ofx::f16, int32_t)
