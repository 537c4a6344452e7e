// SpMM forward kernels for value type float, index type int64_t (spmm_forward_rules.h).
#pragma clang fp contract(off)

#include "spmm_forward_rules.h"

OFX_SPMM_INSTANTIATE(float, int64_t)
