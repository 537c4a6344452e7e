// SpMM forward kernels for value type double, index type int32_t (spmm_forward_rules.h).
#pragma clang fp contract(off)

#include "spmm_forward_rules.h"

OFX_SPMM_INSTANTIATE(double, int32_t)
