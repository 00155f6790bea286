// fpn16_f16.hip -- the kernel of fpn16.hip on IEEE half tensors: fi_fpn16_topdown_grad_f16.  Same grid, same lane map,
// same sums; only the 16-bit type differs (an overflow rounds to infinity, as IEEE says).
#define FI_E16_HALF 1
#include "fpn16.hip"
