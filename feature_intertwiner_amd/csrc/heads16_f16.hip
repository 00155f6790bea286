// heads16_f16.hip -- the kernels of heads16.hip on IEEE half tensors: fi_heads16_*_f16.  Same grids, same lane maps, same
// sums; only the 16-bit type differs (an overflow rounds to infinity, as IEEE says).
#define FI_E16_HALF 1
#include "heads16.hip"
