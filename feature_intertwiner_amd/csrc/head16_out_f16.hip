// head16_out_f16.hip -- the kernel of head16_out.hip on IEEE half operands: fi_head16_out1x1_f16.  Same tiles, same
// summation order (v_mfma_f32_32x32x16_f16), same epilogue.
#define FI_E16_HALF 1
#include "head16_out.hip"
