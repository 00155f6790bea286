// conv_pyr16_f16.hip -- the kernels of conv_pyr16.hip on IEEE half tensors (v_mfma_f32_32x32x16_f16, fp32 accumulation):
// fi_pyr16_lateral_f16, fi_pyr16_head1x1_f16.  Same tiles, same LDS layout, same epilogues; only the 16-bit type and the
// MFMA differ.
#define FI_E16_HALF 1
#include "conv_pyr16.hip"
