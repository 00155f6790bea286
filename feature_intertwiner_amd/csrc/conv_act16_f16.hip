// conv_act16_f16.hip -- the kernels of conv_act16.hip on IEEE half tensors (v_mfma_f32_32x32x16_f16, fp32 accumulation):
// fi_act16_conv_forward_f16, fi_act16_pack_f16, fi_act16_unpack_f16.  Same tiles, same LDS layout, same epilogue; only the
// 16-bit type (RNE to an 11-bit significand and 5-bit exponent: values beyond 65504 become inf) and the MFMA differ.
#define FI_E16_HALF 1
#include "conv_act16.hip"
