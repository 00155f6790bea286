// conv_train16_f16.hip -- the kernel of conv_train16.hip on IEEE half tensors (v_mfma_f32_32x32x16_f16, fp32
// accumulation): fi_train16_conv_dgrad_gated_f16.  Same tiles, same LDS image, same epilogue; only the 16-bit type and
// the MFMA differ.
#define FI_E16_HALF 1
#include "conv_train16.hip"
