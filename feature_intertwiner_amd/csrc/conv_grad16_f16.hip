// conv_grad16_f16.hip -- the kernels of conv_grad16.hip on IEEE half tensors (v_mfma_f32_32x32x16_f16, fp32 accumulation):
// fi_grad16_relu_grad_f16, fi_grad16_conv_dgrad_f16, fi_grad16_conv_wgrad_f16.  Same tiles, same LDS images, same
// epilogues; only the 16-bit type and the MFMA differ (ds_read_b64_tr_b16 moves 16-bit words of either type).
#define FI_E16_HALF 1
#include "conv_grad16.hip"
