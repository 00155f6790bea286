// head16_crop_f16.hip -- the kernel of head16_crop.hip on IEEE half maps: fi_head16_pyramid_crop_forward_f16.  Same tables,
// same gather, same interpolation; only the widening (v_cvt_f32_f16 instead of a shift) and the rounding at the store differ.
#define FI_E16_HALF 1
#include "head16_crop.hip"
