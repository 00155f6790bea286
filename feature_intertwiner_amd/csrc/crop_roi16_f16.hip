// crop_roi16_f16.hip -- the kernel of crop_roi16.hip on IEEE half maps: fi_roi16_pyramid_crop_forward_f16.  Same tables,
// same LDS tile, same interpolation; only the widening differs (v_cvt_f32_f16 instead of a shift).
#define FI_E16_HALF 1
#include "crop_roi16.hip"
