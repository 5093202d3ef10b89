// The SSIM kernels that walk TWO sources per pass (loss_kernel_pair; sfm_ssim_pair.h): pixel-interleaved layout, the product's
// projection, gradient launches of an even number of sources without the warped output.  A translation unit of its own (compiles
// next to sfm_loss.hip).
#include "sfm_loss_kernels.h"

namespace sfm {

const void* kernel_of_pair(const Variant& v) { return lift_variant<Family::Pair>(v); }

}  // namespace sfm
