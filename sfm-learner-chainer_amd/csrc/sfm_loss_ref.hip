// The fused-loss kernels of SfmLossDesc.projection = SFM_PROJECTION_REFERENCE_ORDER: the instantiations of loss_body with the
// per-pixel projection in the reference's own evaluation order (sfm_ssim_pass.h, ref_position; models/transform.py:105-108,122-131,189),
// one for every (entry point, loss mode, smoothness form, layout, warped output) the product's projection has -- except the
// three-waves-per-SIMD builds of the small L1 launches (loss_kernel_wide) and the launches that also produce dL/d(src).
// A translation unit of its own so that it compiles next to sfm_loss.hip (make -j).
#include "sfm_loss_kernels.h"

namespace sfm {

const void* kernel_of_ref(const Variant& v) { return lift_variant<Family::Ref>(v); }

}  // namespace sfm
