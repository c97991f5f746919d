// Convolution instances 8-9 of roma_conv3x3_bias_relu (vgg_conv_instances.h): the two "compute friendly" V3 pipelines that work on gfx950
#include "vgg_conv_instances.h"
#include "ck/tensor_operation/gpu/device/impl/device_grouped_conv_fwd_multiple_abd_xdl_cshuffle_v3.hpp"

namespace roma {
namespace vggconv {

InstanceList instances_c() {
  static const InstanceFn fn[] = {
      run_instance<ROMA_CONV_V3(128, 128, 64, 8, 8, 0, Intrawave, v4)>,
      run_instance<ROMA_CONV_V3(128, 128, 64, 16, 4, 1, Interwave, v1)>,  // double-rate MFMA
  };
  return {fn, (int)(sizeof(fn) / sizeof(fn[0]))};
}

}  // namespace vggconv
}  // namespace roma
