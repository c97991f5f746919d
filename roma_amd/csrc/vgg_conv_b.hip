// Convolution instances 4-7 of roma_conv3x3_bias_relu (vgg_conv_instances.h): the search's pick for conv4_x at 560 and three neighbouring tiles
#include "vgg_conv_instances.h"
#include "ck/tensor_operation/gpu/device/impl/device_grouped_conv_fwd_multiple_abd_xdl_cshuffle.hpp"

namespace roma {
namespace vggconv {

InstanceList instances_b() {
  static const InstanceFn fn[] = {
      run_instance<ROMA_CONV_V1(128, 64, 128, 32, 2, 2, 16, 8)>,  // conv4_x at 560
      run_instance<ROMA_CONV_V1(256, 128, 256, 32, 2, 4, 32, 8)>,
      run_instance<ROMA_CONV_V1(128, 128, 64, 32, 2, 2, 32, 4)>,
      run_instance<ROMA_CONV_V1(256, 64, 128, 32, 1, 2, 32, 8)>,
  };
  return {fn, (int)(sizeof(fn) / sizeof(fn[0]))};
}

}  // namespace vggconv
}  // namespace roma
