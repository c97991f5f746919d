// Convolution instances 0-3 of roma_conv3x3_bias_relu (vgg_conv_instances.h): the four tiles MIOpen's search picks for the 256 x 256-thread layers
#include "vgg_conv_instances.h"
#include "ck/tensor_operation/gpu/device/impl/device_grouped_conv_fwd_multiple_abd_xdl_cshuffle.hpp"

namespace roma {
namespace vggconv {

InstanceList instances_a() {
  static const InstanceFn fn[] = {
      run_instance<ROMA_CONV_V1(256, 128, 64, 32, 2, 1, 32, 8)>,  // conv1_2
      run_instance<ROMA_CONV_V1(256, 256, 128, 32, 4, 2, 32, 8)>,  // conv2_1; conv3_x at 864
      run_instance<ROMA_CONV_V1(256, 128, 128, 32, 2, 2, 32, 8)>,  // conv2_2 at 560
      run_instance<ROMA_CONV_V1(128, 128, 128, 32, 4, 2, 16, 8)>,  // conv2_2 at 864, conv3_x at 560, conv4_x at 864
  };
  return {fn, (int)(sizeof(fn) / sizeof(fn[0]))};
}

}  // namespace vggconv
}  // namespace roma
