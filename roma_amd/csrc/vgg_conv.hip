// Entry points of the fused VGG19-BN layer (3x3 convolution + folded-BN bias + ReLU, channels-last fp16): argument checks and the
// dispatch over the instances of vgg_conv_{a,b,c}.hip.  Which instance a layer runs is the caller's static choice
// (encoders.vgg_conv_impl, filled from tools/vgg_conv_tune.py): nothing is searched or timed here.
#include <climits>
#include <cstring>

#include "common.h"
#include "vgg_conv_instances.h"

using namespace roma;

namespace {

vggconv::InstanceFn find_instance(int index) {
  const vggconv::InstanceList lists[] = {vggconv::instances_a(), vggconv::instances_b(), vggconv::instances_c()};
  for (const auto& l : lists) {
    if (index < l.n) return l.fn[index];
    index -= l.n;
  }
  return nullptr;
}

int instance_count() { return vggconv::instances_a().n + vggconv::instances_b().n + vggconv::instances_c().n; }

}  // namespace

extern "C" int roma_conv3x3_bias_relu_instances(int index, char* name, int cap) {
  const int n = instance_count();
  if (!name) return n;
  ROMA_REQUIRE(index >= 0 && index < n && cap > 0, ROMA_E_ARG, "roma_conv3x3_bias_relu_instances: index %d of %d, cap %d", index, n, cap);
  std::string s;
  find_instance(index)(vggconv::ConvArgs{}, vggconv::kName, &s);
  std::strncpy(name, s.c_str(), (size_t)cap - 1);
  name[cap - 1] = 0;
  return n;
}

extern "C" int roma_conv3x3_bias_relu(const void* x, const void* w, const void* bias, void* y, int B, int Cin, int Cout, int H, int W,
                                      int dtype, int x_pitch, int y_pitch, int instance, void* stream) {
  ROMA_REQUIRE(x && w && bias && y, ROMA_E_ARG, "roma_conv3x3_bias_relu: null pointer");
  ROMA_REQUIRE(dtype == ROMA_F16, dtype == ROMA_F32 || dtype == ROMA_BF16 ? ROMA_E_UNSUPPORTED : ROMA_E_DTYPE,
               "roma_conv3x3_bias_relu: dtype %d (fp16 only)", dtype);
  ROMA_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && x_pitch >= Cin && y_pitch >= Cout, ROMA_E_SHAPE,
               "roma_conv3x3_bias_relu: bad shape B=%d Cin=%d Cout=%d H=%d W=%d x_pitch=%d y_pitch=%d", B, Cin, Cout, H, W, x_pitch, y_pitch);
  ROMA_REQUIRE((long)B * H * W * (x_pitch > y_pitch ? x_pitch : y_pitch) <= INT_MAX && (long)Cout * 9 * Cin <= INT_MAX, ROMA_E_SHAPE,
               "roma_conv3x3_bias_relu: a map of B=%d H=%d W=%d with pitch %d / %d exceeds 2^31 - 1 elements", B, H, W, x_pitch, y_pitch);
  ROMA_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0 && x_pitch % 8 == 0 && y_pitch % 8 == 0 && aligned16(x) && aligned16(w) && aligned16(bias) &&
                   aligned16(y), ROMA_E_ALIGN,
               "roma_conv3x3_bias_relu: Cin = %d, Cout = %d and the pitches %d / %d must be multiples of 8 and the buffers 16-byte aligned",
               Cin, Cout, x_pitch, y_pitch);
  const vggconv::InstanceFn fn = instance >= 0 ? find_instance(instance) : nullptr;
  ROMA_REQUIRE(fn, ROMA_E_ARG, "roma_conv3x3_bias_relu: instance %d of %d", instance, instance_count());
  const vggconv::ConvArgs a{x, w, bias, y, B, Cin, Cout, H, W, x_pitch, y_pitch, static_cast<hipStream_t>(stream)};
  std::string what;
  const int rc = fn(a, vggconv::kRun, &what);
  ROMA_REQUIRE(rc != ROMA_E_UNSUPPORTED, ROMA_E_UNSUPPORTED,
               "roma_conv3x3_bias_relu: instance %d does not support B=%d Cin=%d Cout=%d H=%d W=%d on this device", instance, B, Cin, Cout, H, W);
  ROMA_REQUIRE(rc == 0, rc, "roma_conv3x3_bias_relu: launch failed: %s", what.c_str());
  ROMA_CHECK_LAUNCH();
}
