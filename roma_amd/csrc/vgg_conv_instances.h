// 3x3 / stride 1 / pad 1 convolution with the folded-BatchNorm bias and the ReLU in the store — the VGG19-BN layers of
// romatch/models/encoders.py:68-78 on channels-last fp16 maps.  The convolution is Composable Kernel's grouped forward convolution
// (the kernel family MIOpen's solver search picks for these layers); what is the project's own is the CDE functor below and the
// choice of tile instances.  Shared by vgg_conv.hip (entry points) and vgg_conv_{a,b,c}.hip (the instances, split so that the
// build runs them in parallel).
#pragma once
#include <array>
#include <exception>
#include <string>

#include <hip/hip_runtime.h>

#include "error.h"

#include "ck/ck.hpp"
#include "ck/stream_config.hpp"
#include "ck/tensor_operation/gpu/device/convolution_forward_specialization.hpp"
#include "ck/tensor_operation/gpu/device/gemm_specialization.hpp"
#include "ck/tensor_operation/gpu/device/tensor_layout.hpp"
#include "ck/tensor_operation/gpu/element/element_wise_operation.hpp"

namespace roma {
namespace vggconv {

// e = round(max(float(round(acc)) + float(bias), 0)): the two roundings of F.conv2d (fp32 accumulator -> fp16 map) followed by
// bias_relu_nhwc_kernel (fp16 map + bias in fp32 -> fp16).  CK hands the accumulator over either as fp32 or already rounded to the
// CShuffle type (fp16): the first conversion is the identity then.
struct BiasReluRound {
  static constexpr const char* name = "BiasReluRound";
  template <typename E, typename C, typename D>
  __host__ __device__ constexpr void operator()(E& e, const C& c, const D& d) const {
    const ck::half_t r = ck::type_convert<ck::half_t>(c);
    e = ck::type_convert<E>(fmaxf(ck::type_convert<float>(r) + ck::type_convert<float>(d), 0.f));
  }
};

struct ConvArgs {
  const void* x;
  const void* w;
  const void* bias;
  void* y;
  int B, Cin, Cout, H, W, x_pitch, y_pitch;
  hipStream_t stream;
};

enum Mode { kName, kCheck, kRun };

// One instance: its type string, whether it supports `a`, or the launch.  Returns 0, ROMA_E_UNSUPPORTED or a HIP error code (> 0).
using InstanceFn = int (*)(const ConvArgs& a, Mode mode, std::string* name);

struct InstanceList {
  const InstanceFn* fn;
  int n;
};
InstanceList instances_a();
InstanceList instances_b();
InstanceList instances_c();

using F16 = ck::half_t;
using F32 = float;
template <ck::index_t... Is>
using S = ck::Sequence<Is...>;
using NHWGC = ck::tensor_layout::convolution::NHWGC;
using GKYXC = ck::tensor_layout::convolution::GKYXC;
using NHWGK = ck::tensor_layout::convolution::NHWGK;
using PassThrough = ck::tensor_operation::element_wise::PassThrough;
constexpr auto kConvDefault = ck::tensor_operation::device::ConvolutionForwardSpecialization::Default;
constexpr auto kMNKPadding = ck::tensor_operation::device::GemmSpecialization::MNKPadding;

template <typename Op>
int run_instance(const ConvArgs& a, Mode mode, std::string* name) {
  Op op;
  if (mode == kName) {
    *name = op.GetTypeString();
    return 0;
  }
  using Arr = std::array<ck::index_t, 5>;
  const int B = a.B, C = a.Cin, K = a.Cout, H = a.H, W = a.W, xp = a.x_pitch, yp = a.y_pitch;
  // lengths and strides in CK's (G, N, C|K, H, W) order; the memory orders are NHWGC, GKYXC and NHWGK with G = 1
  const Arr x_len{1, B, C, H, W}, x_str{C, H * W * xp, 1, W * xp, xp};
  const Arr w_len{1, K, C, 3, 3}, w_str{K * 9 * C, 9 * C, 1, 3 * C, C};
  const Arr y_len{1, B, K, H, W}, y_str{K, H * W * yp, 1, W * yp, yp};
  const Arr b_str{K, 0, 1, 0, 0};                             // the bias: one row of K values for every pixel
  const std::array<ck::index_t, 2> one{1, 1};
  try {
    auto arg = op.MakeArgument(a.x, a.w, std::array<const void*, 1>{a.bias}, a.y, x_len, x_str, w_len, w_str,
                               std::array<Arr, 1>{y_len}, std::array<Arr, 1>{b_str}, y_len, y_str, one, one, one, one,
                               PassThrough{}, PassThrough{}, BiasReluRound{});
    if (!op.IsSupportedArgument(arg)) return ROMA_E_UNSUPPORTED;
    if (mode == kCheck) return 0;
    op.MakeInvoker().Run(arg, StreamConfig{a.stream, false});
  } catch (const std::exception& e) {                         // CK reports a failed launch by throwing
    *name = e.what();
    const int rc = (int)hipGetLastError();
    return rc ? rc : (int)hipErrorUnknown;
  }
  return 0;
}

// The rows of CK's instance lists (library/tensor_operation_instance/gpu/grouped_conv_fwd/device_grouped_conv_fwd_xdl_*_instance.hpp)
// with the project's layouts, bias operand and functor.  V1: BlockSize, M/N/KPerBlock, M/NXdlPerWave, the C-shuffle cluster.
#define ROMA_CONV_V1(BLK, M, N, K, MX, NX, CM, CN)                                                                                  \
  ck::tensor_operation::device::DeviceGroupedConvFwdMultipleABD_Xdl_CShuffle<                                                       \
      2, NHWGC, GKYXC, ck::Tuple<NHWGK>, NHWGK, F16, F16, F32, F16, ck::Tuple<F16>, F16, PassThrough, PassThrough, BiasReluRound,   \
      kConvDefault, kMNKPadding, 1, BLK, M, N, K, 8, 8, 32, 32, MX, NX, S<4, BLK / 4, 1>, S<1, 0, 2>, S<1, 0, 2>, 2, 8, 8, 1,        \
      S<4, BLK / 4, 1>, S<1, 0, 2>, S<1, 0, 2>, 2, 8, 8, 1, 1, 1, S<1, CM, 1, CN>, 8>

// V3 (the "comp" lists): KPerBlock, AK1 = BK1, the A/B thread-cluster K0, LDS padding flag, scheduler and pipeline version.
#define ROMA_CONV_V3(M, N, K, K1, K0, PAD, SCHED, VER)                                                                              \
  ck::tensor_operation::device::DeviceGroupedConvFwdMultipleABD_Xdl_CShuffle_V3<                                                    \
      2, NHWGC, GKYXC, ck::Tuple<NHWGK>, NHWGK, F16, F16, F32, F16, ck::Tuple<F16>, F16, PassThrough, PassThrough, BiasReluRound,   \
      kConvDefault, kMNKPadding, 256, M, N, K, K1, K1, 32, 32, 2, 2, S<K0, 256 / K0, 1>, S<1, 0, 2>, S<1, 0, 2>, 2, 8, 8, PAD,      \
      S<K0, 256 / K0, 1>, S<1, 0, 2>, S<1, 0, 2>, 2, 8, 8, PAD, 1, 1, S<1, 32, 1, 8>, 8, ck::BlockGemmPipelineScheduler::SCHED,     \
      ck::BlockGemmPipelineVersion::VER>

}  // namespace vggconv
}  // namespace roma
