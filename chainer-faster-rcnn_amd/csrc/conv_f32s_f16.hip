// conv_f32s_f16.hip -- the fp16 instantiation of conv_f32s.hip's ONE-PART training forms (RPNTrainer(conv_math="f16")):
//   frcnn_conv3x3_f16_train = conv_f32s_kernel<4, 0, 1, 1>      forward / input-gradient 3x3 convolution, dual output, fused ReLU mask
//   frcnn_conv1_f16_train   = conv1_f32s_kernel<NCB, false, true>   conv1_1 on the fp32 image and the packed fp32 master weights
//   frcnn_f16_pack_many     = pack_w_f32s_many_kernel<1>        forward + input-gradient weights of every layer in one launch
// With one operand part only the `h` word of frcnn_split3_pair is used, and h = frcnn_pack_bf16x2, which in this translation unit is
// v_cvt_pk_f16_f32; the MFMA helper is v_mfma_f32_32x32x16_f16.  Nothing else in those kernels depends on the 16-bit format.
// conv_f32s.hip leaves everything that is not one of these forms -- the three-part split kernels, whose m and l terms are bf16 bit
// arithmetic -- out of a translation unit compiled with FRCNN_HALF_F16.  Same signatures, layouts, workspace and error codes as the
// bf16 twins; |v| > 65504 rounds to Inf.  Replaces L.Convolution2D + F.relu of the trunk and rpn_conv_3x3 in the training step
// (models/vgg16.py:39-82, region_proposal_network.py:53) on the fp16 line.
#define FRCNN_HALF_F16 1
#include "frcnn_f16_names.h"
#include "conv_f32s.hip"
