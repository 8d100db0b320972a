// train_f16.hip -- the fp16 instantiation of train.hip's one-part weight gradient (RPNTrainer(conv_math="f16")):
//   frcnn_conv_wgrad_f16 / frcnn_conv_wgrad_f16_workspace_bytes = conv_wgrad_f32s_kernel<1> + wgrad_reduce_kernel
// x and dy (fp32 NCHW) are rounded to fp16 (v_cvt_pk_f16_f32, nearest even) while they are staged, the products run on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation; the kernel moves 16-bit words through LDS and v_alignbit only, so nothing else in it
// depends on the format.  train.hip leaves every other kernel and entry point (targets, losses, the fp32 / split weight gradients, the
// optimizer) out of a translation unit compiled with FRCNN_HALF_F16.  Same arguments, plan, workspace size and error codes as
// frcnn_conv_wgrad_bf16.  Replaces the weight gradient of L.Convolution2D's backward (Chainer v1) on the fp16 line.
#define FRCNN_HALF_F16 1
#include "frcnn_f16_names.h"
#include "train.hip"
