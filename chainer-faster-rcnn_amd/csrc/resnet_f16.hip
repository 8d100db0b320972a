// resnet_f16.hip -- the fp16 instantiation of resnet_bf16.hip: the bottleneck 1x1 convolution, the stem's columns and the 3x3/2 max-pool of the ResNet trunk on
// channel-blocked fp16 maps.  Same kernels, layouts, tiles and split-K workspace as the bf16 line; v_mfma_f32_32x32x16_f16, 10 mantissa bits instead of 7.
// Entry points: the *_f16* twins of the *_bf16* ones (frcnn_f16_names.h; declared in include/frcnn_hip.h).
#define FRCNN_HALF_F16 1
#include "frcnn_f16_names.h"
#include "resnet_bf16.hip"
