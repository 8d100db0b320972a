// linear_train_f16.hip -- the fp16 instantiation of linear_train_bf16.hip: forward, input gradient and weight gradient of an L.Linear on RNE-fp16 operands
// with fp32 accumulation (RCNNTrainer(precision="f16")).  Entry points: the *_f16* twins of the *_bf16* ones (frcnn_f16_names.h; declared in include/frcnn_hip.h).
#define FRCNN_HALF_F16 1
#include "frcnn_f16_names.h"
#include "linear_train_bf16.hip"
