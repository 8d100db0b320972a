#!/usr/bin/env python
"""A/B of the ResNet 1x1 kernel (frcnn_conv1x1_bf16, csrc/resnet_bf16.hip) against the generic frcnn_conv_bf16(ksize=1) path on the stride-1 1x1 shapes of
ResNet-101 at 600 x 1000 (the generic path has no stride and no residual: it is timed with ReLU and no residual, the new kernel with the act the layer
uses).  HIP events around hipGraph replays (bench.graph_time_us).  GPU only.  Usage: python scripts/conv1x1_bf16_ab.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import chainer_faster_rcnn_amd as pkg  # noqa: E402
import bench  # noqa: E402
from resnet16_cases import resnet101_layer_shapes  # noqa: E402


def main():
    rt = pkg.runtime.default_runtime()
    rs = np.random.RandomState(0)
    rows = []
    for cin, cout, h, w, stride, act in resnet101_layer_shapes(600, 1000):
        x = rt.bf16_from_nchw(rt.mem.from_numpy(np.abs(rs.randn(1, cin, h, w)).astype(np.float32)))
        wp = rt.bf16_pack_conv_w(rt.mem.from_numpy((rs.randn(cout, cin, 1, 1) * 0.05).astype(np.float32)), 1)
        b = rt.mem.from_numpy(np.zeros(cout, np.float32))
        ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
        r = rt.bf16_from_nchw(rt.mem.from_numpy(rs.randn(1, cout, ho, wo).astype(np.float32))) if act == 3 else None
        new_us = bench.graph_time_us(torch, lambda: rt.conv1x1_bf16(x, wp, b, cin, cout, stride=stride, act=act, residual=r), 1, 200)
        old_us = bench.graph_time_us(torch, lambda: rt.conv_bf16(x, wp, b, cin, cout, ksize=1, relu=True), 1, 200) if stride == 1 else None
        gflop = 2.0 * cin * cout * ho * wo / 1e9
        rows.append({"shape": [cin, cout, h, w, stride, act], "splits": rt.conv1x1_bf16_splits(cin, cout, h, w, stride), "gflop": round(gflop, 3),
                     "conv1x1_us": round(new_us, 2), "conv_bf16_ksize1_us": None if old_us is None else round(old_us, 2),
                     "conv1x1_tflops": round(gflop / new_us * 1e3, 1)})
        print(json.dumps(rows[-1]), flush=True)


if __name__ == "__main__":
    main()
