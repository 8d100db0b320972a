"""The 16-bit ResNet-101 Faster R-CNN (csrc/resnet_bf16.hip, resnet_f16.hip; models/resnet.py conv_dtype="bf16") on the MI355X: the whole forward
against the fp32 oracle at 600 x 1000 and 600 x 901, the trunk kernels at every distinct ResNet-101 layer shape, and the captured forward."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet16_cases as R  # noqa: E402
from parity_cases import half_format  # noqa: E402

pytestmark = pytest.mark.gpu

# res5 bounds of the issue (fraction of the fp32 oracle's feature scale); cls_prob / pred_boxes: the VGG bf16 test's 3e-2
RES5_TOL = {"bf16": 5e-2, "f16": 1e-2}
HEAD_TOL = 3e-2


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


def resnet_frcnn_params():
    """the parameters of test_gpu_fullsize.py::test_resnet101_config4_600x1000"""
    from chainer_faster_rcnn_amd import synthetic
    params = synthetic.resnet_params(101, seed=2)
    rs = np.random.RandomState(3)
    head = synthetic.params(seed=1, rpn_ch=512, roi_feat=2048 * 49)
    for k in ("fc6", "fc7", "cls_score", "bbox_pred"):
        params[k + "/W"], params[k + "/b"] = head[k + "/W"], head[k + "/b"]
    params["RPN/rpn_conv_3x3/W"] = (rs.randn(512, 2048, 3, 3) * 0.01).astype(np.float32)
    params["RPN/rpn_conv_3x3/b"] = np.zeros(512, np.float32)
    for k in ("rpn_cls_score", "rpn_bbox_pred"):
        params["RPN/%s/W" % k], params["RPN/%s/b" % k] = head["RPN/%s/W" % k], head["RPN/%s/b" % k]
    return params


def make_model(rt, params, dtype):
    from chainer_faster_rcnn_amd.models import FasterRCNN, ResNet101
    model = FasterRCNN(trunk_class=ResNet101, rpn_in_ch=2048, rpn_mid_ch=512, feat_stride=32, runtime=rt, conv_dtype=dtype, head_dtype=dtype)
    model.load_params(params)
    model.RPN.proposal_layer._pre_nms_top_n, model.RPN.proposal_layer._post_nms_top_n = 1000, 300
    return model


@pytest.fixture(scope="module")
def params():
    return resnet_frcnn_params()


_ORACLE = {}


def oracle_res5(params, x, key):
    from oracle import frcnn_oracle as O
    if key not in _ORACLE:
        _ORACLE[key] = O.resnet_forward(params, x)
    return _ORACLE[key]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("im_h,im_w", [(600, 1000), (600, 901)])
def test_resnet101_16bit_forward(rt, params, dtype, im_h, im_w):
    from chainer_faster_rcnn_amd import synthetic
    from oracle import frcnn_oracle as O
    from oracle.parity import rel_err
    model = make_model(rt, params, dtype)
    x = synthetic.image(seed=6, h=im_h, w=im_w) / 64.0
    info = np.array([[im_h, im_w]], dtype=np.int32)
    out = model.forward_device(rt.mem.from_numpy(x), im_h, im_w, keep=True)
    feat = rt.mem.to_numpy(out["feat"])
    want = oracle_res5(params, x, (im_h, im_w))
    assert feat.shape == want.shape == (1, 2048, 19, 32 if im_w == 1000 else 29)
    rep = {"res5_rel_err": rel_err(feat, want)}
    n = int(rt.mem.to_numpy(out["n_out"])[0])
    p2, _, d2 = O.proposal_layer(rt.mem.to_numpy(out["rpn_cls_prob"]), rt.mem.to_numpy(out["rpn_bbox_pred"]), info, train=False,
                                 feat_stride=32, pre_nms_top_n=1000, post_nms_top_n=300, return_debug=True)
    rep["n_rois"] = n
    rep["proposals_index_exact_given_device_maps"] = bool(n == len(p2) and np.array_equal(rt.mem.to_numpy(out["src_index"])[:n],
                                                                                          d2["src_index"].astype(np.int32)))
    rois = rt.mem.to_numpy(out["rois"])[:n]
    pool5 = O.roi_pooling_2d(feat, np.concatenate([np.zeros((n, 1), np.float32), rois], 1), 7, 7, 1 / 32.)
    rep["pool5_exact"] = bool(np.array_equal(rt.mem.to_numpy(out["pool5"])[:n], pool5))
    cp, pb, _ = O.rcnn_head(params, pool5, rois, info)
    rep["cls_prob_rel_err"] = rel_err(rt.mem.to_numpy(out["cls_prob"])[:n], cp)
    rep["pred_boxes_rel_err"] = rel_err(rt.mem.to_numpy(out["pred_boxes"])[:n], pb)
    print("RESNET16 %s %dx%d %s" % (dtype, im_h, im_w, json.dumps(rep)))
    assert n > 0
    assert rep["res5_rel_err"] <= RES5_TOL[dtype], rep
    assert rep["proposals_index_exact_given_device_maps"] and rep["pool5_exact"], rep
    assert rep["cls_prob_rel_err"] <= HEAD_TOL and rep["pred_boxes_rel_err"] <= HEAD_TOL, rep
    # the default (non-keep) forward pools from the blocked map itself: the same RoIs and head outputs
    out2 = model.forward_device(rt.mem.from_numpy(x), im_h, im_w)
    for k in ("rois", "n_out", "cls_prob", "pred_boxes"):
        assert np.array_equal(rt.mem.to_numpy(out2[k]), rt.mem.to_numpy(out[k])), k


@pytest.mark.parametrize("case", R.resnet101_layer_shapes(600, 1000), ids=lambda c: "%d-%d_%dx%d_s%d_a%d" % c)
def test_conv1x1_bf16_resnet101_shapes(rt, case):
    cin, cout, h, w, stride, act = case
    print("conv1x1 %s: %d-way K split" % (case, rt.conv1x1_bf16_splits(cin, cout, h, w, stride)))
    R.check_conv1x1(rt, *case)


@pytest.mark.parametrize("case", [c for c in R.resnet101_layer_shapes(600, 1000) if c[2] <= 38], ids=lambda c: "%d-%d_%dx%d_s%d_a%d" % c)
def test_conv1x1_f16_resnet101_small_maps(rt, case):
    with half_format("f16"):
        R.check_conv1x1(rt.with_half("f16"), *case)


def test_pool_im2col_resnet101_shapes(rt):
    R.check_im2col7x7s2_16(rt, 600, 1000)
    R.check_maxpool3x3s2_16(rt, 64, 300, 500)
    R.check_im2col7x7s2_16(rt, 600, 901, seed=1)
    R.check_maxpool3x3s2_16(rt, 64, 300, 451, seed=1)


def test_resnet16_layers_small_image(rt):
    err, errs = R.check_resnet16_layers(rt, (3, 4, 23, 3), 160, 224, tol_res5=5e-2)
    print("ResNet-101 bf16 at 160x224, layer by layer: worst %.2e, res5 %.2e" % (max(errs.values()), err))


@pytest.mark.parametrize("dtype", ["bf16"])
def test_resnet16_captured_forward(rt, params, dtype):
    import torch
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.graph import CapturedForward
    model = make_model(rt, params, dtype)
    h, w = 600, 1000
    x = rt.mem.from_numpy(synthetic.image(seed=6, h=h, w=w) / 64.0)
    eager = {k: rt.mem.to_numpy(v) for k, v in model.forward_device(x, h, w).items()}
    cap = CapturedForward(model, x, h, w)
    got = {k: rt.mem.to_numpy(v) for k, v in cap.replay().items()}
    torch.cuda.synchronize()
    for k in eager:
        assert np.array_equal(eager[k], got[k]), k
    x2 = rt.mem.from_numpy(synthetic.image(seed=7, h=h, w=w) / 64.0)
    got2 = {k: rt.mem.to_numpy(v) for k, v in cap.replay(x2).items()}
    assert not np.array_equal(got2["cls_prob"], got["cls_prob"])
    eager2 = {k: rt.mem.to_numpy(v) for k, v in model.forward_device(x2, h, w).items()}
    for k in eager2:
        assert np.array_equal(eager2[k], got2[k]), k
