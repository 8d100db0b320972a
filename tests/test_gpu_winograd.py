"""The Winograd F(2x2,3x3) fp32 convolution (csrc/conv_wino.hip) on the MI355X: every full-size VGG-16 layer of the 600 x 1000 inference
forward (and rpn_conv_3x3) against a float64 convolution, under the bar of the split-product path -- its largest error at most 4x the direct
kernel's on the same operands + 2e-7 of the output scale; the fused pool equals the unfused Winograd output followed by maxpool2x2; the K-split
form is bit-identical over repeats; and the FRCNN_CONV_WINO=0 switch returns the direct kernel.  The full-size layers also stand under the
oracle-relative bar (at most 4x the error of the oracle's own fp32 convolution + 2e-7), and the edge-shape table, both chunk sizes, forced
splits, the weight transform, the status codes and U after an optimizer step / load_npz run through the case functions the emulator
suite uses (tests/wino_cases.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_cases as WC  # noqa: E402

pytestmark = pytest.mark.gpu

# name, Cin, Cout, H, W (the VGG-16 inference forward at 600 x 1000; conv5_x and rpn_conv_3x3 share the last shape)
LAYERS = [
    ("conv1_2", 64, 64, 600, 1000), ("conv2_1", 64, 128, 300, 500), ("conv2_2", 128, 128, 300, 500), ("conv3_1", 128, 256, 150, 250),
    ("conv3_2", 256, 256, 150, 250), ("conv4_1", 256, 512, 75, 125), ("conv4_2", 512, 512, 75, 125), ("conv5_1", 512, 512, 38, 63),
]


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


def _operands(cin, cout, h, w, seed):
    rng = np.random.RandomState(seed)
    x = np.maximum(rng.standard_normal((1, cin, h, w)), 0).astype(np.float32)          # post-ReLU activations
    W = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    return x, W, b


def _ref64(x, W, b):
    import torch
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(W).double(), torch.from_numpy(b).double(), padding=1)
    return y.numpy()


def _both(rt, x, W, b, act):
    from chainer_faster_rcnn_amd.models.vgg16 import Conv3x3
    link = Conv3x3(rt, W.shape[1], W.shape[0])
    link.set(W, b)
    xd = rt.mem.from_numpy(x)
    yw = link.wino(xd, relu=act != 0, pool=act == 4)
    yd = link.relu_pool(xd) if act == 4 else link(xd, relu=act != 0)
    rt.mem.synchronize()
    return link, xd, yw.cpu().numpy(), yd.cpu().numpy()


@pytest.mark.parametrize("layer", LAYERS, ids=[l[0] for l in LAYERS])
def test_winograd_full_size_layer_vs_float64(rt, layer):
    name, cin, cout, h, w = layer
    x, W, b = _operands(cin, cout, h, w, seed=cin + cout + h)
    _, _, yw, yd = _both(rt, x, W, b, act=0)
    ref = _ref64(x, W, b)
    scale = np.abs(ref).max()
    ew, ed = np.abs(yw - ref).max() / scale, np.abs(yd - ref).max() / scale
    print("\nWINO %s direct %.3e wino %.3e ratio %.2f" % (name, ed, ew, ew / ed))
    assert ew <= 4 * ed + 2e-7, (name, ew, ed)
    # the same bar with the oracle's fp32 convolution as comparator: a regression of the direct kernel cannot loosen this one
    eo = np.abs(WC.ref32(x, W, b, 0) - ref).max() / scale
    print("WINO %s ref32 %.3e wino / ref32 %.2f" % (name, eo, ew / eo))
    WC.RATIOS.append(((cin, cout, h, w), 0, "full-size", float(ew), float(eo)))
    assert ew <= 4 * eo + 2e-7, (name, ew, eo)


@pytest.mark.parametrize("shape", [(64, 64, 75, 125), (128, 128, 37, 61), (512, 512, 38, 63), (72, 64, 19, 45)])
def test_winograd_fused_pool_equals_unfused_then_pool(rt, shape):
    cin, cout, h, w = shape
    x, W, b = _operands(cin, cout, h, w, seed=7)
    link, xd, yp, _ = _both(rt, x, W, b, act=4)
    yr = rt.maxpool2x2(link.wino(xd, relu=True))
    rt.mem.synchronize()
    assert yp.shape == (1, cout, (h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(yp, yr.cpu().numpy())


@pytest.mark.parametrize("shape", [(512, 512, 38, 63), (100, 64, 23, 37), (256, 128, 75, 125)])
def test_winograd_odd_shapes_and_split_deterministic(rt, shape):
    # ragged Cin (100: not a whole number of 8-channel chunks), odd maps, the split-K launches of the small maps: the float64 bar and
    # bit-identical repeats
    cin, cout, h, w = shape
    x, W, b = _operands(cin, cout, h, w, seed=11)
    link, xd, yw, yd = _both(rt, x, W, b, act=1)
    ref = np.maximum(_ref64(x, W, b), 0)
    scale = np.abs(ref).max()
    ew, ed = np.abs(yw - ref).max() / scale, np.abs(yd - ref).max() / scale
    assert ew <= 4 * ed + 2e-7, (shape, ew, ed)
    for _ in range(3):
        again = link.wino(xd, relu=True)
        rt.mem.synchronize()
        assert np.array_equal(again.cpu().numpy(), yw)


def test_vgg16_inference_routes_through_winograd_and_switch(rt):
    from chainer_faster_rcnn_amd import synthetic, tuning
    from chainer_faster_rcnn_amd.models import FasterRCNN
    params = synthetic.params(seed=1)
    x = synthetic.image(seed=3, h=160, w=224)
    model = FasterRCNN(runtime=rt)
    model.load_params(params)
    assert model.trunk.conv3_2.wino_applies() and model.RPN.rpn_conv_3x3.wino_applies() and not model.trunk.conv1_1.wino_applies()
    xd = rt.mem.from_numpy(x)
    fw = model.trunk(xd)
    with tuning.override(FRCNN_CONV_WINO="0"):
        assert not model.trunk.conv3_2.wino_applies()
        fd = model.trunk(xd)
    rt.mem.synchronize()
    fw, fd = fw.cpu().numpy(), fd.cpu().numpy()
    assert not np.array_equal(fw, fd)                     # two different algorithms ...
    assert np.abs(fw - fd).max() <= 1e-4 * np.abs(fd).max()    # ... on the same features


# ---- the case functions of tests/wino_cases.py on the device
@pytest.mark.parametrize("env", WC.ENVS, ids=WC.env_id)
@pytest.mark.parametrize("shape", WC.EDGE_SHAPES, ids=WC.shape_id)
def test_wino_edge_shape_vs_float64(rt, shape, env):
    WC.check_wino_shape(rt, shape, env)


@pytest.mark.parametrize("shape", WC.EDGE_SHAPES + [(128, 128, 37, 61)], ids=WC.shape_id)
def test_wino_chunk_size_does_not_change_the_bits(rt, shape):
    WC.check_wino_cfg_identical(rt, shape)


@pytest.mark.parametrize("case", [((64, 64, 6, 31), {}), ((68, 64, 5, 35), {"FRCNN_CONV_WINO_SPLIT": "3"}),
                                  ((9, 192, 13, 97), {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "2"}),
                                  ((512, 512, 38, 63), {}), ((256, 128, 75, 125), {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "5"})],
                         ids=lambda c: WC.shape_id(c[0]) + "_" + WC.env_id(c[1]))
def test_wino_split_repeats_and_nan_workspace(rt, case):
    WC.check_wino_split_repeats(rt, *case)


@pytest.mark.parametrize("env", WC.ENVS[1:], ids=WC.env_id)
def test_winograd_full_size_small_maps_under_the_knobs(rt, env):
    # conv5_x / rpn_conv_3x3 and an odd conv4-sized map with 4-channel chunks and forced splits: the oracle-relative bar, all three acts
    WC.check_wino_shape(rt, (512, 512, 38, 63), env, seed=2)
    WC.check_wino_shape(rt, (72, 64, 75, 125), env, seed=3)


def test_wino_pack(rt):
    WC.check_wino_pack(rt)
    WC.check_wino_pack(rt, shapes=((512, 512),), seed=1)


def test_wino_status_codes_and_workspace_bytes(rt):
    WC.check_wino_status(rt)


@pytest.mark.parametrize("variant", ["rpn", "rcnn", "load"])
def test_wino_weights_follow_the_parameters(rt, variant, tmp_path):
    WC.check_wino_derived(rt, variant, tmp_path)


def test_wino_error_ratios_recorded(rt):
    """Prints the range of err_wino / err_ref32 over this file's float64 checks (DESIGN.md 3.12 records it); every check asserts the bar."""
    if not WC.RATIOS:
        WC.check_wino_shape(rt, (12, 64, 7, 37), {})
    n, lo, hi = WC.ratio_summary()
    print("\nWINO MI355X: %d checks, err_wino / err_ref32 = %.2f .. %.2f" % (n, lo, hi))
    full = [ew / er for _, _, tag, ew, er in WC.RATIOS if tag == "full-size"]
    if full:
        print("WINO MI355X full-size layers: err_wino / err_ref32 = %.2f .. %.2f" % (min(full), max(full)))
    assert n > 0 and all(ew <= 4 * er + 2e-7 for _, _, _, ew, er in WC.RATIOS)
