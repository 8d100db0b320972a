"""The detection-head epilogue (csrc/head.hip), the stage-2 loss, the RPN loss at its edges and the stage-2 glue kernels (csrc/train.hip) on
the MI355X, through the case functions the emulator suite uses (tests/head_loss_cases.py): the boxes of frcnn_head_decode,
frcnn_head_decode_stacked, frcnn_bbox_transform_inv and frcnn_clip_boxes word for word against the oracle's restatement with exp evaluated
in double (this is where a contracted multiply-add or an fp32 expf of the device build would show), the fused kernel's probabilities as
the same words as frcnn_softmax_rows's, frcnn_rcnn_loss against float64 under the oracle-relative bars, and the glue kernels exactly."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_loss_cases as HC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


# ---- 1. head epilogue
@pytest.mark.parametrize("shape", HC.HEAD_SHAPES, ids=HC.shape_id)
def test_head_epilogue_bit_for_bit(rt, shape):
    HC.check_head_epilogue(rt, *shape)


def test_head_decode_tightened(rt):
    import parity_cases as P
    P.check_head_decode(rt)
    P.check_head_decode(rt, R=300, seed=1)


def test_head_status_codes(rt):
    HC.check_head_status(rt)


def test_stacked_layouts_include_the_models(rt):
    ld, dcol = HC.model_head_layout(rt)
    lays = HC.stacked_layouts(rt, 21)
    assert (ld, dcol) in lays and len(set(lays)) >= 3
    assert any(d == 24 and l == 24 + 84 for l, d in lays) and any(l > d + 84 for l, d in lays)       # ncls rounded up to 4; padding behind the deltas
    assert dcol % 4 == 0 and dcol >= 21 and ld >= dcol + 84


# ---- 2. frcnn_rcnn_loss
@pytest.mark.parametrize("ncls", HC.RCNN_NCLS)
@pytest.mark.parametrize("R", HC.RCNN_R)
def test_rcnn_loss_vs_float64(rt, R, ncls):
    HC.check_rcnn_loss(rt, R, ncls, seed=R + ncls)


@pytest.mark.parametrize("shape", [(300, 21), (257, 5), (128, 2)], ids=HC.shape_id)
def test_rcnn_loss_huge_logits(rt, shape):
    HC.check_rcnn_loss(rt, *shape, seed=9, big=True)


def test_rcnn_loss_other_delta(rt):
    HC.check_rcnn_loss(rt, 130, 21, seed=4, delta=0.5)


def test_rcnn_loss_status_codes(rt):
    HC.check_rcnn_loss_status(rt)


# ---- 3. frcnn_rpn_loss at its edges
def test_rpn_loss_all_labels_ignored(rt):
    HC.check_rpn_loss_all_ignored(rt)


def test_rpn_loss_no_inside_anchor(rt):
    HC.check_rpn_loss_no_inside(rt)


def test_rpn_loss_more_than_one_pass(rt):
    HC.check_rpn_loss_edges(rt, 20, 25, 9, 1500, seed=1)


@pytest.mark.parametrize("A", [1, 3, 9])
def test_rpn_loss_anchor_counts_and_wide_logits(rt, A):
    HC.check_rpn_loss_edges(rt, 7, 9, A, (7 * 9 * A) * 2 // 3, seed=A)
    HC.check_rpn_loss_edges(rt, 7, 9, A, (7 * 9 * A) * 2 // 3, seed=10 + A, sigma=50.0)


# ---- 4. glue kernels
@pytest.mark.parametrize("shape", HC.GATHER_SHAPES, ids=HC.shape_id)
def test_gather_scatter_rows(rt, shape):
    HC.check_gather_scatter(rt, *shape)


def test_scatter_rows_nothing_to_scatter(rt):
    HC.check_scatter_nothing(rt)


def test_gather_rows_moves_int32_words_unchanged(rt):
    HC.check_gather_int32_words(rt)


@pytest.mark.parametrize("n", [1, 1000, HC.BIG_N])
def test_mul_add_in_place_and_stride_loop(rt, n):
    HC.check_mul_add(rt, n)


def test_relu_bwd_gate(rt):
    HC.check_relu_bwd(rt)


@pytest.mark.parametrize("shape", HC.TRANSPOSE_SHAPES, ids=HC.shape_id)
def test_transpose(rt, shape):
    HC.check_transpose(rt, *shape)


# ---- 6. anchor-target ground-truth edges
@pytest.mark.parametrize("name", HC.ANCHOR_TARGET_EDGES)
def test_anchor_target_gt_edges(rt, name):
    HC.check_anchor_target_edge(rt, name)


def test_head_loss_figures_recorded(rt):
    """Prints the range of the device / oracle error figures of this file's float64 checks; every check asserts its own bar."""
    if not HC.FIGURES:
        HC.check_head_epilogue(rt, 37, 21)
        HC.check_rcnn_loss(rt, 128, 21)
    for what in sorted({f[0] for f in HC.FIGURES}):
        dv, orc = [f[2] for f in HC.FIGURES if f[0] == what], [f[3] for f in HC.FIGURES if f[0] == what]
        print("\nHEADLOSS MI355X %s: %d checks, device %.3e .. %.3e, oracle %.3e .. %.3e" % (what, len(dv), min(dv), max(dv), min(orc), max(orc)))
    assert HC.FIGURES
