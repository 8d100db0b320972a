"""The detection-head epilogue (csrc/head.hip), the stage-2 loss, the RPN loss at its edges and the stage-2 glue kernels (csrc/train.hip) on
the host emulator (tests/hipemu), through the case functions of tests/head_loss_cases.py; and, without a GPU, the build's promise that
the box arithmetic of head.hip is not contracted into fused multiply-adds (the emulator is compiled with -ffp-contract=off on the host
and could never see such a regression of the device build: the gfx950 listing can)."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
import head_loss_cases as HC  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


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
        print("HEADLOSS emulator %s: %d checks, device %.3e .. %.3e, oracle %.3e .. %.3e" % (what, len(dv), min(dv), max(dv), min(orc), max(orc)))
    assert HC.FIGURES


# ---- 5. the build's no-contraction promise, on the gfx950 listing (no GPU needed: hipcc cross-compiles)
FMA_F32 = re.compile(r"\bv_(?:pk_)?(?:fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)_f32(?:_\w+)?\b")       # with or without an encoding suffix (_e32, _e64, _dpp ...)
NO_FMA_KERNELS = ("head_decode_kernel", "clip_boxes_kernel", "class_dets_kernel", "preprocess_kernel")


def kernel_bodies(asm_text):
    """mangled name -> the instructions between the kernel's label and its .Lfunc_end"""
    bodies, name = {}, None
    for ln in asm_text.splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif name is not None and ln.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            bodies[name].append(ln.split(";")[0])
    return bodies


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_head_box_arithmetic_is_not_contracted(tmp_path):
    """csrc/head.hip: "the reference's operation order, no FMA contraction".  The four kernels whose fp32 arithmetic the reference states
    (decode, clip, class_dets, preprocess) hold no fp32 fused multiply-add in the listing the build's own flags give; the f64 FMAs of the
    double exp are expected, and the two softmax kernels carry expf's own, so neither is looked at."""
    spec = importlib.util.spec_from_file_location("_frcnn_build_flags", os.path.join(ROOT, "chainer-faster-rcnn_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-ffp-contract=off" in b.FLAGS
    out = str(tmp_path / "head.s")
    subprocess.run([b.HIPCC if os.path.exists(b.HIPCC) else "hipcc"] + b.FLAGS + ["-S", "--cuda-device-only", os.path.join(b.HERE, "head.hip"), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    bodies = kernel_bodies(open(out).read())
    for frag in NO_FMA_KERNELS:
        hits = {k: v for k, v in bodies.items() if frag in k}
        assert len(hits) == 1, (frag, sorted(bodies))
        for k, lines in hits.items():
            text = "\n".join(lines)
            assert "s_endpgm" in text, k
            if frag in ("head_decode_kernel", "preprocess_kernel"):
                assert re.search(r"\bv_(?:pk_)?mul_f32(?:_\w+)?\b", text) and re.search(r"\bv_(?:pk_)?(?:add|sub)_f32(?:_\w+)?\b", text), k      # the separate multiply and add are there
            found = FMA_F32.findall(text)
            assert not found, "%s: %d fp32 fused multiply-adds (%s): the build contracts head.hip's box arithmetic" % (k, len(found), sorted(set(found)))
    # the scan sees an FMA when there is one: the softmax kernels' expf, and the double exp of the decode kernel
    assert any(FMA_F32.search("\n".join(v)) for k, v in bodies.items() if "row_softmax_kernel" in k)
    assert any(re.search(r"\bv_fma_f64(?:_\w+)?\b", "\n".join(v)) for k, v in bodies.items() if "head_decode_kernel" in k)
