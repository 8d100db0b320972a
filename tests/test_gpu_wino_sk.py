"""The Winograd convolution that finishes its K split inside the kernel (frcnn_conv3x3_wino_sk_f32, csrc/conv_wino.hip) on the MI355X: the
case functions the emulator suite runs (tests/wino_sk_cases.py), a captured graph of three launches replayed three times, and the
compiled kernel's register / LDS / scratch budget."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_sk_cases as SK  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.gpu
@pytest.mark.parametrize("case", SK.TABLE, ids=SK.case_id)
def test_gpu_sk_case_vs_float64(rt, case):
    SK.check_sk_case(rt, case)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SK.PIECE_COUNTS)
@pytest.mark.parametrize("shape", SK.PIECE_SHAPES, ids=SK.WC.shape_id)
def test_gpu_sk_pieces_give_the_classic_bits(rt, shape, n):
    SK.check_sk_bits_against_classic(rt, shape, n)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(68, 64, 5, 35), (512, 512, 38, 63), (256, 512, 75, 125), (128, 128, 37, 61)], ids=SK.WC.shape_id)
def test_gpu_sk_default_gives_the_classic_bits(rt, shape):
    SK.check_sk_default_bits(rt, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SK.REPEAT_CASES, ids=SK.case_id)
def test_gpu_sk_repeats_and_nan_slots(rt, case):
    SK.check_sk_repeats(rt, case)


@pytest.mark.gpu
def test_gpu_sk_two_shapes_on_one_workspace(rt):
    SK.check_sk_two_shapes_one_workspace(rt)


@pytest.mark.gpu
def test_gpu_sk_status_codes_and_workspace_bytes(rt):
    SK.check_sk_status(rt)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [None, "balance"], ids=["default", "balance"])
def test_gpu_sk_full_size_split_layer(rt, G):
    """conv5's shape under the library's own pick (the classic seven pieces per tile) and as 2 x CU count balanced ranges: the bar, the
    epilogue equalities, zero counters."""
    SK.check_sk_case(rt, ((512, 512, 38, 63), G))


@pytest.mark.gpu
def test_gpu_sk_graph_replay(rt):
    """A linear single-stream graph of three launches of a shape that shares tiles, replayed three times: the same bits every time, equal
    to the eager launch, and the counter page zero afterwards."""
    import torch
    from chainer_faster_rcnn_amd import tuning
    shape, G = (100, 64, 23, 37), 29
    Cin, Cout, H, W = shape
    assert max(SK.partition(*SK.dims(*shape), G)[1]) >= 3
    (x, w, b), _, _, _ = SK.reference(shape, 0)
    xd, ud, bd = SK.dev(rt, x), SK.WC.pack_u(rt, w), SK.dev(rt, b)
    with tuning.override(**SK.env_of(G)):
        eager = SK.host(rt, rt.conv3x3_wino(xd, ud, bd, act=1))                   # allocates and initialises the workspace outside the capture
        outs = [SK.dev(rt, np.full((1, Cout, H, W), SK.POISON, np.float32)) for _ in range(3)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for y in outs:
                rt.conv3x3_wino(xd, ud, bd, act=1, out=y)
    for _ in range(3):
        for y in outs:
            y.fill_(float(SK.POISON))
        graph.replay()
        torch.cuda.synchronize()
        for y in outs:
            assert np.array_equal(SK.host(rt, y), eager)
    assert SK.counters_are_zero(rt)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_sk_kernel_keeps_two_workgroups_per_cu(tmp_path):
    """From the compiled assembly (resource fields only): no scratch, at most 256 registers, at most 80 KB of LDS -- two workgroups per CU."""
    from test_isa_waits import asm_of
    text = open(asm_of("conv_wino", tmp_path)).read()
    found = re.findall(r"\.amdhsa_kernel (\S*wino_sk_f32_kernel\S*)\n(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(found) == 2, [k for k, _ in found]                                  # whole chunks (scalar offset) and ragged Cin
    for k, meta in found:
        field = lambda n: int(re.search(r"\.amdhsa_%s\s+(\d+)" % n, meta).group(1))     # noqa: E731
        assert field("private_segment_fixed_size") == 0, k + ": scratch in use"
        assert field("next_free_vgpr") <= 256, "%s: %d registers" % (k, field("next_free_vgpr"))
        assert field("group_segment_fixed_size") <= 81920, "%s: %d bytes of LDS" % (k, field("group_segment_fixed_size"))
