"""The Winograd chunk loop (wino_tile_loop, csrc/conv_wino.hip) on the MI355X, product library: the rows of tests/wino_loop_cases.py under the
float64 bar with no poison left, the in-kernel-split entry against the classic one in bits, 8- against 4-channel chunks, repeats, a captured
graph of three launches, and the research knob refused."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_loop_cases as LC  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.gpu
@pytest.mark.parametrize("case", LC.TABLE, ids=LC.case_id)
def test_gpu_loop_case_vs_float64(rt, case):
    LC.check_case(rt, case, first_loop=False)


@pytest.mark.gpu
@pytest.mark.parametrize("env", LC.SK_ENVS, ids=LC.WC.env_id)
def test_gpu_loop_in_kernel_split_ranges(rt, env):
    LC.check_sk(rt, env, first_loop=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_gpu_loop_in_kernel_split_equals_classic(rt, n):
    LC.check_sk_equals_classic(rt, n)


@pytest.mark.gpu
def test_gpu_loop_chunk_sizes_agree(rt):
    LC.check_chunk_sizes_agree(rt)


@pytest.mark.gpu
def test_gpu_loop_repeats(rt):
    LC.check_repeats(rt)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [((24, 128, 9, 66), {}), (LC.SK_SHAPE, LC.SK_ENVS[2])], ids=LC.case_id)
def test_gpu_loop_graph_replay(rt, case):
    """the same entry replayed from a captured single-stream graph of three launches, three times: the eager launch's bits every time"""
    import torch
    from chainer_faster_rcnn_amd import tuning
    shape, env = case
    Cin, Cout, H, W = shape
    (x, w, b), _, _, _ = LC.reference(shape, 0)
    xd, ud, bd = LC.dev(rt, x), LC.WC.pack_u(rt, w), LC.dev(rt, b)
    with tuning.override(**env):
        eager = LC.host(rt, rt.conv3x3_wino(xd, ud, bd, act=1))                   # allocates and initialises the workspace outside the capture
        outs = [LC.dev(rt, np.full((1, Cout, H, W), LC.POISON, np.float32)) for _ in range(3)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for y in outs:
                rt.conv3x3_wino(xd, ud, bd, act=1, out=y)
    LC.check_bar(shape, 1, eager)
    for _ in range(3):
        for y in outs:
            y.fill_(float(LC.POISON))
        graph.replay()
        torch.cuda.synchronize()
        for y in outs:
            assert np.array_equal(LC.host(rt, y).view(np.uint32), eager.view(np.uint32))


@pytest.mark.gpu
def test_gpu_first_loop_is_a_research_form(rt):
    """FRCNN_CONV_WINO_LOOP=0 (and any form but the shipped one) is refused by the product library before anything is launched"""
    from chainer_faster_rcnn_amd import tuning
    L, m = rt.lib, rt.mem
    shape = (16, 64, 4, 32)
    Cin, Cout, H, W = shape
    (x, w, b), _, _, _ = LC.reference(shape, 0)
    xd, ud, bd = LC.dev(rt, x), LC.WC.pack_u(rt, w), LC.dev(rt, b)
    y = LC.dev(rt, np.full((1, Cout, H, W), LC.POISON, np.float32))
    for form in ("0", "1", "5"):
        with tuning.override(FRCNN_CONV_WINO_LOOP=form):
            assert L.frcnn_conv3x3_wino_f32(m.ptr(xd), m.ptr(ud), m.ptr(bd), m.ptr(y), Cin, Cout, H, W, 1, None, 0, m.stream()) == -1
            assert L.frcnn_conv3x3_wino_sk_f32(m.ptr(xd), m.ptr(ud), m.ptr(bd), m.ptr(y), Cin, Cout, H, W, 1, None, 0, m.stream()) == -1
    m.synchronize()
    assert (LC.host(rt, y) == LC.POISON).all()
    with tuning.override(FRCNN_CONV_WINO_LOOP="7"):                               # the shipped form by its number
        assert L.frcnn_conv3x3_wino_f32(m.ptr(xd), m.ptr(ud), m.ptr(bd), m.ptr(y), Cin, Cout, H, W, 1, None, 0, m.stream()) == 0
    m.synchronize()
    LC.check_bar(shape, 1, LC.host(rt, y))
