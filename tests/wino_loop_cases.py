"""Checks of the Winograd chunk loop (wino_tile_loop, csrc/conv_wino.hip), written once and run on the host emulator
(tests/test_wino_loop_emulated.py, research build: the first loop is there as FRCNN_CONV_WINO_LOOP=0) and on the MI355X
(tests/test_gpu_wino_loop.py, product library).  Operands, references, the poison value and the accuracy bar are tests/wino_cases.py's; the
in-kernel-split checks are tests/wino_sk_cases.py's.

The shipped loop is unrolled by two (the buffer index is a compile-time constant in each half, the odd last chunk of a range runs behind the
loop), reads the next chunk's step-0 fragments in front of the chunk's last MFMAs, writes the right-border zeros before the chunk's barrier
and stages a wave's U pieces four per M0 write.  The table holds the smallest shapes at which each of these can go wrong:
  Cin    8 one chunk (the tail alone), 16 two (one trip through the loop, no tail), 24 three (loop + tail), 20 three with a ragged last one
         (per-chunk descriptors), 12 with FRCNN_CONV_WINO_CFG=2 three 4-channel chunks (two steps per chunk: the prefetch slot parity)
  Cout   64 and 128 (the second cout block's U rows)
  map    4x32 exact tile, W % 4 = 0 (no border fix); 5x7 one ragged tile, W % 4 = 3; 6x33 two x tiles -- the left-border and the
         right-border tile are different tiles, W % 4 = 1; 9x66 three x tiles and three y tiles, W % 4 = 2
  acts   0, 1, 4
and 72 -> 64 at 9x66 (9 chunks) through the in-kernel-split entry with 2 pieces (5 + 4 chunks: an odd and an even range), 3 pieces (3 + 3 + 3:
ranges that begin on either parity) and 5 ranges over the 9 tiles x 9 chunks (a workgroup crosses a tile boundary in mid-range and restarts
its ring)."""
import numpy as np

from chainer_faster_rcnn_amd import tuning
from parity_cases import dev, host
import wino_cases as WC
import wino_sk_cases as SK

__all__ = ["dev", "host", "WC", "SK", "tuning"]

POISON = WC.POISON
FIRST_LOOP = {"FRCNN_CONV_WINO_LOOP": "0"}

CINS = [(8, {}), (16, {}), (24, {}), (20, {}), (12, {"FRCNN_CONV_WINO_CFG": "2"})]
MAPS = [(4, 32), (5, 7), (6, 33), (9, 66)]
# every Cin at every map; Cout alternates so that every Cin and every map meets both 64 and 128
TABLE = [((ci, 64 if (i + j) % 2 == 0 else 128, h, w), env) for i, (ci, env) in enumerate(CINS) for j, (h, w) in enumerate(MAPS)]
SK_SHAPE = (72, 64, 9, 66)
SK_ENVS = [{"FRCNN_CONV_WINO_SK_PIECES": "2"}, {"FRCNN_CONV_WINO_SK_PIECES": "3"}, {"FRCNN_CONV_WINO_SK_G": "5"}]
ORDER_CASES = [((24, 64, 6, 33), {}), ((20, 128, 9, 66), {}), ((12, 128, 5, 7), {"FRCNN_CONV_WINO_CFG": "2"})]      # + SK_SHAPE under SK_ENVS


def case_id(case):
    return "%s_%s" % (WC.shape_id(case[0]), WC.env_id(case[1]))


def table_covers():
    """what the docstring promises, by assertion"""
    shapes = [s for s, _ in TABLE]
    assert {s[0] for s in shapes} == {8, 16, 24, 20, 12} and {(s[2], s[3]) for s in shapes} == set(MAPS) and len(TABLE) == 20
    for ci in (8, 16, 24, 20, 12):
        assert {s[1] for s in shapes if s[0] == ci} == {64, 128}
    for h, w in MAPS:
        assert {s[1] for s in shapes if (s[2], s[3]) == (h, w)} == {64, 128}
    assert {w % 4 for _, w in MAPS} == {0, 1, 2, 3}
    assert all((env == {"FRCNN_CONV_WINO_CFG": "2"}) == (s[0] == 12) for s, env in TABLE)
    ntiles, nchunks = SK.dims(*SK_SHAPE)
    assert (ntiles, nchunks) == (9, 9)
    _, _, two = SK.equal_pieces(ntiles, nchunks, 2)
    assert sorted({c1 - c0 for p in two for _, c0, c1 in p}) == [4, 5]
    _, sharers, five = SK.partition(ntiles, nchunks, 5)
    assert any(len(p) >= 2 and p[0][2] == nchunks and p[1][1] == 0 for p in five) and max(sharers) >= 2      # a range crosses a tile boundary
    assert {c0 % 2 for p in five for _, c0, _ in p} == {0, 1}                                                 # ranges start on either parity


_REF = {}


def reference(shape, act, seed=0):
    """(operands, float64 reference, the oracle's fp32 error, scale) of a shape, computed once per process and left unchanged"""
    key = (tuple(shape), act, seed)
    if key not in _REF:
        x, w, b = WC.operands(*shape, seed)
        want = WC.ref64(x, w, b, act)
        scale = float(np.abs(want).max())
        _REF[key] = ((x, w, b), want, float(np.abs(WC.ref32(x, w, b, act) - want).max() / scale), scale)
    return _REF[key]


def run(rt, shape, env, act, seed=0):
    Cin, Cout, H, W = shape
    (x, w, b), _, _, _ = reference(shape, 0, seed)
    return WC.launch(rt, dev(rt, x), WC.pack_u(rt, w), dev(rt, b), Cout, H, W, act, env)


def check_bar(shape, act, got):
    """wino_cases' bar (at most 4x the oracle's fp32 error + 2e-7, both against float64), the shape, and no poison left"""
    _, want, err_ref32, scale = reference(shape, act)
    assert got.shape == want.shape == WC.out_shape(shape[1], shape[2], shape[3], act)
    assert not (got == POISON).any(), "%d output elements were never written" % int((got == POISON).sum())
    assert np.isfinite(got).all()
    err = float(np.abs(got - want).max() / scale)
    print("WINO-LOOP %s act %d: %.3e ref32 %.3e" % (WC.shape_id(shape), act, err, err_ref32))
    assert err <= 4 * err_ref32 + 2e-7, (shape, act, err, err_ref32)


def check_case(rt, case, first_loop):
    """One table row at acts 0 / 1 / 4: the float64 bar, no poison, act 1 = ReLU(act 0), act 4 = pool(act 1); first_loop (research builds):
    bit for bit the first loop's output"""
    shape, env = case
    outs = []
    for act in (0, 1, 4):
        got = run(rt, shape, env, act)
        check_bar(shape, act, got)
        if first_loop:
            old = run(rt, shape, dict(env, **FIRST_LOOP), act)
            assert not (old == POISON).any()
            assert np.array_equal(got.view(np.uint32), old.view(np.uint32)), (case, act, float(np.abs(got - old).max()))
        outs.append(got)
    y0, y1, y4 = outs
    assert np.array_equal(np.maximum(y0, 0), y1)
    assert np.array_equal(host(rt, rt.maxpool2x2(dev(rt, y1))), y4)


def check_sk(rt, env, first_loop):
    """The in-kernel-split entry on SK_SHAPE under `env`: the bar and the epilogue equalities, zero counters, and (research builds) the first
    loop's bits"""
    outs = []
    for act in (0, 1, 4):
        got = run(rt, SK_SHAPE, env, act)
        check_bar(SK_SHAPE, act, got)
        assert SK.counters_are_zero(rt)
        if first_loop:
            old = run(rt, SK_SHAPE, dict(env, **FIRST_LOOP), act)
            assert np.array_equal(got.view(np.uint32), old.view(np.uint32)), (env, act)
            assert SK.counters_are_zero(rt)
        outs.append(got)
    y0, y1, y4 = outs
    assert np.array_equal(np.maximum(y0, 0), y1)
    assert np.array_equal(host(rt, rt.maxpool2x2(dev(rt, y1))), y4)


def check_sk_equals_classic(rt, n):
    """n pieces finished in the kernel give the classic entry's bits under FRCNN_CONV_WINO_SPLIT=n (slabs + wino_combine_kernel)"""
    for act in (0, 1, 4):
        new = run(rt, SK_SHAPE, {"FRCNN_CONV_WINO_SK_PIECES": str(n)}, act)
        old = run(rt, SK_SHAPE, {"FRCNN_CONV_WINO_SPLIT": str(n)}, act)
        assert not (new == POISON).any() and not (old == POISON).any()
        assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), (n, act)


def check_repeats(rt):
    """Three repeats of the five-range launch are identical, also with every slot of the workspace full of NaN (tests/wino_sk_cases.py), and
    so are three repeats of an unsplit table row"""
    SK.check_sk_repeats(rt, (SK_SHAPE, 5))
    shape, env = TABLE[10]
    first = run(rt, shape, env, 1)
    for _ in range(2):
        assert np.array_equal(run(rt, shape, env, 1), first)


def check_chunk_sizes_agree(rt):
    """unsplit, 8- and 4-channel chunks give the same bits: 24 channels are three chunks of one and six of the other"""
    WC.check_wino_cfg_identical(rt, (24, 64, 6, 33))
    WC.check_wino_cfg_identical(rt, (16, 128, 9, 66))


def order_outputs(rt):
    """act 1 and act 4 outputs of ORDER_CASES and of SK_SHAPE under SK_ENVS (seed 5): compared across DMA landing times and workgroup orders"""
    out = []
    for shape, env in ORDER_CASES + [(SK_SHAPE, e) for e in SK_ENVS]:
        out += [run(rt, shape, env, act, seed=5) for act in (1, 4)]
    return out
