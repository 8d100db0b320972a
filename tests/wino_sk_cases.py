"""Checks of the Winograd convolution that finishes its K split inside the kernel (frcnn_conv3x3_wino_sk_f32, csrc/conv_wino.hip), written
once and run on the host emulator (tests/test_wino_sk_emulated.py) and on the MI355X (tests/test_gpu_wino_sk.py).  Operands, the float64
reference, the poison value and the accuracy bar are tests/wino_cases.py's.

The kernel cuts total = tiles x chunks units (a tile is 64 couts x 4 rows x 32 columns, a chunk 8 input channels) into G contiguous
ranges, workgroup g taking [g * total // G, (g + 1) * total // G).  `partition` below restates that rule; TABLE is checked against it
(test_table_covers_the_partition_cases), so that the cases the kernel can go wrong at are in the table by assertion."""
import numpy as np

from chainer_faster_rcnn_amd import tuning
from parity_cases import dev, host
import wino_cases as WC

POISON = WC.POISON
COUNTER_PAGE = 64 * 1024
SLOT_BYTES = 64 * 4 * 32 * 4

# (Cin, Cout, H, W), forced number of ranges (None: the library's own pick for the chip it runs on -- the classic launch's pieces)
TABLE = [
    ((68, 64, 5, 35), None),           # ragged last chunk, W % 4 = 3, 4 tiles x 9 chunks
    ((68, 64, 5, 35), 1),              # G = 1: one workgroup walks every tile, nothing shared
    ((68, 64, 5, 35), 10),             # tiles shared by 2 and by 3 workgroups
    ((68, 64, 5, 35), 36),             # G = total: one chunk each, every tile shared by 9
    ((100, 64, 23, 37), 5),            # 12 tiles x 13 chunks: whole tiles between two partial ones, W % 4 = 1, ragged last row under the pool
    ((100, 64, 23, 37), 161),          # above total = 156: clipped
    ((9, 192, 13, 97), 7),             # three cout blocks, 48 tiles x 2 chunks (the second ragged): ends one tile, owns six, begins another
    ((9, 192, 13, 97), 48),            # G = tiles: every tile has its single owner
    ((64, 64, 6, 31), None),           # whole chunks (the scalar-offset form), W % 4 = 3, 2 tiles x 8 chunks
    ((64, 64, 6, 31), 7),              # both tiles shared by 4 workgroups
    ((5, 64, 1, 1), 3),                # 1x1 map, one unit: clipped to G = 1
    ((4, 64, 2, 2), None),             # 2x2 map
]
PIECE_SHAPES = [(68, 64, 5, 35), (100, 64, 23, 37), (9, 192, 13, 97), (64, 64, 6, 31)]
PIECE_COUNTS = (2, 3, 4)


def case_id(case):
    return "%s_G%s" % (WC.shape_id(case[0]), "auto" if case[1] is None else case[1])


def env_of(G):
    if G == "balance":
        return {"FRCNN_CONV_WINO_SK_BALANCE": "1"}
    return {} if G is None else {"FRCNN_CONV_WINO_SK_G": str(G)}


def dims(Cin, Cout, H, W):
    """(tiles, chunks) of the 64-cout x 4-row x 32-column, 8-channel decomposition"""
    return -(-W // 32) * -(-H // 4) * (Cout // 64), -(-Cin // 8)


def default_pieces(rt, Cin, Cout, H, W):
    """the library's pick without a knob: the classic launch's K pieces (tests/wino_cases.plan), finished in the kernel; 1 = classic whole tiles"""
    return WC.plan(rt, Cin, Cout, H, W, {})[1]


def balanced_g(rt, Cin, Cout, H, W):
    """FRCNN_CONV_WINO_SK_BALANCE=1: shapes the classic launch splits get min(total, 2 x CU count) ranges, others whole tiles"""
    ntiles, nchunks = dims(Cin, Cout, H, W)
    return min(ntiles * nchunks, 2 * WC.cu_count(rt)) if default_pieces(rt, Cin, Cout, H, W) > 1 else ntiles


def equal_pieces(ntiles, nchunks, pieces):
    """the classic partition restated: (G, sharers per tile, per-workgroup list of (tile, first chunk, end chunk))"""
    pc = -(-nchunks // max(1, min(pieces, nchunks)))
    pieces = -(-nchunks // pc)
    work = [[(t, p * pc, min(nchunks, (p + 1) * pc))] for t in range(ntiles) for p in range(pieces)]
    return ntiles * pieces, [pieces] * ntiles, work


def partition(ntiles, nchunks, G):
    """The range rule restated.  Returns (G after clipping, sharers per tile, per-workgroup list of (tile, first chunk, end chunk))."""
    total = ntiles * nchunks
    G = max(1, min(G, total))
    sharers = [0] * ntiles
    work = []
    for g in range(G):
        it, end, pieces = g * total // G, (g + 1) * total // G, []
        while it < end:
            tile, c0 = divmod(it, nchunks)
            c1 = min(nchunks, c0 + end - it)
            pieces.append((tile, c0, c1))
            sharers[tile] += 1
            it += c1 - c0
        work.append(pieces)
    return G, sharers, work


def slots_needed(ntiles, nchunks, G):
    G, _, _ = partition(ntiles, nchunks, G)
    return 0 if G == ntiles else COUNTER_PAGE + G * 2 * SLOT_BYTES


def plan_of(rt, shape, G):
    """(G, sharers, work) of a table row: the forced range count, or the default pick"""
    ntiles, nchunks = dims(*shape)
    return partition(ntiles, nchunks, G) if G is not None else equal_pieces(ntiles, nchunks, default_pieces(rt, *shape))


# ------------------------------------------------------------------------------------------- launches
def launch(rt, xd, ud, bd, Cout, H, W, act, env):
    """one Runtime.conv3x3_wino (the new entry: no classic knob is set) under `env` into a poisoned output -> host array"""
    assert not any(k in env for k in ("FRCNN_CONV_WINO_SPLIT", "FRCNN_CONV_WINO_CFG", "FRCNN_CONV_WINO_SK"))
    return WC.launch(rt, xd, ud, bd, Cout, H, W, act, env)


def sk_workspace(rt):
    return rt.workspace("conv_wino_sk", 1)


def counters_are_zero(rt):
    ws = sk_workspace(rt)
    return ws.shape[0] < COUNTER_PAGE or not host(rt, ws[:COUNTER_PAGE]).any()


_REF = {}


def reference(shape, act, seed=0):
    """(operands, float64 reference, oracle fp32 error) of a shape, computed once per process"""
    key = (tuple(shape), act, seed)
    if key not in _REF:
        x, w, b = WC.operands(*shape, seed)
        want = WC.ref64(x, w, b, act)
        scale = np.abs(want).max()
        _REF[key] = ((x, w, b), want, float(np.abs(WC.ref32(x, w, b, act) - want).max() / scale), scale)
    return _REF[key]


def check_sk_case(rt, case):
    """Accuracy of one (shape, G) at acts 0 / 1 / 4 under wino_cases' bar, nothing left poisoned, the epilogue equalities (exact on the
    fix-up path as on the whole-tile path), and the counter page zero after every launch."""
    shape, G = case
    Cin, Cout, H, W = shape
    (x, w, b), _, _, _ = reference(shape, 0)
    xd, ud, bd = dev(rt, x), WC.pack_u(rt, w), dev(rt, b)
    outs = []
    for act in (0, 1, 4):
        _, want, err_ref32, scale = reference(shape, act)
        got = launch(rt, xd, ud, bd, Cout, H, W, act, env_of(G))
        assert got.shape == want.shape == WC.out_shape(Cout, H, W, act)
        assert not (got == POISON).any(), "%d output elements were never written" % int((got == POISON).sum())
        assert np.isfinite(got).all()
        err = float(np.abs(got - want).max() / scale)
        print("WINO-SK %s act %d: sk %.3e ref32 %.3e" % (case_id(case), act, err, err_ref32))
        assert err <= 4 * err_ref32 + 2e-7, (case, act, err, err_ref32)
        assert counters_are_zero(rt), (case, act)
        outs.append(got)
    y0, y1, y4 = outs
    assert np.array_equal(np.maximum(y0, 0), y1)
    assert np.array_equal(host(rt, rt.maxpool2x2(dev(rt, y1))), y4)


def check_sk_bits_against_classic(rt, shape, n):
    """FRCNN_CONV_WINO_SK_PIECES=n gives the classic entry's bits under FRCNN_CONV_WINO_SPLIT=n: the same pieces, added in the same order"""
    Cin, Cout, H, W = shape
    (x, w, b), _, _, _ = reference(shape, 0)
    xd, ud, bd = dev(rt, x), WC.pack_u(rt, w), dev(rt, b)
    for act in (0, 1, 4):
        new = launch(rt, xd, ud, bd, Cout, H, W, act, {"FRCNN_CONV_WINO_SK_PIECES": str(n)})
        old = WC.launch(rt, xd, ud, bd, Cout, H, W, act, {"FRCNN_CONV_WINO_SPLIT": str(n)})
        assert not (new == POISON).any() and not (old == POISON).any()
        assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), (shape, n, act, float(np.abs(new - old).max()))
        assert counters_are_zero(rt)


def check_sk_default_bits(rt, shape):
    """Without a knob the new entry gives the classic entry's bits (FRCNN_CONV_WINO_SK=0 selects it in Runtime.conv3x3_wino): the same
    pieces in the same order on the shapes the classic launch splits, the classic launch itself on the others."""
    Cin, Cout, H, W = shape
    x, w, b = WC.operands(Cin, Cout, H, W, seed=2)
    xd, ud, bd = dev(rt, x), WC.pack_u(rt, w), dev(rt, b)
    for act in (0, 1, 4):
        new = launch(rt, xd, ud, bd, Cout, H, W, act, {})
        old = WC.launch(rt, xd, ud, bd, Cout, H, W, act, {"FRCNN_CONV_WINO_SK": "0"})
        assert not (new == POISON).any() and np.array_equal(new.view(np.uint32), old.view(np.uint32)), (shape, act)


REPEAT_CASES = [((68, 64, 5, 35), 10), ((64, 64, 6, 31), 7), ((9, 192, 13, 97), 7)]


def check_sk_repeats(rt, case):
    """Three repeats give the same bits, also with every slot full of NaN beforehand (counter page left alone); the counters read zero
    after every launch."""
    shape, G = case
    Cin, Cout, H, W = shape
    assert max(plan_of(rt, shape, G)[1]) > 1, "this case must share a tile"
    (x, w, b), _, _, _ = reference(shape, 0)
    xd, ud, bd = dev(rt, x), WC.pack_u(rt, w), dev(rt, b)
    for act in (1, 4):
        first = launch(rt, xd, ud, bd, Cout, H, W, act, env_of(G))
        assert not (first == POISON).any() and counters_are_zero(rt)
        for _ in range(2):
            assert np.array_equal(launch(rt, xd, ud, bd, Cout, H, W, act, env_of(G)), first)
            assert counters_are_zero(rt)
        ws = sk_workspace(rt)
        assert ws.shape[0] > COUNTER_PAGE
        ws[COUNTER_PAGE:] = 0xFF
        assert np.isnan(host(rt, rt.mem.bitcast(ws[COUNTER_PAGE:COUNTER_PAGE + 256], "f32"))).all()
        again = launch(rt, xd, ud, bd, Cout, H, W, act, env_of(G))
        assert np.isfinite(again).all() and np.array_equal(again, first), (case, act)
        assert counters_are_zero(rt)


def check_sk_two_shapes_one_workspace(rt):
    """Two shapes back to back (and the first again) on one workspace that was initialised once: all right, the page zero at the end."""
    L, m = rt.lib, rt.mem
    cases = [((100, 64, 23, 37), 5), ((68, 64, 5, 35), 10)]
    need = max(slots_needed(*dims(*s), G) for s, G in cases)
    ws = dev(rt, np.full((need,), 0xFF, np.uint8))
    assert L.frcnn_conv_wino_sk_workspace_init(m.ptr(ws), need, m.stream()) == 0
    for shape, G in cases + cases[:1]:
        Cin, Cout, H, W = shape
        (x, w, b), want, err_ref32, scale = reference(shape, 0)
        xd, ud, bd = dev(rt, x), WC.pack_u(rt, w), dev(rt, b)
        y = dev(rt, np.full((1, Cout, H, W), POISON, np.float32))
        with tuning.override(**env_of(G)):
            assert L.frcnn_conv3x3_wino_sk_f32(m.ptr(xd), m.ptr(ud), m.ptr(bd), m.ptr(y), Cin, Cout, H, W, 0, m.ptr(ws), need, m.stream()) == 0
        m.synchronize()
        got = host(rt, y)
        assert not (got == POISON).any() and float(np.abs(got - want).max() / scale) <= 4 * err_ref32 + 2e-7, shape
        assert not host(rt, ws[:COUNTER_PAGE]).any()


def sk_outputs(rt):
    """act 1 and act 4 outputs of REPEAT_CASES, for the comparison across workgroup orders (a fresh process runs this again)"""
    out = []
    for shape, G in REPEAT_CASES:
        Cin, Cout, H, W = shape
        x, w, b = WC.operands(Cin, Cout, H, W, seed=5)
        xd, ud, bd = dev(rt, x), WC.pack_u(rt, w), dev(rt, b)
        out += [launch(rt, xd, ud, bd, Cout, H, W, act, env_of(G)) for act in (1, 4)]
    return out


# ------------------------------------------------------------------------------------------- status codes
def check_sk_status(rt):
    """Refused before any launch (FRCNN_ERR_INVALID, the output keeps its poison): a NULL or one-byte-short workspace where the launch
    shares a tile, a bad act, Cout % 64 != 0.  The stated workspace size is a multiple of 256 and enough under every knob setting of the
    table; exactly the counter page + 2 slots per workgroup runs."""
    L, m = rt.lib, rt.mem
    INVALID = -1
    shape, G = (68, 64, 5, 35), 10
    Cin, Cout, H, W = shape
    (x, w, b), want, err_ref32, scale = reference(shape, 1)
    xd, ud, bd = dev(rt, x), WC.pack_u(rt, w), dev(rt, b)
    yd = dev(rt, np.full((1, Cout, H, W), POISON, np.float32))
    need = slots_needed(*dims(*shape), G)
    assert need == COUNTER_PAGE + 10 * 2 * SLOT_BYTES
    ws = dev(rt, np.zeros((need,), np.uint8))

    def call(co, act, w_, nbytes):
        return L.frcnn_conv3x3_wino_sk_f32(m.ptr(xd), m.ptr(ud), m.ptr(bd), m.ptr(yd), Cin, co, H, W, act, m.ptr(w_), nbytes, m.stream())

    with tuning.override(**env_of(G)):
        assert L.frcnn_conv_wino_sk_workspace_bytes(Cin, Cout, H, W) == need
        assert call(Cout, 1, None, 0) == INVALID and call(Cout, 1, None, need) == INVALID and call(Cout, 1, ws, need - 1) == INVALID
        for act in (2, 3, 5, -1):
            assert call(Cout, act, ws, need) == INVALID, act
        assert call(96, 1, ws, need) == INVALID and call(32, 1, ws, need) == INVALID
        m.synchronize()
        assert (host(rt, yd) == POISON).all()                                         # nothing above launched anything
        assert call(Cout, 1, ws, need) == 0                                           # exactly enough: runs, and computes the convolution
        m.synchronize()
    got = host(rt, yd)
    assert not (got == POISON).any() and float(np.abs(got - want).max() / scale) <= 4 * err_ref32 + 2e-7
    assert not host(rt, ws[:COUNTER_PAGE]).any()
    with tuning.override(FRCNN_CONV_WINO_SK_G=str(dims(*shape)[0])):                  # whole tiles: no workspace needed
        yd2 = dev(rt, np.full((1, Cout, H, W), POISON, np.float32))
        assert L.frcnn_conv3x3_wino_sk_f32(m.ptr(xd), m.ptr(ud), m.ptr(bd), m.ptr(yd2), Cin, Cout, H, W, 1, None, 0, m.stream()) == 0
        m.synchronize()
        assert not (host(rt, yd2) == POISON).any()
    assert L.frcnn_conv_wino_sk_workspace_init(None, need, m.stream()) == INVALID
    assert L.frcnn_conv_wino_sk_workspace_init(m.ptr(ws), COUNTER_PAGE - 1, m.stream()) == INVALID
    assert L.frcnn_conv_wino_sk_workspace_bytes(0, 64, 5, 5) == 0
    envs = [env_of(G_) for _, G_ in TABLE] + [{"FRCNN_CONV_WINO_SK_PIECES": str(n)} for n in PIECE_COUNTS]
    for s in sorted({c[0] for c in TABLE}):
        ntiles, nchunks = dims(*s)
        for env in envs:
            with tuning.override(**env):
                stated = L.frcnn_conv_wino_sk_workspace_bytes(*s)
            assert stated >= 256 and stated % 256 == 0
            if "FRCNN_CONV_WINO_SK_PIECES" in env:
                pieces = WC.plan(rt, *s, {"FRCNN_CONV_WINO_SPLIT": env["FRCNN_CONV_WINO_SK_PIECES"]})[1]
                want_bytes = COUNTER_PAGE + ntiles * pieces * 2 * SLOT_BYTES if pieces > 1 else 0
            elif "FRCNN_CONV_WINO_SK_G" in env:
                want_bytes = slots_needed(ntiles, nchunks, int(env["FRCNN_CONV_WINO_SK_G"]))
            else:
                G_, sharers, _ = plan_of(rt, s, None)
                want_bytes = COUNTER_PAGE + G_ * 2 * SLOT_BYTES if max(sharers) > 1 else 0
            assert stated >= want_bytes, (s, env, stated, want_bytes)
        with tuning.override(FRCNN_CONV_WINO_SK_BALANCE="1"):
            assert L.frcnn_conv_wino_sk_workspace_bytes(*s) >= slots_needed(ntiles, nchunks, balanced_g(rt, *s)), s
