"""Checks of the Winograd F(2x2,3x3) fp32 convolution (csrc/conv_wino.hip), written once and run on the host emulator
(tests/test_wino_emulated.py) and on the MI355X (tests/test_gpu_winograd.py): the kernel against a float64 convolution at the shapes where
it has edges (16-byte halo groups across the right border, a ragged last K chunk, K pieces through wino_combine_kernel, the fused
ceil-mode pool, masked last rows / columns, the XCD block remap at every grid size mod 8), the exact-equality properties of its
decompositions, the weight transform bit for bit, the status codes, and U following the optimizer and load_npz.

The error bar is the project's Winograd bar with the ORACLE as comparator: max |y - ref64| / max |ref64| of the kernel is at most 4x the
same figure of the oracle's own fp32 convolution (oracle.frcnn_oracle.conv2d) on the same operands, + 2e-7."""
import os

import numpy as np

from oracle import frcnn_oracle as O
from chainer_faster_rcnn_amd import tuning
from parity_cases import dev, host

POISON = np.float32(-12345.0)          # the value HostMemory.empty fills with; the checks fill their outputs with it on either runtime

# Cin, Cout, H, W
EDGE_SHAPES = [
    (8, 64, 5, 33),            # two x tiles, W % 4 = 1
    (12, 64, 7, 37),           # ragged Cin for CK = 8
    (16, 128, 9, 34),          # two cout blocks, W % 4 = 2, odd H under pooling
    (20, 64, 3, 67),           # three x tiles, W % 4 = 3
    (64, 64, 6, 31),           # natural split on the 3-CU emulated chip
    (68, 64, 5, 35),           # ragged Cin and split
    (100, 64, 23, 37),         # ragged Cin, six y tiles
    (5, 64, 1, 1),             # smallest map
    (4, 64, 2, 2),             # smallest map
    (9, 192, 13, 97),          # three cout blocks, odd Cin (ragged for CK = 8 and CK = 4), 48 workgroups
    # the remaining grid sizes mod 8 of the XCD remap (unsplit: 5, 6, 7 workgroups; the table above gives 0 .. 4)
    (8, 64, 18, 30),           # 1 x 5 tiles
    (16, 64, 10, 40),          # 2 x 3 tiles, W % 4 = 0 (no border fix)
    (24, 64, 26, 21),          # 1 x 7 tiles, W % 4 = 1
]
PACKED_SHAPES = {(20, 64, 3, 67)}      # U built from the packed (Cin * 9, Cout) weights, as after an optimizer step

ENVS = [
    {},
    {"FRCNN_CONV_WINO_CFG": "2"},
    {"FRCNN_CONV_WINO_SPLIT": "2"},
    {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "3"},
]


def env_id(env):
    return "-".join("%s%s" % (k.replace("FRCNN_CONV_WINO_", "").lower(), v) for k, v in sorted(env.items())) or "default"


def shape_id(s):
    return "%d-%d_%dx%d" % tuple(s)


# ------------------------------------------------------------------------------------------- the launch plan, restated
def cu_count(rt):
    """compute units the library sees: the emulated chip's (HIPEMU_CUS, default 3) or the device's"""
    if rt.lib.frcnn_device_count() == 0:
        return int(os.environ.get("HIPEMU_CUS", "0")) or 3
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def plan(rt, Cin, Cout, H, W, env):
    """(cfg, pieces, workgroups) of the launch frcnn_conv3x3_wino_f32 makes under `env`, from the rule in the kernel file's comments:
    64 couts x 4 rows x 32 columns per workgroup, CK = 8 (cfg 1) or 4 (cfg 2) channels per chunk; K pieces forced by
    FRCNN_CONV_WINO_SPLIT, else enough for about two workgroups per CU slot (two slots per CU) with pieces of at least four chunks;
    never more pieces than chunks, and no empty piece."""
    cfg = int(env.get("FRCNN_CONV_WINO_CFG", 1))
    ck = 8 if cfg == 1 else 4
    ntiles = -(-W // 32) * -(-H // 4) * (Cout // 64)
    nchunks = -(-Cin // ck)
    forced = int(env.get("FRCNN_CONV_WINO_SPLIT", 0))
    if forced > 0:
        pieces = forced
    else:
        slots = cu_count(rt) * 2
        pieces = 1 if ntiles >= 2 * slots else min(-(-2 * slots // ntiles), max(nchunks // 4, 1))
    pieces = max(1, min(pieces, nchunks))
    pieces = -(-nchunks // -(-nchunks // pieces))
    return cfg, pieces, ntiles * pieces


# ------------------------------------------------------------------------------------------- operands and references
def operands(Cin, Cout, H, W, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((1, Cin, H, W)).astype(np.float32)                       # negative values stay in
    w = (rs.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = (0.1 * rs.standard_normal(Cout)).astype(np.float32)
    return x, w, b


def ref64(x, w, b, act):
    """float64 convolution of the fp32 operands (+ ReLU for act 1 / 4, + the 2x2/2 ceil-mode max-pool for act 4)"""
    import torch
    F = torch.nn.functional
    y = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)
    if act in (1, 4):
        y = torch.relu(y)
    if act == 4:
        y = F.max_pool2d(y, 2, 2, ceil_mode=True)
    return y.numpy()


def ref32(x, w, b, act):
    """the oracle's own fp32 convolution, the comparator of the bar"""
    y = O.conv2d(x, w, b, 1)
    if act in (1, 4):
        y = O.relu(y)
    if act == 4:
        y = O.max_pool_2x2(y)
    return y


def out_shape(Cout, H, W, act):
    return (1, Cout, (H + 1) // 2, (W + 1) // 2) if act == 4 else (1, Cout, H, W)


def pack_u(rt, w, packed=False):
    """U on the device from (Cout, Cin, 3, 3) weights; packed: through frcnn_pack_conv3x3_w's (Cin * 9, Cout) layout, the form a trainer's
    live weights have"""
    wd = dev(rt, w)
    return rt.pack_wino_w(rt.pack_conv3x3_w(wd) if packed else wd)


def launch(rt, xd, ud, bd, Cout, H, W, act, env):
    """one frcnn_conv3x3_wino_f32 under `env` into an output pre-filled with the poison value -> host array"""
    y = dev(rt, np.full(out_shape(Cout, H, W, act), POISON, np.float32))
    with tuning.override(**env):
        rt.conv3x3_wino(xd, ud, bd, act=act, out=y)
    return host(rt, y)


RATIOS = []          # (shape, act, env id, err_wino, err_ref32) of every check_wino_vs_float64 of this process: the suites print the range


def check_wino_vs_float64(rt, Cin, Cout, H, W, act, env, packed=False, seed=0):
    """The kernel under `env` against the float64 convolution: err_wino <= 4 * err_ref32 + 2e-7 (both max |delta| / max |ref64|; err_ref32
    is the oracle's fp32 convolution on the same operands), the output shape, and no element left unwritten.  Returns the output."""
    x, w, b = operands(Cin, Cout, H, W, seed)
    got = launch(rt, dev(rt, x), pack_u(rt, w, packed), dev(rt, b), Cout, H, W, act, env)
    want = ref64(x, w, b, act)
    assert got.shape == want.shape == out_shape(Cout, H, W, act), (got.shape, want.shape)
    assert not (got == POISON).any(), "%d output elements were never written" % int((got == POISON).sum())
    assert np.isfinite(got).all()
    scale = np.abs(want).max()
    assert scale > 0
    err_wino = float(np.abs(got - want).max() / scale)
    err_ref32 = float(np.abs(ref32(x, w, b, act) - want).max() / scale)
    RATIOS.append(((Cin, Cout, H, W), act, env_id(env), err_wino, err_ref32))
    print("WINO %s act %d %s: wino %.3e ref32 %.3e ratio %.2f" % (shape_id((Cin, Cout, H, W)), act, env_id(env), err_wino, err_ref32,
                                                                 err_wino / max(err_ref32, 1e-30)))
    assert err_wino <= 4 * err_ref32 + 2e-7, ((Cin, Cout, H, W), act, env, err_wino, err_ref32)
    return got


def check_wino_shape(rt, shape, env, seed=0):
    """One shape under one environment at act 0, 1 and 4 against float64; act 1 is exactly ReLU of act 0 (the same sums), and act 4 is
    exactly act 1 followed by maxpool2x2 -- in the main kernel's epilogue, and in wino_combine_kernel when the launch is split."""
    Cin, Cout, H, W = shape
    packed = tuple(shape) in PACKED_SHAPES
    y0, y1, y4 = [check_wino_vs_float64(rt, Cin, Cout, H, W, act, env, packed=packed, seed=seed) for act in (0, 1, 4)]
    assert np.array_equal(np.maximum(y0, 0), y1)
    assert np.array_equal(host(rt, rt.maxpool2x2(dev(rt, y1))), y4)
    return y0, y1, y4


def check_wino_cfg_identical(rt, shape, seed=0):
    """Unsplit, 8- and 4-channel chunks give identical bits: the chunk size does not change the order of the K sum."""
    Cin, Cout, H, W = shape
    x, w, b = operands(Cin, Cout, H, W, seed)
    xd, ud, bd = dev(rt, x), pack_u(rt, w), dev(rt, b)
    for act in (0, 4):
        a = launch(rt, xd, ud, bd, Cout, H, W, act, {"FRCNN_CONV_WINO_SPLIT": "1", "FRCNN_CONV_WINO_CFG": "1"})
        c = launch(rt, xd, ud, bd, Cout, H, W, act, {"FRCNN_CONV_WINO_SPLIT": "1", "FRCNN_CONV_WINO_CFG": "2"})
        assert not (a == POISON).any() and np.array_equal(a, c), (shape, act)


def fill_workspace_nan(rt):
    """every byte of the runtime's Winograd workspace 0xFF: every float of it a NaN"""
    ws = rt.workspace("conv_wino", 1)          # the buffer the launches so far have grown: conv3x3_wino hands it out again
    ws[...] = 0xFF
    assert np.isnan(host(rt, rt.mem.bitcast(ws[:256], "f32"))).all()
    return ws


def check_wino_split_repeats(rt, shape, env, seed=0):
    """A split launch three times over gives identical bits (the combine kernel adds the slabs in piece order), and so does one whose
    workspace holds NaN everywhere beforehand: the workspace needs no initialisation."""
    Cin, Cout, H, W = shape
    assert plan(rt, Cin, Cout, H, W, env)[1] > 1, "this case must split"
    x, w, b = operands(Cin, Cout, H, W, seed)
    xd, ud, bd = dev(rt, x), pack_u(rt, w), dev(rt, b)
    for act in (1, 4):
        first = launch(rt, xd, ud, bd, Cout, H, W, act, env)
        assert not (first == POISON).any()
        for _ in range(2):
            assert np.array_equal(launch(rt, xd, ud, bd, Cout, H, W, act, env), first)
        fill_workspace_nan(rt)
        again = launch(rt, xd, ud, bd, Cout, H, W, act, env)
        assert np.isfinite(again).all() and np.array_equal(again, first), (shape, act, env)


SPLIT_CASES = [((68, 64, 5, 35), {"FRCNN_CONV_WINO_SPLIT": "3"}), ((100, 64, 23, 37), {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "4"})]


def split_outputs(rt):
    """the act 1 and act 4 outputs of SPLIT_CASES, for the comparison across workgroup orders (a fresh process runs this again)"""
    out = []
    for shape, env in SPLIT_CASES:
        Cin, Cout, H, W = shape
        x, w, b = operands(Cin, Cout, H, W, seed=5)
        xd, ud, bd = dev(rt, x), pack_u(rt, w), dev(rt, b)
        out += [launch(rt, xd, ud, bd, Cout, H, W, act, env) for act in (1, 4)]
    return out


# ------------------------------------------------------------------------------------------- the weight transform
def u_float64(w):
    """U = G g G^T of (Cout, Cin, 3, 3) fp32 weights in float64, in wino_pack_w_kernel's operation order, rounded once to fp32:
    (Cout, Cin, 4 rows, 4 columns)"""
    g = w.astype(np.float64)
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]                                     # (Cout, Cin, 3 rows): g G^T, column k of every row
    gg = np.stack([g0, 0.5 * ((g0 + g1) + g2), 0.5 * ((g0 - g1) + g2), g2], axis=-1)  # (Cout, Cin, 3, 4)
    r0, r1, r2 = gg[:, :, 0], gg[:, :, 1], gg[:, :, 2]                               # (Cout, Cin, 4)
    u = np.stack([r0, 0.5 * ((r0 + r1) + r2), 0.5 * ((r0 - r1) + r2), r2], axis=2)   # (Cout, Cin, 4 r, 4 k)
    return u.astype(np.float32)


def check_wino_pack(rt, shapes=((64, 4), (128, 12), (64, 100)), seed=0):
    """frcnn_wino_pack_w bit for bit against the float64 evaluation, from both weight layouts, with filters whose nine taps span
    1e-20 .. 1e3, and the [Cin][4][Cout][4] layout spelled out."""
    for Cout, Cin in shapes:
        rs = np.random.RandomState(seed + Cout + Cin)
        w = (rs.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
        mags = np.array([1e-20, 1e-12, 1e-6, 1e-3, 1.0, 7.0, 1e2, 1e3, 3e-9], np.float32).reshape(3, 3)
        w[1, 0] = mags * np.where(rs.rand(3, 3) < 0.5, -1, 1)                        # mixed magnitudes inside one filter
        w[Cout - 1, Cin - 1] = mags.T[::-1] * rs.standard_normal((3, 3)).astype(np.float32)
        want = u_float64(w)
        assert np.isfinite(want).all() and np.abs(want[1, 0]).max() > 100 and 0 < np.abs(want[1, 0]).min() < 1e-19
        wd = dev(rt, w)
        u0 = host(rt, rt.pack_wino_w(wd))
        wp = rt.pack_conv3x3_w(wd)
        assert tuple(wp.shape) == (Cin * 9, Cout)
        u1 = host(rt, rt.pack_wino_w(wp))
        assert u0.shape == (Cin * 16, Cout) and u0.dtype == np.float32
        assert np.array_equal(u0.view(np.uint32), u1.view(np.uint32)), (Cout, Cin)                  # packed = 0 and packed = 1: the same U
        got = u0.reshape(Cin, 4, Cout, 4)                                                             # [ci][r][co][k]
        assert np.array_equal(got.transpose(2, 0, 1, 3).view(np.uint32), want.view(np.uint32)), (Cout, Cin)
        for co, ci, r, k in ((0, 0, 0, 0), (1, 0, 1, 2), (1, 0, 2, 1), (Cout - 1, Cin - 1, 3, 3), (Cout // 2, Cin // 2, 2, 3), (1, 0, 3, 0)):
            assert got[ci, r, co, k] == want[co, ci, r, k], (co, ci, r, k)
        # corner components are the corner taps themselves, and an existing U is rewritten in place
        assert np.array_equal(got[:, 0, :, 0].T, w[:, :, 0, 0]) and np.array_equal(got[:, 3, :, 0].T, w[:, :, 2, 0]) and np.array_equal(got[:, 0, :, 3].T, w[:, :, 0, 2])
        ud = dev(rt, np.full((Cin * 16, Cout), POISON, np.float32))
        assert rt.pack_wino_w(wp, out=ud) is ud and np.array_equal(host(rt, ud), u0)


# ------------------------------------------------------------------------------------------- status codes
def check_wino_status(rt):
    """What frcnn_conv3x3_wino_f32 / frcnn_wino_pack_w refuse (FRCNN_ERR_INVALID, before any launch: the output keeps its poison), and the
    workspace size frcnn_conv_wino_workspace_bytes states against what the launches of the edge table really take."""
    L, m = rt.lib, rt.mem
    INVALID = -1
    Cin, Cout, H, W = 16, 64, 5, 9
    x, w, b = operands(Cin, Cout, H, W, seed=3)
    xd, ud, bd = dev(rt, x), pack_u(rt, w), dev(rt, b)
    yd = dev(rt, np.full((1, 128, H, W), POISON, np.float32))
    big = dev(rt, np.zeros((1 << 16,), np.uint8))

    def call(ci, co, h, wd_, act, ws, ws_bytes):
        return L.frcnn_conv3x3_wino_f32(m.ptr(xd), m.ptr(ud), m.ptr(bd), m.ptr(yd), ci, co, h, wd_, act, m.ptr(ws), ws_bytes, m.stream())

    assert call(Cin, 96, H, W, 1, big, big.shape[0]) == INVALID                       # Cout % 64 != 0
    assert call(Cin, 32, H, W, 1, big, big.shape[0]) == INVALID
    for act in (2, 3, 5, -1):                                                         # the kernel has acts 0, 1 and 4
        assert call(Cin, Cout, H, W, act, big, big.shape[0]) == INVALID, act
    assert call(0, Cout, H, W, 1, big, big.shape[0]) == INVALID and call(Cin, Cout, 0, W, 1, big, big.shape[0]) == INVALID
    # 32-bit buffer offsets: an input of 2 GiB, and a U of 2 GiB, are refused (tiny real buffers: the call returns before it launches)
    assert call(8, Cout, 8192, 8192, 1, big, big.shape[0]) == INVALID
    assert call(2, Cout, 16384, 16384, 0, big, big.shape[0]) == INVALID
    assert call(32768, 1024, 1, 1, 1, big, big.shape[0]) == INVALID
    # a forced split without the room for its slabs
    need = 2 * Cout * H * W * 4
    with tuning.override(FRCNN_CONV_WINO_SPLIT="2"):
        assert plan(rt, Cin, Cout, H, W, {"FRCNN_CONV_WINO_SPLIT": "2"})[1] == 2
        assert call(Cin, Cout, H, W, 1, None, 0) == INVALID
        assert call(Cin, Cout, H, W, 1, None, need) == INVALID
        assert call(Cin, Cout, H, W, 1, big, need - 1) == INVALID
        m.synchronize()
        assert (host(rt, yd) == POISON).all()                                         # nothing above launched anything
        assert call(Cin, Cout, H, W, 1, big, need) == 0                               # exactly enough: runs, and computes the convolution
        m.synchronize()
    got = host(rt, yd).reshape(-1)[:Cout * H * W].reshape(1, Cout, H, W)
    want = ref64(x, w, b, 1)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max() and (host(rt, yd).reshape(-1)[Cout * H * W:] == POISON).all()
    with tuning.override(FRCNN_CONV_WINO_SPLIT="1"):
        assert call(Cin, Cout, H, W, 1, None, 0) == 0                                 # unsplit: no workspace needed
        m.synchronize()
    # frcnn_wino_pack_w: packed is 0 or 1
    wd = dev(rt, w)
    u2 = dev(rt, np.full((Cin * 16, Cout), POISON, np.float32))
    for packed in (2, -1):
        assert L.frcnn_wino_pack_w(m.ptr(wd), Cout, Cin, packed, m.ptr(u2), m.stream()) == INVALID
    assert L.frcnn_wino_pack_w(None, Cout, Cin, 0, m.ptr(u2), m.stream()) == INVALID and L.frcnn_wino_pack_w(m.ptr(wd), Cout, 0, 0, m.ptr(u2), m.stream()) == INVALID
    m.synchronize()
    assert (host(rt, u2) == POISON).all()
    # the stated workspace covers the slabs of the pieces each launch takes, under every knob setting of the set ...
    for shape in EDGE_SHAPES:
        ci, co, h, wd_ = shape
        for env in ENVS + [{"FRCNN_CONV_WINO_SPLIT": "1"}, {"FRCNN_CONV_WINO_SPLIT": "64"}, {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "64"}]:
            pieces = plan(rt, ci, co, h, wd_, env)[1]
            with tuning.override(**env):
                stated = L.frcnn_conv_wino_workspace_bytes(ci, co, h, wd_)
            assert stated >= 256 and stated % 256 == 0
            if pieces > 1:
                assert stated >= pieces * co * h * wd_ * 4, (shape, env, pieces, stated)
    assert L.frcnn_conv_wino_workspace_bytes(0, 64, 5, 5) == 0
    # ... and `pieces` above IS what the launch takes: one byte less than its slabs is refused, the slabs themselves are enough
    for shape, env in (((68, 64, 5, 35), {}), ((68, 64, 5, 35), ENVS[3]), ((100, 64, 23, 37), ENVS[2]), ((9, 192, 13, 97), {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "64"})):
        ci, co, h, wd_ = shape
        pieces = plan(rt, ci, co, h, wd_, env)[1]
        x2, w2, b2 = operands(ci, co, h, wd_, seed=4)
        x2d, u2d, b2d = dev(rt, x2), pack_u(rt, w2), dev(rt, b2)
        y2 = dev(rt, np.full((1, co, h, wd_), POISON, np.float32))
        need = pieces * co * h * wd_ * 4
        ws = dev(rt, np.zeros((max(need, 256),), np.uint8))
        with tuning.override(**env):
            if pieces > 1:
                assert L.frcnn_conv3x3_wino_f32(m.ptr(x2d), m.ptr(u2d), m.ptr(b2d), m.ptr(y2), ci, co, h, wd_, 0, m.ptr(ws), need - 1, m.stream()) == INVALID
                m.synchronize()
                assert (host(rt, y2) == POISON).all()
            assert L.frcnn_conv3x3_wino_f32(m.ptr(x2d), m.ptr(u2d), m.ptr(b2d), m.ptr(y2), ci, co, h, wd_, 0, m.ptr(ws), need if pieces > 1 else 0, m.stream()) == 0
            m.synchronize()
        want = ref64(x2, w2, b2, 0)
        assert np.abs(host(rt, y2) - want).max() <= 1e-5 * np.abs(want).max(), (shape, env)


# ------------------------------------------------------------------------------------------- U follows the parameters
def small_full_model(rt, seed=0, trunk_seed=1):
    """the narrow two-pool FasterRCNN of the training tests (train_cases.SMALL_LAYERS): conv2_1, conv2_2 and rpn_conv_3x3 carry U"""
    import functools
    import train_cases as T
    from chainer_faster_rcnn_amd.models import FasterRCNN, VGG16Prev
    params = T.small_params(seed=trunk_seed)
    params.update(T.small_head_params(np.random.RandomState(seed)))
    model = FasterRCNN(trunk_class=functools.partial(VGG16Prev, layers=T.SMALL_LAYERS), rpn_in_ch=64, rpn_mid_ch=64, feat_stride=4,
                       anchor_scales=(2, 4, 8), runtime=rt)
    model.load_params(params)
    model.RPN.proposal_layer.RPN_MIN_SIZE = 4
    model.RPN.proposal_layer._min_size = 4
    return model, params


WINO_LINKS = ("conv2_1", "conv2_2", "rpn_conv_3x3")
KEPT = ("feat", "rpn_h", "rpn_cls_prob", "rpn_bbox_pred", "rois", "probs", "n_out", "pool5", "fc6", "fc7", "cls_prob", "pred_boxes")


def check_wino_derived(rt, variant, tmp_dir):
    """After an optimizer step ("rpn": one RPNTrainer step, "rcnn": one RCNNTrainer step, both lr 0.05) or a load_npz of other weights
    ("load"), the fp32 inference forward -- conv2_1, conv2_2 and rpn_conv_3x3 through Winograd -- runs on the NEW weights: bit-identical
    to a fresh model loaded with the model's parameters, different from before, and its feature map within 1e-5 of the direct kernels'."""
    import parity_cases as P
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.serializers import load_npz, namedparams, save_npz
    from chainer_faster_rcnn_amd.train import RCNNTrainer, RPNTrainer
    h, w = 40, 56
    rs = np.random.RandomState(0)
    x = rs.randn(1, 3, h, w).astype(np.float32)
    gt = P.gt_case(rs, 2, h, w)
    gt[0, :, 2] = np.minimum(gt[0, :, 0] + 20, w - 1); gt[0, :, 3] = np.minimum(gt[0, :, 1] + 20, h - 1)
    info = np.array([[h, w]], dtype=np.int32)
    xd = dev(rt, x)

    def links(model):
        return [model.trunk.links["conv2_1"], model.trunk.links["conv2_2"], model.RPN.rpn_conv_3x3]

    def forward(model):
        assert all(l.wino_applies() for l in links(model)) and not model.trunk.links["conv1_1"].wino_applies()
        out = model.forward_device(xd, h, w, keep=True)
        rt.mem.synchronize()
        return {k: host(rt, out[k]).copy() for k in KEPT}

    model, _ = small_full_model(rt)
    before = forward(model)
    u_before = [host(rt, l.Wu).copy() for l in links(model)]
    if variant == "rpn":
        model.rpn_train = True
        tr = RPNTrainer(model, lr=0.05)
        np.random.seed(0)
        tr.step(Variable(x), Variable(info), Variable(gt))
        model.rpn_train = False
    elif variant == "rcnn":
        model.rcnn_train = True
        tr = RCNNTrainer(model, lr=0.05)
        np.random.seed(0)
        tr.step(Variable(x), Variable(info), Variable(gt))
        model.rcnn_train = False
    else:
        assert variant == "load"
        other, _ = small_full_model(rt, seed=7, trunk_seed=5)
        path = os.path.join(str(tmp_dir), "other.npz")
        save_npz(path, other)
        load_npz(path, model)
    after = forward(model)
    trained = {k: host(rt, rt.mem.contiguous(v)) for k, v in namedparams(model)}
    fresh, _ = small_full_model(rt)
    fresh.load_params(trained)
    want = forward(fresh)
    for k in KEPT:
        assert after[k].shape == want[k].shape and np.array_equal(after[k], want[k]), (variant, k)
    changed = ("conv2_1", "conv2_2") if variant == "rcnn" else WINO_LINKS          # (stage 2 leaves the RPN's convolution alone)
    for name, l, f, ub in zip(WINO_LINKS, links(model), links(fresh), u_before):
        assert np.array_equal(host(rt, l.Wu), host(rt, f.Wu)), (variant, name)    # U itself: rebuilt from the live packed weights
        if name in changed:
            assert not np.array_equal(host(rt, l.Wu), ub), (variant, name)
    assert not np.array_equal(after["feat"], before["feat"]) and not np.array_equal(after["rpn_h"], before["rpn_h"])
    assert not np.array_equal(after["cls_prob"], before["cls_prob"])
    with tuning.override(FRCNN_CONV_WINO="0"):
        assert not any(l.wino_applies() for l in links(model))
        direct = model.forward_device(xd, h, w, keep=True)
        rt.mem.synchronize()
        fd = host(rt, direct["feat"])
    assert np.abs(after["feat"] - fd).max() <= 1e-5 * np.abs(fd).max(), np.abs(after["feat"] - fd).max() / np.abs(fd).max()


def ratio_summary():
    """(count, smallest, largest) err_wino / err_ref32 over the checks of this process whose oracle error is not zero"""
    r = [ew / er for _, _, _, ew, er in RATIOS if er > 0]
    return (len(r), min(r), max(r)) if r else (0, 0.0, 0.0)
