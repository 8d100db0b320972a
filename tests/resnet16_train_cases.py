"""Checks of the ResNet trunk's bf16 train-mode pass (csrc/conv1x1_train_bf16.hip, models/resnet.py ResNet(train_dtype="bf16"), both trainers on such a
model), written once and run on the host emulator (tests/test_resnet16_train_emulated.py) and on the MI355X (tests/test_gpu_resnet16_train.py).

Kernel level: the three 1x1 entries against float64 products of the ROUND-TO-NEAREST-EVEN images of their fp32 operands (bf16_train_cases.rne), so the
kernel is judged on its summation alone -- a product of two bf16 values is exact in fp32.  Bounds (max-abs error over the result's max-abs): 1e-5 for the
forward pass and the input gradient (bf16_train_cases.check_conv3x3_bf16_train's tol), 1e-4 for the weight gradient -- one sequential fp32
chain of 16-product steps measured 5.1e-7 at K = 2048, 1.8e-6 at K = 37 500 and 3.2e-6 at K = 150 000 unsplit.  A truncating conversion
misses them by two orders of magnitude.  Trunk level: the step is checked LAYER BY LAYER on the device's own tensors (every product against float64 of
the rounded tensors the device fed it, every BatchNormalization against bn_reference on the device's own z / dy, every glue step bit for bit), which pins
the whole pass without depending on where a float64 pass would round an activation to another bf16 value."""
import functools

import numpy as np

import resnet_train_cases as T
from bf16_train_cases import rne
from parity_cases import dev, host

TOL_FWD, TOL_WGRAD = 1e-5, 1e-4
# (Cin, Cout, HW): a K tail below 16, one and several pixel tiles, one and several cout tiles, odd HW, the stem's 152 rows
EMU_SHAPES = [(1, 1, 1), (24, 64, 35), (64, 64, 257), (152, 64, 300), (64, 256, 255), (256, 64, 130), (80, 48, 97)]
# one shape per class of the real network at 600 x 1000 (scripts/resnet16_train_micro.py times the same list)
REAL_SHAPES = [(152, 64, 150000), (64, 256, 37500), (256, 64, 37500), (512, 128, 9375), (1024, 256, 2394), (256, 1024, 2394), (2048, 512, 608),
               (512, 2048, 608)]
SPLITS = (None, 1, 2, 3, 8, 20)         # None: the launcher's own choice; 20: a weight gradient past its in-launch limit goes through slabs
COUNTER_PAGE = 64 * 1024


def _maxabs(a):
    return float(np.abs(a).max())


def _nerr(got, want):
    return _maxabs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / max(_maxabs(want), 1e-30)


def _forced(split):
    from chainer_faster_rcnn_amd import tuning
    if split is None:
        return tuning.override(FRCNN_C1T_SPLIT=None, FRCNN_C1T_WGRAD_SPLITS=None)
    return tuning.override(FRCNN_C1T_SPLIT=str(split), FRCNN_C1T_WGRAD_SPLITS=str(split))


def _counter_page_zero(rt):
    rt.mem.synchronize()
    return not host(rt, rt._ws["conv1x1_train"])[:COUNTER_PAGE].any()


def run_entries(rt, x, w, dz, b):
    """-> host arrays (z with bias, z without, dx, dW) of one call each"""
    xd, wd, dzd = dev(rt, x), dev(rt, w), dev(rt, dz)
    out = (rt.conv1x1_bf16_train(xd, wd, dev(rt, b)), rt.conv1x1_bf16_train(xd, wd), rt.conv1x1_dgrad_bf16(dzd, wd), rt.conv1x1_wgrad_bf16(xd, dzd))
    return [host(rt, a) for a in out]


def products64(x, w, dz, b):
    """float64 of the three products on the given (already rounded) operands: (z + b, z, dx, dW) as flat-pixel matrices"""
    X, W, DZ = [np.asarray(a, np.float64) for a in (x.reshape(x.shape[1], -1), w, dz.reshape(dz.shape[1], -1))]
    z = W.T @ X
    return z + np.asarray(b, np.float64)[:, None], z, W @ DZ, X @ DZ.T


def check_float64(rt, cin, cout, hw, seed=0):
    """all three entries, each launched twice (identical bits), against float64 on RNE operands; the forward entry with a bias and with NULL.
    x is post-ReLU (half zeros), dz small, as in a step.  -> the three errors (forward, input gradient, weight gradient)"""
    rs = np.random.RandomState(seed + cin + 7 * cout + hw)
    x = np.maximum(rs.randn(1, cin, 1, hw), 0).astype(np.float32)
    w = (rs.randn(cin, cout) * np.sqrt(2.0 / cin)).astype(np.float32)
    dz = (rs.randn(1, cout, 1, hw) * 1e-2).astype(np.float32)
    b = (rs.randn(cout) * 0.1).astype(np.float32)
    a, a2 = run_entries(rt, x, w, dz, b), run_entries(rt, x, w, dz, b)
    for u, v in zip(a, a2):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), "two calls on the same inputs differ"
    want = products64(rne(x), rne(w), rne(dz), b)
    assert a[0].shape == (1, cout, 1, hw) and a[2].shape == (1, cin, 1, hw) and a[3].shape == (cin, cout)
    errs = [_nerr(g.reshape(r.shape), r) for g, r in zip(a, want)]
    print("C1T_ERR (%d,%d,%d) fwd+b %.2e fwd %.2e dgrad %.2e wgrad %.2e" % ((cin, cout, hw) + tuple(errs)))
    assert errs[0] <= TOL_FWD and errs[1] <= TOL_FWD and errs[2] <= TOL_FWD and errs[3] <= TOL_WGRAD, errs
    assert _maxabs(want[1]) > 0 and _maxabs(want[2]) > 0 and _maxabs(want[3]) > 0
    # RNE, not truncation: the same float64 products on TRUNCATED operands are far outside the bound (where there are enough terms to tell)
    if cin >= 24 and hw >= 35:
        trunc = lambda t: (np.ascontiguousarray(t, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)      # noqa: E731
        wrong = products64(trunc(x), trunc(w), trunc(dz), b)
        assert _nerr(wrong[1], want[1]) > 10 * TOL_FWD and _nerr(wrong[3], want[3]) > 10 * TOL_WGRAD
    assert _counter_page_zero(rt)
    return errs[1], errs[2], errs[3]


def check_exact(rt, cin, cout, hw, seed=1):
    """operands are small integers times powers of two (bf16 values; every product and every partial sum is exact in fp32): the result equals
    float64 BIT FOR BIT at every forced split count and at the default, and the counter page reads zero after every launch"""
    rs = np.random.RandomState(seed + cin + 7 * cout + hw)
    x = (rs.randint(-3, 4, (1, cin, 1, hw)) * 0.5).astype(np.float32)
    w = (rs.randint(-2, 3, (cin, cout)) * 0.25).astype(np.float32)
    dz = (rs.randint(-3, 4, (1, cout, 1, hw)) * 2.0).astype(np.float32)
    b = (rs.randint(-4, 5, cout) * 0.125).astype(np.float32)
    want = [r.astype(np.float32) for r in products64(x, w, dz, b)]
    assert all(np.array_equal(r.astype(np.float64), r64) for r, r64 in zip(want, products64(x, w, dz, b)))      # representable: nothing was rounded
    from chainer_faster_rcnn_amd import tuning
    for mt in (None, "4"):                                           # the launcher's tile, and the 128-row tile it keeps for very large launches
        for split in SPLITS:
            with _forced(split), tuning.override(FRCNN_C1T_MT=mt):
                got = run_entries(rt, x, w, dz, b)
                for name, g, r in zip(("fwd+b", "fwd", "dgrad", "wgrad"), got, want):
                    assert np.array_equal(g.reshape(r.shape).view(np.uint32), r.view(np.uint32)), (name, (cin, cout, hw), split, mt)
                assert _counter_page_zero(rt), (split, mt)


def check_refusals(rt):
    """a NULL required pointer, a dimension < 1, an operand of 2^31 bytes or more, a NULL or too small workspace: FRCNN_ERR_INVALID from each entry,
    sentinel-filled outputs unwritten; then the valid calls return 0"""
    L, m = rt.lib, rt.mem
    ci, co, hw = 24, 40, 33
    a = lambda *s: dev(rt, np.full(s, 7.0, np.float32))                                              # noqa: E731
    x, w, dz, b, z, dx, dw = a(ci, hw), a(ci, co), a(co, hw), a(co), a(co, hw), a(ci, hw), a(ci, co)
    sizes = [f(ci, co, hw) for f in (L.frcnn_conv1x1_fwd_bf16_train_workspace_bytes, L.frcnn_conv1x1_dgrad_bf16_workspace_bytes,
                                     L.frcnn_conv1x1_wgrad_bf16_workspace_bytes)]
    assert all(s >= COUNTER_PAGE for s in sizes)
    for f in (L.frcnn_conv1x1_fwd_bf16_train_workspace_bytes, L.frcnn_conv1x1_dgrad_bf16_workspace_bytes, L.frcnn_conv1x1_wgrad_bf16_workspace_bytes):
        assert f(0, co, hw) == 0 and f(ci, -1, hw) == 0 and f(ci, co, 0) == 0 and f(1, 1, 1 << 29) == 0
    ws = m.zeros((max(sizes),), "u8")
    P, S = m.ptr, m.stream()

    def fwd(x_=x, w_=w, z_=z, ci_=ci, co_=co, hw_=hw, ws_=ws, n=sizes[0]):
        return L.frcnn_conv1x1_fwd_bf16_train(P(x_), P(w_), P(b), P(z_), ci_, co_, hw_, P(ws_), n, S)

    def dgr(dz_=dz, w_=w, dx_=dx, ci_=ci, co_=co, hw_=hw, ws_=ws, n=sizes[1]):
        return L.frcnn_conv1x1_dgrad_bf16(P(dz_), P(w_), P(dx_), ci_, co_, hw_, P(ws_), n, S)

    def wgr(x_=x, dz_=dz, dw_=dw, ci_=ci, co_=co, hw_=hw, ws_=ws, n=sizes[2]):
        return L.frcnn_conv1x1_wgrad_bf16(P(x_), P(dz_), P(dw_), ci_, co_, hw_, P(ws_), n, S)
    big = 1 << 29                                                   # x 4 bytes = 2^31
    bad = [fwd(x_=None), fwd(w_=None), fwd(z_=None), fwd(ci_=0), fwd(co_=0), fwd(hw_=0), fwd(hw_=-5), fwd(ws_=None), fwd(n=sizes[0] - 1), fwd(n=0),
           fwd(ci_=1, co_=1, hw_=big), fwd(ci_=big, co_=1, hw_=1), fwd(ci_=1 << 15, co_=1 << 14, hw_=1),
           dgr(dz_=None), dgr(w_=None), dgr(dx_=None), dgr(ci_=0), dgr(co_=-1), dgr(hw_=0), dgr(ws_=None), dgr(n=sizes[1] - 1),
           dgr(ci_=1, co_=1, hw_=big), dgr(ci_=1, co_=big, hw_=1),
           wgr(x_=None), wgr(dz_=None), wgr(dw_=None), wgr(ci_=0), wgr(co_=0), wgr(hw_=-1), wgr(ws_=None), wgr(n=sizes[2] - 1),
           wgr(ci_=1, co_=1, hw_=big), wgr(ci_=1 << 15, co_=1 << 14, hw_=1)]
    assert all(v == -1 for v in bad), bad
    m.synchronize()
    for t in (z, dx, dw):
        assert (host(rt, t) == 7.0).all()                                                            # nothing was launched
    assert fwd() == 0 and dgr() == 0 and wgr() == 0
    m.synchronize()
    assert not (host(rt, z) == 7.0).all() and not (host(rt, dx) == 7.0).all() and not (host(rt, dw) == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------ trunk level
def trunk_case(rt, blocks, im_h, im_w, seed, **kw):
    """resnet_train_cases.trunk_case with ResNet keywords"""
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import ResNet
    params = synthetic.resnet_params(seed=seed, blocks=blocks, base_width=T.NARROW)
    params["trunk/conv1/b"] = (np.random.RandomState(seed + 50).randn(T.NARROW) * 0.1).astype(np.float32)
    x = synthetic.image(seed=6, h=im_h, w=im_w) / 64.0
    model = ResNet(runtime=rt, blocks=blocks, base_width=T.NARROW, **kw)
    model.load_params(params)
    model.train = True
    return params, x, model


def _conv3x3_64(x, w_packed, dz):
    """float64 3x3 / pad 1: (z, dW packed like pack_w, dx) of the given operands through torch autograd"""
    import torch
    from chainer_faster_rcnn_amd.models.resnet import pack_w, unpack_w
    ci, co = x.shape[1], w_packed.shape[1]
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    wt = torch.from_numpy(np.asarray(unpack_w(w_packed, co, ci, 3), np.float64)).requires_grad_(True)
    z = torch.nn.functional.conv2d(xt, wt, padding=1)
    (z * torch.from_numpy(np.asarray(dz, np.float64))).sum().backward()
    dw = wt.grad.numpy()
    return z.detach().numpy(), np.ascontiguousarray(dw.reshape(co, -1).T), xt.grad.numpy()


def _bn_check(name, t, tp, res, dy, dz, dgamma, dbeta, rt):
    """one BatchNormalization of the tape, forward and backward, against bn_reference on the device's own z / dy under the fp32 tests' rule:
    4 x torch-fp32's error + 2^-23"""
    import torch
    z, y = host(rt, t["z"]), host(rt, t["y"])
    gamma, beta = host(rt, tp[t["bn"] + "/gamma"]), host(rt, tp[t["bn"] + "/beta"])
    mask = (y > 0) if t["relu"] else None
    r64 = T.bn_reference(z, gamma, beta, res, mask, dy, torch.float64)
    r32 = T.bn_reference(z, gamma, beta, res, mask, dy, torch.float32)
    worst = 0.0
    for key, got in (("y", y), ("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta)):
        e_ref, e_dev = _nerr(r32[key], r64[key]), _nerr(got.reshape(r64[key].shape), r64[key])
        assert e_dev <= 4 * e_ref + 2.0 ** -23, (name, key, e_dev, e_ref)
        worst = max(worst, e_dev / (4 * e_ref + 2.0 ** -23))
    return worst


def check_trunk(rt, blocks, im_h, im_w, seed):
    """One train-mode forward + backward of a train_dtype="bf16" trunk, checked layer by layer on the device's own tensors.
    -> (worst forward, input-gradient, weight-gradient product error; worst BatchNormalization ratio to its bound; res5 distance from the fp32 pass)"""
    import torch
    from chainer_faster_rcnn_amd.models.resnet import block_names, conv_specs
    F = torch.nn.functional
    params, x, model = trunk_case(rt, blocks, im_h, im_w, seed, train_dtype="bf16")
    H = lambda a: host(rt, a)                                                                        # noqa: E731
    xd = dev(rt, x)
    res5 = H(model(xd))
    cot = np.random.RandomState(seed + 7).randn(*res5.shape).astype(np.float32)
    bcol = {}
    grads = model.backward(dev(rt, cot), collect=bcol)
    tape, tp = model.tape, model.tp
    specs = conv_specs(blocks, T.NARROW)
    assert set(c for c, _, _, _, _ in specs) <= set(bcol)
    e_fwd = e_dx = e_dw = bn_worst = 0.0
    for conv, bn, ci, co, k in specs:
        t = tape[conv]
        dy, dz, dx = [None if a is None else H(a) for a in bcol[conv]]
        xin, W, z = H(t["x"]), H(tp[conv + "/W"]), H(t["z"])
        dW = H(grads[conv + "/W"])
        if k == 3:
            z64, dw64, dx64 = _conv3x3_64(rne(xin), rne(W), rne(dz))
            z64w = z64
        else:                                                        # 1x1, and the stem over its columns
            bias = H(tp[conv + "/b"]) if (conv + "/b") in tp else np.zeros(co, np.float32)
            z64w, _, dx64, dw64 = products64(rne(xin), rne(W), rne(dz), bias)
        assert W.shape == dW.shape == dw64.shape, conv
        ez, ew = _nerr(z.reshape(z64w.shape), z64w), _nerr(dW, dw64)
        assert ez <= TOL_FWD and ew <= TOL_WGRAD, (conv, ez, ew)
        assert _maxabs(dW) > 1e-3 and _maxabs(H(grads[bn + "/gamma"])) > 1e-3 and _maxabs(H(grads[bn + "/beta"])) > 1e-3, conv     # non-vacuity
        e_fwd, e_dw = max(e_fwd, ez), max(e_dw, ew)
        if conv == "conv1":
            assert dx is None
        else:
            ex = _nerr(dx.reshape(dx64.shape), dx64)
            assert ex <= TOL_FWD and _maxabs(dx) > 0, (conv, ex)
            e_dx = max(e_dx, ex)
        # its BatchNormalization on the device's own z and dy; conv3's carries the shortcut
        res = None
        if conv.endswith("conv3"):
            p = conv[:-5]
            res = H(tape[p + "conv4"]["y"]) if p.endswith("/a/") else H(tape[p + "conv1"]["x"])
        bn_worst = max(bn_worst, _bn_check(conv, t, tp, res, dy, dz, H(grads[bn + "/gamma"]), H(grads[bn + "/beta"]), rt))
    # conv1/b sits in front of a BatchNormalization: its gradient is analytically 0
    assert _maxabs(H(grads["conv1/b"])) <= 1e-3 * _maxabs(H(grads["conv1/W"]))
    # ---- the glue, bit for bit: what a layer reads is what the layer before produced
    same = lambda a, b: a.shape == b.shape and np.array_equal(a, b)                                  # noqa: E731
    cols = F.unfold(torch.from_numpy(x), 7, padding=3, stride=2).numpy()                             # (1, 147, OH * OW): pure data movement
    stem_x = H(tape["conv1"]["x"])
    assert same(stem_x[0, :147].reshape(147, -1), cols[0]) and not stem_x[0, 147:].any()
    h = F.max_pool2d(torch.from_numpy(H(tape["conv1"]["y"])), 3, 2, ceil_mode=True).numpy()
    for (stage, _, _, _, stride), n in zip(model.stages, blocks):
        for b in block_names(n):
            p = "%s/%s/" % (stage, b)
            xin = h[:, :, ::2, ::2] if (b == "a" and stride == 2) else h
            assert same(H(tape[p + "conv1"]["x"]), xin), p
            if b == "a":
                assert same(H(tape[p + "conv4"]["x"]), xin), p
            assert tape[p + "conv2"]["x"] is tape[p + "conv1"]["y"] and tape[p + "conv3"]["x"] is tape[p + "conv2"]["y"], p
            h = H(tape[p + "conv3"]["y"])
    assert same(h, res5)
    order = [pp for (stage, _, _, _, _), n in zip(model.stages, blocks) for pp in ["%s/%s/" % (stage, b) for b in block_names(n)]]
    for i, p in enumerate(order):
        dy3, dz3, dx3 = [H(a) for a in bcol[p + "conv3"]]
        want_dy3 = cot if i == len(order) - 1 else H(bcol[order[i + 1]][1])
        assert same(dy3, want_dy3), p
        dres = np.where(H(tape[p + "conv3"]["y"]) > 0, dy3, np.float32(0)).astype(np.float32)         # bn3's backward hands the masked dy to the shortcut
        assert same(H(bcol[p + "conv2"][0]), dx3) and same(H(bcol[p + "conv1"][0]), H(bcol[p + "conv2"][2])), p
        other, d = H(bcol[p][0]), H(bcol[p][1])
        d1 = H(bcol[p + "conv1"][2])
        if p.endswith("/a/"):
            assert same(H(bcol[p + "conv4"][0]), dres) and same(other, H(bcol[p + "conv4"][2])), p
        else:
            assert same(other, dres), p
        total = d1 + other                                           # one fp32 addition per element
        if tape[p]["strided"]:
            full = np.zeros((1, total.shape[1]) + tuple(tape[p]["hw"]), np.float32)
            full[:, :, ::2, ::2] = total
            total = full
        assert same(d, total), p
    y1 = torch.from_numpy(H(tape["conv1"]["y"])).requires_grad_(True)
    F.max_pool2d(y1, 3, 2, ceil_mode=True).backward(torch.from_numpy(H(bcol[order[0]][1])))
    assert same(H(bcol["conv1"][0]), y1.grad.numpy())
    # ---- the bf16 pass is not the fp32 pass
    _, _, ref = trunk_case(rt, blocks, im_h, im_w, seed)
    res5_f32 = H(ref(xd))
    dist = _nerr(res5, res5_f32)
    assert not np.array_equal(res5, res5_f32) and dist > 1e-4, dist
    print("TRUNK16 %s %dx%d: forward %.2e, input gradient %.2e (bound %.0e), weight gradient %.2e (bound %.0e), BatchNormalization at %.3f of its bound, "
          "res5 bf16 vs fp32 %.2e" % (blocks, im_h, im_w, e_fwd, e_dx, TOL_FWD, e_dw, TOL_WGRAD, bn_worst, dist))
    return e_fwd, e_dx, e_dw, bn_worst, dist


def _trunk_state(rt, model, xd, seed):
    res5 = host(rt, model(xd))
    grads = model.backward(dev(rt, np.random.RandomState(seed + 7).randn(*res5.shape).astype(np.float32)))
    state = {"res5": res5}
    state.update({"g/" + k: host(rt, v) for k, v in grads.items()})
    state.update({"p/" + k: host(rt, v) for k, v in model.tp.items()})
    return state


def check_f32_unchanged(rt, blocks, im_h, im_w, seed):
    """train_dtype="f32" is the trunk built without the keyword, bit for bit: res5, every gradient, every parameter and running statistic after
    one forward + backward"""
    _, x, plain = trunk_case(rt, blocks, im_h, im_w, seed)
    _, _, named = trunk_case(rt, blocks, im_h, im_w, seed, train_dtype="f32")
    assert plain.train_dtype == named.train_dtype == "f32"
    xd = dev(rt, x)
    a, b = _trunk_state(rt, plain, xd, seed), _trunk_state(rt, named, xd, seed)
    assert set(a) == set(b) and _maxabs(a["g/res5/a/conv3/W"]) > 0
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert not named._w16 and not plain._w16                                                         # no 16-bit weights were packed


def check_constructor_refusals(rt):
    import pytest
    from chainer_faster_rcnn_amd.models import ResNet
    for bad in ("f16", "bf16s", "split", None, 16):
        with pytest.raises(ValueError, match="train_dtype"):
            ResNet(runtime=rt, blocks=T.TRAINER_BLOCKS, train_dtype=bad)
    with pytest.raises(ValueError, match="conv_dtype"):
        ResNet(runtime=rt, blocks=T.TRAINER_BLOCKS, conv_dtype="bf16", train_dtype="bf16")
    assert ResNet(runtime=rt, blocks=T.TRAINER_BLOCKS).train_dtype == "f32"
    assert ResNet(runtime=rt, blocks=T.TRAINER_BLOCKS, train_dtype="bf16").conv_dtype == "f32"


# ------------------------------------------------------------------------------------------------------------------ trainer level
def build_model(rt, params, train_dtype="bf16", blocks=T.TRAINER_BLOCKS):
    """resnet_train_cases.build_model with the trunk's train_dtype"""
    from chainer_faster_rcnn_amd.models import FasterRCNN, ResNet
    model = FasterRCNN(trunk_class=functools.partial(ResNet, blocks=blocks, base_width=T.NARROW, train_dtype=train_dtype), rpn_in_ch=32 * T.NARROW,
                       rpn_mid_ch=64, feat_stride=32, anchor_scales=(1, 2, 3), runtime=rt)
    model.trunk.load_params(params, "trunk/")
    model.RPN.load_params(params, "RPN/")
    model.rpn_train = True
    return model


def make_rpn_trainer(rt, params=None, train_dtype="bf16", **kw):
    from chainer_faster_rcnn_amd.train import RPNTrainer
    return RPNTrainer(build_model(rt, params if params is not None else T.trainer_params(), train_dtype), **kw)


def make_rcnn_trainer(rt, train_dtype="bf16", **kw):
    """resnet_rcnn_train_cases.make_trainer with the trunk's train_dtype"""
    import resnet_rcnn_train_cases as R
    from chainer_faster_rcnn_amd.train import RCNNTrainer
    params = R.rcnn_params()
    model = build_model(rt, params, train_dtype)
    for n in R.HEAD:
        getattr(model, n).set(params[n + "/W"], params[n + "/b"])
    model.RPN.proposal_layer.TEST_RPN_POST_NMS_TOP_N = R.POST_NMS[tuple(T.TRAINER_BLOCKS)]
    model.rcnn_train = True
    kw.setdefault("dropout_rng", "device")
    return RCNNTrainer(model, **kw)


def _record_ready(tr):
    seen, inner = [], tr._grads_ready

    def ready(name):
        seen.append(name)
        return inner(name)
    tr._grads_ready = ready
    return seen


def _one_sgd_step(rt, tr, fill, inputs, loss_key):
    """one step: W and the velocity equal the NumPy restatement of MomentumSGD + WeightDecay on the device's own gradient buffer, bit for bit"""
    import optimizer_cases as OC
    from oracle import frcnn_oracle as O
    assert tr.opt == "MomentumSGD" and tr.model.trunk.train_dtype == "bf16"
    w, v = host(rt, tr.W).copy(), np.zeros(tr.n_flat, np.float32)
    seen = _record_ready(tr)
    out = fill(tr, inputs, 11)
    loss = tr.losses_host(out)
    assert np.isfinite(loss[loss_key]) and loss[loss_key] > 0, loss
    g = host(rt, tr.G).copy()
    got = tr.grads_chainer_layout()
    for k, a in got.items():
        assert np.isfinite(a).all() and (np.abs(a).max() > 0 or k == "trunk/conv1/b"), k
    tr.update()
    w, v = O.momentum_sgd_wd(w, g, v)
    OC.assert_same_bits(host(rt, tr.W), w, "bf16 trunk: MomentumSGD W")
    OC.assert_same_bits(host(rt, tr.V), v, "bf16 trunk: MomentumSGD v")
    assert tr.model.trunk._w16_stale and tr.model.trunk._w16                                          # the 3x3 layers' 16-bit weights are re-packed next step
    return seen, g


def check_rpn_step(rt):
    """one RPNTrainer step on a bf16 trunk; the `ready` callbacks come in the fp32 trunk's order; the gradient is not the fp32 trunk's"""
    inputs = T.trainer_inputs()
    seen, g = _one_sgd_step(rt, make_rpn_trainer(rt), T.fill_grads, inputs, "rpn_loss")
    ref = make_rpn_trainer(rt, train_dtype="f32")
    seen32 = _record_ready(ref)
    T.fill_grads(ref, inputs, 11)
    assert seen == seen32 and len(seen) >= len(ref.resnet.names) > 0, (seen, seen32)
    g32 = host(rt, ref.G)
    assert not np.array_equal(g, g32) and np.isfinite(g).all()


def check_rcnn_step(rt):
    import resnet_rcnn_train_cases as R
    inputs = R.trainer_inputs()
    seen, _ = _one_sgd_step(rt, make_rcnn_trainer(rt), R.fill_grads, inputs, "loss_rcnn")
    ref = make_rcnn_trainer(rt, train_dtype="f32")
    seen32 = _record_ready(ref)
    R.fill_grads(ref, inputs, 11)
    assert seen == seen32 and len(seen) > 0, (seen, seen32)


def check_resume_and_inference(rt, tmp_path, n=3, k=2):
    """resnet_train_cases.check_snapshot_resume on bf16 trunks (k steps + save + load into a trainer built on OTHER parameters + 1 step == n steps,
    bit for bit, running statistics included), then its check_inference_after_training on the n-step trainer: the re-fold is unchanged"""
    from chainer_faster_rcnn_amd.serializers import load_trainer_npz, save_trainer_npz
    inputs = T.trainer_inputs()

    def run(tr, first, last):
        for it in range(first, last):
            T.fill_grads(tr, inputs, 40 + it)
            tr.update()
    a = make_rpn_trainer(rt)
    run(a, 0, n)
    b = make_rpn_trainer(rt)
    run(b, 0, k)
    path = str(tmp_path / "resnet16_snapshot")
    save_trainer_npz(path, b)
    c = load_trainer_npz(path, make_rpn_trainer(rt, params=T.trainer_params(seed=3)))
    assert c.iteration == k and c.model.trunk.train_dtype == "bf16"
    run(c, k, n)
    assert np.array_equal(host(rt, a.W).view(np.uint32), host(rt, c.W).view(np.uint32))
    assert np.array_equal(host(rt, a.V).view(np.uint32), host(rt, c.V).view(np.uint32))
    for q in a.model.trunk.persistent_keys():
        assert np.array_equal(host(rt, a.model.trunk.tp[q]).view(np.uint32), host(rt, c.model.trunk.tp[q]).view(np.uint32)), q
    T.check_inference_after_training(rt, a)


def check_pinned_refusals(rt):
    """the trainers' own arithmetic keywords still refuse a ResNet model, whatever its train_dtype"""
    import pytest
    from chainer_faster_rcnn_amd.train import RPNTrainer
    for math in ("split", "bf16", "f16"):
        with pytest.raises(ValueError, match="ResNet"):
            RPNTrainer(build_model(rt, T.trainer_params()), conv_math=math)
    with pytest.raises(ValueError, match="ResNet"):
        make_rcnn_trainer(rt, precision="bf16")


LOSS_REL, LOSS_ABS = 0.05, 0.01          # DESIGN 3.13's figure for the VGG step


def loss_curves(rt, steps=50, images=5, np_seed=0):
    """`steps` RPN steps from one initialisation on an fp32 and on a bf16 trunk: the same images in the same order, the same NumPy seed per step
    -> (fp32 losses, bf16 losses)"""
    import optimizer_cases as OC
    inputs = [OC.rpn_inputs(s, *T.TRAINER_HW) for s in range(images)]
    curves = []
    for dtype in ("f32", "bf16"):
        tr = make_rpn_trainer(rt, train_dtype=dtype)
        losses = []
        for it in range(steps):
            out = T.fill_grads(tr, inputs[it % images], 1000 * np_seed + it)
            tr.update()
            losses.append(float(tr.losses_host(out)["rpn_loss"]))
        curves.append(np.array(losses))
    return curves


def check_loss_curves(rt):
    f32, b16 = loss_curves(rt)
    dev_abs = np.abs(b16 - f32)
    worst = int(np.argmax(dev_abs - LOSS_REL * np.abs(f32)))
    print("RESNET16_STEP fp32 first10 %.4f last10 %.4f | bf16 first10 %.4f last10 %.4f | largest deviation %.4f (%.2f %% of the fp32 loss %.4f) at step %d"
          % (f32[:10].mean(), f32[-10:].mean(), b16[:10].mean(), b16[-10:].mean(), dev_abs[worst], 100 * dev_abs[worst] / abs(f32[worst]), f32[worst], worst))
    assert np.isfinite(f32).all() and np.isfinite(b16).all()
    assert f32[-10:].mean() < f32[:10].mean() and b16[-10:].mean() < b16[:10].mean()
    assert np.all(dev_abs <= LOSS_REL * np.abs(f32) + LOSS_ABS), (dev_abs.max(), worst)
