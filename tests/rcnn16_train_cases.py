"""bf16 / fp16 mixed-precision stage-2 training (RCNNTrainer(precision="bf16" / "f16")): checks shared by the CPU suite (host-emulated kernels)
and the GPU suite.  The contract: every matrix product of the step -- the trunk's convolutions and the four L.Linear layers, forward, input
gradient and weight gradient -- takes RNE-rounded 16-bit operands with fp32 accumulation; the float64 references below impose exactly that
rounding on their operands, so the kernels are judged on their arithmetic, not on the rounding they were asked to do.

Bars of the L.Linear kernels (error relative to the largest reference entry), on x = relu(randn), W = randn * sqrt(2 / K): a strictly sequential
fp32 sum reaches 5.3e-6 at K = 25088 and at most 2e-6 at K = 4096, and any MFMA / split-K order is at most that deep: 1e-5 up to K = 4096 (the
conv kernels' bar), 2e-5 at K = 25088.  The input gradient sums over N <= 4096 and the weight gradient over M <= 320 rows: 1e-5.  Rounded and
unrounded operands differ by 2.4e-3 (bf16) / 3e-4 (fp16): a kernel that does not round, or rounds in the other format, misses by two orders."""
import numpy as np

from oracle import frcnn_oracle as O
import bf16_train_cases as B
import f16_train_cases as F
import parity_cases as P
import train_cases as T

HEAD = ("fc6", "fc7", "cls_score", "bbox_pred")


def linear_tol(K):
    return 1e-5 if K <= 4096 else 2e-5


def _pick(rs, n, k):
    """k random indices of range(n) plus the first and the last."""
    if k is None or k + 2 >= n:
        return np.arange(n)
    return np.unique(np.concatenate([[0, n - 1], rs.randint(0, n, k)]))


def linear_case(M, N, K, seed=0):
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.randn(M, K), 0).astype(np.float32)
    W = (rs.randn(N, K) * np.sqrt(2.0 / K)).astype(np.float32)
    b = (rs.randn(N) * 0.1).astype(np.float32)
    dy = (rs.randn(M, N) * 1e-2).astype(np.float32)
    return rs, x, W, b, dy


def check_linear_forward(rt, M, N, K, half="bf16", relu=True, seed=0, sample=None):
    """frcnn_linear_{bf16,f16}_train against float64 of RNE(x) RNE(W)^T + b; sample = (rows, cols) for the float64 check of big shapes."""
    rne = F.ROUND[half][0]
    rs, x, W, b, _ = linear_case(M, N, K, seed)
    y = P.host(rt, rt.with_half(half).linear_bf16_train(P.dev(rt, x), P.dev(rt, W), P.dev(rt, b), relu=relu))
    assert y.shape == (M, N)
    rows, cols = _pick(rs, M, sample and sample[0]), _pick(rs, N, sample and sample[1])
    want = rne(x[rows]).astype(np.float64) @ rne(W[cols]).astype(np.float64).T + b[cols]
    if relu:
        want = np.maximum(want, 0)
    err = F.rel(y[np.ix_(rows, cols)], want, 1e-6)
    print("RCNN16_KERNEL forward %s %s err %.3g" % (half, (M, N, K), err))
    assert err <= linear_tol(K), (half, M, N, K, err)
    y0 = P.host(rt, rt.with_half(half).linear_bf16_train(P.dev(rt, x), P.dev(rt, W), None, relu=False))      # no bias term
    assert F.rel(y0[np.ix_(rows, cols)], rne(x[rows]).astype(np.float64) @ rne(W[cols]).astype(np.float64).T, 1e-6) <= linear_tol(K)
    return err


def check_linear_dgrad(rt, M, N, K, half="bf16", seed=0, sample=None):
    """frcnn_linear_dgrad_{bf16,f16} against float64 of RNE(dy) RNE(W), W as stored."""
    rne = F.ROUND[half][0]
    rs, _, W, _, dy = linear_case(M, N, K, seed)
    dx = P.host(rt, rt.with_half(half).linear_dgrad_bf16(P.dev(rt, dy), P.dev(rt, W)))
    assert dx.shape == (M, K)
    rows, cols = _pick(rs, M, sample and sample[0]), _pick(rs, K, sample and sample[1])
    want = rne(dy[rows]).astype(np.float64) @ rne(W[:, cols]).astype(np.float64)
    err = F.rel(dx[np.ix_(rows, cols)], want)
    print("RCNN16_KERNEL dgrad %s %s err %.3g" % (half, (M, N, K), err))
    assert err <= 1e-5, (half, M, N, K, err)
    return err


def check_linear_wgrad(rt, M, N, K, half="bf16", seed=0, sample=None):
    """frcnn_linear_wgrad_{bf16,f16} against float64 of RNE(dy)^T RNE(x)."""
    rne = F.ROUND[half][0]
    rs, x, _, _, dy = linear_case(M, N, K, seed)
    dw = P.host(rt, rt.with_half(half).linear_wgrad_bf16(P.dev(rt, dy), P.dev(rt, x)))
    assert dw.shape == (N, K)
    rows, cols = _pick(rs, N, sample and sample[0]), _pick(rs, K, sample and sample[1])
    want = rne(dy[:, rows]).astype(np.float64).T @ rne(x[:, cols]).astype(np.float64)
    err = F.rel(dw[np.ix_(rows, cols)], want)
    print("RCNN16_KERNEL wgrad %s %s err %.3g" % (half, (M, N, K), err))
    assert err <= 1e-5, (half, M, N, K, err)
    return err


def check_f16_closer_than_bf16(rt, M=60, N=84, K=3200, seed=1):
    """The fp16 entries really compute in fp16: same inputs, and each of the three results closer to the UNROUNDED float64 than the bf16 twin's."""
    _, x, W, b, dy = linear_case(M, N, K, seed)
    x64, W64, dy64 = x.astype(np.float64), W.astype(np.float64), dy.astype(np.float64)
    wants = {"forward": x64 @ W64.T + b, "dgrad": dy64 @ W64, "wgrad": dy64.T @ x64}
    e = {}
    for h in ("bf16", "f16"):
        rth = rt.with_half(h)
        got = {"forward": rth.linear_bf16_train(P.dev(rt, x), P.dev(rt, W), P.dev(rt, b)), "dgrad": rth.linear_dgrad_bf16(P.dev(rt, dy), P.dev(rt, W)),
               "wgrad": rth.linear_wgrad_bf16(P.dev(rt, dy), P.dev(rt, x))}
        e[h] = {k: F.rel(P.host(rt, v), wants[k]) for k, v in got.items()}
    print("RCNN16_KERNEL distance to unrounded float64 %s" % T.json_dumps(e))
    for k in wants:
        assert e["f16"][k] < e["bf16"][k] / 2, (k, e)
    return e


def check_linear_split_k(rt, M, N, K, half="bf16", splits=("2", "3"), seed=0):
    """Operands that are small multiples of powers of two: every partial sum is exact in fp32, so the result with the reduction axis split into
    slabs equals the unsplit one BIT FOR BIT (slabs are added in split order), forward and input gradient, and equals the exact product.
    (These entries keep no counter page: their workspace is slabs only.)"""
    from chainer_faster_rcnn_amd import tuning
    rs = np.random.RandomState(seed)
    x = (rs.randint(0, 9, (M, K)) * 0.25).astype(np.float32)
    W = (rs.randint(-4, 5, (N, K)) * 2.0 ** -5).astype(np.float32)
    b = (rs.randint(-4, 5, N) * 0.125).astype(np.float32)
    dy = (rs.randint(-8, 9, (M, N)) * 2.0 ** -6).astype(np.float32)
    rth = rt.with_half(half)
    outs = []
    try:
        for s in ("1",) + tuple(splits):
            tuning.set("FRCNN_LINEAR_TRAIN_SPLITS", s)
            outs.append((P.host(rt, rth.linear_bf16_train(P.dev(rt, x), P.dev(rt, W), P.dev(rt, b), relu=True)),
                         P.host(rt, rth.linear_dgrad_bf16(P.dev(rt, dy), P.dev(rt, W)))))
    finally:
        tuning.set("FRCNN_LINEAR_TRAIN_SPLITS", None)
    want_y = np.maximum(x.astype(np.float64) @ W.astype(np.float64).T + b, 0).astype(np.float32)
    want_dx = (dy.astype(np.float64) @ W.astype(np.float64)).astype(np.float32)
    assert np.array_equal(outs[0][0], want_y) and np.array_equal(outs[0][1], want_dx)
    for y, dx in outs[1:]:
        assert np.array_equal(y, outs[0][0]) and np.array_equal(dx, outs[0][1])
    dw = P.host(rt, rth.linear_wgrad_bf16(P.dev(rt, dy), P.dev(rt, x)))
    assert np.array_equal(dw, (dy.astype(np.float64).T @ x.astype(np.float64)).astype(np.float32))


def check_roi_pool_bwd_ordered(rt, R=37, C=6, H=9, W=13, bins_hw=(7, 7), seed=0, small_rois=True):
    """frcnn_roi_pool_bwd_ordered: bit for bit the reference's CPU loop (RoIs ascending, bins ascending, fp32 adds), also where several bins of one
    RoI hit the same cell and where arg-max is -1 (an empty bin); within rounding of the atomic plane kernel; the same bits on a second run."""
    rs = np.random.RandomState(seed)
    oh, ow = bins_hw
    dy = rs.randn(R, C, oh, ow).astype(np.float32)
    am = rs.randint(0, H * W, (R, C, oh, ow)).astype(np.int32)
    if small_rois:                                                  # a third of the RoIs small: their bins share a handful of cells
        for r in range(0, R, 3):
            am[r] = np.minimum(rs.randint(0, 4, (C, oh, ow)) + (r % max(H * W - 4, 1)), H * W - 1)
    am[rs.rand(R, C, oh, ow) < 0.05] = -1
    want = np.zeros((C, H * W), np.float32)
    for r in range(R):
        for c in range(C):
            a, v = am[r, c].reshape(-1), dy[r, c].reshape(-1)
            for b in range(oh * ow):
                if a[b] >= 0:
                    want[c, a[b]] = np.float32(want[c, a[b]] + v[b])
    got = P.host(rt, rt.roi_pool_bwd_ordered(P.dev(rt, dy), P.dev(rt, am), C, H, W))
    assert got.shape == (1, C, H, W) and np.array_equal(got.reshape(C, H * W), want)
    again = P.host(rt, rt.roi_pool_bwd_ordered(P.dev(rt, dy), P.dev(rt, am), C, H, W))
    assert np.array_equal(again, got)
    plane = P.host(rt, rt.roi_pool_bwd(P.dev(rt, dy), P.dev(rt, am), C, H, W))
    assert np.abs(plane - got).max() <= 1e-5 * np.abs(got).max()


# ------------------------------------------------------------------------------------------- the step
def small_case(rt, seed=0, im_h=48, im_w=64):
    rs = np.random.RandomState(seed)
    params = T.small_params()
    params.update(T.small_head_params(rs))
    x = rs.randn(1, 3, im_h, im_w).astype(np.float32)
    gt = P.gt_case(rs, 3, im_h, im_w)
    gt[0, :, 2] = np.minimum(gt[0, :, 0] + rs.uniform(10, 30, 3), im_w - 1)
    gt[0, :, 3] = np.minimum(gt[0, :, 1] + rs.uniform(10, 30, 3), im_h - 1)
    info = np.array([[im_h, im_w]], dtype=np.int32)
    return params, x, gt, info


def build_small(rt, params):
    model = T.build_small(rt, params)
    for n in HEAD:
        getattr(model, n).set(params[n + "/W"], params[n + "/b"])
    model.RPN.proposal_layer.RPN_MIN_SIZE = 4
    model.RPN.proposal_layer._min_size = 4
    model.rpn_train = False
    model.rcnn_train = True
    return model


def vgg_case(im_h=160, im_w=224, seed=0):
    from chainer_faster_rcnn_amd import synthetic
    rs = np.random.RandomState(seed)
    params = synthetic.params(seed=1)
    x = synthetic.image(seed=4, h=im_h, w=im_w)
    gt = P.gt_case(rs, 4, im_h, im_w)
    info = np.array([[im_h, im_w]], dtype=np.int32)
    return params, x, gt, info


def build_vgg(rt, params):
    from chainer_faster_rcnn_amd.models import FasterRCNN
    model = FasterRCNN(runtime=rt)
    model.load_params(params)
    model.rcnn_train = True
    return model


def trainer(rt, params, build, precision, **kw):
    from chainer_faster_rcnn_amd.train import RCNNTrainer
    return RCNNTrainer(build(rt, params), precision=precision, **kw)


def fixed_masks(tr, seed):
    """Dropout masks for the ProposalLayer's capacity (the count is known after the forward pass: slice)."""
    rs = np.random.RandomState(seed)
    cap = tr.model.RPN.proposal_layer.TEST_RPN_POST_NMS_TOP_N
    h6, h7 = int(tr.model.fc6.W.shape[0]), int(tr.model.fc7.W.shape[0])
    return ((rs.rand(cap, h6) >= 0.5) * 2.0).astype(np.float32), ((rs.rand(cap, h7) >= 0.5) * 2.0).astype(np.float32)


def run_step(tr, x, gt, info, seed, update=False):
    """forward_backward with fixed masks: one pass to learn the step's own RoI count (proposals are a function of the weights), then the pass
    that is judged."""
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    m6, m7 = fixed_masks(tr, seed)
    np.random.seed(seed + 1)
    n = int(tr.forward_backward(Variable(x), Variable(info), Variable(gt))["n_rois"])
    masks = (m6[:n], m7[:n])
    np.random.seed(seed + 1)
    out = tr.forward_backward(Variable(x), Variable(info), Variable(gt), masks=masks)
    assert out["n_rois"] == n
    if update:
        tr.all_reduce()
        tr.update()
    return out, masks


def _decisions(rt, out, names):
    """Every ReLU sign and pool winner of the device's trunk forward, in the form O.rcnn_train_grads imposes (train_cases.check_rcnn_step)."""
    import torch
    from chainer_faster_rcnn_amd.train import _PoolArg
    linp, dec = out["layer_inputs"], []
    for i, nme in enumerate(names):
        if nme == "pool":
            ent = linp[i]
            assert not isinstance(ent, _PoolArg)                    # the 16-bit trunk runs its pools as launches of their own
            m = torch.from_numpy(rt.mem.to_numpy(ent).reshape(1, *ent.shape[-3:]))
            val, idx = torch.nn.functional.max_pool2d(m, 2, 2, ceil_mode=True, return_indices=True)
            dec.append((idx[0].numpy(), (val[0] > 0).numpy()))
        elif i + 1 < len(names) and names[i + 1] == "pool":
            dec.append(None)
        else:
            nxt = rt.mem.to_numpy(linp[i + 1])
            dec.append(nxt.reshape(nxt.shape[-3:]) > 0)
    return dec


def check_step(rt, params, build, layers, x, gt, info, feat_stride, precision, seed=0, kernel_tol=1e-4, loss_tol=1e-2, given_tol=1e-2, **kw):
    """One mixed-precision stage-2 step.  The step's own RoIs, ProposalTargetLayer sample and masks go to the oracle.  Asserted: the loss within
    loss_tol of the fp32 oracle's; every weight gradient (conv and linear) within kernel_tol of float64 on its own kept (input, upstream
    gradient) pair with the rounding imposed; every gradient within given_tol of the float64 pass with ALL of the device's decisions imposed
    (head ReLU, trunk ReLU signs and pool winners, RoI arg-max cells); the update bit for bit momentum_sgd_wd(W, G / S, V).  Reported: the
    distance to the free-decision fp32 autograd and the flip counts.  -> (losses, worst given-decisions distance, table, site_flips)."""
    rne = F.ROUND["f16" if precision == "f16" else "bf16"][0]
    tr = trainer(rt, params, build, precision, **kw)
    names = [l if l == "pool" else l[0] for l in layers]
    convs = [n for n in names if n != "pool"]
    tr.keep_dy, tr.kept_dy = set(convs) | set(HEAD), {}
    out, masks = run_step(tr, x, gt, info, seed)
    rt.mem.synchronize()
    n = out["n_rois"]
    S = np.float32(tr.loss_scaler.state()["scale"]) if tr.loss_scaler is not None else np.float32(1)
    keep = P.host(rt, out["keep_inds"])
    rois = P.host(rt, out["rois"])[:n]
    np.random.seed(seed + 1)
    use_gt, ext, keep2 = O.proposal_target_layer(rois, gt)
    assert np.array_equal(keep, keep2)
    labels = use_gt[:, -1].astype(np.int64)
    args = (params, x, rois, keep, labels, ext, masks[0], masks[1])
    want_loss, want = O.rcnn_train_grads(*args, layers=names, spatial_scale=1.0 / feat_stride)
    l = tr.losses_host(out)
    print("\nRCNN16_STEP %s %dx%d loss %.6g, fp32 oracle %.6g, scale %g, %d RoIs, %d kept" % (precision, x.shape[2], x.shape[3], l["loss_rcnn"], want_loss,
                                                                                           S, n, len(keep)))
    assert abs(l["loss_rcnn"] - want_loss) <= loss_tol * abs(want_loss), (l, want_loss)
    table = {}
    dims = dict((nm, (int(k.cin), int(k.cout))) for nm, k in tr.convs)
    for name in convs:                                              # (both sides carry the factor S)
        xin, dy = (P.host(rt, a) for a in tr.kept_dy[name])
        kerr = F.rel(P.host(rt, tr.grad[name + "/W"]), B.wgrad64(rne(xin), rne(dy), *dims[name]))
        table[name + "/W kernel_vs_f64_rounded"] = float("%.2g" % kerr)
    for name in HEAD:
        xin, dy = (P.host(rt, a) for a in tr.kept_dy[name])
        kerr = F.rel(P.host(rt, tr.grad[name + "/W"]), rne(dy).astype(np.float64).T @ rne(xin).astype(np.float64))
        table[name + "/W kernel_vs_f64_rounded"] = float("%.2g" % kerr)
    print("RCNN16_STEP kernels %s" % T.json_dumps(table))
    for k, v in table.items():
        assert v <= kernel_tol, (k, v)
    a6, a7 = [P.host(rt, a) for a in out["head_acts"]]
    am = P.host(rt, out["roi_argmax"]).reshape(n, -1, 7, 7)
    _, want_d, site_flips = O.rcnn_train_grads(*args, layers=names, spatial_scale=1.0 / feat_stride, float64=True, head_relu=(a6 > 0, a7 > 0),
                                               trunk_decisions=_decisions(rt, out, names), roi_argmax=am)
    got = tr.grads_chainer_layout()
    grads, worst, worst_free = {}, 0.0, 0.0
    for k in sorted(want):
        e_free = F.rel(got[k], want[k].astype(np.float64), 1e-8)
        e_all = F.rel(got[k], want_d[k], 1e-12)
        grads[k] = {"vs_fp32_autograd": float("%.2g" % e_free), "vs_f64_given_all_device_decisions": float("%.2g" % e_all)}
        worst, worst_free = max(worst, e_all), max(worst_free, e_free)
    print("RCNN16_STEP gradients %s" % T.json_dumps({"worst_vs_f64_given_all_device_decisions": float("%.3g" % worst),
                                                      "worst_vs_fp32_autograd": float("%.3g" % worst_free), "gradients": grads,
                                                      "decisions_that_differ_from_the_float64_pass": site_flips}))
    for k, row in grads.items():
        assert row["vs_f64_given_all_device_decisions"] <= given_tol, (k, row)
    w0, v0, g = P.host(rt, tr.W), P.host(rt, tr.V), P.host(rt, tr.G)
    tr.update()
    w1, v1 = O.momentum_sgd_wd(w0, (g / S).astype(np.float32), v0)
    assert np.array_equal(P.host(rt, tr.W), w1) and np.array_equal(P.host(rt, tr.V), v1)
    return l, worst, grads, site_flips


def check_step_deterministic(rt, params, build, x, gt, info, precision="bf16", seed=0):
    """Two steps from identical state give a bit-identical gradient buffer."""
    gs = []
    for _ in range(2):
        tr = trainer(rt, params, build, precision)
        run_step(tr, x, gt, info, seed)
        gs.append(P.host(rt, tr.G))
    head0 = tr.seg["fc6/W"].offset
    assert np.array_equal(gs[0][head0:], gs[1][head0:]), "the head's gradients differ between two runs"
    assert np.array_equal(gs[0], gs[1]), float(np.abs(gs[0] - gs[1]).max() / np.abs(gs[0]).max())


def check_scale_invariance(rt, params, build, x, gt, info, scales=(2.0 ** 8, 2.0 ** 12), seed=0):
    """Static scales from one state and seed: the raw buffer holds S times the gradient.  The forward pass does not see the scale, so the losses
    are bit-identical and both unscaled gradients are within the step's bar of ONE float64 gradient (check_step): their distance is at most
    twice that bar, 2e-2 (measured: rounding level; operands that are subnormal at one scale and normal at the other are the only difference)."""
    runs = []
    for s in scales:
        tr = trainer(rt, params, build, "f16", loss_scale=s)
        assert not tr.loss_scaler.dynamic and tr.loss_scaler.state()["scale"] == s
        out, _ = run_step(tr, x, gt, info, seed)
        runs.append((P.host(rt, out["losses"]), P.host(rt, tr.G), tr.grads_chainer_layout(), tr))
    a, b = runs
    assert np.array_equal(a[0], b[0])
    assert not np.array_equal(a[1], b[1])
    worst = {}
    for name, sg in sorted(a[3].seg.items()):
        ga = a[1][sg.offset:sg.offset + sg.size].astype(np.float64) / scales[0]
        gb = b[1][sg.offset:sg.offset + sg.size].astype(np.float64) / scales[1]
        worst[name] = float("%.3g" % F.rel(ga, gb))
        assert worst[name] <= 2e-2, (name, worst[name])
    for k in a[2]:                                                  # grads_chainer_layout() is the raw buffer divided by the scale
        sg = a[3].seg[k[len("trunk/"):] if k.startswith("trunk/") else k]
        if not k.startswith("trunk/") or k.endswith("/b"):
            assert np.array_equal(a[2][k].reshape(-1), (a[1][sg.offset:sg.offset + sg.size] / np.float32(scales[0])))
    print("\nRCNN16_STEP scale invariance %s vs %s: losses bit-identical; worst relative difference of G / S per segment %s" % (
        scales[0], scales[1], T.json_dumps(worst)))


def check_overflow_handling(rt, params, build, x, gt, info, seed=0):
    """An Inf planted in trainer.G between forward_backward() and update(): every parameter and velocity keeps its bits and the scale backs off;
    the next clean step updates."""
    tr = trainer(rt, params, build, "f16", loss_scale=dict(init_scale=2.0 ** 10))
    assert tr.loss_scaler.dynamic
    run_step(tr, x, gt, info, seed)
    w0, v0 = P.host(rt, tr.W), P.host(rt, tr.V)
    g = P.host(rt, tr.G)
    g[tr.seg["fc7/W"].offset + 7] = np.inf
    tr.G[...] = P.dev(rt, g)
    tr.update()
    st = tr.loss_scaler.state()
    assert np.array_equal(P.host(rt, tr.W), w0) and np.array_equal(P.host(rt, tr.V), v0)
    assert (st["scale"], st["good_steps"], st["skipped_steps"], st["found_nonfinite"]) == (2.0 ** 9, 0, 1, 0) and tr.iteration == 1
    run_step(tr, x, gt, info, seed + 3, update=True)
    st = tr.loss_scaler.state()
    assert not np.array_equal(P.host(rt, tr.W), w0) and (st["scale"], st["good_steps"], st["skipped_steps"]) == (2.0 ** 9, 1, 1)
    assert np.all(np.isfinite(P.host(rt, tr.W)))


def check_construction(rt, params, build):
    """Static and dynamic construction, and the refusals of the keyword."""
    import pytest
    from chainer_faster_rcnn_amd.train import RCNNTrainer
    tr = trainer(rt, params, build, "f16")
    st = tr.loss_scaler.state()
    assert tr.loss_scaler.dynamic and tr.half == "f16" and (st["scale"], st["good_steps"], st["skipped_steps"]) == (2.0 ** 16, 0, 0)
    tr = trainer(rt, params, build, "f16", loss_scale=2.0 ** 10)
    assert not tr.loss_scaler.dynamic and tr.loss_scaler.state()["scale"] == 2.0 ** 10
    tr = trainer(rt, params, build, "f16", loss_scale=dict(init_scale=2.0 ** 8, growth_interval=3))
    assert tr.loss_scaler.dynamic and tr.loss_scaler.state()["scale"] == 2.0 ** 8
    tr = trainer(rt, params, build, "bf16")
    assert tr.loss_scaler is None and tr.half == "bf16" and tr.precision == "bf16"
    tr = trainer(rt, params, build, None)
    assert tr.loss_scaler is None and tr.precision is None and not hasattr(tr, "wb_fwd")
    for kw in (dict(precision="bf16", conv_math="split"), dict(precision="f16", conv_math="split"),       # precision with split products
               dict(loss_scale="dynamic"), dict(precision="bf16", loss_scale=2.0 ** 10), dict(conv_math="split", loss_scale=2.0 ** 10),   # loss_scale without f16
               dict(precision="fp8"), dict(precision="mfma"), dict(precision=16),                         # an unknown precision
               dict(precision="f16", loss_scale=3.0), dict(precision="f16", loss_scale=dict(growth=3.0))):
        with pytest.raises(ValueError):
            RCNNTrainer(build(rt, params), **kw)
    with pytest.raises((ValueError, AssertionError)):               # conv_math is checked first
        RCNNTrainer(build(rt, params), precision="f16", conv_math="f16")
    with pytest.raises(ValueError):
        RCNNTrainer(build(rt, params), conv_math="bf16")


def check_resume(rt, params, build, other_params, x, gt, info, tmp_path, n=3, k=1):
    """N steps == k steps + save + load + (N - k) steps bit for bit, the scaler's state included (an injected NaN so that the scale moves)."""
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.serializers import load_trainer_npz, save_trainer_npz
    cfg = dict(init_scale=2.0 ** 10, growth_interval=2)

    def run(tr, first, last):
        for it in range(first, last):
            np.random.seed(40 + it)
            tr.forward_backward(Variable(x), Variable(info), Variable(gt))
            if it == 0:
                g = P.host(rt, tr.G)
                g[3] = np.nan
                tr.G[...] = P.dev(rt, g)
            tr.all_reduce()
            tr.update()
    mk = lambda p: trainer(rt, p, build, "f16", loss_scale=cfg, dropout_rng="device", dropout_seed=7)
    a = mk(params)
    run(a, 0, n)
    b = mk(params)
    run(b, 0, k)
    path = str(tmp_path / "rcnn_f16_snapshot")
    save_trainer_npz(path, b)
    with np.load(path) as f:
        assert {"updater/loss_scaler/scale", "updater/loss_scaler/good_steps", "updater/loss_scaler/skipped_steps"} <= set(f.files)
    c = load_trainer_npz(path, mk(other_params))
    sb, sc = b.loss_scaler.state(), c.loss_scaler.state()
    assert all(sb[q] == sc[q] for q in ("scale", "good_steps", "skipped_steps")) and sc["scale"] == 2.0 ** 9 and sc["skipped_steps"] == 1, (sb, sc)
    run(c, k, n)
    sa, sc = a.loss_scaler.state(), c.loss_scaler.state()
    assert a.iteration == c.iteration == n and all(sa[q] == sc[q] for q in ("scale", "good_steps", "skipped_steps")), (sa, sc)
    assert sa["scale"] == 2.0 ** 10                                 # halved by step 0, doubled after two clean steps
    assert np.array_equal(P.host(rt, a.W), P.host(rt, c.W)) and np.array_equal(P.host(rt, a.V), P.host(rt, c.V))
    p2 = str(tmp_path / "rcnn_bf16_snapshot")                       # the other trainers' key set is unchanged
    save_trainer_npz(p2, trainer(rt, params, build, "bf16"))
    with np.load(p2) as f:
        assert not [q for q in f.files if "loss_scaler" in q]


def check_curves(rt, params, build, x, gt, info, steps=30):
    """`steps` steps with device-drawn dropout from one initialisation, fp32 / bf16 / f16: every loss finite, the mean of the last five below the mean
    of the first five.  (No closeness between the curves: a differently rounded trunk legitimately picks other proposals, hence another sample.)"""
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    curves = {}
    for tag, prec in (("fp32", None), ("bf16", "bf16"), ("f16", "f16")):
        tr = trainer(rt, params, build, prec, dropout_rng="device", dropout_seed=3)
        ls = []
        for it in range(steps):
            np.random.seed(200 + it)
            ls.append(tr.losses_host(tr.step(Variable(x), Variable(info), Variable(gt)))["loss_rcnn"])
        curves[tag] = np.array(ls)
        if tr.loss_scaler is not None:
            print("\nRCNN16_CURVE f16 scaler %s" % T.json_dumps(tr.loss_scaler.state()))
    print("\nRCNN16_CURVE %s" % T.json_dumps({k: [float("%.5g" % v) for v in c] for k, c in curves.items()}))
    for tag, c in curves.items():
        assert np.all(np.isfinite(c)), tag
        assert c[-5:].mean() < c[:5].mean(), (tag, c[:5].mean(), c[-5:].mean())
    return curves
