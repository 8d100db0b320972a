"""Isolated checks of the few-line kernels between the heavily tested stages, written once and run on the host emulator
(tests/test_head_loss_emulated.py) and on the MI355X (tests/test_gpu_head_loss.py):

  * csrc/head.hip, the detection-head epilogue: frcnn_head_decode, frcnn_head_decode_stacked (the kernel the inference forward runs),
    frcnn_bbox_transform_inv, frcnn_clip_boxes, frcnn_softmax_rows and frcnn_class_dets.  The file promises "the reference's operation
    order, no FMA contraction; exp evaluated in double and rounded to fp32", so the boxes are compared WORD FOR WORD with the oracle's
    restatement (O.bbox_transform_inv / O.clip_boxes, with O.EXP swapped for that exp), special values included; the fused kernel's
    probabilities are the same words as frcnn_softmax_rows's; the softmax values stand under an oracle-relative bar against float64.
  * frcnn_rcnn_loss (csrc/train.hip): losses, accuracy and both gradients against float64 closed forms, with O.rcnn_loss_grads as the
    comparator of the bars.
  * frcnn_rpn_loss at its edges (all labels ignored, no inside anchor, more than one pass of the 1024-thread loop, A = 1 / 3 / 9).
  * the stage-2 glue kernels (gather / scatter rows, mul, add, relu backward, transpose), exactly.

Every input is drawn from a fixed seed.  The bars:
  softmax   max |p - p64| <= 4 x the same figure of O.softmax on the same scores + 2^-23 (one ulp of a probability near 1; the factor
            allows a different fp32 expf and summation order)
  gradients max |g - g64| / max |g64| <= 4 x the same figure of O.rcnn_loss_grads + 2^-23
  losses    |l - l64| <= 4 x the oracle's own error + 4 fp32 ulps of the scale (loss_cls: the mean over rows of
            max(|logsumexp|, |s[label]|) -- each row's fp32 `logz - s[label]` carries a few ulps of its operands, not of the possibly
            small difference; loss_bbox: the float64 loss)"""
import numpy as np

from oracle import frcnn_oracle as O
from parity_cases import dev, host

INVALID = -1
ULP1 = 2.0 ** -23
POISON = np.float32(-12345.0)

# R, ncls
HEAD_SHAPES = [(1, 21), (37, 21), (257, 2), (300, 21), (64, 81), (2000, 21)]
IMAGES = [(600, 1000), (901, 600)]           # im_h, im_w: never equal, so a swapped bound shows
FIGURES = []                                 # (what, shape, device figure, oracle figure): printed by the two test files


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


# ------------------------------------------------------------------------------------------- word comparison
def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_words(got, want, what):
    """Equal as uint32 words; a position counts as equal when both sides are NaN.  A mismatch reports positions and ulp distances."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    ok = (words(got) == words(want)) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        bad = np.argwhere(~ok)
        lines = []
        for pos in bad[:8]:
            g, w = got[tuple(pos)], want[tuple(pos)]
            gi, wi = int(words(got)[tuple(pos)]), int(words(want)[tuple(pos)])
            ulps = abs((gi if gi < 0x80000000 else 0x80000000 - gi) - (wi if wi < 0x80000000 else 0x80000000 - wi))
            lines.append("%s: got %r (0x%08x) want %r (0x%08x), %d ulp" % (tuple(int(v) for v in pos), g, gi, w, wi, ulps))
        raise AssertionError("%s: %d of %d words differ\n  %s" % (what, len(bad), ok.size, "\n  ".join(lines)))


# ------------------------------------------------------------------------------------------- 1. head epilogue
def exact_exp(v):
    """exp evaluated in double and rounded once to fp32: what csrc/head.hip documents"""
    return np.exp(v.astype(np.float64)).astype(np.float32)


def head_inputs(R, ncls, im_h, im_w, seed):
    """Boxes partly outside the image with widths from 1 px to 600 px, deltas of 1.5 sigma (many boxes clipped on every side), scores
    of 3 sigma, and special values planted in fixed rows (a row or class the shape does not have is skipped)."""
    rs = np.random.RandomState(seed)
    wh = np.exp(rs.uniform(0.0, np.log(600.0), (R, 2)))
    xy = np.stack([rs.uniform(-0.3 * im_w, 1.1 * im_w, R), rs.uniform(-0.3 * im_h, 1.1 * im_h, R)], axis=1)
    boxes = np.hstack([xy, xy + wh - 1.0]).astype(np.float32)
    deltas = (rs.randn(R, 4 * ncls) * 1.5).astype(np.float32)
    score = (rs.randn(R, ncls) * 3).astype(np.float32)
    inf, nan = np.float32(np.inf), np.float32(np.nan)

    def plant(a, r, c, v):
        if r < a.shape[0] and c < a.shape[1]:
            a[r, c] = v
    c1 = 4 * (1 % ncls)
    plant(deltas, 2, c1 + 2, 88.8)                 # exp(88.8) is above the largest fp32: an infinite width
    plant(deltas, 5, 3, 100.0)                     # ... in the height
    plant(deltas, 7, c1 + 3, inf)
    plant(deltas, 9, 2, -inf)                      # exp(-inf) = 0: a zero width
    plant(deltas, 11, c1 + 0, nan)                 # NaN in dx
    plant(deltas, 13, 0, inf); plant(deltas, 13, 2, 100.0)           # inf - inf
    plant(deltas, 15, c1 + 1, -inf); plant(deltas, 15, c1 + 3, 88.8)
    if R > 17:
        boxes[17, 2] = boxes[17, 0] - 40.0         # inverted box: x2 < x1
    plant(boxes, 19, 0, nan)
    plant(boxes, 21, 3, nan)
    if R > 4:
        score[4] = np.float32(0.75)                # all-equal row
    plant(score, 6, ncls - 1, 1e4)
    plant(score, 8, 0, inf)
    plant(score, 10, 1, nan)
    if R > 12:
        score[12] = -inf                           # a row of all -inf
    plant(score, 14, 1, -inf)                      # a single -inf
    return boxes, deltas, score


def ref_boxes(boxes, deltas, im_h, im_w):
    """-> (unclipped, clipped): O.clip_boxes(O.bbox_transform_inv(boxes, deltas), [im_h, im_w]) with the correctly rounded exp.
    O.clip_boxes is NumPy's maximum(minimum(v, hi), 0): NaN goes through."""
    O.EXP = exact_exp
    try:
        with np.errstate(all="ignore"):
            unclipped = O.bbox_transform_inv(boxes, deltas)
            clipped = O.clip_boxes(unclipped.copy(), [im_h, im_w])
    finally:
        O.EXP = np.exp
    return unclipped, clipped


def softmax64(score):
    s = score.astype(np.float64)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


_MODEL_LAYOUT = []


def model_head_layout(rt):
    """(ld, dcol) of the stacked cls_score || bbox_pred GEMM as FasterRCNN builds it for 21 classes, read off a constructed model"""
    if not _MODEL_LAYOUT:
        from wino_cases import small_full_model
        model, _ = small_full_model(rt)
        assert model._num_classes == 21
        _MODEL_LAYOUT.append((int(model.head_out.W.shape[0]), int(model._head_dcol)))
    return _MODEL_LAYOUT[0]


def stacked_layouts(rt, ncls):
    """(ld, dcol): deltas right behind the scores (ncls rounded up to 4); extra padding in front of and behind the deltas; and, for 21
    classes, the model's own layout"""
    d4 = (ncls + 3) // 4 * 4
    out = [(d4 + 4 * ncls, d4), (d4 + 8 + 4 * ncls + 12, d4 + 8)]
    if ncls == 21:
        out.append(model_head_layout(rt))
    return out


def check_head_epilogue(rt, R, ncls, seed=0):
    """Every entry point of the epilogue on one (R, ncls), at both image sizes."""
    import warnings
    for k, (im_h, im_w) in enumerate(IMAGES):
        boxes, deltas, score = head_inputs(R, ncls, im_h, im_w, seed + 100 * k)
        unclipped, clipped = ref_boxes(boxes, deltas, im_h, im_w)
        bd, dd, sd = dev(rt, boxes), dev(rt, deltas), dev(rt, score)
        # frcnn_head_decode: the boxes word for word
        pb, pp = rt.head_decode(bd, dd, sd, im_h, im_w)
        pb_h, pp_h = host(rt, pb), host(rt, pp)
        assert_same_words(pb_h, clipped, "head_decode boxes %s" % ((R, ncls, im_h, im_w),))
        # frcnn_bbox_transform_inv = the unclipped reference; frcnn_clip_boxes on it = the clipped one
        raw = rt.bbox_transform_inv(bd, dd)
        assert_same_words(host(rt, raw), unclipped, "bbox_transform_inv %s" % ((R, ncls),))
        assert_same_words(host(rt, rt.clip_boxes_(raw, im_h, im_w)), clipped, "clip_boxes %s" % ((R, ncls, im_h, im_w),))
        # frcnn_softmax_rows: the same words as head_decode's probabilities (the same kernel), the value bar, the NaN pattern
        sm = host(rt, rt.softmax_rows(sd))
        assert_same_words(sm, pp_h, "softmax_rows vs head_decode %s" % ((R, ncls),))
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            o32 = O.softmax(score, axis=1)
            assert np.array_equal(np.isnan(sm), np.isnan(o32)), "softmax NaN pattern %s" % ((R, ncls),)
            finite = np.isfinite(score).all(axis=1)
            assert finite.sum() >= max(1, R - 8) and not np.isnan(sm[finite]).any()
            p64 = softmax64(score[finite])
        e_dev, e_ora = float(np.abs(sm[finite] - p64).max()), float(np.abs(o32[finite] - p64).max())
        print("HEADLOSS softmax R=%d ncls=%d im=%dx%d: device %.3e oracle %.3e" % (R, ncls, im_h, im_w, e_dev, e_ora))
        FIGURES.append(("softmax", (R, ncls, im_h, im_w), e_dev, e_ora))
        assert e_dev <= 4 * e_ora + ULP1, (R, ncls, e_dev, e_ora)
        # frcnn_head_decode_stacked: scores in [0, ncls), deltas from dcol, seeded noise everywhere else
        rs = np.random.RandomState(seed + 7)
        for ld, dcol in stacked_layouts(rt, ncls):
            out = (rs.randn(R, ld) * 50).astype(np.float32)
            out[:, :ncls] = score
            out[:, dcol:dcol + 4 * ncls] = deltas
            sb, sp = rt.head_decode_stacked(bd, dev(rt, out), ncls, dcol, im_h, im_w)
            assert_same_words(host(rt, sb), pb_h, "stacked boxes %s" % ((R, ncls, ld, dcol),))
            assert_same_words(host(rt, sp), pp_h, "stacked probabilities vs head_decode %s" % ((R, ncls, ld, dcol),))
            assert_same_words(host(rt, sp), sm, "stacked probabilities vs softmax_rows %s" % ((R, ncls, ld, dcol),))
        # frcnn_class_dets on the device's own outputs, specials included
        if ncls >= 2:
            want = np.stack([np.hstack((pb_h[:, 4 * c:4 * c + 4], pp_h[:, c:c + 1])) for c in range(1, ncls)])
            assert_same_words(host(rt, rt.class_dets(pp, pb)), want, "class_dets %s" % ((R, ncls),))


def check_head_status(rt):
    """What the epilogue's entry points refuse before any launch (the outputs keep their poison), and R = 0."""
    L, m = rt.lib, rt.mem
    R, ncls = 5, 21
    boxes, deltas, score = head_inputs(R, ncls, 600, 1000, 3)
    bd = dev(rt, boxes)
    pred, prob = dev(rt, np.full((R, 4 * ncls), POISON)), dev(rt, np.full((R, ncls), POISON))
    out = dev(rt, np.zeros((R, 256), np.float32))

    def stacked(ld, dcol, n=ncls, r=R):
        return L.frcnn_head_decode_stacked(m.ptr(bd), m.ptr(out), ld, dcol, r, n, 600, 1000, m.ptr(pred), m.ptr(prob), m.stream())
    assert stacked(118, 32) == INVALID            # ld % 4
    assert stacked(120, 30) == INVALID            # dcol % 4
    assert stacked(120, 20) == INVALID            # dcol < ncls
    assert stacked(112, 32) == INVALID            # dcol + 4 * ncls > ld
    assert stacked(116, 36) == INVALID
    assert stacked(116, 32, n=0) == INVALID and stacked(116, 32, r=-1) == INVALID
    assert L.frcnn_head_decode_stacked(None, m.ptr(out), 116, 32, R, ncls, 600, 1000, m.ptr(pred), m.ptr(prob), m.stream()) == INVALID
    assert stacked(116, 32, r=0) == 0             # nothing to do
    m.synchronize()
    assert (host(rt, pred) == POISON).all() and (host(rt, prob) == POISON).all()
    assert stacked(116, 32) == 0 and stacked(256, 172) == 0        # the smallest ld for dcol = 32, and the largest dcol for ld = 256
    m.synchronize()
    assert not (host(rt, pred) == POISON).any() and not (host(rt, prob) == POISON).any()
    # frcnn_class_dets: R = 0 is an empty result (nothing launched, nothing written); one class has no detections to list
    dets = dev(rt, np.full((ncls - 1, 1, 5), POISON))
    assert L.frcnn_class_dets(m.ptr(prob), m.ptr(pred), 0, ncls, m.ptr(dets), m.stream()) == 0
    assert L.frcnn_class_dets(m.ptr(prob), m.ptr(pred), R, 1, m.ptr(dets), m.stream()) == INVALID
    assert L.frcnn_class_dets(m.ptr(prob), m.ptr(pred), -1, ncls, m.ptr(dets), m.stream()) == INVALID
    m.synchronize()
    assert (host(rt, dets) == POISON).all() and host(rt, dets)[:, :0].shape == (ncls - 1, 0, 5)
    one = dev(rt, np.zeros((1, 4), np.float32))
    assert L.frcnn_clip_boxes(m.ptr(one), -1, 600, 1000, m.stream()) == INVALID and L.frcnn_clip_boxes(None, 1, 600, 1000, m.stream()) == INVALID
    assert L.frcnn_softmax_rows(m.ptr(one), 1, 0, m.ptr(one), m.stream()) == INVALID
    assert L.frcnn_bbox_transform_inv(m.ptr(one), m.ptr(one), 1, 0, m.ptr(one), m.stream()) == INVALID
    del deltas, score


# ------------------------------------------------------------------------------------------- 2. frcnn_rcnn_loss
RCNN_R = [1, 128, 255, 256, 257, 300, 1000]    # one row per thread of the 256, the boundary, several rows per thread
RCNN_NCLS = [2, 5, 21]


def rcnn_inputs(R, ncls, seed, delta=1.0, big=False):
    """Logits of 6 sigma (big: +-1e4 mixed in), targets non-zero only in the label's four columns (ProposalTargetLayer), bbox_pred spread
    over both Huber branches, one element at |d| == delta exactly, all-equal score rows (arg-max = the first maximum)."""
    rs = np.random.RandomState(seed)
    score = (rs.randn(R, ncls) * 6).astype(np.float32)
    if big:
        pick = rs.randint(0, 3, (R, ncls))
        score = np.where(pick == 0, np.float32(1e4), np.where(pick == 1, np.float32(-1e4), score)).astype(np.float32)
    labels = rs.randint(0, ncls, R).astype(np.int32)
    bbox = (rs.randn(R, 4 * ncls) * 1.0).astype(np.float32)
    targets = np.zeros((R, 4 * ncls), np.float32)
    for r in range(R):
        if labels[r] > 0:
            targets[r, 4 * labels[r]:4 * labels[r] + 4] = rs.randn(4).astype(np.float32)
    free = 4 * ((int(labels[0]) + 1) % ncls)     # a column of row 0 whose target is zero
    bbox[0, free] = np.float32(delta)             # |d| == delta exactly: the linear branch, by `ad < delta`
    bbox[0, free + 1] = np.float32(-delta)
    if R >= 4:
        # all-equal rows: the first maximum is class 0, so rows 1 and 3 count as right and row 2 as wrong (a last-maximum rule would
        # count one right and two wrong: the three rows cannot cancel)
        score[1] = np.float32(1.25); labels[1] = 0
        score[2] = np.float32(-3.0); labels[2] = ncls - 1
        score[3] = np.float32(0.0); labels[3] = 0
        targets[1:4] = 0
        targets[2, 4 * (ncls - 1):] = np.float32(0.5)
    return score, bbox, labels, targets


def rcnn_ref64(score, bbox, labels, targets, delta):
    R = score.shape[0]
    s = score.astype(np.float64)
    mx = s.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(s - mx).sum(axis=1, keepdims=True)))[:, 0]
    picked = s[np.arange(R), labels]
    lc = float((lse - picked).mean())
    scale_c = float(np.maximum(np.abs(lse), np.abs(picked)).mean())
    p = np.exp(s - lse[:, None])
    onehot = np.zeros_like(p)
    onehot[np.arange(R), labels] = 1.0
    gs = (p - onehot) / R
    d = bbox.astype(np.float64) - targets.astype(np.float64)
    a = np.abs(d)
    lb = float(np.where(a < delta, 0.5 * d * d, delta * (a - 0.5 * delta)).sum() / R)
    gb = np.where(a < delta, d, delta * np.sign(d)) / R
    return lc, lb, scale_c, gs, gb


def check_rcnn_loss(rt, R, ncls, seed=0, delta=1.0, big=False):
    score, bbox, labels, targets = rcnn_inputs(R, ncls, seed, delta, big)
    lc64, lb64, scale_c, gs64, gb64 = rcnn_ref64(score, bbox, labels, targets, delta)
    olc, olb, oacc, ogs, ogb = O.rcnn_loss_grads(score, bbox, labels, targets, delta)
    args = [dev(rt, a) for a in (score, bbox, labels, targets)]
    losses, ds, db = rt.rcnn_loss(*args, delta=delta)
    got, ds, db = host(rt, losses), host(rt, ds), host(rt, db)
    # accuracy: exact, first maximum
    acc = np.float32((np.argmax(score, axis=1) == labels).mean())
    assert got[2] == acc and oacc == acc, (got[2], acc, oacc)
    assert np.isfinite(got).all() and np.isfinite(ds).all() and np.isfinite(db).all()
    # gradients against the float64 closed forms, the oracle's own error as the yardstick
    tag = "R=%d ncls=%d%s" % (R, ncls, " +-1e4" if big else "")
    for name, g, o, g64 in (("d_cls_score", ds, ogs, gs64), ("d_bbox_pred", db, ogb, gb64)):
        e_dev = float(np.abs(g - g64).max() / np.abs(g64).max())
        e_ora = float(np.abs(o - g64).max() / np.abs(g64).max())
        print("HEADLOSS rcnn_loss %s %s: device %.3e oracle %.3e" % (tag, name, e_dev, e_ora))
        FIGURES.append((name, (R, ncls, int(big)), e_dev, e_ora))
        assert e_dev <= 4 * e_ora + ULP1, (tag, name, e_dev, e_ora)
    # losses: 4 x the oracle's error + 4 fp32 ulps of the scale
    for name, l, o, l64, scale in (("loss_cls", got[0], olc, lc64, scale_c), ("loss_bbox", got[1], olb, lb64, lb64)):
        e_dev, e_ora = abs(float(l) - l64), abs(float(o) - l64)
        bar = 4 * e_ora + 4 * float(np.spacing(np.float32(scale)))
        print("HEADLOSS rcnn_loss %s %s: device %.3e oracle %.3e (value %.6g, scale %.6g, bar %.3e)" % (tag, name, e_dev, e_ora, l64, scale, bar))
        FIGURES.append((name, (R, ncls, int(big)), e_dev / max(scale, 1e-30), e_ora / max(scale, 1e-30)))
        assert e_dev <= bar, (tag, name, float(l), l64, e_dev, e_ora, bar)
    # want_grad=False: the same three words; a second call: identical words everywhere (one workgroup, a fixed reduction tree)
    only = host(rt, rt.rcnn_loss(*args, delta=delta, want_grad=False))
    assert np.array_equal(words(only), words(got))
    l2, ds2, db2 = rt.rcnn_loss(*args, delta=delta)
    assert np.array_equal(words(host(rt, l2)), words(got))
    assert np.array_equal(words(host(rt, ds2)), words(ds)) and np.array_equal(words(host(rt, db2)), words(db))


def check_rcnn_loss_status(rt):
    L, m = rt.lib, rt.mem
    R, ncls = 4, 5
    score, bbox, labels, targets = rcnn_inputs(R, ncls, 0)
    s, b, l, t = [dev(rt, a) for a in (score, bbox, labels, targets)]
    losses = dev(rt, np.full((3,), POISON))
    ds, db = dev(rt, np.full((R, ncls), POISON)), dev(rt, np.full((R, 4 * ncls), POISON))

    def call(r, n, pds, pdb):
        return L.frcnn_rcnn_loss(m.ptr(s), m.ptr(b), m.ptr(l), m.ptr(t), r, n, 1.0, m.ptr(losses), pds, pdb, m.stream())
    assert call(0, ncls, m.ptr(ds), m.ptr(db)) == INVALID and call(-3, ncls, m.ptr(ds), m.ptr(db)) == INVALID
    assert call(R, 1, m.ptr(ds), m.ptr(db)) == INVALID and call(R, 0, m.ptr(ds), m.ptr(db)) == INVALID
    assert call(R, ncls, m.ptr(ds), None) == INVALID and call(R, ncls, None, m.ptr(db)) == INVALID        # exactly one gradient pointer
    m.synchronize()
    assert (host(rt, losses) == POISON).all() and (host(rt, ds) == POISON).all() and (host(rt, db) == POISON).all()
    assert call(R, ncls, None, None) == 0 and call(R, ncls, m.ptr(ds), m.ptr(db)) == 0
    m.synchronize()
    assert not (host(rt, losses) == POISON).any() and not (host(rt, ds) == POISON).any() and not (host(rt, db) == POISON).any()


# ------------------------------------------------------------------------------------------- 3. frcnn_rpn_loss at its edges
def rpn_case(fh, fw, A, n_in, seed, sigma=1.0, delta=3.0):
    """Synthetic anchor targets on an fh x fw map with A anchors per cell: n_in ascending inside indices, labels from {-1, 0, 1},
    targets of 1 sigma, bbox_pred spread beyond delta, and one |d| == delta exactly."""
    rs = np.random.RandomState(seed)
    n_all = A * fh * fw
    inds = np.sort(rs.permutation(n_all)[:n_in]).astype(np.int64)
    labels = rs.randint(-1, 2, n_in).astype(np.int32)
    targets = rs.randn(n_in, 4).astype(np.float32)
    score = (rs.randn(1, 2 * A, fh, fw) * sigma).astype(np.float32)
    bbox = (rs.randn(1, 4 * A, fh, fw) * 2).astype(np.float32)
    if n_in:
        j = n_in // 2
        k, a = int(inds[j]) // A, int(inds[j]) % A
        targets[j, 1] = 0.0
        bbox[0, 1 * A + a, k // fw, k % fw] = np.float32(delta)         # channel = coord * A + a
    return score, bbox, labels, targets, inds


def check_rpn_loss_case(rt, fh, fw, A, score, bbox, labels, targets, inds, delta=3.0):
    """check_rpn_loss's comparison (the same oracle functions and tolerances) on given operands, + gradient entries outside `inds` are
    exactly zero, + want_grad=False returns the same words."""
    n_all = A * fh * fw
    lc, acc = O.rpn_loss_cls(score, labels, inds, n_all, fh, fw, n_anchors=A)
    lb = O.rpn_loss_bbox(bbox, targets, inds, n_anchors=A, delta=delta)
    _, _, gs, gb = O.rpn_loss_grads(score, bbox, labels, targets, inds, n_all, fh, fw, n_anchors=A, delta=delta)
    ops = (dev(rt, score[0]), dev(rt, bbox[0]), dev(rt, labels), dev(rt, targets), dev(rt, inds.astype(np.int32)), len(inds), A, fh, fw)
    losses, ds, db = rt.rpn_loss(*ops, delta=delta)
    got, ds, db = host(rt, losses), host(rt, ds), host(rt, db)
    assert np.allclose(got, [lc, lb, acc], rtol=1e-5, atol=1e-6), (got, lc, lb, acc)
    assert np.allclose(ds, gs[0], rtol=1e-4, atol=1e-7)
    assert np.allclose(db, gb[0], rtol=1e-4, atol=1e-9)
    inside = np.zeros((fh * fw, A), bool)
    inside.reshape(-1)[inds] = True                                      # idx = k * A + a
    outside = ~inside.T.reshape(A, fh, fw)
    assert not words(ds.reshape(2, A, fh, fw)[:, outside]).any() and not words(db.reshape(4, A, fh, fw)[:, outside]).any()
    ignored = np.zeros((fh * fw, A), bool)
    ignored.reshape(-1)[inds[labels == -1]] = True
    assert not words(ds.reshape(2, A, fh, fw)[:, ignored.T.reshape(A, fh, fw)]).any()
    only = host(rt, rt.rpn_loss(*ops, delta=delta, want_grad=False))
    assert np.array_equal(words(only), words(got))
    return got, ds, db


def check_rpn_loss_all_ignored(rt, fh=14, fw=14, A=9, seed=0):
    """Every label -1: loss_cls and the accuracy are 0 (the count's floor of 1), d_cls_score is all zero, the bbox terms are unchanged."""
    score, bbox, labels, targets, inds = rpn_case(fh, fw, A, 700, seed)
    ref, _, db_ref = check_rpn_loss_case(rt, fh, fw, A, score, bbox, labels, targets, inds)
    got, ds, db = check_rpn_loss_case(rt, fh, fw, A, score, bbox, np.full_like(labels, -1), targets, inds)
    assert words(got)[0] == 0 and words(got)[2] == 0 and ref[0] > 0
    assert not words(ds).any()
    assert words(got)[1] == words(ref)[1] and np.array_equal(words(db), words(db_ref))


def check_rpn_loss_no_inside(rt, fh=6, fw=8, A=9, seed=0):
    """n_inside = 0 with NULL label / target / index pointers: all three losses are 0 and both gradients are all zero."""
    rs = np.random.RandomState(seed)
    score = rs.randn(2 * A, fh, fw).astype(np.float32)
    bbox = rs.randn(4 * A, fh, fw).astype(np.float32)
    losses, ds, db = rt.rpn_loss(dev(rt, score), dev(rt, bbox), None, None, None, 0, A, fh, fw)
    assert not words(host(rt, losses)).any() and not words(host(rt, ds)).any() and not words(host(rt, db)).any()
    only = rt.rpn_loss(dev(rt, score), dev(rt, bbox), None, None, None, 0, A, fh, fw, want_grad=False)
    assert not words(host(rt, only)).any()
    # with anchors to read, the three pointers are required
    L, m = rt.lib, rt.mem
    s, b, out = dev(rt, score), dev(rt, bbox), dev(rt, np.full((3,), POISON))
    assert L.frcnn_rpn_loss(m.ptr(s), m.ptr(b), None, None, None, 5, A, fh, fw, 3.0, 1.0, m.ptr(out), None, None, m.stream()) == INVALID
    m.synchronize()
    assert (host(rt, out) == POISON).all()


def check_rpn_loss_edges(rt, fh, fw, A, n_in, seed=0, sigma=1.0):
    score, bbox, labels, targets, inds = rpn_case(fh, fw, A, n_in, seed, sigma)
    check_rpn_loss_case(rt, fh, fw, A, score, bbox, labels, targets, inds)


# ------------------------------------------------------------------------------------------- 4. glue kernels
GATHER_SHAPES = [(1, 5, 1), (37, 300, 84), (128, 300, 25088), (300, 300, 21)]       # n, rows, cols
TRANSPOSE_SHAPES = [(1, 1), (63, 65), (64, 64), (65, 63), (129, 1), (300, 21), (84, 4096)]
BIG_N = 8192 * 256 + 1000                       # more elements than the capped grid has threads: the stride loop


def check_gather_scatter(rt, n, rows, cols, seed=0):
    L, m = rt.lib, rt.mem
    rs = np.random.RandomState(seed)
    idx = rs.permutation(rows)[:n].astype(np.int32)                     # unsorted, unique
    src = rs.randn(rows, cols).astype(np.float32)
    got = host(rt, rt.gather_rows(dev(rt, src), dev(rt, idx)))
    assert got.shape == (n, cols) and np.array_equal(words(got), words(src[idx]))
    part = rs.randn(n, cols).astype(np.float32)
    want = np.zeros((rows, cols), np.float32)
    want[idx] = part
    got = host(rt, rt.scatter_rows(dev(rt, part), dev(rt, idx), rows))
    assert got.shape == (rows, cols) and np.array_equal(words(got), words(want))
    # into a buffer full of NaN: the rows nobody writes are still zero
    dst = dev(rt, np.full((rows, cols), np.nan, np.float32))
    pd, pi = dev(rt, part), dev(rt, idx)
    assert L.frcnn_scatter_rows_f32(m.ptr(pd), m.ptr(pi), n, cols, m.ptr(dst), rows, m.stream()) == 0
    m.synchronize()
    assert np.array_equal(words(host(rt, dst)), words(want))


def check_scatter_nothing(rt, rows=7, cols=13):
    L, m = rt.lib, rt.mem
    dst = dev(rt, np.full((rows, cols), np.nan, np.float32))
    assert L.frcnn_scatter_rows_f32(None, None, 0, cols, m.ptr(dst), rows, m.stream()) == 0
    m.synchronize()
    assert not words(host(rt, dst)).any()
    got = rt.scatter_rows(dev(rt, np.zeros((1, cols), np.float32))[:0], dev(rt, np.zeros((1,), np.int32))[:0], rows)
    assert tuple(got.shape) == (rows, cols) and not words(host(rt, got)).any()
    assert L.frcnn_scatter_rows_f32(None, None, 3, cols, m.ptr(dst), rows, m.stream()) == INVALID
    assert L.frcnn_scatter_rows_f32(None, None, 0, cols, m.ptr(dst), 0, m.stream()) == INVALID
    assert L.frcnn_gather_rows_f32(m.ptr(dst), None, 3, cols, m.ptr(dst), m.stream()) == INVALID


def check_gather_int32_words(rt):
    """The int32 arg-max rows of the RoI pooling go through the `float` kernel: words that are NaN payloads (quiet and signalling, either
    sign), infinities and 0x80000000 come back unchanged, with a repeated index too."""
    specials = np.array([0x7fc00000, 0x7fc12345, 0x7f800001, 0xffc00000, 0xff800001, 0x7fffffff, 0xffffffff, 0x80000000, 0x7f800000,
                         0xff800000, 0x00000001, 0x80000001, 0, 1234567], np.uint32)
    rs = np.random.RandomState(0)
    src = specials[rs.randint(0, len(specials), (9, 50))]
    src[:, :len(specials)] = specials
    idx = np.array([3, 3, 8, 0, 5, 3, 1], np.int32)
    got = rt.gather_rows(dev(rt, src.view(np.int32)), dev(rt, idx))
    assert rt.mem.dtype_of(got) == "i32"
    got = host(rt, got)
    assert got.dtype == np.int32 and np.array_equal(got.view(np.uint32), src[idx])
    # ... and as fp32 rows
    got = host(rt, rt.gather_rows(dev(rt, src.view(np.float32)), dev(rt, idx)))
    assert np.array_equal(words(got), src[idx])


def check_mul_add(rt, n, seed=0):
    rs = np.random.RandomState(seed)
    a, b = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    for fn, want in ((rt.mul, a * b), (rt.add, a + b)):
        assert np.array_equal(words(host(rt, fn(dev(rt, a), dev(rt, b)))), words(want))
        ad, bd = dev(rt, a), dev(rt, b)
        y = fn(ad, bd, out=ad)                                           # out aliases the first operand
        assert np.array_equal(words(host(rt, y)), words(want)) and np.array_equal(words(host(rt, bd)), words(b))
        ad, bd = dev(rt, a), dev(rt, b)
        y = fn(ad, bd, out=bd)                                           # ... the second
        assert np.array_equal(words(host(rt, y)), words(want)) and np.array_equal(words(host(rt, ad)), words(a))


def check_relu_bwd(rt, n=5 * 1000 + 3, seed=0):
    """g = out > 0 ? g : 0, in place: -0.0 and NaN in `out` close the gate, a NaN in g passes an open one"""
    rs = np.random.RandomState(seed)
    x = np.abs(rs.randn(n)).astype(np.float32) + np.float32(0.01)
    out = x.copy()
    out[1::5] = 0.0
    out[2::5] = -0.0
    out[3::5] = np.nan
    out[4::5] = -x[4::5]
    g = rs.randn(n).astype(np.float32)
    g[::10] = np.nan                                                     # some where out > 0, some where not
    g[3::15] = np.inf
    want = np.where(out > 0, g, np.float32(0)).astype(np.float32)
    assert np.isnan(want).any() and (out[::10] > 0).any()
    gd = dev(rt, g)
    got = host(rt, rt.relu_bwd_(gd, dev(rt, out)))
    assert_same_words(got, want, "relu_bwd")
    assert np.array_equal(np.isnan(got), np.isnan(want))


def check_transpose(rt, rows, cols, seed=0):
    a = np.random.RandomState(seed).randn(rows, cols).astype(np.float32)
    got = host(rt, rt.transpose(dev(rt, a)))
    assert got.shape == (cols, rows) and np.array_equal(words(got), words(np.ascontiguousarray(a.T)))
    out = dev(rt, np.full((cols, rows), POISON))
    rt.transpose(dev(rt, a), out=out)
    assert np.array_equal(words(host(rt, out)), words(np.ascontiguousarray(a.T)))


# ------------------------------------------------------------------------------------------- 6. anchor-target ground-truth edges
def anchor_target_edge_gts():
    """name -> (fh, fw, im_h, im_w, gt (G, 5)) for parity_cases.check_anchor_target's comparison"""
    import parity_cases as P
    rs = np.random.RandomState(5)
    cases = {}
    cases["one_gt"] = (14, 14, 224, 224, P.gt_case(rs, 1, 224, 224)[0])
    g = P.gt_case(rs, 3, 224, 224)[0]
    cases["duplicated_row"] = (14, 14, 224, 224, np.vstack([g, g[1:2]]))
    cases["G33"] = (38, 63, 600, 1000, P.gt_case(rs, 33, 600, 1000)[0])
    cases["G300"] = (38, 63, 600, 1000, P.gt_case(rs, 300, 600, 1000)[0])
    g = P.gt_case(rs, 2, 224, 224)[0]
    g[1, :4] = [5000.0, -4000.0, 5100.0, -3900.0]
    cases["far_outside"] = (14, 14, 224, 224, g)
    anchors = O.generate_all_bbox(O.generate_anchors(), 14, 14, 16)
    _, inside = O.keep_inside(anchors, np.array([224, 224]))
    g = P.gt_case(rs, 2, 224, 224)[0]
    g[0, :4] = inside[len(inside) // 2]
    cases["equals_an_anchor"] = (14, 14, 224, 224, g)
    g = P.gt_case(rs, 2, 224, 224)[0]
    g[1, :4] = [100.0, 90.0, 100.0, 90.0]
    cases["one_pixel"] = (14, 14, 224, 224, g)
    g = P.gt_case(rs, 2, 224, 224)[0]
    g[0, :4] = [60.0, 40.0, 59.0, 120.0]                                 # x2 - x1 + 1 == 0
    cases["zero_width"] = (14, 14, 224, 224, g)
    cases["im600x901"] = (38, 57, 600, 901, P.gt_case(rs, 4, 600, 901)[0])
    return cases


ANCHOR_TARGET_EDGES = ["one_gt", "duplicated_row", "G33", "G300", "far_outside", "equals_an_anchor", "one_pixel", "zero_width", "im600x901"]


def check_anchor_target_edge(rt, name):
    import parity_cases as P
    fh, fw, im_h, im_w, gt = anchor_target_edge_gts()[name]
    with np.errstate(all="ignore"):
        n = P.check_anchor_target(rt, fh, fw, im_h, im_w, len(gt), gt=np.ascontiguousarray(gt, dtype=np.float32)[None])
    assert n > 0
