"""Parity checks of the C-ABI entry points against the oracle, written once and run twice:
  * tests/test_kernels_emulated.py  -- on the host-emulated kernels (CPU, -m "not gpu"): kernel LOGIC
  * tests/test_gpu_parity.py        -- on libfrcnn_hip.so on a real MI355X (-m gpu): the parity tests proper
Every function takes a Runtime (`rt`).  Tolerances are stated where they are used:
  indices / survivors / argmax: bit-exact;  fp32 features: <= 1e-3 relative (north_star)."""
import os

import numpy as np

from oracle import frcnn_oracle as O
from chainer_faster_rcnn_amd import tuning

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def g(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def dev(rt, a):
    return rt.mem.from_numpy(np.ascontiguousarray(a))


def host(rt, a):
    return rt.mem.to_numpy(a)


# ------------------------------------------------------------------------------------------- NMS
def check_nms_golden(rt, tags=("n6000_t07", "n300_t03", "n1_t07", "n65_t05")):
    G = g("cpu_nms")
    for tag in tags:
        dets, thr, want = G[tag + "_dets"], float(G[tag + "_thresh"]), G[tag + "_keep"]
        keep, n = rt.nms(dev(rt, dets), thr)
        n = int(host(rt, n)[0])
        assert n == len(want), (tag, n, len(want))
        assert np.array_equal(host(rt, keep)[:n], want.astype(np.int32)), tag          # bit-exact survivors
        # keep[:k] semantics of proposal_layer.py:189-190
        keep2, n2 = rt.nms(dev(rt, dets), thr, max_out=10)
        k = min(10, len(want))
        assert int(host(rt, n2)[0]) == k and np.array_equal(host(rt, keep2)[:k], want[:k].astype(np.int32))


def check_nms_edges(rt):
    G = g("cpu_nms")
    for thr in (0.7, 0.5, 0.3):      # `ovr >= thresh` compared in double (cpu_nms.pyx:18,66)
        keep, n = rt.nms(dev(rt, G["edge_dets"]), thr)
        n = int(host(rt, n)[0])
        assert host(rt, keep)[:n].tolist() == G["edge_keep_%02d" % int(thr * 10)].tolist(), thr
    keep, n = rt.nms(rt.mem.empty((0, 5), "f32"), 0.7)       # empty input
    assert int(host(rt, n)[0]) == 0
    # ties in score: canonical rule = ascending index among equals
    d = np.array([[0, 0, 10, 10, 0.5], [100, 100, 110, 110, 0.5], [200, 200, 210, 210, 0.9],
                  [1, 1, 11, 11, 0.5]], np.float32)
    keep, n = rt.nms(dev(rt, d), 0.5)
    assert host(rt, keep)[:int(host(rt, n)[0])].tolist() == [2, 0, 1]
    # all boxes identical -> one survivor; thresh 0 -> `0 >= 0` suppresses even disjoint boxes
    same = np.tile(np.array([[5, 5, 50, 50, 0.0]], np.float32), (130, 1))
    same[:, 4] = np.linspace(1, 0, 130)
    keep, n = rt.nms(dev(rt, same), 0.7)
    assert int(host(rt, n)[0]) == 1 and int(host(rt, keep)[0]) == 0
    assert O.cpu_nms(d, 0.0) == host(rt, rt.nms(dev(rt, d), 0.0)[0])[:1].tolist() == [2]


def check_nms_random_box_sets(rt, sizes=(1, 2, 63, 64, 65, 129), seeds=(0, 1)):
    """frcnn_nms against cpu_nms.pyx's arithmetic on random box sets: sparse and crowded, scores from a continuum and from seven values (ties everywhere: the
    kernels visit equal scores in ascending index -- the oracle's tie_rule; without ties NumPy's own order gives the same list), thresholds 0.3 / 0.5 / 0.7.
    (scripts/r06_nms_sweep.py ran 396 such cases up to n = 12000 on the MI355X.)"""
    for n in sizes:
        for seed in seeds:
            rs = np.random.RandomState(1000 * seed + n)
            for dens, tied in ((0.3, False), (3.0, True), (30.0, True)):
                span = max(60.0, np.sqrt(n / dens) * 40.0)
                xy = rs.uniform(0, span, (n, 2))
                sc = rs.choice(np.linspace(0.05, 0.95, 7), n) if tied else rs.uniform(0, 1, n)
                d = np.hstack([xy, xy + rs.uniform(8, 120, (n, 2)), sc[:, None]]).astype(np.float32)
                for thr in (0.3, 0.5, 0.7):
                    want = O.cpu_nms(d, thr, tie_rule="ascending_index")
                    keep, cnt = rt.nms(dev(rt, d), thr)
                    k = int(host(rt, cnt)[0])
                    assert host(rt, keep)[:k].tolist() == want, (n, seed, dens, tied, thr)
                    if len(np.unique(d[:, 4])) == n:
                        assert O.cpu_nms(d, thr) == want


def check_gpu_nms_ffi(rt, tags=("n6000_t07", "n300_t03", "n65_t05", "n1_t07")):
    """`_nms` with the reference's exact C signature (models/gpu_nms.hpp:9-10) through the gpu_nms.pyx-shaped binding: host arrays
    in, list out, equal to the reference's cpu_nms on the reference-generated golden vectors -- including threshold 0.3, where
    nms_kernel.cu's fp32 `>` and cpu_nms's double `>=` differ (the threshold is narrowed to a C float by the FFI and recovered)."""
    from chainer_faster_rcnn_amd.models import gpu_nms
    from chainer_faster_rcnn_amd._lib import FrcnnError
    G = g("cpu_nms")
    for tag in tags:
        dets, thr, want = G[tag + "_dets"], float(G[tag + "_thresh"]), G[tag + "_keep"]
        assert [int(v) for v in gpu_nms(dets, thr, 0, lib=rt.lib)] == want.tolist(), tag
    for thr in (0.7, 0.5, 0.3):          # boxes whose IoU sits exactly on the float32 neighbours of the threshold
        assert [int(v) for v in gpu_nms(G["edge_dets"], thr, 0, lib=rt.lib)] == G["edge_keep_%02d" % int(thr * 10)].tolist(), thr
    wide = np.hstack([G["n65_t05_dets"], np.full((65, 2), 7.0, np.float32)])          # boxes_dim = 7: only the first five columns count
    assert [int(v) for v in gpu_nms(wide, 0.5, 0, lib=rt.lib)] == G["n65_t05_keep"].tolist()
    assert gpu_nms(np.zeros((0, 5), np.float32), 0.7, 0, lib=rt.lib) == []
    try:                                  # errors are reported (num_out = -1), not printed and swallowed
        gpu_nms(G["n65_t05_dets"], 0.5, 4096, lib=rt.lib)
        raise AssertionError("an invalid device id must fail")
    except FrcnnError:
        pass
    assert [int(v) for v in gpu_nms(G["n65_t05_dets"], 0.5, 0, lib=rt.lib)] == G["n65_t05_keep"].tolist()   # and the library still works


def check_nms_random(rt, n=700, seeds=(0, 1), thrs=(0.3, 0.5, 0.7)):
    for seed in seeds:
        rs = np.random.RandomState(seed)
        x1 = rs.uniform(0, 300, n); y1 = rs.uniform(0, 300, n)
        d = np.stack([x1, y1, x1 + rs.uniform(1, 200, n), y1 + rs.uniform(1, 200, n),
                      rs.permutation(n) / float(n)], 1).astype(np.float32)
        for thr in thrs:
            want = O.cpu_nms(d, thr)
            keep, nk = rt.nms(dev(rt, d), thr)
            nk = int(host(rt, nk)[0])
            assert host(rt, keep)[:nk].tolist() == want, (seed, thr)


def check_nms_staged(rt, n=1200, seeds=(0, 1)):
    """keep[:max_out] with a small max_out: the two-stage form (mask + scan of the first 4 * max_out boxes, then -- only if that did
    not yield max_out survivors -- of the rest).  Sparse boxes finish in stage one; a dense pile does not and needs stage two."""
    for seed in seeds:
        rs = np.random.RandomState(seed)
        for dense in (False, True):
            span = 120 if dense else 900
            x1 = rs.uniform(0, span, n); y1 = rs.uniform(0, span, n)
            d = np.stack([x1, y1, x1 + rs.uniform(40, 200, n), y1 + rs.uniform(40, 200, n), rs.permutation(n) / float(n)], 1).astype(np.float32)
            for max_out in (20, 48):
                want = O.cpu_nms(d, 0.7)[:max_out]
                keep, nk = rt.nms(dev(rt, d), 0.7, max_out=max_out)
                nk = int(host(rt, nk)[0])
                assert nk == len(want) and host(rt, keep)[:nk].tolist() == want, (seed, dense, max_out, nk, len(want))
                assert (host(rt, keep)[nk:] == -1).all()


def check_nms_staged_strided_tail(rt):
    """The second-stage mask launch strides a fixed number of workgroups over its tiles: force far fewer workgroups than tiles."""
    with tuning.override(FRCNN_NMS_TAIL_WGS="7"):
        check_nms_staged(rt, n=1200, seeds=(2,))


def check_nms_chains(rt, n=200):
    """Worst cases for the wave-parallel resolve of a 64-box chunk (nms_scan_col_body): suppression CHAINS.  Boxes slide along a line in
    score order so that box i overlaps box i+1 .. i+k above the threshold and nothing beyond: greedy NMS keeps every (k+1)-th box and
    the chunk needs one resolve round per kept box (k = 1: 32 rounds per chunk).  Also a pile of identical boxes (one survivor) and a
    max_out cut that falls inside a chunk."""
    for step, thr in ((10.0, 0.7), (4.0, 0.7), (30.0, 0.3), (1.0, 0.5)):
        x1 = np.arange(n, dtype=np.float64) * step
        d = np.stack([x1, np.zeros(n), x1 + 99.0, np.full(n, 49.0), 1.0 - np.arange(n) / float(n)], 1).astype(np.float32)
        want = O.cpu_nms(d, thr)
        for max_out in (0, 7, len(want) - 1):
            w = want if max_out <= 0 else want[:max_out]
            keep, nk = rt.nms(dev(rt, d), thr, max_out=max_out)
            nk = int(host(rt, nk)[0])
            assert nk == len(w) and host(rt, keep)[:nk].tolist() == w, (step, thr, max_out, nk, len(w))
    d = np.tile(np.array([[10, 10, 60, 60, 0]], np.float32), (130, 1)); d[:, 4] = 1.0 - np.arange(130) / 130.0
    keep, nk = rt.nms(dev(rt, d), 0.7)
    assert int(host(rt, nk)[0]) == 1 and int(host(rt, keep)[0]) == 0


def check_nms_batched(rt, groups=5, n=300):
    """forward.py:48-58: per-class cpu_nms(thresh=0.3) on (300,5) -- all classes in one call."""
    rs = np.random.RandomState(5)
    x1 = rs.uniform(0, 500, (groups, n)); y1 = rs.uniform(0, 400, (groups, n))
    d = np.stack([x1, y1, x1 + rs.uniform(10, 300, (groups, n)), y1 + rs.uniform(10, 200, (groups, n)),
                  rs.rand(groups, n)], 2).astype(np.float32)
    keep, nk = rt.nms_batched(dev(rt, d), 0.3)
    keep, nk = host(rt, keep), host(rt, nk)
    for k in range(groups):
        want = O.cpu_nms(d[k], 0.3)
        assert nk[k] == len(want) and keep[k, :nk[k]].tolist() == want and (keep[k, nk[k]:] == -1).all()


# ------------------------------------------------------------------------------------------- proposals
def check_proposals_golden(rt, case):
    G = g(case)
    anchors = O.generate_anchors()
    pre, post = int(G["pre"]), int(G["post"])
    im_h, im_w = [int(v) for v in G["img_info"][0]]
    rois, probs, n_out, src = rt.proposals(dev(rt, G["rpn_cls_prob"][0]), dev(rt, G["rpn_bbox_pred"][0]), anchors, 16,
                                           im_h, im_w, 16.0, pre, post, 0.7, want_index=True)
    n = int(host(rt, n_out)[0])
    want_p, want_s = G["proposals"], G["probs"].ravel()
    want_src = G["keep0"][G["order"]][G["nms_keep"][:len(want_p)]]
    assert n == len(want_p), (case, n, len(want_p))
    got_src = host(rt, src)[:n]
    assert np.array_equal(got_src, want_src.astype(np.int32)), case                 # bit-exact proposal indices
    assert np.array_equal(host(rt, probs)[:n], want_s), case                         # scores are copied, exact
    # coordinates: exp() is evaluated in double then rounded (NumPy's SIMD fp32 exp is ~1-2 ulp) -> 4 ulp slack
    got = host(rt, rois)[:n]
    assert np.allclose(got, want_p, rtol=5e-7, atol=1e-4), (case, np.abs(got - want_p).max())
    assert (host(rt, rois)[n:] == 0).all() and (host(rt, src)[n:] == -1).all()
    # ... and against the oracle evaluated with that correctly rounded exp (and the kernel's order of equal scores): coordinates bit for bit
    exp_was = O.EXP
    O.EXP = lambda v: np.exp(np.asarray(v, np.float64)).astype(np.float32)
    try:
        p4, s4, d4 = O.proposal_layer(G["rpn_cls_prob"], G["rpn_bbox_pred"], G["img_info"], train=bool(G["train"]), pre_nms_top_n=pre, post_nms_top_n=post,
                                      return_debug=True, tie_rule="ascending_index")
    finally:
        O.EXP = exp_was
    assert np.array_equal(got, p4) and np.array_equal(got_src, d4["src_index"].astype(np.int32)), (case, np.abs(got - p4).max())
    return n


def check_proposals_tied_scores(rt, fh=14, fw=14, seed=0):
    """Equal scores (fp32 softmax outputs of 20 000 anchors tie exactly about a dozen times per image; NumPy's argsort leaves their order
    implementation-defined, in proposal_layer.py:156-157 and again in cpu_nms.pyx:26): the kernels order them by ascending anchor index, in the
    sort AND in the order NMS visits them -- the oracle's tie_rule="ascending_index".  Scores drawn from EIGHT values, so nearly everything ties."""
    rs = np.random.RandomState(seed)
    A = 9
    fgv = rs.choice(np.linspace(0.1, 0.9, 8).astype(np.float32), size=(A, fh, fw))
    prob = np.concatenate([1 - fgv, fgv], 0)[None].astype(np.float32)
    pred = (rs.randn(1, 4 * A, fh, fw) * 0.3).astype(np.float32)
    info = np.array([[fh * 16, fw * 16]], np.int32)
    exp_was = O.EXP
    O.EXP = lambda v: np.exp(np.asarray(v, np.float64)).astype(np.float32)
    try:
        for train, (pre, post) in ((False, (6000, 300)), (True, (12000, 2000)), (False, (50, 20))):
            want_p, want_s, d = O.proposal_layer(prob, pred, info, train=train, pre_nms_top_n=pre, post_nms_top_n=post, return_debug=True, tie_rule="ascending_index")
            rois, probs, n_out, src = rt.proposals(dev(rt, prob[0]), dev(rt, pred[0]), O.generate_anchors(), 16, fh * 16, fw * 16, 16.0, pre, post, 0.7, want_index=True)
            n = int(host(rt, n_out)[0])
            assert n == len(want_p), (n, len(want_p))
            assert np.array_equal(host(rt, src)[:n], d["src_index"].astype(np.int32))
            assert np.array_equal(host(rt, probs)[:n], want_s.ravel()) and np.array_equal(host(rt, rois)[:n], want_p)
    finally:
        O.EXP = exp_was


PROPOSAL_EDGE_TAGS = ("posnan", "negnan", "infs", "negnan_inf", "negnan_train", "deltas")
NMS_EDGE_TAGS = ("negnan_score", "posnan_score", "nan_x1", "nan_y2", "inf_score", "inf_x2")


def check_proposals_edge_goldens(rt, tags=PROPOSAL_EDGE_TAGS):
    """SURVEY 8a-9 / 8a-11's named inputs, fixtures made by the reference's own ProposalLayer (tests/make_golden.py edge_cases):
    a NaN score of EITHER sign bit is ordered first (NumPy's argsort()[::-1]; 0xFFC00000 is what x86 makes of inf - inf), +-inf
    scores, NaN / +-inf deltas, exp() overflow.  Source indices bit-exact, scores bit-exact (NaN payload included)."""
    G = g("edge_cases")
    anchors = O.generate_anchors()
    for tag in tags:
        train = bool(G["p_%s_train" % tag])
        pre, post = (12000, 2000) if train else (6000, 300)
        rois, probs, n_out, src = rt.proposals(dev(rt, G["p_%s_prob" % tag][0]), dev(rt, G["p_%s_pred" % tag][0]), anchors, 16, 224, 224,
                                               16.0, pre, post, 0.7, want_index=True)
        n = int(host(rt, n_out)[0])
        want_p, want_s, want_src = G["p_%s_proposals" % tag], G["p_%s_probs" % tag].ravel(), G["p_%s_src" % tag]
        assert n == len(want_p), (tag, n, len(want_p))
        assert np.array_equal(host(rt, src)[:n], want_src.astype(np.int32)), (tag, host(rt, src)[:8], want_src[:8])
        assert np.array_equal(host(rt, probs)[:n].view(np.uint32), want_s.view(np.uint32)), tag
        got = host(rt, rois)[:n]
        assert np.isfinite(got).all() and np.allclose(got, want_p, rtol=5e-7, atol=1e-4), (tag, np.abs(got - want_p).max())


def check_nms_edge_goldens(rt, tags=NMS_EDGE_TAGS, ffi=True):
    """cpu_nms.pyx on a NaN score of either sign, an infinite score, a NaN / infinite coordinate (the reference's max / min helpers
    are not symmetric in NaN: cpu_nms.pyx:12-16) -- frcnn_nms, the batched form and `_nms` give the reference's keep list."""
    G = g("edge_cases")
    for tag in tags:
        dets = G["n_%s_dets" % tag]
        for thr in (0.7, 0.3):
            want = G["n_%s_keep_%02d" % (tag, int(thr * 10))]
            keep, n = rt.nms(dev(rt, dets), thr)
            n = int(host(rt, n)[0])
            assert n == len(want) and np.array_equal(host(rt, keep)[:n], want.astype(np.int32)), (tag, thr, n, len(want))
            kb, nb = rt.nms_batched(dev(rt, np.stack([dets, dets[::-1].copy()])), thr)
            assert int(host(rt, nb)[0]) == len(want) and np.array_equal(host(rt, kb)[0, :len(want)], want.astype(np.int32)), (tag, thr)
            if ffi:
                from chainer_faster_rcnn_amd.models import gpu_nms
                assert [int(v) for v in gpu_nms(dets, thr, 0, lib=rt.lib)] == want.tolist(), (tag, thr)


# ------------------------------------------------------------------------------------------- RoI pooling
def roi_case(rs, R, C=512, H=38, W=63):
    x = np.abs(rs.randn(1, C, H, W)).astype(np.float32)
    rois = np.zeros((R, 5), np.float32)
    x1 = rs.uniform(0, (W - 2) * 16, R); y1 = rs.uniform(0, (H - 2) * 16, R)
    rois[:, 1], rois[:, 2] = x1, y1
    rois[:, 3] = np.minimum(x1 + rs.uniform(0, 500, R), W * 16 - 9)
    rois[:, 4] = np.minimum(y1 + rs.uniform(0, 400, R), H * 16 - 9)
    k = max(R // 5, 1)
    rois[:k, 1:] = np.round(rois[:k, 1:] / 8) * 8      # exact .5 after *1/16: round-half-even cases
    if R > 3:
        rois[k] = [0, (W - 1) * 16, (H - 1) * 16, W * 16 - 9, H * 16 - 9]   # tiny
        rois[k + 1] = [0, W * 16 + 200, H * 16 + 100, W * 16 + 300, H * 16 + 200]   # outside: empty bins
        rois[k + 2] = [0, 0, 0, W * 16 - 9, H * 16 - 9]                      # whole map
    if R >= 12:     # what ProposalLayer's clipped output never holds but the public ABI accepts
        rois[k + 3] = [0, -1e4, -1e4, 2e4, 2e4]                             # far larger than the map on every side
        rois[k + 4] = [0, W * 12, H * 12, W * 4, H * 4]                      # reversed corners: extent max(., 1)
        rois[k + 5] = [0, -50, -70, W * 8, H * 8]                            # negative corner
        rois[k + 6] = [0, W * 8, H * 8, W * 8, H * 8]                        # a one-point RoI
        rois[k + 7] = [0, -3e6, 100, 1e6, 200]                               # huge one way only
        rois[k + 8] = [0, -50, -70, -10, -20]                                # wholly outside, negative side
    return x, rois


def check_roi_pool(rt, R=12, C=128, H=38, W=63, seed=0):
    rs = np.random.RandomState(seed)
    x, rois = roi_case(rs, R, C, H, W)
    want_y, want_am = O.roi_pooling_2d(x, rois, 7, 7, 0.0625, return_argmax=True)
    y, am = rt.roi_pool_fwd(dev(rt, x[0]), dev(rt, rois), 7, 7, 0.0625, want_argmax=True)
    assert np.array_equal(host(rt, am), want_am)            # bit-exact argmax
    assert np.array_equal(host(rt, y), want_y)              # max of fp32 values: exact (tolerance 1e-3 unused)
    y2 = rt.roi_pool_fwd(dev(rt, x[0]), dev(rt, rois), 7, 7, 0.0625)          # inference path (no argmax)
    assert np.array_equal(host(rt, y2), want_y)
    y3 = rt.roi_pool_fwd_chw(dev(rt, x[0]), dev(rt, np.ascontiguousarray(rois[:, 1:])), 7, 7, 0.0625)   # bare (R,4) rois
    assert np.array_equal(host(rt, y3), want_y)
    if hasattr(rt, "roi_pool_fwd_chw_bf16") and C >= 8 and W <= 64:                # bf16-output form: ONE rounding of the fp32 maximum
        _, want_bits = to_bf16(want_y.reshape(R, -1))
        y5 = host(rt, rt.roi_pool_fwd_chw_bf16(dev(rt, x[0]), dev(rt, np.ascontiguousarray(rois[:, 1:])), 7, 7, 0.0625))
        assert np.array_equal(y5.view(np.uint16), want_bits.view(np.uint16).reshape(y5.shape))
    xt = rt.chw_to_hwc(dev(rt, x[0]))                                          # channel-last gather kernel (any map size)
    y4, am4 = rt.roi_pool_fwd_hwc(xt, C, H, W, dev(rt, rois), 7, 7, 0.0625, want_argmax=True)
    assert np.array_equal(host(rt, y4), want_y) and np.array_equal(host(rt, am4), want_am)
    dy = rs.randn(*want_y.shape).astype(np.float32)
    dx = rt.roi_pool_bwd(dev(rt, dy), am, C, H, W)
    want_dx = O.roi_pooling_2d_backward(dy, want_am, rois, x.shape)
    assert np.allclose(host(rt, dx), want_dx, rtol=1e-4, atol=1e-4)    # atomics: summation order differs
    # the other backward forms (csrc/roi_pool.hip: channels per workgroup; the round-1 global-atomic kernel, also the path of maps beyond the LDS planes)
    for form in ("n1", "n2", "n4", "atomic"):
        if C % int(form[1:] if form[0] == "n" else 1):
            continue
        with tuning.override(FRCNN_ROI_BWD=form):
            dx2 = rt.roi_pool_bwd(dev(rt, dy), am, C, H, W)
        assert np.allclose(host(rt, dx2), want_dx, rtol=1e-4, atol=1e-4), form


def check_roi_pool_extreme_rois(rt):
    """the public ABI takes any RoI, not only ProposalLayer's clipped output.  RoIs far larger than the map (round 5's quad kernel
    clamped the bin OFFSET at 255 cells before adding a far-away origin and lost every bin of [-1e4, -1e4, 2e4, 2e4]; the plane kernel read 12 columns
    of a 63-column bin), reversed, negative, one-point, wholly outside, up to the header's stated domain |v * scale| <= 2^24 -- on every forward kernel:
    quads (38 x 63, both forms), cells, planes (forced, and as the arg-max default of a 45-row map), the channel-last gather (90 x 70)."""
    rois = np.array([[0, -1e4, -1e4, 2e4, 2e4], [0, -1e5, -1e5, 1e5, 1e5], [0, -3e6, -2e6, 1e6, 4e6], [0, 500, 300, 100, 50], [0, -50, -70, -10, -20],
                     [0, -50, -70, 60, 80], [0, 100, 100, 100, 100], [0, 5e3, 5e3, 6e3, 6e3], [0, -1e4, 100, 2e4, 200], [0, 100, -1e4, 300, 2e4],
                     [0, 0, 0, 1e6, 1e6], [0, -2.6e8, -2.6e8, 2.6e8, 2.6e8], [0, -1023 * 16, -1023 * 16, 16 * 40, 16 * 30], [0, 37, 41, 333, 222]], np.float32)
    rs = np.random.RandomState(11)
    for (C, H, W) in [(16, 38, 63), (8, 45, 40), (8, 90, 70)]:
        x = np.abs(rs.randn(1, C, H, W)).astype(np.float32)
        want, wam = O.roi_pooling_2d(x, rois, 7, 7, 0.0625, return_argmax=True)
        assert (want[0, :, 2, 2] == x[0].reshape(C, -1).max(axis=1)).all() and (wam[0, :, 0, 0] == -1).all()   # the whole map lies in bin (2, 2) of the first RoI
        for sel in (None, "planes", "cells"):
            with tuning.override(FRCNN_ROI_KERNEL=sel):
                y, am = rt.roi_pool_fwd(dev(rt, x[0]), dev(rt, rois), 7, 7, 0.0625, want_argmax=True)
                assert np.array_equal(host(rt, y), want) and np.array_equal(host(rt, am), wam), (C, H, W, sel, "argmax form")
                y2 = rt.roi_pool_fwd(dev(rt, x[0]), dev(rt, rois), 7, 7, 0.0625)
                assert np.array_equal(host(rt, y2), want), (C, H, W, sel)
        y4, am4 = rt.roi_pool_fwd_hwc(rt.chw_to_hwc(dev(rt, x[0])), C, H, W, dev(rt, rois), 7, 7, 0.0625, want_argmax=True)
        assert np.array_equal(host(rt, y4), want) and np.array_equal(host(rt, am4), wam)
        if W <= 64 and hasattr(rt, "roi_pool_fwd_chw_bf16"):
            _, want_bits = to_bf16(want.reshape(len(rois), -1))
            y5 = host(rt, rt.roi_pool_fwd_chw_bf16(dev(rt, x[0]), dev(rt, np.ascontiguousarray(rois[:, 1:])), 7, 7, 0.0625))
            assert np.array_equal(y5.view(np.uint16), want_bits.view(np.uint16).reshape(y5.shape))
            xb = to_bf16(x)[0]
            got = host(rt, rt.roi_pool_fwd_blk_bf16(rt.bf16_from_nchw(dev(rt, xb)), C, dev(rt, rois[:, 1:].copy()), 7, 7, 0.0625))
            assert np.array_equal(got, O.roi_pooling_2d(xb, rois, 7, 7, 0.0625))


def check_roi_pool_cells(rt):
    """The cell-major inference kernel (maps up to 76 x 64): ragged channel counts, non-7x7 outputs, the tall-map instantiation,
    RoIs larger than the bin tables, and the oracle's NaN rule -- a NaN in a bin's FIRST cell stays, NaNs elsewhere never win."""
    for (R, C, H, W, oh, ow, seed) in [(23, 16, 38, 63, 7, 7, 0), (9, 11, 19, 32, 7, 7, 1), (11, 8, 50, 40, 7, 7, 2), (7, 24, 12, 17, 3, 5, 3),
                                        (5, 8, 38, 63, 1, 1, 4), (6, 8, 76, 64, 6, 7, 5)]:
        rs = np.random.RandomState(seed)
        x, rois = roi_case(rs, R, C, H, W)
        if seed == 0:                                   # NaNs: top-left cell of some bins, and interior cells
            x[0, 3, 5, 7] = np.nan
            x[0, 3, 6, 9] = np.nan
            x[0, 12, 0, 0] = np.nan
            x[0, 5, 20, 30:34] = np.nan
            rois[0] = [0, 7 * 16, 5 * 16, 30 * 16, 20 * 16]        # bin (0,0) starts exactly at the NaN cell (5,7)
            rois[1] = [0, 0, 0, 40 * 16, 30 * 16]
            rois[2] = [0, 30 * 16, 20 * 16, 33 * 16, 20 * 16]      # a one-row RoI made of NaNs
        if seed == 2:
            rois[0] = [0, -3000, -2000, 9000, 7000]                 # extent >= 72 cells: the arithmetic path
        want = O.roi_pooling_2d(x, rois, oh, ow, 0.0625)
        got = host(rt, rt.roi_pool_fwd(dev(rt, x[0]), dev(rt, rois), oh, ow, 0.0625))
        assert np.array_equal(np.isnan(got), np.isnan(want)), (R, C, H, W)
        assert np.array_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0)), (R, C, H, W, oh, ow)
        if W <= 64 and hasattr(rt, "roi_pool_fwd_chw_f32s") and seed in (0, 1, 3, 5):     # split-tensor output: h + m + l == the fp32 maxima
            ysp = rt.roi_pool_fwd_chw_f32s(dev(rt, x[0]), dev(rt, np.ascontiguousarray(rois[:, 1:])), oh, ow, 0.0625)
            back = host(rt, rt.f32s_join(ysp)).reshape(want.shape)
            assert np.array_equal(np.isnan(back), np.isnan(want)) and np.array_equal(np.nan_to_num(back, nan=-1.0), np.nan_to_num(want, nan=-1.0))
        if W <= 64 and hasattr(rt, "roi_pool_fwd_chw_bf16") and seed in (1, 3):
            _, want_bits = to_bf16(want.reshape(R, -1))
            y5 = host(rt, rt.roi_pool_fwd_chw_bf16(dev(rt, x[0]), dev(rt, np.ascontiguousarray(rois[:, 1:])), oh, ow, 0.0625))
            assert np.array_equal(y5.view(np.uint16), want_bits.view(np.uint16).reshape(y5.shape))


def check_roi_pool_cells_batches(rt):
    """More RoIs per workgroup than one geometry batch holds (128 slots for the 38-row image, 32 for the 76-row one): force ONE RoI
    group per channel group so a workgroup walks all the RoIs in several batches."""
    with tuning.override(FRCNN_ROI_RSPLIT="1"):
        for (R, C, H, W, seed) in [(300, 8, 12, 17, 7), (70, 8, 50, 40, 8)]:
            rs = np.random.RandomState(seed)
            x, rois = roi_case(rs, R, C, H, W)
            want = O.roi_pooling_2d(x, rois, 7, 7, 0.0625)
            got = host(rt, rt.roi_pool_fwd(dev(rt, x[0]), dev(rt, rois), 7, 7, 0.0625))
            assert np.array_equal(got, want), (R, C, H, W)


def check_roi_pool_blk_bf16(rt, R, C, H, W, seed=0):
    """RoI pooling straight from the bf16 chain's channel-blocked map == the oracle's pooling of the same (bf16-valued) map, bit for
    bit -- fp32 output and raw-bf16 output (a maximum of bf16 values is one of them: no rounding happens)."""
    rs = np.random.RandomState(seed)
    x, rois = roi_case(rs, R, C, H, W)
    xb = to_bf16(x)[0]                                                   # the map's values ARE bf16 numbers
    want = O.roi_pooling_2d(xb, rois, 7, 7, 0.0625)
    blk = rt.bf16_from_nchw(dev(rt, xb))
    assert np.array_equal(from_bf16_bits(host(rt, blk)).transpose(0, 3, 1, 2).reshape(-1, H, W)[:C], xb[0])      # the layout the kernel reads
    got = host(rt, rt.roi_pool_fwd_blk_bf16(blk, C, dev(rt, rois[:, 1:].copy()), 7, 7, 0.0625))
    assert got.shape == want.shape and np.array_equal(got, want), (R, C, H, W)
    bits = host(rt, rt.roi_pool_fwd_blk_bf16(blk, C, dev(rt, rois), 7, 7, 0.0625, out_bf16=True))
    assert np.array_equal(from_bf16_bits(bits).reshape(want.shape), want)


# ------------------------------------------------------------------------------------------- conv stack
def check_conv3x3(rt, Cin, Cout, H, W, cfg=-1, seed=0, relu=True):
    rs = np.random.RandomState(seed)
    x = rs.randn(1, Cin, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = rs.randn(Cout).astype(np.float32) * 0.1
    want = O.conv2d(x, w, b, 1)
    if relu:
        want = O.relu(want)
    wp = rt.pack_conv3x3_w(dev(rt, w))
    assert np.array_equal(host(rt, wp), w.reshape(Cout, Cin * 9).T)
    y = rt.conv3x3(dev(rt, x), wp, dev(rt, b), relu=relu, cfg=cfg)
    got = host(rt, y)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)
    assert got.shape == want.shape and err < 1e-4, (Cin, Cout, H, W, cfg, err)     # well inside the 1e-3 budget
    return err


def check_maxpool(rt, C, H, W, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(1, C, H, W).astype(np.float32)
    assert np.array_equal(host(rt, rt.maxpool2x2(dev(rt, x))), O.max_pool_2x2(x))


def check_rpn_heads(rt, Cmid=128, H=9, W=13, A=9, seed=0):
    rs = np.random.RandomState(seed)
    h = np.abs(rs.randn(1, Cmid, H, W)).astype(np.float32)
    p = {"RPN/rpn_cls_score/W": (rs.randn(2 * A, Cmid, 1, 1) * 0.05).astype(np.float32),
         "RPN/rpn_cls_score/b": (rs.randn(2 * A) * 0.1).astype(np.float32),
         "RPN/rpn_bbox_pred/W": (rs.randn(4 * A, Cmid, 1, 1) * 0.05).astype(np.float32),
         "RPN/rpn_bbox_pred/b": (rs.randn(4 * A) * 0.1).astype(np.float32)}
    score = O.conv2d(h, p["RPN/rpn_cls_score/W"], p["RPN/rpn_cls_score/b"], 0)
    prob = O.softmax(score, axis=1)        # 18-way, region_proposal_network.py:119
    bbox = O.conv2d(h, p["RPN/rpn_bbox_pred/W"], p["RPN/rpn_bbox_pred/b"], 0)
    packed = rt.rpn_heads_pack(dev(rt, p["RPN/rpn_cls_score/W"].reshape(2 * A, Cmid)), dev(rt, p["RPN/rpn_cls_score/b"]),
                               dev(rt, p["RPN/rpn_bbox_pred/W"].reshape(4 * A, Cmid)), dev(rt, p["RPN/rpn_bbox_pred/b"]))
    s, pr, bb = rt.rpn_heads(dev(rt, h), packed)
    assert np.allclose(host(rt, s), score, rtol=1e-4, atol=1e-5)
    assert np.allclose(host(rt, pr), prob, rtol=1e-4, atol=1e-6)
    assert np.allclose(host(rt, bb), bbox, rtol=1e-4, atol=1e-5)
    assert np.allclose(host(rt, pr).sum(axis=1), 1.0, atol=1e-5)
    return host(rt, s), host(rt, pr), host(rt, bb)


def check_rpn_heads_forms(rt, monkeypatch, **kw):
    """The fused heads launch (K split over the workgroup's waves, softmax on the tile) against the two-launch form (the 1x1 case of
    the convolution kernel + softmax_channels_kernel): same values up to the order of the fp32 additions, and the probabilities are
    the same softmax operations applied to the fused launch's own scores."""
    fused = check_rpn_heads(rt, **kw)
    tuning.set("FRCNN_RPN_HEADS", "conv")
    conv = check_rpn_heads(rt, **kw)
    tuning.set("FRCNN_RPN_HEADS", None)
    for a, b in zip(fused, conv):
        assert np.abs(a - b).max() <= 2e-6 * max(np.abs(b).max(), 1.0)
    s = fused[0].astype(np.float32)
    e = np.exp(s - s.max(axis=1, keepdims=True), dtype=np.float32)
    assert np.abs(fused[1] - e / e.sum(axis=1, keepdims=True, dtype=np.float32)).max() <= 1e-6


def check_linear(rt, M, N, K, relu, seed=0, bias=True):
    """bias=False: the NULL-bias form of the ABI (the training step's dW / dx products; a single-slab plan then writes y directly)."""
    rs = np.random.RandomState(seed)
    x = rs.randn(M, K).astype(np.float32)
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float32)
    b = rs.randn(N).astype(np.float32) * 0.1 if bias else np.zeros((N,), dtype=np.float32)
    want = O.linear(x, w, b)
    if relu:
        want = O.relu(want)
    got = host(rt, rt.linear(dev(rt, x), dev(rt, w), dev(rt, b) if bias else None, relu=relu))
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)
    assert got.shape == want.shape and err < 1e-4, (M, N, K, err)
    # the two accumulator orientations of the LDS-DMA kernel (default where N % 4 == 0: MFMA operands swapped, 16-byte slab stores): bit for bit
    from chainer_faster_rcnn_amd import tuning
    with tuning.override(FRCNN_LINEAR_F32_TRN="0"):
        got0 = host(rt, rt.linear(dev(rt, x), dev(rt, w), dev(rt, b) if bias else None, relu=relu))
    assert np.array_equal(got0, got), (M, N, K)


def check_head_decode(rt, R=37, ncls=21, seed=0):
    from head_loss_cases import assert_same_words, ref_boxes
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 500, (R, 2))
    boxes = np.hstack([xy, xy + rs.uniform(16, 400, (R, 2))]).astype(np.float32)
    deltas = (rs.randn(R, 4 * ncls) * 0.3).astype(np.float32)
    score = rs.randn(R, ncls).astype(np.float32) * 3
    _, want_boxes = ref_boxes(boxes, deltas, 600, 1000)     # the oracle's restatement with exp evaluated in double and rounded to fp32, as csrc/head.hip does
    want_prob = O.softmax(score, axis=1)
    pb, pp = rt.head_decode(dev(rt, boxes), dev(rt, deltas), dev(rt, score), 600, 1000)
    assert_same_words(host(rt, pb), want_boxes, "head_decode boxes")         # word for word: operation order, no FMA contraction, that exp
    assert np.allclose(host(rt, pp), want_prob, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------- training step
def gt_case(rs, G, im_h, im_w):
    """VOC-shaped ground truth (datasets/pascal_voc_dataset.py:44-47): (1,G,5) float32 [x1,y1,x2,y2,cls]."""
    w = rs.uniform(32, min(400, im_w - 2), G); h = rs.uniform(32, min(400, im_h - 2), G)
    x1 = rs.uniform(0, im_w - 1 - w); y1 = rs.uniform(0, im_h - 1 - h)
    return np.stack([x1, y1, x1 + w, y1 + h, rs.randint(1, 21, G)], axis=1).astype(np.float32)[None]


def check_bbox_overlaps(rt, N=500, K=7, seed=0):
    rs = np.random.RandomState(seed)
    a = rs.uniform(0, 300, (N, 2)); b = rs.uniform(0, 300, (K, 2))
    boxes = np.hstack([a, a + rs.uniform(0, 200, (N, 2))]); q = np.hstack([b, b + rs.uniform(0, 200, (K, 2))])
    got = host(rt, rt.bbox_overlaps(dev(rt, boxes), dev(rt, q)))
    assert np.array_equal(got, O.bbox_overlaps(boxes, q))                      # float64, same operation order: exact


def check_anchor_target(rt, fh, fw, im_h, im_w, G, seed=0, gt=None):
    """`gt`: a given (1, G, 5) ground truth in place of the seeded VOC-shaped one (tests/head_loss_cases.py: its edges)"""
    rs = np.random.RandomState(seed)
    gt = gt_case(rs, G, im_h, im_w) if gt is None else gt
    assert gt.shape == (1, G, 5) and gt.dtype == np.float32
    info = np.array([[im_h, im_w]], dtype=np.int32)

    class NoSubsample(object):          # the device entry point stops before the random subsample
        @staticmethod
        def choice(a, size, replace):
            return a[:0]
    want_l, want_t, want_i, n_all = O.anchor_target_layer(fh, fw, gt, info, rng=NoSubsample)
    inds, n_in, labels, targets, argmax = rt.anchor_target(O.generate_anchors(), fh, fw, 16, im_h, im_w, dev(rt, gt[0]))
    n = int(host(rt, n_in)[0])
    assert n == len(want_i) and n_all == 9 * fh * fw
    assert np.array_equal(host(rt, inds)[:n], want_i)
    assert np.array_equal(host(rt, labels)[:n], want_l)
    assert np.allclose(host(rt, targets)[:n], want_t, rtol=2e-7, atol=1e-7)    # float64 log, then rounded to float32
    return n


def check_anchor_target_empty_cases(rt):
    """anchor_target_layer.py:188-190 on an image without ground truth, or too small for any anchor to lie inside: NumPy's ValueError in the reference
    (checked against the live class: oracle/ref_harness) -- and in the mirror."""
    import pytest
    from chainer_faster_rcnn_amd.models.anchor_target_layer import AnchorTargetLayer
    atl = AnchorTargetLayer(runtime=rt)
    for gt, fh, fw, im_h, im_w in ((np.zeros((1, 0, 5), np.float32), 14, 14, 224, 224), (np.array([[[10, 10, 50, 50, 1]]], np.float32), 6, 8, 96, 128)):
        with pytest.raises(ValueError, match="empty sequence"):
            O.anchor_target_layer(fh, fw, gt, np.array([[im_h, im_w]], np.int32))
        with pytest.raises(ValueError, match="empty sequence"):
            atl.forward_device(fh, fw, dev(rt, gt), im_h, im_w)


def check_rpn_loss(rt, fh=14, fw=14, im=224, G=3, seed=0):
    rs = np.random.RandomState(seed)
    gt = gt_case(rs, G, im, im)
    info = np.array([[im, im]], dtype=np.int32)
    labels, targets, inds, n_all = O.anchor_target_layer(fh, fw, gt, info, rng=np.random.RandomState(seed))
    score = rs.randn(1, 18, fh, fw).astype(np.float32)
    bbox = (rs.randn(1, 36, fh, fw) * 2).astype(np.float32)                    # some |d| beyond delta = 3
    lc, acc = O.rpn_loss_cls(score, labels, inds, n_all, fh, fw)
    lb = O.rpn_loss_bbox(bbox, targets, inds)
    _, _, gs, gb = O.rpn_loss_grads(score, bbox, labels, targets, inds, n_all, fh, fw)
    losses, ds, db = rt.rpn_loss(dev(rt, score[0]), dev(rt, bbox[0]), dev(rt, labels), dev(rt, targets), dev(rt, inds.astype(np.int32)),
                                 len(inds), 9, fh, fw)
    got = host(rt, losses)
    assert np.allclose(got, [lc, lb, acc], rtol=1e-5, atol=1e-6), (got, lc, lb, acc)
    assert np.allclose(host(rt, ds), gs[0], rtol=1e-4, atol=1e-7)
    assert np.allclose(host(rt, db), gb[0], rtol=1e-4, atol=1e-9)
    only = host(rt, rt.rpn_loss(dev(rt, score[0]), dev(rt, bbox[0]), dev(rt, labels), dev(rt, targets), dev(rt, inds.astype(np.int32)),
                                len(inds), 9, fh, fw, want_grad=False))
    assert np.array_equal(only, got)


def check_conv_backward(rt, Cin, Cout, H, W, ksize=3, seed=0):
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.randn(1, Cin, H, W), 0).astype(np.float32)               # a ReLU output: the mask of the fused epilogue
    w = (rs.randn(Cout, Cin, ksize, ksize) * np.sqrt(2.0 / (Cin * ksize * ksize))).astype(np.float32)
    b = np.zeros(Cout, np.float32)
    dy = rs.randn(1, Cout, H, W).astype(np.float32)
    want_dx, want_dw, want_db = O.conv2d_backward(x, w, b, dy, ksize // 2)
    wp = dev(rt, np.ascontiguousarray(w.reshape(Cout, Cin * ksize * ksize).T))   # forward-packed (Cin*k*k, Cout)
    # weight gradient, forward-packed layout
    dwp = host(rt, rt.conv_wgrad(dev(rt, x), dev(rt, dy), ksize))
    want_dwp = want_dw.reshape(Cout, Cin * ksize * ksize).T
    assert np.abs(dwp - want_dwp).max() <= 1e-4 * max(np.abs(want_dwp).max(), 1e-6), np.abs(dwp - want_dwp).max()
    # bias gradient
    db = host(rt, rt.bias_grad(dev(rt, dy)))
    assert np.allclose(db, want_db, rtol=1e-4, atol=1e-3)
    # input gradient = the forward kernel on re-packed weights, ReLU mask of x fused in (needs Cin % 64 == 0)
    if Cin % 64 == 0:
        wd = rt.pack_conv_dgrad_w(wp, ksize)
        zero = dev(rt, np.zeros(Cin, np.float32))
        dx = host(rt, rt.conv_ex(dev(rt, dy), wd, zero, ksize, act=2, mask=dev(rt, x)))
        want = want_dx * (x > 0)
        assert np.abs(dx - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6)


def check_conv_relu_pool_train(rt, Cin, Cout, H, W, seed=0):
    """training form of the fused conv + ReLU + 2x2 max-pool (act 5) against the two-launch path (conv + ReLU, then the pool; another tile
    shape, so sums differ in the last bits): the pooled map within 2e-6, every arg-max byte points at a cell within 2e-6 of its window's
    maximum and is the FIRST such cell wherever the maximum is unique by that margin, and the pool's backward pass from the bytes puts
    each gradient value into exactly that cell."""
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.randn(1, Cin, H, W), 0).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = (rs.randn(Cout) * 0.5).astype(np.float32)             # sizeable biases: whole windows end up <= 0
    wp = dev(rt, np.ascontiguousarray(w.reshape(Cout, Cin * 9).T))
    full = host(rt, rt.conv_ex(dev(rt, x), wp, dev(rt, b), 3, act=1))[0]
    pooled, idx = rt.conv_relu_pool_train(dev(rt, x), wp, dev(rt, b))
    pooled, idx_dev = host(rt, pooled)[0], idx
    raw = host(rt, idx_dev)
    assert np.array_equal((raw & 4) != 0, pooled > 0) and raw.max() <= 7          # bit 2: the ReLU mask of the layer above
    idx = raw & 3
    OH, OW = (H + 1) // 2, (W + 1) // 2
    pad = np.full((Cout, 2 * OH, 2 * OW), -np.inf, np.float32)
    pad[:, :H, :W] = full
    cells = np.stack([pad[:, 0::2, 0::2], pad[:, 0::2, 1::2], pad[:, 1::2, 0::2], pad[:, 1::2, 1::2]], axis=-1)     # window scan order
    wmax = cells.max(axis=-1)
    tol = 2e-6 * max(np.abs(full).max(), 1.0)
    assert np.abs(pooled - wmax).max() <= tol
    chosen = np.take_along_axis(cells, idx[..., None].astype(np.int64), axis=-1)[..., 0]
    assert np.all(chosen >= wmax - tol) and idx.max() <= 3
    clear = (np.sort(cells, axis=-1)[..., -1] - np.sort(cells, axis=-1)[..., -2]) > 4 * tol                          # unique maximum
    assert np.array_equal(idx[clear], cells.argmax(axis=-1)[clear])
    zero = wmax <= 0
    assert zero.any() and np.all(idx[zero & (np.abs(cells).max(axis=-1) == 0)] == 0)                                  # all-zero windows: cell 0
    g = rs.randn(Cout, OH, OW).astype(np.float32)
    dx = host(rt, rt.maxpool2x2_bwd_idx(idx_dev, dev(rt, g[None]), H, W))[0]
    want = np.zeros((Cout, 2 * OH, 2 * OW), np.float32)
    for k, (dy_, dx_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        want[:, dy_::2, dx_::2] = np.where(idx == k, g, 0.0)
    assert np.array_equal(dx, want[:, :H, :W])


def check_conv_dgrad_unpool(rt, Cmid, Cout, H2, W2, seed=0):
    """the input-gradient convolution above a fused pool with the pool's backward pass in its epilogue (act 6) against the three-launch
    path: the same convolution masked by pooled > 0 (act 2), then the pool's backward pass from the arg-max bytes -- bit for bit."""
    rs = np.random.RandomState(seed)
    H, W = (H2 + 1) // 2, (W2 + 1) // 2
    # layer below: Cout channels, pre-pool H2 x W2 -> pooled H x W with arg-max bytes (from the device, so that the bytes are the product's own)
    x0 = np.maximum(rs.randn(1, 8, H2, W2), 0).astype(np.float32)
    w0 = (rs.randn(Cout, 8, 3, 3) * 0.2).astype(np.float32)
    b0 = (rs.randn(Cout) * 0.5).astype(np.float32)
    pooled, idx = rt.conv_relu_pool_train(dev(rt, x0), dev(rt, np.ascontiguousarray(w0.reshape(Cout, 72).T)), dev(rt, b0))
    assert tuple(int(v) for v in pooled.shape) == (1, Cout, H, W)
    # layer above: Cout -> Cmid; its input gradient maps Cmid -> Cout
    w1 = (rs.randn(Cmid, Cout, 3, 3) * np.sqrt(2.0 / (Cout * 9))).astype(np.float32)
    wp1 = dev(rt, np.ascontiguousarray(w1.reshape(Cmid, Cout * 9).T))
    wd = rt.pack_conv_dgrad_w(wp1, 3)
    dy = rs.randn(1, Cmid, H, W).astype(np.float32)
    zero = dev(rt, np.zeros(max(Cout, 512), np.float32))
    g_pooled = rt.conv_ex(dev(rt, dy), wd, zero, 3, act=2, mask=pooled)
    want = host(rt, rt.maxpool2x2_bwd_idx(idx, g_pooled, H2, W2))
    got = host(rt, rt.conv_dgrad_unpool(dev(rt, dy), wd, zero, idx, H2, W2))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert (want != 0).any() and (host(rt, pooled) == 0).any()


def check_pack_dgrad_many(rt, seed=0):
    """one-launch re-pack of several layers' input-gradient weights (tiled transposes) == the per-layer kernel == NumPy"""
    rs = np.random.RandomState(seed)
    shapes = [(64, 64, 3), (3, 64, 3), (70, 130, 3), (128, 54, 1), (5, 7, 3)]
    layers, wants = [], []
    for cin, cout, ks in shapes:
        wp = rs.randn(cin * ks * ks, cout).astype(np.float32)
        w4 = wp.reshape(cin, ks * ks, cout)                                              # [ci][tap][co]
        want = np.ascontiguousarray(w4[:, ::-1, :].transpose(2, 1, 0)).reshape(cout * ks * ks, cin)   # [co][rotated tap][ci]
        d_wp = dev(rt, wp)
        one = host(rt, rt.pack_conv_dgrad_w(d_wp, ks))
        assert np.array_equal(one, want)
        layers.append((d_wp, dev(rt, np.full((cout * ks * ks, cin), np.nan, np.float32)), ks))
        wants.append(want)
    rt.pack_conv_dgrad_w_many(layers)
    for (_, wd, _), want in zip(layers, wants):
        assert np.array_equal(host(rt, wd), want)


def check_conv_wgrad_f32s(rt, Cin, Cout, H, W, seed=0):
    """The 3x3 weight gradient as six bf16 MFMA products of 3-way split operands: against a FLOAT64 accumulation of the same fp32
    inputs, next to the fp32 MFMA kernel (same error class)."""
    import torch
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.randn(1, Cin, H, W), 0).astype(np.float32)
    dy = (rs.randn(1, Cout, H, W) * 0.1).astype(np.float32)
    want = torch.nn.grad.conv2d_weight(torch.from_numpy(x).double(), (Cout, Cin, 3, 3), torch.from_numpy(dy).double(), padding=1).numpy()
    want = want.reshape(Cout, Cin * 9).T
    scale = max(np.abs(want).max(), 1e-12)
    got = host(rt, rt.conv_wgrad_f32s(dev(rt, x), dev(rt, dy)))
    nat = host(rt, rt.conv_wgrad(dev(rt, x), dev(rt, dy), 3))
    err, err_n = np.abs(got - want).max() / scale, np.abs(nat - want).max() / scale
    assert err <= 3e-6 and err <= 4 * err_n + 2e-7, (err, err_n)


def check_maxpool_bwd(rt, C, H, W, seed=0):
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.randn(1, C, H, W), 0).astype(np.float32)                 # many exact ties at 0
    dy = rs.randn(1, C, (H + 1) // 2, (W + 1) // 2).astype(np.float32)
    assert np.array_equal(host(rt, rt.maxpool2x2_bwd(dev(rt, x), dev(rt, dy))), O.max_pool_2x2_backward(x, dy))


def check_sgd(rt, n=100003, seed=0):
    rs = np.random.RandomState(seed)
    w, g, v = [rs.randn(n).astype(np.float32) for _ in range(3)]
    want_w, want_v = O.momentum_sgd_wd(w, g, v)
    dw, dv = dev(rt, w), dev(rt, v)
    rt.sgd_momentum_wd(dw, dev(rt, g), dv, 0.001, 0.9, 0.0005)
    assert np.array_equal(host(rt, dw), want_w) and np.array_equal(host(rt, dv), want_v)      # same operation order: exact


# ------------------------------------------------------------------------------------------- ResNet trunk
def check_resnet(rt, blocks, im_h, im_w, n_layers=101, seed=2, tol=1e-3):
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import ResNet
    params = synthetic.resnet_params(n_layers, seed=seed, blocks=blocks)
    x = synthetic.image(seed=6, h=im_h, w=im_w) / 64.0
    want = O.resnet_forward(params, x, blocks=blocks)
    model = ResNet(n_layers, runtime=rt, blocks=blocks)
    model.load_params(params)
    got = host(rt, model(dev(rt, x)))
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)
    assert err < tol, err
    assert np.abs(want).max() > 1e-3 and np.isfinite(want).all()       # the comparison is not vacuous
    return err


def check_resnet_pieces(rt, seed=0):
    import torch
    rs = np.random.RandomState(seed)
    x = rs.randn(1, 5, 13, 18).astype(np.float32)
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x), 3, 2, ceil_mode=True).numpy()
    assert np.array_equal(host(rt, rt.maxpool3x3s2(dev(rt, x))), want)
    assert np.array_equal(host(rt, rt.subsample2(dev(rt, x))), x[:, :, ::2, ::2])
    x3 = rs.randn(1, 3, 21, 30).astype(np.float32)
    cols = host(rt, rt.im2col7x7s2(dev(rt, x3), 152))
    want = torch.nn.functional.unfold(torch.from_numpy(x3), 7, padding=3, stride=2).numpy().reshape(1, 147, 11, 15)
    assert np.array_equal(cols[:, :147], want) and not cols[:, 147:].any()


# ------------------------------------------------------------------------------------------- bf16 convolution stack
_HALF = ["bf16"]          # the 16-bit operand format the helpers below round to: "bf16", or "f16" inside `half_format("f16")`


class half_format(object):
    """`with half_format("f16"): check_conv_bf16(rt.with_half("f16"), ...)` runs a bf16 parity check as the fp16 instantiation's: the oracle is fed
    fp16-rounded operands (NumPy's float16 conversion: round to nearest even, the v_cvt_pk_f16_f32 rule) and bit comparisons read IEEE binary16."""

    def __init__(self, half):
        self.half = half

    def __enter__(self):
        _HALF.append(self.half)

    def __exit__(self, *a):
        _HALF.pop()


def to_bf16(a):
    """float32 -> (the float32 value of its rounding [nearest even] to the current 16-bit format, raw int16 bits)."""
    if _HALF[-1] == "f16":
        with np.errstate(over="ignore"):
            h = np.ascontiguousarray(a, dtype=np.float32).astype(np.float16)
        return h.astype(np.float32), h.view(np.int16)
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return (r << 16).view(np.float32), r.astype(np.uint16).view(np.int16)


def from_bf16_bits(b):
    if _HALF[-1] == "f16":
        return b.view(np.float16).astype(np.float32)
    return (b.view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def blocked_to_hwc(a):
    """[C/16][H][W][16] -> (H, W, C): the channel-blocked layout of the bf16 kernels, flattened for comparisons."""
    cb, h, w, _ = a.shape
    return np.ascontiguousarray(a.transpose(1, 2, 0, 3)).reshape(h, w, cb * 16)


def check_rpn_heads_bf16(rt, Cmid, H, W, A=9, seed=0):
    """The bf16 chain's RPN heads in one launch against the two-launch form (1x1 bf16 convolution writing fp32 NCHW + the channel
    softmax) on the same operands, and against a float64 accumulation of the bf16-rounded operands."""
    rs = np.random.RandomState(seed)
    h = np.abs(rs.randn(1, Cmid, H, W)).astype(np.float32)
    w = (rs.randn(6 * A, Cmid, 1, 1) * 0.05).astype(np.float32)
    b = (rs.randn(6 * A) * 0.1).astype(np.float32)
    hb = rt.bf16_from_nchw(dev(rt, h))
    wp, bd = rt.bf16_pack_conv_w(dev(rt, w), 1), dev(rt, b)
    score, prob, bbox = [host(rt, t) for t in rt.rpn_heads_bf16(hb, wp, bd, Cmid, A)]
    raw = host(rt, rt.conv_bf16(hb, wp, bd, Cmid, 6 * A, 1, relu=False, out_f32_nchw=True))
    prob2 = host(rt, rt.softmax_channels(dev(rt, np.ascontiguousarray(score[0]))))
    scale = np.abs(raw).max()
    assert score.shape == (1, 2 * A, H, W) and bbox.shape == (1, 4 * A, H, W) and prob.shape == (1, 2 * A, H, W)
    assert np.abs(score - raw[:, :2 * A]).max() <= 2e-6 * scale and np.abs(bbox - raw[:, 2 * A:]).max() <= 2e-6 * scale
    assert np.array_equal(prob, prob2)                       # the same softmax operations on the fused launch's own scores
    want = np.einsum("oc,chw->ohw", to_bf16(w)[0].reshape(6 * A, Cmid).astype(np.float64), to_bf16(h)[0][0].astype(np.float64)) + b[:, None, None]
    assert np.abs(np.concatenate([score, bbox], 1)[0] - want).max() <= 2e-6 * scale


def check_conv_bf16(rt, Cin, Cout, H, W, ksize=3, relu=True, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(1, Cin, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, ksize, ksize) * np.sqrt(2.0 / (Cin * ksize * ksize))).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    xb, xbits = to_bf16(x)
    wb, _ = to_bf16(w)
    xd = rt.bf16_from_nchw(dev(rt, x))
    cp = rt.bf16_pad(Cin)
    got_bits = blocked_to_hwc(host(rt, xd))
    assert np.array_equal(got_bits[:, :, :Cin], xbits[0].transpose(1, 2, 0)) and not got_bits[:, :, Cin:].any()    # conversion: exact
    want = O.conv2d(xb, wb, b, ksize // 2)                       # the kernel's operands exactly; fp32 accumulation
    if relu:
        want = O.relu(want)
    wpk = rt.bf16_pack_conv_w(dev(rt, w), ksize)
    y32 = host(rt, rt.conv_bf16(xd, wpk, dev(rt, b), Cin, Cout, ksize, relu=relu, out_f32_nchw=True))
    scale = max(np.abs(want).max(), 1e-6)
    assert np.abs(y32 - want).max() <= 2e-5 * scale, np.abs(y32 - want).max() / scale           # accumulation order only
    y16 = blocked_to_hwc(host(rt, rt.conv_bf16(xd, wpk, dev(rt, b), Cin, Cout, ksize, relu=relu)))
    got = from_bf16_bits(y16)
    assert got.shape == (H, W, rt.bf16_pad(Cout)) and not got[:, :, Cout:].any()
    want_hwc = want[0].transpose(1, 2, 0)
    assert np.all(np.abs(got[:, :, :Cout] - want_hwc) <= np.abs(want_hwc) * 2.0 ** -8 + 1e-5 * scale)     # one bf16 rounding of the output
    back = host(rt, rt.bf16_to_nchw(rt.conv_bf16(xd, wpk, dev(rt, b), Cin, Cout, ksize, relu=relu), Cout))
    assert np.array_equal(back[0], got[:, :, :Cout].transpose(2, 0, 1))


def split_parts_to_nchw(parts, C):
    """[3][CP/16][H][W][16] raw bf16 bits -> the three fp32 terms, each (C, H, W)."""
    out = []
    for p in range(3):
        hwc = from_bf16_bits(blocked_to_hwc(parts[p]))
        out.append(hwc[:, :, :C].transpose(2, 0, 1))
    return out


def check_conv_f32s(rt, Cin, Cout, H, W, relu=True, seed=0, tol=3e-6):
    """fp32 convolution on split (3 x bf16) tensors, csrc/conv_f32s.hip: the conversion is exact (h + m + l == x bit for bit), the
    result is an fp32 convolution -- compared with a FLOAT64 convolution of the same fp32 operands next to the native fp32 MFMA
    kernel (same accuracy class: the two errors may differ by a small factor, not by orders of magnitude) -- and the three output
    forms (fp32 NCHW, split tensor, split tensor after the fused ReLU + 2x2 max-pool) agree exactly with one another."""
    import torch
    rs = np.random.RandomState(seed)
    x = rs.randn(1, Cin, H, W).astype(np.float32)
    x[0, :, 0, 0] = [1e-30 * (i + 1) for i in range(Cin)]                    # tiny magnitudes: the low terms underflow gracefully
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    xd = rt.f32s_from_nchw(dev(rt, x))
    parts = split_parts_to_nchw(host(rt, xd), Cin)
    assert np.array_equal((parts[0] + parts[1]) + parts[2], x[0])            # exact 3-term representation
    assert np.array_equal(host(rt, rt.f32s_to_nchw(xd, Cin)), x)
    want64 = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1).numpy()
    if relu:
        want64 = np.maximum(want64, 0)
    wpk = rt.f32s_pack_conv_w(dev(rt, w))
    bd = dev(rt, b)
    y = host(rt, rt.conv3x3_f32s(xd, wpk, bd, Cin, Cout, relu=relu, out_f32_nchw=True))
    scale = max(np.abs(want64).max(), 1e-6)
    err = np.abs(y - want64).max() / scale
    assert err <= tol, err
    if Cout % 64 == 0:                                                       # the native fp32 MFMA kernel next to it
        yn = host(rt, rt.conv3x3(dev(rt, x), rt.pack_conv3x3_w(dev(rt, w)), bd, relu=relu))
        err_n = np.abs(yn - want64).max() / scale
        assert err <= 4 * err_n + 2e-7, (err, err_n)
    ys = rt.conv3x3_f32s(xd, wpk, bd, Cin, Cout, relu=relu)
    assert np.array_equal(host(rt, rt.f32s_to_nchw(ys, Cout)), y)            # the split output carries the fp32 result exactly
    pad = host(rt, ys)[:, :, :, :, :]
    if rt.bf16_pad(Cout) != Cout:
        assert not blocked_to_hwc(pad[0])[:, :, Cout:].any()
    if relu:
        yp = rt.conv3x3_f32s(xd, wpk, bd, Cin, Cout, relu=True, pool=True)
        assert np.array_equal(host(rt, rt.f32s_to_nchw(yp, Cout)), O.max_pool_2x2(y))
    # training forms: both outputs in one launch, bit-identical to the separate ones; with a mask, y = (mask > 0) ? y : 0
    ys2, yn2 = rt.conv3x3_f32s_train(xd, wpk, bd, Cin, Cout, relu=relu)
    assert np.array_equal(host(rt, yn2), y) and np.array_equal(host(rt, ys2), host(rt, ys))
    mask = (rs.rand(1, Cout, H, W) > 0.4).astype(np.float32) * rs.rand(1, Cout, H, W).astype(np.float32)
    ys3, yn3 = rt.conv3x3_f32s_train(xd, wpk, bd, Cin, Cout, relu=relu, mask=dev(rt, mask))
    assert np.array_equal(host(rt, yn3), np.where(mask > 0, y, 0).astype(np.float32))
    assert np.array_equal(host(rt, rt.f32s_to_nchw(ys3, Cout)), host(rt, yn3))
    _, yn4 = rt.conv3x3_f32s_train(xd, wpk, bd, Cin, Cout, relu=relu, want_split=False, mask=dev(rt, mask))
    assert np.array_equal(host(rt, yn4), host(rt, yn3))


def check_f32s_weight_packs(rt, Cin=20, Cout=40, seed=0):
    """The three ways to split weights agree bit for bit: from Chainer's (Cout,Cin,3,3) array, from the trainer's packed fp32 layout
    (one layer), and the all-layers-in-one-launch form; the input-gradient pack is the forward pack of the flipped / transposed weights."""
    rs = np.random.RandomState(seed)
    w = rs.randn(Cout, Cin, 3, 3).astype(np.float32)
    wp = rt.pack_conv3x3_w(dev(rt, w))                                   # (Cin*9, Cout) fp32
    a = host(rt, rt.f32s_pack_conv_w(dev(rt, w)))
    b = host(rt, rt.f32s_pack_from_packed(wp, Cin, Cout, dgrad=False))
    assert np.array_equal(a, b)
    wt = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))   # (Cin, Cout, 3, 3): channels swapped, taps rotated
    d_want = host(rt, rt.f32s_pack_conv_w(dev(rt, wt)))
    d = host(rt, rt.f32s_pack_from_packed(wp, Cin, Cout, dgrad=True))
    assert np.array_equal(d, d_want)
    f2, d2 = rt.mem.empty(a.shape, "i16"), rt.mem.empty(d.shape, "i16")
    w3 = rs.randn(16, 3, 3, 3).astype(np.float32)
    f3 = rt.mem.empty((3, 1, 9, 16, 16), "i16")
    rt.f32s_pack_many([(wp, f2, d2, Cin, Cout), (rt.pack_conv3x3_w(dev(rt, w3)), f3, None, 3, 16)])
    assert np.array_equal(host(rt, f2), a) and np.array_equal(host(rt, d2), d_want)
    assert np.array_equal(host(rt, f3), host(rt, rt.f32s_pack_conv_w(dev(rt, w3))))


def check_conv1_f32s(rt, Cin, Cout, H, W, relu=True, seed=0):
    """First-layer form (fp32 NCHW image in, split tensor out): against a float64 convolution and against the generic split kernel."""
    import torch
    rs = np.random.RandomState(seed)
    x = (rs.randn(1, Cin, H, W) * 60).astype(np.float32)                    # mean-subtracted pixel magnitudes
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    want64 = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1).numpy()
    if relu:
        want64 = np.maximum(want64, 0)
    ys = rt.conv1_f32s(dev(rt, x), dev(rt, w), dev(rt, b), relu=relu)
    got = host(rt, rt.f32s_to_nchw(ys, Cout))
    scale = np.abs(want64).max()
    assert np.abs(got - want64).max() <= 1e-6 * scale, np.abs(got - want64).max() / scale
    if rt.bf16_pad(Cout) != Cout:
        assert not blocked_to_hwc(host(rt, ys)[0])[:, :, Cout:].any()
    gen = host(rt, rt.conv3x3_f32s(rt.f32s_from_nchw(dev(rt, x)), rt.f32s_pack_conv_w(dev(rt, w)), dev(rt, b), Cin, Cout, relu=relu, out_f32_nchw=True))
    assert np.abs(got - gen).max() <= 1e-6 * scale
    # training form: the trainers' packed fp32 weights in, the split tensor AND fp32 NCHW out -- the same values bit for bit
    ys2, yn2 = rt.conv1_f32s_train(dev(rt, x), rt.pack_conv3x3_w(dev(rt, w)), dev(rt, b), Cout, relu=relu)
    assert np.array_equal(host(rt, ys2), host(rt, ys)) and np.array_equal(host(rt, yn2), got)


def check_conv1_f32(rt, monkeypatch, Cin, Cout, H, W, relu=True, seed=0):
    """conv1_1 of the fp32 chain through frcnn_conv3x3_f32: the first-layer kernel (native fp32 MFMA, 16-byte NCHW stores) against a
    float64 convolution and against the generic kernel on the same call (FRCNN_CONV1_F32=generic)."""
    import torch
    rs = np.random.RandomState(seed)
    x = (rs.randn(1, Cin, H, W) * 60).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    want64 = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1).numpy()
    if relu:
        want64 = np.maximum(want64, 0)
    xd, wp, bd = dev(rt, x), rt.pack_conv3x3_w(dev(rt, w)), dev(rt, b)
    got = host(rt, rt.conv3x3(xd, wp, bd, relu=relu))
    scale = np.abs(want64).max()
    assert got.shape == want64.shape and np.abs(got - want64).max() <= 1e-6 * scale, np.abs(got - want64).max() / scale
    if Cout % 64 == 0:                          # (the generic kernel takes whole 64-cout tiles only)
        tuning.set("FRCNN_CONV1_F32", "generic")
        gen = host(rt, rt.conv3x3(xd, wp, bd, relu=relu))
        tuning.set("FRCNN_CONV1_F32", None)
        assert np.abs(got - gen).max() <= 2e-6 * scale


def rel_err(got, want):
    want = np.asarray(want, dtype=np.float32)
    return float(np.abs(np.asarray(got, dtype=np.float32) - want).max() / max(float(np.abs(want).max()), 1e-30))


def check_f32s_pipeline_small(rt, im_h=22, im_w=37):
    """conv_dtype="f32s" through the model classes on a narrow trunk (conv, fused conv+pool, an unfused pool, the RPN convolution and
    heads): the same fp32 network as conv_dtype="f32", within accumulation-order noise of it and of the oracle."""
    import functools
    import train_cases as T
    from chainer_faster_rcnn_amd.models import FasterRCNN, VGG16Prev
    params = T.small_params(seed=3)
    x = np.random.RandomState(5).randn(1, 3, im_h, im_w).astype(np.float32)
    outs = {}
    for dt in ("f32", "f32s"):
        model = FasterRCNN(trunk_class=functools.partial(VGG16Prev, layers=T.SMALL_LAYERS), rpn_in_ch=64, rpn_mid_ch=64, feat_stride=4,
                           anchor_scales=(2, 4, 8), runtime=rt, conv_dtype=dt)
        model.trunk.load_params(params, "trunk/")
        model.RPN.load_params(params, "RPN/")
        feat = model.trunk(dev(rt, x))
        xs = getattr(model.trunk, "feat_split", None)
        h, score, prob, bbox = model.RPN.heads(feat, want_score=True, x_split=xs)
        outs[dt] = [host(rt, t) for t in (feat, h, prob, bbox)]
        if dt == "f32s":
            model.trunk.fuse_pool = False                              # the unfused pool path agrees with the fused one exactly ...
            model.trunk.generic_first_layer = True
            assert np.array_equal(host(rt, model.trunk(dev(rt, x))), outs[dt][0])
            model.trunk.generic_first_layer = False                    # ... and the first-layer kernel (fp32 NCHW image in) to rounding
            assert rel_err(host(rt, model.trunk(dev(rt, x))), outs[dt][0]) <= 2e-6
    h_ = x
    for l in T.SMALL_LAYERS:
        h_ = O.max_pool_2x2(h_) if l == "pool" else O.relu(O.conv2d(h_, params["trunk/%s/W" % l[0]], params["trunk/%s/b" % l[0]], 1))
    assert rel_err(outs["f32s"][0], h_) <= 5e-6 and rel_err(outs["f32"][0], h_) <= 5e-6
    for a, b in zip(outs["f32"], outs["f32s"]):
        assert rel_err(b, a) <= 5e-6, rel_err(b, a)


def check_conv1_bf16(rt, Cin, Cout, H, W, seed=0):
    """First-layer bf16 kernel (fp32 NCHW image in, blocked bf16 out) == the generic bf16 kernel on the converted image: same operands
    (bf16-rounded image and weights), fp32 accumulation in a different order, one bf16 rounding of the result."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(1, Cin, H, W) * 60).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    xb, _ = to_bf16(x)
    wb, _ = to_bf16(w)
    want = O.relu(O.conv2d(xb, wb, b, 1))[0].transpose(1, 2, 0)
    got = from_bf16_bits(blocked_to_hwc(host(rt, rt.conv1_bf16(dev(rt, x), dev(rt, w), dev(rt, b), relu=True))))
    assert got.shape == (H, W, rt.bf16_pad(Cout)) and not got[:, :, Cout:].any()
    scale = np.abs(want).max()
    assert np.all(np.abs(got[:, :, :Cout] - want) <= np.abs(want) * 2.0 ** -8 + 2e-5 * scale)


def check_conv_bf16_pool(rt, Cin, Cout, H, W, seed=0):
    """out_mode 2: bf16 conv + ReLU + 2x2 ceil-mode pool in one launch == the two separate bf16 launches, bit for bit."""
    rs = np.random.RandomState(seed)
    x = rs.randn(1, Cin, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = dev(rt, (rs.randn(Cout) * 0.1).astype(np.float32))
    xd = rt.bf16_from_nchw(dev(rt, x))
    wpk = rt.bf16_pack_conv_w(dev(rt, w), 3)
    fused = host(rt, rt.conv_bf16(xd, wpk, b, Cin, Cout, 3, relu=True, pool=True))
    sep = host(rt, rt.maxpool2x2_bf16(rt.conv_bf16(xd, wpk, b, Cin, Cout, 3, relu=True)))
    assert fused.shape == sep.shape and np.array_equal(fused, sep)


def check_conv_bf16_default_pick(rt, Cin, Cout, H, W, expect, expect_pooled, seed=0):
    """The kernel the DEFAULT rule launches for this 3x3 layer size -- asserted through frcnn_conv_bf16_plan: `expect` for the bf16 / fp32 outputs,
    `expect_pooled` for the fused-pool output (910 = strip form D, 903 = strip form C, 0 = conv_dma_bf16_kernel) -- against the ORACLE fed the
    kernel's bf16 operands (fp32 accumulation): fp32 output within summation-order noise, bf16 output one rounding of it, fused ReLU + 2x2
    ceil-mode pool == the oracle's pool of the rounded map (the strip forms had met the oracle only outside their rule)."""
    assert tuning.get("FRCNN_BF16_DMA") is None and tuning.get("FRCNN_BF16_STRIP") is None
    L = rt.lib
    plans = [L.frcnn_conv_bf16_plan(Cin, Cout, H, W, 3, om) for om in (0, 1, 2)]
    assert plans == [expect, expect, expect_pooled], plans
    rs = np.random.RandomState(seed)
    x = rs.randn(1, Cin, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    xb, wb = to_bf16(x)[0], to_bf16(w)[0]
    want = O.relu(O.conv2d(xb, wb, b, 1))
    scale = max(np.abs(want).max(), 1e-6)
    xd, wpk, bd = rt.bf16_from_nchw(dev(rt, x)), rt.bf16_pack_conv_w(dev(rt, w), 3), dev(rt, b)
    y32 = host(rt, rt.conv_bf16(xd, wpk, bd, Cin, Cout, 3, relu=True, out_f32_nchw=True))
    e32 = np.abs(y32 - want).max() / scale
    assert e32 <= 2e-5, e32
    y16 = blocked_to_hwc(host(rt, rt.conv_bf16(xd, wpk, bd, Cin, Cout, 3, relu=True)))
    assert y16.shape == (H, W, rt.bf16_pad(Cout)) and not y16[:, :, Cout:].any()
    # the bf16 store is the RNE of the kernel's own fp32 value (same accumulation in both output modes), exactly
    assert np.array_equal(y16[:, :, :Cout], to_bf16(np.ascontiguousarray(y32[0].transpose(1, 2, 0)))[1])
    got = from_bf16_bits(y16)[:, :, :Cout]
    want_hwc = want[0].transpose(1, 2, 0)
    assert np.all(np.abs(got - want_hwc) <= np.abs(want_hwc) * 2.0 ** -8 + 2e-5 * scale)
    yp = blocked_to_hwc(host(rt, rt.conv_bf16(xd, wpk, bd, Cin, Cout, 3, relu=True, pool=True)))
    wantp = O.max_pool_2x2(want)[0].transpose(1, 2, 0)
    gotp = from_bf16_bits(yp)[:, :, :Cout]
    assert gotp.shape == wantp.shape and not yp[:, :, Cout:].any()
    assert np.all(np.abs(gotp - wantp) <= np.abs(wantp) * 2.0 ** -8 + 2e-5 * scale)
    if expect_pooled == expect or expect != 903:                 # one accumulation chain in both launches: the pooled words are the pool of the plain words, exactly
        assert np.array_equal(yp, blocked_to_hwc(host(rt, rt.maxpool2x2_bf16(rt.conv_bf16(xd, wpk, bd, Cin, Cout, 3, relu=True)))))
    print("PARITY conv_bf16 default pick %d/%d (%d->%d @ %dx%d) vs oracle: fp32 %.2e of scale, bf16 within one rounding" % (expect, expect_pooled, Cin, Cout, H, W, e32))


def check_conv1_pair_bf16(rt, H, W, Cin=3, seed=0, rw=None, form=None):
    """frcnn_conv1_pair_bf16 (conv1_1 + ReLU + conv1_2 + ReLU + 2x2 ceil-mode pool in one launch, csrc/conv_bf16_pair.hip): (1) bit for bit the
    two-launch chain frcnn_conv1_bf16 -> frcnn_conv_bf16(out_mode 2) on the same operands; (2) against the ORACLE: conv1_1 of the bf16-rounded
    image and weights (fp32 accumulation), rounded to bf16 once, conv1_2 of that with bf16-rounded weights, ReLU, ceil-mode pool, one rounding."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(1, Cin, H, W) * 50.0).astype(np.float32)               # image-like magnitudes (mean-subtracted pixels)
    w1 = (rs.randn(64, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9)) / 50.0).astype(np.float32)
    b1 = (rs.randn(64) * 0.1).astype(np.float32)
    w2 = (rs.randn(64, 64, 3, 3) * np.sqrt(2.0 / (64 * 9))).astype(np.float32)
    b2 = (rs.randn(64) * 0.1).astype(np.float32)
    xd, w1d, b1d, b2d = dev(rt, x), dev(rt, w1), dev(rt, b1), dev(rt, b2)
    w2p = rt.bf16_pack_conv_w(dev(rt, w2), 3)
    # form 1 (one wave per SIMD, weights in registers): rows per wave
    knobs = {"FRCNN_BF16_PAIR_RW": str(rw), "FRCNN_BF16_PAIR_FORM": "1"} if rw is not None else {"FRCNN_BF16_PAIR_FORM": str(form)} if form is not None else {}
    with tuning.override(**knobs):
        got = host(rt, rt.conv1_pair_bf16(xd, w1d, b1d, w2p, b2d))
    h1 = rt.conv1_bf16(xd, w1d, b1d, relu=True)
    two = host(rt, rt.conv_bf16(h1, w2p, b2d, 64, 64, 3, relu=True, pool=True))
    assert got.shape == two.shape == (4, (H + 1) // 2, (W + 1) // 2, 16)
    if _HALF[-1] == "f16":
        # the fp16 line's stand-alone conv1_1 is the generic kernel on the blocked image (no fp16 twin of the first-layer kernel): another fp32 summation
        # order, so a handful of fp16 roundings differ -- the pair launch is held to the oracle below, and to the chain within one rounding step
        a, b = from_bf16_bits(got), from_bf16_bits(two)
        assert np.all(np.abs(a - b) <= np.abs(b) * 2.0 ** -10 + 1e-4 * np.abs(b).max())
    else:
        assert np.array_equal(got, two), "%d of %d words differ from the two-launch chain" % (int((got != two).sum()), got.size)
    xb, w1b, w2b = to_bf16(x)[0], to_bf16(w1)[0], to_bf16(w2)[0]
    m1 = to_bf16(O.relu(O.conv2d(xb, w1b, b1, 1)))[0]
    dev1 = from_bf16_bits(blocked_to_hwc(host(rt, h1))).transpose(2, 0, 1)[None]
    s1 = max(np.abs(m1).max(), 1e-6)
    assert np.all(np.abs(dev1 - m1) <= np.abs(m1) * 2.0 ** -7 + 2e-5 * s1)                      # conv1_1: one rounding of fp32-order noise
    want = O.max_pool_2x2(O.relu(O.conv2d(dev1, w2b, b2, 1)))[0].transpose(1, 2, 0)               # conv1_2 of the DEVICE's conv1_1 map: fp32-order noise + one rounding
    s2 = max(np.abs(want).max(), 1e-6)
    g = from_bf16_bits(blocked_to_hwc(got))
    if _HALF[-1] == "f16":
        # `dev1` is the stand-alone chain's conv1_1 map, which in fp16 mode is NOT the map inside the pair launch (see above: a few of its values sit one fp16 step
        # away), and conv1_2 sums 576 of them: the bar is one output rounding plus 5e-4 of the map's scale
        assert np.all(np.abs(g - want) <= np.abs(want) * 2.0 ** -10 + 5e-4 * s2), float(np.abs(g - want).max() / s2)
    else:
        assert np.all(np.abs(g - want) <= np.abs(want) * 2.0 ** -8 + 2e-5 * s2)
    print("PARITY conv1 pair (%dx%d, Cin %d%s): == two-launch chain bit for bit; vs oracle within one rounding" % (H, W, Cin, "" if rw is None else ", RW %d" % rw))


def check_conv_bf16_strip(rt, form, Cin, Cout, H, W, pool=False, seed=0):
    """Strip form `form` (FRCNN_BF16_DMA=901 / 902 / 903 / 907 / 908 / 909, csrc/conv_bf16_strip.h) of the 3x3 bf16 convolution against
    conv_dma_bf16_kernel on the same operands: bit-identical for the forms that keep one accumulation chain per output (A, B, D = 909,
    908); within fp32 summation-order noise of it for the K-split forms (C = 903, 907: the bf16 outputs may then differ by one rounding
    step at a tie)."""
    rs = np.random.RandomState(seed)
    x = rs.randn(1, Cin, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = dev(rt, (rs.randn(Cout) * 0.1).astype(np.float32))
    xd = rt.bf16_from_nchw(dev(rt, x))
    wpk = rt.bf16_pack_conv_w(dev(rt, w), 3)

    def run():
        y32 = host(rt, rt.conv_bf16(xd, wpk, b, Cin, Cout, 3, relu=True, out_f32_nchw=True))
        y16 = host(rt, rt.conv_bf16(xd, wpk, b, Cin, Cout, 3, relu=True, pool=pool))
        return y32, y16
    with tuning.override(FRCNN_BF16_DMA=None, FRCNN_BF16_STRIP="0"):   # the reference: conv_dma_bf16_kernel's pick, not a strip form by the default rule
        ref32, ref16 = run()
        tuning.set("FRCNN_BF16_DMA", str(form))
        got32, got16 = run()
    assert got32.shape == ref32.shape and got16.shape == ref16.shape
    if form in (901, 902, 908, 909, 910, 911, 921, 922):
        assert np.array_equal(got32, ref32) and np.array_equal(got16, ref16)
    else:
        scale = max(np.abs(ref32).max(), 1e-6)
        assert np.abs(got32 - ref32).max() <= 2e-5 * scale, np.abs(got32 - ref32).max() / scale
        a, c = from_bf16_bits(got16), from_bf16_bits(ref16)
        assert np.all(np.abs(a - c) <= np.abs(c) * 2.0 ** -7 + 1e-5 * scale)
        assert np.mean(got16 != ref16) < 0.01                   # a rounding tie here and there, not a different result


def check_ksplit_words(tag, got16, ref16, got_pre, ref_pre, Cout, pooled=False, max_frac=1e-3):
    """bf16 outputs of a K-split kernel (`got16`, channel-blocked [C/16][h][w][16] bits) against a single-chain kernel's (`ref16`) on the same
    operands, given both kernels' fp32 PRE-activations (Cout, H, W; bias added, no ReLU).  Proven word by word:
      1. each kernel's bf16 word IS the round-to-nearest-even of its own fp32 value under ReLU (and the 2x2 ceil-mode max-pool) -- bit for bit,
      2. the two kernels' fp32 values differ by summation-order noise only (<= 2e-5 of the largest magnitude).
    Hence a differing bf16 word is a rounding tie the noise tipped, an output of small magnitude (cancellation: the absolute noise exceeds a bf16
    step there -- the word VERDICT r03 weak #1 asked for: 5.72e-4 vs 5.80e-4 from fp32 values 6e-6 apart) or a ReLU crossing; the report line
    counts them and quotes the worst offender of the old `|c| 2^-7 + 1e-6` bound with both fp32 values."""
    scale = float(max(np.abs(ref_pre).max(), 1e-6))
    noise = 2e-5 * scale
    dpre = float(np.abs(got_pre - ref_pre).max())
    assert dpre <= noise, (tag, dpre / scale)
    a16, c16 = blocked_to_hwc(got16)[:, :, :Cout], blocked_to_hwc(ref16)[:, :, :Cout]

    def relu_pool(p):                                            # (Cout, H, W) fp32 -> (h, w, Cout) fp32 under ReLU (+ the 2x2 ceil-mode pool)
        p = np.maximum(p, 0.0)
        if pooled:
            C, H, W = p.shape
            q = np.zeros((C, H + (H & 1), W + (W & 1)), np.float32)
            q[:, :H, :W] = p
            p = q.reshape(C, (H + 1) // 2, 2, (W + 1) // 2, 2).max(axis=(2, 4))
        return np.ascontiguousarray(p.transpose(1, 2, 0))
    pg, pr = relu_pool(got_pre), relu_pool(ref_pre)
    assert a16.shape == pg.shape, (a16.shape, pg.shape)
    assert np.array_equal(a16, to_bf16(pg)[1]), tag + ": K-split kernel's bf16 words are not the RNE of its own fp32 values"
    assert np.array_equal(c16, to_bf16(pr)[1]), tag + ": single-chain kernel's bf16 words are not the RNE of its own fp32 values"
    a, c = from_bf16_bits(a16), from_bf16_bits(c16)
    diff = a16 != c16
    nd = int(diff.sum())
    assert nd / a.size < max_frac, (tag, nd, a.size)
    crossing = diff & ((a == 0) != (c == 0))
    old_bound = np.abs(a - c) > np.abs(c) * 2.0 ** -7 + 1e-6
    msg = "PARITY %s: K-split vs single chain: %d of %d bf16 words differ (%d ReLU crossings), %d off the r03 bound, fp32 max diff %.2e (scale %.2f)" % (
        tag, nd, a.size, int(crossing.sum()), int(old_bound.sum()), dpre, scale)
    if old_bound.any():
        i = np.unravel_index(np.argmax(np.where(old_bound, np.abs(a - c), -1.0)), a.shape)
        msg += "; worst such word (y,x,c)=(%d,%d,%d) bf16 %.6g vs %.6g from fp32 %.9g vs %.9g" % (i[0], i[1], i[2], a[i], c[i], pg[i], pr[i])
    print(msg)
    assert np.all(np.abs(a - c) <= np.maximum(np.abs(a), np.abs(c)) * 2.0 ** -7 + noise), tag


def check_maxpool_bf16(rt, C, H, W, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(1, C, H, W).astype(np.float32)
    xb, _ = to_bf16(x)
    y = blocked_to_hwc(host(rt, rt.maxpool2x2_bf16(rt.bf16_from_nchw(dev(rt, x)))))
    want = O.max_pool_2x2(xb)[0].transpose(1, 2, 0)
    assert np.array_equal(from_bf16_bits(y)[:, :, :C], want)


def check_vgg_bf16_forward(rt, im_h, im_w, seed=5, dtype="bf16", feat_tol=3e-2, head_tol=2e-2):
    """Config 3 numerics: the bf16-conv pipeline vs the fp32 oracle; bf16 has 8 mantissa bits, so 14 stacked convolutions
    are compared at 3e-2 of the feature scale, and the downstream fp32 stages exactly given the device's own maps.
    dtype="f16": the fp16 instantiation of the same chain (11 mantissa bits: feat_tol / head_tol are passed 8x tighter)."""
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import FasterRCNN
    params = synthetic.params(seed=1)
    x = synthetic.image(seed=seed, h=im_h, w=im_w)
    info = np.array([[im_h, im_w]], dtype=np.int32)
    model = FasterRCNN(runtime=rt, conv_dtype=dtype, head_dtype=dtype)
    model.load_params(params)
    out = model.forward_device(rt.mem.from_numpy(x), im_h, im_w, keep=True)
    feat = host(rt, out["feat"])
    want = O.vgg16_trunk(params, x)
    err = np.abs(feat - want).max() / np.abs(want).max()
    assert err < feat_tol, err
    n = int(host(rt, out["n_out"])[0])
    p2, s2 = O.proposal_layer(host(rt, out["rpn_cls_prob"]), host(rt, out["rpn_bbox_pred"]), info, train=False)
    assert n == len(p2) and np.allclose(host(rt, out["rois"])[:n], p2, rtol=5e-7, atol=1e-4)
    rois = host(rt, out["rois"])[:n]
    pool5 = O.roi_pooling_2d(feat, np.concatenate([np.zeros((n, 1), np.float32), rois], 1), 7, 7, 1 / 16.)
    assert np.array_equal(host(rt, out["pool5"])[:n], pool5)
    cp, pb, _ = O.rcnn_head(params, pool5, rois, info)                       # bf16 head vs the fp32 oracle on the same pool5
    assert np.abs(host(rt, out["cls_prob"])[:n] - cp).max() < head_tol
    assert np.abs(host(rt, out["pred_boxes"])[:n] - pb).max() < head_tol * max(im_h, im_w)
    # the inference path proper (keep=False) pools straight from the channel-blocked bf16 map and never makes the fp32 NCHW copy:
    # same detections, bit for bit
    out2 = model.forward_device(rt.mem.from_numpy(x), im_h, im_w)
    for k in ("n_out", "rois", "cls_prob", "pred_boxes"):
        assert np.array_equal(host(rt, out2[k]), host(rt, out[k])), k
    return err


def check_vgg_bf16_trunk(rt, im_h, im_w, seed=5, upto="conv4_1"):
    """The full-width bf16 trunk through the model class at a small image, conv1_1 ... `upto` (the whole trunk costs the emulator
    minutes: every launch multiplies whole tiles however small the map): within 3e-2 of the fp32 oracle's feature scale, and -- the
    point of running it on the emulator, whose three-CU chip sends conv2_2 (pool-fused), conv3_1, conv3_2, conv3_3 (pool-fused) and
    conv4_1 through strip form D -- the same map bit for bit with the strip rule switched off (form D keeps conv_dma_bf16_kernel's
    accumulation order)."""
    import functools
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import FasterRCNN, VGG16Prev
    from chainer_faster_rcnn_amd.models.vgg16 import LAYERS
    layers = LAYERS[:[l[0] if l != "pool" else None for l in LAYERS].index(upto) + 1]
    params = synthetic.params(seed=1)
    x = synthetic.image(seed=seed, h=im_h, w=im_w)
    outs = {}
    model = FasterRCNN(trunk_class=functools.partial(VGG16Prev, layers=layers), runtime=rt, conv_dtype="bf16", head_dtype="bf16")
    model.trunk.load_params(params, "trunk/")
    for strip in ("1", "0"):                                        # (the library reads its tuning table at every launch)
        with tuning.override(FRCNN_BF16_STRIP=strip):
            outs[strip] = host(rt, model.trunk(rt.mem.from_numpy(x)))
    want = O.vgg16_trunk(params, x, upto=upto)
    err = np.abs(outs["1"] - want).max() / np.abs(want).max()
    assert outs["1"].shape == want.shape and err < 3e-2, err
    assert np.array_equal(outs["1"], outs["0"])
    return err


def check_detections(rt, R=300, ncls=21, seed=0):
    """forward.py:48-58 post-processing: 20 per-class NMS problems (thresh 0.3) + conf cut, batched on the device."""
    from chainer_faster_rcnn_amd.postprocess import detections
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 700, (R, 1, 2)) + rs.uniform(-20, 20, (R, ncls, 2))
    boxes = np.concatenate([xy, xy + rs.uniform(30, 300, (R, ncls, 2))], axis=2).reshape(R, 4 * ncls).astype(np.float32)
    prob = O.softmax((rs.randn(R, ncls) * 4).astype(np.float32), axis=1)
    got = detections(dev(rt, prob), dev(rt, boxes), 0.3, 0.5, im_scale=1.6, runtime=rt)
    total = 0
    for c in range(1, ncls):
        d = np.hstack((boxes[:, 4 * c:4 * c + 4], prob[:, c:c + 1])).astype(np.float32)       # forward.py:50-53
        d = d[O.cpu_nms(d, 0.3)]
        d = d[d[:, -1] >= 0.5].copy()
        d[:, :4] /= 1.6
        assert np.array_equal(got[c], d), c
        total += len(d)
    assert total > 0
    # special values through the same path (forward.py:48-58 on whatever the head produced): a NaN class score of either sign ranks first in cpu_nms
    # (cpu_nms.pyx:26), suppresses what it overlaps, and is then dropped by `>= conf`; +inf passes the cut, -inf does not; a NaN coordinate poisons the IoUs of its
    # row (cpu_nms.pyx:12-16's max / min are not symmetric in NaN); equal scores: ascending row index (the oracle's tie_rule)
    prob2, boxes2 = prob.copy(), boxes.copy()
    prob2[5, 1] = np.float32(np.nan)
    prob2[9, 2] = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    prob2[11, 3], prob2[12, 3] = np.float32(np.inf), np.float32(-np.inf)
    boxes2[20, 4 * 4] = np.float32(np.nan)
    boxes2[21, 4 * 5 + 3] = np.float32(np.nan)
    prob2[30:40, 6] = np.float32(0.75)                                     # ten rows tie
    boxes2[30:34, 4 * 6:4 * 6 + 4] = boxes2[30, 4 * 6:4 * 6 + 4]           # ... four of them on the same box
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = detections(dev(rt, prob2), dev(rt, boxes2), 0.3, 0.5, im_scale=1.6, runtime=rt)
        for c in range(1, ncls):
            d = np.hstack((boxes2[:, 4 * c:4 * c + 4], prob2[:, c:c + 1])).astype(np.float32)
            d = d[O.cpu_nms(d, 0.3, tie_rule="ascending_index")]
            d = d[d[:, -1] >= 0.5].copy()
            d[:, :4] /= 1.6
            assert got[c].shape == d.shape and np.array_equal(got[c].view(np.uint32), d.view(np.uint32)), (c, got[c][:3], d[:3])
            if c not in (6,):                                              # no ties in this class: NumPy's own order gives the same list
                e = np.hstack((boxes2[:, 4 * c:4 * c + 4], prob2[:, c:c + 1])).astype(np.float32)
                e = e[O.cpu_nms(e, 0.3)]
                e = e[e[:, -1] >= 0.5].copy()
                e[:, :4] /= 1.6
                assert np.array_equal(e.view(np.uint32), d.view(np.uint32)), c


def check_linear_bf16(rt, M, N, K, relu, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(M, K).astype(np.float32)
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float32)
    b = rs.randn(N).astype(np.float32) * 0.1
    xb, xbits = to_bf16(x)
    wb, wbits = to_bf16(w)
    assert np.array_equal(host(rt, rt.to_bf16(dev(rt, x))), xbits)
    want = O.linear(xb, wb, b)
    if relu:
        want = O.relu(want)
    y = host(rt, rt.linear_bf16(rt.to_bf16(dev(rt, x)), rt.to_bf16(dev(rt, w)), dev(rt, b), relu=relu))
    assert np.abs(y - want).max() <= 3e-5 * max(np.abs(want).max(), 1e-6), np.abs(y - want).max()
    y16 = from_bf16_bits(host(rt, rt.linear_bf16(rt.to_bf16(dev(rt, x)), rt.to_bf16(dev(rt, w)), dev(rt, b), relu=relu, out_bf16=True)))
    assert np.all(np.abs(y16 - want) <= np.abs(want) * 2.0 ** -8 + 3e-5 * np.abs(want).max())


def check_linear_bf16_tiled(rt, M, N, K, relu, seed=0):
    """frcnn_linear_bf16_tiled (csrc/linear_bf16.hip: the weight-stream kernel on pre-tiled weights) against the oracle fed the same bf16 operands, and
    against frcnn_linear_bf16 on the row-major weights (same products, fp32 accumulation; the split boundaries differ, so not bit for bit)."""
    rs = np.random.RandomState(seed)
    x = rs.randn(M, K).astype(np.float32)
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float32)
    b = rs.randn(N).astype(np.float32) * 0.1
    xb, _ = to_bf16(x)
    wb, wbits = to_bf16(w)
    want = O.linear(xb, wb, b)
    if relu:
        want = O.relu(want)
    wt = rt.linear_bf16_tile_w(rt.to_bf16(dev(rt, w)))
    # the tile layout itself: tile (nb, kc), 16-byte slot row * 4 + (g ^ ((row >> 2) & 3)) = w[nb * 128 + row][kc * 32 + 8 g ..]
    t = host(rt, wt).view(np.uint16).reshape(-1, K // 32, 128, 4, 8)
    nb, kc, row, g = (N - 1) // 128, (K // 32) - 1, (N - 1) % 128, 2
    assert np.array_equal(t[nb, kc, row, g ^ ((row >> 2) & 3)], wbits.view(np.uint16)[N - 1, kc * 32 + 8 * g: kc * 32 + 8 * g + 8])
    if N % 128:
        assert not t[nb, :, N % 128:].any()                                 # rows past N are zero
    y = host(rt, rt.linear_bf16_tiled(rt.to_bf16(dev(rt, x)), wt, N, dev(rt, b), relu=relu))
    assert y.shape == want.shape and np.abs(y - want).max() <= 3e-5 * max(np.abs(want).max(), 1e-6), np.abs(y - want).max()
    y0 = host(rt, rt.linear_bf16(rt.to_bf16(dev(rt, x)), rt.to_bf16(dev(rt, w)), dev(rt, b), relu=relu))
    assert np.abs(y - y0).max() <= 2e-5 * max(np.abs(want).max(), 1e-6)
    y16 = from_bf16_bits(host(rt, rt.linear_bf16_tiled(rt.to_bf16(dev(rt, x)), wt, N, dev(rt, b), relu=relu, out_bf16=True)))
    assert np.all(np.abs(y16 - want) <= np.abs(want) * 2.0 ** -8 + 3e-5 * np.abs(want).max())
    # the two accumulator orientations of the kernel (default where N % 4 == 0: MFMA operands swapped, 16-byte slab stores; FRCNN_LINEAR_RING_FLAGS bit 2:
    # round 6's first form, 4-byte stores): the same products summed by the same instruction -- bit for bit
    from chainer_faster_rcnn_amd import tuning
    with tuning.override(FRCNN_LINEAR_RING_FLAGS="4"):
        y4 = host(rt, rt.linear_bf16_tiled(rt.to_bf16(dev(rt, x)), wt, N, dev(rt, b), relu=relu))
    assert np.array_equal(y4, y)


def check_linear_f32s(rt, M, N, K, relu, seed=0):
    """fp32 L.Linear on split tensors: against a float64 product (next to the native fp32 kernel), the split output form, and the
    split / join conversions."""
    rs = np.random.RandomState(seed)
    x = rs.randn(M, K).astype(np.float32)
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float32)
    b = (rs.randn(N) * 0.1).astype(np.float32)
    xs, ws_ = rt.f32s_split(dev(rt, x)), rt.f32s_split(dev(rt, w))
    parts = from_bf16_bits(host(rt, xs))
    assert np.array_equal((parts[0] + parts[1]) + parts[2], x) and np.array_equal(host(rt, rt.f32s_join(xs)), x)
    want = x.astype(np.float64) @ w.astype(np.float64).T + b
    if relu:
        want = np.maximum(want, 0)
    y = host(rt, rt.linear_f32s(xs, ws_, dev(rt, b), relu=relu))
    scale = np.abs(want).max()
    err = np.abs(y - want).max() / scale
    yn = host(rt, rt.linear(dev(rt, x), dev(rt, w), dev(rt, b), relu=relu))
    err_n = np.abs(yn - want).max() / scale
    assert err <= 3e-6 and err <= 4 * err_n + 2e-7, (err, err_n)
    y3 = rt.linear_f32s(xs, ws_, dev(rt, b), relu=relu, out_split=True)
    assert np.array_equal(host(rt, rt.f32s_join(y3)), y)


def check_conv_relu_pool(rt, Cin, Cout, H, W, seed=0):
    """act = 4: conv + bias + ReLU + F.MaxPooling2D(2,2) (cover_all) in one launch, vs the three separate oracle steps."""
    rs = np.random.RandomState(seed)
    x = rs.randn(1, Cin, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = rs.randn(Cout).astype(np.float32) * 0.1
    want = O.max_pool_2x2(O.relu(O.conv2d(x, w, b, 1)))
    wp = rt.pack_conv3x3_w(dev(rt, w))
    got = host(rt, rt.conv_ex(dev(rt, x), wp, dev(rt, b), 3, act=4))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6)
    sep = host(rt, rt.maxpool2x2(rt.conv3x3(dev(rt, x), wp, dev(rt, b), relu=True, cfg=10)))
    assert np.array_equal(got, sep) or np.abs(got - sep).max() <= 1e-5 * np.abs(sep).max()


def check_preprocess(rt, h, w, seed=0):
    from chainer_faster_rcnn_amd.postprocess import PIXEL_MEANS, img_preprocessing
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    want, want_scale = O.img_preprocessing(img, PIXEL_MEANS)
    got, scale = img_preprocessing(img, runtime=rt)
    assert scale == want_scale and tuple(got.shape) == want.shape, (tuple(got.shape), want.shape)
    assert np.allclose(host(rt, got), want, rtol=0, atol=2e-4)          # float32 blends of values up to 255: a few ulps


def check_conv_workspace_self_cleaning(rt):
    """The stream-K / split-K tile counters live in the first 64 KB of the conv workspaces, are zeroed ONCE
    (frcnn_conv3x3_workspace_init / frcnn_conv_bf16_workspace_init) and must be back to zero after every launch
    (the last arriver of a split tile resets its counter) -- the invariant that lets launches skip the memset."""
    import os
    check_conv3x3(rt, 24, 128, 9, 70, cfg=236)                  # stream-K, LDS-DMA decomposition
    check_conv3x3(rt, 24, 128, 9, 70, cfg=210, seed=1)          # stream-K, register-staged decomposition
    page = host(rt, rt._ws["conv3x3"])[:65536]
    assert not page.any()
    with tuning.override(FRCNN_BF16_SPLIT="2"):
        check_conv_bf16(rt, 128, 64, 9, 37, seed=5)
    page = host(rt, rt._ws["conv_bf16"])[:65536]
    assert not page.any()


def check_empty_proposals_pipeline(rt):
    """Nothing survives the min-size filter (ProposalLayer with a huge min_size): zero proposals out, padding rows zeroed, and the
    downstream stages accept the all-padding RoI block (degenerate RoIs at the origin) without faulting -- the reference would
    hand F.roi_pooling_2d an empty array here; the fixed-capacity device path hands it zero rows that n_out tells the caller to drop."""
    G = g("proposal_14x14_train_rand")
    anchors = O.generate_anchors()
    im_h, im_w = [int(v) for v in G["img_info"][0]]
    rois, probs, n_out, src = rt.proposals(dev(rt, G["rpn_cls_prob"][0]), dev(rt, G["rpn_bbox_pred"][0]), anchors, 16,
                                           im_h, im_w, 1.0e6, 200, 50, 0.7, want_index=True)
    assert int(host(rt, n_out)[0]) == 0
    assert not host(rt, rois).any() and not host(rt, probs).any() and (host(rt, src) == -1).all()
    C, H, W = 16, 14, 14
    x = np.abs(np.random.RandomState(0).randn(1, C, H, W)).astype(np.float32)
    y = host(rt, rt.roi_pool_fwd_chw(dev(rt, x[0]), rois, 7, 7, 0.0625))
    want, _ = O.roi_pooling_2d(x, np.zeros((rois.shape[0], 5), np.float32), 7, 7, 0.0625, return_argmax=True)
    assert np.array_equal(y, want)                        # a (0,0,0,0) RoI is the 1x1 window at the origin in every bin it covers

