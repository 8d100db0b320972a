"""Adam / AdaGrad / RMSprop update rules (csrc/optimizer.hip, RPNTrainer / RCNNTrainer(opt=...)): case bodies shared by the CPU suite
(host-emulated kernels) and the GPU suite.

THE WITNESS is `Witness` below: Chainer v1's update rules restated in NumPy, one np.float32 operation per statement (so every operation
is rounded separately, in the order the kernel header parenthesises them), Adam's lr_t in Python double from two RUNNING PRODUCTS
(p = p * beta once per applied step, starting from 1.0: the rule csrc/optimizer.hip states).  Every comparison with it is BIT EQUALITY
of w and of every state buffer -- no tolerance.  One accommodation, because IEEE 754 leaves it open: where the witness holds a NaN (an
Inf - Inf after |g| = 1e30 twice) the device must hold a NaN too, but the NaN's sign and payload bits are not compared."""
import math
import os

import numpy as np

import parity_cases as P
import train_cases as T

RULES = ("Adam", "AdaGrad", "RMSprop")
# Chainer's defaults (optimizers.Adam / AdaGrad / RMSprop)
DEFAULTS = {"Adam": dict(alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8), "AdaGrad": dict(lr=1e-3, eps=1e-8), "RMSprop": dict(lr=1e-2, alpha=0.99, eps=1e-8)}
STATE_KEYS = {"Adam": ("m", "v"), "AdaGrad": ("h",), "RMSprop": ("ms",)}
RULE_IDS = {"Adam": 1, "AdaGrad": 2, "RMSprop": 3}
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)
ALIGNMENTS = ("aligned", "w_off", "all_off")
F = np.float32


def adam_lr_t(alpha, p1, p2):
    """lr_t from the two running products, in double, rounded to fp32 once."""
    return F(float(alpha) * math.sqrt(1.0 - p2) / (1.0 - p1))


class Witness(object):
    """One parameter buffer under one rule.  step(g) applies an update to self.w and the state arrays (self.state[name]) in place."""

    def __init__(self, rule, w, wd=0.0, **hyper):
        unknown = set(hyper) - set(DEFAULTS[rule])
        assert not unknown, unknown
        self.rule, self.hp, self.wd = rule, dict(DEFAULTS[rule], **hyper), wd
        self.w = np.array(w, dtype=F).reshape(-1).copy()
        self.state = {k: np.zeros_like(self.w) for k in STATE_KEYS[rule]}
        self.t, self.p1, self.p2 = 0, 1.0, 1.0

    def step(self, g, inv_scale=1.0):
        hp, w = self.hp, self.w
        g = np.asarray(g, dtype=F).reshape(-1)
        with np.errstate(all="ignore"):
            ge = g * F(inv_scale)
            dec = F(self.wd) * w
            ge = ge + dec
            eps = F(hp["eps"])
            if self.rule == "Adam":
                self.t += 1
                self.p1 = self.p1 * float(hp["beta1"])
                self.p2 = self.p2 * float(hp["beta2"])
                lr_t = adam_lr_t(hp["alpha"], self.p1, self.p2)
                omb1 = F(1.0 - float(hp["beta1"]))
                omb2 = F(1.0 - float(hp["beta2"]))
                m, v = self.state["m"], self.state["v"]
                a = ge - m
                a = omb1 * a
                m = m + a
                b = ge * ge
                b = b - v
                b = omb2 * b
                v = v + b
                num = lr_t * m
                den = np.sqrt(v)
                den = den + eps
                q = num / den
                w = w - q
                self.state["m"], self.state["v"] = m, v
            elif self.rule == "AdaGrad":
                self.t += 1
                h = self.state["h"]
                b = ge * ge
                h = h + b
                num = F(hp["lr"]) * ge
                den = np.sqrt(h)
                den = den + eps
                q = num / den
                w = w - q
                self.state["h"] = h
            else:
                self.t += 1
                ms = self.state["ms"]
                alpha = F(hp["alpha"])
                oma = F(1.0 - float(hp["alpha"]))
                a = alpha * ms
                b = oma * ge
                b = b * ge
                ms = a + b
                num = F(hp["lr"]) * ge
                den = np.sqrt(ms)
                den = den + eps
                q = num / den
                w = w - q
                self.state["ms"] = ms
        assert w.dtype == F and all(s.dtype == F for s in self.state.values())
        self.w = w
        return w


def assert_same_bits(got, want, what=""):
    got = np.ascontiguousarray(got, dtype=F).reshape(-1)
    want = np.ascontiguousarray(want, dtype=F).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions differ", int(gn.sum()), int(wn.sum()))
    gb, wb = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    if not np.array_equal(gb, wb):
        bad = np.flatnonzero(gb != wb)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d values differ in their bits; first at %d: got %r (%08x) want %r (%08x)" % (
            what, bad.size, gb.size, i, got[~gn][i], gb[i], want[~wn][i], wb[i]))


# ------------------------------------------------------------------------------------------- device side helpers
def cu_count(rt):
    """Compute units the library's launch heuristics see: the emulated chip's (tests/hipemu: HIPEMU_CUS, default 3) or the GPU's."""
    if rt.lib.frcnn_device_count() == 0:
        return int(os.environ.get("HIPEMU_CUS", "0")) or 3
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


TILE_UNITS = 256 * 4        # a workgroup's tile: 256 threads x four units in flight (a unit = a 16-byte vector or, on the unaligned path, one float)


def full_trip(rt, vector=True):
    """Elements one trip of the update launch covers at its grid cap (include/frcnn_hip.h: min(ceil(units / 1024), 8 x CUs) workgroups,
    each taking a contiguous tile of 1024 units per trip)."""
    return 8 * cu_count(rt) * TILE_UNITS * (4 if vector else 1)


def placed(rt, a, off):
    """A device copy of `a` that starts `off` floats behind a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=F).reshape(-1)
    buf = rt.mem.zeros((a.size + 8,), "f32")
    skip = ((-rt.mem.ptr(buf).value) % 16) // 4 + off
    view = buf[skip:skip + a.size]
    view[...] = rt.mem.from_numpy(a)
    assert rt.mem.ptr(view).value % 16 == 4 * off
    return view


def scaler_state(rt, scale):
    buf = rt.mem.zeros((8,), "i32")
    rt.loss_scaler_init(buf, scale)
    return buf


def opt_state(rt):
    buf = rt.mem.zeros((8,), "i32")
    rt.opt_state_init(buf)
    return buf


def opt_words(rt, buf):
    w = np.ascontiguousarray(P.host(rt, buf)).astype(np.int32)
    return dict(t=int(w[0]), lr_t=w.view(F)[1], p1=float(w.view(np.float64)[1]), p2=float(w.view(np.float64)[2]))


def values(rs, n, step=0):
    """Seeded normals x 1e-3 with the edge values planted where the buffer is long enough: exact zeros in w and g, -0.0, subnormals,
    |g| = 1e30 (g * g overflows to +Inf: the state saturates and, for Adam, a second such gradient makes Inf - Inf)."""
    w = (rs.randn(n) * 1e-3).astype(F)
    g = (rs.randn(n) * 1e-3).astype(F)
    if n >= 63:
        w[5], g[5] = 0.0, 0.0
        w[6], g[6] = -0.0, 0.0
        g[7] = -0.0
        g[8] = 1e-40                      # subnormal gradient
        w[9] = -3e-41                     # subnormal weight
        w[10], g[10] = 1e-42, -1e-44
        g[11] = 1e30
        g[12] = -1e30 if step != 1 else 1e-3
        g[n - 1] = 1e30 if step == 0 else 0.0
        w[n - 2], g[n - 2] = 0.0, 0.0
    return w, g


def device_hyper(rule, hp):
    if rule == "Adam":
        return dict(lr=hp["alpha"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"])
    if rule == "AdaGrad":
        return dict(lr=hp["lr"], eps=hp["eps"])
    return dict(lr=hp["lr"], beta1=hp["alpha"], eps=hp["eps"])


class DeviceRun(object):
    """The same buffer under frcnn_opt_step."""

    def __init__(self, rt, rule, w, wd=0.0, align="aligned", scale=None, **hyper):
        self.rt, self.rule, self.wd = rt, rule, wd
        self.hp = dict(DEFAULTS[rule], **hyper)
        self.offs = {"aligned": (0, 0), "w_off": (1, 0), "all_off": (1, 1)}[align]
        n = np.asarray(w).size
        self.w = placed(rt, w, self.offs[0])
        self.state = {k: placed(rt, np.zeros(n, F), self.offs[1]) for k in STATE_KEYS[rule]}
        self.opt = opt_state(rt) if rule == "Adam" else None
        self.scaler = scaler_state(rt, scale) if scale is not None else None

    def step(self, g):
        st = [self.state[k] for k in STATE_KEYS[self.rule]]
        self.rt.opt_step(self.rule, self.w, placed(self.rt, g, self.offs[1]), st[0], st[1] if len(st) > 1 else None, weight_decay=self.wd,
                         opt_state=self.opt, scaler_state=self.scaler, **device_hyper(self.rule, self.hp))

    def compare(self, wit, what):
        assert_same_bits(P.host(self.rt, self.w), wit.w, what + " w")
        for k in STATE_KEYS[self.rule]:
            assert_same_bits(P.host(self.rt, self.state[k]), wit.state[k], what + " " + k)
        if self.opt is not None:
            ow = opt_words(self.rt, self.opt)
            assert ow["t"] == wit.t and ow["p1"] == wit.p1 and ow["p2"] == wit.p2, (what, ow, wit.t, wit.p1, wit.p2)
            if wit.t:
                assert ow["lr_t"].view(np.uint32) == adam_lr_t(wit.hp["alpha"], wit.p1, wit.p2).view(np.uint32), (what, ow)


# ------------------------------------------------------------------------------------------- kernel cases
def check_three_steps(rt, rule, n, align="aligned", scale=None, wd=0.0, seed=0, steps=3):
    """Three consecutive steps (the state carries) against the witness, bit for bit after every step.  scale: run through a loss scaler's
    state with the gradient pre-multiplied by S (exact: S is a power of two and nothing overflows)."""
    rs = np.random.RandomState(seed + 7 * n)
    w0, _ = values(rs, n)
    wit = Witness(rule, w0, wd=wd)
    dev = DeviceRun(rt, rule, w0, wd=wd, align=align, scale=scale)
    for it in range(steps):
        _, g = values(rs, n, step=it)
        if scale is None:
            dev.step(g)
            wit.step(g)
        else:
            gs = g * F(scale)
            assert np.all(np.isfinite(gs))
            dev.step(gs)
            wit.step(gs, inv_scale=1.0 / scale)
        dev.compare(wit, "%s n=%d %s scale=%s wd=%g step %d" % (rule, n, align, scale, wd, it))


def check_sizes_and_alignments(rt, rule, scaled, wd):
    for n in SIZES:
        for align in ALIGNMENTS:
            check_three_steps(rt, rule, n, align=align, scale=2.0 ** 9 if scaled else None, wd=wd, seed=len(align))


def check_second_trip(rt, rule):
    """Just above one full trip of the launch the entry point makes, plus 5: the second trip of the grid-stride loop and the scalar tail
    both run -- on the 16-byte path and on the element path."""
    # one whole tile and a partial one (300 units) for the first workgroups' second trip, then 3 elements behind the last whole vector
    check_three_steps(rt, rule, full_trip(rt, True) + 4 * (TILE_UNITS + 300) + 3, align="aligned", scale=2.0 ** 9, wd=0.0005, seed=1)
    check_three_steps(rt, rule, full_trip(rt, False) + TILE_UNITS + 300, align="w_off", scale=None, wd=0.0005, seed=2)


def check_zero_gradient_keeps_w(rt, rule):
    """g = 0 on a fresh state and wd = 0: 0 / (0 + eps) is 0 and w - 0 keeps w's bits -- zeros of both signs, subnormals, normals."""
    w = np.array([0.0, -0.0, 1e-40, -1e-44, 1.5, -2.5e-3, 3e38, 1e-38] * 9, dtype=F)
    for align in ALIGNMENTS:
        dev = DeviceRun(rt, rule, w, align=align)
        dev.step(np.zeros_like(w))
        got = P.host(rt, dev.w)
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), (rule, align)
        for k in STATE_KEYS[rule]:
            assert not P.host(rt, dev.state[k]).view(np.uint32).any(), (rule, align, k)


def check_overflowing_square(rt, rule):
    """|g| = 1e30: g * g is +Inf, the second-moment state saturates at +Inf and the step's quotient is 0 (w keeps its bits); what the next
    steps do is whatever the restatement says (Adam: Inf - Inf = NaN on a second overflowing gradient) -- and the device says the same."""
    w0 = np.array([0.25, -0.5, 1e-3, 2.0] * 16 + [1.0], dtype=F)
    g = np.array([1e30, -1e30, 1e-3, 0.0] * 16 + [1e30], dtype=F)
    wit, dev = Witness(rule, w0), DeviceRun(rt, rule, w0)
    dev.step(g)
    wit.step(g)
    second = STATE_KEYS[rule][-1]
    assert np.isposinf(wit.state[second][0]) and wit.w[0] == w0[0] and wit.w[1] == w0[1]
    dev.compare(wit, rule + " overflow step 0")
    for it, gi in enumerate((g, np.zeros_like(g))):
        dev.step(gi)
        wit.step(gi)
        dev.compare(wit, rule + " overflow step %d" % (it + 1))
    if rule == "Adam":
        assert np.isnan(wit.w[0]) and np.isfinite(wit.w[2])


def check_skip(rt, rule, n=257):
    """The scaler's flag set by the finite check on a gradient with a NaN and an Inf: every buffer and t keep their bits; after the
    scaler's update cleared the flag the next clean step is step t = 1."""
    rs = np.random.RandomState(n)
    w0, g = values(rs, n)
    S = 2.0 ** 9
    wit = Witness(rule, w0, wd=0.0005)
    dev = DeviceRun(rt, rule, w0, wd=0.0005, scale=S)
    dev.state = {k: placed(rt, np.abs(rs.randn(n)).astype(F) * 1e-3, 0) for k in STATE_KEYS[rule]}       # a state worth keeping
    for k in STATE_KEYS[rule]:
        wit.state[k] = P.host(rt, dev.state[k]).copy()
    before = {k: P.host(rt, dev.state[k]).copy() for k in STATE_KEYS[rule]}
    bad = (g * F(S)).astype(F)
    bad[3], bad[n - 1] = np.nan, np.inf
    rt.grad_check_finite(P.dev(rt, bad), dev.scaler)
    assert int(P.host(rt, dev.scaler)[3]) == 1
    ow0 = opt_words(rt, dev.opt) if dev.opt is not None else None
    dev.step(bad)
    assert np.array_equal(P.host(rt, dev.w).view(np.uint32), w0.view(np.uint32)), rule
    for k in STATE_KEYS[rule]:
        assert np.array_equal(P.host(rt, dev.state[k]).view(np.uint32), before[k].view(np.uint32)), (rule, k)
    if dev.opt is not None:
        ow = opt_words(rt, dev.opt)
        assert ow["t"] == 0 and ow["p1"] == 1.0 and ow["p2"] == 1.0 and ow["lr_t"].view(np.uint32) == ow0["lr_t"].view(np.uint32), ow
    rt.loss_scaler_update(dev.scaler, 2.0, 0.5, 2000, 1.0, 2.0 ** 24)          # S -> 2^8, the flag cleared
    words = np.ascontiguousarray(P.host(rt, dev.scaler)).astype(np.int32)
    assert int(words[3]) == 0 and int(words[4]) == 1 and float(words.view(F)[0]) == S / 2
    _, g1 = values(rs, n, step=1)
    gs = g1 * F(S / 2)
    dev.step(gs)
    wit.step(gs, inv_scale=2.0 / S)
    assert wit.t == 1
    dev.compare(wit, rule + " first clean step after a skip")


def check_scaled_equals_unscaled(rt, rule, n=1025):
    """A clean step through the scaler's state on S * G is bit-identical to the unscaled entry on (S * G) / S, S = 2^9 and 2^16."""
    for S in (2.0 ** 9, 2.0 ** 16):
        rs = np.random.RandomState(int(math.log2(S)))
        w0, g = values(rs, n)
        gs = (g * F(S)).astype(F)
        assert np.all(np.isfinite(gs))
        a, b = DeviceRun(rt, rule, w0, wd=0.0005, scale=S), DeviceRun(rt, rule, w0, wd=0.0005)
        for it in range(2):
            a.step(gs)
            b.step((gs / F(S)).astype(F))
            assert_same_bits(P.host(rt, a.w), P.host(rt, b.w), "%s scale %g step %d w" % (rule, S, it))
            for k in STATE_KEYS[rule]:
                assert_same_bits(P.host(rt, a.state[k]), P.host(rt, b.state[k]), "%s scale %g step %d %s" % (rule, S, it, k))


def check_refusals(rt):
    """Every FRCNN_ERR_INVALID condition of the header, and n == 0."""
    L, m = rt.lib, rt.mem
    n = 64
    bufs = [m.zeros((n,), "f32") for _ in range(4)]
    w, g, s1, s2 = (m.ptr(b) for b in bufs)
    os_ = opt_state(rt)
    o = m.ptr(os_)

    def call(rule, w=w, g=g, s1=s1, s2=s2, n=n, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, o=o, sc=None):
        return L.frcnn_opt_step(rule, w, g, s1, s2, n, lr, b1, b2, eps, wd, o, sc, m.stream())
    OK, INVALID = 0, -1
    for rule in (1, 2, 3):
        assert call(rule) == OK
        assert call(rule, n=0) == OK
        assert call(rule, eps=0.0) == INVALID and call(rule, eps=-1e-8) == INVALID and call(rule, eps=float("nan")) == INVALID
        assert call(rule, w=None) == INVALID and call(rule, g=None) == INVALID and call(rule, s1=None) == INVALID
    for rule in (0, 4, -1, 99):
        assert call(rule) == INVALID                                             # unknown rule
    assert call(1, s2=None) == INVALID and call(1, o=None) == INVALID            # Adam needs both state buffers and the device state
    assert call(2, s2=None, o=None) == OK and call(3, s2=None, o=None) == OK     # the others need neither
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert call(1, b1=bad) == INVALID and call(1, b2=bad) == INVALID         # Adam's betas outside [0, 1)
        assert call(3, b1=bad) == INVALID                                        # RMSprop's alpha outside [0, 1)
    assert call(1, b1=0.0, b2=0.0) == OK and call(3, b1=0.0) == OK
    assert call(2, b1=7.0, b2=-3.0) == OK                                        # AdaGrad ignores them
    assert L.frcnn_opt_state_init(None, 0, 1.0, 1.0, m.stream()) == INVALID
    assert L.frcnn_opt_state_init(o, -1, 1.0, 1.0, m.stream()) == INVALID
    assert L.frcnn_opt_state_init(o, 0, 1.5, 1.0, m.stream()) == INVALID
    # a refused or empty call launched nothing: t counts the accepted calls with n > 0 that were handed the state
    m.synchronize()
    with_state = 3 + 2                                                           # call(rule) for three rules; Adam / RMSprop with beta 0
    assert opt_words(rt, os_)["t"] == with_state + 1, opt_words(rt, os_)          # (+ AdaGrad with ignored betas)
    with np.testing.assert_raises(ValueError):
        rt.opt_step("Adam", bufs[0], bufs[1], bufs[2], bufs[3], lr=1e-3, beta1=0.9, beta2=0.999, eps=0.0, opt_state=os_)
    with np.testing.assert_raises(ValueError):
        rt.opt_step("SGD", bufs[0], bufs[1], bufs[2])


def check_lr_t_rule_against_chainer():
    """CPU only: the running-product rule stays within one fp32 ulp of Chainer's `alpha * math.sqrt(1 - beta2**t) / (1 - beta1**t)` for
    t = 1 .. 3000 at the default betas."""
    hp = DEFAULTS["Adam"]
    p1 = p2 = 1.0
    worst = 0
    for t in range(1, 3001):
        p1 = p1 * hp["beta1"]
        p2 = p2 * hp["beta2"]
        mine = adam_lr_t(hp["alpha"], p1, p2)
        chainer = F(hp["alpha"] * math.sqrt(1.0 - hp["beta2"] ** t) / (1.0 - hp["beta1"] ** t))
        d = abs(int(mine.view(np.int32)) - int(chainer.view(np.int32)))
        worst = max(worst, d)
        assert d <= 1, (t, mine, chainer)
    return worst


# ------------------------------------------------------------------------------------------- trainer cases
def rpn_inputs(seed=0, im_h=40, im_w=56):
    rs = np.random.RandomState(seed)
    x = rs.randn(1, 3, im_h, im_w).astype(F)
    gt = P.gt_case(rs, 3, im_h, im_w)
    gt[0, :, 2] = np.minimum(gt[0, :, 0] + rs.uniform(8, 30, 3), im_w - 1)
    gt[0, :, 3] = np.minimum(gt[0, :, 1] + rs.uniform(8, 30, 3), im_h - 1)
    return x, gt, np.array([[im_h, im_w]], dtype=np.int32)


def make_trainer(rt, kind, params=None, **kw):
    """kind "rpn": RPNTrainer on train_cases' narrow model; "rcnn": RCNNTrainer on rcnn16_train_cases' (the same trunk plus a small head)."""
    from chainer_faster_rcnn_amd.train import RCNNTrainer, RPNTrainer
    import rcnn16_train_cases as R
    if kind == "rpn":
        return RPNTrainer(T.build_small(rt, params if params is not None else T.small_params()), **kw)
    if params is None:
        params = R.small_case(rt)[0]
    if "conv_math" in kw:                                             # one spelling for both trainers' fp16 step
        kw["precision"] = kw.pop("conv_math")
    return RCNNTrainer(R.build_small(rt, params), dropout_rng="device", **kw)       # masks drawn in the dropout kernel: one pass per step


def trainer_inputs(rt, kind):
    import rcnn16_train_cases as R
    return rpn_inputs() if kind == "rpn" else R.small_case(rt)[1:]


def forward_backward(tr, kind, inputs, seed):
    """One forward / backward pass that fills tr.G (the host's draws -- anchor / RoI sampling -- seeded)."""
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    x, gt, info = inputs
    np.random.seed(seed)
    tr.forward_backward(Variable(x), Variable(info), Variable(gt))
    tr.all_reduce()


def trainer_hyper(tr):
    return {k: getattr(tr, k) for k in DEFAULTS[tr.opt]}


def compare_trainer(rt, tr, wit, what):
    assert_same_bits(P.host(rt, tr.W), wit.w, what + " W")
    assert sorted(tr.moments) == sorted(STATE_KEYS[tr.opt])
    for k in STATE_KEYS[tr.opt]:
        assert_same_bits(P.host(rt, tr.moments[k]), wit.state[k], what + " " + k)
    if tr.opt == "Adam":
        st = tr.opt_state.state()
        assert (st["t"], st["beta1_pow_t"], st["beta2_pow_t"]) == (wit.t, wit.p1, wit.p2), (what, st)


def check_trainer_rule(rt, kind, rule, steps=3, **kw):
    """Each step: copy G to the host after forward_backward, apply the restatement, and after update() the trainer's W and state arenas
    equal it bit for bit (the optimizer alone: the gradients are the device's own)."""
    tr = make_trainer(rt, kind, opt=rule, **kw)
    assert tr.opt == rule and tr.weight_decay == 0.0 and tr.V is None
    inputs = trainer_inputs(rt, kind)
    wit = Witness(rule, P.host(rt, tr.W), wd=tr.weight_decay, **trainer_hyper(tr))
    for it in range(steps):
        forward_backward(tr, kind, inputs, 11 + it)
        g = P.host(rt, tr.G).copy()
        assert np.abs(g).max() > 0
        tr.update()
        wit.step(g)
        compare_trainer(rt, tr, wit, "%s %s step %d" % (kind, rule, it))
    assert tr.iteration == steps
    if kind == "rpn":                                                # the links see the update: windows of the arena
        name, link = tr.convs[1]
        seg = tr.seg[name + "/W"]
        assert np.array_equal(P.host(rt, link.Wp).reshape(-1), wit.w[seg.offset:seg.offset + seg.size])
    return tr


def check_trainer_schedule_and_weight_decay(rt):
    """Hyper-parameters are attributes read at every update() (trainer.alpha *= gamma), and an explicit weight_decay is honoured."""
    tr = make_trainer(rt, "rpn", opt="Adam", opt_args=dict(alpha=2e-3, beta1=0.8), weight_decay=0.001)
    assert (tr.alpha, tr.beta1, tr.beta2, tr.eps, tr.weight_decay) == (2e-3, 0.8, 0.999, 1e-8, 0.001)
    inputs = trainer_inputs(rt, "rpn")
    wit = Witness("Adam", P.host(rt, tr.W), wd=0.001, alpha=2e-3, beta1=0.8)
    for it in range(2):
        forward_backward(tr, "rpn", inputs, 3 + it)
        g = P.host(rt, tr.G).copy()
        tr.update()
        wit.step(g)
        compare_trainer(rt, tr, wit, "schedule step %d" % it)
        tr.alpha *= 0.5
        wit.hp["alpha"] = tr.alpha


def check_trainer_f16_skip(rt, kind):
    """fp16 step with Adam: an Inf written into G between forward_backward() and update() (as f16_train_cases.check_overflow_handling):
    W, m, v and the device's t keep their bits, skipped_steps == 1; the following clean step is the restatement's step t = 1."""
    tr = make_trainer(rt, kind, opt="Adam", conv_math="f16", loss_scale=dict(init_scale=2.0 ** 10))
    inputs = trainer_inputs(rt, kind)
    forward_backward(tr, kind, inputs, 21)
    w0 = P.host(rt, tr.W).copy()
    g = P.host(rt, tr.G).copy()
    g[tr.seg[tr.convs[1][0] + "/W"].offset + 7] = np.inf
    tr.G[...] = P.dev(rt, g)
    tr.update()
    st, os_ = tr.loss_scaler.state(), tr.opt_state.state()
    assert np.array_equal(P.host(rt, tr.W).view(np.uint32), w0.view(np.uint32))
    for k in ("m", "v"):
        assert not P.host(rt, tr.moments[k]).view(np.uint32).any(), k
    assert (os_["t"], os_["beta1_pow_t"], os_["beta2_pow_t"]) == (0, 1.0, 1.0), os_
    assert (st["scale"], st["skipped_steps"], st["found_nonfinite"]) == (2.0 ** 9, 1, 0) and tr.iteration == 1, st
    wit = Witness("Adam", w0, wd=tr.weight_decay)
    forward_backward(tr, kind, inputs, 22)
    g = P.host(rt, tr.G).copy()
    assert np.all(np.isfinite(g))
    tr.update()
    wit.step(g, inv_scale=1.0 / 2.0 ** 9)
    assert wit.t == 1
    compare_trainer(rt, tr, wit, kind + " f16 Adam after a skipped step")
    assert tr.loss_scaler.state()["skipped_steps"] == 1 and not np.array_equal(P.host(rt, tr.W), w0)


def check_snapshot_resume(rt, kind, tmp_path, n=3, k=2, **kw):
    """k steps, save, load into a fresh trainer (other parameters), one more step == the uninterrupted run, bit for bit.  With the fp16
    step the first step is skipped (a NaN in G), so the saved t is the DEVICE's count of applied steps, not the iteration."""
    from chainer_faster_rcnn_amd.serializers import load_trainer_npz, save_trainer_npz
    import rcnn16_train_cases as R
    f16 = kw.get("conv_math") == "f16"
    inputs = trainer_inputs(rt, kind)
    base = None if kind == "rpn" else R.small_case(rt)[0]
    other = T.small_params(seed=2) if kind == "rpn" else dict(R.small_case(rt, seed=5)[0], **T.small_params(seed=2))

    def run(tr, first, last):
        for it in range(first, last):
            forward_backward(tr, kind, inputs, 40 + it)
            if f16 and it == 0:
                g = P.host(rt, tr.G).copy()
                g[3] = np.nan
                tr.G[...] = P.dev(rt, g)
            tr.update()
    a = make_trainer(rt, kind, params=base, opt="Adam", **kw)
    run(a, 0, n)
    b = make_trainer(rt, kind, params=base, opt="Adam", **kw)
    run(b, 0, k)
    path = str(tmp_path / ("adam_snapshot_" + kind))
    save_trainer_npz(path, b)
    with np.load(path) as f:
        keys = set(f.files)
        t_saved = int(f["updater/optimizer:main/t"])
    first = "trunk/" + b.convs[0][0]
    assert {"updater/optimizer:main/%s/W/m" % first, "updater/optimizer:main/%s/b/v" % first} <= keys
    assert t_saved == b.opt_state.state()["t"] == (k - 1 if f16 else k)
    c = load_trainer_npz(path, make_trainer(rt, kind, params=other, opt="Adam", **kw))
    assert c.opt_state.state() == dict(b.opt_state.state(), lr_t=0.0) and c.iteration == k
    run(c, k, n)
    assert np.array_equal(P.host(rt, a.W).view(np.uint32), P.host(rt, c.W).view(np.uint32))
    for q in ("m", "v"):
        assert np.array_equal(P.host(rt, a.moments[q]).view(np.uint32), P.host(rt, c.moments[q]).view(np.uint32)), q
    sa, sc = a.opt_state.state(), c.opt_state.state()
    assert sa == sc and sa["t"] == (n - 1 if f16 else n), (sa, sc)
    # a Chainer-written file holds t only: the running products are rebuilt from it by t multiplications, the same bits
    with np.load(path) as f:
        d = {q: f[q] for q in f.files if not q.endswith("_pow_t")}
    p2 = str(tmp_path / ("adam_snapshot_t_only_" + kind))
    with open(p2, "wb") as fh:
        np.savez(fh, **d)
    e = load_trainer_npz(p2, make_trainer(rt, kind, params=other, opt="Adam", **kw))
    assert e.opt_state.state() == dict(b.opt_state.state(), lr_t=0.0)
    return path


def check_snapshot_rule_mismatch(rt, tmp_path):
    """`/v` is MomentumSGD's velocity and Adam's second moment: a snapshot of one rule is refused by a trainer of another."""
    from chainer_faster_rcnn_amd.serializers import load_trainer_npz, save_trainer_npz
    saved = {}
    for rule in ("MomentumSGD",) + RULES:
        tr = make_trainer(rt, "rpn", opt=rule)
        saved[rule] = str(tmp_path / ("snap_" + rule))
        save_trainer_npz(saved[rule], tr)
        with np.load(saved[rule]) as f:
            sfx = set(q.rsplit("/", 1)[1] for q in f.files if q.startswith("updater/optimizer:main/") and q.count("/") > 2)
        assert sfx == set(("v",) if rule == "MomentumSGD" else STATE_KEYS[rule]), (rule, sfx)
    for src in saved:
        for dst in saved:
            tr = make_trainer(rt, "rpn", params=T.small_params(seed=2), opt=dst)
            if src == dst:
                load_trainer_npz(saved[src], tr)
            else:
                w_before = P.host(rt, tr.moments[sorted(tr.moments)[0]]).copy()
                with np.testing.assert_raises(ValueError):
                    load_trainer_npz(saved[src], tr)
                assert np.array_equal(P.host(rt, tr.moments[sorted(tr.moments)[0]]), w_before)


def check_api(rt):
    for make in (lambda **kw: make_trainer(rt, "rpn", **kw), lambda **kw: make_trainer(rt, "rcnn", **kw)):
        for bad in (dict(opt="SGD"), dict(opt="adam"), dict(opt="Adam", opt_args=dict(lr=1e-3)), dict(opt="AdaGrad", opt_args=dict(alpha=0.9)),
                    dict(opt="MomentumSGD", opt_args=dict(eps=1e-8)), dict(opt="Adam", opt_args=dict(eps=0.0)), dict(opt="RMSprop", opt_args=dict(eps=-1.0)),
                    dict(opt="AdaGrad", opt_args=dict(eps=0))):
            with np.testing.assert_raises(ValueError):
                make(**bad)
        tr = make()
        assert tr.opt == "MomentumSGD" and tr.weight_decay == 0.0005 and (tr.lr, tr.momentum) == (0.001, 0.9) and tr.opt_state is None
        assert sorted(tr.moments) == ["v"] and tr.moments["v"] is tr.V
        for rule in RULES:
            tr = make(opt=rule)
            assert tr.weight_decay == 0.0 and trainer_hyper(tr) == DEFAULTS[rule], (rule, trainer_hyper(tr))
            assert make(opt=rule, weight_decay=0.0005).weight_decay == 0.0005
        assert make(weight_decay=0.001).weight_decay == 0.001


def check_default_is_momentum_sgd(rt, kind, steps=3, **common):
    """A default-constructed trainer and one passed opt="MomentumSGD", weight_decay=0.0005 explicitly: the same W and velocity bits.
    (common: arguments both get -- on the GPU RCNNTrainer's fp32 step scatters RoI gradients with float atomics, so two runs of it are
    compared under precision="bf16", whose scatter is ordered.)"""
    inputs = trainer_inputs(rt, kind)
    out = []
    for kw in ({}, dict(opt="MomentumSGD", weight_decay=0.0005)):
        tr = make_trainer(rt, kind, **dict(common, **kw))
        for it in range(steps):
            forward_backward(tr, kind, inputs, 30 + it)
            tr.update()
        out.append((P.host(rt, tr.W).copy(), P.host(rt, tr.V).copy()))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)) and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def check_readoption_keeps_moments(rt):
    """Two trainers on one model orphan each other's windows; re-adoption copies the parameters back and keeps the moments."""
    from chainer_faster_rcnn_amd.train import RPNTrainer
    tr = make_trainer(rt, "rpn", opt="Adam")
    inputs = trainer_inputs(rt, "rpn")
    forward_backward(tr, "rpn", inputs, 1)
    tr.update()
    m1, w1 = P.host(rt, tr.moments["m"]).copy(), P.host(rt, tr.W).copy()
    assert m1.any()
    RPNTrainer(tr.model)                                              # takes the links over
    tr._ensure_adopted()
    assert np.array_equal(P.host(rt, tr.moments["m"]), m1) and np.array_equal(P.host(rt, tr.W), w1) and tr.opt_state.state()["t"] == 1

