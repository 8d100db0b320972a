"""The Winograd F(2x2,3x3) fp32 convolution (csrc/conv_wino.hip) on the host emulator (tests/hipemu): the kernel at its edge shapes, with
both chunk sizes and with forced and natural K splits, against a float64 convolution under the oracle-relative bar (tests/wino_cases.py);
the exact-equality properties of its decompositions; the weight transform bit for bit; the status codes; and U following an optimizer
step and load_npz through the model classes.  The emulated chip has three CUs, so small maps split without being asked."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
import wino_cases as WC  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


@pytest.mark.parametrize("env", WC.ENVS, ids=WC.env_id)
@pytest.mark.parametrize("shape", WC.EDGE_SHAPES, ids=WC.shape_id)
def test_wino_edge_shape_vs_float64(rt, shape, env):
    WC.check_wino_shape(rt, shape, env)


def test_wino_edge_table_covers_every_grid_size_mod_8_and_the_split_paths(rt):
    """What the table is there for, checked instead of assumed: unsplit grids of every size mod 8 (the XCD remap's eight remainders),
    ragged and whole last chunks for both chunk sizes, every W % 4, and launches that do split -- forced, and by the default rule."""
    grids = {WC.plan(rt, *s, {"FRCNN_CONV_WINO_SPLIT": "1"})[2] % 8 for s in WC.EDGE_SHAPES}
    assert grids == set(range(8)), grids
    every = [WC.plan(rt, *s, e)[2] for s in WC.EDGE_SHAPES for e in WC.ENVS]
    assert any(8 < g < 16 for g in every) and any(g > 16 and g % 8 for g in every) and any(g >= 16 and g % 8 == 0 for g in every)   # whole rounds of eight, with and without a rest
    for ck in (8, 4):
        assert {s[0] % ck == 0 for s in WC.EDGE_SHAPES} == {True, False}
    assert {s[3] % 4 for s in WC.EDGE_SHAPES} == {0, 1, 2, 3}
    assert WC.plan(rt, 64, 64, 6, 31, {})[1] == 2 and WC.plan(rt, 68, 64, 5, 35, {})[1] == 2                 # the default rule, three CUs
    assert sum(WC.plan(rt, *s, WC.ENVS[2])[1] == 2 for s in WC.EDGE_SHAPES) >= 6
    assert sum(WC.plan(rt, *s, WC.ENVS[3])[1] == 3 for s in WC.EDGE_SHAPES) >= 6


@pytest.mark.parametrize("shape", WC.EDGE_SHAPES, ids=WC.shape_id)
def test_wino_chunk_size_does_not_change_the_bits(rt, shape):
    WC.check_wino_cfg_identical(rt, shape)


@pytest.mark.parametrize("case", [((64, 64, 6, 31), {}), ((68, 64, 5, 35), {"FRCNN_CONV_WINO_SPLIT": "3"}),
                                  ((9, 192, 13, 97), {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "2"})],
                         ids=lambda c: WC.shape_id(c[0]) + "_" + WC.env_id(c[1]))
def test_wino_split_repeats_and_nan_workspace(rt, case):
    WC.check_wino_split_repeats(rt, *case)


def test_wino_split_does_not_depend_on_workgroup_order(rt, tmp_path):
    """The K pieces land in their own slabs and wino_combine_kernel adds them in piece order: a fresh process that runs the workgroups
    last to first (HIPEMU_BLOCK_ORDER=reverse) gives the same bits."""
    first = WC.split_outputs(rt)
    out = str(tmp_path / "reverse.npz")
    code = ("import sys\nfor p in %r: sys.path.insert(0, p)\n"
            "import numpy as np\nfrom emu_runtime import emu_runtime\nimport wino_cases as WC\n"
            "np.savez(%r, *WC.split_outputs(emu_runtime()))\nprint('ok')\n") % ([os.path.dirname(HERE), HERE, os.path.join(HERE, "hipemu")], out)
    env = {k: v for k, v in os.environ.items() if not k.startswith("FRCNN_CONV_WINO")}
    env["HIPEMU_BLOCK_ORDER"] = "reverse"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as f:
        again = [f["arr_%d" % i] for i in range(len(first))]
    for a, c in zip(first, again):
        assert a.shape == c.shape and not (a == WC.POISON).any() and np.array_equal(a, c)


def test_wino_with_late_landing(rt, monkeypatch):
    """Every LDS-DMA piece lands only at the wait that covers it (HIPEMU_DMA_DEFER=1): a fragment read before the chunk's wait, or an
    edge fix that runs before the halo has landed, shows."""
    monkeypatch.setenv("HIPEMU_DMA_DEFER", "1")
    WC.check_wino_shape(rt, (68, 64, 5, 35), {})                                          # ragged chunks, border fix, split
    WC.check_wino_shape(rt, (16, 128, 9, 34), {"FRCNN_CONV_WINO_CFG": "2", "FRCNN_CONV_WINO_SPLIT": "1"})   # four whole 4-channel chunks, unsplit


def test_wino_pack(rt):
    WC.check_wino_pack(rt)


def test_wino_status_codes_and_workspace_bytes(rt):
    WC.check_wino_status(rt)


@pytest.mark.parametrize("variant", ["rpn", "rcnn", "load"])
def test_wino_weights_follow_the_parameters(rt, variant, tmp_path):
    WC.check_wino_derived(rt, variant, tmp_path)


def test_wino_error_ratios_recorded(rt):
    """Prints the range of err_wino / err_ref32 over this file's float64 checks (DESIGN.md 3.12 records it); the bar itself is asserted
    in every check."""
    if not WC.RATIOS:
        WC.check_wino_shape(rt, (12, 64, 7, 37), {})
    n, lo, hi = WC.ratio_summary()
    print("WINO emulator: %d checks, err_wino / err_ref32 = %.2f .. %.2f" % (n, lo, hi))
    assert n > 0 and all(ew <= 4 * er + 2e-7 for _, _, _, ew, er in WC.RATIOS)
