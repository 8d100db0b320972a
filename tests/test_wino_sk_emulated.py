"""The Winograd convolution that finishes its K split inside the kernel (frcnn_conv3x3_wino_sk_f32, csrc/conv_wino.hip) on the host
emulator (tests/hipemu, three CUs): the (shape, workgroup count) table of tests/wino_sk_cases.py against float64, bit-identity with the
classic entry under the same K pieces, repeatability with a poisoned workspace, the self-cleaning counter page, workgroup order and
late-landing DMA, and the status codes."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
import wino_sk_cases as SK  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


def test_table_covers_the_partition_cases(rt):
    """The table holds, by the restated range rule: a tile finished by its single owner; tiles shared by 2, 3 and >= 4 workgroups; a
    workgroup that ends one tile, owns whole tiles and begins another; G = 1; G = total; a forced G above total."""
    single = shared = ends_owns_begins = g_one = g_total = clipped = False
    counts = set()
    for shape, G in SK.TABLE:
        ntiles, nchunks = SK.dims(*shape)
        Gc, sharers, work = SK.plan_of(rt, shape, G)
        assert sum(c1 - c0 for p in work for _, c0, c1 in p) == ntiles * nchunks and all(work)
        counts |= set(sharers)
        single |= 1 in sharers and max(sharers) > 1               # next to shared tiles, in one launch
        shared |= max(sharers) > 1
        for p in work:
            whole = [c0 == 0 and c1 == nchunks for _, c0, c1 in p]
            ends_owns_begins |= len(p) >= 3 and not whole[0] and not whole[-1] and all(whole[1:-1]) and p[0][2] == nchunks and p[-1][1] == 0
        g_one |= Gc == 1 and ntiles > 1
        g_total |= Gc == ntiles * nchunks and nchunks > 1 and G is not None and G == ntiles * nchunks
        clipped |= G is not None and G > ntiles * nchunks and Gc == ntiles * nchunks
    assert single and shared and ends_owns_begins and g_one and g_total and clipped
    assert {1, 2, 3} <= counts and max(counts) >= 4, counts
    shapes = {s for s, _ in SK.TABLE}
    assert {s[3] % 4 for s in shapes} >= {1, 2, 3} and {s[0] % 8 == 0 for s in shapes} == {True, False}
    assert {s[1] // 64 for s in shapes} >= {1, 3} and (5, 64, 1, 1) in shapes and (4, 64, 2, 2) in shapes
    assert any(s[2] % 2 and s[3] % 2 for s in shapes)              # ragged last row and column under the pool


@pytest.mark.parametrize("case", SK.TABLE, ids=SK.case_id)
def test_sk_case_vs_float64(rt, case):
    SK.check_sk_case(rt, case)


@pytest.mark.parametrize("n", SK.PIECE_COUNTS)
@pytest.mark.parametrize("shape", SK.PIECE_SHAPES, ids=SK.WC.shape_id)
def test_sk_pieces_give_the_classic_bits(rt, shape, n):
    SK.check_sk_bits_against_classic(rt, shape, n)


@pytest.mark.parametrize("shape", [(68, 64, 5, 35), (64, 64, 6, 31), (100, 64, 23, 37)], ids=SK.WC.shape_id)
def test_sk_default_gives_the_classic_bits(rt, shape):
    assert (SK.default_pieces(rt, *shape) > 1) == (shape != (100, 64, 23, 37))          # two that split on three CUs, one that does not
    SK.check_sk_default_bits(rt, shape)


@pytest.mark.parametrize("case", SK.REPEAT_CASES, ids=SK.case_id)
def test_sk_repeats_and_nan_slots(rt, case):
    SK.check_sk_repeats(rt, case)


def test_sk_two_shapes_on_one_workspace(rt):
    SK.check_sk_two_shapes_one_workspace(rt)


def test_sk_does_not_depend_on_workgroup_order(rt, tmp_path):
    """A fresh process that runs the workgroups last to first (HIPEMU_BLOCK_ORDER=reverse) -- another workgroup draws the last ticket of
    every shared tile -- gives the same bits."""
    first = SK.sk_outputs(rt)
    out = str(tmp_path / "reverse.npz")
    code = ("import sys\nfor p in %r: sys.path.insert(0, p)\n"
            "import numpy as np\nfrom emu_runtime import emu_runtime\nimport wino_sk_cases as SK\n"
            "np.savez(%r, *SK.sk_outputs(emu_runtime()))\nprint('ok')\n") % ([os.path.dirname(HERE), HERE, os.path.join(HERE, "hipemu")], out)
    env = {k: v for k, v in os.environ.items() if not k.startswith("FRCNN_CONV_WINO")}
    env["HIPEMU_BLOCK_ORDER"] = "reverse"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as f:
        again = [f["arr_%d" % i] for i in range(len(first))]
    for a, c in zip(first, again):
        assert a.shape == c.shape and not (a == SK.POISON).any() and np.array_equal(a, c)


def test_sk_with_late_landing(rt, monkeypatch):
    """Every LDS-DMA piece lands only at the wait that covers it (HIPEMU_DMA_DEFER=1): the ring restart at a tile boundary included."""
    monkeypatch.setenv("HIPEMU_DMA_DEFER", "1")
    SK.check_sk_case(rt, ((68, 64, 5, 35), 10))
    SK.check_sk_case(rt, ((9, 192, 13, 97), 7))


def test_sk_balanced_ranges_knob(rt):
    """FRCNN_CONV_WINO_SK_BALANCE=1 on a shape the three-CU chip splits: six ranges over 4 tiles x 9 chunks, under the same checks"""
    assert SK.balanced_g(rt, 68, 64, 5, 35) == 6 and SK.default_pieces(rt, 68, 64, 5, 35) == 2
    SK.check_sk_case(rt, ((68, 64, 5, 35), "balance"))


def test_sk_status_codes_and_workspace_bytes(rt):
    SK.check_sk_status(rt)
