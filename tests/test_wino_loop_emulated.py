"""The Winograd chunk loop (wino_tile_loop, csrc/conv_wino.hip) on the host emulator (tests/hipemu, research build): every row of
tests/wino_loop_cases.py bit for bit against the first loop (FRCNN_CONV_WINO_LOOP=0), under the float64 bar, with the epilogue equalities and
no poison left; the in-kernel-split ranges; repeats with a NaN workspace; one pass with every LDS-DMA piece landing at its covering wait and
one with the workgroups run last to first."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
import wino_loop_cases as LC  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


def test_table_covers_the_loop_cases():
    LC.table_covers()


@pytest.mark.parametrize("case", LC.TABLE, ids=LC.case_id)
def test_loop_case_bits_and_float64(rt, case):
    LC.check_case(rt, case, first_loop=True)


@pytest.mark.parametrize("env", LC.SK_ENVS, ids=LC.WC.env_id)
def test_loop_in_kernel_split_ranges(rt, env):
    LC.check_sk(rt, env, first_loop=True)


@pytest.mark.parametrize("n", [2, 3])
def test_loop_in_kernel_split_equals_classic(rt, n):
    LC.check_sk_equals_classic(rt, n)


def test_loop_repeats_with_nan_workspace(rt):
    LC.check_repeats(rt)


def test_loop_chunk_sizes_agree(rt):
    LC.check_chunk_sizes_agree(rt)


def test_every_research_form_gives_the_first_loops_bits(rt):
    """the gate's arms (FRCNN_CONV_WINO_LOOP = 1, 5, 7: whole 8-channel chunks only) against the first loop, classic and in-kernel-split entry"""
    for shape, env in [((24, 64, 6, 33), {}), ((16, 128, 9, 66), {}), (LC.SK_SHAPE, LC.SK_ENVS[2])]:
        want = LC.run(rt, shape, dict(env, **LC.FIRST_LOOP), 4)
        for form in ("1", "5", "7"):
            got = LC.run(rt, shape, dict(env, FRCNN_CONV_WINO_LOOP=form), 4)
            assert not (got == LC.POISON).any() and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, form)


def test_loop_with_late_landing(rt, monkeypatch):
    """Every LDS-DMA piece lands only at the wait that covers it (HIPEMU_DMA_DEFER=1): a step-0 fragment read, or a border zero, that ran ahead
    of the chunk's wait would see the previous chunk's floats."""
    first = LC.order_outputs(rt)
    monkeypatch.setenv("HIPEMU_DMA_DEFER", "1")
    again = LC.order_outputs(rt)
    for a, c in zip(first, again):
        assert not (a == LC.POISON).any() and np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_loop_does_not_depend_on_workgroup_order(rt, tmp_path):
    """a fresh process that runs the workgroups last to first (HIPEMU_BLOCK_ORDER=reverse) gives the same bits"""
    first = LC.order_outputs(rt)
    out = str(tmp_path / "reverse.npz")
    code = ("import sys\nfor p in %r: sys.path.insert(0, p)\n"
            "import numpy as np\nfrom emu_runtime import emu_runtime\nimport wino_loop_cases as LC\n"
            "np.savez(%r, *LC.order_outputs(emu_runtime()))\nprint('ok')\n") % ([os.path.dirname(HERE), HERE, os.path.join(HERE, "hipemu")], out)
    env = {k: v for k, v in os.environ.items() if not k.startswith("FRCNN_CONV_WINO")}
    env["HIPEMU_BLOCK_ORDER"] = "reverse"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as f:
        again = [f["arr_%d" % i] for i in range(len(first))]
    for a, c in zip(first, again):
        assert a.shape == c.shape and not (a == LC.POISON).any() and np.array_equal(a, c)
