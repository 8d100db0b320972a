"""The ResNet trunk's bf16 train-mode pass on the host emulator (tests/hipemu): the three 1x1 training entries of csrc/conv1x1_train_bf16.hip at the
smallest shapes that reach each of their paths, a narrow train_dtype="bf16" trunk checked layer by layer, and one step of each trainer on such a
model (tests/resnet16_train_cases.py)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import resnet16_train_cases as C  # noqa: E402
import resnet_train_cases as T  # noqa: E402

_ID = lambda s: "x".join(str(v) for v in s)  # noqa: E731


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


@pytest.mark.parametrize("shape", C.EMU_SHAPES, ids=_ID)
def test_entries_against_float64(rt, shape):
    C.check_float64(rt, *shape)


@pytest.mark.parametrize("shape", C.EMU_SHAPES, ids=_ID)
def test_entries_exact_at_every_split(rt, shape):
    C.check_exact(rt, *shape)


def test_entry_refusals(rt):
    C.check_refusals(rt)


@pytest.mark.parametrize("case", T.TRUNK_CASES, ids=lambda c: "%s_%dx%d" % ("".join(str(b) for b in c[0]), c[1], c[2]))
def test_trunk_layer_by_layer(rt, case):
    C.check_trunk(rt, *case)


def test_train_dtype_f32_is_the_unchanged_pass(rt):
    C.check_f32_unchanged(rt, *T.TRUNK_CASES[0])


def test_constructor_refusals(rt):
    C.check_constructor_refusals(rt)


def test_rpn_trainer_one_step(rt):
    C.check_rpn_step(rt)


def test_rcnn_trainer_one_step(rt):
    C.check_rcnn_step(rt)


def test_resume_and_inference_after_training(rt, tmp_path):
    C.check_resume_and_inference(rt, tmp_path)


def test_pinned_trainer_refusals(rt):
    C.check_pinned_refusals(rt)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_kernel_listings(tmp_path):
    """conv1x1_train_bf16.hip for gfx950 with the product's flags: no private segment (no spills), one LDS array of 2 x (32 MT + 128) rows x 128
    bytes in the six GEMM forms and none in the slab sum, every product on v_mfma_f32_32x32x16_bf16 and every conversion on v_cvt_pk_bf16_f32."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "chainer-faster-rcnn_amd", "csrc")
    asm = str(tmp_path / "conv1x1_train_bf16.s")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(root, "include"),
                    "-I", csrc, os.path.join(csrc, "conv1x1_train_bf16.hip"), "-o", asm], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(kernels) == 7, [k for k, _ in kernels]                 # (MT 2, 4) x (forward, input gradient, weight gradient) + the slab sum
    for name, body in kernels:
        field = lambda n: int(re.search(r"\.%s\s+(\d+)" % n, body).group(1))     # noqa: E731
        assert field("amdhsa_private_segment_fixed_size") == 0, name
        lds = 0 if "slab_sum" in name else (49152 if "ILi2E" in name else 65536)
        assert field("amdhsa_group_segment_fixed_size") == lds, name
    assert "scratch_" not in text
    assert "v_mfma_f32_32x32x16_bf16" in text and "v_cvt_pk_bf16_f32" in text
