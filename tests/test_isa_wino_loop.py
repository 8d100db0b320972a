"""Static check of the Winograd chunk loop on the compiled kernels (no GPU: hipcc -S cross-compiles gfx950, the mechanism of
tests/test_isa_waits.py): on the listing of every shipped Winograd kernel -- conv_wino_f32_kernel's four instantiations and wino_sk_f32_kernel's
two -- the chunk loop holds no packed fp32 VALU and no address arithmetic, and its instruction counts per 32 MFMAs (one 8-channel chunk of a
wave) stay at or below the adopted form's figures in profiles/wino_loop_gate.txt.  Only ordinary opcodes (v_*, ds_read*, buffer_load ... lds,
s_nop) and the kernel descriptors' register / LDS / scratch fields are looked at (scripts/isa_wino_loop_scan.py)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# profiles/wino_loop_gate.txt, "adopted form" rows (the line "# ISA-BOUNDS ..." there states the same figures; the first loop had 48 VALU, 24 LDS
# reads, 10 DMA pieces and 14 s_nop).  Whole-chunk kernels run the transform's 32 VALU and nothing else; the ragged-Cin kernels build two
# buffer descriptors per chunk on top (2 VALU per chunk: 4 per 32 MFMAs with 4-channel chunks).
BOUNDS = {"valu": 32, "valu_ragged": 36, "lds_read": 24, "dma": 10, "s_nop": 12}
BOUNDS_LINE = "# ISA-BOUNDS per 32 MFMAs: VALU 32 (ragged Cin: 36), LDS reads 24, DMA pieces 10, s_nop 12"
SHIPPED = [("conv_wino_f32_kernelILi2ELi1ELi8ELi2ELb1E", False), ("conv_wino_f32_kernelILi2ELi1ELi8ELi2ELb0E", True),
           ("conv_wino_f32_kernelILi2ELi1ELi4ELi2ELb1E", False), ("conv_wino_f32_kernelILi2ELi1ELi4ELi2ELb0E", True),
           ("wino_sk_f32_kernelILb1E", False), ("wino_sk_f32_kernelILb0E", True)]


@pytest.fixture(scope="module")
def scan():
    spec = importlib.util.spec_from_file_location("isa_wino_loop_scan", os.path.join(ROOT, "scripts", "isa_wino_loop_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from test_isa_waits import asm_of
    return open(asm_of("conv_wino", tmp_path_factory.mktemp("isa_wino"))).read()


def test_bounds_are_the_gate_files():
    text = open(os.path.join(ROOT, "profiles", "wino_loop_gate.txt")).read()
    assert BOUNDS_LINE in text
    nums = [int(v) for v in re.findall(r"\d+", BOUNDS_LINE.split(":", 1)[1])]
    assert nums == [BOUNDS["valu"], BOUNDS["valu_ragged"], BOUNDS["lds_read"], BOUNDS["dma"], BOUNDS["s_nop"]]
    assert BOUNDS["valu"] < 48 and BOUNDS["valu_ragged"] < 48 and BOUNDS["lds_read"] <= 24 and BOUNDS["dma"] <= 10 and BOUNDS["s_nop"] < 14


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("frag,ragged", SHIPPED, ids=[f for f, _ in SHIPPED])
def test_shipped_loop_is_lean(scan, listing, frag, ragged):
    kernels = {k: v for k, v in scan.kernels(listing).items() if frag in k}
    assert len(kernels) == 1, sorted(kernels)
    (name, lines), = kernels.items()
    regs, lds, scratch = scan.descriptors(listing)[name]
    assert scratch == 0 and regs <= 256 and lds <= 81920, (name, regs, lds, scratch)
    span = scan.chunk_loop(lines)
    assert span is not None, name
    body = [t for t in lines[span[0]:span[1] + 1] if not t.endswith(":")]
    mfma = [i for i, t in enumerate(body) if t.startswith("v_mfma")]
    assert len(mfma) in (32, 64), (name, len(mfma))                       # two chunks per trip: 2 x 32 (8-channel chunks) or 2 x 16
    assert all("32x32x2" in body[i] for i in mfma)
    # the whole loop body, a superset of what lies between its first and last MFMA
    ops = [t.split()[0] for t in body]
    assert not [o for o in ops if o.startswith("v_pk_")], name
    assert not [o for o in ops if o.startswith(("v_add_u32", "v_lshl_add_u32", "v_add_co_u32", "v_sub_u32", "v_add3_u32", "v_lshlrev_b32"))], name
    c = scan.counts(lines)
    print("ISA %s: regs %d lds %d; per 32 MFMAs valu %.1f lds_read %.1f dma %.1f s_nop %.1f total %.1f" % (frag, regs, lds, c["valu"], c["lds_read"], c["dma"], c["s_nop"], c["total"]))
    assert c["valu"] <= (BOUNDS["valu_ragged"] if ragged else BOUNDS["valu"]), (name, c)
    assert c["lds_read"] <= BOUNDS["lds_read"] and c["dma"] <= BOUNDS["dma"] and c["s_nop"] <= BOUNDS["s_nop"], (name, c)
    assert c["packed"] == 0 and c["address"] == 0, (name, c)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_first_loop_is_the_comparison(scan, listing):
    """the research build's first loop (wino_lab_f32_kernel<2, 1, 8, 2, true, 0, 0>) still shows the parent's counts: the scan measures what it says"""
    (name, lines), = [(k, v) for k, v in scan.kernels(listing).items() if "wino_lab_f32_kernelILi2ELi1ELi8ELi2ELb1ELi0ELi0E" in k]
    c = scan.counts(lines)
    assert (c["mfma"], c["lds_read"], c["dma"]) == (32, 24, 10), c
    assert c["valu"] >= 48 and c["address"] >= 16 and c["s_nop"] >= 14 and c["packed"] == 0, c
    assert scan.descriptors(listing)[name][2] == 0
