"""Instruction counts of the Winograd chunk loop (csrc/conv_wino.hip) from a gfx950 listing (hipcc -S --cuda-device-only).

The chunk loop of a kernel is its innermost backward-branch region that holds MFMAs; the counts are taken over that whole region (a superset of
what lies between its first and last MFMA, whichever way the compiler rotated the loop) and scaled to 32 MFMAs (one 8-channel chunk of a wave).  Classes: VALU (every v_* that is no MFMA), of which address
arithmetic (v_add_u32 / v_lshl_add_u32 and kin) and packed (v_pk_*); LDS reads (ds_read*); DMA pieces (buffer_load ... lds); s_nop; the rest.
Also the descriptor fields (registers, LDS, scratch).  Used by tests/test_isa_wino_loop.py and for profiles/wino_loop_gate.txt:
    python scripts/isa_wino_loop_scan.py listing.s [name fragment ...]"""
import re
import sys

ADDRESS_OPS = ("v_add_u32", "v_lshl_add_u32", "v_add_co_u32", "v_sub_u32", "v_lshlrev_b32", "v_add3_u32", "v_lshl_or_b32", "v_mad_u32_u24")      # opcode prefixes


def kernels(text):
    """{mangled name: [instruction lines and labels]} of every function of the listing"""
    out, name = {}, None
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and ln.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            t = ln.split(";")[0].strip()
            if t and not t.startswith(".") or re.match(r"^\.LBB\w+:", t or ""):
                out[name].append(t)
    return out


def chunk_loop(lines):
    """(label, back branch) line indices of the innermost backward-branch region with MFMAs: the whole loop, which holds everything between its
    first and its last MFMA whichever way the compiler rotated it"""
    labels = {t[:-1]: i for i, t in enumerate(lines) if t.endswith(":")}
    best = None
    for i, t in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\w+)|s_branch\s+(\.LBB\w+)", t)
        if not m:
            continue
        tgt = labels.get(m.group(1) or m.group(2))
        if tgt is None or tgt >= i:
            continue
        n = sum(1 for x in lines[tgt:i] if x.startswith("v_mfma"))
        if n and (best is None or i - tgt < best[1] - best[0]):
            best = (tgt, i)
    if best is None:
        return None
    return best


def counts(lines):
    """instruction classes of the loop, per 32 MFMAs"""
    span = chunk_loop(lines)
    if span is None:
        return None
    body = [t for t in lines[span[0]:span[1] + 1] if not t.endswith(":")]
    op = lambda t: t.split()[0]                                                   # noqa: E731
    mfma = sum(1 for t in body if op(t).startswith("v_mfma"))
    c = {"mfma": mfma, "total": len(body)}
    c["valu"] = sum(1 for t in body if op(t).startswith("v_") and not op(t).startswith("v_mfma"))
    c["address"] = sum(1 for t in body if op(t).startswith(ADDRESS_OPS))
    c["packed"] = sum(1 for t in body if op(t).startswith("v_pk_"))
    c["lds_read"] = sum(1 for t in body if op(t).startswith("ds_read"))
    c["dma"] = sum(1 for t in body if op(t).startswith("buffer_load") and t.endswith("lds"))
    c["s_nop"] = sum(1 for t in body if op(t) == "s_nop")
    c["m0"] = sum(1 for t in body if re.match(r"s_\w+\s+m0,", t))
    per32 = {k: (v * 32.0 / mfma if k not in ("mfma",) else v) for k, v in c.items()}
    return per32


def descriptors(text):
    """{kernel: (registers, LDS bytes, scratch bytes)} from the .amdhsa_kernel blocks"""
    out = {}
    for k, meta in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        f = lambda n: int(re.search(r"\.amdhsa_%s\s+(\d+)" % n, meta).group(1))     # noqa: E731
        out[k] = (f("next_free_vgpr"), f("group_segment_fixed_size"), f("private_segment_fixed_size"))
    return out


def main(argv):
    text = open(argv[1]).read()
    want = argv[2:]
    desc = descriptors(text)
    for name, lines in sorted(kernels(text).items()):
        if name not in desc or (want and not any(w in name for w in want)):
            continue
        c = counts(lines)
        if c is None:
            continue
        print("%s\n    regs %d lds %d scratch %d | per 32 MFMAs (loop holds %d): total %.1f valu %.1f (address %.1f, packed %.1f) lds_read %.1f dma %.1f s_nop %.1f m0 %.1f"
              % (name, desc[name][0], desc[name][1], desc[name][2], c["mfma"], c["total"], c["valu"], c["address"], c["packed"], c["lds_read"], c["dma"],
                 c["s_nop"], c["m0"]))


if __name__ == "__main__":
    main(sys.argv)
