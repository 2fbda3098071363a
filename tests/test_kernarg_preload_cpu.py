"""Kernarg preload of the decode step's kernels, read from the cross-compiled device assembly that the build leaves next to each object
(csrc/build/*gfx950*.s, the files csrc/check_resources.py reads its metadata from).  For every instantiation of the seven kernel
families: the kernel descriptor asks for a non-zero preload length, and the preloaded dwords cover the arguments that the kernel's
first requests need -- an argument added in front of them, or a by-value struct in their place, fails here.  The metadata
carries the arguments' offsets and sizes but not their names, so the names come from the kernel's signature in the source: argument i
of the metadata is parameter i of the signature."""
import glob
import os
import re
import sys

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "index-tts-lora_amd", "csrc")
sys.path.insert(0, CSRC)
import check_resources  # noqa: E402

# family -> the arguments that must arrive in SGPRs, in the order of the signature (* = a pointer, 8 bytes; the others are 4-byte
# scalars: the metadata carries the arguments' offsets and sizes, not their names)
FAMILIES = {
    "gemm_skinny_kernel": ["*wp", "*x", "*pos", "M", "N", "K", "ksplit", "x_pa", "mtp", "row0", "nw"],
    "attn_decode_kernel": ["*q", "*pad", "*pos", "*skip_rows", "*kv_share", "*kv_tab", "H", "bs_log2"],
    "attn_decode_kv8_kernel": ["*qkv", "*pad", "*pos", "*skip_rows", "*kv_tab", "*kv_scale", "H", "bs_log2"],
    "ln_reduce_wide_kernel": ["*h", "*slab", "*bias", "*w", "*b", "M", "D", "sstride", "lora_r"],
    "embed_step_kernel": ["*tokens", "*step", "*row_step0", "*table", "*pos_table", "pos_add", "D", "pos_rows"],
    "sample_kernel": ["*logits", "*state", "*row_step0", "*finished", "*force_stop", "*rows", "V", "ldl"],
    "beam_step_kernel": ["*state", "*done", "*cand_n", "*cand_s", "*cand_i", "*hist", "B", "nb"],
}


def signature(family):
    """[(parameter name, is a pointer)] of `void <family>(...)` in csrc/, *_PARAMS macros of the same file expanded."""
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        src = open(path).read()
        m = re.search(r"__global__[^;{]*?\bvoid " + family + r"\(", src)
        if not m:
            continue
        text = src[m.end():src.index(")", m.end())]

        def expand(mm):
            d = re.search(r"#define " + mm.group(0) + r"\b((?:.*\\\n)*.*)", src)
            return d.group(1).replace("\\\n", " ") if d else ""      # (the diagnostic build's extra parameters: none in the product build)
        text = re.sub(r"\b[A-Z][A-Z0-9_]*_PARAMS\b", expand, text)
        out = []
        for part in text.split(","):
            part = part.strip()
            if part:
                out.append((re.search(r"(\w+)$", part).group(1), "*" in part))
        return out
    raise AssertionError(f"no kernel {family} in csrc/")


def descriptors(txt):
    """kernel name -> preload length in dwords, from the .amdhsa_kernel blocks."""
    out = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", body)
        out[name] = int(m.group(1)) if m else 0
    return out


def arguments(txt):
    """kernel name -> [(argument name, offset, size)] of the explicit arguments, from the amdhsa.kernels metadata."""
    m = re.search(r"amdhsa\.kernels:(.*?)amdhsa\.target", txt, re.S)
    out = {}
    for blk in re.split(r"\n  - ", m.group(1))[1:] if m else []:
        name = re.search(r"\n    \.name:\s*(\S+)", "\n" + blk).group(1)
        args = []
        for a in re.split(r"\n      - ", blk.split(".args:")[1].split("\n    .", 1)[0])[1:] if ".args:" in blk else []:
            f = dict(re.findall(r"\.(\w+):\s*(\S+)", a))
            if not f.get("value_kind", "").startswith("hidden"):
                args.append((f.get("name"), int(f["offset"]), int(f["size"])))
        out[name] = args
    return out


@pytest.fixture(scope="module")
def kernels():
    files = sorted(glob.glob(os.path.join(CSRC, "build", "*gfx950*.s")))
    assert files, "no device assembly under csrc/build: the library is built with -save-temps=obj (make -C index-tts-lora_amd/csrc)"
    found = {}
    for f in files:
        txt = open(f, errors="replace").read()
        pre, args = descriptors(txt), arguments(txt)
        assert {k["name"] for k in check_resources.kernels(f)} == set(args), f"{f}: the metadata readers disagree about the kernels"
        for name in args:
            found[name] = (pre[name], args[name])
    return found


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_first_request_arguments_are_preloaded(kernels, family):
    mine = {n: v for n, v in kernels.items() if re.search(r"\d" + family + r"[IE]", n)}
    assert mine, f"{family}: no instantiation in the build"
    want = [(f.lstrip("*"), f.startswith("*")) for f in FAMILIES[family]]
    assert signature(family)[:len(want)] == want, f"{family}: the signature in csrc/ begins with {signature(family)[:len(want)]}"
    for name, (dwords, args) in mine.items():
        assert dwords > 0, f"{name}: no kernarg preload"
        at = 0
        for field, (_, off, size) in zip(FAMILIES[family], args):
            want = 8 if field.startswith("*") else 4
            at = (at + want - 1) // want * want
            assert (off, size) == (at, want), f"{name}: {field} expected at bytes [{at}, {at + want}), the argument there is [{off}, {off + size})"
            at += want
            assert at <= 4 * dwords, f"{name}: {field} at bytes [{off}, {at}) lies behind the {dwords} preloaded dwords"


def test_the_flag_is_a_no_op_for_by_value_structs(kernels):
    """The vocoder and big-M GEMM kernels take one by-value struct: the flag must leave them exactly as they were."""
    convs = {n: v for n, v in kernels.items() if re.search(r"\d(gemm_conv_kernel|gemm_plain_kernel|conv_narrow\w*_kernel)[IE]", n)}
    assert convs
    assert all(d == 0 for d, _ in convs.values())
