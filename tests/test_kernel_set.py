"""The product library holds only the kernels the product dispatches to (rag_fin_amd/build.py): the
two translation units with hand-scheduled alternatives, scan_wide.hip and encoder.hip, are compiled
device-only to gfx950 assembly with the product's flags, and the kernels they emit must be exactly
the lists below.  A kernel that appears here without a product path that launches it -- an
instantiation behind a knob that is a constant in the product, a launcher that picks a template
argument at run time -- fails this test; so does a product path whose kernel went missing."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from rag_fin_amd import build

pytestmark = pytest.mark.skipif(not build.have_hipcc(), reason="hipcc not found")

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES_LN, EPI_PRE_LN = 0, 1, 2, 3   # encoder.hip
MODE_SAMPLE, MODE_EMIT = 0, 1                                       # scan_common.h

EXPECTED = {
    # <MODE, DBG, NE>: no diagnostics, the product's 12 LDS-DMA pieces per phase on waves 0-3
    "scan_wide.hip": {("k_scan_w16", (MODE_SAMPLE, 0, 12)), ("k_scan_w16", (MODE_EMIT, 0, 12))},
    "encoder.hip": {
        ("k_tok_offsets", ()), ("k_embed_ln", ()), ("k_attention", ()), ("k_pool_norm", ()), ("k_ln_rows", ()),
        ("k_qkv_attn_one", ()),
        # <key blocks, waves per SIMD, heads per workgroup, key-block groups>
        ("k_attention_mfma", (1, 6, 1, 1)), ("k_attention_mfma", (2, 6, 1, 1)), ("k_attention_mfma", (4, 4, 1, 1)),
        ("k_attention_mfma", (6, 4, 1, 2)), ("k_attention_mfma", (8, 4, 1, 2)),
        # <EPI, KS>: K = 384 for QKV, FFN1 and the out-projection, K = 1536 for FFN2 alone
        ("k_linear_small", (EPI_BIAS, 24)), ("k_linear_small", (EPI_BIAS_GELU, 24)), ("k_linear_small", (EPI_PRE_LN, 24)),
        ("k_linear_small", (EPI_PRE_LN, 96)),
        # <EPI, NTB, KS>
        ("k_linear", (EPI_BIAS, 2, 24)), ("k_linear", (EPI_BIAS_GELU, 2, 24)), ("k_linear", (EPI_BIAS_RES_LN, 2, 24)),
        ("k_linear", (EPI_BIAS_RES_LN, 2, 96)),
        # <WIDE, ABL>: 128- and 256-token workgroups, no ablation
        ("k_linear_dma", (0, 0)), ("k_linear_dma", (1, 0)),
    },
}


def kernel_of(mangled):
    """(name, integer template arguments) of an Itanium-mangled kernel symbol."""
    m = re.match(r"_Z(\d+)", mangled)
    assert m, mangled
    start = m.end()
    name, rest = mangled[start:start + int(m.group(1))], mangled[start + int(m.group(1)):]
    args = re.match(r"I((?:Li\d+E)+)E", rest)
    return name, tuple(int(a) for a in re.findall(r"Li(\d+)E", args.group(1))) if args else ()


def emitted_kernels(source, out_dir):
    out = os.path.join(str(out_dir), os.path.splitext(source)[0] + ".s")
    cmd = [build._hipcc(), *build.FLAGS, "--cuda-device-only", "-S", os.path.join(build.CSRC, source), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(out) as f:
        return [kernel_of(n) for n in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), flags=re.M)]


def test_mangled_names_parse():
    assert kernel_of("_Z10k_scan_w16ILi1ELi0ELi12EEv10WideParams") == ("k_scan_w16", (1, 0, 12))
    assert kernel_of("_Z9k_ln_rowsPKfPKiPKDF16_S4_fPDF16_") == ("k_ln_rows", ())


def test_product_emits_exactly_the_dispatched_kernels(tmp_path):
    with ThreadPoolExecutor(max_workers=2) as ex:
        got = dict(zip(EXPECTED, ex.map(lambda s: emitted_kernels(s, tmp_path), EXPECTED)))
    for source, want in EXPECTED.items():
        assert len(got[source]) == len(set(got[source])), source
        extra, missing = set(got[source]) - want, want - set(got[source])
        assert not extra and not missing, f"{source}: not dispatched by the product {sorted(extra)}, missing {sorted(missing)}"
