"""Build-time properties of the transformer encoder's kernels (kernels_attention.hip; no GPU needed: hipcc cross-compiles gfx950),
the budget DESIGN.md section 4.7 states: every instantiation of self_attention_kernel - three element types x 1 .. 4 32-column
accumulator tiles per head - without scratch or spilled vector registers, at most 256 architectural + 64 accumulator registers,
and the K / V tiles of 64 rows in an LDS footprint that lets two workgroups share a CU; the two row kernels without LDS at full
occupancy."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, device_asm


def _lds_bytes(h16, d32):
    dp = 32 * d32
    if h16:                                               # K [64][DP + 8], V^T [DP][64 + 8], 2 bytes each
        return 64 * (dp + 8) * 2 + dp * 72 * 2
    k = 64 * (dp + 1) * 4                                  # K [64][DP + 1], V [64][DP + 8], 4 bytes each
    return (k + 15) // 16 * 16 + 64 * (dp + 8) * 4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_attention_instantiations_fit_registers_and_lds(tmp_path):
    blocks = re.split(r"remark: [^\n]*Function Name: ", device_asm("kernels_attention", tmp_path / "attention.s"))[1:]
    seen, rows = [], []
    for b in blocks:
        name = b.split()[0]
        field = lambda pat: int(re.search(pat, b).group(1))
        if "self_attention_kernel" in name:
            seen.append(name)
            et, d32 = (int(v) for v in re.search(r"self_attention_kernelILi(\d)ELi(\d)E", name).groups())
            assert field(r"VGPRs Spill: (\d+)") == 0 and field(r"ScratchSize \[bytes/lane\]: (\d+)") == 0, name
            assert field(r" VGPRs: (\d+)") <= 256 and field(r"AGPRs: (\d+)") <= 64, name
            assert field(r"Occupancy \[waves/SIMD\]: (\d+)") >= 1, name
            lds = field(r"LDS Size \[bytes/block\]: (\d+)")
            assert lds == _lds_bytes(et != 0, d32) and 2 * lds <= 160 * 1024, (name, lds)          # ET_F32 = 0
        elif "posenc_kernel" in name or "front_conv_kernel" in name:
            rows.append(name)
            assert field(r"VGPRs Spill: (\d+)") == 0 and field(r"ScratchSize \[bytes/lane\]: (\d+)") == 0, name
            assert field(r"LDS Size \[bytes/block\]: (\d+)") == 0 and field(r"Occupancy \[waves/SIMD\]: (\d+)") == 8, name
    assert len(seen) == 12 and len(rows) == 6, (seen, rows)      # ET_F32 / ET_BF16 / ET_F16 x D32 1 .. 4; two row kernels x three types
    asm = (tmp_path / "attention.s").read_text()
    assert "v_mfma_f32_32x32x2_f32" in asm and "v_mfma_f32_32x32x16_bf16" in asm and "v_mfma_f32_32x32x16_f16" in asm
    assert "v_cvt_pk_bf16_f32" in asm and "v_cvt_pk_f16_f32" in asm          # the probabilities, packed pairwise for the second product
    assert "ds_read_b128" in asm and "ds_read2_b64" in asm                    # K fragments; the two 8-byte halves of a V^T fragment
