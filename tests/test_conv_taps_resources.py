"""Build-time properties of the tap-table grid convolution kernel (kernels_conv_taps.hip; no GPU needed: hipcc cross-compiles
gfx950): every instantiation - three element types x 1 .. 4 output fragments per workgroup - without spilled registers or scratch,
and an LDS window (128 rows + twice the largest halo, 128 bytes each) that leaves room for two workgroups per CU, as the
kernel's launch bounds ask."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, device_asm


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_conv_taps_instantiations_fit_registers_and_lds(tmp_path):
    blocks = re.split(r"remark: [^\n]*Function Name: ", device_asm("kernels_conv_taps", tmp_path / "conv_taps.s"))[1:]
    seen = []
    for b in blocks:
        name = b.split()[0]
        if "grid_conv_taps_kernel" not in name:
            continue
        seen.append(name)
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
        assert int(re.search(r" VGPRs: (\d+)", b).group(1)) <= 256, name
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 2, name
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert lds == (128 + 2 * 168) * 128 and 2 * lds <= 160 * 1024, (name, lds)
    assert len(seen) == 12, seen                      # ET_F32 / ET_BF16 / ET_F16 x NF 1 .. 4
    asm = (tmp_path / "conv_taps.s").read_text()
    assert "v_mfma_f32_32x32x2_f32" in asm and "v_mfma_f32_32x32x16_bf16" in asm and "v_mfma_f32_32x32x16_f16" in asm
    assert "global_load_lds_dwordx4" in asm and "ds_read_b128" in asm
