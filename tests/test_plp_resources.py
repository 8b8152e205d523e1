"""Build-time properties of the PLP / spectrogram kernels (csrc/frontend.hip; no GPU needed: hipcc cross-compiles gfx950), the budget
DESIGN.md section 4.3.4 states:
  plp_lpc_kernel (one lane per frame)          no scratch, no spilled register, at most 64 vector registers (full occupancy of 8 waves
                                               per SIMD), no static LDS - its pLP / pTmp arrays are dynamic LDS, 2 * lpc_order * 64
                                               floats, at most 32256 bytes at the largest order;
  fbank512_kernel<.., PLP | SPECTROGRAM>       no scratch, at most 168 vector registers (3 waves per SIMD, what 4 waves of 256 threads
                                               need to share a CU with two more workgroups), at most the filterbank kernel's 19456 bytes of LDS;
  fbank_kernel<.., PLP | SPECTROGRAM>          no scratch, at most 96 vector registers, no static LDS (two arrays of `padded` floats per wave).
The filterbank / MFCC instantiations are still there, one per sample type, and use no scratch either."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, device_asm

KIND_SPECTROGRAM, KIND_PLP = 1, 2
PLP_MAX_LPC_ORDER = 63


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_plp_and_spectrogram_kernels_fit_their_budget(tmp_path):
    from libs.amd import capi
    assert capi.PLP_MAX_LPC_ORDER == PLP_MAX_LPC_ORDER and 2 * PLP_MAX_LPC_ORDER * 64 * 4 == 32256 <= 64 * 1024
    blocks = re.split(r"remark: [^\n]*Function Name: ", device_asm("frontend", tmp_path / "frontend.s"))[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        field = lambda pat: int(re.search(pat, b).group(1))
        res = dict(vgpr=field(r" VGPRs: (\d+)"), spill=field(r"VGPRs Spill: (\d+)"), scratch=field(r"ScratchSize \[bytes/lane\]: (\d+)"),
                   lds=field(r"LDS Size \[bytes/block\]: (\d+)"), occ=field(r"Occupancy \[waves/SIMD\]: (\d+)"))
        if "plp_lpc_kernel" in name:
            seen["lpc"] = res
            assert res["spill"] == 0 and res["scratch"] == 0 and res["vgpr"] <= 64 and res["lds"] == 0 and res["occ"] == 8, (name, res)
            continue
        m = re.search(r"fbank512_kernelILb([01])E([sf])Li(\d)E", name)
        if m:
            mfcc, sample, kind = int(m.group(1)), m.group(2), int(m.group(3))
            seen[("512", mfcc, sample, kind)] = res
            assert res["spill"] == 0 and res["scratch"] == 0 and res["lds"] <= 19456, (name, res)
            if kind:
                assert not mfcc and res["vgpr"] <= 168 and res["occ"] >= 3, (name, res)
            continue
        m = re.search(r"fbank_kernelI([sf])Li(\d)E", name)
        if m:
            sample, kind = m.group(1), int(m.group(2))
            seen[("generic", sample, kind)] = res
            assert res["spill"] == 0 and res["scratch"] == 0 and res["lds"] == 0, (name, res)
            if kind:
                assert res["vgpr"] <= 96, (name, res)
    assert "lpc" in seen
    for sample in "sf":
        for kind in (KIND_SPECTROGRAM, KIND_PLP):
            assert ("512", 0, sample, kind) in seen and ("generic", sample, kind) in seen, (sample, kind, sorted(map(str, seen)))
        assert ("512", 0, sample, 0) in seen and ("512", 1, sample, 0) in seen and ("generic", sample, 0) in seen
    assert len(seen) == 1 + 8 + 6
    # the recursion's code: no packed arithmetic (every operation rounded on its own), no scratch access
    asm = (tmp_path / "frontend.s").read_text()
    start = re.search(r"^_ZN\S*plp_lpc_kernel\S*:", asm, re.M).end()
    body = asm[start:asm.index("s_endpgm", start)]
    assert "v_pk_fma_f32" not in body and "v_pk_mul_f32" not in body and "v_pk_add_f32" not in body and "scratch_" not in body
    assert "ds_read" in body and "ds_write" in body and "v_add_f64" in body                     # LDS arrays; the double inner sum
