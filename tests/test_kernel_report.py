"""tests/kernel_report.py reads a device assembly text as the resource tests need it: which labels are kernels, their names and
template arguments decoded from the mangled symbol, the report block and the instruction counts.  A short synthetic text, in the
compiler's layout; no compiler needed."""
import pytest

import kernel_report

ASM = """
	.type	_ZN12_GLOBAL__N_19k_gm_foldEijPKjS1_Pf,@function
_ZN12_GLOBAL__N_19k_gm_foldEijPKjS1_Pf:   ; @_ZN12_GLOBAL__N_19k_gm_foldEijPKjS1_Pf
; %bb.0:
	v_cmp_eq_u32_e32 vcc, 0, v0
	;;#ASMSTART
	s_memtime s[6:7]
 s_waitcnt lgkmcnt(0)
	;;#ASMEND
	v_mov_b32_e32 v1, 0
.LBB0_2:
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _ZN12_GLOBAL__N_19k_gm_foldEijPKjS1_Pf
		.amdhsa_next_free_vgpr 4
	.end_amdhsa_kernel
	.set _ZN12_GLOBAL__N_19k_gm_foldEijPKjS1_Pf.num_vgpr, 4
; Kernel info:
; codeLenInByte = 192
; TotalNumSgprs: 18
; NumVgprs: 4
; ScratchSize: 0
; LDSByteSize: 192 bytes/workgroup (compile time only)
; Occupancy: 8
; WaveLimiterHint : 0
; COMPUTE_PGM_RSRC2:SCRATCH_EN: 0
_ZN12_GLOBAL__N_16helperILi3EEEvPf:     ; a device function: its body and report belong to no kernel
	v_readlane_b32 s0, v0, 1
	s_setpc_b64 s[30:31]
; NumVgprs: 99
; ScratchSize: 40
_Z12k_resp_tile3ILi3ELb1ELin2ELj7EdN5lslam4GeomEEvPK15HIP_vector_typeIjLj4EEi:
	v_mfma_i32_16x16x64_i8 a[0:3], v[2:5], v[6:9], a[0:3]
	v_mfma_i32_16x16x64_i8 a[4:7], v[2:5], v[6:9], a[4:7]
	v_permlane32_swap_b32_e64 v1, v2
	v_add_u32_e64 v1, v2, v3
	v_add_u32_e32 v1, v2, v3
	s_endpgm
	.amdhsa_kernel _Z12k_resp_tile3ILi3ELb1ELin2ELj7EdN5lslam4GeomEEvPK15HIP_vector_typeIjLj4EEi
	.end_amdhsa_kernel
; NumVgprs: 45
; NumAgprs: 12
; ScratchSize: 0
; Occupancy: 8
"""


def test_kernels_names_arguments_resources_and_counts():
    seen = kernel_report.parse(ASM)
    fold, tile3 = ("k_gm_fold", ()), ("k_resp_tile3", (3, True, -2, 7, "d", "N5lslam4GeomE"))
    assert set(seen) == {fold, tile3}  # the device function is no kernel
    assert seen[fold].resources == {"TotalNumSgprs": 18, "NumVgprs": 4, "ScratchSize": 0, "LDSByteSize": 192, "Occupancy": 8}
    assert seen[fold].ops == {"v_cmp_eq_u32": 1, "s_memtime": 1, "s_waitcnt": 1, "v_mov_b32": 1, "s_endpgm": 1}
    assert seen[tile3].resources == {"NumVgprs": 45, "NumAgprs": 12, "ScratchSize": 0, "Occupancy": 8}
    assert seen[tile3].ops == {"v_mfma_i32_16x16x64_i8": 2, "v_permlane32_swap_b32": 1, "v_add_u32": 2, "s_endpgm": 1}
    assert seen[tile3].ops["v_readlane_b32"] == 0  # a mnemonic that is not there counts zero


@pytest.mark.parametrize("symbol, key", [
    ("_ZN12_GLOBAL__N_111k_resp_rowsILi3ELi11ELb1ELb0ELb0ELb0EEEvPKhS2_ii", ("k_resp_rows", (3, 11, True, False, False, False))),
    ("_ZN12_GLOBAL__N_112k_match_stepILi4ELi8ELi3EfEEvPKT2_iPKd", ("k_match_step", (4, 8, 3, "f"))),
    ("_ZN12_GLOBAL__N_18k_deskewENS_9DeskewCfgEPKf", ("k_deskew", ())),
    ("_Z6k_testI15HIP_vector_typeIdLj2EEPKS_IfLi4EEEvT_", ("k_test", ("15HIP_vector_typeIdLj2EE", "PKS_IfLi4EE"))),
])
def test_decode(symbol, key):
    assert kernel_report.decode(symbol) == key


@pytest.mark.parametrize("symbol", [
    "k_plain_c_name",                               # not mangled
    "_ZN12_GLOBAL__N_111k_resp_rowsILi3ELi11EEvPKh",   # the nested name is not closed
    "_ZN12_GLOBAL__N_16k_halfILDh15360EEEvPf",      # a literal of a type that is not decoded
    "_Z6k_openILi3E",                               # the arguments run off the end
    "_ZN12_GLOBAL__N_199k_shortEv",                 # the length runs off the end
])
def test_an_undecodable_kernel_symbol_raises(symbol):
    with pytest.raises(ValueError, match=symbol):
        kernel_report.decode(symbol)
    with pytest.raises(ValueError, match=symbol):
        kernel_report.parse("%s:\n\ts_endpgm\n\t.amdhsa_kernel %s\n" % (symbol, symbol))
