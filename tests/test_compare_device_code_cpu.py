"""scripts/compare_device_code.py on literal assembly (no compiler, no GPU): what its normalisation drops, what it
keeps, and what its report says about functions that differ or exist on one side only."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("compare_device_code",
                                               os.path.join(ROOT, "scripts", "compare_device_code.py"))
cdc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cdc)


def kernel(name, index, reg="v2", cuid="1a2b3c", line=10):
    """One kernel as hipcc writes it: the function's index in its file sits in the .LBB / .Lfunc_end labels, the
    descriptor lies between the code and the .size line, the compilation unit's id behind the function."""
    return f"""\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.file\t{index} "somewhere/file{index}.hip"
\t.section\t.text.{name},"axG",@progbits,{name},comdat
\t.globl\t{name} ; -- Begin function {name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
\t.loc\t{index} {line} 3 prologue_end ; file{index}.hip:{line}:3
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_i32_e32 vcc, 1, v0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB{index}_2
; %bb.1: ; in Loop: Header=BB{index}_1 Depth=1
\tv_mov_b32_e32 {reg}, 0
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v0, {reg}, s[0:1]
.LBB{index}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 3
\t.end_amdhsa_kernel
\t.section\t.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{index}:
\t.size\t{name}, .Lfunc_end{index}-{name}
                                        ; -- End function
\t.type\t__hip_cuid_{cuid},@object
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
\t.size\t__hip_cuid_{cuid}, 1
"""


def lib(*texts):
    return cdc.merge(cdc.split_functions(t) for t in texts)


def test_label_indices_cuids_and_line_numbers_do_not_count():
    a = lib(kernel("_Z3fooPi", 0, cuid="aaaa", line=10) + kernel("_Z3barPi", 1, cuid="aaaa", line=20))
    # the same two kernels, instantiated in the other order, in two files, on other source lines
    b = lib(kernel("_Z3barPi", 0, cuid="bbbb", line=31), kernel("_Z3fooPi", 0, cuid="cccc", line=7))
    assert sorted(a) == sorted(b) == ["_Z3barPi", "_Z3fooPi"]   # no __hip_cuid_ object among the functions
    r = cdc.compare(a, b)
    assert r == {"device_functions_compared": 2, "identical": 2, "not_identical": {}, "only_in_first": [],
                 "only_in_second": []}
    text = a["_Z3fooPi"][0]
    assert "\t.amdhsa_kernel _Z3fooPi" in text and "\t\t.amdhsa_next_free_vgpr 3" in text   # the descriptor is compared
    assert "\ts_cbranch_execz .LBB_2" in text and ".LBB_2:" in text and ".Lfunc_end:" in text
    assert not any(";" in line or ".loc" in line or ".file" in line for line in text)


def test_a_changed_register_is_a_difference():
    a = lib(kernel("_Z3fooPi", 0) + kernel("_Z3barPi", 1))
    b = lib(kernel("_Z3fooPi", 0, reg="v3") + kernel("_Z3barPi", 1))
    r = cdc.compare(a, b)
    assert r["device_functions_compared"] == 2 and r["identical"] == 1
    assert r["not_identical"] == {"_Z3fooPi": 2}   # the move and the store
    assert r["only_in_first"] == [] and r["only_in_second"] == []


def test_a_changed_descriptor_is_a_difference():
    a = lib(kernel("_Z3fooPi", 0))
    b = lib(kernel("_Z3fooPi", 0).replace(".amdhsa_next_free_vgpr 3", ".amdhsa_next_free_vgpr 4"))
    assert cdc.compare(a, b)["not_identical"] == {"_Z3fooPi": 1}


def test_a_function_on_one_side_only_is_reported():
    a = lib(kernel("_Z3fooPi", 0) + kernel("_Z3barPi", 1))
    b = lib(kernel("_Z3fooPi", 0), kernel("_Z3bazPi", 0))
    r = cdc.compare(a, b)
    assert r["device_functions_compared"] == 1 and r["identical"] == 1 and r["not_identical"] == {}
    assert r["only_in_first"] == ["_Z3barPi"] and r["only_in_second"] == ["_Z3bazPi"]
    # ... and so is a second definition of a name (kernels in the anonymous namespaces of two files)
    r = cdc.compare(lib(kernel("_Z3fooPi", 0), kernel("_Z3fooPi", 3)), lib(kernel("_Z3fooPi", 0)))
    assert r["device_functions_compared"] == 1 and r["only_in_first"] == ["_Z3fooPi"]
