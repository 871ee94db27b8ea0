"""tools/kernel_asm_diff.py --renamed: a base kernel is compared with the kernel that has another name here, section switches do not count.

The matching code is fed two small hand-written listings with already-demangled names, so neither a compiler nor c++filt is needed.
"""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("kernel_asm_diff", os.path.join(ROOT, "tools", "kernel_asm_diff.py"))
kad = importlib.util.module_from_spec(spec)
spec.loader.exec_module(kad)


def kernel(symbol, section, third, n):
    """the listing of one kernel: its section line, three instructions (one with a jump table that leaves and re-enters the section), descriptor"""
    return [
        "\t" + section,
        "\t.globl\t%s" % symbol,
        "%s:" % symbol,
        "\ts_load_dwordx2 s[0:1], s[4:5], 0x0 ; comment",
        "\ts_cbranch_scc1 .LBB%d_2" % n,
        "\t.section\t.rodata,\"a\",@progbits",
        "\t.p2align\t2, 0x0",
        "\t" + section,
        ".LBB%d_2:" % n,
        "\t" + third,
        "\ts_endpgm",
        ".Lfunc_end%d:" % n,
        "\t.section\t.rodata,\"a\",@progbits",
        "\t.amdhsa_kernel %s" % symbol,
        "\t\t.amdhsa_next_free_vgpr 12",
        "\t.end_amdhsa_kernel",
    ]


def comdat(symbol):
    return '.section\t.text.%s,"axG",@progbits,%s,comdat' % (symbol, symbol)


BASE_PRETTY = {"_Z4sameX": "k_errors_kb8(lba::Dev, kb8::Cam)", "_Z4diffX": "k_lin_all_kb8(lba::Dev, kb8::Cam)", "_Z4keptX": "k_reduce(lba::Dev)"}
HERE_PRETTY = {"_Z4sameY": "k_errors<kb8::Cam>(lba::Dev, kb8::Cam)", "_Z4diffY": "k_lin_all<kb8::Cam>(lba::Dev, kb8::Cam)", "_Z4keptY": "k_reduce(lba::Dev)"}
BASE = kernel("_Z4sameX", ".text", "v_add_f64 v[0:1], v[0:1], v[2:3]", 0) + kernel("_Z4diffX", ".text", "v_add_f64 v[0:1], v[0:1], v[2:3]", 1) + \
    kernel("_Z4keptX", ".text", "v_mul_f64 v[0:1], v[0:1], v[2:3]", 2)
HERE = kernel("_Z4keptY", comdat("_Z4keptY"), "v_mul_f64 v[0:1], v[0:1], v[2:3]", 0) + kernel("_Z4sameY", comdat("_Z4sameY"), "v_add_f64 v[0:1], v[0:1], v[2:3]", 1) + \
    kernel("_Z4diffY", comdat("_Z4diffY"), "v_add_f64 v[0:1], v[0:1], v[4:5]", 2)
RENAMES = [("k_errors_kb8", "k_errors<kb8::Cam>"), ("k_lin_all_kb8", "k_lin_all<kb8::Cam>")]


def listings():
    return kad.kernels_of_lines(BASE, BASE_PRETTY), kad.kernels_of_lines(HERE, HERE_PRETTY)


def test_renamed_kernels_are_compared_with_their_new_names():
    kb, kh = listings()
    same, differ, gone, new = kad.compare(kb, kh, RENAMES)
    assert sorted(same) == ["k_errors<kb8::Cam>(lba::Dev, kb8::Cam)", "k_reduce(lba::Dev)"]     # the second: comdat section line against .text
    assert differ == ["k_lin_all<kb8::Cam>(lba::Dev, kb8::Cam)"]                                # one instruction differs
    assert gone == [] and new == []


def test_without_renames_the_pair_is_missing_plus_new():
    kb, kh = listings()
    same, differ, gone, new = kad.compare(kb, kh)
    assert same == ["k_reduce(lba::Dev)"] and differ == []
    assert sorted(gone) == ["k_errors_kb8(lba::Dev, kb8::Cam)", "k_lin_all_kb8(lba::Dev, kb8::Cam)"]
    assert sorted(new) == ["k_errors<kb8::Cam>(lba::Dev, kb8::Cam)", "k_lin_all<kb8::Cam>(lba::Dev, kb8::Cam)"]


def test_key_of_a_kernel_with_an_empty_parameter_pack():
    """c++filt leaves an empty slot where a pack is empty; the key is the one of the plain function with the same parameters"""
    assert kad.unqualified("void lba::k_errors<>(lba::Dev, , double const*, double const*)") == "k_errors<>(lba::Dev, double const*, double const*)"
    assert kad.unqualified("void lba::k_lin_all_b<kb8::Rig>(lba::BWin const*, lba::BDynAll, kb8::Rig)") == "k_lin_all_b<kb8::Rig>(lba::BWin const*, lba::BDynAll, kb8::Rig)"
    assert kad.unqualified("void poseopt::k_pose_opt<false, 4, poseopt::Fisheye>(poseopt::ProblemDev const*, poseopt::Fisheye)") == \
        "k_pose_opt<false, 4, poseopt::Fisheye>(poseopt::ProblemDev const*, poseopt::Fisheye)"


def test_only_section_switches_are_dropped():
    kb, _ = listings()
    body = kb["k_reduce(lba::Dev)"]
    assert '.section .rodata,"a",@progbits' in body and ".text" not in body           # leaving the text section still counts
    assert "v_mul_f64 v[0:1], v[0:1], v[2:3]" in body and ".amdhsa_next_free_vgpr 12" in body
    assert kad.normalise([".text_like_directive 1", "\t.section .text.x,\"ax\",@progbits"], {}) == [".text_like_directive 1", '.section .text.x,"ax",@progbits']
