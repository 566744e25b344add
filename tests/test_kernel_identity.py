"""tools/kernel_identity.py on hand-written assembly: what it calls identical and what it reports. No compiler, no GPU."""
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("kernel_identity", os.path.join(ROOT, "tools", "kernel_identity.py"))
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)


def unit(kernels):
    """One unit's assembly in the compiler's layout. kernels: [(symbol, function index, body lines, vgprs, lds bytes)]"""
    text, records = ["\t.text"], []
    for symbol, index, body, vgprs, lds in kernels:
        text += ["\t.globl\t%s" % symbol, "\t.type\t%s,@function" % symbol, "%s:                 ; @%s" % (symbol, symbol), "; %bb.0:"]
        text += [line.replace("#", str(index)) for line in body]
        text += ["\ts_endpgm", "\t.section\t.rodata,\"a\",@progbits", "\t.amdhsa_kernel %s" % symbol, "\t\t.amdhsa_group_segment_fixed_size %d" % lds,
                 "\t\t.amdhsa_next_free_vgpr %d" % vgprs, "\t\t.amdhsa_next_free_sgpr 20", "\t.end_amdhsa_kernel", "\t.text", ".Lfunc_end%d:" % index,
                 "\t.size\t%s, .Lfunc_end%d-%s" % (symbol, index, symbol), "; NumVgprs: %d" % vgprs]
        records += ["  - .agpr_count:     0", "    .args:", "      - .offset:         0", "        .size:           8", "        .value_kind:     global_buffer",
                    "    .group_segment_fixed_size: %d" % lds, "    .name:           %s" % symbol, "    .private_segment_fixed_size: 0", "    .sgpr_count:     26",
                    "    .sgpr_spill_count: 0", "    .symbol:         %s.kd" % symbol, "    .vgpr_count:     %d" % vgprs, "    .vgpr_spill_count: 0"]
    return "\n".join(text + ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"] + records + ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata", ""])


LOOP = ["\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\ts_cbranch_scc1 .LBB#_2", ".LBB#_1:        ; =>This Inner Loop Header: Depth=1", "\tv_add_f32_e32 v1, v1, v2",
        "\ts_cbranch_vccnz .LBB#_1", ".LBB#_2:", "\tglobal_store_dword v0, v1, s[0:1]"]
OTHER = ["\tv_mov_b32_e32 v0, 0"]


def report(first, second):
    out = io.StringIO()
    result = tool.compare(first, second, out=out)
    return result, out.getvalue()


def test_the_same_body_under_other_label_numbers_is_identical():
    # kernel_a is function 3 of a big unit on one side and function 0 of its own unit on the other; the comment and the blanks after a label differ too
    first = tool.parse(unit([("kernel_b", 0, OTHER, 4, 0), ("kernel_a", 3, LOOP, 8, 256)]), "big")
    moved = [line.replace("        ; =>This Inner Loop Header: Depth=1", "  ; =>This Loop Header") for line in LOOP]
    second = dict(tool.parse(unit([("kernel_a", 0, moved, 8, 256)]), "small_a"), **tool.parse(unit([("kernel_b", 0, OTHER, 4, 0)]), "small_b"))
    assert first["kernel_a"].text[2:4] == ["s_cbranch_scc1 .L0", ".L1:"] and ".LBB" not in "".join(first["kernel_a"].text)
    assert first["kernel_a"].resources[".vgpr_count"] == "8" and first["kernel_a"].resources[".amdhsa_group_segment_fixed_size"] == "256"
    (identical, differing, only_first, only_second), text = report(first, second)
    assert sorted(identical) == ["kernel_a", "kernel_b"] and not differing and not only_first and not only_second
    assert "big -> small_a" in text and "2 identical in text and resources, 0 differ" in text


def test_a_changed_instruction_is_reported():
    first = tool.parse(unit([("kernel_a", 0, LOOP, 8, 256)]), "u")
    second = tool.parse(unit([("kernel_a", 0, [line.replace("v_add_f32_e32", "v_sub_f32_e32") for line in LOOP], 8, 256)]), "u")
    (identical, differing, only_first, only_second), text = report(first, second)
    assert differing == ["kernel_a"] and not identical
    assert "DIFFERS" in text and "(text)" in text and "-v_add_f32_e32 v1, v1, v2" in text and "+v_sub_f32_e32 v1, v1, v2" in text


def test_a_changed_register_count_is_reported():
    first = tool.parse(unit([("kernel_a", 0, LOOP, 8, 256)]), "u")
    second = tool.parse(unit([("kernel_a", 0, LOOP, 12, 256)]), "u")
    (identical, differing, only_first, only_second), text = report(first, second)
    assert differing == ["kernel_a"] and first["kernel_a"].text == second["kernel_a"].text
    assert ".vgpr_count 8 -> 12" in text and ".amdhsa_next_free_vgpr 8 -> 12" in text and "(text" not in text


def test_a_missing_symbol_is_reported_and_fails_the_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    (a / "u.s").write_text(unit([("kernel_a", 0, LOOP, 8, 256), ("kernel_b", 1, OTHER, 4, 0)]))
    (b / "u.s").write_text(unit([("kernel_a", 0, LOOP, 8, 256), ("kernel_c", 1, OTHER, 4, 0)]))
    (identical, differing, only_first, only_second), text = report(tool.load(str(a), 1), tool.load(str(b), 1))
    assert identical == ["kernel_a"] and only_first == ["kernel_b"] and only_second == ["kernel_c"]
    assert "only in the first: 1" in text and "only in the second: 1" in text
    assert tool.main([str(a), str(b)]) == 1 and tool.main([str(a), str(a)]) == 0
    assert tool.main([str(b / ".." / "a"), str(a)]) == 0
    # a symbol the second side adds does not fail the run: every entry point of the first is present and identical
    (b / "u.s").write_text(unit([("kernel_a", 0, LOOP, 8, 256), ("kernel_b", 1, OTHER, 4, 0), ("kernel_c", 2, OTHER, 4, 0)]))
    assert tool.main([str(a), str(b)]) == 0
