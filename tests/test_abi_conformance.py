"""include/coflux.h, the ctypes mirror (coflux/abi.py) and the Julia binding (julia/CoFluxMI355X.jl) are three hand-kept
copies of one ABI.  tests/abi_model.py parses the three into one vocabulary; here they are held to each other and to what
the host C compiler makes of the header:

  * every struct — field names and order, every field's offset and size, total size and alignment, and the class of every
    field (a double where the header has an int64_t has the same offset and size) — header ↔ compiler ↔ ctypes and
    header ↔ compiler ↔ Julia under C layout rules; a Julia field whose type is a mutable struct is a defect, not a layout;
  * every exported symbol's argtypes / restype and every ccall's return type, type tuple and argument count against the
    prototype, by class (pointer, i32 … f64, usize, cstring, void); a typed pointer's pointee must be the twin of the struct
    the header names, an untyped one matches any pointer and is counted;
  * every integer constant a mirror defines against the header's value, which the compiler confirms.

The Julia file is never executed (no box has Julia): what is held is its TEXT.  Not held: enumerators the stub passes as
literals, GC.@preserve discipline and the wrappers' own logic, opaque handles among themselves (a cf_window* and a cf_ctx*
are both "a pointer" in every copy).

Each planted defect of abi_model.DEFECTS — one wrong copy in memory, no file is touched — must be reported by the name of
its struct or function and its field or position; the clean tree reports nothing.  Without a host C compiler the
compiler-dependent tests skip and the copy-against-copy comparisons still run."""
import pytest

import abi_model as am
from coflux import abi


@pytest.fixture(scope="session")
def header():
    return am.parse_header()


@pytest.fixture(scope="session")
def stub_text():
    return open(am.STUB_PATH).read()


@pytest.fixture(scope="session")
def compiled(header, tmp_path_factory):
    """The compiler's layout of every struct and value of every constant, once per session; None without a host compiler."""
    if am.c_compiler() is None:
        return None
    return am.compile_probe(header, str(tmp_path_factory.mktemp("abi_probe")))


@pytest.fixture(scope="session")
def layout(compiled):
    if compiled is None:
        pytest.skip("no host C compiler (cc, gcc, clang, nor a ROCm tree's clang): the header's layout has no witness")
    return compiled


@pytest.fixture(scope="session")
def clean(header, compiled, stub_text):
    return am.full_report(header, compiled, stub_text, abi, abi.load_library())


def test_the_parser_accounts_for_the_whole_header(header):
    """36 structs, 133 prototypes, 129 integer constants, one #define that is no integer; text the parser cannot place is an
    error that names the line."""
    assert len(header.structs) >= 36 and len(header.prototypes) >= 133 and len(header.constants) >= 129
    assert set(header.prototypes) == set(abi.EXPORTED_SYMBOLS)
    assert set(header.other_defines) == {"CF_STREAM_LEGACY"}
    assert header.prototypes["cf_device_alloc"] == (am.PTR, [("ctx", am.PTR), ("bytes", am.scalar("usize"))])
    assert header.prototypes["cf_debug_salinity_sums_exact"][1][5:] == [("sums_out", ("ptr", am.scalar("f64"))),
                                                                        ("nonfinite_out", ("ptr", am.scalar("u64")))]
    assert header.structs["cf_atmos_source"][0] == ("data", ("array", 9, ("ptr", am.scalar("f32"))))
    assert header.structs["cf_average_term"][:2] == [("kind", am.scalar("i32")), ("flags", am.scalar("i32"))]
    text = open(am.HEADER_PATH).read()
    for bad, line in (("int cf_sync(cf_ctx* ctx);", "int cf_sync(cf_ctx* ctx, struct { int a; } b);"),
                      ("    int32_t ring;", "    int32_t ring : 3;"),
                      ("    int32_t ring;", "    int32_t (*ring)(void);"),
                      ("int cf_sync(cf_ctx* ctx);", "int cf_sync(cf_ctxt* ctx);"),
                      ("int cf_sync(cf_ctx* ctx);", "static inline int cf_two(void) { return 2; }")):
        assert text.count(bad) == 1
        n = text[:text.index(bad)].count("\n") + 1
        with pytest.raises(am.AbiParseError, match=r"line %d\b" % n):
            am.parse_header(text.replace(bad, line))


def test_header_compiles_as_pedantic_c99_and_the_compiler_reads_the_same_constants(header, layout):
    assert set(layout.sizes) == set(header.structs)
    for name, fields in header.structs.items():
        assert [f for f, *_ in layout.fields[name]] == [f for f, _ in fields]
    assert layout.constants == header.constants


def test_header_compiles_as_cxx17(tmp_path):
    if am.cxx_compiler() is None:
        pytest.skip("no host C++ compiler (g++, clang++, nor a ROCm tree's clang++)")
    assert am.compile_cxx_include(str(tmp_path)) == ""


def _of(clean, *labels):
    return [p for p in clean.problems if p.startswith(labels)]


def test_every_struct_has_the_compilers_layout_in_ctypes(header, layout, clean):
    ct = am.ctypes_mirror(header, abi)
    assert sorted(ct.structs) == sorted(header.structs) and not ct.missing and not ct.extra
    assert am.struct_problems(header, layout, ct, "ctypes", am.ctypes_same_scalar) == []


def test_every_struct_has_the_compilers_layout_in_the_julia_stub(header, layout, stub_text):
    jl = am.julia_mirror(header, am.parse_stub(stub_text))
    assert sorted(jl.structs) == sorted(header.structs) and not jl.missing
    assert jl.extra == [] and sorted(jl.extra_layouts) == sorted(am.JULIA_EXTRA) == ["CfIceOceanParamsData"]
    assert am.struct_problems(header, layout, jl, "Julia") == []
    assert am.julia_extra_problems(header, layout, jl) == []


def test_mirrors_agree_with_each_other_field_by_field(header, stub_text):
    """Copy against copy: needs no compiler.  Names, order, offsets, sizes and classes of ctypes' own layout and of the
    stub's under C rules."""
    ct = am.ctypes_mirror(header, abi)
    jl = am.julia_mirror(header, am.parse_stub(stub_text))
    assert am.struct_problems(header, None, ct, "ctypes", am.ctypes_same_scalar) == []
    assert am.struct_problems(header, None, jl, "Julia") == []
    for h in header.structs:
        a, b = ct.structs[h], jl.structs[h]
        assert (a["size"], a["align"]) == (b["size"], b["align"]), h
        assert [(f, o, s) for f, _t, o, s in a["fields"]] == [(f, o, s) for f, _t, o, s in b["fields"]], h


def test_every_exported_symbol_has_its_prototypes_argtypes_and_restype(header):
    ct = am.ctypes_mirror(header, abi, abi.load_library())
    assert set(ct.functions) == set(abi.EXPORTED_SYMBOLS) == set(header.prototypes)
    problems, _untyped, checked = am.ctypes_function_problems(header, ct)
    assert problems == []
    assert checked == sum(len(p) for _r, p in header.prototypes.values())


def test_every_ccall_has_its_prototypes_return_type_tuple_and_argument_count(header, stub_text):
    jl = am.julia_mirror(header, am.parse_stub(stub_text))
    assert len(jl.ccalls) >= 122 and len(jl.ccalls) == stub_text.count("ccall(")
    problems, _untyped, _checked = am.ccall_problems(header, jl)
    assert problems == []


def test_every_constant_a_mirror_defines_has_the_headers_value(header, clean):
    assert _of(clean, "ctypes: CF_", "Julia: CF_", "header: ") == []
    assert clean.counts["ctypes constants compared"] >= 100 and clean.counts["Julia constants compared"] >= 50
    assert abi.ABI_VERSION == header.constants["CF_ABI_VERSION"] and abi.JRA55_NVARS == header.constants["CF_JRA55_NVARS"]


def test_the_clean_tree_reports_nothing(clean):
    assert clean.problems == []


@pytest.mark.parametrize("defect", list(am.DEFECTS))
def test_a_planted_defect_is_reported_by_name_and_position(header, compiled, stub_text, clean, defect):
    report = am.full_report(header, compiled, stub_text, abi, abi.load_library(), defect)
    new = [p for p in report.problems if p not in clean.problems]
    assert new, defect
    text = "\n".join(new)
    for words in am.DEFECTS[defect]:
        assert words in text, (defect, words, new)


def test_report_what_was_compared_and_what_no_mirror_defines(clean, capsys):
    """Informational: the counts are printed, and the header constants a mirror does not define are listed in the message
    of the closing assertion (the stub passes most enumerators as literals; they are not chased here)."""
    with capsys.disabled():
        print("\n[abi conformance] " + "; ".join("%s: %d" % kv for kv in clean.counts.items()))
        for mirror, names in clean.undefined.items():
            print("[abi conformance] header constants %s does not define (%d): %s" % (mirror, len(names), " ".join(names)))
    c = clean.counts
    assert c["structs"] == c["ctypes structs"] == c["Julia structs"] - len(am.JULIA_EXTRA), (c, clean.undefined)
    assert c["ctypes constants compared"] + c["ctypes constants undefined"] == c["constants"], (c, clean.undefined)
    assert c["Julia constants compared"] + c["Julia constants undefined"] == c["constants"], (c, clean.undefined)
