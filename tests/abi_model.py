"""The library's boundary exists in three hand-kept copies — include/coflux.h, the ctypes mirror (coflux/abi.py) and the
Julia binding (julia/CoFluxMI355X.jl).  This module parses each of them into ONE vocabulary, so that
tests/test_abi_conformance.py can compare them field by field and parameter by parameter.

A type is a tuple:
    ("scalar", cls)        cls in i8 u8 i32 u32 i64 u64 f32 f64 usize char void
    ("ptr", pointee)       pointee is a type, or None for an untyped pointer (void*, an opaque handle, c_void_p, Ptr{Cvoid})
    ("cstring",)           const char* / c_char_p / Cstring
    ("struct", name)       by value; `name` is the HEADER's name of the struct (cf_grid), whatever the mirror calls its twin
    ("array", n, element)
    ("mutable", name)      Julia only: a field whose type is a mutable struct — a reference, which has no C layout
Two types agree by CLASS — pointer, cstring, a scalar class, void — and, where both sides name one, by pointee (`compare_types`).

Layout truth is the host C compiler's: `compile_probe` generates a C99 program from the parsed NAMES (never from the parsed
types), builds it with -std=c99 -pedantic -Wall -Wextra -Werror and reads sizeof, alignment, every offsetof and every
constant from its output.  The parsers account for all the text they are given: a declaration, struct body or parameter
list they cannot parse raises AbiParseError with the line, it is never skipped.

Nothing here touches a file of the repository; planted defects (DEFECTS) are applied to copies in memory."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_PATH = os.path.join(ROOT, "include", "coflux.h")
STUB_PATH = os.path.join(ROOT, "climaocean.jl_amd", "julia", "CoFluxMI355X.jl")
C_FLAGS = ["-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror"]
CXX_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]


class AbiParseError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------- the vocabulary
def scalar(cls):
    return ("scalar", cls)


PTR = ("ptr", None)
SCALAR_SIZE = {"i8": 1, "u8": 1, "char": 1, "i32": 4, "u32": 4, "f32": 4, "i64": 8, "u64": 8, "f64": 8, "usize": 8}


def show(t):
    if t is None:
        return "void"
    if t[0] == "scalar":
        return t[1]
    if t[0] == "ptr":
        return "ptr(%s)" % show(t[1])
    if t[0] == "array":
        return "%s[%d]" % (show(t[2]), t[1])
    if t[0] == "cstring":
        return "cstring"
    return "%s %s" % (t[0], t[1])


def compare_types(want, got, same_scalar=lambda a, b: a == b):
    """`want` is the header's type, `got` a mirror's.  Returns (problem or None, untyped): `untyped` is 1 when the two agree
    only as "a pointer" — the mirror's side is untyped where the header names a pointee."""
    if want[0] == "scalar":
        if got[0] != "scalar" or not same_scalar(want[1], got[1]):
            return "%s where the header has %s" % (show(got), show(want)), 0
        return None, 0
    if want[0] == "cstring":
        if got[0] == "cstring" or got == ("ptr", scalar("u8")) or got == ("ptr", scalar("char")):
            return None, 0
        return "%s where the header has const char*" % show(got), 0
    if want[0] == "ptr":
        if got[0] != "ptr":
            return "%s where the header has %s" % (show(got), show(want)), 0
        if got[1] is None:
            return None, (1 if want[1] is not None else 0)
        if want[1] is None:
            return None, 0                      # a typed view of a void* / an opaque handle: the header does not say
        problem, _ = compare_types(want[1], got[1], same_scalar)
        return (None if problem is None else "pointee: " + problem), 0
    if want[0] == "struct":
        if got != want:
            return "%s where the header has %s" % (show(got), show(want)), 0
        return None, 0
    if want[0] == "array":
        if got[0] != "array" or got[1] != want[1]:
            return "%s where the header has %s" % (show(got), show(want)), 0
        return compare_types(want[2], got[2], same_scalar)
    raise AssertionError(want)


# ---------------------------------------------------------------------------------------------- the header
C_SCALARS = {"int32_t": "i32", "int": "i32", "uint32_t": "u32", "unsigned int": "u32", "unsigned": "u32", "int64_t": "i64",
             "long long": "i64", "uint64_t": "u64", "unsigned long long": "u64", "double": "f64", "float": "f32",
             "size_t": "usize", "uint8_t": "u8", "int8_t": "i8", "char": "char", "void": "void"}
KNOWN_DIRECTIVES = re.compile(r"#\s*(ifndef|ifdef|endif|include|if|else)\b")


def strip_c_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def parse_int(text, constants, line):
    s = text.strip()
    while s.startswith("(") and s.endswith(")"):
        s = s[1:-1].strip()
    m = re.fullmatch(r"([-+]?)\s*(0[xX][0-9a-fA-F]+|\d+)[uUlL]*", s)
    if m:
        return int(m.group(1) + m.group(2), 0)
    if s in constants:
        return constants[s]
    raise AbiParseError("line %d: %r is not an integer constant" % (line, text))


class Header:
    """structs: {name: [(field, type)]} in declaration order; opaque: set of handle types; prototypes: {name: (return type,
    [(parameter, type)])}; constants: {name: int} (#define CF_* integers and enumerators); other_defines: {name: text} — the
    #defines that are not integers (CF_STREAM_LEGACY), accounted for and not compared."""

    def __init__(self, text):
        self.structs, self.opaque, self.prototypes, self.constants, self.other_defines = {}, set(), {}, {}, {}
        self.lines = {}
        code = strip_c_comments(text)
        kept = []
        for n, line in enumerate(code.split("\n"), 1):
            if line.lstrip().startswith("#"):
                self._directive(line.strip(), n)
                kept.append("")
            else:
                kept.append(line)
        self._declarations("\n".join(kept))

    def _directive(self, line, n):
        if line.endswith("\\"):
            raise AbiParseError("line %d: a continued preprocessor line is not parsed: %s" % (n, line))
        m = re.fullmatch(r"#\s*define\s+(\w+)(?:\s+(.*))?", line)
        if m:
            name, value = m.group(1), (m.group(2) or "").strip()
            if "(" in name or value == "":
                if value == "" and not name.startswith("CF_"):
                    return                                      # the include guard
                raise AbiParseError("line %d: #define %s has no value" % (n, name))
            try:
                self.constants[name] = parse_int(value, self.constants, n)
            except AbiParseError:
                self.other_defines[name] = value
            self.lines[name] = n
            return
        if not KNOWN_DIRECTIVES.match(line):
            raise AbiParseError("line %d: unknown preprocessor line: %s" % (n, line))

    def _declarations(self, code):
        code, n_extern = re.subn(r'extern\s+"C"\s*\{', lambda m: " " * len(m.group(0)), code)
        depth, start, i, open_extern = 0, 0, 0, n_extern
        while i < len(code):
            ch = code[i]
            if ch in "{(":
                depth += 1
            elif ch in ")":
                depth -= 1
            elif ch == "}":
                if depth == 0 and open_extern and not code[start:i].strip():
                    open_extern -= 1
                    start = i + 1
                else:
                    depth -= 1
            elif ch == ";" and depth == 0:
                lead = len(code[start:i]) - len(code[start:i].lstrip())
                self._statement(code[start:i], code.count("\n", 0, start + lead) + 1)
                start = i + 1
            if depth < 0:
                raise AbiParseError("line %d: unbalanced bracket" % (code.count("\n", 0, i) + 1))
            i += 1
        if code[start:].strip() or depth or open_extern:
            raise AbiParseError("line %d: text after the last declaration: %r" % (code.count("\n", 0, start) + 1, code[start:].strip()[:60]))

    def _statement(self, text, line):
        s = text.strip()
        if not s:
            return
        m = re.fullmatch(r"typedef\s+struct\s+(\w+)\s+(\w+)", s)
        if m:
            if m.group(1) != m.group(2):
                raise AbiParseError("line %d: opaque typedef renames %s to %s" % (line, m.group(1), m.group(2)))
            self.opaque.add(m.group(2))
            self.lines[m.group(2)] = line
            return
        m = re.fullmatch(r"typedef\s+struct\s*(\w*)\s*\{(.*)\}\s*(\w+)", s, re.S)
        if m:
            tag, body, name = m.groups()
            if tag and tag != name:
                raise AbiParseError("line %d: struct tag %s and typedef name %s differ" % (line, tag, name))
            fields = []
            body_line = line + s[:m.start(2)].count("\n")
            for piece in body.split(";"):
                if piece.strip():
                    fields += self._declarators(piece, body_line, field=True)
                body_line += piece.count("\n")
            if not fields:
                raise AbiParseError("line %d: struct %s has no field" % (line, name))
            if len({f for f, _ in fields}) != len(fields):
                raise AbiParseError("line %d: struct %s names a field twice" % (line, name))
            self.structs[name] = fields
            self.lines[name] = line
            return
        m = re.fullmatch(r"(?:typedef\s+)?enum\s*\w*\s*\{(.*)\}\s*(\w*)", s, re.S)
        if m:
            value = -1
            for piece in m.group(1).split(","):
                if not piece.strip():
                    continue
                e = re.fullmatch(r"\s*(\w+)\s*(?:=\s*(.+?))?\s*", piece, re.S)
                if not e:
                    raise AbiParseError("line %d: enumerator %r" % (line, piece.strip()))
                value = parse_int(e.group(2), self.constants, line) if e.group(2) else value + 1
                self.constants[e.group(1)] = value
                self.lines[e.group(1)] = line
            return
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", s, re.S)
        if m and not s.startswith("typedef"):
            ret, name, params = m.groups()
            ret_type = self._declarators(ret + " _", line, field=False)[0][1]
            plist = []
            if params.strip() != "void":
                depth, piece = 0, ""
                for ch in params + ",":
                    if ch == "," and depth == 0:
                        if not piece.strip():
                            raise AbiParseError("line %d: empty parameter of %s" % (line, name))
                        plist += self._declarators(piece, line, field=False)
                        piece = ""
                        continue
                    depth += ch in "(["
                    depth -= ch in ")]"
                    piece += ch
            if name in self.prototypes:
                raise AbiParseError("line %d: %s is declared twice" % (line, name))
            self.prototypes[name] = (ret_type, plist)
            self.lines[name] = line
            return
        raise AbiParseError("line %d: not a declaration this parser knows: %r" % (line, " ".join(s.split())[:80]))

    def _base(self, words, line):
        words = [w for w in words if w != "const"]
        if words[:1] == ["struct"]:
            words = words[1:]
        key = " ".join(words)
        if key in C_SCALARS:
            return scalar(C_SCALARS[key])
        if key in self.structs:
            return ("struct", key)
        if key in self.opaque:
            return ("opaque", key)
        raise AbiParseError("line %d: unknown type %r" % (line, key))

    def _declarators(self, text, line, field):
        """`base declarator[, declarator…]` → [(name, type)].  A parameter list entry has one declarator and its arrays decay."""
        line += text[:len(text) - len(text.lstrip())].count("\n")
        tokens = re.findall(r"\w+|[*\[\],]", text)
        if "".join(tokens) != re.sub(r"\s+", "", text):
            raise AbiParseError("line %d: cannot parse %r" % (line, " ".join(text.split())))
        k, words = 0, []
        while k < len(tokens) and re.fullmatch(r"\w+", tokens[k]) and k + 1 < len(tokens) and tokens[k + 1] not in (",", "["):
            words.append(tokens[k])
            k += 1
        if not words:
            raise AbiParseError("line %d: no type in %r" % (line, " ".join(text.split())))
        is_char = [w for w in words if w != "const"] == ["char"]
        const_base = "const" in words
        base = self._base(words, line)
        out, rest = [], tokens[k:]
        while rest:
            t, stars = base, 0
            while rest and rest[0] in ("*", "const"):
                stars += rest[0] == "*"
                rest = rest[1:]
            if not rest or not re.fullmatch(r"[A-Za-z_]\w*", rest[0]):
                raise AbiParseError("line %d: no name in %r" % (line, " ".join(text.split())))
            name, rest = rest[0], rest[1:]
            for level in range(stars):
                if level == 0 and is_char and const_base:
                    t = ("cstring",)
                elif t[0] == "opaque" or t == scalar("void"):
                    t = PTR
                else:
                    t = ("ptr", t)
            bounds = []
            while rest and rest[0] == "[":
                if len(rest) < 3 or rest[2] != "]":
                    raise AbiParseError("line %d: array bound in %r" % (line, " ".join(text.split())))
                bounds.append(parse_int(rest[1], self.constants, line))
                rest = rest[3:]
            for n in reversed(bounds):
                t = ("array", n, t)
            if bounds and not field:
                t = ("ptr", t[2])
            if t[0] == "opaque" or (t == scalar("void") and (field or name != "_")):
                raise AbiParseError("line %d: %s has an incomplete type" % (line, name))
            out.append((name, t))
            if rest:
                if rest[0] != "," or not field or len(rest) == 1:
                    raise AbiParseError("line %d: cannot parse %r" % (line, " ".join(text.split())))
                rest = rest[1:]
        return out


def parse_header(text=None):
    return Header(open(HEADER_PATH).read() if text is None else text)


# ---------------------------------------------------------------------------------------------- the compiler
def find_compiler(names, rocm_name):
    """The host compiler the way tests/test_exact_sum_cpu.py finds its own, then the clang of a ROCm tree."""
    for name in names:
        path = shutil.which(name)
        if path:
            return path
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for root in roots:
        for sub in ("llvm/bin", "lib/llvm/bin"):
            path = os.path.join(root or "", sub, rocm_name)
            if root and os.path.exists(path):
                return path
    return None


def c_compiler():
    return find_compiler(("cc", "gcc", "clang"), "clang")


def cxx_compiler():
    return find_compiler(("g++", "clang++", "c++"), "clang++")


def probe_source(header):
    """C99 program printing `S struct size align`, `F struct field offset size` and `C constant value`.  _Alignof is C11 and
    the flags are C99: alignment is the offset of a member behind one char."""
    out = ["#include <stddef.h>", "#include <stdio.h>", '#include "coflux.h"']
    for name in header.structs:
        out.append("struct align_of_%s { char c; %s x; };" % (name, name))
    out.append("int main(void) {")
    for name, fields in header.structs.items():
        out.append('    printf("S %s %%lu %%lu\\n", (unsigned long)sizeof(%s), (unsigned long)offsetof(struct align_of_%s, x));' % (name, name, name))
        for f, _t in fields:
            out.append('    printf("F %s %s %%lu %%lu\\n", (unsigned long)offsetof(%s, %s), (unsigned long)sizeof(((%s*)0)->%s));'
                       % (name, f, name, f, name, f))
    for name in header.constants:
        out.append('    printf("C %s %%lld\\n", (long long)(%s));' % (name, name))
    out += ["    return 0;", "}", ""]
    return "\n".join(out)


class CompilerLayout:
    """sizes: {struct: (size, align)}; fields: {struct: [(field, offset, size)]}; constants: {name: int}."""

    def __init__(self, text):
        self.sizes, self.fields, self.constants = {}, {}, {}
        for line in text.splitlines():
            w = line.split()
            if w[0] == "S":
                self.sizes[w[1]] = (int(w[2]), int(w[3]))
                self.fields[w[1]] = []
            elif w[0] == "F":
                self.fields[w[1]].append((w[2], int(w[3]), int(w[4])))
            elif w[0] == "C":
                self.constants[w[1]] = int(w[2])
            else:
                raise AbiParseError("probe output: " + line)


def compile_probe(header, workdir, compiler=None):
    compiler = compiler or c_compiler()
    src, exe = os.path.join(workdir, "abi_probe.c"), os.path.join(workdir, "abi_probe")
    with open(src, "w") as f:
        f.write(probe_source(header))
    build = subprocess.run([compiler] + C_FLAGS + ["-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        raise AssertionError("include/coflux.h does not compile as %s:\n%s" % (" ".join(C_FLAGS), build.stderr))
    run = subprocess.run([exe], capture_output=True, text=True, check=True)
    return CompilerLayout(run.stdout)


def compile_cxx_include(workdir, compiler=None):
    """A translation unit that only includes the header, as C++17.  Returns the compiler's stderr ('' when clean)."""
    compiler = compiler or cxx_compiler()
    src = os.path.join(workdir, "abi_include.cpp")
    with open(src, "w") as f:
        f.write('#include "coflux.h"\nint abi_include_unit(void) { return CF_ABI_VERSION; }\n')
    build = subprocess.run([compiler] + CXX_FLAGS + ["-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(workdir, "abi_include.o")],
                           capture_output=True, text=True)
    return build.stderr if build.returncode != 0 else ""


# ---------------------------------------------------------------------------------------------- name rules
def camel(header_name):
    """cf_flux_params → FluxParams (the ctypes twin); the Julia mirror is Cf + that."""
    assert header_name.startswith("cf_"), header_name
    return "".join(w.capitalize() for w in header_name[3:].split("_"))


# `Cf*` structs of the stub that mirror no header struct of their own name: {stub name: (header struct it lays out as, why)}
JULIA_EXTRA = {
    "CfIceOceanParamsData": ("cf_ice_ocean_params", "the isbits twin of the mutable CfIceOceanParams: as a FIELD (cf_coupled_prepare, "
                             "cf_coupled_step hold the block by value) a mutable struct would be a reference"),
}


# ---------------------------------------------------------------------------------------------- ctypes, from the loaded objects
def ctypes_type(t, struct_names):
    """A ctypes type object → the vocabulary.  `struct_names`: {Structure subclass: header name}."""
    if t is None:
        return scalar("void")
    if t is C.c_void_p:
        return PTR
    if t is C.c_char_p:
        return ("cstring",)
    if isinstance(t, type) and issubclass(t, C.Structure):
        if t not in struct_names:
            raise AbiParseError("ctypes Structure %s mirrors no header struct" % t.__name__)
        return ("struct", struct_names[t])
    if isinstance(t, type) and issubclass(t, C.Array):
        return ("array", t._length_, ctypes_type(t._type_, struct_names))
    if isinstance(t, type) and issubclass(t, C._Pointer):
        inner = ctypes_type(t._type_, struct_names)
        return PTR if inner == scalar("void") else ("ptr", inner)
    if isinstance(t, type) and issubclass(t, C._SimpleCData):
        code, size = t._type_, C.sizeof(t)
        if code in "fd":
            return scalar({4: "f32", 8: "f64"}[size])
        if code in "bhilq":
            return scalar({1: "i8", 4: "i32", 8: "i64"}[size])
        if code in "BHILQ":
            return scalar({1: "u8", 4: "u32", 8: "u64"}[size])
        if code == "c":
            return scalar("char")
        if code in "Pz":
            return PTR if code == "P" else ("cstring",)
    raise AbiParseError("ctypes type %r is outside the vocabulary" % (t,))


def ctypes_same_scalar(want, got):
    """ctypes has no size_t of its own: c_size_t IS the unsigned integer of that width, so usize and u64 are one class there."""
    fold = {"usize": "u64"} if C.sizeof(C.c_size_t) == 8 else {"usize": "u32"}
    return fold.get(want, want) == fold.get(got, got)


class Mirror:
    """One mirror in the vocabulary.  structs: {header name: {"name": the mirror's own name, "size", "align",
    "fields": [(field, type, offset, size)]}}; missing: header structs without a twin; extra: twins without a header struct;
    functions: {symbol: (return type, [types] or None when unset)}; constants: {header constant name: int};
    defects: what the mirror's own text or objects already rule out (a mutable struct as a field)."""

    def __init__(self):
        self.structs, self.missing, self.extra, self.functions, self.constants, self.defects = {}, [], [], {}, {}, []
        self.ccalls, self.extra_layouts, self.struct_names = [], {}, {}


def ctypes_struct(cls, struct_names):
    fields = []
    for entry in cls._fields_:
        d = getattr(cls, entry[0])
        fields.append((entry[0], ctypes_type(entry[1], struct_names), d.offset, d.size))
    return {"name": cls.__name__, "size": C.sizeof(cls), "align": C.alignment(cls), "fields": fields}


def ctypes_mirror(header, abi_module, lib=None):
    m = Mirror()
    classes = {n: v for n, v in vars(abi_module).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    by_twin = {camel(h): h for h in header.structs}
    struct_names = {cls: by_twin[n] for n, cls in classes.items() if n in by_twin}
    m.missing = sorted(h for t, h in by_twin.items() if t not in classes)
    m.extra = sorted(n for n in classes if n not in by_twin)
    m.struct_names = struct_names
    for cls, h in struct_names.items():
        m.structs[h] = ctypes_struct(cls, struct_names)
    for name, value in vars(abi_module).items():
        if isinstance(value, int) and not isinstance(value, bool) and "CF_" + name in header.constants:
            m.constants["CF_" + name] = value
    if lib is not None:
        for name in abi_module.EXPORTED_SYMBOLS:
            fn = getattr(lib, name)
            args = fn.argtypes
            m.functions[name] = (ctypes_type(fn.restype, struct_names),
                                 None if args is None else [ctypes_type(a, struct_names) for a in args])
    return m


# ---------------------------------------------------------------------------------------------- the Julia text
JL_SCALARS = {"Cint": "i32", "Int32": "i32", "Cuint": "u32", "UInt32": "u32", "Int64": "i64", "Clonglong": "i64", "UInt64": "u64",
              "Culonglong": "u64", "Float32": "f32", "Cfloat": "f32", "Float64": "f64", "Cdouble": "f64", "Csize_t": "usize",
              "UInt8": "u8", "Int8": "i8", "Cchar": "char", "Cvoid": "void"}


def strip_jl_comments(text):
    out = []
    for line in text.split("\n"):
        quoted, k = False, 0
        while k < len(line):
            if line[k] == "\\" and quoted:
                k += 1
            elif line[k] == '"':
                quoted = not quoted
            elif line[k] == "#" and not quoted:
                break
            k += 1
        out.append(line[:k])
    return "\n".join(out)


def split_top(text, sep=","):
    """Split at `sep` outside every bracket."""
    parts, depth, piece = [], 0, ""
    for ch in text:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == sep and depth == 0:
            parts.append(piece)
            piece = ""
        else:
            piece += ch
    parts.append(piece)
    return parts


def matching(text, start):
    """Index of the bracket that closes the one at `start`."""
    depth = 0
    for k in range(start, len(text)):
        if text[k] in "([{":
            depth += 1
        elif text[k] in ")]}":
            depth -= 1
            if depth == 0:
                return k
    raise AbiParseError("line %d: unbalanced bracket" % (text.count("\n", 0, start) + 1))


class Stub:
    """raw_structs: {name: (mutable, [(field, type text)], line)}; ccalls: [(symbol, return text, [type texts], n arguments,
    line)]; constants: {name: int}."""

    def __init__(self, text):
        code = strip_jl_comments(text)
        self.raw_structs, self.ccalls, self.constants = {}, [], {}
        for m in re.finditer(r"^[ \t]*(mutable[ \t]+)?struct[ \t]+(\w+)([^\n;]*)", code, re.M):
            name, line = m.group(2), code.count("\n", 0, m.start()) + 1
            end = re.compile(r"\bend\b").search(code, m.end())
            if not end:
                raise AbiParseError("line %d: struct %s never ends" % (line, name))
            if not name.startswith("Cf"):
                continue
            if m.group(3).strip():
                raise AbiParseError("line %d: struct %s: %r after the name" % (line, name, m.group(3).strip()))
            fields = []
            for piece in re.split(r"[;\n]", code[m.end():end.start()]):
                p = piece.strip()
                if not p or re.match(r"%s\s*\(.*\)\s*=" % name, p):      # an inner constructor
                    continue
                f = re.fullmatch(r"(\w+)::(.+)", p)
                if not f:
                    raise AbiParseError("line %d: struct %s: cannot parse %r" % (line, name, p))
                fields.append((f.group(1), f.group(2).strip()))
            if name in self.raw_structs:
                raise AbiParseError("line %d: struct %s is defined twice" % (line, name))
            self.raw_structs[name] = (bool(m.group(1)), fields, line)
        for m in re.finditer(r"\bccall\s*\(", code):
            line = code.count("\n", 0, m.start()) + 1
            close = matching(code, m.end() - 1)
            parts = [p.strip() for p in split_top(code[m.end():close])]
            target = re.fullmatch(r"\(\s*:(\w+)\s*,\s*libcoflux\s*\)", parts[0])
            if not target or len(parts) < 3 or not (parts[2].startswith("(") and matching(parts[2], 0) == len(parts[2]) - 1):
                raise AbiParseError("line %d: cannot parse ccall(%s…" % (line, " ".join(code[m.end():close].split())[:60]))
            tuple_types = [p.strip() for p in split_top(parts[2][1:-1]) if p.strip()]
            self.ccalls.append((target.group(1), parts[1], tuple_types, len(parts) - 3, line))
        for m in re.finditer(r"^[ \t]*const[ \t]+((?:CF_\w+)(?:[ \t]*,[ \t]*CF_\w+)*)[ \t]*=[ \t]*([^\n]*)", code, re.M):
            line = code.count("\n", 0, m.start()) + 1
            names, values = [n.strip() for n in m.group(1).split(",")], [v.strip() for v in split_top(m.group(2))]
            if len(names) != len(values):
                raise AbiParseError("line %d: %d names and %d values" % (line, len(names), len(values)))
            for name, value in zip(names, values):
                v = re.fullmatch(r"(?:(?:Cint|Int32|Int64|UInt32|UInt64|Int|Cuint)\((.+)\)|(.+))", value)
                self.constants[name] = parse_int(v.group(1) or v.group(2), self.constants, line)

    def jl_type(self, text, header_of, where):
        """A Julia type text → the vocabulary.  `header_of`: {stub struct name: header struct name}."""
        t = text.strip()
        if t in JL_SCALARS:
            return scalar(JL_SCALARS[t])
        if t == "Cstring":
            return ("cstring",)
        m = re.fullmatch(r"(?:Ptr|Ref)\{(.*)\}", t)
        if m:
            inner = m.group(1).strip()
            if inner == "Cvoid":
                return PTR
            if inner in self.raw_structs:               # a pointer to a struct, mutable or not, is a pointer to its fields
                if inner not in header_of:
                    raise AbiParseError("%s: %s mirrors no header struct" % (where, inner))
                return ("ptr", ("struct", header_of[inner]))
            return ("ptr", self.jl_type(inner, header_of, where))
        m = re.fullmatch(r"NTuple\{\s*(\d+)\s*,(.*)\}", t)
        if m:
            return ("array", int(m.group(1)), self.jl_type(m.group(2), header_of, where))
        if t in self.raw_structs:
            if self.raw_structs[t][0]:
                return ("mutable", t)
            if t not in header_of:
                raise AbiParseError("%s: %s mirrors no header struct" % (where, t))
            return ("struct", header_of[t])
        raise AbiParseError("%s: Julia type %r is outside the vocabulary" % (where, t))


def julia_layout(t, layouts):
    """(size, align) of a vocabulary type under C layout rules; `layouts`: {header name: {"size", "align"}} of the stub's own
    structs, already laid out."""
    if t[0] == "scalar":
        return SCALAR_SIZE[t[1]], SCALAR_SIZE[t[1]]
    if t[0] in ("ptr", "cstring"):
        return 8, 8
    if t[0] == "array":
        size, align = julia_layout(t[2], layouts)
        return t[1] * size, align
    if t[0] == "struct":
        return layouts[t[1]]["size"], layouts[t[1]]["align"]
    raise AssertionError(t)


def julia_mirror(header, stub):
    m = Mirror()
    header_of = {"Cf" + camel(h): h for h in header.structs}
    m.missing = sorted(h for j, h in header_of.items() if j not in stub.raw_structs)
    header_of = {j: h for j, h in header_of.items() if j in stub.raw_structs}
    alias = dict(header_of)
    for j, (h, _why) in JULIA_EXTRA.items():
        if j in stub.raw_structs:
            alias[j] = h
    m.extra = sorted(j for j in stub.raw_structs if j not in alias)
    pending = {j: stub.raw_structs[j] for j in alias}
    own = {}                                            # {stub name: layout}; nested lookups go by header name
    by_header = {}
    while pending:
        progressed = False
        for j in list(pending):
            _mutable, raw_fields, _line = pending[j]
            fields, offset, align, ready, broken = [], 0, 1, True, False
            for f, text in raw_fields:
                t = stub.jl_type(text, alias, "%s.%s" % (j, f))
                inner = t
                while inner[0] == "array":
                    inner = inner[2]
                if inner[0] == "mutable":
                    m.defects.append("%s.%s: its type %s is a mutable struct — a reference in Julia, not the struct's bytes" % (j, f, inner[1]))
                    broken = True
                    continue
                if inner[0] == "struct" and inner[1] not in by_header:
                    ready = False
                    break
                size, al = julia_layout(t, by_header)
                offset = (offset + al - 1) // al * al
                fields.append((f, t, offset, size))
                offset += size
                align = max(align, al)
            if not ready:
                continue
            layout = {"name": j, "size": (offset + align - 1) // align * align, "align": align, "fields": fields, "broken": broken}
            own[j] = layout
            if j in header_of:
                by_header[header_of[j]] = layout
            del pending[j]
            progressed = True
        if not progressed:
            raise AbiParseError("the stub's structs %s nest in a cycle or in a struct that is missing" % sorted(pending))
    m.structs = {h: own[j] for j, h in header_of.items()}
    m.extra_layouts = {j: own[j] for j in JULIA_EXTRA if j in own}
    m.constants = {n: v for n, v in stub.constants.items()}
    m.ccalls = []
    for symbol, ret, types, n_args, line in stub.ccalls:
        where = "ccall of %s (line %d)" % (symbol, line)
        m.ccalls.append((symbol, stub.jl_type(ret, alias, where), [stub.jl_type(t, alias, where) for t in types], n_args, line))
    return m


def parse_stub(text=None):
    return Stub(open(STUB_PATH).read() if text is None else text)


# ---------------------------------------------------------------------------------------------- the comparisons
def same_scalar_strict(a, b):
    return a == b


def struct_problems(header, layout, mirror, label, same_scalar=same_scalar_strict):
    """Header ↔ compiler ↔ one mirror, every struct.  `layout` is a CompilerLayout or None (no host compiler: names, order and
    types are still compared, offsets and sizes are not)."""
    out = [] + ["%s: %s" % (label, d) for d in mirror.defects]
    for h in mirror.missing:
        out.append("%s: header struct %s has no twin" % (label, h))
    for e in mirror.extra:
        out.append("%s: %s mirrors no header struct" % (label, e))
    for h, fields in header.structs.items():
        if h not in mirror.structs:
            continue
        out += one_struct_problems(h, fields, layout, mirror.structs[h], label, same_scalar)
    return out


def one_struct_problems(h, fields, layout, twin, label, same_scalar=same_scalar_strict):
    out, name = [], "%s %s (%s)" % (label, twin["name"], h)
    want_names, got_names = [f for f, _ in fields], [f for f, *_ in twin["fields"]]
    if twin.get("broken"):
        return out                                      # reported among the mirror's defects; it has no layout to compare
    if want_names != got_names:
        for k, (a, b) in enumerate(zip(want_names, got_names)):
            if a != b:
                out.append("%s: field %d is %s where the header has %s" % (name, k, b, a))
                break
        else:
            out.append("%s: %d fields where the header has %d" % (name, len(got_names), len(want_names)))
        return out
    for (f, t), (_f, got, offset, size) in zip(fields, twin["fields"]):
        problem, _ = compare_types(t, got, same_scalar)
        if problem:
            out.append("%s.%s: %s" % (name, f, problem))
    if layout is not None:
        for (f, c_offset, c_size), (_f, _t, offset, size) in zip(layout.fields[h], twin["fields"]):
            if (c_offset, c_size) != (offset, size):
                out.append("%s.%s: offset %d size %d where the compiler has offset %d size %d" % (name, f, offset, size, c_offset, c_size))
        if layout.sizes[h] != (twin["size"], twin["align"]):
            out.append("%s: size %d align %d where the compiler has size %d align %d" % ((name, twin["size"], twin["align"]) + layout.sizes[h]))
    return out


def signature_problems(name, prototype, ret, args, label, same_scalar=same_scalar_strict):
    """One symbol's return type and argument list against its prototype.  Returns (problems, untyped pointer parameters)."""
    want_ret, params = prototype
    out, untyped = [], 0
    problem, _ = compare_types(want_ret, ret, same_scalar)
    if problem:
        out.append("%s %s: return type: %s" % (label, name, problem))
    if len(args) != len(params):
        out.append("%s %s: %d argument types where the prototype has %d parameters" % (label, name, len(args), len(params)))
        return out, untyped
    for k, ((p, want), got) in enumerate(zip(params, args)):
        problem, u = compare_types(want, got, same_scalar)
        untyped += u
        if problem:
            out.append("%s %s: argument %d (%s): %s" % (label, name, k, p, problem))
    return out, untyped


def ctypes_function_problems(header, mirror):
    out, untyped, checked = [], 0, 0
    for name, (ret, args) in mirror.functions.items():
        if name not in header.prototypes:
            out.append("ctypes %s: no prototype in the header" % name)
            continue
        want_ret, params = header.prototypes[name]
        if args is None:
            if params or want_ret != scalar("i32"):
                out.append("ctypes %s: argtypes is not set" % name)      # only `int f(void)` may stay on ctypes' defaults
                continue
            args = []
        problems, u = signature_problems(name, header.prototypes[name], ret, args, "ctypes", ctypes_same_scalar)
        out += problems
        untyped += u
        checked += len(params)
    for name in header.prototypes:
        if name not in mirror.functions:
            out.append("ctypes: %s is declared in the header and not among the exported symbols" % name)
    return out, untyped, checked


def ccall_problems(header, mirror):
    out, untyped, checked = [], 0, 0
    for symbol, ret, types, n_args, line in mirror.ccalls:
        if symbol not in header.prototypes:
            out.append("ccall %s (line %d): no prototype in the header" % (symbol, line))
            continue
        problems, u = signature_problems(symbol, header.prototypes[symbol], ret, types, "ccall", same_scalar_strict)
        out += ["%s (line %d)" % (p, line) for p in problems]
        untyped += u
        checked += len(types)
        if n_args != len(types):
            out.append("ccall %s (line %d): %d arguments follow a tuple of %d types" % (symbol, line, n_args, len(types)))
    return out, untyped, checked


def constant_problems(header_constants, mirror_constants, label):
    out = []
    for name, value in mirror_constants.items():
        if name not in header_constants:
            out.append("%s: %s is not a constant of the header" % (label, name))
        elif header_constants[name] != value:
            out.append("%s: %s = %d where the header has %d" % (label, name, value, header_constants[name]))
    return out


def julia_extra_problems(header, layout, mirror):
    out = []
    for j, (h, _why) in JULIA_EXTRA.items():
        if j not in mirror.extra_layouts:
            out.append("Julia: %s is listed as a stand-in for %s and is not in the stub" % (j, h))
            continue
        out += one_struct_problems(h, header.structs[h], layout, mirror.extra_layouts[j], "Julia")
    return out


# ---------------------------------------------------------------------------------------------- the whole report, and defects
# Deliberately wrong variants of ONE copy, applied in memory (the stub's text, a throw-away Structure subclass, a copied
# argtypes list): {defect: the words its report must contain — the struct or function and the field or position}
DEFECTS = {
    "julia_fields_swapped": ("CfMonitorDesc", "max_workgroups"),
    "ccall_cint_widened": ("ccall cf_set_option", "argument 1 (option)", "i64 where the header has i32"),
    "ccall_last_type_dropped": ("ccall cf_h2d", "3 argument types where the prototype has 4", "4 arguments follow a tuple of 3"),
    "ccall_device_alloc_returns_cint": ("ccall cf_device_alloc", "return type", "i32 where the header has ptr"),
    "julia_field_is_mutable_struct": ("CfCoupledPrepare.ice_ocean", "CfIceOceanParams is a mutable struct"),
    "ctypes_fields_swapped": ("ctypes MonitorDesc (cf_monitor_desc)", "field 4 is row_length where the header has max_workgroups"),
    "ctypes_cint_widened": ("ctypes cf_set_option", "argument 1 (option)", "i64 where the header has i32"),
    "ctypes_pointee_retyped": ("ctypes cf_regrid_create", "argument 1 (desc)", "struct cf_monitor_desc where the header has struct cf_regrid_desc"),
    "constant_off_by_one": ("Julia: CF_NORMALIZE_EXACT = 3 where the header has 2", "ctypes: CF_NORMALIZE_EXACT = 3 where the header has 2"),
    "twin_removed": ("ctypes: header struct cf_checkpoint_desc has no twin",),
}


def replace_once(text, old, new):
    assert text.count(old) >= 1, old
    k = text.index(old)
    return text[:k] + new + text[k + len(old):]


def defective_stub(text, defect):
    if defect == "julia_fields_swapped":       # two adjacent Int32 of CfMonitorDesc
        return replace_once(text, "max_workgroups::Int32; row_length::Int32\n    entries::NTuple{16, CfMonitorEntry}",
                            "row_length::Int32; max_workgroups::Int32\n    entries::NTuple{16, CfMonitorEntry}")
    if defect == "ccall_cint_widened":
        return replace_once(text, "(:cf_set_option, libcoflux), Cint, (Ptr{Cvoid}, Cint, Cint)", "(:cf_set_option, libcoflux), Cint, (Ptr{Cvoid}, Int64, Cint)")
    if defect == "ccall_last_type_dropped":
        return replace_once(text, "(:cf_h2d, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t)", "(:cf_h2d, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})")
    if defect == "ccall_device_alloc_returns_cint":
        return replace_once(text, "(:cf_device_alloc, libcoflux), Ptr{Cvoid},", "(:cf_device_alloc, libcoflux), Cint,")
    if defect == "julia_field_is_mutable_struct":
        return replace_once(text, "ice_ocean::CfIceOceanParamsData", "ice_ocean::CfIceOceanParams")
    return text


class Report:
    """problems: every disagreement found, one line each; counts: what was compared."""

    def __init__(self):
        self.problems, self.counts, self.undefined = [], {}, {}


def full_report(header, layout, stub_text, abi_module, lib, defect=None):
    """Every comparison of tests/test_abi_conformance.py in one pass.  `layout` may be None (no host compiler) and `lib` may
    be None (signatures of the ctypes mirror are then not compared)."""
    assert defect is None or defect in DEFECTS, defect
    r = Report()
    namespace = abi_module
    if defect == "twin_removed":
        import types
        namespace = types.SimpleNamespace(**{k: v for k, v in vars(abi_module).items() if k != "CheckpointDesc"})
    ct = ctypes_mirror(header, namespace, None if defect == "twin_removed" else lib)
    vp = C.c_void_p
    if defect == "ctypes_fields_swapped":
        fields = list(abi_module.MonitorDesc._fields_)
        fields[4], fields[5] = fields[5], fields[4]
        ct.structs["cf_monitor_desc"] = ctypes_struct(type("MonitorDesc", (C.Structure,), {"_fields_": fields}), ct.struct_names)
    if defect == "ctypes_cint_widened":
        args = list(lib.cf_set_option.argtypes)
        assert args[1] is C.c_int
        args[1] = C.c_longlong
        ct.functions["cf_set_option"] = (ct.functions["cf_set_option"][0], [ctypes_type(a, ct.struct_names) for a in args])
    if defect == "ctypes_pointee_retyped":
        args = [vp, C.POINTER(abi_module.MonitorDesc), C.POINTER(vp)]
        ct.functions["cf_regrid_create"] = (ct.functions["cf_regrid_create"][0], [ctypes_type(a, ct.struct_names) for a in args])
    jl = julia_mirror(header, parse_stub(defective_stub(stub_text, defect)))
    if defect == "constant_off_by_one":
        ct.constants = dict(ct.constants, CF_NORMALIZE_EXACT=ct.constants["CF_NORMALIZE_EXACT"] + 1)
        jl.constants = dict(jl.constants, CF_NORMALIZE_EXACT=jl.constants["CF_NORMALIZE_EXACT"] + 1)

    r.problems += struct_problems(header, layout, ct, "ctypes", ctypes_same_scalar)
    r.problems += struct_problems(header, layout, jl, "Julia")
    r.problems += julia_extra_problems(header, layout, jl)
    problems, ct_untyped, ct_params = ctypes_function_problems(header, ct) if ct.functions else ([], 0, 0)
    r.problems += problems
    problems, jl_untyped, jl_params = ccall_problems(header, jl)
    r.problems += problems
    truth = dict(header.constants)
    if layout is not None:
        for name, value in header.constants.items():
            if layout.constants.get(name) != value:
                r.problems.append("header: the parser reads %s = %d, the compiler %r" % (name, value, layout.constants.get(name)))
    r.problems += constant_problems(truth, ct.constants, "ctypes")
    r.problems += constant_problems(truth, jl.constants, "Julia")
    r.undefined = {"ctypes": sorted(set(truth) - set(ct.constants)), "Julia": sorted(set(truth) - set(jl.constants))}
    r.counts = {"structs": len(header.structs), "fields": sum(len(f) for f in header.structs.values()),
                "prototypes": len(header.prototypes), "constants": len(truth), "ccalls": len(jl.ccalls),
                "ctypes structs": len(ct.structs), "Julia structs": len(jl.structs) + len(jl.extra_layouts),
                "ctypes parameters": ct_params, "ctypes parameters checked only as a pointer": ct_untyped,
                "ccall parameters": jl_params, "ccall parameters checked only as a pointer": jl_untyped,
                "ctypes constants compared": len(ct.constants), "ctypes constants undefined": len(r.undefined["ctypes"]),
                "Julia constants compared": len(jl.constants), "Julia constants undefined": len(r.undefined["Julia"])}
    return r
