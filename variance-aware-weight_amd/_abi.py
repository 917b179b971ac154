"""What include/vaw_hip.h declares, read from the header itself: functions, structs, enums and integer #defines.  _lib.py builds
the whole ctypes binding from this, so an entry point is its declaration in the header and its definition in csrc/, nothing else.

This reads the plain-C subset the header is written in, not C.  It is strict: once comments, the include guard, #include, the
extern "C" bracket and `typedef void* vaw_stream;` are gone, all that is left must be declarations of the four forms below over
types it knows; anything else raises AbiError with the header line.  Nothing is skipped."""
import os
import re
from collections import namedtuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaw_hip.h")

Type = namedtuple("Type", "base pointer")                 # `const` says nothing about the ABI and is dropped
Function = namedtuple("Function", "ret params")           # params: [(Type, name)]
Header = namedtuple("Header", "functions structs enums defines")
# functions: name -> Function; structs: name -> [(field, Type)]; enums: name -> {enumerator: value}; defines: name -> int

BUILTIN_TYPES = ("void", "char", "int", "int32_t", "int64_t", "uint8_t", "float", "double", "vaw_stream")


class AbiError(ValueError):
    pass


_CPLUSPLUS = re.compile(r'#ifdef __cplusplus\n(?:extern "C" \{|\})\n#endif')
_PREPROCESSOR = re.compile(r"#\s*(?:ifndef\s+\w+|define\s+\w+|include\s*<[\w./]+>|endif)$")          # the guard and <stdint.h>
_DEFINE = re.compile(r"#\s*define\s+(\w+)\s+(-?\d+)$")
_BLANKS = re.compile(r"\s*")
_DECLARATION = re.compile(r"""(?:
      (?P<stream>typedef\s+void\s*\*\s*vaw_stream)
    | typedef\s+enum\s*\{(?P<enumerators>[^{};]*)\}\s*(?P<enum>\w+)
    | typedef\s+struct\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)
    | (?P<ret>[\w\s*]+?)\b(?P<function>\w+)\s*\((?P<params>[^(){};]*)\)
    )\s*;""", re.X)
_DECLARATOR = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)$")
_ENUMERATOR = re.compile(r"(\w+)\s*=\s*(-?\d+)$")


def parse(text, where="include/vaw_hip.h"):
    """-> Header of the declarations in `text`; AbiError (with the line) for anything that is not one."""
    def fail(pos, what):
        raise AbiError(f"{where}:{text.count(chr(10), 0, pos) + 1}: {what}")

    # comments become blanks of the same shape, so a position in `code` is the same position in `text`
    blank = lambda m: re.sub(r"[^\n]", " ", m.group(0))
    code = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    code = _CPLUSPLUS.sub(blank, code)
    header = Header({}, {}, {}, {})
    lines, pos = code.split("\n"), 0
    for i, line in enumerate(lines):
        s = line.strip()
        if s.startswith("#"):
            d = _DEFINE.match(s)
            if d:
                header.defines[d.group(1)] = int(d.group(2))
            elif not _PREPROCESSOR.match(s):
                fail(pos, f"unrecognised preprocessor line {s!r}")
            lines[i] = " " * len(line)
        pos += len(line) + 1
    code = "\n".join(lines)

    def known(base, pos):
        if base not in BUILTIN_TYPES and base not in header.enums and base not in header.structs:
            fail(pos, f"unknown type {base!r}")
        return base

    def declarators(decl, pos, many):
        """`const float* x` -> [(Type('float', True), 'x')]; with `many`, `int a, b` -> two entries (not for pointers)"""
        m = _DECLARATOR.match(" ".join(decl.split()))
        names = m.group(3).replace(" ", "").split(",") if m else []
        if not m or (len(names) > 1 and (not many or m.group(2))):
            fail(pos, f"unrecognised declarator {decl.strip()!r}")
        return [(Type(known(m.group(1), pos), bool(m.group(2))), n) for n in names]

    pos = len(code) - len(code.lstrip())
    while pos < len(code):
        m = _DECLARATION.match(code, pos)
        if not m:
            fail(pos, f"unrecognised construct {' '.join(code[pos:pos + 200].split(';')[0].split())[:80]!r}")
        at, name = m.start(), m.group("enum") or m.group("struct") or m.group("function")
        if name and any(name in d for d in header[:3]):
            fail(at, f"{name} is declared twice")
        if m.group("enum"):
            values = {}
            for e in m.group("enumerators").split(","):
                em = _ENUMERATOR.match(e.strip())
                if not em or em.group(1) in values:
                    fail(at, f"enumerator {e.strip()!r} of {name} is not `NAME = <int>`")
                values[em.group(1)] = int(em.group(2))
            header.enums[name] = values
        elif m.group("struct"):
            body = m.group("fields")
            if body.strip() and not body.rstrip().endswith(";"):
                fail(at, f"field list of {name} does not end in `;`")
            header.structs[name] = [(n, t) for f in body.split(";")[:-1] for t, n in declarators(f, at, many=True)]
        elif m.group("function"):
            ret = re.match(r"(?:const\s+)?(\w+)\s*(\*?)$", " ".join(m.group("ret").split()))
            if not ret:
                fail(at, f"unrecognised return type {m.group('ret').strip()!r} of {name}")
            params = m.group("params").strip()
            header.functions[name] = Function(Type(known(ret.group(1), at), bool(ret.group(2))),
                                              [] if params == "void" else [d for p in params.split(",") for d in declarators(p, at, many=False)])
        pos = _BLANKS.match(code, m.end()).end()
    return header


with open(HEADER_PATH) as _f:
    HEADER = parse(_f.read())
