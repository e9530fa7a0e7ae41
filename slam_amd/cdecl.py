"""Reads the C-ABI headers of include/ into ctypes: integer #defines, Structure classes and every prototype's
restype / argtypes, so that slam_amd/api.py restates none of them.  It loads no library.

The dialect is what those headers use: comments, #define NAME <integer>, `typedef void *X;`, `typedef struct s s_t;`,
`typedef struct [tag] { ... } name;`, function-pointer typedefs and prototypes.  Anything else raises CDeclError naming
the text: a declaration the reader does not know must stop lib(), not go unbound.
"""
import ctypes as C
import keyword
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t, "long": C.c_long, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "char": C.c_char}
SCALARS.update(("%sint%d_t" % (u, n), getattr(C, "c_%sint%d" % (u, n))) for u in ("", "u") for n in (8, 16, 32, 64))

_INT = r"([-+]?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*"


class CDeclError(ValueError):
    pass


def _py(name):
    return name + "_" if keyword.iskeyword(name) else name


class Header:
    """defines: name -> int; structs: C name -> Structure class; functions: name -> (restype, argtypes);
    callbacks: function-pointer typedef name -> CFUNCTYPE class.  read() adds one header to them."""

    def __init__(self):
        self.defines, self.structs, self.functions, self.callbacks = {}, {}, {}, {}
        self.pointees = {"void"}      # opaque struct types: only ever pointed to
        self.handles = set()          # typedef void *X

    def read(self, name):
        """Adds include/<name>; returns the names of the functions it declares, in order."""
        with open(os.path.join(INCLUDE, name)) as f:
            return self.parse(f.read())

    def parse(self, text):
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        text = re.sub(r"^\s*#\s*ifdef\s+__cplusplus\b.*?^\s*#\s*endif\b[^\n]*", " ", text, flags=re.S | re.M)
        code = []
        for line in text.splitlines():
            if not line.lstrip().startswith("#"):
                code.append(line)
                continue
            m = re.match(r"\s*#\s*define\s+(\w+)\s+%s\s*$" % _INT, line)
            if m:
                self.defines[m.group(1)] = int(m.group(2), 0)
            elif not re.match(r"\s*#\s*(ifndef\s+\w+|define\s+\w+|endif|include\s+[<\"][\w./]+[>\"])\s*$", line):
                raise CDeclError("unknown preprocessor line: %r" % line.strip())
        names, depth, start, text = [], 0, 0, " ".join(code)
        for i, ch in enumerate(text):
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                names += self._statement(" ".join(text[start:i].split()))
                start = i + 1
        if text[start:].strip():
            raise CDeclError("unterminated declaration: %r" % text[start:].strip())
        return names

    def _statement(self, s):
        m = re.fullmatch(r"typedef void \*(\w+)", s)
        if m:
            self.handles.add(m.group(1))
            return []
        m = re.fullmatch(r"typedef struct (\w+) (\w+)", s)
        if m:
            self.pointees.add(m.group(2))
            return []
        m = re.fullmatch(r"typedef struct (?:\w+ )?\{(.*)\} ?(\w+)", s)
        if m:
            fields = [f for decl in m.group(1).split(";") if decl.strip() for f in self._fields(decl.strip(), m.group(2))]
            self.structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
            return []
        m = re.fullmatch(r"typedef (\w[\w ]*?[ *]+)\(\*(\w+)\)\((.*)\)", s)
        if m:
            self.callbacks[m.group(2)] = C.CFUNCTYPE(self._ret(m.group(1), s), *self._params(m.group(3), s, True))
            return []
        m = re.fullmatch(r"(\w[\w ]*?[ *]+)(slam_\w+) ?\((.*)\)", s)
        if m:
            self.functions[m.group(2)] = (self._ret(m.group(1), s), self._params(m.group(3), s))
            return [m.group(2)]
        raise CDeclError("unknown declaration: %r" % s)

    def _fields(self, decl, struct):
        m = re.fullmatch(r"((?:\w+ )+?)(\w+(?: ?\[\w+\])?(?: ?, ?\w+(?: ?\[\w+\])?)*)", decl)
        base = m and m.group(1).strip()
        ctype = SCALARS.get(base) or self.structs.get(base)
        if ctype is None:
            raise CDeclError("struct %s: unknown field type in %r" % (struct, decl))
        for d in m.group(2).split(","):
            name, _, bound = d.strip().rstrip("]").partition("[")
            if bound:
                bound = bound.strip()
                n = int(bound, 0) if re.fullmatch(_INT, bound) else self.defines.get(bound)
                if n is None:
                    raise CDeclError("struct %s: array bound %r of %r is neither a literal nor a defined constant"
                                     % (struct, bound, decl))
                yield _py(name.strip()), ctype * n
            else:
                yield _py(name.strip()), ctype

    def _type(self, decl, where, named):
        """(base type, pointer depth) of `const T *name`, `T name[N]`, `T`: an array counts as one pointer level"""
        words = re.sub(r"\bconst\b|\*|\[\w*\]", " ", decl).split()
        if named and len(words) > 1 and " ".join(words) not in SCALARS:
            words = words[:-1]
        base = " ".join(words)
        known = base in SCALARS or base in self.pointees or base in self.handles or base in self.structs or base in self.callbacks
        if not known or not re.fullmatch(r"[\w *]+(\[\w*\])?", decl.strip()):
            raise CDeclError("unknown type in %r of %r" % (decl.strip(), where))
        return base, decl.count("*") + decl.count("[")

    def _params(self, params, where, callback=False):
        """callback: Python receives these arguments, so a pointer to a scalar keeps its type there (it arrives as
        something np.ctypeslib.as_array can read); Python only passes the others, and c_void_p takes every form it passes"""
        if params.strip() == "void":
            return []
        out = []
        for decl in params.split(","):
            base, depth = self._type(decl, where, True)
            if depth == 0:
                if base in SCALARS:
                    out.append(SCALARS[base])
                elif base in self.handles:
                    out.append(C.c_void_p)
                elif base in self.callbacks:
                    out.append(self.callbacks[base])
                else:
                    raise CDeclError("%r of %r is passed by value" % (decl.strip(), where))
            elif depth == 1 and base == "char" and "[" not in decl:
                out.append(C.c_char_p)
            elif depth == 1 and base in self.structs:
                out.append(C.POINTER(self.structs[base]))
            elif depth == 1 and callback and base in SCALARS:
                out.append(C.POINTER(SCALARS[base]))
            else:
                out.append(C.c_void_p)
        return out

    def _ret(self, decl, where):
        base, depth = self._type(decl, where, False)
        if (base, depth) == ("void", 0):
            return None
        if (base, depth) == ("char", 1):
            return C.c_char_p
        if depth or base not in SCALARS:
            raise CDeclError("unknown return type %r of %r" % (decl.strip(), where))
        return SCALARS[base]

    def bind(self, library, names):
        """Sets restype and argtypes on every one of `names` in a loaded library."""
        for n in names:
            f = getattr(library, n)
            f.restype, f.argtypes = self.functions[n]
