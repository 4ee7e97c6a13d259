"""A small reader of include/dmp_hip.h for tests/test_lib_abi.py: the functions, structs and numeric ``#define``s the header
declares, mapped to the ctypes types the binding (dualmessagepassing_amd/_abi.py) has to use for them.  Test-side only: the
product binds through its explicit table, never through this reading of C.  Anything it cannot read is an error."""
import ctypes
import re

SCALARS = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8,
    "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
    "double": ctypes.c_double,
}
POINTEES = set(SCALARS) | {"void", "char"}      # what a plain data pointer (-> c_void_p) may point to
_IDENT = r"[A-Za-z_]\w*"


class HeaderError(ValueError):
    pass


class Header:
    """``defines``: name -> int; ``structs``: name -> [(field, base type, is pointer, array length or None)] in order;
    ``functions``: name -> ((base, is pointer), [(arg name, base, is pointer)])."""

    def __init__(self, text):
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        if "//" in text or "/*" in text:
            raise HeaderError("comment syntax the reader does not know")
        self.defines = {}
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(%s)[ \t]+\(?(-?\d+)\)?[ \t]*$" % _IDENT, text, flags=re.M):
            self.defines[m.group(1)] = int(m.group(2))
        text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
        text, n = re.subn(r'extern\s+"C"\s*\{', "", text)
        if n != 1:
            raise HeaderError('expected one extern "C" block')
        self.structs = {}

        def take_struct(m):
            if m.group(2) in self.structs:
                raise HeaderError("struct %s declared twice" % m.group(2))
            self.structs[m.group(2)] = self._fields(m.group(2), m.group(1))
            return ""
        text = re.sub(r"typedef\s+struct\s*\{([^{}]*)\}\s*(%s)\s*;" % _IDENT, take_struct, text)
        text, n = re.subn(r"\}\s*$", "", text.rstrip())       # the closing brace of extern "C"
        if n != 1 or "{" in text or "}" in text or "typedef" in text or "struct" in text:
            raise HeaderError("braces / typedefs the reader does not know")
        self.functions = {}
        *decls, rest = text.split(";")
        if rest.strip():
            raise HeaderError("declaration without its semicolon: %r" % rest.strip())
        for decl in decls:
            decl = " ".join(decl.split())
            if not decl:
                continue
            m = re.fullmatch(r"(.+?)\b(%s) ?\((.*)\)" % _IDENT, decl)
            if m is None:
                raise HeaderError("not a function declaration: %r" % decl)
            name = m.group(2)
            if name in self.functions:
                raise HeaderError("function %s declared twice" % name)
            args = [] if m.group(3).strip() == "void" else [self._arg(name, a) for a in m.group(3).split(",")]
            self.functions[name] = (self._type(name, m.group(1), named=False)[1:], args)

    def _type(self, where, text, named=True):
        """'const float *X' -> ('X', 'float', True)."""
        toks = re.findall(r"%s|\*" % _IDENT, text)
        if "".join(toks) != re.sub(r"\s+", "", text):
            raise HeaderError("%s: cannot read %r" % (where, text))
        toks = [t for t in toks if t != "const"]
        name = toks.pop() if named else None
        stars = toks.count("*")
        base = [t for t in toks if t != "*"]
        if len(base) != 1 or (named and (name == "*" or name in SCALARS)) or (stars > 1 and base[0] in self.structs):
            raise HeaderError("%s: cannot read %r" % (where, text))
        if not (base[0] == "void" and not named):       # a void return
            self._known(where, base[0], stars > 0)
        return name, base[0], stars > 0                  # an array of device pointers is a data pointer as well

    def _known(self, where, base, pointer):
        ok = (base in POINTEES or base in self.structs) if pointer else (base in SCALARS or base in self.structs)
        if not ok:
            raise HeaderError("%s: unknown type %r" % (where, base + (" *" if pointer else "")))

    def _arg(self, fn, text):
        return self._type(fn, text)

    def _fields(self, struct, body):
        out = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            m = re.fullmatch(r"((?:const )?%s) ?(.+)" % _IDENT, decl)
            if m is None:
                raise HeaderError("%s: cannot read field %r" % (struct, decl))
            base = m.group(1).replace("const ", "")
            for d in m.group(2).split(","):
                dm = re.fullmatch(r"\s*(\*?)\s*(%s)\s*(?:\[\s*(\w+)\s*\])?\s*" % _IDENT, d)
                if dm is None:
                    raise HeaderError("%s: cannot read declarator %r of %r" % (struct, d, decl))
                length = dm.group(3)
                if length is not None:
                    if not length.isdigit() and length not in self.defines:
                        raise HeaderError("%s: array length %r is no #define of the header" % (struct, length))
                    length = int(length) if length.isdigit() else self.defines[length]
                self._known(struct, base, bool(dm.group(1)))
                out.append((dm.group(2), base, bool(dm.group(1)), length))
        if not out:
            raise HeaderError("%s: no fields" % struct)
        return out

    # ---- the ctypes image of the declarations; ``abi`` is the module that holds the struct classes
    def ctype(self, abi, base, pointer, ret=False):
        if pointer:
            if base in self.structs:
                return ctypes.POINTER(getattr(abi, base))
            return ctypes.c_char_p if (ret and base == "char") else ctypes.c_void_p
        if base == "void" and ret:
            return None
        return getattr(abi, base) if base in self.structs else SCALARS[base]

    def signature(self, abi, name):
        (rb, rp), args = self.functions[name]
        return self.ctype(abi, rb, rp, ret=True), [self.ctype(abi, b, p) for _, b, p in args]

    def fields(self, abi, name):
        return [(f, self.ctype(abi, b, p) if n is None else self.ctype(abi, b, p) * n) for f, b, p, n in self.structs[name]]


def read(path):
    with open(path) as f:
        return Header(f.read())
