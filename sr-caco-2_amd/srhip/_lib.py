"""ctypes binding of libsrhip.so (the C-ABI declared in include/srhip.h).

The library is the product: there is no CPU or PyTorch fallback.  If it is
missing or fails to load, importing this module raises."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRHIP_LIB: another build of the same library (same-box A/B of two builds, tools/ab_lib.sh)
LIB_PATH = os.environ.get("SRHIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libsrhip.so")

HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "srhip.h")
_CT = {"p": ctypes.c_void_p, "l": ctypes.c_long, "i": ctypes.c_int, "u": ctypes.c_uint,
       "f": ctypes.c_float, "d": ctypes.c_double}
_BASE = {"long": "l", "int": "i", "unsigned": "u", "float": "f", "double": "d"}


def _header_text(path=HEADER):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def parse_header(path=HEADER):
    """include/srhip.h is the single source of truth: returns
    {name: (return_code, arg_codes)} with p pointer, l long, i int, u unsigned int,
    f float, d double, s const char*."""
    text = _header_text(path)
    protos = {}
    for m in re.finditer(r"(const char\*|int|long)\s+(srhip_\w+)\s*\(([^)]*)\)\s*;", text):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        codes = ""
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    codes += "p"
                else:
                    codes += _BASE[a.split()[0]]
        protos[name] = ({"const char*": "s", "int": "i", "long": "l"}[ret], codes)
    return protos


_DECLARATOR = re.compile(r"([\w\s]*?)([\s*]*)\b(\w+)\s*(?:\[\s*(\d+)\s*\])?")


def parse_structs(text=None):
    """{C name: ctypes.Structure subclass} of every ``typedef struct [tag] { ... } name;`` of the header (or of ``text``):
    any ``*`` is a c_void_p, int / long / unsigned / float / double as in _CT, ``name[N]`` an array, the declarators of a comma
    list share the base type but not the ``*``.  Anything else (another base type, a nested struct, a bit-field, a function
    pointer) raises with the struct and the declaration: a layout is never guessed."""
    text = _header_text() if text is None else re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{", text):
        end, depth = m.end(), 1
        while depth:        # the brace that closes the struct, past any nested ones
            depth += {"{": 1, "}": -1}.get(text[end], 0)
            end += 1
        name = re.match(r"\s*(\w+)\s*;", text[end:]).group(1)
        body = text[m.end():end - 1]

        def refuse(decl):
            return ValueError(f"struct {name}: cannot take the layout of {' '.join(decl.split())!r}")
        if "{" in body:
            raise refuse(body)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base = None
            for item in decl.split(","):
                d = _DECLARATOR.fullmatch(item.strip())
                words = d and [w for w in d.group(1).split() if w != "const"]
                if not d or (base is None) != bool(words):
                    raise refuse(decl)
                base = " ".join(words) if base is None else base
                if "*" not in d.group(2) and base not in _BASE:
                    raise refuse(decl)
                ct = ctypes.c_void_p if "*" in d.group(2) else _CT[_BASE[base]]
                fields.append((d.group(3), ct * int(d.group(4)) if d.group(4) else ct))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    return structs


_STRUCTS = parse_structs()


def struct(name):
    """the ctypes mirror of a struct of include/srhip.h, by its C name"""
    return _STRUCTS[name]


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"libsrhip.so not found at {LIB_PATH}: build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` or "
            f"`make -C sr-caco-2_amd/csrc` (hipcc, --offload-arch=gfx950). "
            f"There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (ret, codes) in parse_header().items():
        fn = getattr(lib, name)           # AttributeError if a symbol is missing
        fn.restype = {"s": ctypes.c_char_p, "i": ctypes.c_int, "l": ctypes.c_long}[ret]
        fn.argtypes = [_CT[c] for c in codes]
    return lib


lib = _load()


class SrhipError(RuntimeError):
    pass


def call(name, *args):
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise SrhipError(f"{name} failed ({rc}): {lib.srhip_last_error().decode()}")
