"""One signature per entry point, two statements of it: a header of include/ and the table of its _lib.Abi.  The parser and the two
checks every *_host test file runs on its own header, with its own maps of the C types the header may use."""
import ctypes as C
import os
import re

from gaussianprediction_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTYPES = {"int": C.c_int32, "int64_t": C.c_int64, "const char*": C.c_char_p}


def header_text(name):
    """include/`name` without its comments (the #define lines stay: the tests read constants from them)."""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def header_prototypes(name):
    """{function: (return type, [parameter type])} of include/`name`, types as text without `const` and the parameter name."""
    hdr = re.sub(r"^\s*#.*$", "", header_text(name), flags=re.M)
    hdr = re.sub(r"typedef struct \w*\s*\{.*?\}\s*\w+\s*;", "", hdr, flags=re.S)
    hdr = re.sub(r"enum\s*\{.*?\}\s*;", "", hdr, flags=re.S)
    protos = {}
    for ret, fn, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(gp_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", hdr):
        assert fn not in protos, fn
        params = " ".join(params.split())
        plist = [] if params in ("", "void") else [re.sub(r"\s*\w+$", "", p.strip()) for p in params.split(",")]
        protos[fn] = (" ".join(ret.split()), [" ".join(t.replace("const", " ").replace("*", " * ").split()) for t in plist])
    return protos


def check_table(abi, count, scalars, pointees, structs={}):
    """abi.prototypes is what the header declares: the same `count` names, every restype, every argument count, and per argument the
    class the binding's rules give its C type -- POINTER(the struct) for a pointer to a struct of `structs` ({C name: ctypes class}),
    _lib.Ptr for any other pointer, whose pointee must be in `pointees`, and scalars[type] otherwise.  Returns the parsed header."""
    protos, table = header_prototypes(abi.header), abi.prototypes
    assert set(protos) == set(table), (abi.header, set(protos) ^ set(table))
    assert len(protos) == len(table) == count, (abi.header, len(protos))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is RESTYPES[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for k, (ctype, cls) in enumerate(zip(params, argtypes)):
            base = ctype.split("*")[0].strip()
            if "*" not in ctype:
                assert cls is scalars[ctype], (name, k, ctype, cls)
            elif base in structs:
                assert ctype == base + " *" and cls is C.POINTER(structs[base]), (name, k, ctype, cls)      # (POINTER(X) is cached)
            else:
                assert base in pointees and cls is _lib.Ptr, (name, k, ctype, cls)
    return protos


def check_applied(abi):
    """abi.lib() is the one handle, of the version the binding is written against, with the table on every function."""
    l = abi.lib()
    assert l is _lib.lib()
    assert int(getattr(l, abi.version_fn)()) == abi.version
    for name, (restype, argtypes) in abi.prototypes.items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    return l
