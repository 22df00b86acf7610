"""ctypes binding of the C-ABI kernel library declared in include/fsv2v.h.

The product path loads ``libfsv2v_hip.so`` (gfx950 code objects) and refuses to work without it: there is no
CPU fallback.  The only other library this module will ever load is the SIMT-emulated build of the *same* kernel
sources, and only when the test-suite asks for it explicitly with ``FSV2V_EMU=1`` (see tests/emu/hip_emu.h).
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_is_emu = False


class FsvError(RuntimeError):
    pass


# ---- the binding is read from include/fsv2v.h: to add an entry point, declare it there and define it in csrc/ ----------------
HEADER = os.path.join(os.path.dirname(_HERE), "include", "fsv2v.h")
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
# the only renames: a member that is a Python keyword, and the class names the descriptor structs have always had in conv.py / hconv.py
_PY_NAMES = {"in": "inp", "fsv_conv_desc": "ConvDesc", "fsv_wgrad_desc": "WgradDesc", "fsv_hconv_desc": "HConvDesc"}


def _declarator(text, where):
    """`const float* in` / `int ty[16]` / `ty[16]` -> (ctypes type or None when the text names no type, name, array length or 0)"""
    m = re.fullmatch(r"\s*(.*?)\s*\b(\w+)\s*(?:\[(\d+)\])?\s*", text, re.S)
    if not m:
        raise FsvError("include/fsv2v.h: cannot read `%s` in %s" % (text.strip(), where))
    base = " ".join(m.group(1).replace("*", " * ").split())
    base = re.sub(r"\bconst ", "", base)
    if not base:
        ctype = None
    elif base.endswith("*") or base == "fsv_stream_t":
        ctype = ctypes.c_void_p
    elif base in _SCALARS:
        ctype = _SCALARS[base]
    else:
        raise FsvError("include/fsv2v.h: no ctypes type for `%s` in %s" % (text.strip(), where))
    return ctype, m.group(2), int(m.group(3) or 0)


def parse_header(path=HEADER):
    """-> (name -> argtypes of every `int fsv_*(...);`, class name -> ctypes.Structure of every `typedef struct`, enumerator -> value).
    Raises FsvError on anything it does not understand: it never guesses a type."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    enums = {}
    for body in re.findall(r"\benum\s+\w+\s*\{(.*?)\}", text, re.S):
        for item in body.split(","):
            name, value = item.split("=")
            enums[name.strip()] = int(value)
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        fields = []
        for stmt in filter(str.strip, body.split(";")):          # `int N, H;` / `int ty[16], tx[16];`: one type, several members
            members = stmt.split(",")
            ctype = _declarator(members[0], name)[0]
            if ctype is None or (ctype is ctypes.c_void_p and len(members) > 1):
                raise FsvError("include/fsv2v.h: cannot read `%s` in %s" % (stmt.strip(), name))
            for member in members:
                _, field, count = _declarator(member, name)
                fields.append((_PY_NAMES.get(field, field), ctype * count if count else ctype))
        pyname = _PY_NAMES.get(name, name)
        structs[pyname] = type(pyname, (ctypes.Structure,), {"_fields_": fields, "__doc__": "include/fsv2v.h " + name})
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    sigs = {}
    for ret, name, params in re.findall(r"([\w \t*]*?)\b(fsv_\w+)\s*\(([^()]*)\)\s*;", text):
        if ret.strip() != "int" or name in sigs:
            raise FsvError("include/fsv2v.h: `%s %s(...)` is not an int-returning entry point declared once" % (ret.strip(), name))
        sigs[name] = [] if params.strip() == "void" else [_declarator(p, name)[0] for p in params.split(",")]
        if None in sigs[name]:
            raise FsvError("include/fsv2v.h: a parameter of %s has no type" % name)
    if len(sigs) != len(re.findall(r"\bfsv_\w+\s*\(", text)):
        raise FsvError("include/fsv2v.h: a declaration was not understood")
    return sigs, structs, enums


# _SIGS: name -> argtypes (all functions return int status; 0 == FSV_OK)
_SIGS, STRUCTS, ENUMS = parse_header()


def emu_requested():
    return os.environ.get("FSV2V_EMU", "0") == "1"


def get_lib():
    global _lib, _is_emu
    if _lib is not None:
        return _lib
    if emu_requested():
        path = os.path.join(_HERE, "libfsv2v_emu.so")
        _is_emu = True
    else:
        # FSV2V_LIB: a diagnostic build of the SAME sources (build.build_hip_diag, tools/knockout.py); never set by the product
        path = os.environ.get("FSV2V_LIB") or os.path.join(_HERE, "libfsv2v_hip.so")
        _is_emu = False
    if not os.path.exists(path):
        raise FsvError("fsv2v kernel library %s is missing; run `python __graft_entry__.py` (build()) first. "
                       "There is no CPU fallback for the product path." % path)
    lib = ctypes.CDLL(path)
    for name, argtypes in _SIGS.items():
        fn = getattr(lib, name)      # AttributeError here == header/library drift; let it propagate loudly
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    _lib = lib
    return lib


def is_emu():
    get_lib()
    return _is_emu


def stream_ptr(t=None):
    if is_emu():
        return None
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_device(*tensors):
    """The HIP library dereferences raw device pointers: refuse host tensors unless emulating."""
    emu = is_emu()
    for t in tensors:
        if t is None:
            continue
        if emu:
            if t.is_cuda:
                raise FsvError("emulated library got a device tensor")
        elif not t.is_cuda:
            raise FsvError("fsv2v HIP kernels need device tensors (got a CPU tensor); no CPU fallback exists")
        if t.dtype not in (torch.float32, torch.int32, torch.float64, torch.float16):
            raise FsvError("unsupported dtype %s" % t.dtype)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def int_array(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def call_status(name, *args):
    """like call(), but returns the fsv_status instead of raising (entry points that may decline with FSV_ERR_UNSUPPORTED)"""
    return int(getattr(get_lib(), name)(*args))


def call(name, *args):
    rc = getattr(get_lib(), name)(*args)
    if rc != 0:
        raise FsvError("%s failed with fsv_status %d" % (name, rc))
