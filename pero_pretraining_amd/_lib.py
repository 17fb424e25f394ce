"""ctypes binding of libpero_hip.so.  include/pero_hip.h is the one description of the C ABI: it is parsed at import into FUNCTIONS
(name -> restype, argtypes) and DEFINES (name -> int), so an entry point or a constant is declared there and nowhere else.

The product path has no fallback: if the shared library is missing this module raises at import of
the first op, and every non-zero return code becomes a Python exception carrying pero_last_error().
"""
import ast
import ctypes
import operator
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpero_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pero_hip.h")


class PeroHipError(RuntimeError):
    pass


# the closed type map: parameters by value, and return types; every pointer parameter is c_void_p except `const char*`
_VALUE_TYPES = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int, "float": ctypes.c_float,
                "double": ctypes.c_double, "uint64_t": ctypes.c_uint64}
_RETURN_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"(.*?)\b(pero_\w+)\s*\(([^()]*)\)", re.S)
_POINTER = re.compile(r"((?:\w+ )*\w+) ?\*+ ?\w+")
_DEFINE = re.compile(r"#\s*define\s+(PERO_\w+)[ \t]+(\S.*)")   # object-like only: a function-like macro has `(` right behind its name
_INT_EXPR = re.compile(r"[0-9\s()+\-*<]+")
_INT_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.LShift: operator.lshift}


def int_expr(text):
    """Value of an expression of decimal literals, ( ) + - * <<: a walk over its syntax tree, nothing is executed.  ValueError otherwise."""
    def value(node):
        if isinstance(node, ast.Constant) and type(node.value) is int:
            return node.value
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            return -value(node.operand)
        if isinstance(node, ast.BinOp) and type(node.op) in _INT_OPS:
            return _INT_OPS[type(node.op)](value(node.left), value(node.right))
        raise ValueError(f"not an integer expression: {text!r}")
    try:
        if _INT_EXPR.fullmatch(text):
            return value(ast.parse(text.strip(), mode="eval").body)
    except SyntaxError:
        pass
    raise ValueError(f"not an integer expression: {text!r}")


def _argtype(func, param):
    param = " ".join(param.split())
    m = _POINTER.fullmatch(param)
    if m:
        return ctypes.c_char_p if m.group(1) == "const char" else ctypes.c_void_p
    ctype, _, name = param.rpartition(" ")
    if ctype not in _VALUE_TYPES or not name.isidentifier():
        raise PeroHipError(f"{func}: no ctypes type for `{ctype or param}` (parameter `{param}`)")
    return _VALUE_TYPES[ctype]


def parse_header(text):
    """(functions, defines) of a header written like include/pero_hip.h: functions[name] = (restype, argtypes) for every `pero_*`
    prototype, defines[name] = int for every object-like `#define PERO_<NAME> <integer expression>`.  Comments declare nothing.
    Nothing is guessed: a statement that is no prototype, or a type outside the closed map, raises, naming the function and the token."""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    # a value that is no integer expression (a string, another name) is no constant of this module's
    defines = {name: int_expr(value) for name, value in _DEFINE.findall(text) if _INT_EXPR.fullmatch(value)}
    functions = {}
    body = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        m = _PROTOTYPE.fullmatch(stmt)
        if not m:
            raise PeroHipError(f"cannot parse the declaration `{' '.join(stmt.split())}`")
        ret, name, params = re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())), m.group(2), m.group(3).strip()
        if ret not in _RETURN_TYPES:
            raise PeroHipError(f"{name}: no ctypes type for the return type `{ret}`")
        functions[name] = (_RETURN_TYPES[ret], [] if params == "void" else [_argtype(name, p) for p in params.split(",")])
    return functions, defines


if not os.path.exists(HEADER_PATH):
    raise PeroHipError(f"{HEADER_PATH} not found: the binding is read from the header the library is compiled against "
                       "(include/ next to the package, where the Makefile expects it).")
with open(HEADER_PATH) as _f:
    FUNCTIONS, DEFINES = parse_header(_f.read())


def _names(prefix):
    return {v: k[len(prefix):].lower() for k, v in DEFINES.items() if k.startswith(prefix)}


PERO_F32, PERO_BF16, LN_BWD_BLOCKS = DEFINES["PERO_F32"], DEFINES["PERO_BF16"], DEFINES["PERO_LN_BWD_BLOCKS"]
(GEMM_RELU, GEMM_ATOMIC, GEMM_ACCUM, GEMM_TRANS_A, GEMM_TRANS_B, GEMM_FORCE_GENERIC, GEMM_ROWDOT, GEMM_RELU_BITS, GEMM_MASK_TILED,
 GEMM_COLSUM, GEMM_TILE_V, GEMM_TILE128, GEMM_TILE256) = (DEFINES["PERO_GEMM_" + n] for n in (
     "RELU", "ATOMIC", "ACCUM", "TRANS_A", "TRANS_B", "FORCE_GENERIC", "ROWDOT", "RELU_BITS", "MASK_TILED",
     "COLSUM", "TILE_V", "TILE128", "TILE256"))
# pero_gemm_plan: the kernel family that takes a product, and the pass pero_gemm runs over C where that kernel has no fused side output
GEMM_KERNELS = _names("PERO_GEMM_KERNEL_")
GEMM_PASSES = {0: None, **_names("PERO_GEMM_PASS_")}

# name -> argtypes of the functions that return an int: a status (those are for call()), a count, or pero_gemm_plan's kernel family
SIGNATURES = {name: argtypes for name, (restype, argtypes) in FUNCTIONS.items()
              if restype is ctypes.c_int and name not in ("pero_abi_version", "pero_set_option")}

ABI_VERSION = 2
_lib = None
_lib_lock = threading.Lock()


def lib():
    """Load (once) and return the ctypes handle.  Raises if the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise PeroHipError(
                f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        h = ctypes.CDLL(LIB_PATH)
        if h.pero_abi_version() != ABI_VERSION:   # before the loop: an older library may lack a symbol, and says so less clearly
            raise PeroHipError(f"{LIB_PATH} has ABI version {h.pero_abi_version()}, this package binds version {ABI_VERSION}: rebuild it "
                               f"(`make -C {os.path.join(_HERE, 'csrc')}`)")
        for name, (restype, argtypes) in FUNCTIONS.items():
            fn = getattr(h, name)   # declared in the header but not exported: fails here, at load
            fn.restype, fn.argtypes = restype, argtypes
        # PERO_OPTIONS="name=value,name=value": pero_set_option knobs for a whole process (A/B runs of a tool or of bench.py under a profiler); unknown names raise
        for item in filter(None, os.environ.get("PERO_OPTIONS", "").split(",")):
            name, _, value = item.partition("=")
            if h.pero_set_option(name.strip().encode(), int(value)) != 0:
                raise PeroHipError(f"PERO_OPTIONS: {h.pero_last_error().decode()}")
        _lib = h
    return _lib


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise PeroHipError(f"{name} failed ({rc}): {lib().pero_last_error().decode()}")
