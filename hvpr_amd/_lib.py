"""ctypes binding of libhvpr_amd.so, derived from the declaration of its C-ABI, include/hvpr_amd.h: one header, one pair of tables.

parse_header turns the header's prototypes into ctypes signatures (SIGNATURES) and, per parameter, the element type a
tensor passed there must have (PARAMS); call() checks every tensor against that before it becomes a pointer.
The product path has NO CPU fallback: if the library is missing or fails to load, every op raises.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 8          # hvpr_abi_version() of the library these wrappers were written against (csrc/abi.hip)
LIB_PATH = os.environ.get("HVPR_AMD_LIB", os.path.join(_HERE, "libhvpr_amd.so"))   # override: kernel experiments only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hvpr_amd.h")

_c = ctypes
# hvpr_allreduce_fn: (double *buf, int n, hvpr_stream_t stream, void *ctx) -> int
ALLREDUCE_FN = _c.CFUNCTYPE(_c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p)


class HvprLibraryError(RuntimeError):
    pass


# The closed vocabulary of the header; any other type in a prototype is an error, never a guess.
ANY = "any dtype"        # parameter kind of a `void *`
_RETURNS = {"int": _c.c_int, "size_t": _c.c_size_t, "void": None, "const char *": _c.c_char_p}
_SCALARS = {"int": _c.c_int, "float": _c.c_float, "double": _c.c_double, "size_t": _c.c_size_t, "long long": _c.c_longlong,
            "hvpr_stream_t": _c.c_void_p, "hvpr_allreduce_fn": _c.c_void_p}
_ELEMENTS = {"float": torch.float32, "int32_t": torch.int32, "int64_t": torch.int64, "long long": torch.int64,
             "double": torch.float64, "uint8_t": torch.uint8, "void": ANY}
_PROTOTYPE = re.compile(r"([^;{}()]+?)\b(\w+)\s*\(([^()]*)\)\s*;")
_PARAMETER = re.compile(r"(?:const )?([\w ]+?) ?(\*)? ?(\w+)")


def parse_header(text):
    """name -> (restype, argtypes, params) for every `ret name(params);` of a C header; params is a tuple of (name, kind) with kind
    a torch dtype for a typed pointer, ANY for a `void *` and None for a scalar.  A name declared twice raises."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*(#|typedef\b|extern\b).*$", "", text, flags=re.M)
    table = {}
    for m in _PROTOTYPE.finditer(text):
        proto = " ".join(m.group(0).split())
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        if ret not in _RETURNS:
            raise HvprLibraryError(f"unknown return type in `{proto}`")
        argtypes, kinds = [], []
        for p in ([] if params in ("", "void") else params.split(",")):
            pm = _PARAMETER.fullmatch(p.strip())
            known = pm and pm.group(1) in (_ELEMENTS if pm.group(2) else _SCALARS)
            if not known:
                raise HvprLibraryError(f"unknown parameter type `{p.strip()}` in `{proto}`")
            argtypes.append(_c.c_void_p if pm.group(2) else _SCALARS[pm.group(1)])
            kinds.append((pm.group(3), _ELEMENTS[pm.group(1)] if pm.group(2) else None))
        if name in table:
            raise HvprLibraryError(f"{name} is declared twice")
        table[name] = (_RETURNS[ret], argtypes, tuple(kinds))
    return table


def read_header(path):
    if not os.path.exists(path):
        raise HvprLibraryError(f"{path} is missing: the binding is derived from it")
    with open(path) as f:
        return parse_header(f.read())


PARAMS = {}              # name -> ((parameter name, kind), ...)
SIGNATURES = {}          # name -> (restype, argtypes)
for _name, (_res, _args, _params) in read_header(HEADER_PATH).items():
    SIGNATURES[_name], PARAMS[_name] = (_res, _args), _params

_lib = None
_calls = {}              # name -> (bound function, ((index, name, kind) of each pointer), (index of each scalar)): made once in lib(),
                         # for the functions that return a status


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HvprLibraryError(
                f"{LIB_PATH} is missing: build it with `python -m hvpr_amd.build` (hipcc --offload-arch=gfx950). "
                "hvpr_amd has no CPU fallback.")
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise HvprLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
            if res is _c.c_int:
                kinds = PARAMS[name]
                _calls[name] = (fn, tuple((i, p, k) for i, (p, k) in enumerate(kinds) if k is not None),
                                tuple(i for i, (_, k) in enumerate(kinds) if k is None))
        if L.hvpr_abi_version() != ABI_VERSION:      # a stale .so next to newer Python wrappers (buffer sizes, argument lists)
            raise HvprLibraryError(f"{LIB_PATH} has ABI version {L.hvpr_abi_version()}, these wrappers need {ABI_VERSION}: "
                                   "rebuild it with `python -m hvpr_amd.build`")
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().hvpr_status_string(int(status))
        raise RuntimeError(f"{what} failed: {msg.decode() if msg else status}")


_PLAIN = {int, float, bool}          # what a scalar argument usually is; anything else gets a closer look


def call(name, *args):
    """lib().name(*args) for a function that returns a status, raising on a non-zero one.  A tensor stands for its device pointer
    and is checked against the header's parameter (GPU, element type, contiguous); None, addresses, ctypes objects and numbers
    go to ctypes as they are."""
    if _lib is None:
        lib()
    if name not in _calls:
        raise HvprLibraryError(f"{name} is not a status-returning function of {HEADER_PATH}")
    fn, pointers, scalars = _calls[name]
    if len(args) != len(pointers) + len(scalars):
        raise TypeError(f"{name} takes {len(pointers) + len(scalars)} arguments, got {len(args)}")
    if not _PLAIN.issuperset(map(type, map(args.__getitem__, scalars))):      # one pass in C: this runs hundreds of times a step
        for i in scalars:
            if isinstance(args[i], torch.Tensor):
                raise TypeError(f"{name}: {PARAMS[name][i][0]} is a scalar, got a tensor")
    argv = list(args)
    for i, pname, kind in pointers:
        t = argv[i]
        if t is not None and isinstance(t, torch.Tensor):
            if not t.is_cuda:
                raise RuntimeError(f"{name}: {pname} must live on the GPU (the HIP path has no CPU fallback)")
            if t.dtype is not kind and kind is not ANY:
                raise TypeError(f"{name}: {pname} must be {kind}, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{name}: {pname} must be contiguous")
            argv[i] = t.data_ptr()
    check(fn(*argv), name)
