"""ctypes binding of libtoda_hip.so (the C ABI of include/toda.h).

There is no CPU fallback: if the shared library is missing, cannot be loaded, or an entry point
reports an error, a RuntimeError is raised.  Tensors are marshalled as raw device pointers and the
current HIP stream; the library never allocates device memory.
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TODA_HIP_LIB") or os.path.join(_HERE, "libtoda_hip.so")   # env override: A/B of kernel builds

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toda.h")

_SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float, "unsigned": C.c_uint,
            "long long": C.c_longlong}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(TODA_\w+)[ \t]+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*\)?[ \t]*$", re.M)
_ENTRY = re.compile(r"\btoda_\w+\s*\(")
_PROTO = re.compile(r"\s*([\w\s*]+?)\b(toda_\w+)\s*\(([^()]*)\)\s*")
_PARAM = re.compile(r"\s*(.*?)\b([A-Za-z_]\w*)\s*(\[[^\]]*\])?\s*", re.S)


def _scalar(decl, symbol):
    scalar = " ".join(w for w in decl.split() if w != "const")
    if scalar not in _SCALARS:
        raise RuntimeError(f"include/toda.h: {symbol}: no ctypes type for '{' '.join(decl.split())}'")
    return _SCALARS[scalar]


def parse_header(text):
    """Text of include/toda.h -> (name -> (restype, argtypes), name -> parameter names, TODA_* integer macro -> value).
    Pointers and array parameters are c_void_p, a `const char*` result is c_char_p, scalars are looked up in _SCALARS.
    Every `toda_x(` outside comments and preprocessor lines must belong to a plain prototype: anything else raises."""
    text = _COMMENT.sub(" ", text)
    defines = {m[1]: int(m[2], 0) for m in _DEFINE.finditer(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    signatures, arg_names = {}, {}
    for decl in re.split(r"[;{}]", text):
        if not _ENTRY.search(decl):
            continue
        m = _PROTO.fullmatch(decl)
        if m is None:
            raise RuntimeError(f"include/toda.h: cannot parse the declaration '{' '.join(decl.split())}'")
        ret, name, params = " ".join(m[1].split()), m[2], m[3].strip()
        types, names = [], []
        for param in ([] if params == "void" else params.split(",")):
            pm = _PARAM.fullmatch(param)
            if pm is None:
                raise RuntimeError(f"include/toda.h: {name}: cannot parse the parameter '{' '.join(param.split())}'")
            types.append(C.c_void_p if "*" in pm[1] or pm[3] else _scalar(pm[1], name))
            names.append(pm[2])
        signatures[name] = (C.c_char_p if ret == "const char*" else _scalar(ret, name), types)
        arg_names[name] = tuple(names)
    if len(_ENTRY.findall(text)) != len(signatures):      # one name declared twice, or two names inside one declaration
        raise RuntimeError(f"include/toda.h: {len(_ENTRY.findall(text))} times `toda_x(`, but {len(signatures)} prototypes")
    return signatures, arg_names, defines


def _header_text():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} not found: toda_amd reads the prototypes of libtoda_hip.so from it.")
    with open(HEADER_PATH) as f:
        return f.read()


# name -> (restype, argtypes), name -> parameter names, and the integer TODA_* macros: all as include/toda.h declares them
SIGNATURES, ARG_NAMES, DEFINES = parse_header(_header_text())

_lib = None


def load():
    """Load libtoda_hip.so (once) and attach prototypes.  Raises RuntimeError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  toda_amd has no CPU fallback."
        )
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the host
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load().toda_last_error().decode()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {last_error()}")


def ptr(t):
    """Device pointer of a CUDA tensor (None -> NULL).  Refuses host tensors loudly."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("toda_amd ops need tensors on the GPU (there is no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError("toda_amd ops need contiguous tensors")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """Raw handle of torch's current HIP stream on the current device.  (torch.cuda.current_stream() builds a Stream object
    and resolves the device through three Python layers: ~9 us per call, ~200 calls per training step.)"""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def host_ptrs(tensors):
    """Host array of device pointers (None -> NULL) for the entry points that take several tensors per call."""
    return (C.c_void_p * len(tensors))(*[ptr(t) for t in tensors])


def host_addrs(addrs):
    """Host array of raw device addresses (slices of one tensor)."""
    return (C.c_void_p * len(addrs))(*[int(a) for a in addrs])


def host_i32(vals):
    arr = (C.c_int32 * len(vals))(*[int(v) for v in vals])
    return arr


def host_f32(vals):
    arr = (C.c_float * len(vals))(*[float(v) for v in vals])
    return arr


def host_f64(vals):
    arr = (C.c_double * len(vals))(*[float(v) for v in vals])
    return arr


def hptr(arr):
    return C.cast(arr, C.c_void_p)


class Conv3x3WeightEntry(C.Structure):
    """toda_conv3x3_weight_entry of include/toda.h."""
    _fields_ = [("w", C.c_void_p), ("cout", C.c_int32), ("cin", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32), ("u", C.c_void_p)]
