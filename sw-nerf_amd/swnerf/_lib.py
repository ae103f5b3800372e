"""ctypes binding of libswnerf_hip.so, derived from include/swnerf.h: the header is the only place a signature, struct field,
constant or version number is written.  There is NO fallback: if the shared library is missing or a GPU is absent, every op
raises - the product path never routes through a CPU implementation."""
import ctypes
import os
import re
from ctypes import c_void_p, c_char_p, POINTER, Structure

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libswnerf_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "swnerf.h"))

C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
             "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_STRUCT_POINTERS = {}                      # "const swnerf_pass_args*" -> POINTER(PassArgs), filled below


def _c_type(text):
    return re.sub(r"\s+\*", "*", " ".join(text.split()))


def _declarator(decl, where):
    """'const float* A' / 'int L_pos, L_dir' -> (C type, [names])"""
    m = re.fullmatch(r"(.*?[\s*])(\w+(?:\s*,\s*\w+)*)", decl.strip(), re.S)
    if not m:
        raise RuntimeError(f"swnerf.h: cannot read the declaration '{' '.join(decl.split())}' of {where}")
    return _c_type(m[1]), re.split(r"\s*,\s*", m[2])


def parse_header(text):
    """Text of swnerf.h -> (signatures {name: (return C type, [argument C types])} in header order, structs {C name: [(C type,
    field)]}, defines {name minus SWNERF_: int}).  A few regular expressions, not a C front end - so it refuses what it cannot
    read: a swnerf_x( that no parsed prototype accounts for raises and names x."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^#define SWNERF_(\w+)[ \t]+\(?([-+]?\d+)\)?[ \t]*$", text, re.M)}
    structs = {}
    for m in re.finditer(r"typedef struct (swnerf_\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        decls = [_declarator(d, m[1]) for d in m[2].split(";") if d.strip()]
        structs[m[1]] = [(c, f) for c, names in decls for f in names]
    signatures = {}
    for m in re.finditer(r"^([A-Za-z_][\w \t*]*?)\s*\b(swnerf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text, re.M):
        args = [] if m[3].strip() == "void" else [_declarator(a, m[2]) for a in m[3].split(",")]
        if any(len(names) != 1 for _, names in args):
            raise RuntimeError(f"swnerf.h: cannot read the argument list of {m[2]}")
        signatures[m[2]] = (_c_type(m[1]), [c for c, _ in args])
    unread = sorted(set(re.findall(r"\b(swnerf_[a-z_0-9]+)\s*\(", text)) - set(signatures))
    if unread:
        raise RuntimeError(f"swnerf.h: no prototype could be parsed for {', '.join(unread)}")
    return signatures, structs, defines


def ctype_of(c, ret=False):
    """The one rule from C type text to ctypes: the scalars of C_SCALARS; as a return type void -> None and const char* -> c_char_p;
    a pointer to one of the two structs -> POINTER(its Structure), so callers pass the Structure (or an array of them) and get the
    automatic by-reference; EVERY other pointer, device or host, -> c_void_p, whose from_param takes a ctypes array, byref(),
    a typed pointer, a c_void_p, an int and None.  Anything else is an error."""
    if c in C_SCALARS:
        return C_SCALARS[c]
    if ret and c in ("void", "const char*"):
        return None if c == "void" else c_char_p
    if c in _STRUCT_POINTERS:
        return _STRUCT_POINTERS[c]
    if c.endswith("*") and not re.search(r"\bswnerf_", c):
        return c_void_p
    raise RuntimeError(f"swnerf.h: no ctypes mapping for the C type '{c}'")


def _structure(name, c_name):
    cls = type(name, (Structure,), {"__doc__": f"struct {c_name} (include/swnerf.h)",
                                    "_fields_": [(f, ctype_of(c)) for c, f in STRUCTS[c_name]]})
    _STRUCT_POINTERS[f"const {c_name}*"] = POINTER(cls)
    return cls


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"swnerf: {HEADER_PATH} not found - the ctypes binding is derived from it")
with open(HEADER_PATH) as _f:
    SIGNATURES, STRUCTS, DEFINES = parse_header(_f.read())
# the header's integer constants under their names minus SWNERF_: VERSION, E_*, NET_*, ACT_*, SSIM_*, RANGE_*, BWD_*, ADAM_*
globals().update(DEFINES)
EXPORTS = list(SIGNATURES)
GemmItem = _structure("GemmItem", "swnerf_gemm_item")
PassArgs = _structure("PassArgs", "swnerf_pass_args")
_PROTOTYPES = {name: (ctype_of(ret, True), [ctype_of(a) for a in args]) for name, (ret, args) in SIGNATURES.items()}

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"swnerf: {LIB_PATH} not found - build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback for the render path")
    # torch bundles its own libamdhip64/libhsa-runtime64; ours must bind to THAT copy (same SONAME), not
    # pull /opt/rocm's into the process first - two HSA runtimes in one process cannot both own the GPU
    # ("no ROCm-capable device is detected").  So: torch first, always.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.swnerf_version() != DEFINES["VERSION"]:
        raise RuntimeError(f"swnerf: {LIB_PATH} has version {L.swnerf_version()}, expected {DEFINES['VERSION']} - rebuild it "
                           "(python __graft_entry__.py)")
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        msg = lib().swnerf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"swnerf.{what} failed (code {rc}): {msg}")


def stream_of(t):
    import torch
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def dev_f32(t, name, shape_last=None):
    """Validate a device operand the way the C ABI requires (fp32, contiguous, cuda)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"swnerf: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"swnerf: {name} must live on the GPU (got device {t.device}); "
                           "the HIP render path has no CPU implementation")
    if t.dtype != torch.float32:
        t = t.float()
    if not t.is_contiguous():
        t = t.contiguous()
    if shape_last is not None and t.shape[-1] != shape_last:
        raise ValueError(f"swnerf: {name} last dim must be {shape_last}, got {tuple(t.shape)}")
    return t
