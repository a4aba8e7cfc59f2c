"""ctypes binding of libqpg_hip.so (the C ABI declared in include/qpg.h).

The library is the product: if it is missing or a call fails this module raises —
there is no CPU or PyTorch fallback anywhere in the package.
"""
import collections
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# QPG_LIB_PATH: kernel experiments only (a variant build of the same sources); the product is the in-tree library
LIB_PATH = os.environ.get("QPG_LIB_PATH") or os.path.join(_HERE, "libqpg_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "qpg.h")

_lib = None
_ctx = {}

c_void_p = ctypes.c_void_p

# The binding is derived from include/qpg.h: the header is the one place that states a prototype or a constant.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_HOOKS_RE = re.compile(r"#ifdef QPG_DEBUG_HOOKS\n(.*?)#endif", re.S)
_PROTO_RE = re.compile(r"\s*([\w\s*]+?)\s*\b(qpg_\w+)\s*\(([^()]*)\)\s*")
# on_stream: the entry point starts (qpg_ctx*, void* stream, ...) - the ones call() / prepare() launch; hook: it sits in
# the #ifdef QPG_DEBUG_HOOKS block (experiment builds only, the product library does not export it)
Prototype = collections.namedtuple("Prototype", "restype argtypes on_stream hook")


def _ctype(decl, name, ret=False):
    """ctypes type of one C parameter or return type.  Any pointer is a c_void_p (it accepts byref(), string buffers, None,
    integers and c_void_p handles; a returned char* is a c_char_p), a scalar goes by its type word.  A word _SCALARS does
    not know raises with the function's name: guessing `int` would corrupt the call silently."""
    words = [w for w in decl.replace("*", " ").split() if w != "const"]
    if "*" in decl:
        return ctypes.c_char_p if ret and words[0] == "char" else c_void_p
    if ret and words == ["void"]:
        return None
    if not words or words[0] not in _SCALARS:
        raise TypeError("%s: no ctypes mapping for %r" % (name, " ".join(decl.split())))
    return _SCALARS[words[0]]


def _number(text):
    text = text.strip()
    while text.startswith("(") and text.endswith(")"):
        text = text[1:-1].strip()
    m = re.fullmatch(r"(\d+)\s*<<\s*(\d+)", text)
    if m:
        return int(m.group(1)) << int(m.group(2))
    try:
        return int(text, 0)
    except ValueError:
        return float(text)


def parse_header(path=HEADER_PATH):
    """One pass over the header: ({function name: Prototype}, {QPG_* constant: int or float})."""
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    consts = {m.group(1): _number(m.group(2)) for m in re.finditer(r"^#define[ \t]+(QPG_\w+)[ \t]+(\S.*)$", txt, re.M)}
    protos = {}
    for hook, body in [(False, _HOOKS_RE.sub("", txt))] + [(True, blk) for blk in _HOOKS_RE.findall(txt)]:
        body = re.sub(r'^[ \t]*(#.*|extern "C" \{)$', "", body, flags=re.M)
        for stmt in body.split(";"):
            if "(" not in stmt:
                continue                                 # (typedefs, struct members)
            m = _PROTO_RE.fullmatch(stmt)
            if not m:
                raise TypeError("%s: not a prototype: %r" % (path, " ".join(stmt.split())))
            ret, name, params = m.groups()
            params = [] if params.strip() in ("", "void") else params.split(",")
            on_stream = len(params) > 1 and "qpg_ctx" in params[0] and params[1].split() == ["void*", "stream"]
            protos[name] = Prototype(_ctype(ret, name, ret=True), [_ctype(p, name) for p in params], on_stream, hook)
    return protos, consts


_PROTOS, CONSTANTS = parse_header()
globals().update(CONSTANTS)              # every `#define QPG_X <number>` of the header is _lib.QPG_X


def prototypes():
    """{name: Prototype} of every function include/qpg.h declares (what load() binds)."""
    return _PROTOS


def declared_symbols():
    """Every function name include/qpg.h declares for the PRODUCT library (used by the CPU symbol-export test); the
    #ifdef QPG_DEBUG_HOOKS block - experiment builds only - is debug_hook_symbols()."""
    return sorted(n for n, p in _PROTOS.items() if not p.hook)


def debug_hook_symbols():
    return sorted(n for n, p in _PROTOS.items() if p.hook)


class ConvDesc(ctypes.Structure):
    _fields_ = [("w", c_void_p), ("b", c_void_p), ("taps", ctypes.c_int32), ("cin", ctypes.c_int32),
                ("cin_pad", ctypes.c_int32), ("cout", ctypes.c_int32), ("cout_pad", ctypes.c_int32),
                ("wt", c_void_p)]


class VqModel(ctypes.Structure):
    """qpg_vq_model of include/qpg.h."""
    _fields_ = [("in_dim", ctypes.c_int32), ("width", ctypes.c_int32), ("emb", ctypes.c_int32),
                ("bins", ctypes.c_int32), ("down_t", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("growth", ctypes.c_int32), ("reverse_dec", ctypes.c_int32),
                ("enc_down", ConvDesc * QPG_VQ_MAX_DOWN),
                ("enc_res", ((ConvDesc * 2) * QPG_VQ_MAX_DEPTH) * QPG_VQ_MAX_DOWN),
                ("enc_out", ConvDesc), ("dec_in", ConvDesc),
                ("dec_res", ((ConvDesc * 2) * QPG_VQ_MAX_DEPTH) * QPG_VQ_MAX_DOWN),
                ("dec_up_even", ConvDesc * QPG_VQ_MAX_DOWN), ("dec_up_odd", ConvDesc * QPG_VQ_MAX_DOWN),
                ("dec_out", ConvDesc), ("kT", ConvDesc), ("k", c_void_p), ("kk", c_void_p),
                ("enc_res_pack", (c_void_p * QPG_VQ_MAX_DEPTH) * QPG_VQ_MAX_DOWN),
                ("dec_res_pack", (c_void_p * QPG_VQ_MAX_DEPTH) * QPG_VQ_MAX_DOWN)]


def load():
    """dlopen the library (works without a GPU: symbols only)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libqpg_hip.so is missing (%s). Build it with `python -m qpgesture_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no fallback path." % LIB_PATH)
    if not os.environ.get("QPG_LIB_PATH"):
        # the in-tree library must be the one compiled from THIS tree's sources (a stale prebuilt would be tested and
        # benchmarked as if it were HEAD): compare its stamped id with the tree's hash BEFORE mapping it; rebuild on a mismatch
        from . import build as _build
        want = _build.source_hash()
        if _build.lib_build_id(LIB_PATH) != want:
            _build.build_lib(verbose=False)
    lib = ctypes.CDLL(LIB_PATH)
    for name, proto in _PROTOS.items():
        if proto.hook and not hasattr(lib, name):
            continue                                     # (-DQPG_DEBUG_HOOKS variant libraries only: QPG_LIB_PATH)
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = proto.argtypes, proto.restype
    _lib = lib
    return lib



def set_option(device, option, value):
    """qpg_ctx_set_option on `device`'s context (per-context knob, include/qpg.h)."""
    rc = load().qpg_ctx_set_option(ctx(device), option, value)
    if rc != 0:
        raise RuntimeError("qpg_ctx_set_option failed (%d): %s" % (rc, last_error()))


def last_error():
    buf = ctypes.create_string_buffer(512)
    load().qpg_last_error(buf, 512)
    return buf.value.decode()


def ctx(device):
    """Per-device opaque context (created on first use)."""
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    if idx not in _ctx:
        h = c_void_p()
        rc = load().qpg_ctx_create(idx, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError("qpg_ctx_create(%d) failed: %s" % (idx, last_error()))
        _ctx[idx] = h
    return _ctx[idx]


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return c_void_p(t.data_ptr())


_cur_dev = None
_dev_index = {}
n_calls = 0          # launches made through call() / prepare() (parallel.SegmentRecorder: is a captured segment empty?)
# torch's C entry points behind torch.cuda.current_device() / current_stream().cuda_stream: the Python wrappers cost ~1 and
# ~3 us per call (lazy-init checks, a Stream object per call) and this module makes a dozen calls per 0.36 ms step
_get_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
_raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_stream(idx):
    if _raw is not None:
        return _raw(idx)
    return torch.cuda.current_stream(idx).cuda_stream


def _convert(args):
    """What the foreign call receives: tensors as their data_ptr() integers, structures by reference."""
    conv = []
    for a in args:
        if isinstance(a, torch.Tensor):
            if not (a.is_cuda and a.is_contiguous()):
                raise AssertionError("device-resident contiguous tensor required")
            conv.append(a.data_ptr())
        elif isinstance(a, ctypes.Structure):
            conv.append(ctypes.byref(a))
        else:
            conv.append(a)                      # (ints, floats, None, c_void_p handles)
    return conv


class Unsupported(RuntimeError):
    """An entry point returned QPG_EUNSUP: the compiled kernels do not take this shape.  Nothing was launched."""


def _raise(name, rc):
    raise (Unsupported if rc == QPG_EUNSUP else RuntimeError)("%s failed (%d): %s" % (name, rc, last_error()))


def call(name, device, *args):
    """Invoke a C-ABI entry point on torch's current stream of `device`; raise on error.

    HIP launches go to the CURRENT device (a stream handle of 0 means "the current device's default stream"),
    so when `device` is not the calling thread's current device the call is made under torch.cuda.device(device):
    a GestureDB / VQVAE built on cuda:1 works whatever device the caller has selected.
    (This wrapper sits in front of every launch of a clip - a dozen per 0.4 ms step - so it avoids what it can:
    device indices are cached, tensors go in as their data_ptr() integers.)"""
    global n_calls
    lib = _lib if _lib is not None else load()
    idx = _dev_index.get(device)
    if idx is None:
        idx = torch.device(device).index
        if idx is None:
            idx = torch.cuda.current_device()
        _dev_index[device] = idx
    if idx != _get_device():
        with torch.cuda.device(idx):
            return call(name, device, *args)
    n_calls += 1
    stream = _raw_stream(idx)
    conv = _convert(args)
    h = _ctx.get(idx)
    if h is None:
        h = ctx(device)
    rc = getattr(lib, name)(h, stream, *conv)
    if rc != 0:
        _raise(name, rc)


def prepare(name, device, *args):
    """call() in two halves: everything but the foreign call happens now, the returned function makes the launch (on the
    stream that is current NOW).  For a launch that has to follow another one closely - the sweep behind its query pack:
    the argument conversion of its 15 arguments would otherwise sit between the two launches (~5 us of idle GPU)."""
    lib = _lib if _lib is not None else load()
    idx = _dev_index.get(device)
    if idx is None or idx != _get_device():
        return lambda: call(name, device, *args)
    stream = _raw_stream(idx)
    conv = _convert(args)
    h = _ctx.get(idx)
    if h is None:
        h = ctx(device)
    fn = getattr(lib, name)

    def launch(_keep=args):          # (the tensors stay alive until the launch has been made)
        global n_calls
        n_calls += 1
        rc = fn(h, stream, *conv)
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, rc, last_error()))
    return launch
