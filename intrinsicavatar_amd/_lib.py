"""ctypes loader for libia_amd.so -- the ONLY compute backend of this package.

There is deliberately no CPU / PyTorch fallback: if the HIP library is missing or a
tensor is not on a GPU, the call fails loudly.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("IA_AMD_LIB") or os.path.join(_HERE, "libia_amd.so")     # IA_AMD_LIB: another build of the same library (A/B runs)
_lib = None


class IaError(RuntimeError):
    pass


_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ia_amd.h")
_CTYPE = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
          "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "ia_stream_t": C.c_void_p, "void": None}


def _header_entries(path: str):
    """(name, restype, [argtypes], takes_stream) of every `ia_*` prototype in the header"""
    import re
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    txt = re.sub(r"^\s*#[^\n]*", " ", txt, flags=re.M)                # preprocessor lines
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(ia_\w+)\s*\(([^()]*)\)\s*;", txt):
        def ctype(decl, is_ret=False):
            decl = decl.replace("const", " ").strip()
            if "*" in decl:
                return C.c_char_p if (is_ret and "char" in decl) else C.c_void_p
            base = decl.split()[0] if is_ret else decl.split()[0]
            if base not in _CTYPE:
                raise IaError(f"include/ia_amd.h: unknown type in prototype of {name}: {decl!r}")
            return _CTYPE[base]
        ret = ret.strip()
        if ret.startswith("typedef") or not ret:
            continue
        arglist = [a_.strip() for a_ in args.split(",") if a_.strip()]
        if arglist == ["void"]:
            arglist = []
        takes_stream = any(a_.split()[0] == "ia_stream_t" for a_ in arglist)
        if takes_stream and (arglist[-1].split()[0] != "ia_stream_t" or ret != "int"):
            raise IaError(f"include/ia_amd.h: {name} takes a stream, so the stream must be its last parameter and its result an int status")
        yield name, ctype(ret, True), [ctype(a_) for a_ in arglist], takes_stream


def header_prototypes(path: str = _HEADER):
    """{name: (restype, [argtypes])} of every `ia_*` prototype in include/ia_amd.h -- the header is the single source of the
    ABI: the loader declares argtypes / restype for EVERY entry point from it, so a call with a missing, extra or mistyped
    argument raises in Python instead of reading garbage off the stack.  Pointers (device or host) are void*."""
    return {name: (restype, argtypes) for name, restype, argtypes, _ in _header_entries(path)}


def header_host_only(path: str = _HEADER):
    """names of the entry points that enqueue nothing -- size queries, constants, diagnostics: an entry point launches work if
    and only if its prototype takes an ia_stream_t.  The binding hands these out as they are."""
    return frozenset(name for name, _, _, takes_stream in _header_entries(path) if not takes_stream)


class _TensorPtr(C.c_void_p):
    """device pointer that OWNS a reference to its tensor: the wrapped spelling of a pointer argument (ptr() below), for callers that
    build an argument before the call that consumes it (bench.py, tools/).  It keeps `ptr(x.contiguous())` alive as long as itself."""


def _address(t):
    if not t.is_cuda:
        raise IaError("intrinsicavatar_amd operators need GPU tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise IaError("tensor must be contiguous")
    return t.data_ptr()


def ptr(t):
    """device pointer of a contiguous CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return C.c_void_p(0)
    p = _TensorPtr(_address(t))
    p._keep = t
    return p


def _row_address(t):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() >= 1 and t.stride(-1) == 1):
        raise IaError("row-strided operands must be float32 GPU tensors with unit inner stride")
    return t.data_ptr()


def base_ptr(t):
    """base address of a row-strided view (the entry point takes the row stride as a parameter of its own): a GPU float32 tensor
    with unit inner stride, which need not be contiguous."""
    p = _TensorPtr(_row_address(t))
    p._keep = t
    return p


def segments(segs):
    """the segment table of the MLP entry points -- segs: [(tensor [n, >= width], width, mul, add)] -> (ns, ptrs, strides, widths,
    muls, adds), host arrays in the order the prototypes take them.  The caller's list keeps the tensors alive."""
    ns = len(segs)
    ptrs, strides, widths = (C.c_void_p * ns)(), (C.c_int * ns)(), (C.c_int * ns)()
    muls, adds = (C.c_float * ns)(), (C.c_float * ns)()
    for i, (t, w, m, a) in enumerate(segs):
        ptrs[i], strides[i], widths[i], muls[i], adds[i] = _row_address(t), t.stride(0), w, m, a
    return ns, ptrs, strides, widths, muls, adds


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


i64 = C.c_int64
i32 = C.c_int
f32 = C.c_float


def _value(a):
    return a.value if isinstance(a, C._SimpleCData) else a          # plain or wrapped (i64(..), ptr(..): NULL reads as None)


# optional outputs that change an entry point's compulsory traffic: ia_fuse_broyden(..., x, J_inv, is_valid, fwd_J, stream)
_EXTRAS = {"ia_fuse_broyden": lambda a: dict(I=int(_value(a[2])), J_inv=_value(a[16]) is not None, fwd_J=_value(a[18]) is not None),
           "ia_fuse_broyden_spec": lambda a: dict(I=int(_value(a[1])), J_inv=_value(a[15]) is not None, fwd_J=_value(a[17]) is not None),
           "ia_fuse_broyden_spec_rows": lambda a: dict(I=int(_value(a[1])), J_inv=_value(a[15]) is not None,
                                                       fwd_J=_value(a[16]) is not None, rows=True)}


class _Binding:
    """one callable per entry point of a (library, header) pair.  A launch -- an entry point whose prototype ends in an ia_stream_t --
    takes tensors and plain numbers, gets torch's current stream when the caller leaves it out, and raises IaError on a non-zero
    status; a host-only query is the ctypes function itself (argtypes convert its numbers, its result is a value, not a status).

    Optional per-entry-point HIP-event timing (bench.py): start() ... report(); events are recorded on the stream the kernels are
    launched on (torch's current stream), nothing synchronises until report()."""

    def __init__(self, so: str, header: str):
        self._cdll = C.CDLL(so)
        self.enabled = False
        self.events = {}
        untimed = []
        for name, restype, argtypes, takes_stream in _header_entries(header):
            fn = getattr(self._cdll, name)         # AttributeError: the header declares a symbol the library does not export
            fn.restype, fn.argtypes = restype, argtypes
            if takes_stream:
                fn = self._launch(name, fn, argtypes)
            else:
                untimed.append(name)
            setattr(self, name, fn)
        self._untimed = frozenset(untimed)         # host-only entry points (header_host_only): nothing to put events around

    def _launch(self, name, fn, argtypes):
        # (everything the header says about the call is worked out here, once: the 4096-ray training step is bound by the host's
        #  launch rate, profiles/r06_launch_audit_before.json)
        nargs = len(argtypes)
        pointers = tuple(i for i, t in enumerate(argtypes[:-1]) if t is C.c_void_p)         # (the stream, last, is ctypes' to convert)
        numbers = tuple(i for i, t in enumerate(argtypes) if t is not C.c_void_p)
        units_at = next((i for i, t in enumerate(argtypes) if t is C.c_int64), None)    # every entry point leads with its element count
        extras = _EXTRAS.get(name)

        def call(*args):
            if len(args) == nargs - 1:
                args += (stream(),)
            elif len(args) != nargs:
                raise TypeError(f"{name} takes {nargs} arguments ({nargs - 1} without the stream), {len(args)} given")
            # LIFETIME: a temporary such as `x.contiguous()` must stay alive until its kernel is ENQUEUED -- otherwise the caching
            # allocator may hand its block to the next temporary (after the enqueue, stream order makes reuse safe).  The tensors are
            # arguments of this call, so `args` holds every one of them until fn() has returned; only addresses go into `raw`.
            raw = list(args)
            for i in pointers:
                a = args[i]
                if isinstance(a, torch.Tensor):
                    raw[i] = _address(a)
                elif isinstance(a, int):
                    raise TypeError(f"{name}: argument {i} is a pointer, a bare int was passed (tensor, None, ctypes array or ptr())")
            for i in numbers:
                if isinstance(args[i], torch.Tensor):          # (ctypes alone would read a one-element tensor back through __index__)
                    raise TypeError(f"{name}: argument {i} is a number, a tensor was passed")
            if self.enabled:
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*raw)
                e1.record()
                # units of the launch = its first int64_t parameter; per-entry extras (which optional outputs were requested) for
                # the algorithmic-bytes model of bench.py
                units = int(_value(args[units_at])) if units_at is not None else 0
                self.events.setdefault(name, []).append((e0, e1, units, extras(args) if extras else None))
            else:
                rc = fn(*raw)
            if rc != 0:
                raise IaError(f"{name} failed (code {rc}): {self._cdll.ia_last_error().decode(errors='replace')}")
            return rc
        return call

    def start(self):
        self.events = {}
        self.enabled = True

    def report(self, detail: bool = False):
        """-> {entry point: (n_calls, total_ms)}; synchronises.  detail=True: {entry point: [(ms, units, extras), ...]}."""
        self.enabled = False
        torch.cuda.synchronize()
        if detail:
            return {k: [(a.elapsed_time(b), u, x) for a, b, u, x in v] for k, v in self.events.items()}
        return {k: (len(v), sum(a.elapsed_time(b) for a, b, _, _ in v)) for k, v in self.events.items()}


def load(so: str, header: str) -> _Binding:
    """the binding of a (library, header) pair; lib() is this for the package's own."""
    if not os.path.exists(so):
        raise IaError(
            f"{so} not found: build it with `python -m intrinsicavatar_amd.build` "
            "(there is no CPU fallback for the MI355X hot path)")
    if not os.path.exists(header):
        raise IaError(f"{header} not found: the C-ABI header declares the argument types of {os.path.basename(so)}")
    return _Binding(so, header)


def lib():
    global _lib
    if _lib is None:
        _lib = load(_SO, _HEADER)
    return _lib


def check(rc: int, what: str = ""):
    """the wrapped spelling's status check: a launch has raised by itself before it returns, so this only ever sees 0."""
    if rc != 0:
        msg = lib().ia_last_error().decode(errors="replace")
        raise IaError(f"{what} failed (code {rc}): {msg}")


_SCRATCH = {}


def scratch(name: str, nbytes: int, device):
    """grow-only scratch buffer `name` of at least `nbytes` bytes on `device` (uint8 view).  For the big per-call work areas that a
    launch consumes before the next call on the same stream can touch them (level-major hash features: 128 B / point; the sort's
    key / index columns): when the batch size changes from call to call -- another pose every frame -- the caching allocator
    cannot reuse its blocks and every call pays a multi-GB hipMalloc / hipFree (2.7 against 0.9 s per relit 540 x 540 frame)."""
    nbytes = int(nbytes)
    key = (name, str(device), torch.cuda.current_stream(device).cuda_stream)
    buf = _SCRATCH.get(key)
    # (no automatic trimming: the batches of ONE step differ by 10 x in size, and giving a work area back after a small batch makes the
    #  next large one pay a multi-GB hipMalloc -- measured: +37 ms per headline step; scratch_clear() is the explicit release)
    if buf is None or buf.numel() < nbytes:
        _SCRATCH[key] = None
        del buf
        buf = torch.empty(nbytes + nbytes // 4 + 4096, dtype=torch.uint8, device=device)
        _SCRATCH[key] = buf
    return buf[:nbytes]


def scratch_clear():
    """release every grow-only scratch buffer (they are views into the binding's own cache: a view must not outlive the call it was
    made for, and nothing else holds them).  Long-running hosts call this after an unusually large batch."""
    _SCRATCH.clear()


def work_area(nbytes: int, device, name: str = None):
    """the `tmp` / `scratch` of one entry-point call: `nbytes` (what the entry point's ia_*_bytes query returned -- the library measures
    a work area with the code that carves it, nothing is added here) as a uint8 tensor; a fresh one, or with `name` the grow-only
    buffer of that name (scratch() above: which call sites take it was measured)."""
    if name is not None:
        return scratch(name, nbytes, device)
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def scan_tmp(n: int, device):
    return work_area(int(lib().ia_scan_tmp_bytes(max(int(n), 1))) + 64, device)      # (+ 64: slack every scan caller has always had)


def zeros(shape, device, dtype=torch.float32):
    """zero-filled tensor through a fill KERNEL (torch.full) instead of torch.zeros' hipMemsetAsync: on the launch-rate-bound 4096-ray step
    the device idles ~30 us in front of every memset against ~5 us in front of a kernel (profiles/r06_launch_audit_after_stepops.json:
    455 us of idle in front of 15 memsets)."""
    return torch.full(shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,), 0, dtype=dtype, device=device)


def zeros_like(t):
    return zeros(tuple(t.shape), t.device, t.dtype)
