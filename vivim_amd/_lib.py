"""ctypes binding of libvivim_hip.so (C ABI: include/vivim_hip.h, frozen at ABI version 8, and the extension headers next to it).

Each header is the one description of what it declares: parsed once, at import, into params structs, entry points and constants,
by a parser that refuses whatever it does not understand instead of guessing.  A feature added after version 8 gets
include/vivim_hip_ext_<feature>.h, a row in EXTENSIONS and a struct that opens with `struct_bytes`; `lib()` binds all tables in one
loop.  The library is the product: if it is missing or fails to load this module raises -- no PyTorch/CPU fallback in vivim_amd.
"""
import collections
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("VIVIM_LIB") or os.path.join(CSRC, "libvivim_hip.so")   # VIVIM_LIB: A/B builds
HEADER = os.path.join(os.path.dirname(_HERE), "include", "vivim_hip.h")

i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

# The one table kept by hand: C struct -> Python class.  Everything else about the ABI -- fields, entry points, constants --
# is read from the header.  The order is vivim_sizeof's (not the header's: wgrad_nt comes before add_layernorm); the structs
# that open with `struct_bytes` have no vivim_sizeof row and come last.
STRUCT_NAMES = {
    "vivim_ssm_fwd_params": "SsmFwdParams", "vivim_ssm_bwd_params": "SsmBwdParams",
    "vivim_conv_fwd_params": "ConvFwdParams", "vivim_conv_bwd_params": "ConvBwdParams",
    "vivim_dwconv_params": "DwConvParams", "vivim_dwconv_wgrad_params": "DwConvWgradParams",
    "vivim_dir_params": "DirParams", "vivim_conv_update_params": "ConvUpdateParams",
    "vivim_state_update_params": "StateUpdateParams", "vivim_layernorm_params": "LayerNormParams",
    "vivim_wgrad_nt_params": "WgradNtParams", "vivim_add_layernorm_params": "AddLayerNormParams",
    "vivim_seg_loss_params": "SegLossParams", "vivim_seg_metrics_params": "SegMetricsParams",
    "vivim_upsample_params": "UpsampleParams",
    "vivim_decode_head_params": "DecodeHeadParams", "vivim_token_layernorm_params": "TokenLayerNormParams",
    "vivim_token_add_norm_params": "TokenAddNormParams", "vivim_opt_step_params": "OptStepParams",
    "vivim_opt_mw_params": "OptMwParams",
}
# The same table per extension header, by file name under include/ in the order added: (C struct -> Python class, entry points).
EXTENSIONS = {"vivim_hip_ext.h": ({"vivim_structure_loss_params": "StructureLossParams"}, {}),
              "vivim_hip_ext_head.h": ({"vivim_head_concat_params": "HeadConcatParams"}, {}),
              "vivim_hip_ext_binary_metrics.h": ({"vivim_binary_metrics_params": "BinaryMetricsParams"}, {})}

# One entry per exported function: its params struct (or None), the ctypes types of the arguments between `params` and
# `stream` in the C signature, whether a stream comes last, and the restype.
Entry = collections.namedtuple("Entry", "struct extra stream restype")

_FIELD_TYPES = {"int32_t": i32, "int64_t": i64, "float": ctypes.c_float, "double": ctypes.c_double,
                "void *": vp, "const void *": vp, "const void *const *": ctypes.POINTER(vp),
                "const int64_t *": ctypes.POINTER(i64)}
_ARG_TYPES = {"void *": vp, "size_t": ctypes.c_size_t, "int": ctypes.c_int}
_RESTYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
_DIRECTIVES = r"\s*#\s*(include|define|ifndef\s+VIVIM_HIP(_[A-Z0-9]+)*_H|endif)\b"        # what may stand outside a struct


def _refuse(header, what, text):
    raise ValueError(f"{header}: {what}: {' '.join(text.split())!r}")


def _ctype(text):
    """Canonical spelling of a C type: 'const  void * const*' -> 'const void *const *'."""
    return re.sub(r"\s*\*\s*", " *", " ".join(text.split()))


def _declarator(text, table, context, header):
    """'const void *u' -> ('u', c_void_p), 'int32_t map_h[4]' -> ('map_h', c_int32 * 4), the type looked up in `table`."""
    m = re.fullmatch(r"([\w\s*]*?)(\w+)\s*(?:\[\s*(\d+)\s*\])?", text.strip())
    if not m:                                                           # a bit-field, a function pointer, ...
        _refuse(header, "cannot parse the declarator", context)
    if _ctype(m[1]) not in table:
        _refuse(header, f"unknown type {_ctype(m[1])!r}", context)
    ctype = table[_ctype(m[1])]
    return m[2], (ctype * int(m[3]) if m[3] else ctype)


def _has_sizeof_row(cls):
    return cls._fields_[0][0] != "struct_bytes"       # such a struct states its own sizeof and the entry point checks it


def parse_header(text, names=STRUCT_NAMES, header="vivim_hip.h"):
    """-> (constants, classes, entry points) of a header written like include/vivim_hip.h: the `#define VIVIM_* <int>` and
    enumerator values by name; one ctypes.Structure per `typedef struct { ... } vivim_*;`, by Python name in the order of
    `names`; one Entry per function declaration, in header order.  ValueError naming `header` on anything else: it never guesses."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(VIVIM_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    by_c_name = {}

    def struct(m):
        body, c_name = m[1], m[2]
        if "{" in body or "#" in body:
            _refuse(header, "nested braces or a preprocessor line in a struct", m[0])
        if c_name not in names:
            _refuse(header, "a struct without a Python name in STRUCT_NAMES", c_name)
        types = {**_FIELD_TYPES, **by_c_name}                           # an earlier struct may be a field, by value
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            base = re.match(r"(?:const\s+)?\w+", stmt) or _refuse(header, "cannot parse the field", stmt)
            first, *more = stmt.split(",")                              # `const void *u, *delta`: the stars belong to the names
            for decl in [first] + [f"{base[0]} {d}" for d in more]:
                fields.append(_declarator(decl, types, stmt, header))
        by_c_name[c_name] = type(names[c_name], (ctypes.Structure,), {"_fields_": fields, "__module__": __name__})
        return " "

    def enum(m):
        for item in filter(None, (s.strip() for s in m[1].split(","))):
            kv = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item) or _refuse(header, "cannot parse the enumerator", item)
            consts[kv[1]] = int(kv[2])
        return " "

    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    text = re.sub(r"(?:typedef\s+)?enum\s*\{([^{}]*)\}\s*\w*\s*;", enum, text)
    missing = [c for c in names if c not in by_c_name]
    if missing:
        _refuse(header, "STRUCT_NAMES names structs the header does not have", ", ".join(missing))
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b", " ", text, flags=re.S | re.M)   # extern "C"
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        if not re.match(_DIRECTIVES, line):
            _refuse(header, "a preprocessor line it does not know", line)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    entries = {}
    for decl in filter(None, (s.strip() for s in text.split(";"))):     # what is left: function declarations
        m = re.fullmatch(r"([\w\s*]+?)(\w+)\s*\(([\w\s*,]*)\)", decl) or _refuse(header, "cannot parse the declaration", decl)
        if _ctype(m[1]) not in _RESTYPES:
            _refuse(header, f"unknown return type {_ctype(m[1])!r}", decl)
        args = [] if m[3].strip() == "void" else [a.strip() for a in m[3].split(",")]
        stream = bool(args) and re.fullmatch(r"void\s*\*\s*stream", args[-1]) is not None
        args = args[:-1] if stream else args
        params, extra = None, []
        for k, arg in enumerate(args):
            p = re.fullmatch(r"const\s+(vivim_\w+)\s*\*\s*\w+", arg) if k == 0 else None
            if not p:
                extra.append(_declarator(arg, _ARG_TYPES, decl, header)[1])
            elif p[1] not in by_c_name:
                _refuse(header, f"unknown struct {p[1]}", decl)
            elif _has_sizeof_row(by_c_name[p[1]]):
                params = by_c_name[p[1]]
            else:
                extra.append(ctypes.POINTER(by_c_name[p[1]]))
        entries[m[2]] = Entry(params, tuple(extra), stream, _RESTYPES[_ctype(m[1])])
    return consts, {names[c]: by_c_name[c] for c in names}, entries


def _read_header(path=None):
    path = path or HEADER
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise ImportError(f"{path} cannot be read ({e}): the binding is derived from it") from e


def load_extensions(extensions, include_dir, taken_entries, taken_classes):
    """Parse every header of `extensions` (a table like EXTENSIONS) under `include_dir`, fill in each row's entry points, return
    (classes, entry points) of all rows.  ImportError naming the file: a struct that does not open with `struct_bytes`, a name taken."""
    classes, entries = {}, {}
    for file, (names, own) in extensions.items():
        _, new, parsed = parse_header(_read_header(os.path.join(include_dir, file)), names, file)
        bad = [f"{n} does not open with struct_bytes" for n, c in new.items() if _has_sizeof_row(c)]
        bad += [f"another header already declares {n}" for n in parsed if n in taken_entries or n in entries]
        bad += [f"the name {n} is already taken" for n in new if n in taken_classes or n in classes]
        if bad:
            raise ImportError(f"{file}: {'; '.join(bad)}")
        own.update(parsed)
        entries.update(parsed)
        classes.update(new)
    return classes, entries


_consts, _classes, ENTRY_POINTS = parse_header(_read_header())
globals().update(_classes)                              # SsmFwdParams ... OptMwParams, the classes STRUCT_NAMES names
STRUCTS = tuple(c for c in _classes.values() if _has_sizeof_row(c))    # in vivim_sizeof order
EXPORTS = tuple(ENTRY_POINTS)
ABI_VERSION = _consts["VIVIM_ABI_VERSION"]
F32, F16, BF16 = _consts["VIVIM_F32"], _consts["VIVIM_F16"], _consts["VIVIM_BF16"]
OPT_CHUNK, OPT_MAX_TENSORS, OPT_STATE_WORDS = (_consts["VIVIM_OPT_" + n] for n in ("CHUNK", "MAX_TENSORS", "STATE_WORDS"))
_classes, _entries = load_extensions(EXTENSIONS, os.path.dirname(HEADER), ENTRY_POINTS, globals())
globals().update(_classes)                              # StructureLossParams, HeadConcatParams, BinaryMetricsParams
ALL_ENTRY_POINTS = {**ENTRY_POINTS, **_entries}         # every table: what lib() binds and `call` takes

_lib = None


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-j4"])
    return SO_PATH


def lib():
    """The loaded library; raises if it is not built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(
                f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C vivim_amd/csrc`). vivim_amd has no fallback path.")
        # torch is imported above, before the library: its bundled HIP runtime must be the one this process initialises --
        # loading the library (and with it /opt/rocm's libamdhip64) before `import torch` leaves two runtimes in the process
        # and every launch of ours then fails with "no ROCm-capable device is detected" (seen with build() followed by
        # smoke() in one process)
        L = ctypes.CDLL(SO_PATH)
        for name, e in ALL_ENTRY_POINTS.items():
            fn = getattr(L, name)
            fn.argtypes = ([ctypes.POINTER(e.struct)] if e.struct else []) + list(e.extra) + ([vp] if e.stream else [])
            fn.restype = e.restype
        if L.vivim_abi_version() != ABI_VERSION:
            raise ImportError("libvivim_hip.so ABI version mismatch")
        for which, st in enumerate(STRUCTS):
            if L.vivim_sizeof(which) != ctypes.sizeof(st):
                raise ImportError(f"struct layout mismatch for {st.__name__}: "
                                  f"C {L.vivim_sizeof(which)} vs ctypes {ctypes.sizeof(st)}")
        _lib = L
    return _lib


_ISIZE = {F32: 4, F16: 2, BF16: 2}


def algorithmic_bytes(name, P):
    """Compulsory HBM traffic of one launch: every tensor of the op read or written once
    (the checkpoint tensor x is an implementation choice and is excluded).  A `*_det` entry point
    moves the bytes of its default twin."""
    name = name.removesuffix("_det")
    f = P.f if isinstance(P, (SsmBwdParams, ConvBwdParams)) else P       # the forward half of a backward struct
    if name.startswith("vivim_opt"):                                    # g once | the slots | p, m, v read and written, g read
        if name.endswith("finalise"):
            return 8 * P.total_blocks + 4 * OPT_STATE_WORDS
        n = sum(P.numel[i] for i in range(P.count) if P.grads[i])
        if name.endswith("_mw"):                                        # a 2-byte g | master, m, v read and written, g read, p16 written
            return 2 * n + 8 * P.n_blocks if name.endswith("stats_mw") else 28 * n
        return 4 * n + 8 * P.n_blocks if name.endswith("stats") else 28 * n
    if name.startswith("vivim_add_layernorm"):
        n = P.batch * P.seqlen * P.channels
        if not P.weight:                                               # add-only: x, branch, x_new / dres, dbranch
            return n * ((2 if name.endswith("fwd") else 1) * _ISIZE[P.itype] + _ISIZE[P.btype])
        if name.endswith("fwd"):                                       # x, branch, x_new, y + mean, rstd
            return n * (2 * _ISIZE[P.itype] + _ISIZE[P.btype] + _ISIZE[P.otype]) + 8 * P.batch * P.seqlen + 8 * P.channels
        res = (_ISIZE[P.itype] if P.dres else 0) + (_ISIZE[P.otype] if P.dy else 0) + (_ISIZE[P.btype] if P.dbranch else 0)
        return n * (2 * _ISIZE[P.itype] + res) + 8 * P.batch * P.seqlen + 12 * P.channels   # x_new, dx + what is present
    if name.startswith("vivim_token_add_norm"):                         # every tensor that is given, once
        n, b, r = P.rows * P.channels, _ISIZE[P.btype], _ISIZE[P.rtype]
        stats = 8 * P.rows if P.mean and P.weight else 0
        small = (4 * (P.rows // P.rows_per_sample) if P.scale else 0) + (4 * P.channels if P.weight else 0)
        if name.endswith("fwd"):
            small += 4 * P.channels if P.weight and P.bias else 0
            return n * (b + (r if P.res else 0) + (r if P.res_out else 0) + (b if P.weight else 0)) + stats + small
        norm = bool(P.weight and P.dy)                                  # else the saved row and the statistics are not read
        small += (4 * P.channels if norm and P.dweight else 0) + (4 * P.channels if norm and P.dbias else 0)
        return (n * ((r + b if norm else 0) + (r if P.dres else 0) + (r if P.dres_in else 0) + (b if P.dbranch else 0))
                + (stats if norm else 0) + small)
    if name.startswith("vivim_token_layernorm"):                        # x, y + mean, rstd | x, dy, dx + mean, rstd, weight + dweight, dbias
        n = P.rows * P.channels
        stats = 8 * P.rows if P.mean else 0
        if name.endswith("fwd"):
            return n * (_ISIZE[P.itype] + _ISIZE[P.otype]) + stats
        return n * (2 * _ISIZE[P.itype] + _ISIZE[P.otype]) + stats + 12 * P.channels
    if name.startswith("vivim_decode_head"):                            # the maps once, the logits once, bias + w_out + b_out
        px = sum(P.map_h[s] * P.map_w[s] for s in range(P.n_maps))
        return (P.batch * (px * P.hidden + P.classes * P.out_h * P.out_w) * _ISIZE[P.itype]
                + 4 * (P.hidden + P.classes * P.hidden + P.classes))
    if name.startswith("vivim_head_concat"):                            # the maps, the masks, the concat: once each, either direction
        px = P.out_h * P.out_w
        maps = sum(P.map_c[s] * (P.map_h[s] * P.map_w[s] + px) for s in range(P.n_maps)) * _ISIZE[P.itype]
        return P.batch * (maps + sum(P.map_c[s] * px for s in range(P.n_maps) if P.keep[s]))
    if name.startswith("vivim_upsample"):                               # the small and the large tensor once, either direction
        return P.batch * P.channels * (P.in_h * P.in_w + P.out_h * P.out_w) * _ISIZE[P.itype]
    if name.startswith("vivim_seg_metrics"):                            # logits, labels, the prediction map if wanted, the counts
        n = P.batch * P.pixels
        return n * (P.classes * _ISIZE[P.itype] + (8 if P.ttype == 0 else 1) + (1 if P.pred else 0)) + 12 * P.batch * P.classes
    if name.startswith("vivim_structure_loss"):                         # logits (+ dlogits), labels, the per-image factors
        n = P.batch * P.height * P.width
        return (n * ((2 if name.endswith("bwd") else 1) * P.classes * _ISIZE[P.itype] + (8 if P.ttype == 0 else 1))
                + 12 * P.batch * P.classes)
    if name.startswith("vivim_seg_loss"):                               # logits (+ dlogits), labels, the per-image factors
        n = P.batch * P.pixels
        return (n * ((2 if name.endswith("bwd") else 1) * P.classes * _ISIZE[P.itype] + (8 if P.ttype == 0 else 1))
                + 8 * P.batch * P.classes)
    if name.startswith("vivim_binary_metrics"):                         # pred and gt read by three launches | values, histograms, state
        n = P.batch * P.height * P.width
        return (3 * n * (_ISIZE[P.ptype] + _ISIZE.get(P.gtype, 1)) + P.batch * (72 + (4096 if P.hist else 0))
                + (160 if P.state else 0))
    if name.startswith("vivim_selective_scan"):
        s = _ISIZE[f.itype]
        act = f.batch * f.dim * f.seqlen * s
        bc = (f.batch * f.n_groups * f.dstate * f.seqlen) if f.is_variable_B else f.dim * f.dstate
        has_z = bool(f.z)
        if name.endswith("fwd_lean"):                             # u, delta, out | u, delta, z, out_z
            return (4 if has_z else 3) * act + 2 * bc * (s if f.is_variable_B else 4) + 4 * (f.dim * f.dstate + 2 * f.dim)
        if name.endswith("fwd"):
            n_act = 3 + (2 if has_z else 0)                       # u, delta, out (+ z, out_z)
            return n_act * act + 2 * bc * (s if f.is_variable_B else 4) + 4 * (f.dim * f.dstate + 2 * f.dim)
        n_act = 5 + (3 if has_z else 0) + (1 if (has_z and f.out_z) else 0)   # u, delta, dout, du, ddelta (+ z, out, dz) (+ out_z)
        return (n_act * act + 2 * bc * (s if f.is_variable_B else 4) + 2 * bc * 4
                + 4 * (2 * f.dim * f.dstate + 4 * f.dim))
    if name.endswith("_update"):
        return 0                                                       # latency-bound single-token steps: not profiled
    if name.startswith("vivim_dir"):
        return 4 * P.batch * P.channels * P.seqlen * _ISIZE[P.itype]  # one flat tensor + three stacked copies
    if name.startswith("vivim_dwconv"):
        act = P.batch * P.depth * P.height * P.width * P.channels * _ISIZE[P.itype]
        return 2 * act + 4 * P.channels * (P.kd * 9 + 1)            # x and y (or x and dy) once + taps
    if name.startswith("vivim_layernorm"):                              # x, y + mean, rstd | x, dy, dx + mean, rstd
        n = P.batch * P.seqlen * P.channels
        if name.endswith("fwd"):
            return n * (_ISIZE[P.itype] + _ISIZE[P.otype]) + 8 * P.batch * P.seqlen + 8 * P.channels
        return n * (2 * _ISIZE[P.itype] + _ISIZE[P.otype]) + 8 * P.batch * P.seqlen + 12 * P.channels
    if name.startswith("vivim_wgrad"):                                  # both operands, the fp32 products
        return P.groups * ((P.m + P.n) * P.k * _ISIZE[P.itype] + 4 * P.m * P.n)
    s = _ISIZE[f.itype]
    act = f.batch * f.dim * f.seqlen * s
    if name.endswith("fwd"):
        return 2 * act + 4 * f.dim * (f.width + 1)
    return 3 * act + 8 * f.dim * (f.width + 1)


_profile = None
_event_pool = []
_PROFILED = ("vivim_selective_scan_fwd", "vivim_selective_scan_bwd", "vivim_causal_conv1d_fwd",
             "vivim_causal_conv1d_bwd")


def profile_begin(all_kernels=False):
    """Start recording one (name, algorithmic bytes, start event, end event) tuple per C-ABI call of the hot-path
    kernels (with all_kernels=True of every launching entry point, under its own name); events are recorded on the stream the kernel is launched on
    (torch's current stream) and come from a reusable pool, so the timed region pays two hipEventRecord per call."""
    global _profile
    _profile = ([], bool(all_kernels))


def profile_end():
    """Stop recording; -> list of (name, bytes, seconds) after synchronising the recorded events."""
    global _profile
    rec = _profile[0] if _profile else []
    _profile = None
    out = []
    for name, nbytes, e0, e1 in rec:
        e1.synchronize()
        out.append((name, nbytes, e0.elapsed_time(e1) * 1e-3))
        _event_pool.extend((e0, e1))
    return out


def _event():
    if _event_pool:
        return _event_pool.pop()
    return torch.cuda.Event(enable_timing=True)


# ---- VIVIM_GUARD=1: debug mode that brackets every buffer the wrappers allocate for a kernel to write with canary
# bytes and verifies them (device sync) after each launch -- finds out-of-bounds writes without waiting for a fault.
GUARD = os.environ.get("VIVIM_GUARD", "0") not in ("0", "")
_GUARD_BYTES = 1 << 16
_guards = []


def _guarded_storage(nbytes, device):
    buf = torch.full((nbytes + 2 * _GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=device)
    _guards.append(buf)
    return buf[_GUARD_BYTES:_GUARD_BYTES + nbytes]


def empty(shape, dtype, device):
    """torch.empty, or its canary-bracketed twin under VIVIM_GUARD=1."""
    if not GUARD:
        return torch.empty(shape, dtype=dtype, device=device)
    n = 1
    for d in shape:
        n *= d
    return _guarded_storage(n * torch.empty((), dtype=dtype).element_size(), device).view(dtype).view(shape)


def zeros(n, device):
    """A zeroed fp32 accumulator of n elements (dA / dB / dC / dD / dbias, dweight / dbias of the convolutions: what the
    kernels ADD into), or its canary-bracketed twin under VIVIM_GUARD=1."""
    if not GUARD:
        return torch.zeros(n, dtype=torch.float32, device=device)
    return _guarded_storage(4 * n, device).view(torch.float32).zero_()


def empty_like(t):
    """torch.empty_like (dense, same strides), or its canary-bracketed twin under VIVIM_GUARD=1."""
    if not GUARD:
        return torch.empty_like(t)
    ref = torch.empty_like(t)                               # for its strides
    flat = _guarded_storage(t.numel() * t.element_size(), t.device).view(t.dtype)
    return flat.as_strided(ref.shape, ref.stride())


def check_guards(what):
    torch.cuda.synchronize()
    for buf in _guards:
        lo, hi = buf[:_GUARD_BYTES], buf[-_GUARD_BYTES:]
        if not (bool((lo == 0xA5).all()) and bool((hi == 0xA5).all())):
            nlo, nhi = int((lo != 0xA5).sum()), int((hi != 0xA5).sum())
            _guards.clear()
            raise RuntimeError(f"VIVIM_GUARD: {what} wrote outside a {buf.numel() - 2 * _GUARD_BYTES}-byte buffer "
                               f"({nlo} bytes below, {nhi} bytes above)")
    _guards.clear()


def deterministic():
    """True while torch.use_deterministic_algorithms is on (warn_only included): the backward entry points then take
    their deterministic variants."""
    return torch.are_deterministic_algorithms_enabled()


def call(name, params, stream, *extra):
    """Enqueue one entry point on `stream` (int hipStream_t): fn(&params, *extra, stream), `extra` being what the C
    signature has between the two (ENTRY_POINTS).  RuntimeError on a nonzero return, like the TORCH_CHECKs of the
    reference bindings."""
    L = lib()
    fn = getattr(L, name)
    if _profile is not None and (_profile[1] or name in _PROFILED):
        e0, e1 = _event(), _event()
        e0.record()
        rc = fn(ctypes.byref(params), *extra, stream)
        e1.record()
        _profile[0].append((name, algorithmic_bytes(name, params), e0, e1))
    else:
        rc = fn(ctypes.byref(params), *extra, stream)
    if rc != 0:
        raise RuntimeError(L.vivim_last_error().decode())
    if GUARD:
        check_guards(name)


def launch(name, params, device, *extra):
    """`call` on torch's current stream of `device`.  The step is host-paced: the device context manager (~15 us) is
    entered only when `device` is not already the current one."""
    if device.index == torch.cuda.current_device():
        call(name, params, torch.cuda.current_stream().cuda_stream, *extra)
    else:
        with torch.cuda.device(device):
            call(name, params, torch.cuda.current_stream().cuda_stream, *extra)


# ---- what every wrapper module needs around a launch
ITYPE = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}


def ptr(t):
    return None if t is None else t.data_ptr()


def check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def workspace(query, params, device):
    """-> (bytes the query `query` asks for `params`, a uint8 buffer of that size on `device` or None for 0 bytes)."""
    n = getattr(lib(), query)(params)
    return n, (empty((n,), torch.uint8, device) if n else None)
