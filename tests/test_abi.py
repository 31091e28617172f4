"""CPU: the C-ABI shared library loads without a GPU, exports every symbol include/vivim_hip.h declares,
agrees with the ctypes struct layouts, and rejects bad params before any launch."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from vivim_amd import _lib


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "vivim_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vivim_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported():
    L = _lib.lib()
    names = _declared_functions()
    assert set(_lib.EXPORTS) == set(names)
    for n in names:
        assert hasattr(L, n), n


def test_struct_layouts_match():
    L = _lib.lib()
    assert len(_lib.STRUCTS) == 15
    for which, st in enumerate(_lib.STRUCTS):
        assert L.vivim_sizeof(which) == ctypes.sizeof(st), st.__name__
    assert len(_lib.STRUCTS) == 1 + max(which for which in range(256) if L.vivim_sizeof(which))
    assert L.vivim_sizeof(99) == 0 and L.vivim_sizeof(-1) == 0
    assert L.vivim_abi_version() == 8
    assert L.vivim_scan_chunk_len(_lib.F32) > 0 and L.vivim_scan_chunk_len(_lib.BF16) % 64 == 0


def test_checkpoint_length_is_a_function_of_shape_and_tuning():
    """vivim_scan_ckpt_len: short rows (16 tokens per dstate-16 row) for the shapes the lanes=states backward is chosen for,
    the long rows otherwise; forward tuning 1-3 (families that write long rows) and 5 / 6 (short rows) override the choice."""
    L = _lib.lib()
    s = _lib.SsmFwdParams()
    s.batch, s.dim, s.n_groups, s.dstate, s.seqlen, s.itype = 2, 64, 1, 16, 1280, _lib.BF16
    s.is_variable_B = s.is_variable_C = 1
    s.u_d_stride = s.delta_d_stride = s.B_dstate_stride = s.C_dstate_stride = 1280
    long_rows = L.vivim_scan_chunk_len(_lib.BF16)
    prev = L.vivim_set_tuning(0, 0)
    try:
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 16
        s.seqlen = 20480                                  # 16-bit rows up to 32768 tokens: still the lanes=states backward (round 3)
        s.u_d_stride = s.delta_d_stride = s.B_dstate_stride = s.C_dstate_stride = 20480
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 16
        s.itype = _lib.F32                                # fp32 rows longer than 8192: the lanes=tokens backward, long checkpoint rows
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == L.vivim_scan_chunk_len(_lib.F32)
        s.itype = _lib.BF16
        s.seqlen = 40960
        s.u_d_stride = s.delta_d_stride = s.B_dstate_stride = s.C_dstate_stride = 40960
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
        L.vivim_set_tuning(0, 6)
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 16
        s.dstate = 64
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == 64
        s.dstate = 24                                     # not a whole number of 16-lane rows
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
        s.dstate = 16
        L.vivim_set_tuning(0, 1)
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
        s.is_variable_B = s.is_variable_C = 0
        L.vivim_set_tuning(0, 0)
        assert L.vivim_scan_ckpt_len(ctypes.byref(s)) == long_rows
    finally:
        L.vivim_set_tuning(0, prev)


def test_scan_plan_queries_pinned():
    """vivim_scan_ckpt_len / vivim_scan_*_workspace_bytes for one shape per forward family and for the backward families,
    as literals.  None of them depends on an occupancy query (those differ between a build host and the GPU)."""
    L = _lib.lib()

    def query(itype, batch, dim, groups, dstate, seqlen, variable=1):
        s = _lib.SsmFwdParams()
        s.batch, s.dim, s.n_groups, s.dstate, s.seqlen, s.itype = batch, dim, groups, dstate, seqlen, itype
        s.is_variable_B = s.is_variable_C = variable
        s.u_d_stride = s.delta_d_stride = s.out_d_stride = s.B_dstate_stride = s.C_dstate_stride = seqlen
        s.u_batch_stride = s.delta_batch_stride = s.out_batch_stride = seqlen * dim
        s.B_group_stride = s.C_group_stride = seqlen * dstate
        s.B_batch_stride = s.C_batch_stride = seqlen * dstate * groups
        return (L.vivim_scan_ckpt_len(ctypes.byref(s)), L.vivim_scan_fwd_workspace_bytes(ctypes.byref(s)),
                L.vivim_scan_bwd_workspace_bytes(ctypes.byref(s)))

    prev = (L.vivim_set_tuning(0, 0), L.vivim_set_tuning(1, 0))
    try:
        # lanes = channels forward (fp32 B / C copy + segment carries), lanes = tokens backward (8 segments)
        assert query(_lib.BF16, 2, 768, 3, 16, 40960) == (256, 39813888, 1622016)
        assert query(_lib.F16, 2, 768, 3, 64, 8192) == (256, 50727936, 6340608)
        assert query(_lib.BF16, 2, 768, 3, 24, 5124)[:2] == (256, 0)                     # n-split forward: no workspace
        assert query(_lib.F32, 2, 64, 1, 16, 1280, variable=0) == (256, 0, 0)           # generic kernels
        ck, fwd_ws, _ = query(_lib.BF16, 2, 64, 1, 16, 1280)                              # lanes = states forward, 20 segments
        assert (ck, fwd_ws) == (16, 337920)
        # lanes = states backward: whole (batch, dim, segment) records of 2 * dstate + 1 floats; none when unsegmented
        unit = 2 * 768 * (2 * 16 + 1) * 4
        for seqlen in (320, 1280, 20480):
            ck, _, bwd_ws = query(_lib.BF16, 2, 768, 3, 16, seqlen)
            assert ck == 16 and bwd_ws % unit == 0 and bwd_ws // unit >= 2
        assert query(_lib.BF16, 2, 768, 3, 16, 64)[2] == 0                                 # four checkpoint blocks: one segment
    finally:
        L.vivim_set_tuning(0, prev[0])
        L.vivim_set_tuning(1, prev[1])


def test_rejects_before_launch():
    """Invalid params are refused on the host (no GPU needed): null struct, bad width, bad dtype."""
    L = _lib.lib()
    assert L.vivim_selective_scan_fwd(None, None) == 1
    assert b"check failed" in L.vivim_last_error()
    p = _lib.ConvFwdParams()
    p.batch, p.dim, p.seqlen, p.width = 1, 4, 8, 5
    p.x, p.weight, p.out = 1, 1, 1
    p.x_l_stride = p.out_l_stride = 1
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1
    assert b"width between 2 and 4" in L.vivim_last_error()
    p.width, p.itype = 4, 7
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1
    p.itype, p.x_l_stride, p.x_c_stride = 0, 4, 2
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1          # neither seqlen nor channels contiguous
    assert b"unit stride along seqlen or along channels" in L.vivim_last_error()
    p.x_c_stride = 1                                                      # channel-last x needs a channel-last out
    assert L.vivim_causal_conv1d_fwd(ctypes.byref(p), None) == 1
    s = _lib.SsmFwdParams()
    s.batch = s.dim = s.seqlen = s.n_groups = 1
    s.dstate = 300
    assert L.vivim_selective_scan_fwd(ctypes.byref(s), None) == 1


def test_call_raises_runtime_error():
    with pytest.raises(RuntimeError, match="check failed"):
        _lib.call("vivim_selective_scan_fwd", _lib.SsmFwdParams(), 0)


LAUNCHING = [name for name, e in _lib.ENTRY_POINTS.items() if e.struct is not None and e.stream]


def test_entry_point_table_is_the_header():
    """Every declared function has one entry; the launching ones are those that take a params struct and a stream."""
    assert list(_lib.EXPORTS) == list(_lib.ENTRY_POINTS) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert len(LAUNCHING) == 24 and all(_lib.ENTRY_POINTS[n].restype is ctypes.c_int for n in LAUNCHING)
    with_extras = {n: _lib.ENTRY_POINTS[n].extra for n in LAUNCHING if _lib.ENTRY_POINTS[n].extra}
    det = (ctypes.c_void_p, ctypes.c_size_t)
    assert with_extras == {"vivim_selective_scan_fwd_lean": (ctypes.c_void_p,), "vivim_selective_scan_bwd_det": det,
                           "vivim_causal_conv1d_bwd_det": det, "vivim_dwconv_wgrad_det": det}


@pytest.mark.parametrize("name", LAUNCHING)
def test_call_reaches_every_entry_point(name):
    """An all-zero struct fails the entry point's first size check: `call` passes the right number of arguments to every
    launching function, and nothing is launched."""
    e = _lib.ENTRY_POINTS[name]
    with pytest.raises(RuntimeError) as info:
        _lib.call(name, e.struct(), 0, *([0] * len(e.extra)))
    assert str(info.value)


def _both_ways(name, P, *extra):
    """The refusal text of `name` through _lib.call and through the ctypes function itself."""
    L = _lib.lib()
    assert getattr(L, name)(ctypes.byref(P), *extra, None) != 0
    direct = L.vivim_last_error().decode()
    with pytest.raises(RuntimeError) as info:
        _lib.call(name, P, 0, *extra)
    assert direct and str(info.value) == direct
    return direct


def test_call_passes_extras_in_c_order():
    """The arguments between params and stream arrive in the C signature's order: the workspace refusals of the three
    deterministic calls print the pointer and the byte count they were given, the lean forward takes last_state."""
    import test_abi_deterministic as det
    import test_abi_lean_fwd as lean
    conv, conv_need = det._conv_bwd_params()
    dw, dw_need = det._dw_wgrad_params()
    scan = det._bwd_params()
    scan_need = _lib.lib().vivim_scan_bwd_det_call_workspace_bytes(ctypes.byref(scan))
    for name, P, need in (("vivim_selective_scan_bwd_det", scan, scan_need), ("vivim_causal_conv1d_bwd_det", conv, conv_need),
                          ("vivim_dwconv_wgrad_det", dw, dw_need)):
        assert need > 4
        assert "workspace of %d bytes at (nil)" % need in _both_ways(name, P, None, need)              # null workspace
        assert "workspace of %d bytes at 0x1000" % (need - 4) in _both_ways(name, P, 4096, need - 4)   # short workspace
    for z in (True, False):
        P = lean._params(z=z)
        P.x = lean.PTR
        for last_state in (None, lean.PTR):
            assert "x must be NULL" in _both_ways(lean.LEAN, P, last_state)


def test_launch_enters_the_device_context_only_off_the_current_device(monkeypatch):
    """_lib.launch with torch.cuda stubbed out (no GPU here): on the current device it calls `call` on the current stream
    with no context manager; for another device it enters torch.cuda.device(that device) first and takes that device's
    current stream.  The extras are passed through after the stream."""
    import contextlib
    import types

    import torch
    state = {"current": 0}
    events = []

    @contextlib.contextmanager
    def device(dev):
        prev, state["current"] = state["current"], dev.index
        events.append(("enter", dev.index))
        yield
        state["current"] = prev
        events.append(("exit", dev.index))

    monkeypatch.setattr(torch.cuda, "current_device", lambda: state["current"])
    monkeypatch.setattr(torch.cuda, "device", device)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: types.SimpleNamespace(cuda_stream=1000 + state["current"]))
    monkeypatch.setattr(_lib, "call", lambda *args: events.append(("call",) + args))
    P = _lib.ConvBwdParams()
    _lib.launch("vivim_causal_conv1d_bwd", P, torch.device("cuda", 0))
    assert events == [("call", "vivim_causal_conv1d_bwd", P, 1000)]
    del events[:]
    _lib.launch("vivim_causal_conv1d_bwd_det", P, torch.device("cuda", 1), 4096, 64)
    assert events == [("enter", 1), ("call", "vivim_causal_conv1d_bwd_det", P, 1001, 4096, 64), ("exit", 1)]
    assert state["current"] == 0


def test_algorithmic_bytes_of_the_deterministic_twins():
    """A `*_det` name counts the bytes of its default twin, read from the struct's forward half."""
    import test_abi_deterministic as det
    for name, P in (("vivim_selective_scan_bwd", det._bwd_params()), ("vivim_causal_conv1d_bwd", det._conv_bwd_params()[0]),
                    ("vivim_dwconv_wgrad", det._dw_wgrad_params()[0])):
        assert _lib.algorithmic_bytes(name + "_det", P) == _lib.algorithmic_bytes(name, P) > 0
    conv = det._conv_bwd_params()[0]
    assert _lib.algorithmic_bytes("vivim_causal_conv1d_bwd_det", conv) == 3 * 2 * 64 * 4096 * 2 + 8 * 64 * 5


def test_python_surface_imports_without_gpu():
    import causal_conv1d  # noqa: F401
    import causal_conv1d_cuda
    import mamba_ssm
    import selective_scan_cuda
    from modeling.vivim import MambaLayer, Vivim, mamba_block  # noqa: F401
    assert callable(selective_scan_cuda.fwd) and callable(selective_scan_cuda.bwd)
    assert callable(causal_conv1d_cuda.causal_conv1d_fwd) and callable(causal_conv1d_cuda.causal_conv1d_bwd)
    assert hasattr(mamba_ssm, "Mamba") and hasattr(mamba_ssm, "selective_scan_fn")


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under vivim_amd/ (or the alias packages) may reference it."""
    bad = []
    for top in ("vivim_amd", "mamba_ssm", "causal_conv1d", "modeling"):
        for dp, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".cuh", ".h")):
                    src = open(os.path.join(dp, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b|ssm_oracle|ref_torch", src, flags=re.M):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_tuning_roundtrip():
    """vivim_set_tuning returns the previous value and rejects bad arguments (no GPU needed)."""
    L = _lib.lib()
    prev = L.vivim_set_tuning(0, 5)
    assert prev >= 0
    assert L.vivim_set_tuning(0, prev) == 5
    assert L.vivim_set_tuning(2, 0) == -1 and L.vivim_set_tuning(0, -3) == -1


def test_dir_maps_reject_bad_arguments_on_host():
    """vivim_dir_scatter / vivim_dir_gather validate before launching (no GPU needed for the rejections)."""
    import ctypes
    L = _lib.lib()
    P = _lib.DirParams()
    P.batch, P.channels, P.seqlen, P.nframes, P.csplit, P.itype, P.scale = 1, 4, 30, 5, 2, _lib.BF16, 1.0
    P.src = P.dst = 0
    for fn in (L.vivim_dir_scatter, L.vivim_dir_gather):
        assert fn(ctypes.byref(P), None) != 0                      # null pointers
    P.src = P.dst = 4096
    assert L.vivim_dir_scatter(ctypes.byref(P), None) != 0        # 30 bf16 tokens are not whole 16-byte vectors
    P.seqlen, P.nframes = 32, 5
    assert L.vivim_dir_scatter(ctypes.byref(P), None) != 0        # seqlen not a multiple of nframes
    assert b"" != L.vivim_last_error()


def test_graft_entry_build_is_consistent():
    """__graft_entry__.build() (what the driver runs every round) must accept the library it has just built: its ABI
    assertion is derived from the header, not hard-coded."""
    import __graft_entry__ as g
    g.build()


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_no_experiment_scaffolding_in_kernel_sources():
    """Timing-ablation switches (FOO_ABL) and in-kernel stamp hooks (VIVIM_STAMP*) are retired: the product build is the
    only build of the kernel sources."""
    bad = []
    for top in (os.path.join("vivim_amd", "csrc"), "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".hip", ".cuh", ".h", ".hpp", ".cpp")) or f == "Makefile":
                    src = open(os.path.join(dp, f)).read()
                    bad += ["%s: %s" % (f, m) for m in re.findall(r"\b[A-Z0-9]+_ABL\b|VIVIM_STAMP", src)]
    assert not bad, bad


def test_env_switches_match_integration_table():
    """The VIVIM_* variables the library, its Python wrappers and bench.py read are exactly the rows of INTEGRATION.md §4."""
    read = set()
    csrc = os.path.join(ROOT, "vivim_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".cuh", ".h")):
            src = _read("vivim_amd", "csrc", f)
            read |= set(re.findall(r'\b(?:getenv|num)\(\s*"(VIVIM_\w+)"', src))
            read |= set(re.findall(r'\btuning_get\([^,()]*,\s*"(VIVIM_\w+)"', src))
    py = [os.path.join("vivim_amd", f) for f in sorted(os.listdir(os.path.join(ROOT, "vivim_amd"))) if f.endswith(".py")]
    for f in py + ["bench.py"]:
        src = _read(f)
        for m in re.findall(r'os\.(?:environ\.get|getenv)\(\s*["\'](VIVIM_\w+)|os\.environ\[\s*["\'](VIVIM_\w+)|'
                            r'["\'](VIVIM_\w+)["\']\s+(?:not\s+)?in\s+os\.environ', src):
            read |= {n for n in m if n}
    doc = _read("INTEGRATION.md")
    section = re.search(r"^## 4\..*?$(.*?)^## ", doc, flags=re.S | re.M).group(1)
    documented = set()
    for line in section.splitlines():
        if line.startswith("| `"):
            documented |= set(re.findall(r"`(VIVIM_\w+)", line.split("|")[1]))
    assert read, "no environment reads found: the patterns above no longer match the code"
    assert read == documented, {"read but not in INTEGRATION.md §4": sorted(read - documented),
                                "in INTEGRATION.md §4 but not read": sorted(documented - read)}
